"""CPU: the fused smoothed cross-entropy and the evaluation accumulators -- header <-> bindings <-> exports of the new
entry points, their argument checks (decided on the host before any launch), the accumulator's size, the confusion CSV of
evaluate.write_confusion_csv against the text gen_cm_w writes (reference hwgat/utils.py:338-350) and the refusals of
evaluate.Evaluator that need no device."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
evaluate = importlib.import_module("sl-hwgat_amd.evaluate")
train = importlib.import_module("sl-hwgat_amd.train")
NEW_SYMBOLS = {"hwgat_sce_fwd", "hwgat_sce_bwd", "hwgat_eval_acc_bytes", "hwgat_eval_accumulate"}


def test_new_entry_points_declared_bound_and_exported():
    assert NEW_SYMBOLS <= set(hw._lib.declared_symbols())
    assert NEW_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith(("hwgat_sce_", "hwgat_eval_"))}
    handle = hw._lib.lib()
    for n in NEW_SYMBOLS:
        assert getattr(handle, n) is not None
    assert handle.hwgat_abi_version() == hw._lib.header_abi_version() == 4007
    assert hw.evaluate is evaluate and "evaluate" in hw.__all__


def test_arguments_are_refused_before_any_launch():
    """NULL pointers: HWGAT_EINVAL (-1); B < 1 or C outside 1..65536 with non-null pointers: HWGAT_ESHAPE (-2).  The
    pointers are never read."""
    L = hw._lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.hwgat_sce_fwd(*([None] * 8), 4, 10, 0.01, None) == -1
    assert L.hwgat_sce_bwd(*([None] * 6), 4, 10, 0.01, None) == -1
    assert L.hwgat_eval_accumulate(*([None] * 7), 4, 10, 5, 0, None) == -1
    for hole in (0, 1, 3, 4, 5, 6, 7):                       # every required pointer on its own; n_valid (2) may be NULL
        args = [p] * 8
        args[hole] = None
        assert L.hwgat_sce_fwd(*args, 4, 10, 0.01, None) == -1, hole
    for hole in (0, 1, 3, 4, 5):
        args = [p] * 6
        args[hole] = None
        assert L.hwgat_sce_bwd(*args, 4, 10, 0.01, None) == -1, hole
    for hole in range(6):
        args = [p] * 7
        args[hole] = None
        assert L.hwgat_eval_accumulate(*args, 4, 10, 5, 0, None) == -1, hole
    assert L.hwgat_eval_accumulate(*([p] * 7), 4, 10, -1, 0, None) == -1            # k_max < 0
    assert L.hwgat_eval_accumulate(*([p] * 7), 4, 10, 5, -1, None) == -1            # log capacity < 0
    for C in (0, 65537):
        assert L.hwgat_sce_fwd(*([p] * 8), 4, C, 0.01, None) == -2
        assert L.hwgat_sce_bwd(*([p] * 6), 4, C, 0.01, None) == -2
        assert L.hwgat_eval_accumulate(*([p] * 7), 4, C, 5, 0, None) == -2
        assert L.hwgat_eval_acc_bytes(C, 5, 0) == -1
    for B in (0, -3, 1 << 31):
        assert L.hwgat_sce_fwd(*([p] * 8), B, 10, 0.01, None) == -2
        assert L.hwgat_sce_bwd(*([p] * 6), B, 10, 0.01, None) == -2
        assert L.hwgat_eval_accumulate(*([p] * 7), B, 10, 5, 0, None) == -2


def test_accumulator_size_follows_the_documented_layout():
    L = hw._lib.lib()
    HF = hw.functional
    # 3 int64 counters + 2 doubles, k_max + 1 histogram words, C x C confusion words, two int32 logs of `cap` entries
    assert L.hwgat_eval_acc_bytes(3, 5, 0) == 8 * (5 + 6 + 9)
    assert L.hwgat_eval_acc_bytes(3, 5, 8) == 8 * (5 + 6 + 9) + 2 * 4 * 8
    assert L.hwgat_eval_acc_bytes(65536, 0, 0) == 8 * (5 + 1 + 65536 * 65536)
    assert L.hwgat_eval_acc_bytes(3, -1, 0) == -1 and L.hwgat_eval_acc_bytes(3, 5, -1) == -1
    assert HF.eval_acc_words(2002, 5, 100) == 5 + 6 + 2002 * 2002 + 100 and HF.EVAL_ACC_HEADER_WORDS == 5
    with pytest.raises(ValueError, match="no accumulator"):
        HF.eval_acc_words(0, 5, 0)


def test_confusion_csv_is_the_reference_file(tmp_path):
    cm = np.array([[2, 1, 0],
                   [0, 0, 0],
                   [1, 0, 3]], dtype=np.int64)
    path = tmp_path / "cm.csv"
    evaluate.write_confusion_csv(path, ["hello", "thank you", "yes, please"], cm)
    with open(path, newline="") as fh:
        text = fh.read()
    # csv.writer's defaults, as the reference uses them: \r\n line ends, a field is quoted only when it holds a comma
    assert text == ("word,total,predicted\r\n"
                    "Word-hello,3.0,word-hello(2.0) word-thank you(1.0) \r\n"
                    "Word-thank you,0.0,\r\n"
                    "\"Word-yes, please\",4.0,\"word-hello(1.0) word-yes, please(3.0) \"\r\n")
    evaluate.write_confusion_csv(path, ["a", "b", "c"], torch.from_numpy(cm))       # a CPU tensor is as good
    with open(path, newline="") as fh:
        assert fh.read().splitlines()[3] == "Word-c,4.0,word-a(1.0) word-c(3.0) "
    with pytest.raises(ValueError, match="one name per class"):
        evaluate.write_confusion_csv(path, ["a", "b"], cm)


def test_evaluator_and_launchers_refuse_the_cpu():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, None, num_kps=32)
    model = hw.Model(*hp.get_model_params()).eval()
    with pytest.raises(ValueError, match="must live on the GPU"):
        evaluate.Evaluator(model, 5, torch.zeros(2, 16, 32, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # never torch arithmetic instead
        hw.functional.smooth_ce(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train.FusedSmoothedCrossEntropyLoss()(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        hw.functional.sce_forward(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32), 0.01)
    crit = train.FusedSmoothedCrossEntropyLoss(0.2)
    assert crit.smooth_factor == 0.2 and crit.last_rank is None and train.FusedSmoothedCrossEntropyLoss().smooth_factor == 0.01
    # the default criterion is the torch one, and it has no correct() of its own: TrainStep keeps its argmax line for it
    assert type(train.TrainStep(model).criterion) is train.SmoothedCrossEntropyLoss
    assert not hasattr(train.SmoothedCrossEntropyLoss(), "correct")
