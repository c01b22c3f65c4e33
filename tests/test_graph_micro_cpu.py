"""CPU: what micro-batches and short batches in the graphed train step decide without a device -- the refusals of
train.GraphedTrainStep(micro_batch=..., ragged=True) and train.TrainStep(pad_to=...), the `clips_independent_in_train`
attribute of the seven models, the padding buffers, the slice loop of TrainStep on a torch-only model, and header <->
bindings <-> exports of hwgat_bsce_fwd / hwgat_bsce_bwd with their argument checks (made before any launch)."""
import ctypes
import importlib

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
train = importlib.import_module("sl-hwgat_amd.train")
NEW_SYMBOLS = {"hwgat_bsce_fwd", "hwgat_bsce_bwd"}
DS = {"src_len": 16, "num_class": 7}


def _hwgate():
    return hw.Model(*hw.HWGATEParams(DS, 2, None, num_kps=32).get_model_params()).train()


def _batch(model, B=8):
    g = torch.Generator().manual_seed(3)
    return torch.rand(B, 16, 32, 2, generator=g), torch.randint(0, 7, (B,), generator=g)


def _adamw(model):
    return torch.optim.AdamW(model.parameters(), lr=5e-4)


# ------------------------------------------------------------------------------------------ the entry points
def test_new_entry_points_declared_bound_and_exported():
    assert NEW_SYMBOLS <= set(hw._lib.declared_symbols())
    assert NEW_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_bsce_")}
    assert set(hw._lib.declared_symbols()) == set(hw._lib._SIGS)
    handle = hw._lib.lib()
    for n in NEW_SYMBOLS:
        assert getattr(handle, n) is not None
    assert handle.hwgat_abi_version() == hw._lib.header_abi_version()


def test_arguments_are_refused_before_any_launch():
    """NULL pointers and an offset outside [0, 2^31): HWGAT_EINVAL (-1); B < 1 or C outside 1..65536 with non-null
    pointers: HWGAT_ESHAPE (-2).  The pointers are never read."""
    L = hw._lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(ptrs, offset=0, B=4, C=10):
        return L.hwgat_bsce_fwd(*ptrs[:3], offset, *ptrs[3:], B, C, 0.01, None)

    def bwd(ptrs, offset=0, B=4, C=10):
        return L.hwgat_bsce_bwd(*ptrs[:3], offset, *ptrs[3:], B, C, 0.01, None)

    assert fwd([None] * 10) == -1 and bwd([None] * 6) == -1
    for hole in range(10):                                   # every pointer is required, the row count included
        args = [p] * 10
        args[hole] = None
        assert fwd(args) == -1, hole
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert bwd(args) == -1, hole
    for offset in (-1, 1 << 31):
        assert fwd([p] * 10, offset=offset) == -1 and bwd([p] * 6, offset=offset) == -1
    for C in (0, 65537):
        assert fwd([p] * 10, C=C) == -2 and bwd([p] * 6, C=C) == -2
    for B in (0, -3, 1 << 31):
        assert fwd([p] * 10, B=B) == -2 and bwd([p] * 6, B=B) == -2


def test_launchers_and_criterion_refuse_the_cpu_and_bad_arguments():
    HF = hw.functional
    z, y = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64)
    word = torch.full((1,), 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # never torch arithmetic instead
        HF.batch_sliced_ce(z, y, 0.01, word, 0)
    crit = train.BatchSlicedCrossEntropyLoss(0.2)
    assert crit.smooth_factor == 0.2 and train.BatchSlicedCrossEntropyLoss().smooth_factor == 0.01
    with pytest.raises(RuntimeError, match="place"):
        crit(z, y)
    crit.place(word, 3)
    assert crit.n_rows is word and crit.offset == 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(z, y)
    with pytest.raises(ValueError, match="n_rows"):
        HF.bsce_forward(z, y, 0.01, torch.zeros(1, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="n_rows"):
        HF.bsce_forward(z, y, 0.01, None, 0)
    with pytest.raises(ValueError, match="offset"):
        HF.bsce_backward(z, y, torch.zeros(2), torch.ones(1), 0.01, word, -1)
    with pytest.raises(ValueError, match="int64"):
        HF.bsce_forward(z, y.int(), 0.01, word, 0)


# ------------------------------------------------------------------------------------------ refusals of the steps
@pytest.mark.parametrize("bad", [0, -2, 2.5, "3", True])
def test_bad_micro_batch_values_are_refused(bad):
    m = _hwgate()
    x, y = _batch(m)
    with pytest.raises(ValueError, match="micro_batch"):
        train.GraphedTrainStep(m, _adamw(m), x, y, micro_batch=bad)
    with pytest.raises(ValueError, match="micro_batch"):
        train.TrainStep(m, _adamw(m), micro_batch=bad, pad_to=8)


def test_reducer_with_micro_batch_or_padding_is_refused():
    m = _hwgate()
    x, y = _batch(m)
    with pytest.raises(NotImplementedError, match="reducer"):
        train.GraphedTrainStep(m, _adamw(m), x, y, reducer=object(), micro_batch=3)
    with pytest.raises(NotImplementedError, match="reducer"):
        train.GraphedTrainStep(m, _adamw(m), x, y, reducer=object(), ragged=True)
    with pytest.raises(NotImplementedError, match="reducer"):
        train.TrainStep(m, _adamw(m), reducer=object(), pad_to=8)


@pytest.mark.parametrize("crit", [train.SmoothedCrossEntropyLoss, train.FusedSmoothedCrossEntropyLoss, torch.nn.CrossEntropyLoss])
def test_padding_needs_the_sliced_criterion(crit):
    m = _hwgate()
    x, y = _batch(m)
    with pytest.raises(ValueError, match="BatchSlicedCrossEntropyLoss"):
        train.GraphedTrainStep(m, _adamw(m), x, y, criterion=crit(), ragged=True)
    with pytest.raises(ValueError, match="BatchSlicedCrossEntropyLoss"):
        train.TrainStep(m, _adamw(m), criterion=crit(), pad_to=8)


def test_models_say_whether_their_train_forward_keeps_clips_apart():
    apart = [_hwgate(),
             hw.HGATEModel(*hw.HGATEParams(DS, 2, None).get_model_params()),
             hw.WGATEModel(*hw.WGATEParams(DS, 2, None, num_kps=32).get_model_params()),
             hw.GATEModel(*hw.GATEParams(DS, 2, None).get_model_params()),
             hw.TransformerModel(*hw.TransformerParams(DS, 2).get_model_params())]
    coupled = [hw.STGCNModel(*hw.STGCNParams(DS, 2).get_model_params()),
               hw.DecoupledGCNModel(*hw.DecoupledGCNParams(DS, 2).get_model_params())]
    assert all(m.clips_independent_in_train is True for m in apart)
    assert all(m.clips_independent_in_train is False for m in coupled)
    for m in coupled:                                        # BatchNorm statistics and DropGraph normalisers would see the padding
        m.train()
        x, y = torch.rand(4, 8, 29, 2), torch.zeros(4, dtype=torch.int64)
        with pytest.raises(ValueError, match="couples the clips"):
            train.GraphedTrainStep(m, _adamw(m), x, y, ragged=True)
        with pytest.raises(ValueError, match="couples the clips"):
            train.TrainStep(m, _adamw(m), pad_to=4)
    with pytest.raises(ValueError, match="couples the clips"):                     # a model that does not say is refused too
        train.TrainStep(torch.nn.Linear(4, 3), pad_to=4)


def test_pad_to_is_checked_and_the_defaults_stay():
    m = _hwgate()
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="pad_to"):
            train.TrainStep(m, pad_to=bad)
    s = train.TrainStep(m, pad_to=8, micro_batch=3)
    assert type(s.criterion) is train.BatchSlicedCrossEntropyLoss and s.n_rows is None
    s = train.TrainStep(m)
    assert type(s.criterion) is train.SmoothedCrossEntropyLoss and s.pad_to is None and s.n_rows is None
    # the graphed step still starts with its device check when the new arguments are fine
    x, y = _batch(m)
    with pytest.raises(ValueError, match="device inputs"):
        train.GraphedTrainStep(m, _adamw(m), x, y, micro_batch=3, ragged=True)


# ------------------------------------------------------------------------------------------ the padding buffers
def test_padded_batch_zero_fills_and_writes_the_row_count_on_change():
    x, y = torch.rand(5, 3, 2) + 1.0, torch.arange(1, 6)
    pad = train._PaddedBatch(5, x, y)
    assert pad.x.shape == (5, 3, 2) and pad.y.dtype == torch.int64 and pad.n_rows.dtype == torch.int32
    pad.load(x, y)
    assert torch.equal(pad.x, x) and torch.equal(pad.y, y) and pad.n_rows.item() == 5
    word = pad.n_rows
    pad.load(x[:2] + 1.0, y[:2] + 1)
    assert torch.equal(pad.x[:2], x[:2] + 1.0) and not pad.x[2:].any() and not pad.y[2:].any()
    assert pad.n_rows is word and word.item() == 2
    pad.x[2:] = 7.0                                          # the same row count again: the tail is left alone
    version = word._version
    pad.load(x[:2], y[:2])
    assert (pad.x[2:] == 7.0).all() and word._version == version
    pad.load(x[:4], y[:4])
    assert torch.equal(pad.x[:4], x[:4]) and not pad.x[4:].any() and word.item() == 4
    for bad_x, bad_y in ((torch.rand(6, 3, 2), torch.zeros(6, dtype=torch.int64)),        # n > B
                         (torch.rand(0, 3, 2), torch.zeros(0, dtype=torch.int64)),        # no rows
                         (torch.rand(2, 3, 3), torch.zeros(2, dtype=torch.int64)),        # another clip shape
                         (torch.rand(2, 3, 2), torch.zeros(3, dtype=torch.int64))):       # targets of another length
        with pytest.raises(ValueError, match="built for 1 to 5"):
            pad.load(bad_x, bad_y)


# ------------------------------------------------------------------------------------------ the slice loop, torch only
def test_slice_loop_of_the_eager_step_on_a_torch_model():
    """TrainStep's slices on a model that needs no device: the loss and the gradient of 3 + 3 + 2 rows are the full
    batch's up to fp64 rounding, `correct` is the full count, and micro_batch None / >= n is one slice"""
    torch.manual_seed(0)
    net = torch.nn.Linear(6, 4).double()
    x, y = torch.randn(8, 6, dtype=torch.float64), torch.randint(0, 4, (8,))
    res = {}
    for mb in (None, 3, 8, 100):
        net.zero_grad()
        s = train.TrainStep(net, None, None, micro_batch=mb)
        s(x, y)
        res[mb] = (s.loss.clone(), int(s.correct), net.weight.grad.clone())
    want = int((net(x).argmax(-1) == y).sum())
    for mb in (3, 8, 100):
        assert abs(float(res[mb][0] - res[None][0])) < 1e-14 and res[mb][1] == res[None][1] == want
        assert (res[mb][2] - res[None][2]).abs().max() < 1e-14
    assert torch.equal(res[8][0], res[None][0]) and torch.equal(res[100][2], res[None][2])
