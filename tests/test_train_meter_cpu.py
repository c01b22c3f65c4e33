"""CPU: the host side of the train meters and the epoch loop (csrc/train_meter.hip, train.TrainMeter, train.EarlyStopper,
train.EpochBook, train.EpochLoop, checkpoint.save_checkpoint(extra=...) / read_extra) -- the entry points in the header, the
binding and the library, their argument checks, the slot constants, the meter's state dict before any device exists, the
early-stopping rule and the loop's bookkeeping against hand-written tables, the checkpoint's extra key, and the refusal of
a short batch for a model that cannot be padded."""
import ctypes
import importlib
import re
import struct

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
train = importlib.import_module("sl-hwgat_amd.train")
optim = importlib.import_module("sl-hwgat_amd.optim")
ck = hw.checkpoint
CPU = torch.device("cpu")
METER_SYMBOLS = {"hwgat_meter_bytes", "hwgat_meter_fold", "hwgat_meter_close"}
NINE = {"model_state_dict", "optimizer_state_dict", "train_loss_list", "val_loss_list", "train_acc_list", "val_acc_list",
        "epoch", "learning_rate", "scheduler"}


def _f64_word(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _f32_word(v):
    return struct.unpack("<q", struct.pack("<fI", v, 0))[0]


# ------------------------------------------------------------------------------------------ header, binding, library
def test_symbols_abi_and_constants_follow_the_header():
    assert METER_SYMBOLS <= set(hw._lib.declared_symbols())
    assert METER_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_meter_")}
    L = hw._lib.lib()
    for name in METER_SYMBOLS:
        assert getattr(L, name) is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HWGAT_METER_(\w+)\s+(\d+)\s*$", src, flags=re.M)}
    running = {k[2:]: v for k, v in slots.items() if k.startswith("R_")}
    mine = dict(STEPS=train.METER_R_STEPS, ROWS=train.METER_R_ROWS, CORRECT=train.METER_R_CORRECT,
                LOSS_SUM=train.METER_R_LOSS_SUM, FINITE_STEPS=train.METER_R_FINITE_STEPS,
                NONFINITE_LOSS=train.METER_R_NONFINITE_LOSS, SKIPPED=train.METER_R_SKIPPED, LAST_LOSS=train.METER_R_LAST_LOSS,
                MAX_LOSS=train.METER_R_MAX_LOSS, MAX_GRAD_NORM=train.METER_R_MAX_GRAD_NORM)
    assert running == mine and sorted(mine.values()) == list(range(10)) and max(mine.values()) < train.METER_NRUN
    assert (slots["LOG_TOTAL"], slots["CLOSED"], slots["OVERFLOW"]) == (train.METER_LOG_TOTAL, train.METER_CLOSED,
                                                                       train.METER_OVERFLOW) == (0, 1, 2)
    assert slots["RUN"] == train.METER_RUN == 4 and slots["NRUN"] == train.METER_NRUN == 12
    assert re.search(r"#define\s+HWGAT_METER_LOG\s+\(HWGAT_METER_RUN \+ HWGAT_METER_NRUN\)", src)
    assert train.METER_LOG == train.METER_RUN + train.METER_NRUN
    assert re.search(r"#define\s+HWGAT_METER_MAX_CAPACITY\s+\(1 << 24\)", src) and train.METER_MAX_CAPACITY == 1 << 24
    # the guard slots the fold kernel reads
    assert int(re.search(r"#define\s+HWGAT_GGUARD_SKIP\s+(\d+)", src).group(1)) == optim.G_SKIP
    assert int(re.search(r"#define\s+HWGAT_GGUARD_TOTAL_NORM\s+(\d+)", src).group(1)) == optim.G_TOTAL_NORM


def test_block_size_and_argument_checks_without_launching():
    L = hw._lib.lib()
    for log, hist in ((0, 0), (0, 1), (4, 1), (7, 1024), (1 << 24, 1 << 24)):
        assert L.hwgat_meter_bytes(log, hist) == 8 * (16 + 2 * log + 12 * hist)
        if log <= 1024:
            assert train.TrainMeter(log, hist).words * 8 == L.hwgat_meter_bytes(log, hist)
            assert hw.functional.meter_words(log, hist) == train.TrainMeter(log, hist).words
    for log, hist in ((-1, 0), (0, -1), ((1 << 24) + 1, 0), (0, (1 << 24) + 1)):
        assert L.hwgat_meter_bytes(log, hist) == -1
        with pytest.raises(ValueError):
            hw.functional.meter_words(log, hist)
    buf = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)      # aligned host memory: never dereferenced
    odd = ctypes.c_void_p(buf.value + 4)
    fold, close = L.hwgat_meter_fold, L.hwgat_meter_close
    assert fold(None, buf, buf, None, 4, None, 0, None) == -1
    assert fold(odd, buf, buf, None, 4, None, 0, None) == -1           # the block holds 8-byte words
    assert fold(buf, None, buf, None, 4, None, 0, None) == -1
    assert fold(buf, buf, None, None, 4, None, 0, None) == -1
    assert fold(buf, buf, odd, None, 4, None, 0, None) == -1           # an int64 word
    assert fold(buf, buf, buf, None, -1, None, 0, None) == -1
    assert fold(buf, buf, buf, None, 4, None, -1, None) == -1
    assert close(None, 0, 1, None) == -1
    assert close(odd, 0, 1, None) == -1
    assert close(buf, -1, 1, None) == -1
    assert close(buf, 0, -1, None) == -1


def test_wrappers_refuse_cpu_tensors_and_wrong_words(monkeypatch):
    HF = hw.functional
    block = torch.zeros(train.TrainMeter(0, 1).words, dtype=torch.int64)
    loss, correct = torch.zeros((), dtype=torch.float32), torch.zeros((), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.meter_fold(block, loss, correct, None, 4, None, 0, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.meter_close(block, 0, 1)
    with pytest.raises(ValueError, match="meter block"):
        HF.meter_fold(block[:-1], loss, correct, None, 4, None, 0, 1)
    with pytest.raises(ValueError, match="meter block"):
        HF.meter_close(block.double(), 0, 1)
    with pytest.raises(ValueError, match="fp32"):
        HF.meter_fold(block, loss.double(), correct, None, 4, None, 0, 1)
    with pytest.raises(ValueError, match="int64"):
        HF.meter_fold(block, loss, correct.int(), None, 4, None, 0, 1)
    with pytest.raises(ValueError, match="n_rows"):
        HF.meter_fold(block, loss, correct, torch.zeros(1, dtype=torch.int64), 4, None, 0, 1)
    with pytest.raises(ValueError, match="batch_rows"):
        HF.meter_fold(block, loss, correct, None, -1, None, 0, 1)
    with pytest.raises(ValueError, match="guard"):
        HF.meter_fold(block, loss, correct, None, 4, torch.zeros(16), 0, 1)
    m = train.TrainMeter()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.fold(loss, correct, batch_rows=4)
    with pytest.raises(ValueError, match="row count"):
        m.fold(loss, correct)
    with pytest.raises(RuntimeError, match="folded nothing"):
        m.close_epoch()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before capturing"):      # never allocates inside a capture
        m.bind(torch.device("cuda:0"))
    assert m._block is None
    for bad in (-1, 1.5, True, (1 << 24) + 1):
        with pytest.raises(ValueError):
            train.TrainMeter(log_capacity=bad)
        with pytest.raises(ValueError):
            train.TrainMeter(history_capacity=bad)


# ------------------------------------------------------------------------------------------ the meter's state dict
def _hand_state():
    """a meter with log capacity 2 and history capacity 3: one closed epoch, an open one, three logged steps"""
    run = [0] * 12
    run[train.METER_R_STEPS], run[train.METER_R_ROWS], run[train.METER_R_CORRECT] = 3, 10, 7
    run[train.METER_R_LOSS_SUM] = _f64_word(0.1 + 2.5)
    run[train.METER_R_FINITE_STEPS], run[train.METER_R_NONFINITE_LOSS], run[train.METER_R_SKIPPED] = 2, 1, 1
    run[train.METER_R_LAST_LOSS], run[train.METER_R_MAX_LOSS] = _f32_word(float("inf")), _f32_word(2.5)
    run[train.METER_R_MAX_GRAD_NORM] = _f64_word(3.25)
    closed = [0] * 12
    closed[train.METER_R_STEPS], closed[train.METER_R_ROWS], closed[train.METER_R_CORRECT] = 2, 8, 2
    closed[train.METER_R_LOSS_SUM], closed[train.METER_R_FINITE_STEPS] = _f64_word(3.0), 2
    rec = lambda loss, c, n, g: list(struct.unpack("<qq", struct.pack("<fiif", loss, c, n, g)))
    log = rec(0.75, 1, 2, 0.5) + rec(1.5, 3, 4, 1.25)        # slot 0 holds record 2, slot 1 record 1
    return dict(log_capacity=2, history_capacity=3, head=[3, 1, 0, 0] + run, log=log, history=closed)


def test_state_dict_round_trips_before_any_device_exists(tmp_path):
    fresh = train.TrainMeter(2, 3).state_dict()
    assert fresh == dict(log_capacity=2, history_capacity=3, head=[0] * 16, log=[0] * 4, history=[])
    sd = _hand_state()
    m = train.TrainMeter(2, 3)
    m.load_state_dict(sd)
    assert m.state_dict() == sd and m._block is None
    r = m.result()
    assert (r["steps"], r["rows"], r["correct"], r["finite_steps"], r["nonfinite_loss"], r["skipped"]) == (3, 10, 7, 2, 1, 1)
    assert r["loss_sum"] == 0.1 + 2.5 and r["loss"] == (0.1 + 2.5) / 2 and r["acc"] == 7 / 10
    assert r["last_loss"] == float("inf") and r["max_loss"] == 2.5 and r["max_grad_norm"] == 3.25
    assert (r["log_total"], r["epochs_closed"], r["overflow"]) == (3, 1, 0)
    h = m.history()
    assert len(h) == 1 and (h[0]["steps"], h[0]["rows"], h[0]["correct"], h[0]["loss"], h[0]["acc"]) == (2, 8, 2, 1.5, 0.25)
    assert m.step_log() == [dict(step=1, loss=1.5, correct=3, rows=4, grad_norm=1.25),
                            dict(step=2, loss=0.75, correct=1, rows=2, grad_norm=0.5)]
    # plain values: the safe loader takes them
    path = str(tmp_path / "meter.pt")
    torch.save({"meter": sd}, path)
    assert torch.load(path, weights_only=True)["meter"] == sd
    other = train.TrainMeter(2, 3)
    other.load_state_dict(torch.load(path, weights_only=True)["meter"])
    assert other.state_dict() == sd
    with pytest.raises(ValueError, match="capacities"):
        train.TrainMeter(4, 3).load_state_dict(sd)
    with pytest.raises(ValueError, match="do not fit"):
        train.TrainMeter(2, 3).load_state_dict(dict(sd, history=[0] * 48))
    m.reset()
    assert m.state_dict() == fresh
    empty = train.TrainMeter().result()
    assert empty["steps"] == 0 and empty["loss"] == 0.0 and empty["acc"] == 0.0 and train.TrainMeter().history() == []


# ------------------------------------------------------------------------------------------ early stopping
# (patience, min_delta, accuracies, the answer to each)
EARLY_TABLE = [
    (1, 0, [0.1, 0.2, 0.3, 0.4], [False, False, False, False]),                      # rising: never
    (1, 0, [0.5, 0.4], [False, True]),
    (1, 0, [0.5, 0.5, 0.5, 0.4], [False, False, False, True]),                       # a tie neither resets nor counts
    (3, 0, [0.5, 0.4, 0.3, 0.6, 0.5, 0.5, 0.4, 0.3], [False, False, False, False, False, False, True, True]),
    (3, 0, [0.5, 0.4, 0.4, 0.4], [False, False, False, True]),                       # a plateau below the best counts
    (2, 0.05, [0.5, 0.5, 0.5], [False, False, True]),                                # with a margin a tie counts
    (2, 0.05, [0.5, 0.52, 0.5, 0.56, 0.6], [False, False, False, False, False]),     # any rise resets
    (2, 0.05, [0.5, 0.46, 0.54], [False, False, False]),
    (1, 0, [0.0, 0.0], [False, False]),                                              # 0 is not above the start value 0
    (1, 0.05, [0.0], [True]),
]


@pytest.mark.parametrize("patience,min_delta,accs,want", EARLY_TABLE)
def test_early_stopper_follows_the_table(patience, min_delta, accs, want):
    s = train.EarlyStopper(patience, min_delta)
    assert [s.early_stop(a) for a in accs] == want
    assert s.max_validation_acc == max([0.0] + accs)


# ------------------------------------------------------------------------------------------ the loop's bookkeeping
# epoch: (val_loss, val_acc) and the files that epoch writes with save_interval 3.  Ties at epochs 1, 4, 6 and 7
BOOK_TABLE = [
    ((2.0, 0.10), ["best_loss", "best_acc"]),
    ((2.0, 0.10), []),                         # both tie: strict < and > write nothing
    ((1.5, 0.10), ["best_loss"]),
    ((1.7, 0.25), ["best_acc", "3"]),
    ((1.5, 0.25), []),                         # ties with the best loss (epoch 2) and the best accuracy (epoch 3)
    ((1.2, 0.30), ["best_loss", "best_acc"]),
    ((1.3, 0.30), ["6"]),
    ((1.2, 0.35), ["best_acc"]),               # the loss ties the best
]


def test_book_writes_the_files_of_the_table_and_resumes_from_lists():
    book = train.EpochBook(save_interval=3)
    assert (book.best_val_loss, book.best_val_acc) == (9999, 0.0)
    for epoch, ((vl, va), files) in enumerate(BOOK_TABLE):
        got, stop = book.record(epoch, 3.0 - 0.1 * epoch, 0.05 * epoch, vl, va)
        assert got == files and stop is False, epoch
    assert book.val_loss_list == [t[0][0] for t in BOOK_TABLE] and book.val_acc_list == [t[0][1] for t in BOOK_TABLE]
    assert book.train_loss_list == [3.0 - 0.1 * e for e in range(8)] and book.train_acc_list == [0.05 * e for e in range(8)]
    assert (book.best_val_loss, book.best_val_acc) == (1.2, 0.35)
    again = train.EpochBook.resumed(book.lists, save_interval=3)
    assert again.lists == book.lists and again.lists[0] is not book.lists[0]
    assert (again.best_val_loss, again.best_val_acc) == (1.2, 0.35)
    assert again.record(8, 1.0, 0.5, 1.2, 0.35) == ([], False)
    assert again.record(9, 1.0, 0.5, 1.1, 0.20) == (["best_loss", "9"], False)
    empty = train.EpochBook.resumed([[], [], [], []])
    assert (empty.best_val_loss, empty.best_val_acc) == (99999, 0.0)
    assert empty.record(0, 1.0, 0.5, 5.0, 0.0) == (["best_loss"], False)     # epoch 0 is never an interval file
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            train.EpochBook(save_interval=bad)


def test_book_stops_when_the_stopper_says_so():
    book = train.EpochBook(save_interval=1, early_stopper=train.EarlyStopper(patience=2))
    stops = [book.record(e, 1.0, 0.5, 1.0, a)[1] for e, a in enumerate([0.3, 0.2, 0.4, 0.1, 0.1])]
    assert stops == [False, False, False, False, True]


# ------------------------------------------------------------------------------------------ the checkpoint's extra key
def _hwgate():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, CPU, num_kps=32)
    return hw.Model(*hp.get_model_params())


def test_checkpoint_extra_round_trips_and_is_absent_by_default(tmp_path):
    model = _hwgate()
    opt = ck.get_optimizer(model)
    sch = ck.get_scheduler(opt)
    plain, extra_path = str(tmp_path / "plain.pt"), str(tmp_path / "extra.pt")
    ck.save_checkpoint(plain, model, opt, sch, [0.1], [2.0], [0.2], [1.9], 6, 4.5e-4)
    assert set(torch.load(plain, map_location="cpu", weights_only=True)) == NINE
    assert ck.read_extra(plain) == {}
    guard = optim.GradGuard(max_norm=1.0, on_nonfinite="skip")
    meter = train.TrainMeter(2, 3)
    meter.load_state_dict(_hand_state())
    extra = dict(guard=guard.state_dict(), averager=None, meter=meter.state_dict(), drop_calls=41)
    ck.save_checkpoint(extra_path, model, opt, sch, [0.1], [2.0], [0.2], [1.9], 6, 4.5e-4, extra=extra)
    raw = torch.load(extra_path, map_location="cpu", weights_only=True)
    assert set(raw) == NINE | {"extra"} and ck.EXTRA_KEY == "extra"
    assert ck.read_extra(extra_path) == extra
    assert ck.read_extra(extra_path)["meter"] == _hand_state()
    # the nine keys hold the same whatever the extras are, and the file still resumes
    both = torch.load(plain, map_location="cpu", weights_only=True)
    assert all(torch.equal(both["model_state_dict"][k], v) for k, v in raw["model_state_dict"].items())
    assert {k: both[k] for k in NINE - {"model_state_dict", "optimizer_state_dict"}} == \
        {k: raw[k] for k in NINE - {"model_state_dict", "optimizer_state_dict"}}
    _, _, _, lists, start = ck.load_checkpoint(extra_path, _hwgate(), ck.get_optimizer(model), ck.get_scheduler(opt))
    assert lists == [[2.0], [1.9], [0.1], [0.2]] and start == 7
    with pytest.raises(TypeError, match="extra"):
        ck.save_checkpoint(plain, model, opt, sch, [], [], [], [], 0, 1e-3, extra=[1, 2])


# ------------------------------------------------------------------------------------------ the loop on the host
def _stgcn():
    hp = hw.STGCNParams({"src_len": 32, "num_class": 7}, 2, CPU)
    return hw.STGCNModel(*hp.get_model_params())


def test_loop_refuses_a_short_batch_for_a_coupled_model_before_any_kernel(monkeypatch):
    model = _stgcn()
    assert model.clips_independent_in_train is False
    opt = optim.DeviceAdamW(list(model.parameters()), lr=1e-3)

    def no_launch(name, *args):
        raise AssertionError(f"{name} was launched")
    for mod in (hw.functional, optim, hw._lib):
        monkeypatch.setattr(mod, "call", no_launch)
    x, y = torch.zeros(4, 32, 29, 2), torch.zeros(4, dtype=torch.int64)
    for graph in (True, False):
        loop = train.EpochLoop(model, opt, None, batch_size=4, example=(x, y), num_classes=7, graph=graph)
        assert loop.padded is False
        with pytest.raises(ValueError, match="drop_last"):
            loop.run([(x[:3], y[:3]), (x, y)], [(x, y)], epochs=1)
        assert loop.step is None and loop.evaluator is None and loop.meter._block is None
        assert loop.book.lists == [[], [], [], []] and loop.written == []


def test_loop_argument_checks():
    model = _hwgate()
    opt = optim.DeviceAdamW(list(model.parameters()), lr=2e-3)
    x, y = torch.zeros(4, 16, 32, 2), torch.zeros(4, dtype=torch.int64)
    loop = train.EpochLoop(model, opt, None, batch_size=4, example=(x, y), num_classes=5)
    assert loop.padded is True and loop.lr == 2e-3 and loop.start_epoch == 0
    assert (loop.book.save_interval, loop.smooth_factor, loop.k, loop.graph) == (100, 0.01, 1, True)
    with pytest.raises(ValueError, match="batch_size"):
        train.EpochLoop(model, opt, None, batch_size=8, example=(x, y), num_classes=5)
    with pytest.raises(ValueError, match="k must"):
        train.EpochLoop(model, opt, None, batch_size=4, example=(x, y), num_classes=5, k=0)
    with pytest.raises(ValueError, match="averager"):
        train.EpochLoop(model, opt, None, batch_size=4, example=(x, y), num_classes=5, eval_averaged=True)
    with pytest.raises(ValueError, match="history_capacity"):
        train.EpochLoop(model, opt, None, batch_size=4, example=(x, y), num_classes=5, meter=train.TrainMeter(4, 0))
    with pytest.raises(ValueError, match="micro_batch"):
        train.EpochLoop(model, opt, None, batch_size=4, example=(x, y), num_classes=5, micro_batch=0)
