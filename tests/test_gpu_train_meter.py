"""GPU: the train meters (csrc/train_meter.hip, train.TrainMeter) and the epoch loop on top of them (train.EpochLoop).

The fold kernel against a Python restatement on hand-set inputs; the meter inside the captured and the eager train step
against the host's own sums of the same run's per-step `loss` / `correct`; a NaN batch under a skipping guard; that a meter
changes nothing the step computes; the loop end to end with its checkpoints, a resume that must repeat the uninterrupted
run bit for bit, and the early stop.

No tolerance appears below.  The integer words count; `loss_sum` is one fp64 addition per step of a float32 widened to
double, which is exactly what Python's `total += loss.item()` does, in the same order; `max_grad_norm` and `max_loss`
are copies of an input.  Every comparison is for equality."""
import importlib
import math
import os

import pytest
import torch

import stgcn_helpers as SH

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
optim = importlib.import_module("sl-hwgat_amd.optim")
evaluate = importlib.import_module("sl-hwgat_amd.evaluate")
ck = hw.checkpoint
DEV = torch.device("cuda:0")
THRESHOLDS = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]   # HWGATE.py:96 draws these at random
NC = 10
NINE = {"model_state_dict", "optimizer_state_dict", "train_loss_list", "val_loss_list", "train_acc_list", "val_acc_list",
        "epoch", "learning_rate", "scheduler"}
SENTINEL = -0x0123456789ABCDEF


def _same(a, b):
    """equal, a NaN being equal to a NaN; lists and dicts element-wise"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b or (a != a and b != b)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


# ------------------------------------------------------------------------------------------ the kernels alone
class _Python:
    """the running words, the log and the history as include/hwgat_hip.h describes them, in Python"""

    def __init__(self, log_capacity, history_capacity):
        self.L, self.H = log_capacity, history_capacity
        self.log, self.history, self.closed, self.overflow = [], [], 0, 0
        self.zero()

    def zero(self):
        self.run = dict(steps=0, rows=0, correct=0, loss_sum=0.0, finite_steps=0, nonfinite_loss=0, skipped=0,
                        last_loss=0.0, max_loss=0.0, max_grad_norm=0.0)

    def fold(self, loss, correct, rows, guard):
        r = self.run
        r["steps"] += 1
        r["rows"] += rows
        r["correct"] += correct
        if math.isfinite(loss):
            r["finite_steps"] += 1
            r["loss_sum"] += loss                                 # Python's float: one fp64 addition
            if r["finite_steps"] == 1 or loss > r["max_loss"]:
                r["max_loss"] = loss
        else:
            r["nonfinite_loss"] += 1
        r["last_loss"] = loss
        norm = 0.0
        if guard is not None:
            skip, norm = guard
            r["skipped"] += int(skip != 0.0)
            if norm > r["max_grad_norm"]:
                r["max_grad_norm"] = norm
        if self.L:
            self.log.append(dict(step=len(self.log), loss=loss, correct=correct, rows=rows, grad_norm=_f32(norm)))

    def close(self):
        entry = dict(self.run)
        if self.closed < self.H:
            self.history.append(entry)
        else:
            self.overflow += 1
            if self.H:
                self.history[-1] = entry
        self.closed += 1
        self.zero()

    def result(self, run=None):
        r = dict(self.run if run is None else run)
        r["loss"] = r["loss_sum"] / max(r["finite_steps"], 1)
        r["acc"] = r["correct"] / max(r["rows"], 1)
        return r

    def header(self):
        return dict(log_total=len(self.log), epochs_closed=self.closed, overflow=self.overflow)


LOSSES = [1.0 / 3.0, 123.456, float("nan"), 1e-3, 0.7, float("inf"), 2.0 / 7.0, 5.5, 0.1]
CORRECT = [3, 0, 1, 1, 4, 2, 0, 1, 7]
ROWS = [4, 4, 1, 2, 4, 3, 1, 1, 8]                         # a batch of one row among them
SKIP = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]       # the guard skipped folds 2 and 6
NORMS = [1.0, 2.5000000001, float("nan"), 0.75, 2.25, 0.1, 1e-3, 0.7000000001, 0.3]


@pytest.mark.parametrize("with_guard", [True, False])
@pytest.mark.parametrize("log_capacity", [4, 0])
def test_fold_and_close_against_python(log_capacity, with_guard):
    """nine folds, a close after the fifth and one after the ninth with room for one closed epoch: the second close
    overflows.  With log capacity 4 the ring wraps twice.  Rows come from the device word on even folds and from the
    host integer on odd ones.  The block sits inside a larger buffer whose other words must not change"""
    m = train.TrainMeter(log_capacity, 1)
    buf = torch.full((m.words + 16,), SENTINEL, dtype=torch.int64, device=DEV)
    m._block = buf[8:8 + m.words]
    m._block.zero_()
    ref = _Python(log_capacity, 1)
    guard = torch.zeros(optim.GUARD_NSTATE, dtype=torch.float64, device=DEV) if with_guard else None
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    correct = torch.zeros((), dtype=torch.int64, device=DEV)
    n_rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    for i in range(9):
        loss.fill_(LOSSES[i])
        correct.fill_(CORRECT[i])
        n_rows.fill_(ROWS[i])
        if with_guard:
            guard[optim.G_SKIP], guard[optim.G_TOTAL_NORM] = SKIP[i], NORMS[i]
        if i % 2 == 0:
            m.fold(loss, correct, n_rows=n_rows, guard=guard)
        else:
            m.fold(loss, correct, batch_rows=ROWS[i], guard=guard)
        ref.fold(loss.item(), CORRECT[i], ROWS[i], (SKIP[i], NORMS[i]) if with_guard else None)
        if i == 3:                                           # an open epoch: four folds, nothing closed
            got = m.result()
            assert _same({k: got[k] for k in ref.result()}, ref.result())
            assert {k: got[k] for k in ref.header()} == ref.header() and m.history() == []
        if i in (4, 8):
            before = ref.result()
            m.close_epoch()
            ref.close()
            got = m.result()
            assert _same({k: got[k] for k in ref.result()}, ref.result()) and got["steps"] == 0 and got["loss_sum"] == 0.0
            assert {k: got[k] for k in ref.header()} == ref.header()
            hist = m.history()
            assert len(hist) == 1 and _same(hist[0], before) and _same(hist, [ref.result(h) for h in ref.history])
            assert _same(m.step_log(), ref.log[-log_capacity:] if log_capacity else [])
    got = m.result()
    assert (got["epochs_closed"], got["overflow"], got["log_total"]) == (2, 1, 9 if log_capacity else 0)
    hist = m.history()[0]                                     # the second epoch: folds 5..8
    assert (hist["steps"], hist["rows"], hist["correct"]) == (4, 13, 10)
    assert (hist["finite_steps"], hist["nonfinite_loss"], hist["skipped"]) == (3, 1, 1 if with_guard else 0)
    total = 0.0
    for v in (LOSSES[6], LOSSES[7], LOSSES[8]):
        total += _f32(v)
    assert hist["loss_sum"] == total and hist["max_loss"] == 5.5 and hist["last_loss"] == _f32(0.1)
    assert hist["max_grad_norm"] == (0.7000000001 if with_guard else 0.0)
    if log_capacity:
        assert [r["step"] for r in m.step_log()] == [5, 6, 7, 8]
    torch.cuda.synchronize()
    assert (buf[:8] == SENTINEL).all().item() and (buf[8 + m.words:] == SENTINEL).all().item()
    # snapshot / restore / reset / the state dict of a live block
    snap, sd = m.snapshot(), m.state_dict()
    m.fold(loss, correct, batch_rows=2, guard=guard)
    assert m.result()["steps"] == 1
    m.restore(snap)
    assert m.state_dict() == sd and m.result()["steps"] == 0
    other = train.TrainMeter(log_capacity, 1)
    other.load_state_dict(sd)
    other.bind(DEV)
    assert torch.equal(other._block, m._block)
    m.reset()
    assert not m._block.any().item()


# ------------------------------------------------------------------------------------------ the meter in the step
def _hwgate(dtype, seed=11):
    torch.manual_seed(seed)
    hp = hw.HWGATEParams({"src_len": 32, "num_class": NC}, 2, DEV, num_kps=32)
    model = hw.Model(*hp.get_model_params()).to(DEV)
    model.set_activation_dtype(dtype)
    model.train()
    model.threshold_override = THRESHOLDS
    model.deterministic_train = True
    return model


def _clips(n, seed, T=32, V=32, C=2, device=DEV):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, T, V, C, generator=g)
    y = torch.randint(0, NC, (n,), generator=g)
    return x.to(device), y.to(device)


def _guarded_adamw(model):
    opt = optim.DeviceAdamW(list(model.parameters()), lr=5e-4)
    opt.guard = optim.GradGuard(max_norm=1.0, on_nonfinite="skip")
    return opt


def _make_step(model, opt, x, y, graphed, meter):
    if graphed:
        return train.GraphedTrainStep(model, opt, x, y, ragged=True, micro_batch=2, meter=meter)
    return train.TrainStep(model, opt, micro_batch=2, pad_to=4, meter=meter)


@pytest.mark.parametrize("graphed", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_meter_in_the_step_equals_the_hosts_own_sums(dtype, graphed):
    """batches of 4, 4 and 2 rows for two epochs through a step built for 4 rows in micro-batches of 2, with a guard that
    clips.  `loss` and `correct` are cloned on the device after every step and read at the end; the closed epochs must be
    their Python sums.  A fold of the warm-up would show in `steps`"""
    model = _hwgate(dtype)
    opt = _guarded_adamw(model)
    x, y = _clips(10, 5)
    meter = train.TrainMeter(log_capacity=8)
    step = _make_step(model, opt, x[:4], y[:4], graphed, meter)
    if graphed:
        assert meter.result()["steps"] == 0 and meter.result()["log_total"] == 0      # the warm-up left no trace
    trace = []
    for epoch in range(2):
        for lo, hi in ((0, 4), (4, 8), (8, 10)):
            step(x[lo:hi], y[lo:hi])
            trace.append((step.loss.clone(), step.correct.clone(), opt.guard.total_norm.clone(), hi - lo))
        meter.close_epoch()
    torch.cuda.synchronize()
    host = [(l.item(), int(c.item()), n.item(), rows) for l, c, n, rows in trace]
    hist = meter.history()
    assert len(hist) == 2 and meter.result()["steps"] == 0 and meter.result()["overflow"] == 0
    for e in range(2):
        mine = host[3 * e:3 * e + 3]
        total = 0.0
        for l, _, _, _ in mine:
            total += l
        h = hist[e]
        print(f"epoch {e}: loss_sum {h['loss_sum']!r} host {total!r}; correct {h['correct']} rows {h['rows']}")
        assert all(math.isfinite(l) for l, _, _, _ in mine)
        assert (h["steps"], h["rows"], h["finite_steps"], h["nonfinite_loss"], h["skipped"]) == (3, 10, 3, 0, 0)
        assert h["correct"] == sum(c for _, c, _, _ in mine)
        assert h["loss_sum"] == total and h["loss"] == total / 3 and h["acc"] == h["correct"] / 10
        assert h["last_loss"] == mine[-1][0] and h["max_loss"] == max(l for l, _, _, _ in mine)
        assert h["max_grad_norm"] == max(n for _, _, n, _ in mine) > 0.0          # the guard's own fp64 word
    assert meter.step_log() == [dict(step=i, loss=l, correct=c, rows=rows, grad_norm=_f32(n))
                                for i, (l, c, n, rows) in enumerate(host)]


def test_a_nan_batch_under_a_skipping_guard_is_counted_once():
    model = _hwgate(torch.float32)
    opt = _guarded_adamw(model)
    x, y = _clips(12, 6)
    x[5, 3, 7, 1] = float("nan")                              # in the second batch
    meter = train.TrainMeter()
    step = _make_step(model, opt, x[:4], y[:4], True, meter)
    for lo in (0, 4, 8):
        step(x[lo:lo + 4], y[lo:lo + 4])
    r = meter.result()
    assert (r["steps"], r["rows"], r["skipped"], r["nonfinite_loss"], r["finite_steps"]) == (3, 12, 1, 1, 2)
    assert math.isfinite(r["loss_sum"]) and r["loss_sum"] > 0.0 and math.isfinite(r["max_grad_norm"])
    assert all(torch.isfinite(p).all().item() for p in model.parameters())
    assert opt.guard.counters()["skipped"] == 1


def test_a_meter_changes_nothing_the_step_computes():
    runs = []
    for meter in (train.TrainMeter(log_capacity=2), None):
        model = _hwgate(torch.float32)
        opt = _guarded_adamw(model)
        x, y = _clips(10, 5)
        step = train.GraphedTrainStep(model, opt, x[:4], y[:4], ragged=True, micro_batch=2, meter=meter)
        losses = []
        for lo, hi in ((0, 4), (4, 8), (8, 10)):
            losses.append(step(x[lo:hi], y[lo:hi]).clone())
        runs.append((losses, [p.detach().clone() for p in model.parameters()]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_with_a_torch_optimizer_the_fold_is_still_captured():
    """the optimizer steps after the replay, the fold is a node behind the backward: no guard, the static batch size"""
    model = _hwgate(torch.float32)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    x, y = _clips(4, 8)
    meter = train.TrainMeter(log_capacity=2)
    step = train.GraphedTrainStep(model, opt, x, y, meter=meter)
    assert meter.result()["steps"] == 0
    clones = []
    for _ in range(3):
        step(x, y)
        clones.append((step.loss.clone(), step.correct.clone()))
    r = meter.result()
    total = 0.0
    for l, _ in clones:
        total += l.item()
    assert (r["steps"], r["rows"], r["finite_steps"], r["skipped"], r["max_grad_norm"]) == (3, 12, 3, 0, 0.0)
    assert r["loss_sum"] == total and r["correct"] == sum(int(c.item()) for _, c in clones)
    assert [s["step"] for s in meter.step_log()] == [1, 2] and all(s["grad_norm"] == 0.0 for s in meter.step_log())


# ------------------------------------------------------------------------------------------ the epoch loop
def _batches(x, y, B):
    return [(x[i:i + B], y[i:i + B]) for i in range(0, x.shape[0], B)]


def test_eval_averaged_validates_on_the_averaged_weights():
    model = _hwgate(torch.float32)
    opt = ck.get_device_optimizer(model, lr=5e-3, weight_average=dict(decay=0.5))
    xt, yt = _clips(8, 5)
    xv, yv = _clips(6, 7)
    loop = train.EpochLoop(model, opt, None, batch_size=4, example=(xt[:4], yt[:4]), num_classes=NC, eval_averaged=True)
    book = loop.run(_batches(xt, yt, 4), _batches(xv, yv, 4), epochs=0)
    assert not opt.averager.is_applied and [len(v) for v in book.lists] == [1] * 4
    model.eval()
    ev = evaluate.Evaluator(model, NC, xv[:4], k_max=1)
    seen = {}
    for name in ("live", "averaged"):
        ev.reset()
        with (opt.averager.applied() if name == "averaged" else torch.no_grad()):
            for xb, yb in _batches(xv, yv, 4):
                ev.update(xb, yb)
            seen[name] = ev.result()["loss"]
    print(f"val loss {book.val_loss_list[0]!r}; separate passes {seen}")
    assert book.val_loss_list[0] == seen["averaged"] != seen["live"]


def test_epoch_loop_end_to_end(tmp_path):
    """10 train clips (on the CPU: the loop copies them) and 6 validation clips at batch size 4, epochs=2: three epochs"""
    model = _hwgate(torch.float32)
    opt = ck.get_device_optimizer(model, lr=5e-4, max_grad_norm=1.0, on_nonfinite="skip", weight_average={})
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20)
    xt, yt = _clips(10, 5, device="cpu")
    xv, yv = _clips(6, 7)
    prefix = str(tmp_path / "run")
    loop = train.EpochLoop(model, opt, sched, batch_size=4, example=(xt[:4], yt[:4]), num_classes=NC, out_prefix=prefix,
                           save_interval=1, lr=5e-4)
    book = loop.run(_batches(xt, yt, 4), _batches(xv, yv, 4), epochs=2)
    assert book is loop.book and all(len(v) == 3 for v in book.lists) and loop.start_epoch == 3
    assert sched.last_epoch == 3
    hist = loop.meter.history()
    assert len(hist) == 3 and all((h["steps"], h["rows"]) == (3, 10) for h in hist)
    assert book.train_loss_list == [h["loss"] for h in hist] and book.train_acc_list == [h["acc"] for h in hist]
    assert all(math.isfinite(v) for v in book.train_loss_list + book.val_loss_list)
    # the last epoch's validation numbers: a separate evaluator over the final weights
    model.eval()
    ev = evaluate.Evaluator(model, NC, xv[:4], k_max=1)
    ev.reset()
    for xb, yb in _batches(xv, yv, 4):
        ev.update(xb, yb)
    r = ev.result()
    print(f"val loss {book.val_loss_list} acc {book.val_acc_list}; separate pass {r['loss']!r} {r['acc'][1]!r}")
    assert (book.val_loss_list[-1], book.val_acc_list[-1]) == (r["loss"], r["acc"][1])
    # the files: what the bookkeeping rules give for the recorded numbers
    replay, want = train.EpochBook(save_interval=1), []
    for e in range(3):
        suffixes, _ = replay.record(e, book.train_loss_list[e], book.train_acc_list[e], book.val_loss_list[e],
                                    book.val_acc_list[e])
        want += [f"{prefix}_{s}.pt" for s in suffixes]
    assert loop.written == want and f"{prefix}_1.pt" in want and f"{prefix}_2.pt" in want and f"{prefix}_0.pt" not in want
    assert sorted(os.listdir(tmp_path)) == sorted({os.path.basename(p) for p in want})
    for path in set(want):
        raw = torch.load(path, map_location="cpu", weights_only=True)
        assert set(raw) == NINE | {"extra"} and raw["learning_rate"] == 5e-4
        assert set(raw["extra"]) == {"guard", "averager", "meter", "drop_calls"}
        n = raw["epoch"] + 1
        assert [len(raw[k]) for k in ("train_loss_list", "val_loss_list", "train_acc_list", "val_acc_list")] == [n] * 4
        assert raw["extra"]["guard"]["steps"] == 3 * n and raw["extra"]["averager"]["steps_seen"] == 3 * n
        assert raw["extra"]["meter"]["head"][train.METER_CLOSED] == n
    last = torch.load(f"{prefix}_2.pt", map_location="cpu", weights_only=True)
    assert last["epoch"] == 2 and last["val_loss_list"] == book.val_loss_list
    assert last["extra"]["drop_calls"] == model._drop_calls


def _stgcn(seed):
    cfg = SH.CONFIGS["a"]
    torch.manual_seed(seed)
    model = hw.STGCNModel(*SH.model_args(cfg, 0.0)).to(DEV)
    model.deterministic_train = True
    opt = optim.DeviceAdamW(list(model.parameters()), lr=1e-3)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=20)
    return model, opt, sched


def test_resumed_run_repeats_the_uninterrupted_one(tmp_path):
    """ST-GCN without dropout draws nothing and has no float atomics: epochs 0..3 in one piece, and epochs 0..1, a
    checkpoint, fresh objects, resume, epochs 2..3 must give the same four lists and the same weights and statistics"""
    cfg = SH.CONFIGS["a"]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(8, cfg["T"], cfg["V"], cfg["C"], generator=g).to(DEV)
    y = torch.randint(0, cfg["nclass"], (8,), generator=g).to(DEV)
    tr, va = _batches(x, y, 4), _batches(x.flip(0), y.flip(0), 4)
    kw = dict(batch_size=4, example=(x[:4], y[:4]), num_classes=cfg["nclass"], save_interval=1)

    model_a, opt_a, sched_a = _stgcn(3)
    one = train.EpochLoop(model_a, opt_a, sched_a, **kw)
    assert one.padded is False
    one.run(tr, va, epochs=3)

    model_b, opt_b, sched_b = _stgcn(3)
    first = train.EpochLoop(model_b, opt_b, sched_b, out_prefix=str(tmp_path / "half"), **kw)
    first.run(tr, va, epochs=1)
    assert first.book.lists == [v[:2] for v in one.book.lists]
    del first

    model_c, opt_c, sched_c = _stgcn(4)                       # other initial weights: everything must come from the file
    second = train.EpochLoop(model_c, opt_c, sched_c, **kw)
    assert second.resume(str(tmp_path / "half_1.pt")) == 2
    assert second.book.lists == [v[:2] for v in one.book.lists]
    assert second.book.best_val_loss == min(one.book.val_loss_list[:2])
    second.run(tr, va, epochs=3)
    print(f"one piece {one.book.lists}\nresumed   {second.book.lists}")
    assert second.book.lists == one.book.lists and all(len(v) == 4 for v in one.book.lists)
    sa, sc = model_a.state_dict(), model_c.state_dict()
    assert sa.keys() == sc.keys() and all(torch.equal(sa[k], sc[k]) for k in sa)
    assert sched_c.last_epoch == sched_a.last_epoch == 4
    assert [h["loss_sum"] for h in second.meter.history()] == [h["loss_sum"] for h in one.meter.history()]
    with pytest.raises(ValueError, match="drop_last"):
        second.run([(x[:3], y[:3])], va, epochs=5)


class _ScriptedEvaluator:
    """stands in for evaluate.Evaluator: the validation accuracy of epoch e is accs[e]"""

    def __init__(self, accs):
        self.accs, self.epoch, self.batches = accs, -1, 0

    def reset(self):
        self.epoch += 1
        self.batches = 0

    def update(self, x, y):
        assert x.is_cuda and y.is_cuda
        self.batches += 1

    def result(self):
        return {"loss": 2.0 - 0.1 * self.epoch, "acc": {1: self.accs[self.epoch]}}


def test_the_loop_ends_where_the_early_stopper_says():
    """patience 1: [0.5, 0.5, 0.25] answers [False, False, True] (the table of tests/test_train_meter_cpu.py: a tie does
    not count, a fall does), so a run asked for six epochs ends after its third.  The eager step: TrainStep(pad_to=4)"""
    model = _hwgate(torch.float32)
    opt = optim.DeviceAdamW(list(model.parameters()), lr=5e-4)
    x, y = _clips(6, 9)
    ev = _ScriptedEvaluator([0.5, 0.5, 0.25, 0.9, 0.9, 0.9])
    loop = train.EpochLoop(model, opt, None, batch_size=4, example=(x[:4], y[:4]), num_classes=NC, graph=False,
                           early_stopper=train.EarlyStopper(patience=1), evaluator=ev)
    book = loop.run(_batches(x, y, 4), _batches(x, y, 4), epochs=5)
    assert isinstance(loop.step, train.TrainStep) and loop.step.pad_to == 4
    assert book.val_acc_list == [0.5, 0.5, 0.25] and book.val_loss_list == [2.0 - 0.1 * e for e in range(3)] and ev.batches == 2
    assert len(book.train_loss_list) == 3 and loop.start_epoch == 3 and loop.written == []
    hist = loop.meter.history()
    assert len(hist) == 3 and all((h["steps"], h["rows"]) == (2, 6) for h in hist)
