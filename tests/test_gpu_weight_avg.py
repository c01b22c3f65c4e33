"""optim.WeightAverage on the device (csrc/weight_avg.hip): the update and swap kernels on seated synthetic tensors, the
state machine of the advance kernel against its closed forms, 20 training steps against
torch.optim.swa_utils.AveragedModel on the CPU in float64, the averager inside the graph of train.GraphedTrainStep (with a
GradGuard that skips, with micro-batches), the averaged weights swapped in under a captured serve.GraphedEval, BatchNorm
running statistics, and the averager's two state dicts.

Bounds.  One update is  a' = fma((float)coef, p - a, a)  in fp32: the subtraction, the coefficient's conversion and the
fused multiply-add each round once, each at 2^-24 of a quantity of at most 2 max(|a|, |p|) (coef <= 1), so against
a'_64 = a + coef (p - a) in fp64 from the same fp32 inputs and the device's own COEF word
    |a' - a'_64| <= 2^-21 max(|a|, |p|)                       per entry (the three roundings stay below 7 * 2^-24).
Over n updates the error of step k is carried on by factors 1 - coef <= 1, so per tensor
    max |a - a_64| <= n 2^-21 M,      M = the largest magnitude among the tensor's weights and averages over the run.
The counters and the coefficient are fp64 words computed by the formulas the test restates with the same IEEE operations:
they are compared for equality.

Measured on an MI355X (this file's own print-out): one update, largest |a' - a'_64| over its bound 0.124 - 0.129 on the
size list and 0.125 - 0.148 on the 300-entry list, the same whatever the seating; 20 training updates of 101 tensors,
largest max |a - a_64| over its bound: HWGATE EMA 0.0299, equal weight 0.0366, HGATE 0.0308 and 0.0353; the 46 running
statistics of ST-GCN over 3 updates 0.0643."""
import importlib

import pytest
import torch

from test_gpu_graph import _batch, _build
from test_gpu_grad_guard import _intact, _same_bits, _seat_at

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
optim = importlib.import_module("sl-hwgat_amd.optim")
train = importlib.import_module("sl-hwgat_amd.train")
serve = importlib.import_module("sl-hwgat_amd.serve")
ck = hw.checkpoint
call, ptr, stream = hw._lib.call, hw._lib.ptr, hw._lib.stream
DEV = torch.device("cuda:0")
CHUNK = optim.CHUNK
SIZES = (1, 3, 4, 5, 255, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
MANY = tuple(1 + (37 * i) % CHUNK for i in range(299)) + (CHUNK,)          # 300 single-chunk entries: the binary search
LISTS = {"sizes": SIZES, "many": MANY}
# (avg, src) element offsets of tensor i inside its buffer: both 16-byte aligned; every pair of different misalignments
SEATINGS = {"aligned": lambda i: (4, 0), "mixed": lambda i: (i % 4, (i % 4 + 1 + (i // 4) % 3) % 4)}
EPS = 2.0 ** -21
EMA, SWA = 0, 1


# ------------------------------------------------------------------------------------------ kernel level
def _values(sizes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in sizes]


class _Lab:
    """avg and src tensors seated in sentinel-filled buffers, a hand-packed table and a zeroed state block"""

    def __init__(self, sizes, seating, avg_values, src_values):
        offs = [SEATINGS[seating](i) for i in range(len(sizes))]
        self.ab, self.avg = _seat_at(avg_values, [o[0] for o in offs])
        self.sb, self.src = _seat_at(src_values, [o[1] for o in offs])
        blob, total = bytearray(), 0
        for a, s in zip(self.avg, self.src):
            blob += optim.WAVG_ENTRY.pack(a.data_ptr(), s.data_ptr(), a.numel(), total, 0)
            total += -(-a.numel() // CHUNK)
        self.table = torch.frombuffer(blob, dtype=torch.uint8).to(DEV)
        self.n, self.total = len(sizes), total
        self.state = torch.zeros(optim.WAVG_NSTATE, dtype=torch.float64, device=DEV)

    def set(self, mode=EMA, decay=0.9, warmup=0, start=0, every=1):
        call("hwgat_wavg_set", ptr(self.state), mode, decay, warmup, start, every, stream())

    def step(self, guard=None):
        call("hwgat_wavg_advance", ptr(self.state), None if guard is None else ptr(guard), stream())
        call("hwgat_wavg_update", ptr(self.table), self.n, ptr(self.state), self.total, stream())

    def swap(self):
        call("hwgat_wavg_swap", ptr(self.table), self.n, self.total, stream())

    def words(self):
        """(steps_seen, n_averaged, coef, active)"""
        return tuple(self.state[optim.W_STEPS_SEEN:optim.W_ACTIVE + 1].tolist())

    def put_src(self, values):
        for s, v in zip(self.src, values):
            s.copy_(v)

    def buffers(self, which):
        return [b[0].clone() for b in (self.ab if which == "avg" else self.sb)]

    def intact(self):
        torch.cuda.synchronize()
        _intact(dict(avg=self.ab, src=self.sb))


def _all_same_bits(xs, ys):
    return len(xs) == len(ys) and all(_same_bits(x.cpu(), y.cpu()) for x, y in zip(xs, ys))


@pytest.mark.parametrize("seating", list(SEATINGS))
@pytest.mark.parametrize("which", list(LISTS))
def test_first_update_copies_the_bits_of_src(which, seating):
    sizes = LISTS[which]
    src = _values(sizes, 5)
    src[-1][0], src[-1][-1] = float("nan"), -0.0             # the same bits, not the same values
    if sizes[4] > 8:
        src[4][3], src[4][-2] = float("inf"), -0.0
    lab = _Lab(sizes, seating, _values(sizes, 6), src)
    lab.set()
    assert lab.words() == (0.0, 0.0, 0.0, 0.0)
    before = lab.buffers("src")
    lab.step()
    assert lab.words() == (1.0, 1.0, 1.0, 1.0)
    assert _all_same_bits(lab.avg, src) and _all_same_bits(lab.src, src)
    assert _all_same_bits(lab.buffers("src"), before)        # update never writes src
    lab.intact()


@pytest.mark.parametrize("seating", list(SEATINGS))
def test_an_inactive_update_writes_nothing(seating):
    """before `start`, off the `every` period, and under a gradient guard's skip word"""
    a0, p0 = _values(SIZES, 7), _values(SIZES, 8)
    lab = _Lab(SIZES, seating, a0, p0)
    keep = (lab.buffers("avg"), lab.buffers("src"))

    def untouched():
        return _all_same_bits(lab.buffers("avg"), keep[0]) and _all_same_bits(lab.buffers("src"), keep[1])

    lab.set(start=3, every=2)
    for seen in (1, 2, 3, 4):                                # 1..3: not past start; 4: (4 - 3) % 2 == 1
        lab.step()
        assert lab.words() == (float(seen), 0.0, 0.0, 0.0) and untouched(), seen
    guard = torch.zeros(optim.GUARD_NSTATE, dtype=torch.float64, device=DEV)
    guard[optim.G_SKIP] = 1.0
    lab.step(guard)                                          # would have been due (5 - 3 = 2): the step did not happen
    assert lab.words() == (4.0, 0.0, 0.0, 0.0) and untouched()
    guard[optim.G_SKIP] = 0.0
    lab.step(guard)
    assert lab.words() == (5.0, 1.0, 1.0, 1.0)
    assert _all_same_bits(lab.avg, p0) and _all_same_bits(lab.buffers("src"), keep[1])
    keep = (lab.buffers("avg"), keep[1])
    guard[optim.G_SKIP] = 1.0
    lab.step(guard)                                          # after an active step: COEF and ACTIVE are rewritten
    assert lab.words() == (5.0, 1.0, 0.0, 0.0) and untouched()
    lab.intact()


def _check_update(lab, a_before, p, what):
    """the seated averages against fp64 from the same fp32 inputs and the device's COEF word; returns the worst ratio"""
    coef = lab.words()[2]
    worst = 0.0
    for i, (got, a, q) in enumerate(zip(lab.avg, a_before, p)):
        a, q = a.double(), q.double()
        want = a + coef * (q - a)
        err = (got.cpu().double() - want).abs()
        bound = EPS * torch.maximum(a.abs(), q.abs())
        assert bool((err <= bound).all()), (what, i, float((err / bound.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


@pytest.mark.parametrize("mode", [EMA, SWA], ids=["ema", "swa"])
@pytest.mark.parametrize("seating", list(SEATINGS))
@pytest.mark.parametrize("which", list(LISTS))
def test_general_update_against_float64(which, seating, mode):
    sizes = LISTS[which]
    lab = _Lab(sizes, seating, _values(sizes, 9), _values(sizes, 10))
    lab.set(mode=mode, decay=0.9)
    lab.step()                                               # the copy
    worst = 0.0
    for k, scale in enumerate((1.0, 1e-3, 1e3, 1.0)):        # weights far below and far above the average
        p = _values(sizes, 20 + k, scale)
        if k == 3:
            for t in p:
                t[::2] = 0
        lab.put_src(p)
        a_before = [a.cpu().clone() for a in lab.avg]
        src_before = lab.buffers("src")
        lab.step()
        seen, n, coef, active = lab.words()
        assert (seen, n, active) == (k + 2.0, k + 2.0, 1.0)
        assert coef == (1.0 - 0.9 if mode == EMA else 1.0 / (k + 2.0))
        worst = max(worst, _check_update(lab, a_before, p, (which, seating, mode, k)))
        assert _all_same_bits(lab.buffers("src"), src_before)
        assert any(not _same_bits(a.cpu(), b) for a, b in zip(lab.avg, a_before))
    print(f"update {which} {seating} mode {mode}: largest |a' - a'_64| / bound {worst:.3f}")
    lab.intact()


def test_same_bits_whatever_the_seating():
    """the vector path, the element path and the tails give an element the same bits"""
    runs = []
    for seating in SEATINGS:
        lab = _Lab(SIZES, seating, _values(SIZES, 9), _values(SIZES, 10))
        lab.set(decay=0.75)
        lab.step()
        for k in range(3):
            lab.put_src(_values(SIZES, 30 + k))
            lab.step()
        runs.append([a.clone() for a in lab.avg])
    assert _all_same_bits(runs[0], runs[1])


def _machine(mode, decay, warmup, start, every, skips, steps):
    """the advance kernel restated: [(steps_seen, n_averaged, coef, active)] after each step"""
    seen = n = 0
    coef, out = 0.0, []
    for k in range(steps):
        if k in skips:
            coef, active = 0.0, 0.0
        else:
            seen += 1
            active = float(seen > start and (seen - start) % every == 0)
            if active:
                if n == 0:
                    coef = 1.0
                elif mode == EMA:
                    coef = 1.0 - (min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay)
                else:
                    coef = 1.0 / (n + 1.0)
                n += 1
        out.append((float(seen), float(n), coef, active))
    return out


MACHINES = {"ema": dict(mode=EMA, decay=0.999, warmup=0, start=0, every=1),
            "ema-warmup": dict(mode=EMA, decay=0.999, warmup=1, start=0, every=1),
            "ema-warmup-low-decay": dict(mode=EMA, decay=0.3, warmup=1, start=1, every=2),
            "swa-start2-every3": dict(mode=SWA, decay=0.9, warmup=0, start=2, every=3)}


@pytest.mark.parametrize("skips", [(), (0, 4, 5, 10)], ids=["every-step-counts", "skipped-steps-do-not"])
@pytest.mark.parametrize("name", list(MACHINES))
def test_counters_and_coefficient_equal_the_closed_forms(name, skips):
    cfg, steps = MACHINES[name], 12 + len(skips)
    sizes = (5, CHUNK + 1)
    lab = _Lab(sizes, "mixed", _values(sizes, 1), _values(sizes, 2))
    lab.set(**cfg)
    guard = torch.zeros(optim.GUARD_NSTATE, dtype=torch.float64, device=DEV)
    want = _machine(skips=skips, steps=steps, **cfg)
    for k in range(steps):
        guard[optim.G_SKIP] = float(k in skips)
        before = [a.clone() for a in lab.avg]
        lab.step(guard)
        assert lab.words() == want[k], (name, k, lab.words(), want[k])
        if want[k][3] == 0.0:
            assert _all_same_bits(lab.avg, before), (name, k)
    assert want[-1][0] == 12.0                               # twelve steps that counted
    if name == "swa-start2-every3":
        assert [w[1] for w in want if w[3]] == [1.0, 2.0, 3.0] and want[-1][2] in (1.0 / 3.0, 0.0)
        assert sorted({w[0] for w in want if w[3]}) == [5.0, 8.0, 11.0]
    lab.intact()


@pytest.mark.parametrize("seating", list(SEATINGS))
@pytest.mark.parametrize("which", list(LISTS))
def test_swap_exchanges_exactly_and_twice_is_the_identity(which, seating):
    sizes = LISTS[which]
    a0, p0 = _values(sizes, 3), _values(sizes, 4)
    a0[-1][0], p0[0][0] = float("nan"), -0.0
    lab = _Lab(sizes, seating, a0, p0)
    keep = (lab.buffers("avg"), lab.buffers("src"))
    lab.swap()
    assert _all_same_bits(lab.avg, p0) and _all_same_bits(lab.src, a0)
    lab.intact()
    lab.swap()
    assert _all_same_bits(lab.buffers("avg"), keep[0]) and _all_same_bits(lab.buffers("src"), keep[1])
    assert not bool(lab.state.any())                         # swap has no state
    lab.intact()


# ------------------------------------------------------------------------------------------ against torch
class _Holder(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


@pytest.mark.parametrize("mode", ["ema", "swa"])
@pytest.mark.parametrize("kind", ["hwgate", "hgate"])
def test_training_follows_averaged_model_in_float64(kind, mode):
    """20 eager DeviceAdamW steps; the weights of every step are downloaded and fed to AveragedModel in float64"""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    steps = 20
    m = _build(torch.float32, kind)
    x, y = _batch(m)
    o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
    avg = o.averager = optim.WeightAverage(m, mode=mode, decay=0.9)
    step = train.TrainStep(m, o, None)
    holder = _Holder([p.detach().cpu().double() for p in m.parameters()])
    ref = AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(0.9)) if mode == "ema" else AveragedModel(holder)
    M = [torch.zeros((), dtype=torch.float64) for _ in holder.ps]
    for k in range(steps):
        step(x, y)
        with torch.no_grad():
            for i, (h, p) in enumerate(zip(holder.ps, m.parameters())):
                h.copy_(p.detach().cpu().double())
        ref.update_parameters(holder)
        for i, (h, a) in enumerate(zip(holder.ps, ref.module.ps)):
            M[i] = torch.maximum(M[i], torch.maximum(h.detach().abs().max(), a.detach().abs().max()))
    assert avg.counters() == dict(steps_seen=steps, n_averaged=steps) and int(ref.n_averaged) == steps
    assert float(avg.coef) == (1.0 - 0.9 if mode == "ema" else 1.0 / steps)
    worst = 0.0
    for i, (s, a) in enumerate(zip(avg._shadow, ref.module.ps)):
        err = float((s.cpu().double() - a.detach()).abs().max())
        bound = steps * EPS * float(M[i])
        worst = max(worst, err / bound)
        assert err <= bound, (kind, mode, avg.keys()[i], err, bound)
    assert any(not torch.equal(s, p.detach()) for s, p in zip(avg._shadow, m.parameters()))    # an average, not a copy
    print(f"{kind} {mode}: {steps} updates of {len(avg._shadow)} tensors, largest max |a - a_64| / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------ in the graph
GRAPHED = [("hgate", torch.bfloat16), ("hwgate", torch.float32)]
C0 = 17


def _fresh(kind, dtype, guard=None, **kw):
    m = _build(dtype, kind)
    m.deterministic_train = True
    m._drop_calls = C0
    o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
    o.guard = guard
    o.averager = optim.WeightAverage(m, **dict(dict(decay=0.9), **kw))
    return m, o, o.averager, _batch(m)


def _result_words(avg):
    return avg._state[optim.W_STEPS_SEEN:optim.W_ACTIVE + 1].clone()


@pytest.mark.parametrize("kind, dtype", GRAPHED, ids=["hgate-bf16", "hwgate-fp32"])
def test_averager_inside_the_graph_equals_the_eager_step(kind, dtype):
    k = 4
    runs = []
    for graphed in (False, True):
        m, o, avg, (x, y) = _fresh(kind, dtype)
        initial = [p.detach().clone() for p in m.parameters()]
        if graphed:
            s = train.GraphedTrainStep(m, o, x, y)
            assert s.in_graph
            # the warm-up stepped and averaged; nothing of it is left
            assert float(avg.n_averaged) == 0.0 and float(avg.steps_seen) == 0.0 and not bool(_result_words(avg).any())
            assert all(torch.equal(a, b) for a, b in zip(avg._shadow, initial))
            assert all(torch.equal(p.detach(), b) for p, b in zip(m.parameters(), initial))
        else:
            s = train.TrainStep(m, o, None)
        for _ in range(k):
            s(x, y)
        runs.append((m, o, avg, s, x, y))
    (me, _, ae, _, _, _), (mg, og, ag, s, x, y) = runs
    assert all(torch.equal(p, q) for p, q in zip(me.parameters(), mg.parameters()))
    assert len(ae._shadow) == len(ag._shadow) and all(torch.equal(a, b) for a, b in zip(ae._shadow, ag._shadow))
    assert torch.equal(_result_words(ae), _result_words(ag))
    assert _result_words(ag).tolist() == [float(k), float(k), 1.0 - 0.9, 1.0]
    assert any(not torch.equal(a, p.detach()) for a, p in zip(ag._shadow, mg.parameters()))
    # a new decay reaches the next replay of the same graph
    graph = s.graph
    for avg, step in ((ae, runs[0][3]), (ag, s)):
        avg.decay = 0.5
        step(x, y)
        assert float(avg.coef) == 0.5 and float(avg.n_averaged) == k + 1.0
    assert s.graph is graph
    assert all(torch.equal(a, b) for a, b in zip(ae._shadow, ag._shadow))


@pytest.mark.parametrize("micro_batch", [None, 4], ids=["whole", "micro4"])
@pytest.mark.parametrize("kind, dtype", GRAPHED, ids=["hgate-bf16", "hwgate-fp32"])
def test_a_skipped_replay_is_not_averaged_in(kind, dtype, micro_batch):
    guard = optim.GradGuard(on_nonfinite="skip")
    m, o, avg, (x, y) = _fresh(kind, dtype, guard=guard)
    s = train.GraphedTrainStep(m, o, x, y, micro_batch=micro_batch)
    assert s.n_slices == (2 if micro_batch else 1)
    for r in (1, 2):                                         # once per replay, not once per slice
        s(x, y)
        assert avg.counters() == dict(steps_seen=r, n_averaged=r)
    bad = x.clone()
    bad[-1, 0, 0, 0] = float("nan")                          # in the last slice
    keep = ([p.detach().clone() for p in m.parameters()], [a.clone() for a in avg._shadow], _result_words(avg))
    s(bad, y)
    assert guard.counters()["skipped"] == 1 and float(guard.nonfinite) == 1.0
    assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), keep[0]))
    assert all(torch.equal(a, q) for a, q in zip(avg._shadow, keep[1]))
    assert avg.counters() == dict(steps_seen=2, n_averaged=2)
    assert _result_words(avg).tolist() == [2.0, 2.0, 0.0, 0.0]
    s(x, y)                                                  # the next clean replay averages again
    assert guard.counters()["skipped"] == 1 and float(guard.nonfinite) == 0.0
    assert avg.counters() == dict(steps_seen=3, n_averaged=3) and float(avg.coef) == 1.0 - 0.9
    assert any(not torch.equal(a, q) for a, q in zip(avg._shadow, keep[1]))
    assert all(bool(torch.isfinite(a).all()) for a in avg._shadow)


# ------------------------------------------------------------------------------------------ applied
def test_applied_swaps_the_averages_in_under_captured_graphs():
    m, o, avg, (x, y) = _fresh("hwgate", torch.float32)
    m.eval()
    ge = serve.GraphedEval(m, x)                             # captured on the live weights, before any training
    m.train()
    s = train.GraphedTrainStep(m, o, x, y)
    for _ in range(3):
        s(x, y)
    m.eval()
    file = avg.model_state_dict()
    second = _build(torch.float32, "hwgate").eval()
    second.load_state_dict(file)
    with torch.no_grad():
        live_out, avg_out = m(x), second(x)
    assert not torch.equal(live_out, avg_out)
    live = [p.detach().clone() for p in m.parameters()]
    assert not avg.is_applied
    with avg.applied() as inside:
        assert inside is avg and avg.is_applied
        assert torch.equal(ge(x), avg_out)
        assert all(torch.equal(p.detach(), file[k]) for k, p in m.named_parameters())
        again = avg.model_state_dict()                       # the averaged values, wherever they are at the moment
        assert all(torch.equal(again[k], file[k]) for k in file)
        ge.check()
        assert s._addresses() == s._addr
        with pytest.raises(RuntimeError, match="swapped in"):
            o.step()
        with pytest.raises(RuntimeError, match="swapped in"):
            avg.update()
        with pytest.raises(RuntimeError, match="swapped in"):
            with avg.applied():
                pass
        m.train()
        with pytest.raises(RuntimeError, match="swapped in"):
            s(x, y)
        m.eval()
        assert avg.is_applied and avg.counters() == dict(steps_seen=3, n_averaged=3)
    assert not avg.is_applied
    assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), live))
    assert torch.equal(ge(x), live_out)
    ge.check()
    assert s._addresses() == s._addr
    with pytest.raises(KeyError):                            # swapped back on an exception as well
        with avg.applied():
            raise KeyError("body")
    assert not avg.is_applied and all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), live))
    m.train()
    s(x, y)                                                  # and training goes on
    assert avg.counters() == dict(steps_seen=4, n_averaged=4)


# ------------------------------------------------------------------------------------------ BatchNorm buffers
def _stgcn(buffers, graphed):
    import stgcn_helpers as SH
    from test_gpu_stgcn import _model
    cfg = SH.CONFIGS["a"]
    x, y = (t.to(DEV) for t in SH.make_input(cfg))
    assert x.shape[0] == 2 and 16 in x.shape                 # B 2, T 16
    m = _model("a", dropout=0.05)[0].train()
    o = optim.DeviceAdamW(list(m.parameters()), lr=3e-4)
    avg = o.averager = optim.WeightAverage(m, decay=0.9, buffers=buffers)
    torch.manual_seed(5)
    s = train.GraphedTrainStep(m, o, x, y) if graphed else train.TrainStep(m, o)
    return m, o, avg, s, x, y


def test_batchnorm_running_statistics_are_averaged():
    steps = 3
    m, o, avg, s, x, y = _stgcn(True, False)
    stats = [k for k in avg.keys() if k.endswith(("running_mean", "running_var"))]
    assert len(stats) >= 4 and len(stats) == len(avg.keys()) - len(list(m.parameters()))
    ref, M = {}, {}
    counts0 = {k: int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    for k in range(steps):
        s(x, y)
        sd = m.state_dict()
        coef = 1.0 if k == 0 else 1.0 - 0.9
        for name in stats:
            p = sd[name].cpu().double()
            ref[name] = p.clone() if k == 0 else ref[name] + coef * (p - ref[name])
            M[name] = max(M.get(name, 0.0), float(p.abs().max()), float(ref[name].abs().max()))
    got = avg.model_state_dict()
    worst = 0.0
    for name in stats:
        err, bound = float((got[name].cpu().double() - ref[name]).abs().max()), steps * EPS * M[name]
        worst = max(worst, err / bound)
        assert err <= bound, (name, err, bound)
        assert not torch.equal(got[name], m.state_dict()[name]), name       # an average, not the live value
    print(f"ST-GCN a: {len(stats)} running statistics over {steps} updates, largest max |a - a_64| / bound {worst:.4f}")
    counts = {k: v.clone() for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")}
    assert counts and all(int(v) == counts0[k] + steps for k, v in counts.items())   # the model's own count, never the averager's
    with avg.applied():
        now = m.state_dict()
        assert all(torch.equal(now[k], v) for k, v in counts.items())
        assert all(torch.equal(now[name], got[name]) for name in stats)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in counts.items())
    assert all(torch.equal(got[k], v) for k, v in counts.items())

    # the graphed step agrees bit for bit, running statistics and their averages included
    mg, og, ag, sg, x, y = _stgcn(True, True)
    assert float(ag.n_averaged) == 0.0
    for _ in range(steps):
        sg(x, y)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), mg.state_dict().values()))
    assert ag.keys() == avg.keys() and all(torch.equal(a, b) for a, b in zip(avg._shadow, ag._shadow))
    assert torch.equal(_result_words(avg), _result_words(ag))


def test_without_buffers_the_running_statistics_stay_the_live_ones():
    m, o, avg, s, x, y = _stgcn(False, False)
    for _ in range(3):
        s(x, y)
    assert avg.keys() == [n for n, _ in m.named_parameters()]
    live = {k: v.clone() for k, v in m.state_dict().items()}
    stats = [k for k in live if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    file = avg.model_state_dict()
    with avg.applied():
        now = m.state_dict()
        assert all(torch.equal(now[k], live[k]) for k in stats)
        assert any(not torch.equal(now[k], live[k]) for k in avg.keys())
    assert all(torch.equal(file[k], live[k]) for k in stats)
    assert all(torch.equal(v, live[k]) for k, v in m.state_dict().items())


# ------------------------------------------------------------------------------------------ checkpoint
def test_state_dict_round_trip_and_the_averaged_weights_file(tmp_path):
    m, o, avg, (x, y) = _fresh("hwgate", torch.float32, warmup=True, start=1)
    step = train.TrainStep(m, o, None)
    for _ in range(3):
        step(x, y)
    torch.save(avg.state_dict(), tmp_path / "avg.pt")
    loaded = torch.load(tmp_path / "avg.pt", weights_only=True)
    assert loaded["steps_seen"] == 3 and loaded["n_averaged"] == 2
    others = []
    for launched in (False, True):
        m2 = _build(torch.float32, "hwgate")
        m2.load_state_dict(m.state_dict())
        a2 = optim.WeightAverage(m2)
        if launched:                                         # one update of its own first: the device block exists
            a2.update()
            assert a2.counters() == dict(steps_seen=1, n_averaged=1)
        addresses = [t.data_ptr() for t in a2._shadow]
        a2.load_state_dict(loaded)
        assert (a2.mode, a2.decay, a2.warmup, a2.start, a2.every) == ("ema", 0.9, True, 1, 1)
        assert a2.counters() == dict(steps_seen=3, n_averaged=2)
        assert all(torch.equal(a, b) for a, b in zip(a2._shadow, avg._shadow))
        others.append((a2, addresses))
    avg.update()
    want = _machine(EMA, 0.9, 1, 1, 1, (), 4)[-1]
    assert tuple(_result_words(avg).tolist()) == want and want[1] == 3.0
    for a2, addresses in others:
        a2.update()
        assert [t.data_ptr() for t in a2._shadow] == addresses
        assert torch.equal(_result_words(a2), _result_words(avg))
        assert all(torch.equal(a, b) for a, b in zip(a2._shadow, avg._shadow))
    # the averaged weights as a weights file
    torch.save({"model_state_dict": avg.model_state_dict()}, tmp_path / "averaged.pt")
    report = {}
    fresh = ck.load_weights_from_pretrained(_build(torch.float32, "hwgate"), str(tmp_path / "averaged.pt"), device=DEV,
                                            report=report)
    assert report == dict(unknown=[], mismatched=[], missing=[])
    assert all(torch.equal(p.detach(), a) for p, a in zip(fresh.parameters(), avg._shadow))
