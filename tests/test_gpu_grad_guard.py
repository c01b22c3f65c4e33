"""optim.GradGuard on the device (csrc/grad_guard.hip): the global gradient norm, torch's clip coefficient, the in-place
scaling, the "skip" of a step with non-finite gradients in all three device optimizers, and the guard inside the graph of
train.GraphedTrainStep.  Reference: torch.nn.utils.clip_grad_norm_ followed by torch's optimizer, on the CPU in float64.

Inputs, seating and the training bound are those of tests/test_gpu_optim.py:
    max |p - p_64| <= 4 max |p_torch32 - p_64| + 4 * 2^-24 max |p_64|      per tensor.
The guard's readouts are float64 words, so the norm is held to  |norm - norm_64| <= n 2^-52 norm_64  with n the number
of elements: g^2 is exact in fp64, a sum of n non-negative terms in any order is within (n - 1) 2^-53 of the exact one,
the square root halves that and rounds once more; norm_64 is the correctly rounded root of the exactly rounded sum
(math.fsum).  The inf-norm is a maximum of exactly converted values: equal.  A scaled gradient is held to
|g' - g coef_64| <= 3 * 2^-24 |g coef_64|: the coefficient rounded to fp32 (2^-24), the product rounded (2^-24), and the
device's fp64 coefficient against coef_64 (orders below).

Measured on an MI355X (this file's own print-out): norm error 0 to 2 units in the last place (2.8e-14 at 145.52 against
a bound of 6.9e-10), inf-norm equal; scale, largest error over the bound 0.45; training, largest max |p - p_64| over the
bound: AdamW 0.277, SGD with momentum 0.207, NAdam 0.223, the skip runs 0.208 - 0.217; 15 of the reference's 25 steps clip."""
import functools
import importlib
import math

import pytest
import torch

from test_gpu_graph import _batch, _build
from test_gpu_optim import PAD, SENTINEL, _inputs, _seat, _within_bound

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
optim = importlib.import_module("sl-hwgat_amd.optim")
train = importlib.import_module("sl-hwgat_amd.train")
DEV = torch.device("cuda:0")
CHUNK = optim.CHUNK
SIZES = (1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
MANY = (300 * CHUNK + 3, 257 * CHUNK + 1)   # more workgroups than the finish kernel has threads: its later rounds
STEPS, MAX_NORM = 25, 0.5
INF = math.inf
OPT = {"adamw": (optim.DeviceAdamW, torch.optim.AdamW, dict(lr=1e-3, weight_decay=0.01), ("exp_avg", "exp_avg_sq")),
       "sgd": (optim.DeviceSGD, torch.optim.SGD, dict(lr=1e-2, momentum=0.9, weight_decay=0.01), ("momentum_buffer",)),
       "nadam": (optim.DeviceNAdam, torch.optim.NAdam, dict(lr=1e-3, weight_decay=0.01), ("exp_avg", "exp_avg_sq"))}


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _seat_at(values, offsets):
    """tensor i as a view at element offset offsets[i] of its own sentinel-filled buffer, PAD sentinels after it"""
    bufs, views = [], []
    for t, off in zip(values, offsets):
        buf = torch.full((off + t.numel() + PAD,), SENTINEL, device=DEV)
        view = buf[off:off + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 * off) % 16
        bufs.append((buf, off, t.numel()))
        views.append(view)
    return bufs, views


def _intact(guards):
    for name, bufs in guards.items():
        for i, (buf, off, n) in enumerate(bufs):
            assert bool((buf[:off] == SENTINEL).all()), (name, i, "before")
            assert bool((buf[off + n:] == SENTINEL).all()) and buf.numel() == off + n + PAD, (name, i, "after")


def _norm64(gs, norm_type):
    flat = torch.cat([g.detach().cpu().double().flatten() for g in gs])
    if norm_type == INF:
        return float(flat.abs().max())
    return math.sqrt(math.fsum((flat * flat).tolist()))       # each square is exact; fsum rounds the exact sum once


def _coef64(norm, max_norm):
    c = max_norm / (norm + 1e-6)
    return c if c < 1.0 else 1.0


def _holders(views):
    """parameters whose gradients are the seated views"""
    ps = [torch.nn.Parameter(torch.empty_like(v)) for v in views]
    for p, v in zip(ps, views):
        p.grad = v
    return ps


@functools.lru_cache(maxsize=None)
def _values(sizes, scale, sparse):
    g = torch.Generator().manual_seed(11)
    out = [torch.randn(n, generator=g) * scale for n in sizes]
    if sparse:
        for t in out:
            t[::2] = 0
    return out


NORM_CASES = [(SIZES, 1.0, False), (SIZES, 1e-4, True), (SIZES, 1e2, False), (MANY, 1e-2, False)]


@pytest.mark.parametrize("norm_type", [2.0, INF], ids=["l2", "linf"])
@pytest.mark.parametrize("sizes, scale, sparse", NORM_CASES, ids=["unit", "small-sparse", "large", "many-blocks"])
def test_total_norm_against_float64(norm_type, sizes, scale, sparse):
    values = _values(sizes, scale, sparse)
    bufs, views = _seat(values)                              # odd tensors at a 4-byte offset: the element path
    guard = optim.GradGuard(norm_type=norm_type)             # max_norm inf: measures only
    got = optim.clip_grad_norm_(_holders(views), guard)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.data_ptr() == guard.total_norm.data_ptr()
    n, want = sum(sizes), _norm64(values, norm_type)
    err = abs(float(got) - want)
    bound = 0.0 if norm_type == INF else n * 2.0 ** -52 * want
    print(f"norm {norm_type} {sizes[0]}.. x {scale}: {float(got)!r} against {want!r}, err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float(guard.clip_coef) == 1.0 and float(guard.nonfinite) == 0.0
    for v, t in zip(views, values):                          # coefficient 1: multiplied all the same, same bits
        assert _same_bits(v.cpu(), t)
    assert guard.counters() == dict(steps=1, clipped=0, skipped=0)
    _intact(dict(g=bufs))


@pytest.mark.parametrize("norm_type", [2.0, INF], ids=["l2", "linf"])
def test_all_zero_gradients(norm_type):
    bufs, views = _seat([torch.zeros(n) for n in SIZES])
    guard = optim.GradGuard(max_norm=1.0, norm_type=norm_type, on_nonfinite="skip")
    optim.clip_grad_norm_(_holders(views), guard)
    assert float(guard.total_norm) == 0.0 and float(guard.clip_coef) == 1.0 and float(guard.nonfinite) == 0.0
    assert all(not bool(v.any()) and not bool(v.isnan().any()) for v in views)
    assert guard.counters() == dict(steps=1, clipped=0, skipped=0)
    _intact(dict(g=bufs))


@pytest.mark.parametrize("norm_type", [2.0, INF], ids=["l2", "linf"])
def test_same_bits_aligned_and_misaligned_and_repeated(norm_type):
    """the same values 16-byte aligned, at a 4-byte offset and at an 8-byte offset: equal norms, equal scaled gradients;
    and the same launches once more on the same inputs"""
    values = _values(SIZES, 1.0, False)
    want = _norm64(values, norm_type)
    runs = []
    for offs in ([4] * len(SIZES), [1] * len(SIZES), [2] * len(SIZES), [4] * len(SIZES)):
        bufs, views = _seat_at(values, offs)
        guard = optim.GradGuard(max_norm=0.5 * want, norm_type=norm_type)
        norm = optim.clip_grad_norm_(_holders(views), guard).clone()
        _intact(dict(g=bufs))
        assert guard.counters() == dict(steps=1, clipped=1, skipped=0)
        runs.append((norm, guard.clip_coef.clone(), [v.clone() for v in views]))
    for norm, coef, scaled in runs[1:]:
        assert torch.equal(norm, runs[0][0]) and torch.equal(coef, runs[0][1])
        for a, b in zip(scaled, runs[0][2]):
            assert torch.equal(a, b)
    assert any(not _same_bits(a.cpu(), t) for a, t in zip(runs[0][2], values))   # and they were scaled


@pytest.mark.parametrize("norm_type", [2.0, INF], ids=["l2", "linf"])
def test_scale_against_float64_and_the_threshold(norm_type):
    values = _values(SIZES, 1.0, False)
    norm = _norm64(values, norm_type)
    for max_norm in (0.37 * norm, 1e-3, 0.0):
        bufs, views = _seat(values)
        guard = optim.GradGuard(max_norm=max_norm, norm_type=norm_type)
        optim.clip_grad_norm_(_holders(views), guard)
        coef = _coef64(norm, max_norm)
        assert abs(float(guard.clip_coef) - coef) <= 2.0 ** -40 * coef
        worst = 0.0
        for v, t in zip(views, values):
            want = t.double() * coef
            err, tol = (v.cpu().double() - want).abs(), 3 * 2.0 ** -24 * want.abs()
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert bool((err <= tol).all())
        print(f"scale, norm {norm_type}, max_norm {max_norm:.4g}: coef {coef:.6g}, largest err / bound {worst:.3f}")
        assert guard.counters()["clipped"] == 1
        _intact(dict(g=bufs))
    # a norm just below max_norm: nothing changes and nothing is counted; just above: counted
    bufs, views = _seat(values)
    params = _holders(views)
    guard = optim.GradGuard(max_norm=(norm + 1e-6) * (1 + 1e-9), norm_type=norm_type)
    optim.clip_grad_norm_(params, guard)
    assert float(guard.clip_coef) == 1.0 and guard.counters() == dict(steps=1, clipped=0, skipped=0)
    assert all(_same_bits(v.cpu(), t) for v, t in zip(views, values))
    guard.max_norm = (norm + 1e-6) * (1 - 1e-9)              # a new value reaches the device with the next run
    optim.clip_grad_norm_(params, guard)
    assert float(guard.clip_coef) < 1.0 and guard.counters() == dict(steps=2, clipped=1, skipped=0)
    _intact(dict(g=bufs))


# ---- the three optimizers under a guard
def _cpu_run(name, dtype, max_norm, none_at=None):
    """clip_grad_norm_ + torch's optimizer on the CPU in `dtype`; every gradient is None at step `none_at`.  Returns the
    parameters as float64 and the number of steps whose coefficient was below 1"""
    _, like, kw, _ = OPT[name]
    p0, grads = _inputs(SIZES, STEPS)
    ps = [torch.nn.Parameter(p.to(dtype, copy=True)) for p in p0]          # a copy: the shared inputs are never written
    o = like(ps, **kw)
    s = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
    clipped = 0
    for k, gs in enumerate(grads):
        for p, g in zip(ps, gs):
            p.grad = None if k == none_at else g.to(dtype, copy=True)
        if k != none_at:
            total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            clipped += int(max_norm / (float(total) + 1e-6) < 1.0)
        o.step()
        s.step()
    return [p.detach().double() for p in ps], clipped


@functools.lru_cache(maxsize=None)
def _reference(name, none_at=None):
    """((p_64, clipped steps), p_torch32): computed once, shared, never written"""
    return _cpu_run(name, torch.float64, MAX_NORM, none_at), _cpu_run(name, torch.float32, MAX_NORM, none_at)[0]


def _everything(o, params, gv):
    """clones of every parameter, every state tensor and private word, every gradient"""
    return ([p.detach().clone() for p in params] + [t.clone() for p in params for t in o._live.get(p, {}).values()]
            + [g.clone() for g in gv])


def _device_run(name, guard, poison=None):
    """25 guarded steps on seated tensors; poison = (step, tensor, element, value) writes one bad gradient element, and
    that step is checked to have changed nothing"""
    cls, _, kw, arrays = OPT[name]
    p0, grads = _inputs(SIZES, STEPS)
    pb, pv = _seat(p0)
    gb, gv = _seat([torch.zeros(n) for n in SIZES])
    params = [torch.nn.Parameter(v) for v in pv]
    o = cls(params, **kw)
    o.guard = guard
    guards, seated = dict(p=pb, g=gb), {}
    for key in arrays:                                       # the state arrays seated by the caller, in guarded buffers
        guards[key], seated[key] = _seat([torch.zeros(n) for n in SIZES])
    for i, p in enumerate(params):
        st = {key: views[i] for key, views in seated.items()}
        if name != "sgd":
            st = dict(step=torch.zeros((), device=DEV), **st)
        if name == "nadam":
            st = dict(st, mu_product=torch.ones((), device=DEV))
        o.state[p] = st
    s = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
    for k in range(STEPS):
        for p, g, src in zip(params, gv, grads[k]):
            g.copy_(src)
            p.grad = g
        if poison is not None and k == poison[0]:
            gv[poison[1]][poison[2]] = poison[3]
            before, count = _everything(o, params, gv), guard.counters()
        o.step()
        if poison is not None and k == poison[0] and guard.on_nonfinite == "skip":
            after = _everything(o, params, gv)
            assert len(after) == len(before) and all(_same_bits(a, b) for a, b in zip(after, before))
            assert float(guard.nonfinite) == 1.0 and not math.isfinite(float(guard.total_norm))
            now = guard.counters()
            assert now == dict(steps=count["steps"] + 1, clipped=count["clipped"], skipped=1)
        elif poison is not None and k == poison[0] + 1:
            assert float(guard.nonfinite) == 0.0             # rewritten by every step
        s.step()
    torch.cuda.synchronize()
    _intact(guards)
    return dict(opt=o, params=params, p=[p.detach() for p in params], state=seated)


@pytest.mark.parametrize("name", list(OPT))
def test_guarded_training_follows_clip_grad_norm_and_torch(name):
    """25 steps under CosineAnnealingLR(T_max=20); max_norm 0.5 clips the three larger of the five gradient scales"""
    (p64, clipped), p32 = _reference(name)
    assert 5 <= clipped <= STEPS - 5, clipped                # clipping is exercised both ways
    guard = optim.GradGuard(max_norm=MAX_NORM)
    run = _device_run(name, guard)
    _within_bound(run["p"], p64, p32, f"{name} + guard")
    assert guard.counters() == dict(steps=STEPS, clipped=clipped, skipped=0)
    again = _device_run(name, optim.GradGuard(max_norm=MAX_NORM))           # and repeats bit for bit
    for x, y in zip(run["p"], again["p"]):
        assert torch.equal(x, y)


BAD_STEP = 3
POISON = {"nan-aligned": (BAD_STEP, 8, CHUNK + 7, float("nan")),           # tensor 8: 16-byte aligned, second workgroup
          "inf-misaligned-last": (BAD_STEP, 7, CHUNK, INF)}                 # tensor 7: 4-byte offset, its last element


@pytest.mark.parametrize("case", list(POISON))
@pytest.mark.parametrize("name", list(OPT))
def test_nonfinite_step_is_skipped(name, case):
    """the step with the bad element changes no parameter, state tensor, step count or private word and leaves the
    gradients unscaled (checked inside _device_run); all other steps follow torch's run without gradients at that step"""
    (p64, clipped), p32 = _reference(name, BAD_STEP)
    guard = optim.GradGuard(max_norm=MAX_NORM, on_nonfinite="skip")
    run = _device_run(name, guard, POISON[case])
    _within_bound(run["p"], p64, p32, f"{name} skip {case}")
    assert guard.counters() == dict(steps=STEPS, clipped=clipped, skipped=1)
    o = run["opt"]
    if name != "sgd":
        assert all(float(o.state[p]["step"]) == STEPS - 1 for p in run["params"])
    assert all(bool(torch.isfinite(p).all()) for p in run["p"])


@pytest.mark.parametrize("case", list(POISON))
@pytest.mark.parametrize("name", list(OPT))
def test_nonfinite_step_propagates_as_in_torch(name, case):
    cls, _, kw, _ = OPT[name]
    _, tensor, element, value = POISON[case]
    p0, grads = _inputs(SIZES, STEPS)
    params = [torch.nn.Parameter(p.to(DEV)) for p in p0]
    for p, g in zip(params, grads[0]):
        p.grad = g.to(DEV)
    params[tensor].grad[element] = value
    o = cls(params, **kw)
    o.guard = optim.GradGuard(max_norm=MAX_NORM)             # "propagate"
    o.step()
    assert not math.isfinite(float(o.guard.total_norm)) and float(o.guard.nonfinite) == 1.0
    assert bool(params[tensor].detach()[element].isnan())    # NaN coefficient, or Inf * 0
    assert o.guard.counters()["skipped"] == 0 and o.guard.counters()["steps"] == 1
    if name != "sgd":
        assert float(o.state[params[0]]["step"]) == 1.0


# ---- inside the graph
GRAPH = {"adamw": (optim.DeviceAdamW, dict(lr=5e-4)), "sgd": (optim.DeviceSGD, dict(lr=2e-2, momentum=0.9)),
         "nadam": (optim.DeviceNAdam, dict(lr=2e-4))}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(GRAPH))
def test_guard_inside_the_graph(name, dtype):
    """eager TrainStep against GraphedTrainStep, both with the same guarded device optimizer, under `deterministic_train`
    with a CosineAnnealingLR: equal losses, weights, optimizer state, norms and coefficients; a new max_norm reaches the
    next replay without a new capture"""
    cls, kw = GRAPH[name]
    steps, c0 = 5, 17

    def fresh(guard):
        m = _build(dtype, "hwgate")
        m.deterministic_train = True
        m._drop_calls = c0
        o = cls(list(m.parameters()), **kw)
        o.guard = guard
        return m, o, _batch(m)

    m, o, (x, y) = fresh(optim.GradGuard())                  # two measuring steps: what norm do these gradients have?
    s = train.TrainStep(m, o, None)
    seen = []
    for _ in range(2):
        s(x, y)
        seen.append(float(o.guard.total_norm))
        assert float(o.guard.clip_coef) == 1.0
    assert all(math.isfinite(v) and v > 0 for v in seen)
    max_norm = 0.5 * min(seen)
    runs = []
    for graphed in (False, True):
        guard = optim.GradGuard(max_norm=max_norm)
        m, o, (x, y) = fresh(guard)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
        if graphed:
            s = train.GraphedTrainStep(m, o, x, y)
            assert s.in_graph and guard.counters() == dict(steps=0, clipped=0, skipped=0)   # the warm-up left nothing
        else:
            s = train.TrainStep(m, o, None)
        trace = []
        for k in range(steps):
            loss = s(x, y).clone()
            trace.append((loss, guard.total_norm.clone(), guard.clip_coef.clone()))
            sched.step()
        assert guard.counters() == dict(steps=steps, clipped=steps, skipped=0)
        state = [t.clone() for p in m.parameters() for t in o._live.get(p, {}).values()]
        runs.append((trace, [p.detach().clone() for p in m.parameters()], state, s, guard, x, y))
    (te, we, se, _, _, _, _), (tg, wg, sg, s, guard, x, y) = runs
    print(f"{name} {dtype}: norms {[round(float(t[1]), 4) for t in tg]}, coefficients {[round(float(t[2]), 4) for t in tg]}")
    for k in range(steps):
        for a, b, what in zip(te[k], tg[k], ("loss", "total_norm", "clip_coef")):
            assert torch.equal(a, b), (k, what, float(a), float(b))
        assert float(tg[k][2]) < 1.0
    assert len(we) == len(wg) and all(torch.equal(a, b) for a, b in zip(we, wg))
    assert len(se) == len(sg) > 0 and all(torch.equal(a, b) for a, b in zip(se, sg))
    # halve max_norm: the same graph, the next replay's coefficient follows
    graph = s.graph
    guard.max_norm = 0.5 * max_norm
    s(x, y)
    norm, coef = float(guard.total_norm), float(guard.clip_coef)
    assert s.graph is graph and coef == pytest.approx(0.5 * max_norm / (norm + 1e-6), rel=1e-12)
    assert guard.counters() == dict(steps=steps + 1, clipped=steps + 1, skipped=0)
