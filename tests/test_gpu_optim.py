"""optim.DeviceAdamW on the device: the HIP Adam / AdamW kernels (csrc/optim.hip) against the reference's optimizer,
torch.optim.AdamW / Adam (hwgat/utils.py:71-82), run on the CPU in float64; and the whole train step -- optimizer
included -- replayed as one HIP graph (train.GraphedTrainStep; reference loop hwgat/utils.py:93-116).

The bound of every value comparison, per tensor:   max |p - p_64| <= 4 max |p_torch32 - p_64| + 4 * 2^-24 max |p_64|
where p_64 is torch's optimizer in float64 and p_torch32 the same run with torch's fp32 CPU optimizer.  4x: the device's
fp32 divide and square root are not correctly rounded and FMA contraction moves single roundings; a wrong formula (a
bias-correction slip, a misplaced eps, coupled instead of decoupled decay) misses by orders of magnitude more.  The floor
covers the 1-element tensor, where torch's own error can come out near zero.

Measured on an MI355X (this file's own print-out, test 1, largest over the nine tensors): max |p - p_64| over the bound
0.198 (AdamW) and 0.210 (Adam); over torch's own fp32 error 0.872 (AdamW) and 1.000 (Adam: the same error to the printed
digits on every tensor)."""
import copy
import functools
import importlib

import pytest
import torch

from test_gpu_graph import _batch, _build

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
optim = importlib.import_module("sl-hwgat_amd.optim")
train = importlib.import_module("sl-hwgat_amd.train")
DEV = torch.device("cuda:0")
CHUNK = optim.CHUNK
SIZES = [1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
STEPS, LR, WD = 25, 1e-3, 0.01
SENTINEL, PAD = -12345.0, 8
TORCH = {True: torch.optim.AdamW, False: torch.optim.Adam}


@functools.lru_cache(maxsize=None)
def _inputs(sizes=tuple(SIZES), steps=STEPS):
    """seeded start values and gradients: the gradient scale moves over four decades between steps, and every fourth
    step every other entry is zero"""
    g = torch.Generator().manual_seed(7)
    p0 = [torch.randn(n, generator=g) for n in sizes]
    scales = [1.0, 1e-2, 1e-4, 1e-1, 1e-3]
    grads = []
    for k in range(steps):
        gs = [torch.randn(n, generator=g) * scales[k % 5] for n in sizes]
        if k % 4 == 2:
            for t in gs:
                t[::2] = 0
        grads.append(gs)
    return p0, grads


def _cpu_run(dtype, decoupled, p0, grads, first_grad=None, schedule=True):
    """torch's optimizer on the CPU in `dtype`; tensor i gets no gradient before step first_grad[i]"""
    ps = [torch.nn.Parameter(p.to(dtype, copy=True)) for p in p0]          # a copy: the shared inputs are never written
    o = TORCH[decoupled](ps, lr=LR, weight_decay=WD)
    s = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20) if schedule else None
    for k, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = g.to(dtype, copy=True) if first_grad is None or k >= first_grad[i] else None
        o.step()
        if s is not None:
            s.step()
    return [p.detach().double() for p in ps]


@functools.lru_cache(maxsize=None)
def _reference(decoupled):
    """(p_64, p_torch32) of test 1: computed once, shared, never written"""
    p0, grads = _inputs()
    return _cpu_run(torch.float64, decoupled, p0, grads), _cpu_run(torch.float32, decoupled, p0, grads)


def _within_bound(got, p64, p32, what):
    worst = 0.0
    for i, (a, r, t) in enumerate(zip(got, p64, p32)):
        err = (a.detach().cpu().double() - r).abs().max().item()
        err32 = (t - r).abs().max().item()
        bound = 4 * err32 + 4 * 2.0 ** -24 * r.abs().max().item()
        print(f"{what}: tensor {i} (n = {r.numel()}): err {err:.3e}, torch fp32 err {err32:.3e}, bound {bound:.3e}, "
              f"err / bound {err / bound:.3f}, err / torch fp32 err {err / max(err32, 1e-300):.3f}")
        worst = max(worst, err / bound)
        assert err <= bound, (what, i, err, bound)
    print(f"{what}: largest err / bound {worst:.3f}")


def _seat(values):
    """tensor i as a view into its own sentinel-filled buffer: at element offset 1 (4-byte aligned: the scalar path) for
    odd i, at offset 4 (16-byte aligned: the vector path) for even i, PAD sentinels after it"""
    bufs, views = [], []
    for i, t in enumerate(values):
        off = 1 if i % 2 else 4
        buf = torch.full((off + t.numel() + PAD,), SENTINEL, device=DEV)
        view = buf[off:off + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == (4 if off == 1 else 0)
        bufs.append((buf, off, t.numel()))
        views.append(view)
    return bufs, views


def _device_run(decoupled, sizes=tuple(SIZES), steps=STEPS, first_grad=None, probe=None):
    p0, grads = _inputs(sizes, steps)
    pb, pv = _seat(p0)
    mb, mv = _seat([torch.zeros(n) for n in sizes])
    vb, vv = _seat([torch.zeros(n) for n in sizes])
    gb, gv = _seat([torch.zeros(n) for n in sizes])
    params = [torch.nn.Parameter(v) for v in pv]
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(params, pv))
    o = optim.DeviceAdamW(params, lr=LR, weight_decay=WD, decoupled_weight_decay=decoupled)
    for p, m, v in zip(params, mv, vv):                      # the moments seated by the caller, in guarded buffers
        o.state[p] = {"step": torch.zeros((), device=DEV), "exp_avg": m, "exp_avg_sq": v}
    s = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
    for k in range(steps):
        for i, (p, g) in enumerate(zip(params, gv)):
            if first_grad is None or k >= first_grad[i]:
                g.copy_(grads[k][i])
                p.grad = g
            else:
                p.grad = None
        if probe is not None:
            probe(k, o, params)
        o.step()
        s.step()
    torch.cuda.synchronize()
    return dict(opt=o, params=params, p=[p.detach() for p in params], m=mv, v=vv, guards=dict(p=pb, m=mb, v=vb))


@functools.lru_cache(maxsize=None)
def _device_reference_run(decoupled):
    return _device_run(decoupled)


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_kernel_follows_torch_in_float64(decoupled):
    """25 steps, weight decay 0.01, CosineAnnealingLR(T_max=20) stepped after every optimizer step, tensors of every size
    class, half of them 4-byte aligned"""
    run = _device_reference_run(decoupled)
    p64, p32 = _reference(decoupled)
    _within_bound(run["p"], p64, p32, "adamw" if decoupled else "adam")
    for p in run["params"]:
        assert float(run["opt"].state[p]["step"]) == STEPS
    assert run["opt"].device_hyper()[0]["decoupled_weight_decay"] is decoupled


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_nothing_outside_the_tensors_is_touched(decoupled):
    run = _device_reference_run(decoupled)
    for name, bufs in run["guards"].items():
        for i, (buf, off, n) in enumerate(bufs):
            assert bool((buf[:off] == SENTINEL).all()), (name, i, "before")
            assert bool((buf[off + n:] == SENTINEL).all()) and buf.numel() == off + n + PAD, (name, i, "after")
    assert all(bool((m != 0).any()) and bool((v != 0).any()) for m, v in zip(run["m"], run["v"]))   # the seated moments were used


def test_skipped_parameter_and_per_tensor_step_counts():
    """a parameter without a gradient keeps its bits and has no entry; given one from step 3 on, its own step count
    lags by 3 and its values follow torch's float64 run"""
    sizes, steps, first = (3, 257, CHUNK + 1), 8, (0, 3, 0)
    p0, grads = _inputs(sizes, steps)
    seen = []

    def probe(k, o, params):
        recs = o.table_records()
        seen.append(len(recs))
        if k <= first[1]:                                     # untouched so far (checked before this step's launch)
            assert torch.equal(params[1].detach().cpu(), p0[1]), k

    run = _device_run(True, sizes, steps, first_grad=first, probe=probe)
    assert seen == [2, 2, 2] + [3] * (steps - 3)
    counts = [float(run["opt"].state[p]["step"]) for p in run["params"]]
    assert counts == [steps, steps - 3, steps]
    _within_bound(run["p"], _cpu_run(torch.float64, True, p0, grads, first), _cpu_run(torch.float32, True, p0, grads, first),
                  "late gradient")
    # and a parameter that never gets one: no state at all
    frozen = torch.nn.Parameter(torch.randn(5, device=DEV))
    live = torch.nn.Parameter(torch.randn(5, device=DEV))
    keep = frozen.detach().clone()
    o = optim.DeviceAdamW([frozen, live])
    live.grad = torch.ones_like(live)
    o.step()
    o.step()
    assert frozen not in o.state and torch.equal(frozen.detach(), keep) and float(o.state[live]["step"]) == 2.0


def test_repeats_bit_for_bit():
    a, b = _device_reference_run(True), _device_run(True)
    for name in ("p", "m", "v"):
        for x, y in zip(a[name], b[name]):
            assert torch.equal(x, y), name


@pytest.mark.parametrize("direction", ["device_to_torch", "torch_to_device"])
def test_state_interchange_on_the_device(direction):
    """three steps with one optimizer, its state_dict() loaded into the other kind on clones of the parameters, one more
    step on both with the same gradients: both follow torch's float64 run of the four steps"""
    sizes, steps = (3, 257, CHUNK + 1), 4
    p0, grads = _inputs(sizes, steps)
    p64 = _cpu_run(torch.float64, True, p0, grads, schedule=False)
    p32 = _cpu_run(torch.float32, True, p0, grads, schedule=False)

    def make(kind, values):
        ps = [torch.nn.Parameter(v.detach().clone().to(DEV)) for v in values]
        if kind == "device":
            return ps, optim.DeviceAdamW(ps, lr=LR, weight_decay=WD)
        return ps, torch.optim.AdamW(ps, lr=LR, weight_decay=WD, fused=True, capturable=True)

    def step(ps, o, k):
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(DEV)
        o.step()

    first, second = ("device", "torch") if direction == "device_to_torch" else ("torch", "device")
    ps1, o1 = make(first, p0)
    for k in range(3):
        step(ps1, o1, k)
    ps2, o2 = make(second, ps1)
    o2.load_state_dict(copy.deepcopy(o1.state_dict()))       # as out of a file: torch's loader keeps tensors that already fit, so a
                                                             # live state_dict() handed over as it is would be shared by both
    for p in ps2:
        assert float(o2.state[p]["step"]) == 3.0 and o2.state[p]["exp_avg"].is_cuda
    step(ps1, o1, 3)
    step(ps2, o2, 3)
    _within_bound([p.detach() for p in ps1], p64, p32, f"{direction}: {first}")
    _within_bound([p.detach() for p in ps2], p64, p32, f"{direction}: {second} after load_state_dict")
    for p in ps2:
        assert float(o2.state[p]["step"]) == 4.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["hwgate", "hgate"])
def test_whole_train_step_in_one_graph(dtype, kind):
    """eager TrainStep + DeviceAdamW against GraphedTrainStep + DeviceAdamW under `deterministic_train`, with a
    CosineAnnealingLR stepped after every train step: the same kernels run on the same bits, so every loss and every
    weight is equal; the replays never enter the optimizer's Python step"""
    steps, c0 = 5, 17
    runs = []
    for graphed in (False, True):
        m = _build(dtype, kind)
        m.deterministic_train = True
        x, y = _batch(m)
        o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)           # ALL parameters: the frozen `B` is entry 0
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
        entered = []
        o.register_step_pre_hook(lambda *a, **k: entered.append(1))
        m._drop_calls = c0
        if graphed:
            w0 = [p.detach().clone() for p in m.parameters()]
            s = train.GraphedTrainStep(m, o, x, y)
            assert s.in_graph and m._drop_calls == c0
            assert all(torch.equal(a, b.detach()) for a, b in zip(w0, m.parameters()))   # capture left the weights,
            for st in o.state.values():                                                  # moments and step counts alone
                assert float(st["step"]) == 0.0 and not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())
            entered.clear()
        else:
            s = train.TrainStep(m, o, None)
        losses, lrs = [], []
        for k in range(steps):
            losses.append(s(x, y).clone())
            held = o.device_hyper()[0]["lr"]
            assert held == sched.get_last_lr()[0], (k, held, sched.get_last_lr())        # as a double, exactly
            lrs.append(held)
            sched.step()
        assert len(entered) == (0 if graphed else steps)
        assert len(set(lrs)) == steps and lrs[0] == 5e-4
        assert m.B not in o.state
        assert all(float(st["step"]) == steps for st in o.state.values())
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}, s, m, x, y))
    (le, we, _, _, _, _), (lg, wg, s, m, x, y) = runs
    for k in range(steps):
        assert torch.equal(le[k], lg[k]), (k, float(le[k]), float(lg[k]))
    assert float(lg[-1]) < float(lg[0])
    for n in we:
        assert torch.equal(we[n], wg[n]), n
    # guard: a parameter reallocated after the capture
    w = m.head.weight
    w.data = w.data.clone()
    with pytest.raises(RuntimeError, match="capture again"):
        s(x, y)


def test_guards():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.DeviceAdamW([p]).step()
    q = torch.nn.Parameter(torch.zeros(4, device=DEV))
    q.grad = torch.ones(4, device=DEV)
    o = optim.DeviceAdamW([q])
    o.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        o.step()
    assert torch.equal(q.detach().cpu(), torch.zeros(4))
