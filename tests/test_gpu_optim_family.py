"""optim.DeviceSGD and optim.DeviceNAdam on the device: the HIP kernels of csrc/optim.hip against the reference's
other two optimizer types, torch.optim.SGD / torch.optim.NAdam (cfg.optimizer_type 'sgd' / 'nadam', hwgat/utils.py:73-84),
run on the CPU in float64; and the whole train step -- optimizer included -- replayed as one HIP graph
(train.GraphedTrainStep; reference loop hwgat/utils.py:93-116).

Inputs, seating and the bound are those of tests/test_gpu_optim.py, per tensor:
    max |p - p_64| <= 4 max |p_torch32 - p_64| + 4 * 2^-24 max |p_64|
where p_64 is torch's optimizer in float64 and p_torch32 the same run with torch's fp32 CPU optimizer.

Measured on an MI355X (this file's own print-out, test 1, largest max |p - p_64| over the bound among the nine tensors):
SGD lr 1e-3 0.205, with momentum 0.244, with dampening 0.240, nesterov 0.239; NAdam coupled 0.219, decoupled 0.391.  Over
torch's own fp32 error the same runs give 1.000 (the same error to the printed digits) except decoupled NAdam, 2.03 at
the most: torch multiplies p by the rounded (1 - lr wd), the kernel forms p - (lr wd) p in one rounding.  Test 3 (first
step, late gradient) 0.185; test 4 (state interchange) 0.157 for SGD and 0.162 for NAdam on either side."""
import copy
import functools
import importlib

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
STEPS = 25
SGD, NADAM = (optim.DeviceSGD, torch.optim.SGD), (optim.DeviceNAdam, torch.optim.NAdam)
CONFIGS = {
    "sgd": SGD + (dict(lr=1e-3),),
    "sgd-momentum": SGD + (dict(lr=1e-2, momentum=0.9, weight_decay=0.01),),
    "sgd-dampening": SGD + (dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.01),),
    "sgd-nesterov": SGD + (dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01),),
    "nadam": NADAM + (dict(lr=1e-3, weight_decay=0.01),),
    "nadam-decoupled": NADAM + (dict(lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True),),
    "sgd-first-step": SGD + (dict(lr=1e-2, momentum=0.9, dampening=0.5),),
}
SIX = [n for n in CONFIGS if n != "sgd-first-step"]


def _arrays(name):
    """the state arrays of a configuration: the keys of state[p] that have the parameter's shape"""
    cls, _, kw = CONFIGS[name]
    if cls is optim.DeviceNAdam:
        return ("exp_avg", "exp_avg_sq")
    return ("momentum_buffer",) if kw.get("momentum", 0.0) else ()


def _cpu_run(name, dtype, p0, grads, first_grad=None, schedule=True):
    """torch's optimizer on the CPU in `dtype`; tensor i gets no gradient before step first_grad[i]"""
    _, like, kw = CONFIGS[name]
    ps = [torch.nn.Parameter(p.to(dtype, copy=True)) for p in p0]          # a copy: the shared inputs are never written
    o = like(ps, **kw)
    s = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20) if schedule else None
    for k, gs in enumerate(grads):
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = g.to(dtype, copy=True) if first_grad is None or k >= first_grad[i] else None
        o.step()
        if s is not None:
            s.step()
    return [p.detach().double() for p in ps]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(p_64, p_torch32) of test 1: computed once, shared, never written"""
    p0, grads = _inputs(SIZES, STEPS)
    return _cpu_run(name, torch.float64, p0, grads), _cpu_run(name, torch.float32, p0, grads)


def _device_run(name, sizes=SIZES, steps=STEPS, first_grad=None, probe=None, fill=0.0):
    cls, _, kw = CONFIGS[name]
    p0, grads = _inputs(tuple(sizes), steps)
    pb, pv = _seat(p0)
    gb, gv = _seat([torch.zeros(n) for n in sizes])
    params = [torch.nn.Parameter(v) for v in pv]
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(params, pv))
    o = cls(params, **kw)
    guards, seated = dict(p=pb), {}
    for key in _arrays(name):                                # the state arrays seated by the caller, in guarded buffers
        guards[key], seated[key] = _seat([torch.full((n,), fill) for n in sizes])
    if seated:
        for i, p in enumerate(params):
            o.state[p] = {key: views[i] for key, views in seated.items()}
            if cls is optim.DeviceNAdam:
                o.state[p] = dict(step=torch.zeros((), device=DEV), mu_product=torch.ones((), device=DEV), **o.state[p])
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
        last_lr = o.param_groups[0]["lr"]
        o.step()
        s.step()
    torch.cuda.synchronize()
    return dict(opt=o, last_lr=last_lr, params=params, p=[p.detach() for p in params], state=seated, guards=guards)


@functools.lru_cache(maxsize=None)
def _device_reference_run(name):
    return _device_run(name)


@pytest.mark.parametrize("name", SIX)
def test_kernel_follows_torch_in_float64(name):
    """25 steps, CosineAnnealingLR(T_max=20) stepped after every optimizer step, tensors of every size class, half of
    them 4-byte aligned"""
    run = _device_reference_run(name)
    p64, p32 = _reference(name)
    _within_bound(run["p"], p64, p32, name)
    o = run["opt"]
    if name.startswith("nadam"):
        for p in run["params"]:
            assert float(o.state[p]["step"]) == STEPS and 0.0 < float(o.state[p]["mu_product"]) < 1.0
        assert o.device_hyper()[0]["decoupled_weight_decay"] is (name == "nadam-decoupled")
    elif name == "sgd":
        assert len(o.state) == 0                             # no momentum: no state, as torch
    held = o.device_hyper()[0]
    # the lr the last step ran with: the scheduler's double, not its float32 rounding
    assert held["lr"] == run["last_lr"] and run["last_lr"] != CONFIGS[name][2]["lr"], (held["lr"], run["last_lr"])
    for k, v in CONFIGS[name][2].items():
        if k != "lr":
            assert held[k] == v, k


@pytest.mark.parametrize("name", SIX)
def test_nothing_outside_the_tensors_is_touched_and_runs_repeat(name):
    run = _device_reference_run(name)
    for what, bufs in run["guards"].items():
        for i, (buf, off, n) in enumerate(bufs):
            assert bool((buf[:off] == SENTINEL).all()), (what, i, "before")
            assert bool((buf[off + n:] == SENTINEL).all()) and buf.numel() == off + n + PAD, (what, i, "after")
    assert set(run["state"]) == set(_arrays(name))
    for key, views in run["state"].items():                  # the seated arrays were used, and are the state
        for p, v in zip(run["params"], views):
            assert bool((v != 0).any()), key
            assert run["opt"].state[p][key].data_ptr() == v.data_ptr()
    again = _device_run(name)
    for x, y in zip(run["p"], again["p"]):
        assert torch.equal(x, y)
    for key in run["state"]:
        for x, y in zip(run["state"][key], again["state"][key]):
            assert torch.equal(x, y), key
    if name.startswith("nadam"):
        for p, q in zip(run["params"], again["params"]):
            for key in ("step", "mu_product"):
                assert torch.equal(run["opt"].state[p][key], again["opt"].state[q][key]), key


def test_first_step_with_dampening():
    """torch clones the gradient into a tensor's FIRST momentum buffer, whatever the dampening and whatever the buffer's
    storage held (here NaN: a multiply by zero would keep it); a tensor that first gets a gradient at step 3 has its
    first step then"""
    name, sizes, steps, first = "sgd-first-step", (3, 257, CHUNK + 1), 8, (0, 3, 0)
    p0, grads = _inputs(sizes, steps)

    def probe(k, o, params):                                 # before step k is issued
        bufs = [o.state[p]["momentum_buffer"] for p in params]
        if k == 1:
            for i in (0, 2):
                assert torch.equal(bufs[i].cpu(), grads[0][i]), i
        if k <= first[1]:
            assert torch.equal(params[1].detach().cpu(), p0[1]), k
            assert bool(bufs[1].isnan().all())               # its storage is still as seated
        if k == first[1] + 1:
            assert torch.equal(bufs[1].cpu(), grads[first[1]][1])
        assert len(o.table_records()) == (2 if k < first[1] else 3)

    run = _device_run(name, sizes, steps, first_grad=first, probe=probe, fill=float("nan"))
    _within_bound(run["p"], _cpu_run(name, torch.float64, p0, grads, first), _cpu_run(name, torch.float32, p0, grads, first),
                  "first step, late gradient")
    # and a parameter that never gets a gradient: no state at all
    frozen = torch.nn.Parameter(torch.randn(5, device=DEV))
    live = torch.nn.Parameter(torch.randn(5, device=DEV))
    keep = frozen.detach().clone()
    o = optim.DeviceSGD([frozen, live], **CONFIGS[name][2])
    live.grad = torch.ones_like(live)
    o.step()
    o.step()
    assert frozen not in o.state and torch.equal(frozen.detach(), keep)
    assert torch.allclose(o.state[live]["momentum_buffer"], torch.full_like(live, 1.0 * 0.9 + 0.5))


@pytest.mark.parametrize("direction", ["device_to_torch", "torch_to_device"])
@pytest.mark.parametrize("name", ["sgd-dampening", "nadam"])
def test_state_interchange(name, direction):
    """three steps with one optimizer, its state_dict() loaded into the other kind (torch's class on the CPU) on clones of
    the parameters, one more step on both with the same gradients: both follow torch's float64 run of the four steps"""
    cls, like, kw = CONFIGS[name]
    sizes, steps = (3, 257, CHUNK + 1), 4
    p0, grads = _inputs(sizes, steps)
    p64 = _cpu_run(name, torch.float64, p0, grads, schedule=False)
    p32 = _cpu_run(name, torch.float32, p0, grads, schedule=False)

    def make(kind, values):
        dev = DEV if kind == "device" else torch.device("cpu")
        ps = [torch.nn.Parameter(v.detach().clone().to(dev)) for v in values]
        return ps, (cls if kind == "device" else like)(ps, **kw)

    def step(ps, o, k):
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(p.device, copy=True)
        o.step()

    first, second = ("device", "torch") if direction == "device_to_torch" else ("torch", "device")
    ps1, o1 = make(first, p0)
    for k in range(3):
        step(ps1, o1, k)
    ps2, o2 = make(second, ps1)
    o2.load_state_dict(copy.deepcopy(o1.state_dict()))       # as out of a file
    if second == "torch":
        for grp in o2.param_groups:                          # torch's capturable NAdam does not step CPU tensors
            if "capturable" in grp:
                grp["capturable"] = False
    for p in ps2:
        assert all(t.device == p.device for t in o2.state[p].values() if torch.is_tensor(t) and t.dim())
        if cls is optim.DeviceNAdam:
            assert float(o2.state[p]["step"]) == 3.0
    step(ps1, o1, 3)
    step(ps2, o2, 3)
    _within_bound([p.detach() for p in ps1], p64, p32, f"{name} {direction}: {first}")
    _within_bound([p.detach() for p in ps2], p64, p32, f"{name} {direction}: {second} after load_state_dict")
    if cls is optim.DeviceNAdam:
        for p in ps2:
            assert float(o2.state[p]["step"]) == 4.0


GRAPH_CASES = [("sgd", dict(lr=5e-2), "hwgate", torch.float32),
               ("sgd", dict(lr=2e-2, momentum=0.9, dampening=0.1), "hwgate", torch.float32),
               ("sgd", dict(lr=2e-2, momentum=0.9, nesterov=True), "hwgate", torch.float32),
               ("nadam", dict(lr=2e-4), "hwgate", torch.float32),
               ("nadam", dict(lr=2e-4), "hgate", torch.bfloat16)]
# lr of the NAdam cases: NAdam's first steps move a weight by up to (1 - mu) / (1 - mu_product) + mu' / (1 - mu_product mu')
# ~ 1.9 times lr, Adam's by lr, and these models' loss falls from the first step under AdamW at 5e-4
# (tests/test_gpu_optim.py); 2e-4 stays under that


@pytest.mark.parametrize("opt_type, kw, kind, dtype", GRAPH_CASES,
                         ids=["sgd", "sgd-dampening", "sgd-nesterov", "nadam", "nadam-hgate-bf16"])
def test_whole_train_step_in_one_graph(opt_type, kw, kind, dtype):
    """eager TrainStep against GraphedTrainStep, both with the same device optimizer, under `deterministic_train`, with
    a CosineAnnealingLR stepped after every train step: the same kernels run on the same bits, so every loss and every
    weight is equal; the replays never enter the optimizer's Python step"""
    cls = optim.DeviceSGD if opt_type == "sgd" else optim.DeviceNAdam
    steps, c0 = 5, 17
    runs = []
    for graphed in (False, True):
        m = _build(dtype, kind)
        m.deterministic_train = True
        x, y = _batch(m)
        o = cls(list(m.parameters()), **kw)                   # ALL parameters: the frozen `B` is entry 0
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
        entered = []
        o.register_step_pre_hook(lambda *a, **k: entered.append(1))
        m._drop_calls = c0
        if graphed:
            w0 = [p.detach().clone() for p in m.parameters()]
            s = train.GraphedTrainStep(m, o, x, y)
            assert s.in_graph and m._drop_calls == c0
            assert all(torch.equal(a, b.detach()) for a, b in zip(w0, m.parameters()))   # capture left the weights
            for st in o.state.values():                                                  # and the state alone
                for key, t in st.items():
                    assert bool((t == (1.0 if key == "mu_product" else 0.0)).all()), key
            entered.clear()
        else:
            s = train.TrainStep(m, o, None)
        losses, lrs = [], []
        for k in range(steps):
            losses.append(s(x, y).clone())
            if k == 0 and graphed and kw.get("dampening"):
                # the first replay of a fresh SGD clones the gradient: the warm-up did not leave the private word set
                assert torch.equal(o.state[m.head.weight]["momentum_buffer"], m.head.weight.grad)
            held = o.device_hyper()[0]["lr"]
            assert held == sched.get_last_lr()[0], (k, held, sched.get_last_lr())        # as a double, exactly
            lrs.append(held)
            sched.step()
        assert len(entered) == (0 if graphed else steps)
        assert len(set(lrs)) == steps and lrs[0] == kw["lr"]
        assert m.B not in o.state
        if opt_type == "nadam":
            assert len(o.state) > 0 and all(float(st["step"]) == steps for st in o.state.values())
        elif "momentum" in kw:
            assert len(o.state) > 0 and all(bool(st["momentum_buffer"].any()) for st in o.state.values())
        else:
            assert len(o.state) == 0
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (le, we), (lg, wg) = runs
    print(f"{opt_type} {kw}: losses {[round(float(v), 4) for v in lg]}")
    for k in range(steps):
        assert torch.equal(le[k], lg[k]), (k, float(le[k]), float(lg[k]))
    assert float(lg[-1]) < float(lg[0])
    for n in we:
        assert torch.equal(we[n], wg[n]), n


def test_guards():
    for cls in (optim.DeviceSGD, optim.DeviceNAdam):
        q = torch.nn.Parameter(torch.zeros(4, device=DEV))
        q.grad = torch.ones(4, device=DEV)
        o = cls([q])
        o.param_groups[0]["maximize"] = True
        with pytest.raises(ValueError, match="maximize"):
            o.step()
        assert torch.equal(q.detach().cpu(), torch.zeros(4))
    # a captured table has the buffers its group's momentum asked for at capture: 0.9 -> 0 afterwards is refused
    q = torch.nn.Parameter(torch.zeros(4, device=DEV))
    q.grad = torch.ones(4, device=DEV)
    o = optim.DeviceSGD([q], lr=0.5, momentum=0.9)
    o.step()                                                 # state, hyper-parameter block
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    o.begin_capture()
    with torch.cuda.graph(graph):
        o.step()
    table = o.end_capture()
    graph.replay()
    torch.cuda.synchronize()
    assert table.n == 1 and torch.allclose(q.detach().cpu(), torch.full((4,), -0.5 - 0.5 * 1.9))
    keep = q.detach().clone()
    o.param_groups[0]["momentum"] = 0.0
    with pytest.raises(ValueError, match="momentum.*capture"):
        o.push_hyper()
    with pytest.raises(ValueError, match="momentum.*capture"):
        o.step()
    assert torch.equal(q.detach(), keep)
    o.param_groups[0]["momentum"] = 0.5                      # another non-zero value is a hyper-parameter like any other
    o.push_hyper()
    assert o.device_hyper()[0]["momentum"] == 0.5
