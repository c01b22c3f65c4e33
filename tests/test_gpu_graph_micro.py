"""GPU: micro-batches and short batches inside the captured train step (train.GraphedTrainStep(micro_batch=..., ragged=True))
against their eager twins (train.TrainStep(micro_batch=..., pad_to=...); reference loop hwgat/utils.py:93-116, whose loaders
keep the short last batch, hwgat/utils.py:44-49), and the slice-aware criterion kernels hwgat_bsce_fwd / hwgat_bsce_bwd of
csrc/loss_eval.hip on their own.

Graph against eager is `torch.equal` throughout, under `deterministic_train`: a replay issues the eager step's kernels on the
eager step's inputs.  The criterion kernels are held against the reference's formula (hwgat/losses/SmoothCrossEntropy.py)
evaluated by torch in fp64 on the live rows and divided by the batch's row count, with the bound of
tests/test_gpu_loss_eval.py: max(FLOOR, 4 x refdev), refdev being the deviation of the same formula in fp32 on the CPU."""
import functools
import gc
import importlib
import math

import pytest
import torch

import stgcn_helpers as SH
from helpers import rel_err

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
optim = importlib.import_module("sl-hwgat_amd.optim")
DEV = torch.device("cuda:0")
C0 = 17                 # dropout counter the runs start from
THRESHOLDS = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]   # HWGATE.py:96 draws these at random


def _build(dtype, kind="hwgate", drop=True):
    """the tiny models of tests/test_gpu_graph.py: src_len 16, 7 classes, 32 joints, dropout on at 0.1"""
    torch.manual_seed(11)
    ds = {"src_len": 16, "num_class": 7}
    if kind == "hwgate":
        hp = hw.HWGATEParams(ds, 2, DEV, num_kps=32)
        cls = hw.Model
    elif kind == "hgate":
        hp, cls = hw.HGATEParams(ds, 2, DEV), hw.HGATEModel
    else:
        hp, cls = hw.WGATEParams(ds, 2, DEV, num_kps=32), hw.WGATEModel
    if not drop:
        hp.drop_rate = 0.0
    model = cls(*hp.get_model_params()).to(DEV)
    assert model.drop_rate == (0.1 if drop else 0.0)
    model.set_activation_dtype(dtype)
    model.train()
    if kind == "hwgate":
        model.threshold_override = THRESHOLDS
    model.deterministic_train = True
    model._drop_calls = C0
    return model


def _batch(model, B=8):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(B, model.temporal_dim, model.num_kps, model.kp_dim, device=DEV, generator=g)
    y = torch.randint(0, 7, (B,), device=DEV, generator=g)
    return x, y


def _probe(model):
    """the mask a kernel draws NOW from the model's device seed word"""
    return HF.dropout_mask((2048,), model._site_seeds(2)[1], 0.5, DEV, seed_base=model._seed_base())


def _opt_state(opt, model):
    if isinstance(opt, optim.DeviceOptimizer):
        return [t.clone() for p in model.parameters() for t in opt._live.get(p, {}).values()]
    return [t.clone() for p in model.parameters() for t in opt.state.get(p, {}).values() if torch.is_tensor(t)]


DEVICE_OPTS = {"adamw": (optim.DeviceAdamW, dict(lr=5e-4)), "sgd": (optim.DeviceSGD, dict(lr=2e-2, momentum=0.9)),
               "nadam": (optim.DeviceNAdam, dict(lr=2e-4))}


def _make_opt(name, model, guard=None):
    if name == "torch":
        return torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    cls, kw = DEVICE_OPTS[name]
    o = cls(list(model.parameters()), **kw)
    o.guard = guard
    return o


def _run(kind, dtype, opt_name, graphed, feed, max_norm=None, B=8, sched_after=2, **step_kw):
    """one run of len(feed) steps, feed[k] being the number of rows of step k; everything a comparison needs"""
    m = _build(dtype, kind)
    x, y = _batch(m, B)
    guard = None if max_norm is None else optim.GradGuard(max_norm=max_norm, on_nonfinite="skip")
    o = _make_opt(opt_name, m, guard)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
    if graphed:
        s = train.GraphedTrainStep(m, o, x, y, **step_kw)
        assert m._drop_calls == C0                           # capture left the counter alone
    else:
        kw = dict(step_kw)
        if kw.pop("ragged", False):
            kw["pad_to"] = B
        s = train.TrainStep(m, o, **kw)
    graph = s.graph if graphed else None
    trace = []
    for k, n in enumerate(feed):
        loss = s(x[:n], y[:n]).clone()
        rec = [loss, s.correct.clone(), _probe(m)]
        if guard is not None:
            rec += [guard.total_norm.clone(), guard.clip_coef.clone()]
        trace.append(rec)
        if k == sched_after:
            sched.step()
    assert graph is (s.graph if graphed else None)           # one capture serves every step
    return dict(trace=trace, weights=[p.detach().clone() for p in m.parameters()], state=_opt_state(o, m), model=m, step=s,
                guard=guard, buffers={k: v.clone() for k, v in m.state_dict().items()})


def _same(a, b):
    for k, (ra, rb) in enumerate(zip(a["trace"], b["trace"])):
        for i, (ta, tb) in enumerate(zip(ra, rb)):
            assert torch.equal(ta, tb), (k, ("loss", "correct", "mask", "total_norm", "clip_coef")[i], ta, tb)
    assert len(a["weights"]) == len(b["weights"]) and all(torch.equal(p, q) for p, q in zip(a["weights"], b["weights"]))
    assert len(a["state"]) == len(b["state"]) > 0 and all(torch.equal(p, q) for p, q in zip(a["state"], b["state"]))
    assert a["model"]._drop_calls == b["model"]._drop_calls


@functools.lru_cache(maxsize=None)
def _half_the_smaller_norm(kind, dtype, opt_name):
    """two measuring steps of the eager micro-batched step under a guard that only measures"""
    m = _build(dtype, kind)
    x, y = _batch(m)
    o = _make_opt(opt_name, m, optim.GradGuard())
    s = train.TrainStep(m, o, micro_batch=3)
    seen = []
    for _ in range(2):
        s(x, y)
        seen.append(float(o.guard.total_norm))
        assert float(o.guard.clip_coef) == 1.0
    assert all(math.isfinite(v) and v > 0 for v in seen)
    return 0.5 * min(seen)


# ------------------------------------------------------------------------------------------ 1. graph equals eager
def _graph_equals_eager(kind, dtype, opt_name):
    max_norm = None if opt_name == "torch" else _half_the_smaller_norm(kind, dtype, opt_name)
    runs = [_run(kind, dtype, opt_name, graphed, [8] * 5, max_norm=max_norm, micro_batch=3) for graphed in (False, True)]
    eager, graph = runs
    s = graph["step"]
    assert s.n_slices == 3 and s.in_graph == (opt_name != "torch")
    _same(eager, graph)
    assert eager["model"]._drop_calls == graph["model"]._drop_calls == C0 + 15
    losses = [float(r[0]) for r in graph["trace"]]
    masks = [r[2] for r in graph["trace"]]
    assert all(math.isfinite(v) for v in losses)
    assert not torch.equal(masks[0], masks[1])                                       # fresh masks every step
    assert all(0 <= int(r[1]) <= 8 for r in graph["trace"])
    if max_norm is not None:
        assert float(graph["trace"][0][4]) < 1.0                                     # the guard clips, inside the graph
        counters = graph["guard"].counters()
        assert counters == eager["guard"].counters() and counters["steps"] == 5 and counters["skipped"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["hwgate", "hgate", "wgate"])
def test_micro_batched_graph_equals_the_eager_micro_batched_step(kind, dtype):
    """slices 3 + 3 + 2, DeviceAdamW under a clipping GradGuard inside the graph, a CosineAnnealingLR stepped after step 2:
    losses, correct counts, weights, optimizer state, norms, coefficients, the counter and the masks drawn after each step"""
    _graph_equals_eager(kind, dtype, "adamw")


@pytest.mark.parametrize("opt_name", ["sgd", "nadam"])
def test_micro_batched_graph_with_the_other_device_optimizers(opt_name):
    _graph_equals_eager("hgate", torch.float32, opt_name)


def test_micro_batched_graph_with_the_optimizer_out_of_the_graph():
    """torch's AdamW(fused, capturable) is stepped after the replay, once, on the accumulated gradients"""
    _graph_equals_eager("hwgate", torch.float32, "torch")


# ------------------------------------------------------------------------------------------ 2. a BatchNorm model
def test_batchnorm_model_normalises_and_counts_per_slice():
    cfg = dict(SH.CONFIGS["a"], B=8, T=8)
    x, y = (t.to(DEV) for t in SH.make_input(cfg))
    runs = []
    for graphed in (False, True):
        torch.manual_seed(21)
        m = hw.STGCNModel(*SH.model_args(cfg, 0.05)).to(DEV).train()     # a new model: no batch has been tracked yet
        m.deterministic_train = True
        torch.manual_seed(5)
        o = optim.DeviceAdamW(list(m.parameters()), lr=3e-4)
        s = train.GraphedTrainStep(m, o, x, y, micro_batch=4) if graphed else train.TrainStep(m, o, micro_batch=4)
        losses = [s(x, y).clone() for _ in range(3)]
        runs.append((losses, {k: v.clone() for k, v in m.state_dict().items()}, s))
    (le, sde, _), (lg, sdg, s) = runs
    assert s.n_slices == 2
    assert all(torch.equal(a, b) for a, b in zip(le, lg))
    names = [k for k in sde if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert len(names) >= 3 and set(sde) == set(sdg)
    for k in sde:                                            # parameters, running statistics, batch counts
        assert torch.equal(sde[k], sdg[k]), k
    for k in names:
        if k.endswith("num_batches_tracked"):
            assert int(sdg[k]) == 6, (k, int(sdg[k]))        # two slices per step, and the warm-up left no trace


# ------------------------------------------------------------------------------------------ 3. degenerate values
def test_values_that_do_not_slice_take_the_unsliced_step():
    plain = _run("hwgate", torch.float32, "adamw", True, [8] * 3)
    assert plain["step"].n_slices == 1
    for mb in (None, 8, 100):
        other = _run("hwgate", torch.float32, "adamw", True, [8] * 3, micro_batch=mb)
        assert other["step"].n_slices == 1
        _same(plain, other)
    assert plain["model"]._drop_calls == C0 + 3


def test_one_clip_slices():
    eager, graph = (_run("hwgate", torch.float32, "adamw", g, [8] * 3, micro_batch=1) for g in (False, True))
    assert graph["step"].n_slices == 8
    _same(eager, graph)
    assert graph["model"]._drop_calls == C0 + 24


# ------------------------------------------------------------------------------------------ 4. memory
def test_sliced_capture_holds_one_slice_of_activations():
    """hwgate fp32 at B 16: the peak of allocated bytes over construction and three replays must be lower with 4-clip
    slices than unsliced -- a capture that kept every slice's saved activations alive would need as much as the unsliced
    one.  The condition is the strict inequality; the figures are printed (DESIGN.md section 6o records them)."""
    peak = {}
    for mb in (None, 4):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m = _build(torch.float32, "hwgate")
        x, y = _batch(m, 16)
        o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
        s = train.GraphedTrainStep(m, o, x, y, micro_batch=mb)
        for _ in range(3):
            s(x, y)
        torch.cuda.synchronize()
        peak[mb] = torch.cuda.max_memory_allocated()
        assert s.n_slices == (1 if mb is None else 4) and math.isfinite(float(s.loss))
        print(f"PEAK micro_batch={mb}: {peak[mb]} bytes allocated at the most ({base} before the variant)")
        del s, o, m, x, y
    assert peak[4] < peak[None], peak


# ------------------------------------------------------------------------------------------ 5. ragged equals its eager twin
FEED = [8, 5, 3, 1, 8]  # 5: the third slice is empty; 3: two slices are; 1: a partly filled first slice


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["hwgate", "hgate"])
def test_ragged_graph_equals_the_padded_eager_step(kind, dtype):
    eager, graph = (_run(kind, dtype, "adamw", g, FEED, micro_batch=3, ragged=True) for g in (False, True))
    s = graph["step"]
    assert s.n_slices == 3 and s.ragged and type(s.criterion) is train.BatchSlicedCrossEntropyLoss
    _same(eager, graph)
    assert graph["model"]._drop_calls == C0 + 15             # empty slices run (and draw) like full ones
    for n, rec in zip(FEED, graph["trace"]):
        assert math.isfinite(float(rec[0])) and 0 <= int(rec[1]) <= n, (n, float(rec[0]), int(rec[1]))
    assert int(s.n_rows) == 8 and int(eager["step"].n_rows) == 8
    # the padding rows hold zeros, but nothing depends on it: a third run refills them with other finite clips and
    # other labels between staging a batch and its replay
    m = _build(dtype, kind)
    x, y = _batch(m)
    o = _make_opt("adamw", m)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
    s = train.GraphedTrainStep(m, o, x, y, micro_batch=3, ragged=True)
    graph_obj = s.graph
    g = torch.Generator(device=DEV).manual_seed(99)
    for k, n in enumerate(FEED):
        s._pad.load(x[:n], y[:n])                            # stage: rows, zeros, the row count
        s.x[n:] = torch.rand(s.x[n:].shape, device=DEV, generator=g) * 3.0 - 1.0
        s.y[n:] = torch.randint(0, 7, (8 - n,), device=DEV, generator=g)
        loss = s(s.x[:n], s.y[:n]).clone()                   # the staged buffers themselves: nothing is copied or zeroed
        assert n == 8 or bool((s.x[n:] != 0).any())
        assert torch.equal(loss, graph["trace"][k][0]) and torch.equal(s.correct, graph["trace"][k][1]), (k, n)
        if k == 2:
            sched.step()
    assert s.graph is graph_obj
    assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), graph["weights"]))


def test_row_counts_the_step_was_not_built_for_are_refused():
    m = _build(torch.float32, "hgate")
    x, y = _batch(m, 9)
    o = _make_opt("adamw", m)
    s = train.GraphedTrainStep(m, o, x[:8], y[:8], micro_batch=3, ragged=True)
    with pytest.raises(ValueError, match="built for 1 to 8"):
        s(x, y)                                              # n > B
    with pytest.raises(ValueError, match="built for 1 to 8"):
        s(x[:0], y[:0])
    with pytest.raises(ValueError, match="built for 1 to 8"):
        s(x[:4], y[:5])
    e = train.TrainStep(m, o, micro_batch=3, pad_to=8)
    with pytest.raises(ValueError, match="built for 1 to 8"):
        e(x, y)
    m2 = _build(torch.float32, "hgate")
    s2 = train.GraphedTrainStep(m2, _make_opt("adamw", m2), x[:8], y[:8], micro_batch=3)
    with pytest.raises(ValueError, match="captured for"):
        s2(x[:5], y[:5])                                     # without `ragged` only the captured batch size
    with pytest.raises(ValueError, match="captured for"):
        s2(x, y)


# ------------------------------------------------------------------------------------------ 6. ragged means what it says
def test_padded_step_is_the_step_on_the_real_clips():
    """5 clips padded to 8 against the plain micro-batched step on the 5 clips, no dropout: the same sums in another
    order, so the bounds are those of tests/test_gpu_model.py::test_micro_batched_step_equals_full_batch_step"""
    res = []
    for pad_to in (None, 8):
        m = _build(torch.float32, "hwgate", drop=False)
        x, y = _batch(m)
        s = train.TrainStep(m, None, None, micro_batch=3, pad_to=pad_to)
        s(x[:5], y[:5])
        res.append((float(s.loss), int(s.correct), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    (l0, c0, g0), (l1, c1, g1) = res
    print(f"plain {l0:.7f} padded {l1:.7f}")
    assert abs(l1 - l0) < 1e-4 and c0 == c1
    assert set(g0) == set(g1) and len(g0) > 10
    for k in g0:
        if k.endswith("attn.qkv.bias"):
            continue                                         # the key third has an exactly-zero true gradient: pure rounding noise
        assert rel_err(g1[k].cpu(), g0[k].cpu()) < 1e-4, (k, rel_err(g1[k].cpu(), g0[k].cpu()))


# ------------------------------------------------------------------------------------------ 7. the criterion kernels alone
FLOOR = 2e-5            # the floor of tests/test_gpu_loss_eval.py for hwgat_sce_fwd / hwgat_sce_bwd in fp32
EPS, G_UP = 0.01, 0.37
KERNEL_CASES = [(3, 7, 0), (5, 2002, 0), (4, 2003, 1),      # (b, C, floats the logits sit past a 16-byte boundary)
                (3, 2004, 0), (3, 2004, 1)]                  # C % 4 == 0: 16-byte loads, and the same rows unaligned


def _rows(z, y):
    lp = torch.log_softmax(z, dim=-1)
    return (1.0 - EPS) * (-lp.gather(-1, y.unsqueeze(1)).squeeze(1)) + EPS * (-lp.mean(-1))


def _slice_ref(z, y, v, n_rows):
    """(loss, d loss / d z * G_UP) of the slice in z's dtype: the live rows' sum over the batch's row count"""
    z = z.clone().requires_grad_(True)
    loss = _rows(z[:v], y[:v]).sum() / n_rows
    (loss * G_UP).backward()
    return loss.detach(), z.grad


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())


def _entry(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("b,C,shift", KERNEL_CASES)
def test_criterion_kernels_against_fp64(b, C, shift):
    g = torch.Generator().manual_seed(1000 * b + C)
    z = torch.randn(b, C, generator=g)
    y = torch.randint(0, C, (b,), generator=g)
    flat = torch.zeros(b * C + 4, device=DEV)
    zd = flat[shift:shift + b * C].view(b, C)
    zd.copy_(z)
    assert zd.data_ptr() % 16 == 4 * shift and zd.is_contiguous()
    yd = y.to(DEV)
    g_dev = torch.tensor([G_UP], device=DEV)
    full = HF.sce_forward(zd, yd, EPS)                       # rank and pred of every row by the batch kernel
    worst = {"loss": 0.0, "dz": 0.0}
    for offset in (0, 3):
        for n_rows in range(0, offset + b + 3):
            v = min(max(n_rows - offset, 0), b)
            word = torch.tensor([n_rows], device=DEV, dtype=torch.int32)
            out = tuple(torch.full_like(t, 77) for t in HF.bsce_forward(zd, yd, EPS, word, offset))
            loss, row_loss, lse, rank, pred, correct, live = HF.bsce_forward(zd, yd, EPS, word, offset, out=out)
            dz = HF.bsce_backward(zd, yd, lse, g_dev, EPS, word, offset, out=torch.full((b, C), 7.5, device=DEV))
            assert int(live) == v, (offset, n_rows)
            assert bool((dz[v:] == 0).all()), (offset, n_rows)                       # dead rows: exactly zero
            for t in (row_loss, lse, rank, pred):                                    # and untouched in the forward
                assert bool((t[v:] == 77).all()), (offset, n_rows)
            assert torch.equal(rank[:v], full[3][:v]) and torch.equal(pred[:v], full[4][:v])
            assert torch.equal(row_loss[:v], full[1][:v]) and torch.equal(lse[:v], full[2][:v])
            assert correct.dtype == torch.int64 and int(correct) == int((full[3][:v] == 0).sum())
            if v == 0:
                assert float(loss) == 0.0 and not bool(dz.any()), (offset, n_rows, float(loss))
                continue
            ref_loss, ref_dz = _slice_ref(z.double(), y, v, n_rows)
            loss32, dz32 = _slice_ref(z, y, v, n_rows)
            e_loss, e_dz = _rel(loss[0], ref_loss), _entry(dz, ref_dz)
            worst = {"loss": max(worst["loss"], e_loss), "dz": max(worst["dz"], e_dz)}
            assert e_loss <= max(FLOOR, 4 * _rel(loss32, ref_loss)), (offset, n_rows, e_loss)
            assert e_dz <= max(FLOOR, 4 * _entry(dz32, ref_dz)), (offset, n_rows, e_dz)
            # a repeat is bit-equal
            again = HF.bsce_forward(zd, yd, EPS, word, offset)
            assert torch.equal(again[0], loss) and torch.equal(again[5], correct)
            assert torch.equal(HF.bsce_backward(zd, yd, again[2], g_dev, EPS, word, offset), dz)
    print(f"WORST_bsce b={b} C={C} shift={shift}: loss {worst['loss']:.2e}, dz {worst['dz']:.2e}")


def test_criterion_autograd_node_and_slices_add_up_to_the_batch_mean():
    """the slices' losses of a batch of 8 with 5 real rows add up to the mean over the 5, their gradients are the batch
    kernel's on those rows within the fp32 bound, and the module counts the real rows' hits"""
    g = torch.Generator().manual_seed(8)
    z, y = torch.randn(8, 7, generator=g), torch.randint(0, 7, (8,), generator=g)
    word = torch.tensor([5], device=DEV, dtype=torch.int32)
    crit = train.BatchSlicedCrossEntropyLoss(EPS)
    total, hits, grads = 0.0, 0, []
    for i in range(0, 8, 3):
        zs = z[i:i + 3].to(DEV).requires_grad_(True)
        crit.place(word, i)
        loss = crit(zs, y[i:i + 3].to(DEV))
        assert loss.dim() == 0 and not crit.last_rank.requires_grad
        loss.backward()
        total += float(loss.detach())
        hits += int(crit.correct())
        grads.append(zs.grad.cpu())
    ref = _rows(z[:5].double(), y[:5])
    assert abs(total - float(ref.mean())) <= FLOOR * max(1.0, float(ref.mean()))
    assert hits == int((z[:5].argmax(-1) == y[:5]).sum())
    dz = torch.cat(grads)
    assert not bool(dz[5:].any()) and float(grads[2].abs().max()) == 0.0
    zr = z[:5].double().clone().requires_grad_(True)
    _rows(zr, y[:5]).mean().backward()
    assert _entry(dz[:5], zr.grad) <= FLOOR
