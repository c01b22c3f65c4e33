"""GPU parity of the ST-GCN baseline: every new HIP kernel through the C ABI against fp64 torch (entry by entry and in
norm), one block at a time through stgcn_block.st_gcn_block against the fp64 restatement of tests/stgcn_helpers.py, and
the whole `STGCNModel` against the reference-generated fixtures tests/golden/stgcn_{a,b,c,d}.npz -- forward quantities
tightly everywhere; gradients tightly on the margin-selected fixtures a-c and within the wiring bound on all four (see
make_fixtures_stgcn.py for why: 20 ReLUs behind BatchNorms make the whole-model gradient discontinuous in the rounding)."""
import importlib

import numpy as np
import pytest
import torch

import stgcn_helpers as SH
from helpers import load_fixture, rel_err, entrywise, grad_digest_check, probe_vectors

pytestmark = pytest.mark.gpu

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
serve = importlib.import_module("sl-hwgat_amd.serve")
SB = importlib.import_module("sl-hwgat_amd.stgcn_block")
STGCN = importlib.import_module("sl-hwgat_amd.models.STGCN")
DEV = torch.device("cuda:0")

# Entry-wise / norm bounds of the kernel and block tests: about 3x the worst error observed on the MI355X over this
# module's cases (observed values beside each bound), capped at 1e-4.
KERNEL_ENTRY = 1.3e-5   # observed 4.4e-6 (conv dX, 1024 wide: a K = 9 216 fp32 accumulation); aggregation, pool < 1e-6
KERNEL_NORM = 5e-6      # observed 1.7e-6 (conv fwd / dX, 1024 wide)
BN_ENTRY = 1.3e-5       # observed 4.2e-6 (d gamma at M = 237 568 rows, mean 100 / std 1); also the BatchNorm norm bound
BLOCK_ENTRY = 3e-6      # observed 9.6e-7 (a parameter gradient of the 256 -> 128 block)
BLOCK_NORM = 2.7e-6     # observed 8.8e-7


def _close(got, ref, what, entry=KERNEL_ENTRY, norm=KERNEL_NORM, floor=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if floor is not None:
        scale_n, scale_e = max(ref.norm().item(), floor), max(ref.abs().max().item(), floor)
        en = (got - ref).norm().item() / scale_n
        ee = (got - ref).abs().max().item() / scale_e
    else:
        en, ee = rel_err(got, ref), entrywise(got, ref)
    print(f"{what}: norm {en:.3g} entry {ee:.3g}")
    assert en < norm, (what, "norm", en)
    assert ee < entry, (what, "entry", ee)
    return en, ee


# ------------------------------------------------------------------------------------------ temporal convolution
@pytest.mark.parametrize("T", [1, 4, 9, 37, 128])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [64, 128, 192, 256, 1024])
def test_temporal_conv_against_fp64(C, stride, T):
    g = torch.Generator().manual_seed(C + 7 * T + stride)
    N, V = 2, 29
    x = torch.randn(N, T, V, C, generator=g)
    W = (torch.rand(C, C, 9, 1, generator=g) * 2 - 1) * (3.0 / (9 * C)) ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    To = (T - 1) // stride + 1
    dy = torch.randn(N, To, V, C, generator=g)
    xr, Wr, br = (t.double().to(DEV).requires_grad_(True) for t in (x, W, b))
    ref = SH.temporal_conv(xr, Wr, br, stride)
    ref.backward(dy.double().to(DEV))
    xd, Wd, bd, dyd = x.to(DEV), W.to(DEV), b.to(DEV), dy.to(DEV)
    out = HF.stgcn_conv(xd, HF.stgcn_weight_image(Wd, 0), bd, stride, 4)
    _close(out, ref, "conv fwd")
    runs = []
    for _ in range(2):
        dx = HF.stgcn_conv_dx(dyd, HF.stgcn_weight_image(Wd, 1), T, stride, 4)
        dW = HF.stgcn_conv_dw(xd, dyd, W.shape, stride, 4)
        db = HF.stgcn_colsum(dyd)
        runs.append((dx, dW, db))
    assert all(torch.equal(a, b_) for a, b_ in zip(*runs))
    _close(runs[0][0], xr.grad, "conv dX")
    _close(runs[0][1], Wr.grad, "conv dW")
    _close(runs[0][2], br.grad, "conv db")


@pytest.mark.parametrize("stride", [1, 2])
def test_temporal_conv_stays_inside_its_clip(stride):
    """an input (and an output gradient) that is non-zero in one clip only leaves the neighbouring clips exactly zero"""
    g = torch.Generator().manual_seed(3)
    N, T, V, C = 3, 9, 29, 64
    To = (T - 1) // stride + 1
    x = torch.zeros(N, T, V, C)
    x[1] = torch.randn(T, V, C, generator=g)
    W = torch.randn(C, C, 9, 1, generator=g).to(DEV)
    out = HF.stgcn_conv(x.to(DEV), HF.stgcn_weight_image(W, 0), None, stride, 4)
    assert out[1].abs().max().item() > 0 and out[0].abs().max().item() == 0 and out[2].abs().max().item() == 0
    dy = torch.zeros(N, To, V, C)
    dy[1] = torch.randn(To, V, C, generator=g)
    dx = HF.stgcn_conv_dx(dy.to(DEV), HF.stgcn_weight_image(W, 1), T, stride, 4)
    assert dx[1].abs().max().item() > 0 and dx[0].abs().max().item() == 0 and dx[2].abs().max().item() == 0
    # the weight gradient sees no product across the clip boundary either: x in clip 0 only, dy in clip 1 only
    x0 = torch.zeros(N, T, V, C)
    x0[0] = torch.randn(T, V, C, generator=g)
    dW = HF.stgcn_conv_dw(x0.to(DEV), dy.to(DEV), W.shape, stride, 4)
    assert dW.abs().max().item() == 0


def test_conv_refuses_other_shapes():
    x = torch.zeros(1, 4, 29, 48, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        HF.stgcn_conv(x, torch.zeros(9, 48, 64, device=DEV), None, 1, 4)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        HF.stgcn_conv(torch.zeros(1, 4, 29, 64, device=DEV), torch.zeros(9, 64, 64, device=DEV), None, 3, 4)


# ------------------------------------------------------------------------------------------ projection + aggregation
@pytest.mark.parametrize("N,T,V,Cin,Cout,imp", [
    pytest.param(2, 5, 29, 64, 64, True, id="29-64-64-True"), pytest.param(2, 5, 32, 64, 128, True, id="32-64-128-True"),
    pytest.param(2, 5, 17, 128, 64, True, id="17-128-64-True"), pytest.param(2, 5, 29, 3, 64, True, id="29-3-64-True"),
    pytest.param(2, 5, 29, 64, 64, False, id="29-64-64-False"),
    pytest.param(3, 171, 29, 64, 64, True, id="frames513-29-64-64-True")])
def test_projection_and_aggregation_against_fp64(N, T, V, Cin, Cout, imp):
    """the graph convolution: 1x1 projection with bias, then the importance-weighted aggregation; forward, input gradient,
    weight / bias gradients and the (3, V, V) importance gradient.  C_in = 3 runs the zero-padded input path.  N T = 513
    frames are one more than the 512 block images of d edge_importance: two frames per image, 257 images, the last with
    one frame."""
    g = torch.Generator().manual_seed(V + Cin)
    x = torch.randn(N, T, V, Cin, generator=g)
    W = torch.randn(3 * Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = 0.3 * torch.randn(3 * Cout, generator=g)
    A = (torch.rand(3, V, V, generator=g) < 0.2).float() * torch.rand(3, V, V, generator=g)
    E = 1.0 + 0.3 * torch.randn(3, V, V, generator=g) if imp else None
    dout = torch.randn(N, T, V, Cout, generator=g)
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, b))
    Er = E.double().requires_grad_(True) if imp else None
    y = (xr @ Wr[:, :, 0, 0].T + br).reshape(N, T, V, 3, Cout)
    ref = torch.einsum("ntvkc,kvw->ntwc", y, A.double() * Er if imp else A.double())
    ref.backward(dout.double())
    CinP = HF.pad32(Cin)
    xd, Wd, Ad, Ed = x.to(DEV), W.to(DEV), A.to(DEV), E.to(DEV) if imp else None
    xp = xd if CinP == Cin else HF.stgcn_copy_cols(xd, CinP)
    yd = HF.stgcn_conv(xp, HF.stgcn_weight_image(Wd, 0, CinP), b.to(DEV))
    out = HF.stgcn_aggregate(yd, Ad, Ed)
    _close(out, ref, "aggregate fwd")
    runs = []
    for _ in range(2):
        dy, dE = HF.stgcn_aggregate_backward(yd, dout.to(DEV), Ad, Ed, imp)
        dx = HF.stgcn_conv_dx(dy, HF.stgcn_weight_image(Wd, 1, CinP), T, 1, 0)
        if CinP != Cin:
            dx = HF.stgcn_copy_cols(dx, Cin)
        runs.append((dx, HF.stgcn_conv_dw(xp, dy, W.shape, 1, 0), HF.stgcn_colsum(dy)) + ((dE,) if imp else ()))
    assert all(torch.equal(a, b_) for a, b_ in zip(*runs))
    _close(runs[0][0], xr.grad, "aggregate dx")
    _close(runs[0][1], Wr.grad, "projection dW")
    _close(runs[0][2], br.grad, "projection db")
    if imp:
        _close(runs[0][3], Er.grad, "d edge_importance")


# ------------------------------------------------------------------------------------------ BatchNorm
def _away_from_zero(make_pre, x, gen, tries=20):
    """resample the entries of x whose pre-activation make_pre(x) is within 1e-3 of zero, until none is"""
    for _ in range(tries):
        near = make_pre(x).abs() < 1e-3
        if not near.any():
            return x
        x = torch.where(near, 100.0 + torch.randn(x.shape, generator=gen, dtype=x.dtype), x)
    raise AssertionError("could not move the pre-activations away from zero")


@pytest.mark.parametrize("res", ["none", "plain", "bn"])
@pytest.mark.parametrize("M", [58, 3712, 237568])
def test_batch_norm_against_fp64(M, res):
    """statistics, running update, apply + ReLU (+ residual, + normalised residual) and backward on columns whose mean
    (100) is far above their deviation (1): E[x^2] - E[x]^2 in fp32 fails this"""
    C = 64
    g = torch.Generator().manual_seed(M)
    x = 100.0 + torch.randn(M, C, generator=g, dtype=torch.float64)
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64), 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    r = torch.randn(M, C, generator=g, dtype=torch.float64) if res != "none" else None
    gr, br_ = 1.0 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64), 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    rm, rv = 0.1 * torch.randn(C, generator=g, dtype=torch.float64), 0.5 + torch.rand(C, generator=g, dtype=torch.float64)

    def bn(t, w, b):
        return (t - t.mean(0)) / torch.sqrt(t.var(0, unbiased=False) + 1e-5) * w + b

    def pre_of(xx):
        xx = xx.float().double()
        p = bn(xx, gamma.float().double(), beta.float().double())
        if res == "plain":
            p = p + r.float().double()
        elif res == "bn":
            p = p + bn(r.float().double(), gr.float().double(), br_.float().double())
        return p

    x = _away_from_zero(pre_of, x, g)
    f = lambda t: t.float()
    xr = f(x).double().requires_grad_(True)
    wr, br = f(gamma).double().requires_grad_(True), f(beta).double().requires_grad_(True)
    rr = f(r).double().requires_grad_(True) if r is not None else None
    pre = bn(xr, wr, br)
    if res == "plain":
        pre = pre + rr
    elif res == "bn":
        pre = pre + bn(rr, f(gr).double(), f(br_).double())
    ref = torch.relu(pre)
    dy = torch.randn(M, C, generator=g)
    ref.backward(dy.double())
    xd, rd = f(x).to(DEV), f(r).to(DEV) if r is not None else None
    rmd, rvd, nbt = f(rm).to(DEV), f(rv).to(DEV), torch.tensor(3, dtype=torch.int64, device=DEV)
    mean, rstd = HF.stgcn_bn_stats(xd, rmd, rvd, nbt)
    assert nbt.item() == 4
    _close(mean, xr.detach().mean(0), "bn mean", entry=1e-6, norm=1e-6)
    _close(rstd, 1 / torch.sqrt(xr.detach().var(0, unbiased=False) + 1e-5), "bn rstd", entry=BN_ENTRY)
    _close(rmd, 0.9 * f(rm).double() + 0.1 * xr.detach().mean(0), "running_mean", entry=1e-6, norm=1e-6)
    _close(rvd, 0.9 * f(rv).double() + 0.1 * xr.detach().var(0, unbiased=True), "running_var", entry=BN_ENTRY)
    wd, bd = f(gamma).to(DEV), f(beta).to(DEV)
    res_bn = None
    if res == "bn":
        res_bn = HF.stgcn_bn_stats(rd) + (f(gr).to(DEV), f(br_).to(DEV))
    out = HF.stgcn_bn_apply(xd, mean, rstd, wd, bd, True, rd, res_bn)
    _close(out, ref, "bn apply", entry=BN_ENTRY, norm=BN_ENTRY)
    assert torch.equal(out > 0, (ref > 0).to(DEV)), "a ReLU decision differs although every pre-activation is >= 1e-3 from 0"
    runs = [HF.stgcn_bn_backward(dy.to(DEV), out, xd, mean, rstd, wd, True) for _ in range(2)]
    assert all(torch.equal(a, b_) for a, b_ in zip(*runs))
    # dx is the difference of large terms when mean >> std: relative to the gradient's own scale
    _close(runs[0][0], xr.grad, "bn dx", entry=BN_ENTRY, norm=BN_ENTRY)
    _close(runs[0][1], wr.grad, "bn dgamma", entry=BN_ENTRY, norm=BN_ENTRY)
    _close(runs[0][2], br.grad, "bn dbeta", entry=BN_ENTRY, norm=BN_ENTRY)
    # eval mode: the running values normalise, the backward has no statistics terms
    em, er = HF.stgcn_bn_eval_stats(rmd, rvd)
    xe = xr.detach().clone().requires_grad_(True)
    ev = (xe - rmd.double().cpu()) / torch.sqrt(rvd.double().cpu() + 1e-5) * wr.detach() + br.detach()
    ev.backward(dy.double())
    _close(HF.stgcn_bn_apply(xd, em, er, wd, bd, False), ev, "bn eval apply", entry=BN_ENTRY, norm=BN_ENTRY)
    _close(HF.stgcn_bn_backward(dy.to(DEV), None, xd, em, er, wd, False)[0], xe.grad, "bn eval dx")


def test_batch_norm_refuses_a_single_row():
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        HF.stgcn_bn_stats(torch.zeros(1, 64, device=DEV))


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_pool_and_head_dropout(p):
    g = torch.Generator().manual_seed(5)
    N, R, C = 3, 4 * 29, 192
    x = torch.randn(N, R, C, generator=g)
    seed = 12345
    keep = HF.dropout_mask((N, C), seed, p, DEV).double().cpu() if p else torch.ones(N, C, dtype=torch.float64)
    if p:
        assert set(keep.unique().tolist()) == {0.0, float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))}
    xr = x.double().requires_grad_(True)
    ref = xr.mean(1) * keep
    dout = torch.randn(N, C, generator=g)
    ref.backward(dout.double())
    xd = x.to(DEV).requires_grad_(True)
    out = SB.mean_pool(xd, p, seed, None)
    out.backward(dout.to(DEV))
    _close(out, ref, "pool")
    _close(xd.grad, xr.grad, "pool dx")
    again = HF.stgcn_pool_backward(dout.to(DEV), R, p, seed, None)
    assert torch.equal(again, xd.grad) and torch.equal(HF.stgcn_pool(x.to(DEV), p, seed, None), out.detach())


# ------------------------------------------------------------------------------------------ one block at a time
def _block_params(blk, seed):
    w = SH.recipe_weights({k: v for k, v in blk.state_dict().items()}, seed)
    blk.load_state_dict(w, strict=True)
    return w


@pytest.mark.parametrize("T", [8, 13])
@pytest.mark.parametrize("ci,co,stride,residual", [(64, 64, 1, True), (64, 64, 1, False), (64, 64, 2, True), (64, 128, 1, True),
                                                   (64, 128, 2, True), (256, 128, 1, True), (256, 128, 2, True), (3, 64, 1, False)])
def test_block_against_fp64(ci, co, stride, residual, T):
    """the public block function, forward + backward, against the fp64 restatement of the block on an input whose two ReLU
    sites are both >= 1e-5 from zero everywhere (first such input seed, found in fp64 on the CPU): an order above what
    one block's fp32 rounding moves a unit-scale BatchNorm output, so the comparison is held to the arithmetic"""
    V, N = 29, 2
    blk = STGCN.Block(ci, co, stride, residual)
    kind = ["none", "identity", "conv"][blk.residual_kind]
    w = _block_params(blk, 100 + ci + co + stride)
    g = torch.Generator().manual_seed(9)
    A = ((torch.rand(3, V, V, generator=g) < 0.15).float() * torch.rand(3, V, V, generator=g))
    E = 1.0 + 0.2 * torch.randn(3, V, V, generator=g)
    for seed in range(200):
        gx = torch.Generator().manual_seed(seed)
        x = torch.randn(N, T, V, ci, generator=gx)
        dout = torch.randn(N, (T - 1) // stride + 1, V, co, generator=gx)
        rec = SH.Record()
        P = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in w.items()}
        xr, Er = x.double().requires_grad_(True), E.double().requires_grad_(True)
        ref = SH.block(xr, P, "", A.double(), Er, stride, kind, True, rec=rec)
        if rec.margin >= 1e-5:
            break
    else:
        raise AssertionError("no input seed with a ReLU margin >= 1e-5")
    ref.backward(dout.double())
    blk = blk.to(DEV)
    outs = []
    for _ in range(2):
        blk.load_state_dict(w, strict=True)
        blk.zero_grad()
        xd, Ed = x.to(DEV).requires_grad_(True), E.to(DEV).requires_grad_(True)
        out = SB.st_gcn_block(xd, blk, A.to(DEV), Ed, training=True)
        out.backward(dout.to(DEV))
        outs.append([out.detach(), xd.grad, Ed.grad] + [p.grad for p in blk.parameters()] + [b.clone() for b in blk.buffers()])
    assert all(torch.equal(a, b_) for a, b_ in zip(*outs))
    _close(out, ref, "block out", BLOCK_ENTRY, BLOCK_NORM)
    assert torch.equal(out > 0, (ref > 0).to(DEV))
    _close(xd.grad, xr.grad, "block dx", BLOCK_ENTRY, BLOCK_NORM)
    _close(Ed.grad, Er.grad, "block dE", BLOCK_ENTRY, BLOCK_NORM)
    zero = SH.zero_grad_biases([n for n, _ in blk.named_parameters()])
    for n, p in blk.named_parameters():
        floor = P[zero[n]].grad.norm().item() if n in zero else None
        _close(p.grad, P[n].grad, "block d " + n, BLOCK_ENTRY, BLOCK_NORM, floor=floor)
    sd = blk.state_dict()
    for k, v in rec.stats.items():
        if v.is_floating_point():
            _close(sd[k], v, "block " + k, BLOCK_ENTRY, BLOCK_NORM)
        else:
            assert sd[k].item() == v.item(), k


# ------------------------------------------------------------------------------------------ whole model
def _model(name, dropout=0.0):
    cfg = SH.CONFIGS[name]
    m = hw.STGCNModel(*SH.model_args(cfg, dropout))
    w = SH.fixture_weights(m.state_dict(), cfg)
    m.load_state_dict(w, strict=False)
    return m.to(DEV), dict(w, A=m.A.detach().cpu()), cfg


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_model_forward_quantities_against_fixture(name):
    fx = load_fixture(f"stgcn_{name}.npz")
    m, w, cfg = _model(name)
    x, y = (t.to(DEV) for t in SH.fixture_input(fx, cfg))
    crit = train.SmoothedCrossEntropyLoss()
    m.eval()
    with torch.no_grad():
        logits = m(x)
    assert rel_err(logits.cpu(), fx["eval.logits"]) < 2e-5, rel_err(logits.cpu(), fx["eval.logits"])
    assert abs(crit(logits, y).item() - float(fx["eval.loss"])) < 2e-5 * max(1.0, abs(float(fx["eval.loss"])))
    m.train()
    m.block_tap = []
    with torch.no_grad():
        logits = m(x)
    assert rel_err(logits.cpu(), fx["train.logits"]) < 2e-5, rel_err(logits.cpu(), fx["train.logits"])
    assert abs(crit(logits, y).item() - float(fx["train.loss"])) < 2e-5 * max(1.0, abs(float(fx["train.loss"])))
    for i, h in enumerate(m.block_tap):
        e = rel_err(SH.block_samples(h).cpu(), fx[f"train.block{i}"])
        assert e < 2e-5, (i, e)
    sd = m.state_dict()
    n_stats = 0
    for k in fx:
        if k.startswith("train.stat."):
            key = k[len("train.stat."):]
            n_stats += 1
            if key.endswith("num_batches_tracked"):
                assert sd[key].item() == int(fx[k]) == 4, key
            else:
                assert rel_err(sd[key].cpu(), fx[k]) < 2e-5, (key, rel_err(sd[key].cpu(), fx[k]))
    assert n_stats == 3 * sum(1 for k in sd if k.endswith("running_mean"))


def _digest_errors(name, g, fx, prefix, floor=0.0):
    gd = g.detach().double().flatten().cpu()
    ref_norm = float(fx[prefix + "gn." + name][0])
    scale = max(ref_norm, floor, 1e-30)
    e1 = abs(gd.norm().item() - ref_norm) / scale
    # the error's +-1 projections have mean square |error|^2: their RMS estimates the L2 distance to the reference
    e3 = float(np.sqrt(np.mean((probe_vectors(name, gd.numel()) @ gd.numpy() - fx[prefix + "gp." + name]) ** 2))) / scale
    return e1, e3


def _model_grads(m, x, y, training):
    m.train(training)
    m.zero_grad()
    train.SmoothedCrossEntropyLoss()(m(x), y).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_model_gradients_tight(name, training):
    """margin-selected fixtures: every parameter gradient within max(2e-5, 4 x the reference's own fp32-vs-fp64
    deviation) of the reference's; the analytically zero train-mode biases against the floor (the matching weight
    gradient's norm)"""
    fx = load_fixture(f"stgcn_{name}.npz")
    m, _, _ = _model(name)
    tag = "train." if training else "eval."
    grads = _model_grads(m, *(t.to(DEV) for t in SH.fixture_input(fx, SH.CONFIGS[name])), training)
    zero = SH.zero_grad_biases(grads) if training else {}
    worst = ("", 0.0)
    for n, g in grads.items():
        tol = max(2e-5, 4.0 * float(fx[f"refdev.{tag}g.{n}"]))
        if n in zero:
            floor = float(fx[tag + "gn." + zero[n]][0])
            e = g.double().norm().item() / floor
            assert e < tol, (n, "zero-gradient bias against the floor", e)
            continue
        e = grad_digest_check({n: g}, fx, tag, tol)
        worst = max(worst, (n, e), key=lambda t: t[1])
    print("worst gradient digest error", worst)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_model_gradients_wiring(name, training):
    """every parameter gradient within the wiring bound (4 x the largest flip-induced fp32-vs-fp64 deviation of the
    reference over 20 inputs of shape d) of the reference's: a wrong residual, stride, tap order or importance product
    moves a gradient by order 1"""
    fx = load_fixture(f"stgcn_{name}.npz")
    bound = float(load_fixture("stgcn_d.npz")["wiring_bound"])
    assert 0 < bound < 0.1
    m, _, _ = _model(name)
    tag = "train." if training else "eval."
    grads = _model_grads(m, *(t.to(DEV) for t in SH.fixture_input(fx, SH.CONFIGS[name])), training)
    zero = SH.zero_grad_biases(grads) if training else {}
    for n, g in grads.items():
        floor = float(fx[tag + "gn." + zero[n]][0]) if n in zero else 0.0
        e1, e3 = _digest_errors(n, g, fx, tag, floor)
        assert e1 < bound and e3 < bound, (n, e1, e3, bound)


def test_head_dropout_mask_and_interleaved_forwards():
    m, w, cfg = _model("b", dropout=0.25)
    x, y = SH.make_input(cfg, seed=3)
    xa, xb, yd = x.to(DEV), x.flip(0).contiguous().to(DEV), y.to(DEV)
    crit = train.SmoothedCrossEntropyLoss()
    m.train()
    torch.manual_seed(11)
    m._drop_calls = 0
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    logits = m(xa)
    keep = HF.dropout_mask((cfg["B"], cfg["n_out"]), m._seeds(0)[0], 0.25, DEV).double().cpu()
    assert abs(float((keep != 0).double().mean()) - 0.75) < 0.11          # 256 draws: 4 sigma
    ref = SH.restate(w, x, cfg, training=True, head_keep=keep)
    assert rel_err(logits.detach().cpu(), ref) < 2e-5, rel_err(logits.detach().cpu(), ref)
    crit(logits, yd).backward()
    alone = [p.grad.clone() for p in m.parameters()]
    # forwards A, B, then backward A: bit for bit the gradient of A alone (B redraws the seed word, not A's copy of it)
    m.load_state_dict(sd0)
    m.zero_grad()
    m._drop_calls = 0
    la = m(xa)
    m(xb)
    crit(la, yd).backward()
    assert all(torch.equal(p.grad, q) for p, q in zip(m.parameters(), alone))


def test_graphed_eval_bit_equal():
    m, _, cfg = _model("a")
    m.eval()
    x, _ = SH.make_input(cfg)
    x = x.to(DEV)
    fast = serve.GraphedEval(m, x)
    with torch.no_grad():
        ref = m(x)
    assert torch.equal(fast(x), ref)


def test_graphed_train_step_equals_eager():
    cfg = SH.CONFIGS["a"]
    x, y = SH.make_input(cfg)
    x, y = x.to(DEV), y.to(DEV)
    ms = [_model("a", dropout=0.05)[0].train() for _ in range(2)]
    opts = [torch.optim.AdamW(m.parameters(), lr=torch.tensor(3e-4, device=DEV), fused=True, capturable=True) for m in ms]
    scheds = [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in opts]
    torch.manual_seed(5)
    eager = train.TrainStep(ms[0], opts[0])
    graphed = train.GraphedTrainStep(ms[1], opts[1], x, y)
    nbt = "st_gcn_networks.3.tcn.3.num_batches_tracked"
    rv = "st_gcn_networks.3.tcn.3.running_var"
    for i in range(5):
        before = (ms[1].state_dict()[nbt].item(), ms[1].state_dict()[rv].clone())
        le, lg = eager(x, y), graphed(x, y)
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert ms[1].state_dict()[nbt].item() == before[0] + 1 and not torch.equal(ms[1].state_dict()[rv], before[1])
        if i == 2:
            for s in scheds:
                s.step()
    assert all(torch.equal(p, q) for p, q in zip(ms[0].parameters(), ms[1].parameters()))


def test_adamw_trajectory_tracks_fp64():
    """20 AdamW steps from fixture a's weights follow the fp64 restatement; the bound is 4 x the reference's own
    fp32-vs-fp64 drift over the same 20 steps (worst of 5 inputs, flips included), measured by the fixture generator"""
    fx = load_fixture("stgcn_a.npz")
    loss_bound, w_bound = 4 * float(fx["adamw.loss_dev"]), 4 * float(fx["adamw.w_dev"])
    m, w, cfg = _model("a")
    m.train()
    x, y = SH.make_input(cfg, seed=100)
    opt = torch.optim.AdamW(m.parameters(), lr=3e-4)
    names = [n for n, _ in m.named_parameters()]
    P = {k: (v.double().clone().requires_grad_(k in names) if v.is_floating_point() else v.clone()) for k, v in w.items()}
    ref_opt = torch.optim.AdamW([P[n] for n in names], lr=3e-4)
    step = train.TrainStep(m, opt)
    for i in range(20):
        loss = step(x.to(DEV), y.to(DEV)).item()
        ref_opt.zero_grad()
        rec = SH.Record()
        rl = SH.smoothed_ce(SH.restate(P, x, cfg, training=True, rec=rec), y)
        rl.backward()
        ref_opt.step()
        for k, v in rec.stats.items():
            P[k] = v
        assert abs(loss - rl.item()) < loss_bound * max(1.0, abs(rl.item())), (i, loss, rl.item())
    for n, p in m.named_parameters():
        assert rel_err(p.detach().cpu(), P[n].detach()) < w_bound, (n, rel_err(p.detach().cpu(), P[n].detach()))


def test_full_size_train_step_is_reproducible():
    """B = 64, T = 128: one train step runs, is finite, and loss and gradients repeat bit for bit"""
    hp = hw.STGCNParams({"num_class": 2002}, 2)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(64, 128, 29, 2, generator=g).to(DEV)
    y = torch.randint(0, 2002, (64,), generator=g).to(DEV)
    torch.manual_seed(1)
    m = hw.STGCNModel(*hp.get_model_params()).to(DEV).train()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    res = []
    for _ in range(2):
        m.load_state_dict(sd0)
        m._drop_calls = 0
        step = train.TrainStep(m)
        m.zero_grad()
        loss = step(x, y)
        assert torch.isfinite(loss).item()
        res.append([loss.clone()] + [p.grad.clone() for p in m.parameters()])
    assert all(torch.isfinite(t).all().item() for t in res[0])
    assert all(torch.equal(a, b) for a, b in zip(*res))
