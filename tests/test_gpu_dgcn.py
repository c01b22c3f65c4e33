"""GPU parity of the DecoupledGCN baseline: every new HIP kernel through its functional wrapper against fp64 torch (entry by
entry and in norm), one unit at a time through dgcn_block.dgcn_unit against the fp64 restatement of tests/dgcn_helpers.py,
and the whole `DecoupledGCNModel` against the reference-generated fixtures tests/golden/dgcn_{a,b,c,d}.npz.

Bounds.  Kernel and unit checks use max(4 x d, K): d is the deviation of the same computation run in fp32 on the CPU from
the fp64 one on the same inputs, computed in the test, and K the ST-GCN kernel bounds KERNEL_ENTRY / KERNEL_NORM of
tests/test_gpu_stgcn.py (copied below).  Model-level gradient checks use max(2e-5, 4 x refdev) from the fixture on the
margin-selected fixtures a-c and the fixture's wiring bound on all four, as the ST-GCN tests do."""
import importlib

import numpy as np
import pytest
import torch

import dgcn_helpers as DH
from helpers import load_fixture, rel_err, probe_vectors

pytestmark = pytest.mark.gpu

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
serve = importlib.import_module("sl-hwgat_amd.serve")
DB = importlib.import_module("sl-hwgat_amd.dgcn_block")
DGCN = importlib.import_module("sl-hwgat_amd.models.DecoupledGCN")
DEV = torch.device("cuda:0")

# tests/test_gpu_stgcn.py: KERNEL_ENTRY = 1.3e-5, KERNEL_NORM = 5e-6 (about 3 x the worst error observed there).
# Observed worst on the MI355X over this module's cases (norm / entry): aggregation 1.7e-7 / 4.3e-7 (d An); gates
# 1.6e-7 / 2.0e-7 (d s_t); DropGraph probabilities 1.2e-7 / 2.3e-7 at the kernel, 3.8e-7 / 9.0e-7 in the whole model
# (l10), mask factors 4.6e-8, scales exact; merge 7.8e-8 / 1.6e-7 and its gradients 8.6e-8 / 1.6e-7; one unit below 1.3e-6
# on every tensor.  A gate convolution's one bias gradient, at the scale of its own sum: at most 3.7e-7 of sum |dz| in
# the unit cases (the sum itself 1.8e-4 .. 0.5 of its terms: at 1.8e-4 an error of 2.0e-7 of the terms is 1.1e-3 of the
# value), 6.5e-6 in the whole model (bound 2e-5).  Whole model: logits 2.9e-7 .. 7.3e-7 of the fixtures', tight gradient
# digests at most 6.0e-6 (heads of the nearly cancelling bn0.bias gradients 2.2e-3, inside 4 x the reference's own head
# deviation; every other head inside 10 x tol), wiring errors at most 7.6e-3 (fixture d) against the bound 5.2e-2.
# AdamW: loss deviation 0.36 against 4 x 0.32 -- the reference's own fp32 and fp64 trajectories part by a factor of
# about ten per step from the third step on, with DropGraph or at keep_prob 1 and at any learning rate down to 1e-5
# (B = 2 is fitted within a few steps and Adam turns every near-zero gradient entry into a full step), so past the
# first steps this check can only catch a gross error; the per-step gradients are pinned by the tests above it.
KERNEL_ENTRY = 1.3e-5
KERNEL_NORM = 5e-6
E = DH.EDGES_29


def _close(got, ref, what, ref32=None, floor=None, entry=KERNEL_ENTRY, norm=KERNEL_NORM):
    """entry-wise and norm comparison of `got` with the fp64 `ref`; bounds max(4 x d, K), d the deviation of the fp32 CPU
    computation `ref32` from `ref` (K alone without it)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    scale_n = max(ref.norm().item(), floor or 0.0, 1e-300)
    scale_e = max(ref.abs().max().item(), floor or 0.0, 1e-300)
    en, ee = (got - ref).norm().item() / scale_n, (got - ref).abs().max().item() / scale_e
    if ref32 is not None:
        r32 = ref32.detach().double().cpu()
        norm = max(norm, 4 * (r32 - ref).norm().item() / scale_n)
        entry = max(entry, 4 * (r32 - ref).abs().max().item() / scale_e)
    print(f"{what}: norm {en:.3g} (bound {norm:.3g}) entry {ee:.3g} (bound {entry:.3g})")
    assert en < norm, (what, "norm", en, norm)
    assert ee < entry, (what, "entry", ee, entry)
    return en, ee


def _close_gate_bias(got, ref, terms, what, ref32=None, bound=KERNEL_ENTRY):
    """a gate convolution's one bias gradient against the fp64 `ref` at the scale of its own sum, `terms` = sum |dz|:
    bound max(4 x d, K_entry), d the deviation of the fp32 CPU `ref32` at the same scale"""
    e, left = DH.gate_bias_error(got, ref, terms)
    if ref32 is not None:
        bound = max(bound, 4 * DH.gate_bias_error(ref32, ref, terms)[0])
    print(f"{what}: {e:.3g} of its terms (bound {bound:.3g}); the sum is {left:.3g} of them, off by {e / max(left, 1e-300):.3g}")
    assert e < bound, (what, e, bound)
    return e


# ------------------------------------------------------------------------------------------ aggregation
def _agg_reference(y, An, d, dtype):
    """(out, dy, dAn) of the decoupled aggregation in `dtype` on the CPU"""
    yr, Ar = y.to(dtype).requires_grad_(True), An.to(dtype).requires_grad_(True)
    N, T, V, C3 = y.shape
    C, G = C3 // 3, An.shape[1]
    out = torch.einsum("ntvkc,kcvw->ntwc", yr.reshape(N, T, V, 3, C), Ar.repeat(1, C // G, 1, 1))
    out.backward(d.to(dtype))
    return out.detach(), yr.grad, Ar.grad


@pytest.mark.parametrize("NT", [1, 58, 129, 300])
@pytest.mark.parametrize("V,C,G", [(29, 64, 8), (32, 128, 4), (17, 64, 1), (29, 256, 8)])
def test_aggregation_against_fp64(V, C, G, NT):
    """NT 129 and 300 exceed the 128 block images of d An: two frames per image with a short last one (65 images), and
    three frames per image (100 images); groups 8 of 64 and 4 of 128 channels are ragged 8- and 32-channel chunks"""
    g = torch.Generator().manual_seed(V + C + G + NT)
    y = torch.randn(1, NT, V, 3 * C, generator=g)
    An = torch.rand(3, G, V, V, generator=g) * (torch.rand(3, G, V, V, generator=g) < 0.3).float()
    d = torch.randn(1, NT, V, C, generator=g)
    ref, ref32 = _agg_reference(y, An, d, torch.float64), _agg_reference(y, An, d, torch.float32)
    yd, Ad, dd = y.to(DEV), An.to(DEV), d.to(DEV)
    out = HF.dgcn_aggregate(yd, Ad, G)
    _close(out, ref[0], "aggregate fwd", ref32[0])
    runs = [HF.dgcn_aggregate_backward(yd, dd, Ad, G, True) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    _close(runs[0][0], ref[1], "aggregate dy", ref32[1])
    _close(runs[0][1], ref[2], "aggregate dAn", ref32[2])
    assert HF.dgcn_aggregate_backward(yd, dd, Ad, G, False)[1] is None


def test_aggregation_keeps_the_groups_apart():
    """every group has its own adjacency and group 2's is zero: a wrong c mod G mapping or any mixing of groups shows entry
    by entry, and the channels of group 2 come out exactly zero"""
    g = torch.Generator().manual_seed(5)
    V, C, G, NT = 29, 64, 8, 3
    base = torch.rand(3, 1, V, V, generator=g)
    An = base * torch.arange(1, G + 1).view(1, G, 1, 1).float() + torch.rand(3, G, V, V, generator=g)
    An[:, 2] = 0
    y = torch.randn(1, NT, V, 3 * C, generator=g)
    d = torch.randn(1, NT, V, C, generator=g)
    ref, ref32 = _agg_reference(y, An, d, torch.float64), _agg_reference(y, An, d, torch.float32)
    out = HF.dgcn_aggregate(y.to(DEV), An.to(DEV), G)
    dy, dAn = HF.dgcn_aggregate_backward(y.to(DEV), d.to(DEV), An.to(DEV), G, True)
    for grp in range(G):
        _close(out[..., grp::G], ref[0][..., grp::G], f"group {grp} fwd", ref32[0][..., grp::G], floor=1e-30)
        _close(dAn[:, grp], ref[2][:, grp], f"group {grp} dAn", ref32[2][:, grp])
    assert out[..., 2::G].abs().max().item() == 0.0
    assert dy.view(1, NT, V, 3, C)[..., 2::G].abs().max().item() == 0.0
    _close(dy, ref[1], "dy", ref32[1])


# ------------------------------------------------------------------------------------------ gates
def _gate_reference(h, sv, st, sc, dh3, dm1, dm0, dtype):
    """the squeezes, h3 and the gradients of  sum dh3 h3 + sum dm1 m1 + sum dm0 m0  in `dtype` on the CPU"""
    hr, a, b, c = (t.to(dtype).requires_grad_(True) for t in (h, sv, st, sc))
    m0 = hr.mean(1)
    h1 = hr * (1 + a[:, None, :, None])
    m1 = h1.mean(2)
    h2 = h1 * (1 + b[:, :, None, None])
    m2 = h2.mean(2).mean(1)
    h3 = h2 * (1 + c[:, None, None, :])
    (h3 * dh3.to(dtype)).sum().backward(retain_graph=True)
    direct = (hr.grad.clone(), a.grad.clone(), b.grad.clone(), c.grad.clone())
    ((m1 * dm1.to(dtype)).sum() + (m0 * dm0.to(dtype)).sum()).backward()
    return dict(m0=m0.detach(), m1=m1.detach(), m2=m2.detach(), h3=h3.detach(), dh_direct=direct[0], dsv_direct=direct[1],
                dst=direct[2], dsc=direct[3], dh=hr.grad, dsv=a.grad)


@pytest.mark.parametrize("N,T,V,C", [(2, 1, 29, 64), (2, 9, 29, 64), (3, 8, 17, 128), (2, 4, 32, 256)])
def test_gates_against_fp64(N, T, V, C):
    g = torch.Generator().manual_seed(N + T + V + C)
    h = torch.randn(N, T, V, C, generator=g)
    sv, st, sc = torch.rand(N, V, generator=g), torch.rand(N, T, generator=g), torch.rand(N, C, generator=g)
    dh3 = torch.randn(N, T, V, C, generator=g)
    dm1, dm0 = torch.randn(N, T, C, generator=g), torch.randn(N, V, C, generator=g)
    R, R32 = (_gate_reference(h, sv, st, sc, dh3, dm1, dm0, dt) for dt in (torch.float64, torch.float32))
    hd, svd, std, scd, dd, dm1d, dm0d = (t.to(DEV) for t in (h, sv, st, sc, dh3, dm1, dm0))
    got = {}
    got["m0"] = HF.dgcn_gate_sum(hd, 0, 1.0 / T)
    got["m1"] = HF.dgcn_gate_sum(hd, 1, 1.0 / V, sv=svd)
    got["m2"] = ((1.0 + std).unsqueeze(-1) * got["m1"]).mean(dim=1)
    got["h3"] = HF.dgcn_gate_apply(hd, svd, std, scd)
    u = HF.dgcn_gate_sum(hd, 1, 1.0, g=dd, sv=svd)
    got["dsc"] = ((1.0 + std).unsqueeze(-1) * u).sum(dim=1)
    got["dst"] = ((1.0 + scd).unsqueeze(1) * u).sum(dim=2)
    got["dsv_direct"] = HF.dgcn_gate_sum(hd, 0, 1.0, g=dd, st=std, sc=scd).sum(dim=2)
    got["dsv"] = HF.dgcn_gate_sum(hd, 0, 1.0, g=dd, st=std, sc=scd, m=dm1d, m_scale=1.0 / V).sum(dim=2)
    got["dh_direct"] = HF.dgcn_gate_backward(dd, svd, std, scd, None, None)
    got["dh"] = HF.dgcn_gate_backward(dd, svd, std, scd, dm1d, dm0d)
    for k, v in got.items():
        _close(v, R[k], "gate " + k, R32[k])
        for n in range(N):                               # one clip against another: a gate read from the wrong clip fails
            _close(v[n], R[k][n], f"gate {k} clip {n}", R32[k][n])
    # by row (a frame) and by column (a joint) of the two full-size results
    for k in ("h3", "dh"):
        for t in range(T):
            _close(got[k][:, t], R[k][:, t], f"gate {k} frame {t}", R32[k][:, t])
        for v in range(0, V, 7):
            _close(got[k][:, :, v], R[k][:, :, v], f"gate {k} joint {v}", R32[k][:, :, v])


# ------------------------------------------------------------------------------------------ DropGraph
def _graph_A():
    return DGCN.Unit(64, 64, DGCN.spatial_graph(29, E), 8, 29).A.detach()


@pytest.mark.parametrize("res_bn", [False, True])
@pytest.mark.parametrize("block,T", [(41, 4), (41, 13), (41, 24), (5, 4), (5, 13), (5, 24), (3, 4), (3, 13), (3, 24)])
def test_drop_graph_against_fp64(block, T, res_bn):
    """explicit seeds: spatial at a leaf (joint 1), a hub (joint 9), nowhere, and everywhere but joint 28; temporal at frame
    0, the last frame, the middle and nowhere -- so a clip without a seed stands beside fully blanked ones (block 41,
    T <= 21).  Probabilities, masks (exact), scales, the merged output and both gradients."""
    g = torch.Generator().manual_seed(block * 100 + T)
    N, V, C, keep, drop_size = 4, 29, 64, 0.9, DH.find_drop_size(29, len(E))
    A = _graph_A()
    c, r, dout = (torch.randn(N, T, V, C, generator=g) for _ in range(3))
    bn = [0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g),
          0.1 * torch.randn(C, generator=g)]
    rbn = [0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g),
           0.1 * torch.randn(C, generator=g)] if res_bn else None
    sp = torch.zeros(N, V)
    sp[0, 1], sp[1, 9], sp[3, :28] = 1, 1, 1
    tp = torch.zeros(N, T)
    tp[0, 0], tp[1, T - 1], tp[2, T // 2] = 1, 1, 1
    seeds = {(7, 0): sp, (7, 1): tp, (7, 2): sp.roll(1, 0), (7, 3): tp.roll(1, 0)}

    def reference(dtype):
        read = lambda x, p: x if p is None else (x - p[0].to(dtype)) * p[1].to(dtype) * p[2].to(dtype) + p[3].to(dtype)
        a = read(c.to(dtype), bn).requires_grad_(True)
        q = read(r.to(dtype), rbn).requires_grad_(True)
        log = []
        s64 = {k: v.to(dtype) for k, v in seeds.items()}
        pre = DH.drop_graph(a, A.to(dtype), keep, drop_size, 41, 7, 0, s64, log) + \
            DH.drop_graph(q, A.to(dtype), keep, drop_size, block, 7, 2, s64, log)
        return a, q, pre, log

    a64, q64, pre64, log64 = reference(torch.float64)
    a32, q32, pre32, log32 = reference(torch.float32)
    tap = []
    cd, rd = c.to(DEV), r.to(DEV)
    bnd = tuple(t.to(DEV) for t in bn)
    rbnd = tuple(t.to(DEV) for t in rbn) if res_bn else None
    inj = {k: v.to(DEV) for k, v in seeds.items()}
    fs1, ft1 = DB.drop_masks(cd, bnd, A.to(DEV), keep, drop_size, 41, (0, 0), None, inj, tap, (7, 0))
    fs2, ft2 = DB.drop_masks(rd, rbnd, A.to(DEV), keep, drop_size, block, (0, 0), None, inj, tap, (7, 2))
    assert len(tap) == 4
    for rec, l64, l32 in zip(tap, log64, log32):
        unit, site, p, s, mask, scale = l64
        assert (rec["unit"], rec["site"]) == (unit, site)
        _close(rec["p"], p, f"p site {site}", l32[2])
        assert torch.equal((rec["factor"] != 0).cpu(), mask != 0), site                    # the mask, exactly
        assert 0 < mask.sum() < mask.numel()
        _close(rec["scale"], torch.as_tensor([float(scale)]), f"scale site {site}")
        _close(rec["factor"], mask * scale, f"factor site {site}")
    out = HF.dgcn_merge(cd, bnd, rd, rbnd, fs1, ft1, fs2, ft2)
    _close(out, torch.relu(pre64), "merge out", torch.relu(pre32))
    # the gradients, held on the kernel's side of the ReLU
    gate = (out > 0).cpu()
    (pre64 * (dout.double() * gate)).sum().backward()
    (pre32 * (dout * gate)).sum().backward()
    dz1, dz2 = HF.dgcn_merge_backward(dout.to(DEV), out, fs1, ft1, fs2, ft2)
    _close(dz1, a64.grad, "merge dz1", a32.grad)
    _close(dz2, q64.grad, "merge dz2", q32.grad)
    # a fully blanked clip is exactly zero, forward and backward
    blank = [n for n in range(N) if float(log64[1][4][n].sum()) == 0 and float(log64[3][4][n].sum()) == 0]
    for n in blank:
        assert out[n].abs().max().item() == 0 and dz1[n].abs().max().item() == 0 and dz2[n].abs().max().item() == 0
    if block == 41 and T <= 13:
        assert blank


def test_masked_sum():
    g = torch.Generator().manual_seed(1)
    a, ma, b, mb = (torch.randn(3, 5, 29, 64, generator=g).to(DEV) for _ in range(4))
    assert torch.equal(HF.dgcn_masked_sum(a, ma, b, mb), a * (ma > 0) + b * (mb > 0))
    assert torch.equal(HF.dgcn_masked_sum(a, ma, b, None), a * (ma > 0) + b)


# ------------------------------------------------------------------------------------------ seed draw
def test_seed_draw():
    n = 65536
    base = torch.tensor([12345], dtype=torch.int32, device=DEV)
    full = lambda v: torch.full((n,), v, device=DEV)
    assert HF.dgcn_draw(full(0.0), 77, base).sum().item() == 0
    assert HF.dgcn_draw(full(1.0), 77, base).sum().item() == n and HF.dgcn_draw(full(1.5), 77, base).sum().item() == n
    d03, d15 = HF.dgcn_draw(full(0.03), 77, base), HF.dgcn_draw(full(0.15), 77, base)
    assert ((d03 == 0) | (d03 == 1)).all() and ((d15 - d03) >= 0).all()                   # a subset at the smaller p
    assert torch.equal(d15, HF.dgcn_draw(full(0.15), 77, base))                            # the same base word repeats
    other = HF.dgcn_draw(full(0.15), 77, base + 1)
    assert not torch.equal(d15, other) and not torch.equal(d15, HF.dgcn_draw(full(0.15), 78, base))
    assert torch.equal(HF.dgcn_draw(full(0.15), 78, base), HF.dgcn_draw(full(0.15), 77, base + 1))   # seed + base word
    for p, d in ((0.03, d03), (0.15, d15), (0.15, other)):
        count, dev = d.sum().item(), 5 * (n * p * (1 - p)) ** 0.5
        print(f"draw p {p}: {count} seeds, expected {n * p:.0f} +- {dev:.0f}")
        assert abs(count - n * p) < dev
    # a per-element probability: seeds only where p > 0
    p = torch.zeros(n, device=DEV)
    p[::2] = 0.5
    d = HF.dgcn_draw(p, 5, None)
    assert d[1::2].sum().item() == 0 and abs(d[::2].sum().item() - n / 4) < 5 * (n / 8) ** 0.5


# ------------------------------------------------------------------------------------------ one unit
# The two one-channel gate convolutions have ONE bias each, d bias = sum_{n, l} dz[n, l] over terms of both signs: it is
# judged at the scale of its own sum, sum |dz| (dgcn_helpers.gate_biases; the restatement records the terms), against
# the same max(4 x d, K_entry) as every entry, d the fp32 CPU restatement's deviation at that scale.
GATE_BIASES = ("conv_sa.bias", "conv_ta.bias")
UNIT_SHAPES = [(2, 64, 1, False), (64, 64, 1, True), (64, 128, 2, True), (256, 256, 1, True)]
# DropGraph needs a skip path (the reference raises without one: it never drops in l1), so the unit without a residual
# runs in eval and train mode only
UNIT_CASES = [(ci, co, s, r, T, mode) for ci, co, s, r in UNIT_SHAPES for T in (8, 13) for mode in ("eval", "train", "drop")
              if r or mode != "drop"]


@pytest.mark.parametrize("ci,co,stride,residual,T,mode", UNIT_CASES)
def test_unit_against_fp64(ci, co, stride, residual, T, mode):
    """one unit through dgcn_block.dgcn_unit against the fp64 restatement: output, input gradient, every parameter
    gradient and the running statistics.  The input seed is walked until every ReLU of the fp64 run has a margin >= 1e-5,
    the fp32 restatement then takes the fp64 run's ReLU masks, and the kernel's own decisions are asserted equal to them:
    the comparison stays on one side of every ReLU."""
    N, V, G, block = 2, 29, 8, 5
    training = mode != "eval"
    unit = DGCN.Unit(ci, co, DGCN.spatial_graph(V, E), G, V, stride=stride, residual=residual)
    kind = ["none", "identity", "conv"][unit.residual_kind]
    w = DH.recipe_weights(unit.state_dict(), 300 + ci + co + stride)
    To = (T - 1) // stride + 1
    cfg = dict(seed=900 + ci)
    seeds = {(7, s): DH.drop_seed_pattern(cfg, 7, s, (N, V) if s % 2 == 0 else (N, To)) for s in range(4)}
    drop_size = DH.find_drop_size(V, len(E))
    drop = (0.9, drop_size, block, 7, seeds) if mode == "drop" else None

    def run(x, dout, dtype, masks=None, rec=None):
        P = {k: (v.detach().clone().to(dtype).requires_grad_(DH.is_trainable(k, v)) if v.is_floating_point() else v)
             for k, v in w.items()}
        xr = x.detach().clone().to(dtype).requires_grad_(True)
        out = DH.unit(xr, P, "", G, stride, kind, training, drop, masks, rec)
        out.backward(dout.to(dtype))
        return out.detach(), xr.grad, {k: v.grad for k, v in P.items() if torch.is_tensor(v) and v.requires_grad}

    for seed in range(200):
        gx = torch.Generator().manual_seed(seed)
        x = torch.randn(N, T, V, ci, generator=gx)
        dout = torch.randn(N, To, V, co, generator=gx)
        rec = DH.Record()
        ref = run(x, dout, torch.float64, rec=rec)
        if rec.margin >= 1e-5:
            break
    else:
        raise AssertionError("no input seed with a ReLU margin >= 1e-5")
    ref32 = run(x, dout, torch.float32, masks=rec.masks)
    unit = unit.to(DEV)
    outs = []
    for _ in range(2):
        unit.load_state_dict(w, strict=True)
        unit.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        d = None
        if mode == "drop":
            d = (0.9, drop_size, block, (1, 2, 3, 4), None, {k: v.to(DEV) for k, v in seeds.items()}, None, 7)
        out = DB.dgcn_unit(xd, unit, training, d)
        out.backward(dout.to(DEV))
        outs.append([out.detach(), xd.grad] + [p.grad for p in unit.parameters() if p.requires_grad] +
                    [b.clone() for b in unit.buffers()])
    assert all(torch.equal(a, b_) for a, b_ in zip(*outs))
    _close(out, ref[0], "unit out", ref32[0])
    assert torch.equal(out > 0, (ref[0] > 0).to(DEV))
    _close(xd.grad, ref[1], "unit dx", ref32[1])
    zero = DH.zero_grad_biases(ref[2]) if training else {}
    named = dict(unit.named_parameters())
    for n, p in named.items():
        if not p.requires_grad:
            assert p.grad is None
            continue
        if n in GATE_BIASES:
            continue
        floor = ref[2][zero[n]].norm().item() if n in zero else None
        _close(p.grad, ref[2][n], "unit d " + n, ref32[2][n], floor=floor)
    for b in GATE_BIASES:
        _close_gate_bias(named[b].grad, ref[2][b], rec.terms[b], "unit d " + b, ref32[2][b])
    sd = unit.state_dict()
    for k, v in rec.stats.items():
        if v.is_floating_point():
            _close(sd[k], v, "unit " + k)
        else:
            assert sd[k].item() == v.item(), k
    assert training == bool(rec.stats)


# ------------------------------------------------------------------------------------------ whole model
def _model(name, dropout=0.0):
    cfg = DH.CONFIGS[name]
    m = hw.DecoupledGCNModel(*DH.model_args(cfg, dropout))
    w = DH.fixture_weights(m.state_dict(), cfg)
    m.load_state_dict(w, strict=True)
    return m.to(DEV), w, cfg


def _inject(m, cfg, B=None, T=None):
    m.drop_seeds = {k: v.float().to(DEV) for k, v in DH.all_drop_seeds(cfg, B, T).items()}


def _fx_bound(fx, key):
    return max(2e-5, 4.0 * float(fx[key]))


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_model_forward_quantities_against_fixture(name):
    fx = load_fixture(f"dgcn_{name}.npz")
    m, w, cfg = _model(name)
    x, y = (t.to(DEV) for t in DH.fixture_input(fx, cfg))
    crit = train.SmoothedCrossEntropyLoss()
    m.eval()
    m.drop_tap = []
    with torch.no_grad():
        logits = m(x)
    assert not m.drop_tap                                                       # eval mode: DropGraph is the identity
    e = rel_err(logits.cpu(), fx["eval.logits"])
    print("eval logits", e)
    assert e < _fx_bound(fx, "refdev.eval.logits"), e
    assert abs(crit(logits, y).item() - float(fx["eval.loss"])) < _fx_bound(fx, "refdev.eval.loss") * max(1.0, abs(float(fx["eval.loss"])))
    m.train()
    _inject(m, cfg)
    m.block_tap, m.drop_tap = [], []
    with torch.no_grad():
        logits = m(x, DH.KEEP_PROB)
    e = rel_err(logits.cpu(), fx["train.logits"])
    print("train logits", e)
    assert e < _fx_bound(fx, "refdev.train.logits"), e
    assert abs(crit(logits, y).item() - float(fx["train.loss"])) < _fx_bound(fx, "refdev.train.loss") * max(1.0, abs(float(fx["train.loss"])))
    for i, h in enumerate(m.block_tap):
        e = rel_err(DH.block_samples(h).cpu(), fx[f"train.block{i}"])
        assert e < _fx_bound(fx, f"refdev.train.block{i}"), (i, e)
    assert len(m.drop_tap) == 16
    for rec in m.drop_tap:
        key = f"{rec['unit']}.{rec['site']}"
        e = rel_err(rec["p"].cpu(), fx["train.p." + key])
        assert e < _fx_bound(fx, "refdev.train.p." + key), (key, e)
        assert torch.equal(rec["seeds"].cpu().double(), DH.all_drop_seeds(cfg)[(rec["unit"], rec["site"])])
    sd = m.state_dict()
    n_stats = 0
    for k in fx:
        if k.startswith("train.stat."):
            key = k[len("train.stat."):]
            n_stats += 1
            if key.endswith("num_batches_tracked"):
                assert sd[key].item() == int(fx[k]) == 4, key
            else:
                assert rel_err(sd[key].cpu(), fx[k]) < _fx_bound(fx, "refdev." + k), (key, rel_err(sd[key].cpu(), fx[k]))
    assert n_stats == 3 * sum(1 for k in sd if k.endswith("running_mean"))
    # keep_prob 1 in train mode draws nothing
    m.drop_tap = []
    with torch.no_grad():
        m(x, 1.0)
    assert not m.drop_tap


def _digest_errors(name, g, fx, prefix, floor=0.0):
    gd = g.detach().double().flatten().cpu()
    ref_norm = float(fx[prefix + "gn." + name][0])
    scale = max(ref_norm, floor, 1e-30)
    e1 = abs(gd.norm().item() - ref_norm) / scale
    # the error's +-1 projections have mean square |error|^2: their RMS estimates the L2 distance to the reference
    e3 = float(np.sqrt(np.mean((probe_vectors(name, gd.numel()) @ gd.numpy() - fx[prefix + "gp." + name]) ** 2))) / scale
    return e1, e3


def _model_grads(m, x, y, training, cfg):
    m.train(training)
    _inject(m, cfg)
    m.zero_grad()
    train.SmoothedCrossEntropyLoss()(m(x, DH.KEEP_PROB), y).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_model_gradients_tight(name, training):
    """margin-selected fixtures: every parameter gradient within max(2e-5, 4 x the reference's own fp32-vs-fp64
    deviation) of the reference's; the analytically zero train-mode biases against the floor (the matching weight
    gradient's norm), a gate convolution's one bias at the scale of its own sum (dgcn_helpers.digest_check).  The train
    runs use the fixtures' injected DropGraph seeds."""
    fx = load_fixture(f"dgcn_{name}.npz")
    m, _, cfg = _model(name)
    tag = "train." if training else "eval."
    grads = _model_grads(m, *(t.to(DEV) for t in DH.fixture_input(fx, cfg)), training, cfg)
    zero = DH.zero_grad_biases(grads) if training else {}
    worst = ("", 0.0)
    for n, g in grads.items():
        tol = max(2e-5, 4.0 * float(fx[f"refdev.{tag}g.{n}"]))
        if n in zero:
            floor = float(fx[tag + "gn." + zero[n]][0])
            e = g.double().norm().item() / floor
            assert e < tol, (n, "zero-gradient bias against the floor", e)
            continue
        e = DH.digest_check(n, g, fx, tag, tol)
        worst = max(worst, (n, e), key=lambda t: t[1])
    print("worst gradient digest error", worst)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_model_gradients_wiring(name, training):
    """every parameter gradient within the wiring bound (4 x the largest flip-induced fp32-vs-fp64 deviation of the
    reference over 20 inputs of shape d) of the reference's: a wrong residual, stride, group or gate moves a gradient by
    order 1"""
    fx = load_fixture(f"dgcn_{name}.npz")
    bound = float(load_fixture("dgcn_d.npz")["wiring_bound"])
    assert 0 < bound < 1
    m, _, cfg = _model(name)
    tag = "train." if training else "eval."
    grads = _model_grads(m, *(t.to(DEV) for t in DH.fixture_input(fx, cfg)), training, cfg)
    zero, gate = DH.gradient_floors(grads, training), DH.gate_biases(grads)
    worst = 0.0
    for n, g in grads.items():
        if n in gate:
            e = DH.gate_bias_error(g, fx[tag + "gh." + n], float(fx[tag + "gs." + n]))[0]
            worst = max(worst, e)
            assert e < bound, (n, e, bound)
            continue
        floor = float(fx[tag + "gn." + zero[n]][0]) if n in zero else 0.0
        e1, e3 = _digest_errors(n, g, fx, tag, floor)
        worst = max(worst, e1, e3)
        assert e1 < bound and e3 < bound, (n, e1, e3, bound)
    print("worst wiring error", worst, "bound", bound)


def _tapped_seeds(tap):
    return {(r["unit"], r["site"]): r["seeds"].detach().double().cpu() for r in tap}


def test_hash_drawn_drop_graph_reproduced_by_the_restatement():
    """one train forward with the hash-drawn seeds: the fp64 restatement, fed the tapped seeds, reproduces the logits
    (max(2e-5, 4 x refdev) of fixture a) and the gradients (within the wiring bound: the tapped masks are not the ones
    fixture a's input was margin-selected for); the tapped probabilities match fp64"""
    fx, bound = load_fixture("dgcn_a.npz"), float(load_fixture("dgcn_d.npz")["wiring_bound"])
    m, w, cfg = _model("a")
    x, y = DH.fixture_input(fx, cfg)
    m.train()
    torch.manual_seed(3)
    m.drop_tap = []
    m.zero_grad()
    logits = m(x.to(DEV), DH.KEEP_PROB)
    train.SmoothedCrossEntropyLoss()(logits, y.to(DEV)).backward()
    tap = m.drop_tap
    assert len(tap) == 16 and all(((r["seeds"] == 0) | (r["seeds"] == 1)).all() for r in tap)
    log = []
    rec, log32 = DH.Record(), []
    ref, _, grads = DH.grads_of(w, x, y, cfg, True, rec=rec, seeds=_tapped_seeds(tap), log=log)
    with torch.no_grad():
        DH.restate(w, x, cfg, training=True, dtype=torch.float32, seeds=_tapped_seeds(tap), log=log32)
    e = rel_err(logits.detach().cpu(), ref)
    print("hash-drawn logits", e)
    assert e < _fx_bound(fx, "refdev.train.logits"), e
    for r, (unit, site, p, s, mask, scale), l32 in zip(tap, log, log32):
        _close(r["p"], p, f"p {unit}.{site}", l32[2])
        assert torch.equal((r["factor"] != 0).cpu(), mask != 0)
    zero, gate = DH.gradient_floors(grads, True), DH.gate_biases(grads)
    for n, p in m.named_parameters():
        if n in gate:
            _close_gate_bias(p.grad, grads[n], rec.terms[n], "d " + n, bound=bound)
        elif p.requires_grad:
            floor = grads[zero[n]].norm().item() if n in zero else 1e-300
            e = (p.grad.double().cpu() - grads[n]).norm().item() / max(grads[n].norm().item(), floor)
            assert e < bound, (n, e)


def test_seeds_across_interleaved_forwards():
    """forwards A, B, then backward A: bit for bit the gradient of A alone (B redraws the seed word, not A's copy of it),
    head dropout and DropGraph masks included"""
    m, w, cfg = _model("b", dropout=0.25)
    x, y = DH.make_input(cfg, seed=3)
    xa, xb, yd = x.to(DEV), x.flip(0).contiguous().to(DEV), y.to(DEV)
    crit = train.SmoothedCrossEntropyLoss()
    m.train()
    torch.manual_seed(11)
    m._drop_calls = 0
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m.drop_tap = []
    crit(m(xa), yd).backward()
    first = _tapped_seeds(m.drop_tap)
    alone = [p.grad.clone() for p in m.parameters() if p.requires_grad]
    m.load_state_dict(sd0)
    m.zero_grad()
    m._drop_calls = 0
    m.drop_tap = []
    la = m(xa)
    m(xb)
    crit(la, yd).backward()
    assert all(torch.equal(v, first[k]) for k, v in _tapped_seeds(m.drop_tap[:16]).items())
    assert any(not torch.equal(v, first[k]) for k, v in _tapped_seeds(m.drop_tap[16:]).items())
    assert all(torch.equal(p.grad, q) for p, q in zip([p for p in m.parameters() if p.requires_grad], alone))


def test_graphed_eval_bit_equal():
    m, _, cfg = _model("a")
    m.eval()
    x, _ = DH.make_input(cfg)
    x = x.to(DEV)
    fast = serve.GraphedEval(m, x)
    with torch.no_grad():
        ref = m(x)
    assert torch.equal(fast(x), ref)


def test_graphed_train_step_equals_eager():
    cfg = DH.CONFIGS["a"]
    x, y = DH.make_input(cfg)
    x, y = x.to(DEV), y.to(DEV)
    ms = [_model("a", dropout=0.05)[0].train() for _ in range(2)]
    opts = [torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=torch.tensor(3e-4, device=DEV), fused=True,
                              capturable=True) for m in ms]
    scheds = [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in opts]
    torch.manual_seed(5)
    ms[1].drop_tap = []
    eager = train.TrainStep(ms[0], opts[0])
    graphed = train.GraphedTrainStep(ms[1], opts[1], x, y)
    taps = list(ms[1].drop_tap[-16:])                    # the captured forward's tensors: every replay rewrites them
    assert len(taps) == 16
    ms[1].drop_tap = None
    nbt, rv = "l4.tcn1.bn.num_batches_tracked", "l4.tcn1.bn.running_var"
    drawn = []
    for i in range(5):
        before = (ms[1].state_dict()[nbt].item(), ms[1].state_dict()[rv].clone())
        le, lg = eager(x, y), graphed(x, y)
        assert torch.equal(le, lg), (i, le.item(), lg.item())
        assert ms[1].state_dict()[nbt].item() == before[0] + 1 and not torch.equal(ms[1].state_dict()[rv], before[1])
        drawn.append(torch.cat([r["seeds"].flatten() for r in taps]).clone())
        if i == 2:
            for s in scheds:
                s.step()
    assert all(torch.equal(p, q) for p, q in zip(ms[0].parameters(), ms[1].parameters()))
    assert all(d.sum().item() > 0 for d in drawn)
    assert all(not torch.equal(drawn[i], drawn[i + 1]) for i in range(4))      # replays draw different masks


def test_adamw_trajectory_tracks_fp64():
    """20 AdamW steps from fixture a's weights follow the fp64 restatement fed each step's tapped DropGraph seeds; the
    bound is 4 x the reference's own fp32-vs-fp64 drift over the same 20 steps (worst of 5 inputs, flips included),
    measured by the fixture generator.  Every parameter is compared on its own, the gate convolutions' single biases
    too."""
    fx = load_fixture("dgcn_a.npz")
    loss_bound, w_bound = 4 * float(fx["adamw.loss_dev"]), 4 * float(fx["adamw.w_dev"])
    m, w, cfg = _model("a")
    m.train()
    x, y = DH.make_input(cfg, seed=100)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=3e-4)
    P = {k: (v.double().clone().requires_grad_(k in names) if v.is_floating_point() else v.clone()) for k, v in w.items()}
    ref_opt = torch.optim.AdamW([P[n] for n in names], lr=3e-4)
    step = train.TrainStep(m, opt)
    worst = 0.0
    for i in range(20):
        m.drop_tap = []
        loss = step(x.to(DEV), y.to(DEV)).item()
        ref_opt.zero_grad()
        rec = DH.Record()
        rl = DH.smoothed_ce(DH.restate(P, x, cfg, training=True, rec=rec, seeds=_tapped_seeds(m.drop_tap)), y)
        rl.backward()
        ref_opt.step()
        for k, v in rec.stats.items():
            P[k] = v
        worst = max(worst, abs(loss - rl.item()) / max(1.0, abs(rl.item())))
        assert abs(loss - rl.item()) < loss_bound * max(1.0, abs(rl.item())), (i, loss, rl.item())
    print("AdamW worst loss deviation", worst, "bound", loss_bound)
    mine = dict(m.named_parameters())
    for n in names:
        e = rel_err(mine[n].detach().cpu(), P[n].detach())
        assert e < w_bound, (n, e)


def test_full_size_train_step_is_reproducible():
    """B = 64, T = 128, keep_prob 0.9: one train step runs, is finite, and loss and gradients repeat bit for bit"""
    hp = hw.DecoupledGCNParams({"num_class": 2002}, 2)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(64, 128, 29, 2, generator=g).to(DEV)
    y = torch.randint(0, 2002, (64,), generator=g).to(DEV)
    torch.manual_seed(1)
    m = hw.DecoupledGCNModel(*hp.get_model_params()).to(DEV).train()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    res = []
    for _ in range(2):
        m.load_state_dict(sd0)
        m._drop_calls = 0
        m.drop_tap = []
        step = train.TrainStep(m)
        m.zero_grad()
        loss = step(x, y)
        assert torch.isfinite(loss).item() and len(m.drop_tap) == 16
        res.append([loss.clone()] + [p.grad.clone() for p in m.parameters() if p.requires_grad])
    assert all(torch.isfinite(t).all().item() for t in res[0])
    assert all(torch.equal(a, b) for a, b in zip(*res))
