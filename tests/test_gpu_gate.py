"""GPU parity for the GATE model and for WGATE with window sizes other than 16: the wide band attention kernels
(csrc/wband_attn.hip) and the LayerNorm + weighted token pool through the C ABI vs the dense fp64 restatement of
tests/gate_helpers.py (which tests/test_gate_cpu.py pins to the reference-made fixtures), and the whole models vs those
fixtures.

fp32: norm-relative 2e-5; bf16 storage: 1e-2 (o) / 2e-2 (gradients) -- the bounds of tests/test_gpu_wgate.py.
"""
import importlib

import pytest
import torch

import gate_helpers as GH
from oracle import hwgat_oracle as O
import torch.nn.functional as tF
from helpers import load_fixture, rel_err, entrywise, grad_digest_check, attn_parity

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
serve = importlib.import_module("sl-hwgat_amd.serve")
ck = hw.checkpoint
DEV = "cuda:0"
F32_TOL, BF16_TOL = 2e-5, 1e-2
BF16_NORM = dict(o=BF16_TOL, dq=2 * BF16_TOL, dk=2 * BF16_TOL, dv=2 * BF16_TOL)
# entry-wise bounds of attn_parity (the worst error relative to the part's largest reference entry): about 3x the worst
# value observed on an MI355X over this module's cases (o / dq / dk / dv in the comments), never above the caps 1e-4
# (fp32) and 2e-2 (bf16)
WBAND_ENTRY_F32 = dict(o=7e-7, dq=9e-7, dk=9e-7, dv=6e-7)               # observed 2.3e-7 / 2.8e-7 / 2.8e-7 / 1.9e-7
WBAND_ENTRY_BF16 = dict(o=1.5e-2, dq=1.8e-2, dk=1.8e-2, dv=1.9e-2)      # observed 5.1e-3 / 6.1e-3 / 6.1e-3 / 6.5e-3
FIXTURES = ["gate_a.npz", "gate_b.npz", "wgate_w32.npz", "wgate_w8.npz"]


def _gate_adj(F, W=29):
    """GATE's graph: the 29-joint skeleton without self loops, the same joint in the neighbouring frames; for other W the
    first W joints' sub-graph plus a ring (so that every joint keeps a same-frame neighbour)"""
    hp = hw.GATEParams({"src_len": 1, "num_class": 2}, 2, None)
    edges = [e for e in hp.edges if max(e) < W] + [[i, (i + 1) % W] for i in range(W) if W > 1 and i != (i + 1) % W]
    return GH.default_adjacency([edges], W, F, self_loops=(W == 1))


def _random_adj(F, nW, W, seed, self_loops=True):
    g = torch.Generator().manual_seed(seed)
    diag = (torch.rand(nW, W, W, generator=g) < 0.25).float()
    if self_loops:
        diag = torch.maximum(diag, torch.eye(W))
    else:
        diag[:, torch.arange(W), torch.arange(W)] = 0.0
        diag[:, torch.arange(W), (torch.arange(W) + 1) % W] = 1.0          # no self loops (W > 1), every row non-empty
    prev = (torch.rand(nW, W, W, generator=g) < 0.2).float()
    nxt = (torch.rand(nW, W, W, generator=g) < 0.2).float()
    return GH.band_adjacency(diag, prev, nxt, F)


def _parity(qkv, do, adj, nH, W, what, drop=None, keep=None):
    """forward + backward of the kernels vs the dense fp64 form, fp32 and bf16 storage, every entry compared; prints the
    measured figures before asserting"""
    d = qkv.shape[-1] // 3
    rows = HF.wband_mask_rows(adj, qkv.shape[1], W).to(DEV)
    out_errs = {}
    for dtype, tol, entry in ((torch.float32, F32_TOL, WBAND_ENTRY_F32), (torch.bfloat16, BF16_NORM, WBAND_ENTRY_BF16)):
        x = qkv.to(DEV, dtype).requires_grad_(True)
        ref_in = x.detach().cpu().double().requires_grad_(True)
        ref = GH.dense_band_attention(ref_in, adj.double(), nH, W, keep)
        ref.backward(do.double())
        out = HF.wband_attention(x, rows, nH, drop=drop)
        out.backward(do.to(DEV, dtype))
        errs = {}
        for i, part in enumerate(("o", "dq", "dk", "dv")):
            a = out.detach() if part == "o" else x.grad[..., (i - 1) * d:i * d]
            b = ref.detach() if part == "o" else ref_in.grad[..., (i - 1) * d:i * d]
            errs[part] = (rel_err(a.float().cpu(), b), entrywise(a.float().cpu(), b))
        print(f"wband {what} {str(dtype)[6:]}: " + "  ".join(f"{k} norm {v[0]:.2e} entry {v[1]:.2e}" for k, v in errs.items()))
        attn_parity(out, ref, x.grad, ref_in.grad, d, tol, entry, f"wband {what} {dtype}")
        out_errs[dtype] = (out.detach(), x.grad.detach(), ref.detach())
    return out_errs


# (W, nW, hd, nH, F, B): W in {29, 32, 8, 17}; head_dim 16 and 32; head counts that leave a part workgroup (4 waves =
# 4 heads: 6, 3, 2, 5); F = 1, 2; frame segments (B nW nH < 2048 and F >= 32: segments of at least 8 frames): F 32 -> 2 x 16
# or 4 x 8, F 50 -> 13 / 13 / 13 / 11 (ragged), F 65 nH 2 -> 7 x 9 + 2 (>= 3 segments, ragged); nW 1 and > 1
CASES = [(29, 1, 16, 8, 8, 2), (29, 1, 32, 4, 5, 2), (29, 1, 16, 6, 1, 3), (29, 1, 16, 3, 2, 1), (29, 1, 16, 8, 50, 1),
         (29, 1, 32, 2, 65, 1), (32, 2, 16, 8, 6, 2), (32, 3, 32, 2, 32, 1), (32, 1, 16, 5, 37, 1), (8, 4, 32, 4, 6, 2),
         (8, 2, 16, 2, 65, 1), (17, 2, 16, 4, 9, 2), (17, 1, 32, 3, 33, 1), (1, 3, 16, 2, 4, 1), (16, 2, 16, 4, 5, 1)]


@pytest.mark.parametrize("W,nW,hd,nH,F,B", CASES)
def test_wband_attention_fwd_bwd(W, nW, hd, nH, F, B):
    g = torch.Generator().manual_seed(W + 3 * nW + hd + F)
    d, K = nH * hd, nW * W
    qkv = torch.randn(B, F, K, 3 * d, generator=g) * 0.8
    do = torch.randn(B, F, K, d, generator=g)
    if nW == 1 and W > 1:
        adj = _gate_adj(F, W)                                              # GATE: no self loops
        assert not bool(torch.diagonal(adj[0]).any())
    else:
        edges = [[[i, (i + 3) % W] for i in range(W) if W > 3] + [[0, W - 1]] * (W > 1) for _ in range(nW)]
        adj = GH.default_adjacency([[e for e in ed if e[0] != e[1]] for ed in edges], W, F, self_loops=True)
    _parity(qkv, do, adj, nH, W, f"W{W} nW{nW} hd{hd} nH{nH} F{F} B{B}")


@pytest.mark.parametrize("W,nW,hd,nH,F,B,loops", [(29, 1, 16, 4, 7, 2, False), (32, 2, 16, 2, 7, 2, True),
                                                  (17, 2, 32, 2, 35, 1, False), (8, 3, 16, 4, 5, 1, True)])
def test_wband_attention_general_blocks(W, nW, hd, nH, F, B, loops):
    """arbitrary asymmetric blocks (prev != next exercise the three mask words separately), with and without a diagonal"""
    g = torch.Generator().manual_seed(5 * W + F)
    d, K = nH * hd, nW * W
    qkv = torch.randn(B, F, K, 3 * d, generator=g)
    do = torch.randn(B, F, K, d, generator=g)
    _parity(qkv, do, _random_adj(F, nW, W, W + F, loops), nH, W, f"general blocks W{W} nW{nW} hd{hd} F{F}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("W,nW,hd,nH,F,B", [(29, 1, 16, 4, 9, 2), (17, 2, 32, 2, 4, 1), (29, 1, 16, 2, 40, 1)])
def test_pad_slots_are_never_touched(W, nW, hd, nH, F, B, dtype):
    """W = 29 / 17: slots W .. 31 of a frame are padding.  The tensors sit inside buffers full of NaN canaries: a pad key
    that was loaded (from behind the frame, or the tensor) would put NaN into the results, and a pad query that was
    stored would overwrite the next frame's rows (caught by the parity) or the canaries behind the last frame."""
    g = torch.Generator().manual_seed(W + F)
    d, K = nH * hd, nW * W
    pad = 4096
    adj = _random_adj(F, nW, W, 3, self_loops=False)
    rows = HF.wband_mask_rows(adj, F, W).to(DEV)

    def canaried(t):
        buf = torch.full((pad + t.numel() + pad,), float("nan"), device=DEV, dtype=dtype)
        view = buf[pad:pad + t.numel()].view(t.shape)
        view.copy_(t.to(DEV, dtype))
        return buf, view

    qkv_h = torch.randn(B, F, K, 3 * d, generator=g)
    do_h = torch.randn(B, F, K, d, generator=g)
    qb, qkv = canaried(qkv_h)
    gb, do = canaried(do_h)
    ob, o = canaried(torch.zeros(B, F, K, d))
    db, dqkv = canaried(torch.zeros(B, F, K, 3 * d))
    HF.attn_fwd("wband", qkv, o, rows, None, nH, False)
    HF.attn_bwd("wband", qkv, do, dqkv, rows, None, nH, False)
    torch.cuda.synchronize()
    for buf, view in ((qb, qkv), (gb, do), (ob, o), (db, dqkv)):
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + view.numel():]).all())
        assert bool(torch.isfinite(view).all())
    ref_in = qkv.detach().cpu().double().requires_grad_(True)
    ref = GH.dense_band_attention(ref_in, adj.double(), nH, W)
    ref.backward(do.cpu().double())
    tol = F32_TOL if dtype == torch.float32 else BF16_NORM
    attn_parity(o, ref, dqkv, ref_in.grad, d, tol, WBAND_ENTRY_F32 if dtype == torch.float32 else WBAND_ENTRY_BF16, "canaries")


@pytest.mark.parametrize("W,nW,hd,nH,F,B", [(29, 1, 16, 8, 6, 2), (29, 1, 32, 3, 5, 1), (32, 2, 16, 2, 34, 1), (8, 2, 32, 2, 4, 2),
                                            (17, 1, 16, 4, 3, 1)])
def test_wband_attention_with_attention_dropout(W, nW, hd, nH, F, B):
    """attn_drop_rate > 0 (reference GATE.py:42,64 / WGATE.py:81,103): the mask is the library's hash over the element
    index of the reference's DENSE (B nW, nH, F W, F W) attention tensor, so hwgat_dropout_mask_f32 hands the whole of it
    to the dense restatement; forward and backward, both dtypes, segments included; another seed changes the result"""
    g = torch.Generator().manual_seed(7 * hd + W + F)
    d, K, p_drop, seed = nH * hd, nW * W, 0.2, 0xBEEF03
    qkv = torch.randn(B, F, K, 3 * d, generator=g) * 0.8
    do = torch.randn(B, F, K, d, generator=g)
    adj = _gate_adj(F, W) if nW == 1 else _random_adj(F, nW, W, 11)
    keep = HF.dropout_mask((B, nW, nH, F * W, F * W), seed, p_drop, DEV).cpu().double()
    res = _parity(qkv, do, adj, nH, W, f"dropout W{W} hd{hd} F{F}", drop=(seed, p_drop), keep=keep)
    rows = HF.wband_mask_rows(adj, F, W).to(DEV)
    out, _, ref = res[torch.float32]
    x = qkv.to(DEV)
    other = HF.wband_attention(x, rows, nH, drop=(seed + 1, p_drop))
    assert rel_err(other.cpu(), ref) > 0.05
    assert torch.equal(HF.wband_attention(x, rows, nH, drop=(seed, 0.0)), HF.wband_attention(x, rows, nH))
    base = torch.tensor([77], dtype=torch.int32, device=DEV)
    assert torch.equal(HF.wband_attention(x, rows, nH, drop=(seed - 77, p_drop, base)), out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_size_properties(dtype):
    """GATE at the headline batch (B64 T128 K29 d128, 8 heads): size-independent properties; batch order and frame
    segmentation (one clip alone is cut into more segments) do not change a bit, forward and backward"""
    B, F, W, nH, hd = 64, 128, 29, 8, 16
    d = nH * hd
    bf = dtype == torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(B, F, W, 3 * d, device=DEV, generator=g).to(dtype)
    do = torch.randn(B, F, W, d, device=DEV, generator=g).to(dtype)
    adj = _gate_adj(F)
    rows = HF.wband_mask_rows(adj, F, W).to(DEV)
    q1 = qkv.clone()
    q1[..., 2 * d:] = 1.0
    assert (HF.wband_attention(q1, rows, nH).float() - 1).abs().max() < (2e-2 if bf else 1e-5)   # rows of P sum to 1
    x = qkv.clone().requires_grad_(True)
    a = HF.wband_attention(x, rows, nH)
    a.backward(do)
    q2 = qkv.clone()
    q2[..., 2 * d:] *= -2.0
    assert (HF.wband_attention(q2, rows, nH).float() + 2 * a.detach().float()).abs().max() < (0.1 if bf else 1e-4)   # linear in V
    perm = torch.randperm(B, device=DEV)
    xp = qkv[perm].contiguous().requires_grad_(True)
    ap = HF.wband_attention(xp, rows, nH)
    ap.backward(do[perm].contiguous())
    assert torch.equal(ap, a[perm]) and torch.equal(xp.grad, x.grad[perm])
    x1 = qkv[5:6].contiguous().requires_grad_(True)
    a1 = HF.wband_attention(x1, rows, nH)
    a1.backward(do[5:6].contiguous())
    assert torch.equal(a1, a[5:6]) and torch.equal(x1.grad, x.grad[5:6])
    # one clip against the dense fp64 form (two heads at a time: 3712^2 scores per head)
    tol = BF16_TOL / 2 if bf else F32_TOL
    for h0 in (0, 6):
        cols = torch.cat([torch.arange(h0 * hd, (h0 + 2) * hd) + part * d for part in range(3)]).to(DEV)
        ref_in = qkv[7:8][..., cols].cpu().double().requires_grad_(True)
        ref = GH.dense_band_attention(ref_in, adj.double(), 2, W)
        ref.backward(do[7:8, ..., h0 * hd:(h0 + 2) * hd].cpu().double())
        assert rel_err(a[7:8, ..., h0 * hd:(h0 + 2) * hd].float().cpu(), ref.detach()) < tol
        assert rel_err(x.grad[7:8][..., cols].float().cpu(), ref_in.grad) < tol


# ------------------------------------------------------------------------------------------ LayerNorm + weighted pool
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B,n_tok,d", [(3, 145, 128), (4, 3712, 128), (2, 300, 256)])
def test_ln_weighted_pool(B, n_tok, d, det, dtype):
    g = torch.Generator().manual_seed(n_tok + d)
    x = (torch.randn(B, n_tok, d, generator=g) * 1.5 + 0.3).to(dtype)
    gamma = 1.0 + 0.1 * torch.randn(d, generator=g)
    beta = 0.1 * torch.randn(d, generator=g)
    w = (0.25 + 1.5 * torch.rand(1, n_tok, generator=g)) / n_tok
    bias = torch.tensor([0.03])
    dfeat = torch.randn(B, d, generator=g)
    ref_in = [t.double().requires_grad_(True) for t in (x, gamma, beta, w, bias)]
    ref = GH.ln_weighted_pool(*ref_in)
    ref.backward(dfeat.double())
    dev_in = [t.to(DEV).requires_grad_(True) for t in (x, gamma, beta, w, bias)]
    out = HF.ln_weighted_pool(*dev_in, deterministic=det)
    out.backward(dfeat.to(DEV))
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    errs = [rel_err(out.detach().cpu(), ref.detach())] + [rel_err(a.grad.float().cpu(), b.grad) for a, b in zip(dev_in, ref_in)]
    print(f"ln_weighted_pool B{B} n{n_tok} d{d} det{int(det)} {str(dtype)[6:]}: feat, dx, dgamma, dbeta, dw, dbias =",
          " ".join(f"{e:.2e}" for e in errs))
    assert out.dtype == torch.float32 and dev_in[3].grad.shape == w.shape and dev_in[4].grad.shape == bias.shape
    assert max(errs[:1] + errs[2:]) < 2e-5 and errs[1] < tol          # x's gradient is stored in the activation dtype
    if det:
        again = [t.detach().clone().requires_grad_(True) for t in dev_in]
        out2 = HF.ln_weighted_pool(*again, deterministic=True)
        out2.backward(dfeat.to(DEV))
        assert torch.equal(out2, out) and all(torch.equal(a.grad, b.grad) for a, b in zip(again, dev_in))
    # a mean pool cannot pass: permuting the token weights changes the output ...
    xd, gd, bd, wd, biasd = [t.detach() for t in dev_in]
    moved = HF.ln_weighted_pool(xd, gd, bd, wd.flip(-1), biasd, deterministic=det)
    assert rel_err(moved.cpu(), ref.detach()) > 1e-3
    # ... and w = 1/n, bias = 0 IS the mean pool
    uniform = HF.ln_weighted_pool(xd, gd, bd, torch.full_like(wd, 1.0 / n_tok), torch.zeros_like(biasd), deterministic=det)
    e_mean = rel_err(uniform.cpu(), HF.ln_mean_pool(xd, gd, bd, deterministic=det).cpu())
    print("   w = 1/n vs ln_mean_pool:", f"{e_mean:.2e}")
    assert e_mean < 1e-5                # fp32 rounding of n_tok-term sums taken in two different orders


def test_ln_weighted_pool_refuses_other_widths():
    x = torch.zeros(1, 4, 192, device=DEV)
    with pytest.raises(NotImplementedError, match="width 192"):
        HF.ln_weighted_pool(x, torch.ones(192, device=DEV), torch.zeros(192, device=DEV), torch.ones(4, device=DEV),
                            torch.zeros(1, device=DEV))


# ------------------------------------------------------------------------------------------ whole models
def use_library_linears(model):
    """TEST-ONLY second formulation of a block (as tests/libgemm_path.py, which knows the W = 16 kernels only): torch
    library GEMMs and torch GELU around the standalone HIP LayerNorm and the wide band attention (drop_rate 0 only)"""
    import types

    def _block(self, h, blk, n_heads, shifted, thr, k, hand):
        assert self._attn_kind == "wband" and not (self.training and self.drop_rate > 0.0)
        xn = HF.layer_norm(h, blk.norm1.weight, blk.norm1.bias)
        o = HF.wband_attention(tF.linear(xn, blk.attn.qkv.weight, blk.attn.qkv.bias), self._mask_bits, n_heads)
        y = h + tF.linear(o, blk.attn.proj.weight, blk.attn.proj.bias)
        z = HF.layer_norm(y, blk.norm2.weight, blk.norm2.bias)
        u = tF.gelu(tF.linear(z, blk.ff.fc1.weight, blk.ff.fc1.bias))
        return y + tF.linear(u, blk.ff.fc2.weight, blk.ff.fc2.bias)

    model._block = types.MethodType(_block, model)
    return model


def _model_from_fixture(fx, dtype=torch.float32):
    cfg, params, adj = GH.fixture_setup(fx)
    ds = {"src_len": cfg["temporal_dim"], "num_class": cfg["num_classes"]}
    if cfg["kind"] == "gate":
        hp = hw.GATEParams(ds, cfg["kp_dim"], DEV)
        hp.num_heads, hp.depths, hp.pe, hp.drop_rate = cfg["num_heads"], cfg["depths"], cfg["use_pe"], 0.0
        model = hw.GATEModel(*hp.get_model_params())
    else:
        hp = hw.WGATEParams(ds, cfg["kp_dim"], DEV, num_kps=cfg["num_kps"], embed_dim=cfg["embed_dim"])
        hp.num_heads, hp.depths, hp.drop_rate = cfg["num_heads"], cfg["depths"], 0.0
        hp.window_size, hp.edges = cfg["W"], fx["edges"].tolist()           # W-slot edge lists, as for HWGATE
        hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
        assert torch.equal(hp.adj_mat, adj)                                  # the reference's adjacency
        model = hw.WGATEModel(*hp.get_model_params())
        assert model._attn_kind == "wband"
    res = model.load_state_dict(params, strict=False)
    assert not res.unexpected_keys and res.missing_keys == ["adj_mask"]
    return model.set_activation_dtype(dtype), params, cfg, adj


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("fused", [True, False])
def test_model_matches_reference_fixture(name, fused):
    fx = load_fixture(name)
    model, _, cfg, _ = _model_from_fixture(fx)
    if not fused:
        use_library_linears(model)
    x = torch.from_numpy(fx["x"]).to(DEV)
    y = torch.from_numpy(fx["y"]).to(DEV)
    crit = train.SmoothedCrossEntropyLoss()
    for mode in ("eval", "train"):                    # drop 0: the same function
        getattr(model, mode)()
        model.zero_grad()
        logits = model(x)
        loss = crit(logits, y)
        loss.backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        print(f"{name} fused{int(fused)} {mode}: logits {rel_err(logits.detach().cpu(), fx['eval.logits']):.2e} "
              f"loss diff {abs(loss.item() - float(fx['evalbwd.loss'])):.2e}")
        assert rel_err(logits.detach().cpu(), fx["eval.logits"]) < 1e-4, mode
        assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-4
        if cfg["kind"] == "gate":
            assert "weightedAvg.weight" in grads and "weightedAvg.bias" in grads
        grad_digest_check(grads, fx, "evalbwd.", 1e-3)
    model.eval()
    with torch.no_grad():
        assert rel_err(model.forward_features(x).cpu(), fx["eval.feat"]) < 1e-4


@pytest.mark.parametrize("name", ["gate_a.npz", "wgate_w32.npz"])
def test_model_bf16_and_seeded_dropout(name):
    fx = load_fixture(name)
    model, params, cfg, _ = _model_from_fixture(fx, torch.bfloat16)
    model.eval()
    x = torch.from_numpy(fx["x"]).to(DEV)
    with torch.no_grad():
        logits = model(x)
    assert rel_err(logits.float().cpu(), fx["eval.logits"]) < 1e-2
    model.set_activation_dtype(torch.float32)
    model.drop_rate, model.attn_drop_rate = 0.1, 0.1
    model.train()
    a = model(x)
    model._drop_calls = 0
    b = model(x)
    assert torch.allclose(a, b, atol=1e-6) and torch.isfinite(a).all()
    model.eval()
    assert (model(x) - a).abs().max() > 1e-3
    a.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def _small_gate(dtype, T=16, nc=7):
    torch.manual_seed(11)
    hp = hw.GATEParams({"src_len": T, "num_class": nc}, 2, DEV)
    hp.depths = 3
    model = hw.GATEModel(*hp.get_model_params()).to(DEV)
    assert model.drop_rate == 0.1                         # the reference default: dropout is ON in these runs
    with torch.no_grad():                                 # a pool that is not (nearly) zero at the start
        model.weightedAvg.weight.copy_((0.25 + 1.5 * torch.rand(1, T * 29)) / (T * 29))
    return model.set_activation_dtype(dtype)


def _batch(model, B=8, nc=7):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(B, model.temporal_dim, model.num_kps, model.kp_dim, device=DEV, generator=g)
    y = torch.randint(0, nc, (B,), device=DEV, generator=g)
    return x, y


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_eval_is_bit_equal_to_eager(dtype):
    model = _small_gate(dtype).eval()
    x, _ = _batch(model)
    with torch.no_grad():
        eager = model(x)
    ge = serve.GraphedEval(model, x)
    assert torch.equal(ge(x), eager)
    x2 = torch.rand_like(x)
    with torch.no_grad():
        assert torch.equal(ge(x2), model(x2))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_train_step_is_bit_equal_to_the_eager_step_when_deterministic(dtype):
    """`deterministic_train`: losses and every weight of 5 graphed steps equal the eager steps bit for bit, with the
    cosine schedule stepped between them (attention kind 'wband', the weighted pool and its parameters included)"""
    steps, c0 = 5, 17
    runs = []
    for graphed in (False, True):
        m = _small_gate(dtype).train()
        m.deterministic_train = True
        x, y = _batch(m)
        o = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
        sch = ck.get_scheduler(o)
        m._drop_calls = c0
        s = train.GraphedTrainStep(m, o, x, y) if graphed else train.TrainStep(m, o, None)
        losses = []
        for _ in range(steps):
            losses.append(s(x, y).clone())
            sch.step()
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (le, we), (lg, wg) = runs
    for k in range(steps):
        assert torch.equal(le[k], lg[k]), (k, float(le[k]), float(lg[k]))
    assert float(lg[-1]) < float(lg[0])
    for n in we:
        assert torch.equal(we[n], wg[n]), n
    assert not torch.equal(we["weightedAvg.weight"], _small_gate(dtype).weightedAvg.weight.detach())   # the pool trains


def test_twenty_adamw_cosine_steps_match_the_restatement():
    """AdamW(lr 5e-4) + CosineAnnealingLR, 20 steps of GATE on the HIP backend vs the fp64 dense restatement: learning rate
    per step identical, loss per step and final parameters within the bounds of
    test_gpu_train_parity.py::test_twenty_adamw_cosine_steps_match_the_oracle"""
    T, C, nc, B, steps, depths, heads = 8, 2, 6, 4, 20, 2, 8
    cfg = dict(kp_dim=C, temporal_dim=T, num_kps=29, num_classes=nc, embed_dim=128, depths=depths, ff_ratio=2.0,
               use_pe=True, pool="weighted")
    params = GH.synth_params(51, **cfg)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, T, 29, C, generator=g)
    y = torch.randint(0, nc, (B,), generator=g)
    hp = hw.GATEParams({"src_len": T, "num_class": nc}, C, DEV)
    hp.depths, hp.num_heads, hp.drop_rate = depths, heads, 0.0

    ref_p = {k: torch.nn.Parameter(v.double(), requires_grad=k not in ("B", "pos_encoder.pe")) for k, v in params.items()}
    dense = GH.DenseBandModel(ref_p, adj=hp.adj_mat.cpu(), W=29, depths=depths, num_heads=heads, use_pe=True, pool="weighted")
    opt_r = ck.get_optimizer(torch.nn.ParameterList(ref_p.values()))
    sch_r = ck.get_scheduler(opt_r)
    ref_losses, ref_lr = [], []
    for s in range(steps):
        opt_r.zero_grad()
        loss = O.smoothed_cross_entropy(dense.forward(x.double()), y)
        loss.backward()
        opt_r.step()
        ref_lr.append(opt_r.param_groups[0]["lr"])
        sch_r.step()
        ref_losses.append(loss.item())

    model = hw.GATEModel(*hp.get_model_params())
    model.load_state_dict(params, strict=False)
    model.train()
    opt = ck.get_optimizer(model, fused=True)
    sch = ck.get_scheduler(opt)
    step = train.TrainStep(model, opt)
    losses, lrs = [], []
    for s in range(steps):
        losses.append(float(step(x.to(DEV), y.to(DEV))))
        lrs.append(opt.param_groups[0]["lr"])
        sch.step()
    assert max(abs(a - b) for a, b in zip(lrs, ref_lr)) < 1e-12
    worst_loss = max(abs(a - b) for a, b in zip(losses, ref_losses))
    sd = model.state_dict()
    worst = max(rel_err(sd[k].cpu(), v.detach()) for k, v in ref_p.items()
                if v.requires_grad and not k.endswith("attn.qkv.bias"))
    print("20 steps: worst loss diff", worst_loss, "worst param rel err", worst, "loss", losses[0], "->", losses[-1])
    assert worst_loss < 1e-3 and losses[-1] < losses[0]
    assert worst < 2e-3
