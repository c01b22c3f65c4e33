"""GPU parity for HWGATE window sizes other than 16: the part-window attention kernels (hwgat_pwin_attn_*) through the
C-ABI against an fp64 dense restatement of the reference's MSA (hwgat/models/HWGATE.py:30-38, 89-114, 169-187) written
here (the oracle package is W = 16 only), and whole models against tests/golden/window_*.npz."""
import importlib
import os
import sys

import pytest
import torch

from helpers import load_fixture, rel_err, grad_digest_check, attn_parity, tie_free_threshold
from libgemm_path import use_library_linears
from oracle import hwgat_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_fixtures_window import edge_list  # noqa: E402

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
HW = importlib.import_module("sl-hwgat_amd.models.HWGATE")
train = importlib.import_module("sl-hwgat_amd.train")
serve = importlib.import_module("sl-hwgat_amd.serve")
DEV = "cuda:0"
F32_TOL, BF16_TOL = 2e-5, 1e-2
# entry-wise bounds of attn_parity (the worst error relative to the part's largest reference entry): about 3x the
# worst value observed on an MI355X over this module's cases (o / dq / dk / dv in the comments), capped at 1e-4 (fp32)
# and 2e-2 (bf16)
PWIN_ENTRY_F32 = dict(o=1.7e-6, dq=2e-6, dk=2.2e-6, dv=1.6e-6)         # observed 5.7e-7 / 6.6e-7 / 7.3e-7 / 5.4e-7
PWIN_ENTRY_BF16 = dict(o=1.1e-2, dq=1.1e-2, dk=1e-2, dv=1e-2)          # observed 3.8e-3 / 3.5e-3 / 3.5e-3 / 3.5e-3


def dense_attention(qkv, adj, W, nH, shifted, thr=None, keep=None):
    """(B,F,K,3d) fp64 -> (B,F,K,d): roll, window_partition (token t = tp W + j), scaled logits, the threshold drop
    over a softmax of the 2W keys, shift mask and adjacency products, == 0 -> -10000, softmax, dropout, P V, reverse"""
    B, F, K, d3 = qkv.shape
    d, f, nW, n = d3 // 3, F // 2, K // W, 2 * W
    hd = d // nH
    x = torch.roll(qkv, -1, 1) if shifted else qkv
    w = x.reshape(B, f, 2, nW, W, 3, nH, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * f * nW, nH, n, hd)
    q, k, v = w[0] * hd ** -0.5, w[1], w[2]
    attn = q @ k.transpose(-2, -1)
    if thr is not None:
        attn = attn * torch.where(attn.detach().softmax(-1) > thr, 0, 1)
    if shifted:
        attn = (attn.view(B, f * nW, nH, n, n) * HW._last_slot_mask(F, nW, W).to(attn).unsqueeze(1)).view_as(attn)
    attn = (attn.view(B, f, nW, nH, n, n) * adj.to(attn).view(1, 1, nW, 1, n, n)).view_as(attn)
    attn = attn.masked_fill(attn == 0, -10000.0).softmax(-1)
    if keep is not None:
        attn = attn * keep.to(attn).view_as(attn)
    o = (attn @ v).view(B, f, nW, nH, 2, W, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, F, K, d)
    return torch.roll(o, 1, 1) if shifted else o


def unmasked_p0(qkv, W, nH, shifted):
    """the selector's input (HWGATE.py:97): softmax over the 2W keys of a window of the UNMASKED scaled scores, fp64"""
    B, F, K, d3 = qkv.shape
    d, f, nW, n = d3 // 3, F // 2, K // W, 2 * W
    hd = d // nH
    x = torch.roll(qkv.detach().double(), -1, 1) if shifted else qkv.detach().double()
    w = x.reshape(B, f, 2, nW, W, 3, nH, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * f * nW, nH, n, hd)
    return torch.softmax((w[0] * hd ** -0.5) @ w[1].transpose(-2, -1), dim=-1)


def _adj(nW, W, g):
    n = 2 * W
    a = (torch.rand(nW, n, n, generator=g) < 0.5).float()
    return ((a + a.transpose(1, 2) + torch.eye(n)) > 0).float()


def _run(qkv, do, bits, thr, nH, shifted, drop):
    x = qkv.to(DEV).requires_grad_(True)
    t = None if thr is None else torch.full((1,), thr, device=DEV)
    o = torch.empty(*qkv.shape[:-1], qkv.shape[-1] // 3, device=DEV, dtype=qkv.dtype)
    HF.attn_fwd("pwin", x.detach(), o, bits, t, nH, shifted, drop)
    dqkv = torch.empty_like(x)
    HF.attn_bwd("pwin", x.detach(), do.to(DEV), dqkv, bits, t, nH, shifted, drop)
    return o, dqkv


def _keep(B, F, K, W, nH, seed, p):
    n = 2 * W
    return HF.dropout_mask((B * (F // 2) * (K // W) * nH * n * n,), seed, p, DEV).cpu().double()


@pytest.mark.parametrize("W", [1, 4, 7, 8, 14, 28, 32])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("mode", ["eval", "thr", "thr_drop"])
def test_pwin_attention_fp32_matches_dense(W, hd, shifted, mode):
    g = torch.Generator().manual_seed(W * 7 + hd + shifted)
    nH, nW, B, F = 2, 3 if W <= 8 else 2, 2, 4
    K, d = nW * W, nH * hd
    qkv = torch.randn(B, F, K, 3 * d, generator=g)
    do = torch.randn(B, F, K, d, generator=g)
    adj = _adj(nW, W, g)
    bits = HF.pwin_mask_bits(adj, W).to(DEV)
    thr = None if mode == "eval" else 0.35
    drop = (1234, 0.3) if mode == "thr_drop" else None
    keep = _keep(B, F, K, W, nH, 1234, 0.3) if drop else None
    ref_in = qkv.double().requires_grad_(True)
    ref = dense_attention(ref_in, adj, W, nH, shifted, thr, keep)
    ref.backward(do.double())
    o, dqkv = _run(qkv, do, bits, thr, nH, shifted, drop)
    assert rel_err(o.cpu(), ref.detach()) < F32_TOL
    assert rel_err(dqkv.cpu(), ref_in.grad) < F32_TOL
    attn_parity(o, ref, dqkv, ref_in.grad, d, F32_TOL, PWIN_ENTRY_F32, "pwin fp32")


@pytest.mark.parametrize("W,hd", [(4, 32), (8, 64), (28, 32), (32, 64)])
@pytest.mark.parametrize("mode", ["eval", "thr_drop"])
def test_pwin_attention_bf16_matches_dense(W, hd, mode):
    g = torch.Generator().manual_seed(W + hd)
    nH, nW, B, F = 2, 2, 2, 4
    K, d = nW * W, nH * hd
    qkv = torch.randn(B, F, K, 3 * d, generator=g).bfloat16()
    do = torch.randn(B, F, K, d, generator=g).bfloat16()
    adj = _adj(nW, W, g)
    bits = HF.pwin_mask_bits(adj, W).to(DEV)
    thr = None
    if mode != "eval":               # the nominal 0.35, moved where no probability of the bf16 inputs is close to it
        thr, margin = tie_free_threshold(unmasked_p0(qkv, W, nH, True), 0.35)
        assert margin > 2e-4, (thr, margin)
    drop = (77, 0.2) if mode == "thr_drop" else None
    keep = _keep(B, F, K, W, nH, 77, 0.2) if drop else None
    ref_in = qkv.double().requires_grad_(True)
    ref = dense_attention(ref_in, adj, W, nH, True, thr, keep)
    ref.backward(do.double())
    o, dqkv = _run(qkv, do, bits, thr, nH, True, drop)
    assert rel_err(o.float().cpu(), ref.detach()) < BF16_TOL
    assert rel_err(dqkv.float().cpu(), ref_in.grad) < BF16_TOL
    attn_parity(o, ref, dqkv, ref_in.grad, d, BF16_TOL, PWIN_ENTRY_BF16, "pwin bf16")


@pytest.mark.parametrize("W", [1, 4, 7, 8, 14, 28, 32])
@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("nH", [2, 3])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("mode", ["eval", "thr", "thr_drop"])
def test_pwin_attention_bf16_grid(W, hd, nH, shifted, mode):
    """bf16 storage over the fp32 test's grid: every NMAX bucket (W 1, 4 -> 8; 7, 8 -> 16; 14 -> 32; 28, 32 -> 64), lanes
    left idle (2W does not divide 64: W 7, 14, 28), eval / threshold only / threshold + dropout, both masks, 2 and 3
    heads.  Every case has 9 windows (W <= 14) against G = 64 / 2W windows per wave = 32 / 8 / 4 / 4 / 2: the last wave
    group is only partly filled."""
    g = torch.Generator().manual_seed(W * 13 + hd + 5 * nH + shifted)
    nW = 3 if W <= 14 else 2
    B, F = (1, 6) if nH == 2 else (3, 2)
    K, d = nW * W, nH * hd
    qkv = torch.randn(B, F, K, 3 * d, generator=g).bfloat16()
    do = torch.randn(B, F, K, d, generator=g).bfloat16()
    adj = _adj(nW, W, g)
    bits = HF.pwin_mask_bits(adj, W).to(DEV)
    thr = None
    if mode != "eval":               # no probability of the bf16 inputs within `margin` of the threshold
        thr, margin = tie_free_threshold(unmasked_p0(qkv, W, nH, shifted), 0.35)
        assert margin > 2e-4, (thr, margin)
    drop = (78, 0.2) if mode == "thr_drop" else None
    keep = _keep(B, F, K, W, nH, 78, 0.2) if drop else None
    ref_in = qkv.double().requires_grad_(True)
    ref = dense_attention(ref_in, adj, W, nH, shifted, thr, keep)
    ref.backward(do.double())
    o, dqkv = _run(qkv, do, bits, thr, nH, shifted, drop)
    assert rel_err(o.float().cpu(), ref.detach()) < BF16_TOL
    assert rel_err(dqkv.float().cpu(), ref_in.grad) < BF16_TOL
    attn_parity(o, ref, dqkv, ref_in.grad, d, BF16_TOL, PWIN_ENTRY_BF16, "pwin bf16")


def test_exact_zero_logits_and_all_masked_rows():
    W, nH, hd, B, F, nW = 7, 1, 32, 1, 2, 2
    K, d, n = nW * W, nH * hd, 2 * W
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, F, K, 3 * d, generator=g)
    qkv[0, 0, 2, :d] = 0.0                                  # a zero query: every logit of its row is exactly 0
    adj = _adj(nW, W, g)
    adj[1, 5] = 0.0                                         # a query of window 1 that sees no key
    bits = HF.pwin_mask_bits(adj, W).to(DEV)
    do = torch.randn(B, F, K, d, generator=g)
    ref_in = qkv.double().requires_grad_(True)
    ref = dense_attention(ref_in, adj, W, nH, False)
    ref.backward(do.double())
    o, dqkv = _run(qkv, do, bits, None, nH, False, None)
    assert rel_err(o.cpu(), ref.detach()) < F32_TOL and rel_err(dqkv.cpu(), ref_in.grad) < F32_TOL
    v = qkv[..., 2 * d:].view(B, F, nW, W, d)
    # uniform over the 2W real keys of its window (slot 5 = frame 0, joint 5 of window 1)
    uni = torch.cat([v[0, 0, 1], v[0, 1, 1]]).mean(0)
    assert torch.allclose(o[0, 0, W + 5].cpu(), uni, atol=1e-5)
    uni0 = torch.cat([v[0, 0, 0], v[0, 1, 0]]).mean(0)
    assert torch.allclose(o[0, 0, 2].cpu(), uni0, atol=1e-5)


def test_nan_stays_in_its_window():
    W, nH, hd, B, F, nW = 8, 2, 64, 2, 4, 4
    K, d = nW * W, nH * hd
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B, F, K, 3 * d, generator=g)
    bits = HF.pwin_mask_bits(_adj(nW, W, g), W).to(DEV)
    do = torch.randn(B, F, K, d, generator=g)
    clean, dclean = _run(qkv, do, bits, None, nH, False, None)
    bad = qkv.clone()
    bad[1, 2, W + 3, d + 5] = float("nan")                   # a key of window (b 1, frame pair 1, wi 1), head 0
    o, dq = _run(bad, do, bits, None, nH, False, None)
    hit = torch.zeros(B, F, K, dtype=torch.bool)
    hit[1, 2:4, W:2 * W] = True
    assert not torch.isfinite(o[hit.to(DEV)]).all()
    assert torch.equal(o[~hit.to(DEV)], clean[~hit.to(DEV)])
    assert torch.equal(dq[~hit.to(DEV)], dclean[~hit.to(DEV)])


def test_argument_rejection():
    W, nH, hd, B, F, nW = 8, 2, 64, 1, 2, 2
    K, d = nW * W, nH * hd
    qkv = torch.randn(B, F, K, 3 * d, device=DEV)
    o = torch.empty(B, F, K, d, device=DEV)
    bits = HF.pwin_mask_bits(torch.ones(nW, 2 * W, 2 * W), W).to(DEV)
    p = HF.ptr
    call = lambda *a: hw._lib.lib().hwgat_pwin_attn_fwd(p(qkv), p(o), p(bits), None, *a, 0, HF.stream())   # noqa: E731
    assert call(B, F, K, W, nH, hd, 0) == 0
    assert call(B, F, K, 33, nH, hd, 0) == -2                # W > 32
    assert call(B, F, K, 0, nH, hd, 0) == -2
    assert call(B, F, K, 6, nH, hd, 0) == -2                 # K % W
    assert call(B, 3, K, W, nH, hd, 0) == -2                 # odd F
    assert call(B, F, K, W, 1, 128, 0) == -2                 # head_dim 128
    assert hw._lib.lib().hwgat_pwin_attn_fwd(p(qkv), p(o), None, None, B, F, K, W, nH, hd, 0, 0, HF.stream()) == -1
    assert hw._lib.lib().hwgat_pwin_attn_fwd(p(qkv), p(o), p(bits), None, B, F, K, W, nH, hd, 0, 7, HF.stream()) == -3
    assert hw._lib.lib().hwgat_pwin_attn_fwd_drop(p(qkv), p(o), p(bits), None, B, F, K, W, nH, hd, 0, 0, 1, 0.1, None,
                                                  HF.stream()) == -1          # dropout without the train threshold
    with pytest.raises(NotImplementedError, match="head_dim"):
        HF.attn_fwd("pwin", torch.empty(B, F, K, 3 * 128, device=DEV), torch.empty(B, F, K, 128, device=DEV), bits,
                    None, 1, False)
    with pytest.raises(ValueError):
        HF.attn_fwd("pwin", qkv, o, HF.mask_bits(torch.ones(1, 32, 32)).to(DEV), None, nH, False)


def test_kernels_are_bit_reproducible():
    W, nH, hd, B, F, nW = 28, 4, 32, 2, 8, 2
    K, d = nW * W, nH * hd
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, F, K, 3 * d, generator=g)
    do = torch.randn(B, F, K, d, generator=g)
    bits = HF.pwin_mask_bits(_adj(nW, W, g), W).to(DEV)
    a = _run(qkv, do, bits, 0.2, nH, True, (5, 0.1))
    b = _run(qkv, do, bits, 0.2, nH, True, (5, 0.1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ whole models vs the reference's fixtures
def _model_from_fixture(fx, dtype=torch.float32):
    T, K, C, d0, nc, B, seed, W = [int(v) for v in fx["cfg"]]
    hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, C, None, num_kps=K)
    hp.window_size, hp.num_heads, hp.drop_rate = W, [int(h) for h in fx["heads"]], 0.0
    hp.edges = [edge_list(W, w) for w in range(K // W)]
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    model = hw.Model(*hp.get_model_params())
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0, depths=tuple(hp.depths), ff_ratio=hp.ff_ratio,
               use_pe=hp.pe, num_kps=K, tp=2)
    model.load_state_dict(O.synth_params(seed, weight_std=0.08, **cfg), strict=False)
    return model.to(DEV).set_activation_dtype(dtype)


FIXTURES = ["window_w8.npz", "window_w32.npz", "window_w28.npz"]


def _use_library_linears(model):
    """tests/libgemm_path.py's library-GEMM formulation of a block, with the part-window attention of W != 16"""
    import types
    import torch.nn.functional as tF
    use_library_linears(model)

    def _block(self, h, blk, n_heads, shifted, thr, k, hand):
        xn = HF.layer_norm(h, blk.norm1.weight, blk.norm1.bias)
        o = HF.part_window_attention(tF.linear(xn, blk.attn.qkv.weight, blk.attn.qkv.bias), self._mask_bits, thr,
                                     n_heads, shifted)
        y = h + tF.linear(o, blk.attn.proj.weight, blk.attn.proj.bias)
        z = HF.layer_norm(y, blk.norm2.weight, blk.norm2.bias)
        u = tF.gelu(tF.linear(z, blk.ff.fc1.weight, blk.ff.fc1.bias))
        return y + tF.linear(u, blk.ff.fc2.weight, blk.ff.fc2.bias)

    model._block = types.MethodType(_block, model)
    return model


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("fused", [True, False])
def test_model_matches_reference_fixture(name, fused):
    fx = load_fixture(name)
    model = _model_from_fixture(fx)
    if not fused:
        _use_library_linears(model)                       # (drop_rate is 0: no dropout sites to restate)
    x = torch.from_numpy(fx["x"]).to(DEV)
    y = torch.from_numpy(fx["y"]).to(DEV)
    crit = train.SmoothedCrossEntropyLoss()
    model.eval()
    with torch.no_grad():
        assert rel_err(model(x).cpu(), fx["eval.logits"]) < 1e-4
    model.zero_grad()
    loss = crit(model(x), y)
    loss.backward()
    assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-4
    grad_digest_check({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, fx, "evalbwd.", 1e-3)
    model.train()
    model.threshold_override = [float(t) for t in fx["train.thr"]]
    model.zero_grad()
    out = model(x)
    loss = crit(out, y)
    loss.backward()
    assert rel_err(out.detach().cpu(), fx["train.logits"]) < 1e-4
    assert abs(loss.item() - float(fx["train.loss"])) < 1e-4
    grad_digest_check({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, fx, "train.", 1e-3)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_bf16_matches_reference_fixture(name):
    fx = load_fixture(name)
    model = _model_from_fixture(fx, torch.bfloat16).eval()
    x = torch.from_numpy(fx["x"]).to(DEV)
    with torch.no_grad():
        assert rel_err(model(x).float().cpu(), fx["eval.logits"]) < 1e-2
    model.zero_grad()
    loss = train.SmoothedCrossEntropyLoss()(model(x).float(), torch.from_numpy(fx["y"]).to(DEV))
    loss.backward()
    assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-2 * max(1.0, abs(float(fx["evalbwd.loss"])))


def _small(W, dtype=torch.float32, K=64):
    torch.manual_seed(11)
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 7}, 2, DEV, num_kps=K)
    hp.window_size = W
    hp.edges = [edge_list(W, w) for w in range(K // W)]
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    hp.attn_drop_rate = 0.1
    model = hw.Model(*hp.get_model_params()).to(DEV)
    model.set_activation_dtype(dtype)
    return model


def test_deterministic_train_gives_equal_gradients():
    model = _small(8).train()
    model.deterministic_train = True
    model.threshold_override = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.rand(8, 16, 64, 2, device=DEV, generator=g)
    y = torch.randint(0, 7, (8,), device=DEV, generator=g)
    grads = []
    for _ in range(2):
        model._drop_calls = 4
        model.zero_grad()
        train.SmoothedCrossEntropyLoss()(model(x), y).backward()
        grads.append([p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_eval_is_bit_equal_to_eager(dtype):
    model = _small(32, dtype).eval()
    x = torch.rand(4, 16, 64, 2, device=DEV)
    fast = serve.GraphedEval(model, x)
    with torch.no_grad():
        want = model(x)
    assert torch.equal(fast(x), want)


def test_part_table_input():
    model = _small(8).eval()
    idx = torch.randperm(70)[:64]
    model.use_part_table(idx)
    raw = torch.rand(2, 16, 70, 2, device=DEV)
    with torch.no_grad():
        a = model(raw)
        model.part_index = None
        b = model(raw[:, :, idx.to(DEV)].contiguous())
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_train_step_matches_eager(dtype):
    steps, c0 = 4, 17
    thr = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(8, 16, 64, 2, device=DEV, generator=g)
    y = torch.randint(0, 7, (8,), device=DEV, generator=g)
    m1 = _small(32, dtype).train()
    m1.threshold_override = thr
    o1 = torch.optim.AdamW([p for p in m1.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    m1._drop_calls = c0
    s1 = train.TrainStep(m1, o1, None)
    eager = [s1(x, y).clone() for _ in range(steps)]
    m2 = _small(32, dtype).train()
    m2.threshold_override = thr
    o2 = torch.optim.AdamW([p for p in m2.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    m2._drop_calls = c0
    w0 = [p.detach().clone() for p in m2.parameters()]
    s2 = train.GraphedTrainStep(m2, o2, x, y)
    graphed = [s2(x, y).clone() for _ in range(steps)]
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    for a, b in zip(eager, graphed):
        assert abs(float(a) - float(b)) <= tol * max(1.0, abs(float(a))), (float(a), float(b))
    num = den = 0.0
    for a, p1, p2 in zip(w0, m1.parameters(), m2.parameters()):
        if p1.requires_grad:
            u1, u2 = (p1.detach() - a).double(), (p2.detach() - a).double()
            num += float((u1 - u2).pow(2).sum())
            den += float(u1.pow(2).sum())
    assert den > 0 and (num / den) ** 0.5 < (0.02 if dtype == torch.float32 else 0.25), (num / den) ** 0.5
