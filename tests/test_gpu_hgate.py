"""GPU parity for the HGATE sibling model: the block-attention kernels through the
C-ABI vs the fp64 oracle, and the whole `HGATEModel` vs the reference-generated fixtures.

fp32: bound 1e-3 relative (north_star), observed ~1e-6; bf16 storage: 1e-2.
"""
import importlib

import pytest
import torch

from oracle import hgat_oracle as OH
from libgemm_path import use_library_linears
from helpers import load_fixture, hgate_oracle_from_fixture, sub, rel_err, grad_digest_check, attn_parity

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
DEV = "cuda:0"
F32_TOL, BF16_TOL = 2e-5, 1e-2
BF16_NORM = dict(o=BF16_TOL, dq=2 * BF16_TOL, dk=2 * BF16_TOL, dv=2 * BF16_TOL)
# entry-wise bounds of attn_parity (the worst error relative to the part's largest reference entry): about 3x the
# worst value observed on an MI355X over this module's cases (o / dq / dk / dv in the comments), capped at 1e-4 (fp32)
# and 2e-2 (bf16)
BLK_ENTRY_F32 = dict(o=1e-6, dq=1.2e-6, dk=1.3e-6, dv=1e-6)             # observed 3.4e-7 / 3.7e-7 / 4.2e-7 / 3.2e-7
BLK_ENTRY_BF16 = dict(o=1.7e-2, dq=2e-2, dk=2e-2, dv=1.6e-2)           # observed 5.5e-3 / 6.7e-3 / 7.6e-3 / 5.3e-3


def _adj(KJ, g):
    """the shipped skeleton for 29 joints, else a random symmetric graph with unit diagonal"""
    if KJ == 29:
        return OH.block_adjacency()
    a = (torch.rand(KJ, KJ, generator=g) < 0.3).float()
    a = ((a + a.t() + torch.eye(KJ)) > 0).float()
    return OH.block_adjacency(a)


def _tile_sparse_adj(KJ, g):
    """joints 0-15 and 16..KJ-2 form two groups without an edge between them and joint KJ-1 sees only itself: every
    16-query tile of a frame then sees keys of two of the four 16-slot key tiles only (cross-frame links join a joint
    to itself), so whole 16 x 16 tiles of S and of P are empty"""
    a = torch.zeros(KJ, KJ)
    for lo, hi in ((0, 16), (16, KJ - 1)):
        a[lo:hi, lo:hi] = (torch.rand(hi - lo, hi - lo, generator=g) < 0.5).float()
    a = ((a + a.t() + torch.eye(KJ)) > 0).float()
    assert a[:16, 16:].sum() == 0 and a[KJ - 1].sum() == 1
    return OH.block_adjacency(a)


def _oracle_attn(qkv, adj, n_heads, shifted, attn_keep=None):
    """natural-order qkv (B,F,K,3d) -> o (B,F,K,d) through the oracle's roll / partition / attention chain"""
    B, F, K, d3 = qkv.shape
    d = d3 // 3
    hd = d // n_heads
    x = torch.roll(qkv, -1, 1) if shifted else qkv
    w = x.reshape(B, F // 2, 2 * K, 3, n_heads, hd).permute(3, 0, 1, 4, 2, 5)
    sm = OH.block_shift_mask(F, K, 2, 1, qkv.dtype) if shifted else None
    o, _ = OH.block_attention(w[0], w[1], w[2], adj.to(qkv.dtype), sm, attn_keep)
    o = o.reshape(B, F, K, d)
    return torch.roll(o, 1, 1) if shifted else o


@pytest.mark.parametrize("hd,nH,KJ,F,B", [(64, 2, 29, 8, 2), (64, 4, 32, 4, 3), (32, 4, 29, 6, 2), (32, 2, 17, 4, 1),
                                          (64, 1, 1, 2, 2), (64, 2, 5, 2, 1),
                                          # KJ 16: slots 16-31 of each frame are all padding (key tiles 1, 3 empty);
                                          # KJ 31: one pad slot per frame; an odd head count above 1
                                          (64, 3, 16, 4, 2), (64, 3, 31, 4, 1), (32, 3, 16, 6, 1), (32, 3, 31, 4, 2)])
@pytest.mark.parametrize("shifted", [False, True])
def test_block_attention_fwd_bwd(hd, nH, KJ, F, B, shifted):
    g = torch.Generator().manual_seed(hd + KJ + F)
    d = nH * hd
    qkv = torch.randn(B, F, KJ, 3 * d, generator=g) * 0.8
    do = torch.randn(B, F, KJ, d, generator=g)
    adj = _adj(KJ, g)
    bits = HF.blk_mask_bits(adj, KJ).to(DEV)

    ref_in = qkv.double().requires_grad_(True)
    ref = _oracle_attn(ref_in, adj, nH, shifted)
    ref.backward(do.double())

    x = qkv.to(DEV).requires_grad_(True)
    out = HF.block_attention(x, bits, nH, shifted)
    out.backward(do.to(DEV))
    assert rel_err(out.detach().cpu(), ref.detach()) < F32_TOL
    assert rel_err(x.grad.cpu(), ref_in.grad) < F32_TOL
    attn_parity(out, ref, x.grad, ref_in.grad, d, F32_TOL, BLK_ENTRY_F32, "block fp32")

    xb = qkv.to(DEV, torch.bfloat16).requires_grad_(True)
    refb_in = xb.detach().cpu().double().requires_grad_(True)
    refb = _oracle_attn(refb_in, adj, nH, shifted)
    refb.backward(do.double())
    outb = HF.block_attention(xb, bits, nH, shifted)
    outb.backward(do.to(DEV, torch.bfloat16))
    assert rel_err(outb.detach().float().cpu(), refb.detach()) < BF16_TOL
    assert rel_err(xb.grad.float().cpu(), refb_in.grad) < 2 * BF16_TOL
    attn_parity(outb, refb, xb.grad, refb_in.grad, d, BF16_NORM, BLK_ENTRY_BF16, "block bf16")


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("KJ", [24, 31])
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("p_drop", [0.0, 0.2])
def test_block_attention_tile_sparse(hd, KJ, shifted, p_drop):
    """an adjacency that empties whole 16 x 16 tiles of S and of P: the ballot skip branches of blk_attn_f32.hip (hd 64,
    fp32) for S tiles and for P / dS tiles, and the same masks in the hd-32 kernels and the bf16 16 x 16-tile kernels,
    with and without attention dropout"""
    g = torch.Generator().manual_seed(11 * hd + KJ + int(shifted))
    B, F, nH, seed = 2, 4, 2, 0xBEEF03
    d = nH * hd
    qkv = torch.randn(B, F, KJ, 3 * d, generator=g) * 0.8
    do = torch.randn(B, F, KJ, d, generator=g)
    adj = _tile_sparse_adj(KJ, g)
    bits = HF.blk_mask_bits(adj, KJ).to(DEV)
    drop = (seed, p_drop) if p_drop > 0 else None
    keep = HF.dropout_mask((B, F // 2, nH, 2 * KJ, 2 * KJ), seed, p_drop, DEV).cpu().double() if drop else None
    for dtype, norm_tol, entry_tol in ((torch.float32, F32_TOL, BLK_ENTRY_F32),
                                       (torch.bfloat16, BF16_NORM, BLK_ENTRY_BF16)):
        x = qkv.to(DEV, dtype).requires_grad_(True)
        ref_in = x.detach().cpu().double().requires_grad_(True)
        ref = _oracle_attn(ref_in, adj, nH, shifted, keep)
        ref.backward(do.to(dtype).double())
        out = HF.block_attention(x, bits, nH, shifted, drop=drop)
        out.backward(do.to(DEV, dtype))
        attn_parity(out, ref, x.grad, ref_in.grad, d, norm_tol, entry_tol, f"block tile-sparse {dtype}")


@pytest.mark.parametrize("hd,nH,KJ,F,B", [(64, 2, 29, 8, 2), (64, 4, 32, 4, 3), (32, 4, 29, 6, 2), (64, 2, 5, 2, 1),
                                          (64, 3, 31, 4, 1), (32, 3, 16, 4, 2)])     # odd head count, 1 / 16 pad slots
@pytest.mark.parametrize("shifted", [False, True])
def test_block_attention_with_attention_dropout(hd, nH, KJ, F, B, shifted):
    """attn_drop_rate > 0 (reference HGATE.py:78,106): the kernels' mask is the library's hash over the element index of the
    reference's (B f, nH, 2 KJ, 2 KJ) attention tensor, so hwgat_dropout_mask_f32 hands it to the oracle; forward and
    backward (which recomputes the mask), fp32 and bf16 storage -- i.e. the 32x32-tile kernels (fp32; bf16 at head_dim 32)
    and the 16x16-tile bf16 kernels (head_dim 64)."""
    g = torch.Generator().manual_seed(5 * hd + KJ + F)
    d, p_drop, seed = nH * hd, 0.2, 0xBEEF01
    qkv = torch.randn(B, F, KJ, 3 * d, generator=g) * 0.8
    do = torch.randn(B, F, KJ, d, generator=g)
    adj = _adj(KJ, g)
    bits = HF.blk_mask_bits(adj, KJ).to(DEV)
    keep = HF.dropout_mask((B, F // 2, nH, 2 * KJ, 2 * KJ), seed, p_drop, DEV).cpu().double()
    kept = keep[keep > 0]
    assert float((kept - 1.0 / (1.0 - p_drop)).abs().max()) < 1e-6 and abs(kept.numel() / keep.numel() - (1 - p_drop)) < 0.03

    ref_in = qkv.double().requires_grad_(True)
    ref = _oracle_attn(ref_in, adj, nH, shifted, keep)
    ref.backward(do.double())
    x = qkv.to(DEV).requires_grad_(True)
    out = HF.block_attention(x, bits, nH, shifted, drop=(seed, p_drop))
    out.backward(do.to(DEV))
    assert rel_err(out.detach().cpu(), ref.detach()) < F32_TOL
    assert rel_err(x.grad.cpu(), ref_in.grad) < F32_TOL
    attn_parity(out, ref, x.grad, ref_in.grad, d, F32_TOL, BLK_ENTRY_F32, "block fp32 dropout")
    # a different seed is a different mask; p = 0 is the plain kernel, bit for bit; the seed may come from the device word
    other = HF.block_attention(x.detach(), bits, nH, shifted, drop=(seed + 1, p_drop))
    assert rel_err(other.cpu(), ref.detach()) > 0.05
    assert torch.equal(HF.block_attention(x.detach(), bits, nH, shifted, drop=(seed, 0.0)), HF.block_attention(x.detach(), bits, nH, shifted))
    base = torch.tensor([1000], dtype=torch.int32, device=DEV)
    assert torch.equal(HF.block_attention(x.detach(), bits, nH, shifted, drop=(seed - 1000, p_drop, base)), out.detach())

    xb = qkv.to(DEV, torch.bfloat16).requires_grad_(True)
    refb_in = xb.detach().cpu().double().requires_grad_(True)
    refb = _oracle_attn(refb_in, adj, nH, shifted, keep)
    refb.backward(do.double())
    outb = HF.block_attention(xb, bits, nH, shifted, drop=(seed, p_drop))
    outb.backward(do.to(DEV, torch.bfloat16))
    assert rel_err(outb.detach().float().cpu(), refb.detach()) < BF16_TOL
    assert rel_err(xb.grad.float().cpu(), refb_in.grad) < 2 * BF16_TOL
    attn_parity(outb, refb, xb.grad, refb_in.grad, d, BF16_NORM, BLK_ENTRY_BF16, "block bf16 dropout")
    L = hw._lib
    o = torch.empty(B, F, KJ, d, device=DEV)
    assert L.lib().hwgat_blk_attn_fwd_drop(L.ptr(x), L.ptr(o), L.ptr(bits), B, F, KJ, nH, hd, int(shifted), 0, seed, 1.0, None, None) < 0


def test_block_attention_edge_rows():
    """exact-zero logits (-> -10000, HGATE.py:104) and a query whose every logit is zero: uniform over the
    58 REAL keys only -- the 6 pad slots of the 64-slot tile must not get any probability"""
    g = torch.Generator().manual_seed(5)
    B, F, KJ, nH, hd = 1, 4, 29, 2, 64
    d = nH * hd
    qkv = torch.randn(B, F, KJ, 3 * d, generator=g)
    qkv[0, 0, 3, :d] = 0.0            # a query row of zeros
    qkv[0, 1, 28, d:2 * d] = 0.0      # a key row of zeros (last joint: next to the pad slots)
    adj = OH.block_adjacency()
    bits = HF.blk_mask_bits(adj, KJ).to(DEV)
    for shifted in (False, True):
        ref_in = qkv.double().requires_grad_(True)
        ref = _oracle_attn(ref_in, adj, nH, shifted)
        ref.sum().backward()
        x = qkv.to(DEV).requires_grad_(True)
        out = HF.block_attention(x, bits, nH, shifted)
        out.sum().backward()
        assert rel_err(out.detach().cpu(), ref.detach()) < F32_TOL, shifted
        assert (x.grad.cpu() - ref_in.grad).abs().max() < 1e-5, shifted
        attn_parity(out, ref, x.grad, ref_in.grad, d, F32_TOL, BLK_ENTRY_F32, f"block fp32 edge rows shifted={shifted}")
        # bf16 storage: the 16x16-tile backward (blk_attn_bf16.hip) has its own copy of the masks / fill / pad logic
        xb = qkv.to(DEV, torch.bfloat16).requires_grad_(True)
        refb_in = xb.detach().cpu().double().requires_grad_(True)
        refb = _oracle_attn(refb_in, adj, nH, shifted)
        refb.sum().backward()
        outb = HF.block_attention(xb, bits, nH, shifted)
        outb.sum().backward()
        assert rel_err(outb.detach().float().cpu(), refb.detach()) < BF16_TOL, shifted
        assert rel_err(xb.grad.float().cpu(), refb_in.grad) < BF16_TOL, shifted
        assert bool(torch.isfinite(xb.grad).all())
        attn_parity(outb, refb, xb.grad, refb_in.grad, d, BF16_NORM, BLK_ENTRY_BF16, f"block bf16 edge rows shifted={shifted}")
    out = HF.block_attention(qkv.to(DEV), bits, nH, False).cpu()
    v = qkv[0, 0:2, :, 2 * d:].reshape(58, d)
    assert torch.allclose(out[0, 0, 3], v.mean(0), atol=1e-5)
    # outputs for a poisoned input stay confined: NaN in one block must not leak into another block
    q2 = qkv.clone()
    q2[0, 2, 7, 5] = float("nan")
    o2 = HF.block_attention(q2.to(DEV), bits, nH, False).cpu()
    assert torch.equal(o2[0, :2], out[0, :2])


def test_block_attention_argument_checks():
    x = torch.zeros(1, 2, 29, 3 * 128, device=DEV)
    o = torch.zeros(1, 2, 29, 128, device=DEV)
    bits = HF.blk_mask_bits(OH.block_adjacency(), 29).to(DEV)
    L = hw._lib
    rc = L.lib().hwgat_blk_attn_fwd(L.ptr(x), L.ptr(o), L.ptr(bits), 1, 3, 29, 2, 64, 0, 0, None)
    assert rc < 0          # odd frame count
    rc = L.lib().hwgat_blk_attn_fwd(L.ptr(x), L.ptr(o), L.ptr(bits), 1, 2, 33, 2, 64, 0, 0, None)
    assert rc < 0          # more than 32 joints
    rc = L.lib().hwgat_blk_attn_fwd(L.ptr(x), L.ptr(o), L.ptr(bits), 1, 2, 29, 1, 128, 0, 0, None)
    assert rc < 0          # head_dim 128 not built for the block kernel
    rc = L.lib().hwgat_blk_attn_bwd(L.ptr(x), None, L.ptr(x), L.ptr(bits), 1, 2, 29, 2, 64, 0, 0, None)
    assert rc < 0


def test_full_size_properties():
    """HGATE at the BASELINE batch (B64 T128 K29 d128): size-independent properties"""
    B, F, KJ, nH, hd = 64, 128, 29, 2, 64
    d = nH * hd
    g = torch.Generator(device=DEV).manual_seed(0)
    qkv = torch.randn(B, F, KJ, 3 * d, device=DEV, generator=g)
    bits = HF.blk_mask_bits(OH.block_adjacency(), KJ).to(DEV)
    for shifted in (False, True):
        q1 = qkv.clone()
        q1[..., 2 * d:] = 1.0
        assert (HF.block_attention(q1, bits, nH, shifted) - 1).abs().max() < 1e-5      # rows of P sum to 1
        a = HF.block_attention(qkv, bits, nH, shifted)
        q2 = qkv.clone()
        q2[..., 2 * d:] *= -2.0
        assert (HF.block_attention(q2, bits, nH, shifted) + 2 * a).abs().max() < 1e-4   # linear in V
        perm = torch.randperm(B, device=DEV)
        assert torch.equal(HF.block_attention(qkv[perm].contiguous(), bits, nH, shifted), a[perm])
    ref = _oracle_attn(qkv[7:8, :8].cpu().double(), OH.block_adjacency(), nH, False)
    assert rel_err(HF.block_attention(qkv[7:8, :8].contiguous(), bits, nH, False).cpu(), ref) < F32_TOL
    x = qkv.clone().requires_grad_(True)
    HF.block_attention(x, bits, nH, False).sum().backward()
    per_block = x.grad[..., 2 * d:].view(B, F // 2, 2 * KJ, d).sum(dim=2)            # dO == 1: dV sums to 58
    assert (per_block - 58).abs().max() < 1e-3
    x = qkv.clone()
    x[..., d:2 * d] = 1.0                                                            # k == 1 -> dq = 0
    x.requires_grad_(True)
    g2 = torch.randn(B, F, KJ, d, device=DEV, generator=g)
    HF.block_attention(x, bits, nH, True).backward(g2)
    assert x.grad[..., :d].abs().max() < 1e-3
    # the fp32 kernels of blk_attn_f32.hip walk several units per persistent workgroup here (8 192 units, 768 / 512
    # workgroups): the batch order does not change a bit of the gradients, and one clip equals the dense fp64 oracle
    for shifted in (False, True):
        x = qkv.clone().requires_grad_(True)
        HF.block_attention(x, bits, nH, shifted).backward(g2)
        perm = torch.randperm(B, device=DEV)
        xp = qkv[perm].contiguous().requires_grad_(True)
        HF.block_attention(xp, bits, nH, shifted).backward(g2[perm].contiguous())
        assert torch.equal(xp.grad, x.grad[perm])
        ref_in = qkv[5:6].cpu().double().requires_grad_(True)
        _oracle_attn(ref_in, OH.block_adjacency(), nH, shifted).backward(g2[5:6].cpu().double())
        assert rel_err(x.grad[5:6].cpu(), ref_in.grad) < F32_TOL


def test_full_size_properties_bf16_backward():
    """the bf16 backward on 16x16 tiles (blk_attn_bf16.hip) at the BASELINE batch: gradients do not depend on the batch
    order (bit for bit), dV of an all-ones dO sums to the number of queries, k == const gives dq == 0, and one clip
    against the dense fp64 oracle"""
    B, F, KJ, nH, hd = 64, 128, 29, 2, 64
    d = nH * hd
    g = torch.Generator(device=DEV).manual_seed(2)
    qkv = torch.randn(B, F, KJ, 3 * d, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, F, KJ, d, device=DEV, generator=g).to(torch.bfloat16)
    bits = HF.blk_mask_bits(OH.block_adjacency(), KJ).to(DEV)
    for shifted in (False, True):
        x = qkv.clone().requires_grad_(True)
        HF.block_attention(x, bits, nH, shifted).backward(do)
        perm = torch.randperm(B, device=DEV)
        xp = qkv[perm].contiguous().requires_grad_(True)
        HF.block_attention(xp, bits, nH, shifted).backward(do[perm].contiguous())
        assert torch.equal(xp.grad, x.grad[perm])
        ref_in = qkv[5:6].cpu().double().requires_grad_(True)
        _oracle_attn(ref_in, OH.block_adjacency(), nH, shifted).backward(do[5:6].cpu().double())
        assert rel_err(x.grad[5:6].float().cpu(), ref_in.grad) < BF16_TOL
    x = qkv.clone().requires_grad_(True)
    HF.block_attention(x, bits, nH, False).backward(torch.ones_like(do))
    per_block = x.grad[..., 2 * d:].float().view(B, F // 2, 2 * KJ, d).sum(dim=2)    # dO == 1: dV sums to 58 (P rounded to bf16)
    assert (per_block - 58).abs().max() < 0.5
    x = qkv.clone()
    x[..., d:2 * d] = 1.0                                                            # k == 1 -> dq = 0
    x.requires_grad_(True)
    HF.block_attention(x, bits, nH, True).backward(do)
    assert x.grad[..., :d].float().abs().max() < 2e-2


# ------------------------------------------------------------------------------------------ whole model
def _model_from_fixture(fx, dtype=torch.float32):
    oracle, params, cfg = hgate_oracle_from_fixture(fx)
    hp = hw.HGATEParams({"src_len": cfg["temporal_dim"], "num_class": cfg["num_classes"]}, cfg["kp_dim"], DEV,
                        embed_dim=cfg["embed_dim"])
    hp.num_heads = [int(h) for h in fx["heads"]]
    hp.drop_rate = 0.0
    model = hw.HGATEModel(*hp.get_model_params())
    res = model.load_state_dict(params, strict=False)
    assert not res.unexpected_keys and all(k.endswith("attn_mask") for k in res.missing_keys)
    return model.set_activation_dtype(dtype), params


@pytest.mark.parametrize("name", ["hgate_a.npz", "hgate_b.npz"])
@pytest.mark.parametrize("fused", [True, False])
def test_model_matches_reference_fixture(name, fused):
    fx = load_fixture(name)
    model, _ = _model_from_fixture(fx)
    if not fused:
        use_library_linears(model)
    x = torch.from_numpy(fx["x"]).to(DEV)
    y = torch.from_numpy(fx["y"]).to(DEV)
    crit = importlib.import_module("sl-hwgat_amd.train").SmoothedCrossEntropyLoss()
    for mode in ("eval", "train"):                    # no threshold, drop 0: the same function
        getattr(model, mode)()
        model.zero_grad()
        logits = model(x)
        loss = crit(logits, y)
        loss.backward()
        assert rel_err(logits.detach().cpu(), fx["eval.logits"]) < 1e-4, mode
        assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-4
        grad_digest_check({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, fx, "evalbwd.", 1e-3)
    model.eval()
    with torch.no_grad():
        assert rel_err(model.forward_features(x).cpu(), fx["eval.feat"]) < 1e-4


def test_model_bf16_and_state_dict_contract():
    fx = load_fixture("hgate_a.npz")
    model, params = _model_from_fixture(fx, torch.bfloat16)
    model.eval()
    with torch.no_grad():
        logits = model(torch.from_numpy(fx["x"]).to(DEV))
    assert rel_err(logits.float().cpu(), fx["eval.logits"]) < 1e-2                  # BASELINE configs[2] contract: bf16 within 1e-2 of fp32
    sd = model.state_dict()
    for k, v in fx.items():
        if k.startswith("mask."):
            assert torch.equal(sd[k[5:]].cpu().to(torch.uint8), torch.from_numpy(v)), k
    with pytest.raises(NotImplementedError):
        model.use_part_table(torch.arange(29))


def test_model_train_dropout_runs_and_is_seeded():
    hp = hw.HGATEParams({"src_len": 32, "num_class": 11}, 2, DEV)
    torch.manual_seed(3)
    model = hw.HGATEModel(*hp.get_model_params()).train()
    x = torch.rand(16, 32, 29, 2, device=DEV)
    a = model(x)
    model._drop_calls = 0
    b = model(x)
    assert torch.allclose(a, b, atol=1e-6) and torch.isfinite(a).all()    # same masks (pool sums use atomics)
    model.eval()
    assert (model(x) - a).abs().max() > 1e-3
    a.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@pytest.mark.parametrize("kind", ["hgate", "wgate"])
def test_sibling_models_with_attention_dropout_train_and_eval_ignores_it(kind):
    """attn_drop_rate is a constructor hyper-parameter of the reference's sibling models too (HGATE.py:232, WGATE.py:165):
    a model built with it runs train steps whose loss differs from the attn_drop_rate = 0 model on the same weights and
    seeds, produces finite gradients for every parameter, and its eval forward is identical to the plain model's."""
    torch.manual_seed(11)
    if kind == "hgate":
        hp = hw.HGATEParams({"src_len": 16, "num_class": 5}, 2, DEV)
        make = lambda: hw.HGATEModel(*hp.get_model_params()).to(DEV)
    else:
        hp = hw.WGATEParams({"src_len": 16, "num_class": 5}, 2, DEV, num_kps=32)
        make = lambda: hw.WGATEModel(*hp.get_model_params()).to(DEV)
    plain = make()
    hp.attn_drop_rate = 0.25
    dropped = make()
    dropped.load_state_dict(plain.state_dict())
    assert dropped.attn_drop_rate == 0.25 and plain.attn_drop_rate == 0.0
    x = torch.rand(4, 16, plain.num_kps, 2, device=DEV)
    plain.eval(); dropped.eval()
    assert torch.equal(plain(x), dropped(x))
    plain.train(); dropped.train()
    losses = []
    for m in (plain, dropped):
        m._drop_calls = 7
        out = m(x)
        loss = out.float().logsumexp(-1).sum()
        loss.backward()
        losses.append(float(loss.detach()))
        for n, q in m.named_parameters():
            if q.requires_grad:
                assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n
    assert abs(losses[0] - losses[1]) > 1e-6 * abs(losses[0])
