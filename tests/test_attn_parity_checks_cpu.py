"""CPU proof that helpers.attn_parity has teeth: faults planted in fp64 oracle results that the old combined norm checks
of the bf16 attention tests accept (output rel_err < 1e-2, whole dqkv rel_err < 2e-2) must be rejected by attn_parity at
the bf16 bounds (o in norm 1e-2, each gradient part in its own norm 2e-2, every part entry-wise 2e-2)."""
import pytest
import torch

from helpers import attn_parity, entrywise, rel_err
from oracle import hgat_oracle as OH
from oracle import wgat_oracle as OW

OLD_OUT, OLD_GRAD = 1e-2, 2e-2
NORM = dict(o=1e-2, dq=2e-2, dk=2e-2, dv=2e-2)
ENTRY = 2e-2


def _block_case(hd=64, nH=2, KJ=29, F=8, B=2, seed=0):
    """unshifted HGATE block attention on the shipped skeleton: (out, dqkv) of the fp64 oracle"""
    g = torch.Generator().manual_seed(seed)
    d = nH * hd
    qkv = (torch.randn(B, F, KJ, 3 * d, generator=g) * 0.8).double().requires_grad_(True)
    do = torch.randn(B, F, KJ, d, generator=g).double()
    w = qkv.reshape(B, F // 2, 2 * KJ, 3, nH, hd).permute(3, 0, 1, 4, 2, 5)
    o, _ = OH.block_attention(w[0], w[1], w[2], OH.block_adjacency().double())
    o = o.reshape(B, F, KJ, d)
    o.backward(do)
    return o.detach(), qkv.grad.detach()


def _band_case(hd=16, nH=2, nW=1, F=32, B=1, seed=0):
    """WGATE band attention: (out, dqkv) of the dense fp64 oracle"""
    g = torch.Generator().manual_seed(seed)
    d, K = nH * hd, nW * 16
    qkv = (torch.randn(B, F, K, 3 * d, generator=g) * 0.8).double().requires_grad_(True)
    do = torch.randn(B, F, K, d, generator=g).double()
    w = OW.to_windows(qkv).reshape(B, nW, F * 16, 3, nH, hd).permute(3, 0, 1, 4, 2, 5)
    o, _ = OW.band_attention(w[0], w[1], w[2], OW.additive_mask(OW.band_adjacency(F, nW).double()))
    o = OW.from_windows(o, F)
    o.backward(do)
    return o.detach(), qkv.grad.detach()


def _old_checks_accept(out, ref, dqkv, ref_dqkv):
    e_out, e_grad = rel_err(out, ref), rel_err(dqkv, ref_dqkv)
    assert e_out < OLD_OUT and e_grad < OLD_GRAD, (e_out, e_grad)
    return e_out, e_grad


def test_exact_results_pass_and_report_every_part():
    ref, gref = _block_case()
    errs = attn_parity(ref.clone(), ref, gref.clone(), gref, 128, NORM, ENTRY)
    assert set(errs) == {"o", "dq", "dk", "dv"} and all(e == (0.0, 0.0) for e in errs.values())
    # a fault is reported with its part and its worst index
    bad = gref.clone()
    bad[1, 3, 7, 128 + 5] += 1.0
    with pytest.raises(AssertionError, match=r"dk: entry-wise error .*\(1, 3, 7, 5\)"):
        attn_parity(ref, ref, bad, gref, 128, NORM, ENTRY)


def test_block_dq_scaled_by_1_04_is_rejected():
    ref, gref = _block_case()
    d = 128
    bad = gref.clone()
    bad[..., :d] *= 1.04
    _, e_grad = _old_checks_accept(ref, ref, bad, gref)
    assert e_grad > 0.01                                     # a fault the old bound only just tolerated
    assert rel_err(bad[..., :d], gref[..., :d]) == pytest.approx(0.04)
    with pytest.raises(AssertionError, match="dq: norm error"):
        attn_parity(ref, ref, bad, gref, d, NORM, ENTRY)
    with pytest.raises(AssertionError, match="dq: entry-wise error"):
        attn_parity(ref, ref, bad, gref, d, 1.0, ENTRY)       # the entry-wise check alone catches it too


def test_block_one_head_at_one_query_slot_scaled_by_1_2_is_rejected():
    ref, gref = _block_case()
    B, F, KJ, d = ref.shape
    nH, hd = 2, 64
    heads = ref.view(B, F, KJ, nH, hd)
    b, f, k, h, c = (int(i) for i in torch.unravel_index(heads.abs().argmax(), heads.shape))
    bad = ref.clone()
    bad.view(B, F, KJ, nH, hd)[b, f, k, h] *= 1.2            # one head of the query slot that holds the largest |o|
    e_out, _ = _old_checks_accept(bad, ref, gref, gref)
    assert e_out > 0.005
    assert entrywise(bad, ref) == pytest.approx(0.2)
    with pytest.raises(AssertionError, match=rf"o: entry-wise error .*\({b}, {f}, {k}, {h * hd + c}\)"):
        attn_parity(bad, ref, gref, gref, d, NORM, ENTRY)


def test_band_dk_of_one_head_in_one_frame_segment_scaled_by_1_08_is_rejected():
    ref, gref = _band_case()
    d, hd = 32, 16
    bad = gref.clone()
    bad[:, 16:32, :, d:d + hd] *= 1.08                       # dk of head 0, frames 16-31: one 16-frame segment
    _, e_grad = _old_checks_accept(ref, ref, bad, gref)
    assert e_grad > 0.01
    assert rel_err(bad[..., d:2 * d], gref[..., d:2 * d]) > 2e-2
    with pytest.raises(AssertionError, match="dk: norm error"):
        attn_parity(ref, ref, bad, gref, d, NORM, ENTRY)
    with pytest.raises(AssertionError, match="dk: entry-wise error"):
        attn_parity(ref, ref, bad, gref, d, 1.0, ENTRY)
