"""CPU: the host restatement of the dropout hash (tests/mask_helpers.py) pinned to vectors worked out by hand from the
comment and the formulas of csrc/fused_ops.h -- not from any implementation in this repository -- and the proof that the
comparisons of tests/test_gpu_leaf_kernels.py (tests/leaf_helpers.py) reject faults planted in results built on the CPU,
naming the entry, half, frame or slot, while the unfaulted results pass the same comparisons."""
import importlib

import numpy as np
import pytest
import torch

import leaf_helpers as LH
import mask_helpers as MH

hw_parts = importlib.import_module("sl-hwgat_amd.parts")


# ---------------------------------------------------------------------------------------------- fixed vectors
@pytest.mark.parametrize("seed,pair,want", [
    (0, 0, 0x00000000),
    (1, 0, 0x205F0435),
    (0, 1, 0x205F0435),
    (1234, 5, 0x1DED7408),
    (0xFFFFFFFF, 0x100000003, 0xE97DBF2A),
    (0x80000000, 123456789, 0x06541BA1),
])
def test_mix32_vectors(seed, pair, want):
    assert int(MH.mix32(seed, pair)) == want
    assert int(MH.mix32(np.array([seed, seed]), np.array([pair, pair], dtype=np.uint64))[1]) == want


@pytest.mark.parametrize("p,want", [
    (0.0, 0), (0.4 / 65536, 0), (0.6 / 65536, 1), (1e-5, 1), (0.1, 6554), (0.2, 13107), (0.5, 32768), (0.999, 65470),
    (0.99999, 65535),
])
def test_thresh_vectors(p, want):
    assert MH.thresh(p) == want


def test_keep_pattern_count_and_seed_wrap():
    assert MH.keep_bits(16, 0, 0.5).astype(int).tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1]
    assert int(MH.keep_bits(2 ** 20, 1234, 0.1).sum()) == 943559
    assert np.array_equal(MH.keep_mask(4099, 0xFFFFFFFF, 0.3, seed_base=2), MH.keep_mask(4099, 1, 0.3))
    assert not np.array_equal(MH.keep_mask(4099, 0xFFFFFFFF, 0.3), MH.keep_mask(4099, 1, 0.3))


def test_pair_halves_and_the_high_word_of_the_pair():
    # mix32(1, 0) = 0x205f0435: element 0 takes 0x0435 = 1077, element 1 takes 0x205f = 8287; thresh(0.1) = 6554
    assert MH.keep_bits(2, 1, 0.1).tolist() == [False, True]
    assert MH.keep_bits(2, 1, 0.01).tolist() == [True, True]          # thresh 655
    assert MH.keep_bits(2, 1, 0.2).tolist() == [False, False]         # thresh 13107
    # mix32(0xffffffff, 0x100000003) = 0xe97dbf2a: elements 0x200000006 / 7 take 0xbf2a = 48938 / 0xe97d = 59773;
    # thresh(0.8) = 52429.  (No entry point reaches such an index at a testable size: pinned here only.)
    assert MH.thresh(0.8) == 52429
    assert MH.keep_bits(2, 0xFFFFFFFF, 0.8, start=0x200000006).tolist() == [False, True]


def test_keep_mask_values():
    m = MH.keep_mask((3, 5, 7), 77, 0.1)
    assert m.dtype == np.float32 and m.shape == (3, 5, 7)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.1)))}
    assert np.array_equal(m.reshape(-1) != 0, MH.keep_bits(105, 77, 0.1))
    assert np.array_equal(MH.keep_mask(9, 5, 0.0), np.ones(9, dtype=np.float32))
    # p below half a step of 1 / 65536 drops nothing, but the survivors still carry 1 / (1 - p)
    tiny = MH.keep_mask(9, 5, 1e-6)
    assert (tiny == MH.scale(1e-6)).all() and MH.scale(1e-6) > 1.0
    assert abs((MH.keep_mask(2 ** 16, 3, 0.5) == 0).mean() - 0.5) < 0.01


# ---------------------------------------------------------------------------------------------- the mask comparison
def test_mask_check_rejects_a_shift_by_one_element_and_an_off_scale():
    p = 0.1
    ref = MH.keep_mask(2049, 1234, p)
    assert LH.mask_check(ref.copy(), ref, p) == float(MH.scale(p))
    first = int(np.flatnonzero((np.roll(ref, 1) == 0) != (ref == 0))[0])
    with pytest.raises(AssertionError, match=rf"kept / dropped differently, the first at entry {first}:"):
        LH.mask_check(np.roll(ref, 1), ref, p, "shifted")
    one_ulp = np.where(ref != 0, np.nextafter(MH.scale(p), np.float32(2.0)), np.float32(0.0)).astype(np.float32)
    LH.mask_check(one_ulp, ref, p)                                       # a division that is 1 ulp off is allowed
    two_ulp = np.where(ref != 0, np.nextafter(np.nextafter(MH.scale(p), np.float32(2.0)), np.float32(2.0)), np.float32(0.0))
    with pytest.raises(AssertionError, match="2 ulp from"):
        LH.mask_check(two_ulp.astype(np.float32), ref, p, "scale")
    kept = np.flatnonzero(ref)
    odd = ref.copy()
    odd[kept[40]] = 1.0
    with pytest.raises(AssertionError, match=rf"more than one value, the first other one at entry {int(kept[40])}"):
        LH.mask_check(odd, ref, p, "odd one")


# ---------------------------------------------------------------------------------------------- embed
def _embed_case(d0=64, C=2, J=29):
    B, T, K = 2, 5, 64
    x, bmat, pe = LH.embed_inputs(B, T, J, C, d0, 11)
    idx = hw_parts.part_table(J, 4)
    return x, idx, bmat, pe


@pytest.mark.parametrize("d0,C", [(64, 2), (192, 3)])
def test_embed_checks_pass_clean_results_and_name_a_wrong_pe_row_or_gather(d0, C):
    x, idx, bmat, pe = _embed_case(d0, C)
    ref = LH.embed_ref(x, idx, bmat, pe)
    cpu = LH.embed_ref(x, idx, bmat, pe, torch.float32)
    bound, d_cpu = LH.embed_f32_bound(cpu, ref)
    assert 1e-6 < d_cpu < 5e-5 and bound == 4 * d_cpu
    assert LH.embed_f32_check(cpu, ref, bound, "clean") == d_cpu
    LH.embed_bf16_check(cpu.to(torch.bfloat16), ref, "clean bf16")
    # the PE row of frame t + 1 in frame 2
    pe_bad = pe.clone()
    pe_bad[2] = pe[3]
    bad = LH.embed_ref(x, idx, bmat, pe_bad, torch.float32)
    with pytest.raises(AssertionError, match=r"error .* at clip \d frame 2 slot \d+ column \d+ \(the (sine|cosine) half"):
        LH.embed_f32_check(bad, ref, bound, "pe row")
    with pytest.raises(AssertionError, match=r"at clip \d frame 2 slot"):
        LH.embed_bf16_check(bad.to(torch.bfloat16), ref, "pe row bf16")
    # slot 5 gathered through idx[6]
    idx_bad = idx.clone()
    idx_bad[5] = idx[6]
    assert int(idx[5]) != int(idx[6])
    bad = LH.embed_ref(x, idx_bad, bmat, pe, torch.float32)
    with pytest.raises(AssertionError, match=r"at clip \d frame \d slot 5 column"):
        LH.embed_f32_check(bad, ref, bound, "gather")
    with pytest.raises(AssertionError, match=r"at clip \d frame \d slot 5 column"):
        LH.embed_bf16_check(bad.to(torch.bfloat16), ref, "gather bf16")


@pytest.mark.parametrize("d0", [64, 192, 256])
def test_embed_dropout_checks_name_the_cosine_half_masked_with_the_sine_index(d0):
    x, idx, bmat, pe = _embed_case(d0)
    p, seed = 0.1, 4321
    ref = LH.embed_ref(x, idx, bmat, pe)
    base = LH.embed_ref(x, idx, bmat, pe, torch.float32)
    keep = torch.from_numpy(MH.keep_mask(tuple(base.shape), seed, p))
    LH.bits_equal_check(base * keep, base * keep.clone(), "clean")
    sc = float(MH.scale(p))
    LH.embed_bf16_check((base * keep).to(torch.bfloat16), ref, "clean bf16", scale=sc, keep=keep, past_two=True)
    # why past_two: with the PE added, survivors of p = 0.1 reach [2, 4), where the correctly rounded fp64 result itself is
    # up to 2^-7 off -- more than 4.2e-3 / 0.9.  Without the PE (survivors below 1.12), and at p = 0.5 (a scale of exactly
    # 2 moves every value up one binade with its rounding step), the plain scaled bound is attainable and is what is held.
    best = (ref * keep.double()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match=r"error 0\.007\d+ >= 0\.00467"):
        LH.embed_bf16_check(best, ref, "best bf16", scale=sc, keep=keep)
    nope64, nope32 = LH.embed_ref(x, idx, bmat, None), LH.embed_ref(x, idx, bmat, None, torch.float32)
    LH.embed_bf16_check((nope32 * keep).to(torch.bfloat16), nope64, "clean bf16, no pe", scale=sc, keep=keep)
    keep5 = torch.from_numpy(MH.keep_mask(tuple(base.shape), seed, 0.5))
    LH.embed_bf16_check((base * keep5).to(torch.bfloat16), ref, "clean bf16, p = 0.5", scale=2.0, keep=keep5)
    half = d0 // 2
    keep_bad = keep.clone()
    keep_bad[..., half:] = keep[..., :half]                   # hashed with e0 + m instead of e0 + half + m
    assert bool((keep_bad[..., :half] == keep[..., :half]).all())
    with pytest.raises(AssertionError, match=r"entries differ, the first at clip 0 frame 0 slot 0 column \d+ \(the cosine half"):
        LH.bits_equal_check(base * keep_bad, base * keep, "cosine mask")
    with pytest.raises(AssertionError, match=r"kept / dropped differently, the first at clip 0 frame 0 slot 0 column \d+ \(the cosine"):
        LH.embed_bf16_check((base * keep_bad).to(torch.bfloat16), ref, "cosine mask bf16", scale=float(MH.scale(p)), keep=keep)
    # the whole mask one element late
    shifted = torch.roll(keep.flatten(), 1).view_as(keep)
    with pytest.raises(AssertionError, match="entries differ, the first at clip 0 frame 0 slot 0 column"):
        LH.bits_equal_check(base * shifted, base * keep, "shifted mask")


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("d0", [64, 128, 192, 1024])
@pytest.mark.parametrize("with_pe", [True, False])
def test_bf16_rounding_of_a_float32_embed_stays_inside_the_two_percent_cap(C, d0, with_pe):
    """the cap on entries that differ from the bf16 rounding of fp64 comes from d0 = 128 / 256 with x in [0, 1): before it
    is applied at the new widths and to signed coordinates, the float32 evaluation on the CPU has to stay well inside"""
    x, bmat, pe = LH.embed_inputs(2, 8, 16, C, d0, 100 * C + d0)
    pe = pe if with_pe else None
    ref = LH.embed_ref(x, None, bmat, pe)
    e_max, e_mean, flips = LH.embed_bf16_check(LH.embed_ref(x, None, bmat, pe, torch.float32).to(torch.bfloat16), ref, "cpu bf16")
    assert flips < 0.005


# ---------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_merge_check_names_a_swapped_pair_of_frames(dtype):
    x = LH.index_tensor((2, 6, 3, 8), dtype)
    ref = LH.merge_ref(x)
    assert ref.shape == (2, 3, 3, 16)
    LH.merge_check(ref.clone(), ref, "clean")
    LH.merge_check(LH.unmerge_ref(ref), x, "round trip", merged=False)
    # in words: out[b, f, k, tp d + c] = x[b, 2 f + tp, k, c]
    assert torch.equal(ref[1, 2, 1, 8:].float(), x[1, 5, 1].float()) and torch.equal(ref[1, 2, 1, :8].float(), x[1, 4, 1].float())
    swapped = x.clone()
    swapped[1, 2], swapped[1, 3] = x[1, 3], x[1, 2]
    with pytest.raises(AssertionError, match=r"the first at clip 1 merged frame 1 \(frame 2 of the pair\) slot 0 column 0"):
        LH.merge_check(LH.merge_ref(swapped), ref, "swapped")
    with pytest.raises(AssertionError, match=r"the first at clip 1 frame 2 slot 0 column 0"):
        LH.merge_check(swapped, x, "swapped back", merged=False)


# ---------------------------------------------------------------------------------------------- seq_embed
def test_seq_checks_name_a_dw_that_lacks_one_row_split():
    B, T, F, d, p, seed = 3, 37, 87, 128, 0.1, 99
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, T, F, generator=g) * 2 - 1
    W, b = torch.randn(d, F, generator=g) * 0.1, torch.randn(d, generator=g) * 0.1
    pe = LH.sinusoid(T, d)
    keep = MH.keep_mask((B, T, d), seed, p)
    ref = LH.seq_embed_ref(x, W, b, pe, keep)
    cpu = LH.seq_embed_ref(x, W, b, pe, keep, torch.float32)
    bounds = LH.seq_bounds(cpu, ref)
    assert bounds == (LH.KERNEL_ENTRY, LH.KERNEL_NORM)          # the fp32 evaluation is well below a quarter of K
    LH.seq_check(cpu, ref, bounds, "out")
    LH.seq_check(cpu.to(torch.bfloat16), ref, bounds, "out bf16", bf16_stored=True)
    with pytest.raises(AssertionError, match="entry-wise error"):
        LH.seq_check(cpu.to(torch.bfloat16), ref, bounds, "bf16 held to the fp32 bound")
    dout = torch.randn(B, T, d, generator=g)
    dW, db = LH.seq_embed_grads_ref(dout, x, keep, d)
    dW32, db32 = LH.seq_embed_grads_ref(dout, x, keep, d, torch.float32)
    LH.seq_check(dW32, dW, LH.seq_bounds(dW32, dW), "dW")
    LH.seq_check(db32, db, LH.seq_bounds(db32, db), "db")
    # 111 rows in splits of 32: the second one (rows 32 .. 63) never added
    lost_W, lost_b = LH.seq_embed_grads_ref(dout, x, keep, d, torch.float32, rows=slice(32, 64))
    with pytest.raises(AssertionError, match=r"dW: entry-wise error .* at entry \(\d+, \d+\)"):
        LH.seq_check(dW32 - lost_W, dW, LH.seq_bounds(dW32, dW), "dW")
    with pytest.raises(AssertionError, match=r"db: entry-wise error .* at entry \(\d+,\)"):
        LH.seq_check(db32 - lost_b, db, LH.seq_bounds(db32, db), "db")
    # a mask one element late, and a single padded frame that the words miss
    late = np.roll(keep.reshape(-1), 1).reshape(keep.shape)
    with pytest.raises(AssertionError, match=r"out: entry-wise error .* at entry \(\d, \d+, \d+\)"):
        LH.seq_check(LH.seq_embed_ref(x, W, b, pe, late, torch.float32), ref, bounds, "out")
    xp = x.clone()
    xp[1, 31] = -1.0
    xp[2, 36] = -1.0
    words = LH.pad_words(xp, -1.0)
    assert words.dtype == np.uint32 and words.tolist() == [[0, 0], [0x80000000, 0], [0, 1 << 4]]


# ---------------------------------------------------------------------------------------------- max pool
def test_torch_max_propagates_nan_with_the_first_index():
    """the behaviour the pool is held to: a NaN beats every number and the first NaN keeps its place"""
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, nan, -inf, 2.0], [nan, 5.0, -inf, 2.0], [3.0, nan, -inf, 7.0], [inf, 1.0, -inf, 7.0]]).view(1, 4, 4)
    v, i = x.max(dim=1)
    assert i.tolist() == [[1, 0, 0, 2]]
    assert torch.isnan(v[0, :2]).all() and v[0, 2] == -inf and v[0, 3] == 7.0


def test_pool_check_names_an_index_that_takes_the_last_tie():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6, 8, generator=g)
    x[1, 1, 3] = x[1, 4, 3] = 10.0
    xr = x.clone().requires_grad_(True)
    ref = xr.max(dim=1).values
    dout = torch.randn(2, 8, generator=g)
    ref.backward(dout)
    LH.pool_check(ref.detach().clone(), xr.grad.clone(), ref, xr.grad, "clean")
    bad = xr.grad.clone()
    bad[1, 4, 3], bad[1, 1, 3] = bad[1, 1, 3].item(), 0.0
    with pytest.raises(AssertionError, match=r"gradient of clip 1 column 3 lands on frames \[4\], torch.max's on \[1\]"):
        LH.pool_check(ref.detach(), bad, ref, xr.grad, "last tie")
    swallowed = ref.detach().clone()
    nan_ref = ref.detach().clone()
    nan_ref[0, 2] = float("nan")
    LH.pool_check(nan_ref.clone(), xr.grad, nan_ref, xr.grad, "nan equals nan")
    with pytest.raises(AssertionError, match=r"value of clip 0 column 2: .* vs nan"):
        LH.pool_check(swallowed, xr.grad, nan_ref, xr.grad, "swallowed nan")
