"""GPU: the small kernels at the two ends of every model, entry by entry -- hwgat_dropout_mask_f32 bit for bit against the
host restatement of the hash (tests/mask_helpers.py, itself pinned by hand-computed vectors in test_mask_hash_cpu.py),
hwgat_embed_fwd, hwgat_merge, hwgat_seq_embed_fwd / _bwd and hwgat_seq_maxpool_* against fp64 / exact torch restatements
(tests/leaf_helpers.py; test_mask_hash_cpu.py proves that those comparisons reject planted faults).  Every dropout mask here
comes from keep_mask on the host, never from the device.

Bounds and the worst error observed on an MI355X over this module's cases:
  embed fp32      bound min(2e-4, max(4 d_cpu, 1e-6)) absolute, d_cpu = the torch fp32 evaluation's own worst deviation
                  from fp64 (up to 4.8e-5 here, bound up to 1.9e-4): observed 4.8e-5, at most 0.25 of its case's bound
  embed bf16      max < 4.2e-3, mean < 1.2e-3, <= 2 % of entries off the bf16 rounding of fp64: observed 3.92e-3 /
                  1.07e-3 / 0.39 %; survivors of dropout: 7.8e-3 / 1.3e-3 at p = 0.1 (entries past 2, see
                  leaf_helpers.embed_bf16_check), 7.8e-3 / 2.1e-3 at p = 0.5 (bounds 8.4e-3 / 2.4e-3)
  seq_embed       entry (relative to the largest reference entry) / norm: max(4 d_cpu, 1.3e-5 / 5e-6) -- 4 d_cpu stayed
                  below the pair everywhere; a bf16-stored out gets 2^-8 |ref| per entry and 2^-9 in norm on top (the
                  entry figure quoted for it is what is left after that allowance)
                  fp32 storage: out 8.9e-7 / 4.2e-7, dW 3.4e-7 / 1.9e-7, db 1.9e-7 / 1.7e-7
                  bf16 storage: out 1.8e-7 / 1.78e-3 (bound 1.96e-3), dW 3.8e-7 / 1.9e-7, db 1.9e-7 / 1.9e-7
  mask (survivors carry exactly the restated scale), merge, max pool, fp32 embed dropout: exact."""
import importlib

import numpy as np
import pytest
import torch

import leaf_helpers as LH
import mask_helpers as MH

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.bfloat16]
WORST = {}


def _note(key, *vals):
    """keep and print the worst figures of a family (pytest -s shows them; the header of this module quotes them)"""
    old = WORST.get(key, tuple(0.0 for _ in vals))
    WORST[key] = tuple(max(a, b) for a, b in zip(old, vals))
    print(f"[leaf] {key}: " + " ".join(f"{v:.3g}" for v in vals) + "   worst so far " + " ".join(f"{v:.3g}" for v in WORST[key]))


def _word(value):
    """a device `seed_base` word"""
    value &= 0xFFFFFFFF
    return torch.tensor([value - (1 << 32) if value >= 1 << 31 else value], dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------- the mask kernel
MASK_N = [1, 2, 255, 256, 257, 2048 * 256 + 3]               # the last crosses the 2048-block grid cap (a grid-stride trip)
MASK_P = [0.0, 0.4 / 65536, 1e-5, 0.1, 0.5, 0.999, 0.99999]
MASK_SEEDS = [0, 1, 0x80000000, 0xFFFFFFFF]


@pytest.mark.parametrize("n", MASK_N)
def test_mask_kernel_bit_for_bit(n):
    """hwgat_dropout_mask_f32 == keep_mask for every p and seed: the same zero pattern, one survivor value, within 1 ulp
    of float32(1) / (float32(1) - float32(p)).  Element indices >= 2^32 (the high word of `pair`) would take a 16 GiB mask
    through this entry point: they are pinned on the host side only (test_mask_hash_cpu.py)."""
    exact = True
    for p in MASK_P:
        for seed in MASK_SEEDS:
            got = HF.dropout_mask((n,), seed, p, DEV).cpu().numpy()
            v = LH.mask_check(got, MH.keep_mask(n, seed, p), p, f"mask n={n} p={p:.3g} seed={seed:#x}")
            exact = exact and (v is None or v == float(MH.scale(p)))
    print(f"[leaf] mask n={n}: survivors carry exactly the restated scale: {exact}")


@pytest.mark.parametrize("seed,base", [(0xFFFFFFFF, 2), (0x80000001, 0x80000005), (7, 0), (1234, 0xDEADBEEF)])
def test_mask_kernel_adds_the_device_seed_word_with_wrap(seed, base):
    n, p = 4099, 0.2
    got = HF.dropout_mask((n,), seed, p, DEV, seed_base=_word(base)).cpu().numpy()
    LH.mask_check(got, MH.keep_mask(n, seed, p, seed_base=base), p, f"mask seed={seed:#x} + {base:#x}")
    wrapped = (seed + base) & 0xFFFFFFFF
    assert np.array_equal(got, HF.dropout_mask((n,), wrapped, p, DEV).cpu().numpy())
    if base:
        assert not np.array_equal(got, HF.dropout_mask((n,), seed, p, DEV).cpu().numpy())


# ---------------------------------------------------------------------------------------------- embed
def _embed_inputs(B, T, J, C, d0):
    nW = {29: 4, 133: 7}.get(J)
    idx = hw.part_table(J, nW) if nW else None
    K = nW * 16 if nW else J
    x, bmat, pe = LH.embed_inputs(B, T, J, C, d0, 1000 * C + d0 + 7 * J + B * T)
    return x, idx, bmat, pe, K


def _embed_run(x, idx, bmat, pe, K, dtype, **kw):
    dev = lambda t: None if t is None else t.to(DEV)          # noqa: E731
    return HF.embed(dev(x), dev(idx), dev(bmat), dev(pe), K, out_dtype=dtype, **kw).cpu()


def _embed_values(B, T, J, C, d0):
    x, idx, bmat, pe, K = _embed_inputs(B, T, J, C, d0)
    for table in (pe, None):
        ref = LH.embed_ref(x, idx, bmat, table)
        bound, d_cpu = LH.embed_f32_bound(LH.embed_ref(x, idx, bmat, table, torch.float32), ref)
        what = f"embed B T={B * T} J={J} C={C} d0={d0} pe={table is not None}"
        out = _embed_run(x, idx, bmat, table, K, torch.float32)
        assert out.shape == (B, T, K, d0)
        e = LH.embed_f32_check(out, ref, bound, what + " fp32")
        _note("embed fp32 (error, d_cpu, bound)", e, d_cpu, bound)
        _note("embed fp32 error / bound", e / bound)
        out_b = _embed_run(x, idx, bmat, table, K, torch.bfloat16)
        e_max, e_mean, flips = LH.embed_bf16_check(out_b, ref, what + " bf16")
        _note("embed bf16 (max, mean, flips)", e_max, e_mean, flips)


@pytest.mark.parametrize("J", [16, 29, 133])
@pytest.mark.parametrize("d0", [64, 128, 192, 1024])
@pytest.mark.parametrize("C", [2, 3])
def test_embed_against_fp64(C, d0, J):
    """every entry of hwgat_embed_fwd, fp32 and bf16, with and without the PE table, at B T = 1, 5 and 16 rows (5: not a
    multiple of the 4 waves of a block); d0 = 64 and 192 leave idle lanes in the last 64-lane trip over the half width
    (whose PE loads are guarded), 1024 takes 8 trips; J = 16 feeds the slots directly (idx = None), 29 and 133 go
    through hw.part_table"""
    for B, T in ((1, 1), (1, 5), (2, 8)):
        _embed_values(B, T, J, C, d0)


def test_embed_grid_stride_rows():
    """16 387 (clip, frame) rows: 4096 blocks of 4 waves take 16 384, three rows take the second grid-stride trip"""
    _embed_values(7, 2341, 16, 2, 64)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("d0", [64, 192, 256])
def test_embed_dropout_against_keep_mask(d0, p):
    """PositionalEncoding's dropout inside hwgat_embed_fwd, with a device seed word that wraps the sum.  fp32, with and
    without the PE: the output equals the p = 0 output of the same launch configuration times keep_mask((B, T, K, d0))
    bit for bit (the sine half hashes element e0 + m, the cosine half e0 + half + m).  bf16: dropped entries are exactly
    0, survivors are not, and the survivors are within 4.2e-3 / (1 - p) (mean 1.2e-3 / (1 - p)) of fp64 -- without the PE
    at p = 0.1 and with it at p = 0.5, where that bound is attainable; with the PE at p = 0.1 entries of 2 and more get
    the wider rounding step of their binade (leaf_helpers.embed_bf16_check, past_two)."""
    B, T, J, C = 2, 5, 29, 3
    x, idx, bmat, pe, K = _embed_inputs(B, T, J, C, d0)
    seed, base = 0xFFFFFF00 + d0, 0x1234
    keep = torch.from_numpy(MH.keep_mask((B, T, K, d0), seed, p, seed_base=base))
    sc = float(MH.scale(p))
    for table in (pe, None):
        what = f"embed dropout d0={d0} p={p} pe={table is not None}"
        plain = _embed_run(x, idx, bmat, table, K, torch.float32)
        drop = _embed_run(x, idx, bmat, table, K, torch.float32, drop_p=p, seed=seed, seed_base=_word(base))
        LH.bits_equal_check(drop, plain * keep, what + " fp32")
        drop_b = _embed_run(x, idx, bmat, table, K, torch.bfloat16, drop_p=p, seed=seed, seed_base=_word(base))
        ref = LH.embed_ref(x, idx, bmat, table)
        e_max, e_mean, _ = LH.embed_bf16_check(drop_b, ref, what + " bf16", scale=sc, keep=keep,
                                               past_two=table is not None and p == 0.1)
        _note(f"embed bf16 dropout p={p} (max, mean)", e_max, e_mean)


# ---------------------------------------------------------------------------------------------- merge
MERGE_SHAPES = [(1, 2, 16, 64), (2, 8, 32, 128), (3, 6, 80, 192), (2, 4, 29, 72)]
# the last of each list has more than 1 048 576 16-byte chunks (4096 blocks x 256 threads): a grid-stride trip
MERGE_LAST = {torch.float32: (5, 6, 144, 1024), torch.bfloat16: (5, 12, 144, 1024)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(5))
def test_merge_is_the_torch_permutation(i, dtype):
    """forward and backward of HF.temporal_merge bit-equal to the reshape / transpose of TemporalMerging; fp32 elements
    carry their own flat index, bf16 elements the bit pattern of it, so no wrong permutation can pass"""
    shape = (MERGE_SHAPES + [MERGE_LAST[dtype]])[i]
    B, F, K, d = shape
    if i == 4:
        assert B * F * K * d * (4 if dtype == torch.float32 else 2) // 16 > 4096 * 256
    x = LH.index_tensor(shape, dtype)
    xg = x.to(DEV).requires_grad_(True)
    out = HF.temporal_merge(xg)
    LH.merge_check(out, LH.merge_ref(x), f"merge {shape} {dtype}")
    dout = LH.index_tensor((B, F // 2, K, 2 * d), dtype)
    out.backward(dout.to(DEV))
    LH.merge_check(xg.grad, LH.unmerge_ref(dout), f"merge backward {shape} {dtype}", merged=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_refuses_odd_frames_and_ragged_widths(dtype):
    epv = 4 if dtype == torch.float32 else 8
    with pytest.raises(RuntimeError, match="ESHAPE"):
        HF.temporal_merge(torch.zeros(1, 3, 16, 64, device=DEV, dtype=dtype))
    for d in (epv + 1, epv + 2, 64 + epv // 2):
        with pytest.raises(RuntimeError, match="ESHAPE"):
            HF.temporal_merge(torch.zeros(1, 2, 16, d, device=DEV, dtype=dtype))
    HF.temporal_merge(torch.zeros(1, 2, 16, epv, device=DEV, dtype=dtype))


# ---------------------------------------------------------------------------------------------- seq_embed
SEQ_SHAPES = [(1, 1, 58, 192), (2, 32, 58, 64), (3, 37, 87, 128), (2, 65, 399, 512), (2, 33, 512, 200), (7, 293, 87, 128)]
PAD_INDEX = -1.0


def _pad_frames(kind, B, T):
    """[(clip, frame)] of the padded frames; None where the shape has no such frame"""
    if kind == "none":
        return []
    if kind == "clip":                                        # one whole clip (the middle one where there are three)
        return [(B // 2, t) for t in range(T)]
    if kind == "frame31":                                     # bit 31 of a padding word
        return [(B - 1, 31)] if T >= 32 else None
    return [(0, T - 1)]                                       # "last"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,F,d", SEQ_SHAPES)
def test_seq_embed_and_its_gradients_against_fp64(B, T, F, d, dtype):
    """hwgat_seq_embed_fwd / _bwd at p = 0 and 0.1 under four padding patterns: F > 128 (399, 512) runs the backward's loop
    over feature pieces, d = 512 the forward's column loop, d = 200 the ragged last 64-column block, M = B T = 1 a single
    short split and M = 2051 33 splits, T = 32 / 33 / 65 / 293 the word boundaries of the padding bits.  out, dW and db
    entry by entry and in norm against fp64 with the host's keep_mask; padding words exact; two backward runs
    bit-equal."""
    g = torch.Generator().manual_seed(B * 1000 + T + F + d)
    W, b = torch.randn(d, F, generator=g) * 0.1, torch.randn(d, generator=g) * 0.1
    pe = LH.sinusoid(T, d)
    dout = torch.randn(B, T, d, generator=g).to(dtype)
    Wt = W.t().contiguous().to(DEV)
    stored = dtype == torch.bfloat16
    seed, base = 99 + T, 0xFFFFFFF0
    for kind in ("none", "clip", "frame31", "last"):
        frames = _pad_frames(kind, B, T)
        if frames is None:
            continue
        x = torch.rand(B, T, F, generator=g) * 2 - 1
        x[x == PAD_INDEX] = -0.5
        for bb, t in frames:
            x[bb, t] = PAD_INDEX
        want_words = LH.pad_words(x, PAD_INDEX)
        assert int(np.unpackbits(want_words.view(np.uint8)).sum()) == len(frames)
        for p in (0.0, 0.1):
            what = f"seq_embed {(B, T, F, d)} {dtype} pad={kind} p={p}"
            keep = MH.keep_mask((B, T, d), seed, p, seed_base=base) if p else None
            word = _word(base) if p else None
            out, words = HF.seq_embed(x.to(DEV), Wt, b.to(DEV), pe.to(DEV), dtype, PAD_INDEX, p, seed, word)
            got_words = words.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_words, want_words), (what, "padding words", got_words.tolist(), want_words.tolist())
            ref = LH.seq_embed_ref(x, W, b, pe, keep)
            bounds = LH.seq_bounds(LH.seq_embed_ref(x, W, b, pe, keep, torch.float32), ref)
            _note(f"seq_embed out {dtype} (entry, norm)", *LH.seq_check(out, ref, bounds, what + " out", bf16_stored=stored))
            runs = []
            for _ in range(2):
                dW, db = torch.zeros(d, F, device=DEV), torch.zeros(d, device=DEV)
                HF.seq_embed_backward(dout.to(DEV), x.to(DEV), dW, db, p, seed, word)
                runs.append((dW.cpu(), db.cpu()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what + ": backward not bit-reproducible"
            dW_ref, db_ref = LH.seq_embed_grads_ref(dout, x, keep, d)
            dW32, db32 = LH.seq_embed_grads_ref(dout, x, keep, d, torch.float32)
            _note(f"seq_embed dW {dtype} (entry, norm)", *LH.seq_check(runs[0][0], dW_ref, LH.seq_bounds(dW32, dW_ref), what + " dW"))
            _note(f"seq_embed db {dtype} (entry, norm)", *LH.seq_check(runs[0][1], db_ref, LH.seq_bounds(db32, db_ref), what + " db"))


def test_seq_embed_backward_accumulates_and_takes_no_bias_gradient():
    """dW and db are added to what the buffers hold; db = None is allowed"""
    B, T, F, d = 2, 33, 133, 200
    g = torch.Generator().manual_seed(8)
    x, dout = torch.rand(B, T, F, generator=g) * 2 - 1, torch.randn(B, T, d, generator=g)
    dW0, db0 = torch.randn(d, F, generator=g), torch.randn(d, generator=g)
    dW, db = dW0.to(DEV), db0.to(DEV)
    HF.seq_embed_backward(dout.to(DEV), x.to(DEV), dW, db)
    dW_ref, db_ref = LH.seq_embed_grads_ref(dout, x, None, d)
    dW32, db32 = LH.seq_embed_grads_ref(dout, x, None, d, torch.float32)
    LH.seq_check(dW, dW_ref + dW0.double(), LH.seq_bounds(dW32 + dW0, dW_ref + dW0.double()), "dW on top")
    LH.seq_check(db, db_ref + db0.double(), LH.seq_bounds(db32 + db0, db_ref + db0.double()), "db on top")
    dW2 = dW0.to(DEV)
    HF.seq_embed_backward(dout.to(DEV), x.to(DEV), dW2, None)
    assert torch.equal(dW2, dW)


# ---------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T,d", [(1, 1, 64), (3, 37, 128), (2, 512, 200)])
def test_max_pool_equals_torch_max(B, T, d, dtype):
    """value and gradient of HF.seq_max_pool equal torch.max's exactly: ties (the first index wins) at frame 0, mid-clip
    and the last frame, a column of -inf, a NaN in frame 0 and NaNs in later frames (a NaN wins, the first one's index)"""
    g = torch.Generator().manual_seed(T + d)
    x = torch.randn(B, T, d, generator=g)
    nan, inf = float("nan"), float("inf")
    x[:, :, 5] = -inf
    x[0, 0, 6] = nan
    if T > 8:
        b = B - 1
        x[b, 0, 0] = x[b, 5, 0] = 10.0                         # ties of the maximum: frame 0 and later
        x[b, T // 2, 1] = x[b, T // 2 + 3, 1] = x[b, T - 2, 1] = 10.0
        x[b, T - 4, 2] = x[b, T - 1, 2] = 10.0                 # ... with the last frame
        x[b, 3:, 3] = x[b, 3, 3]                               # a run of equal values that may or may not hold the maximum
        x[0, 7, 7] = nan                                       # one NaN after the start, larger values behind it
        x[0, 8, 7] = 50.0
        x[0, 4, 8] = x[0, T - 1, 8] = nan                      # two NaNs: the first keeps the index
        x[0, T - 1, 9] = nan                                   # a NaN in the last frame only
        x[0, 2, 10], x[0, 6, 10] = inf, nan                    # +inf ahead of a NaN
    x = x.to(dtype)
    xr = x.float().clone().requires_grad_(True)
    ref = xr.max(dim=1).values
    dout = torch.randn(B, d, generator=g)
    ref.backward(dout)
    xd = x.to(DEV).requires_grad_(True)
    out = HF.seq_max_pool(xd)
    assert out.dtype == torch.float32
    out.backward(dout.to(DEV))
    LH.pool_check(out, xd.grad, ref, xr.grad.to(dtype), f"max pool {(B, T, d)} {dtype}")
    assert bool(torch.isnan(out[0, 6])) and bool(torch.isinf(out[:, 5]).all())
