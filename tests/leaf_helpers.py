"""References and comparisons of the leaf kernels (embed.hip, seq_embed.hip, the dropout mask): plain torch restatements
at any precision, and the checks tests/test_gpu_leaf_kernels.py holds the kernels to.  Everything here runs on the CPU, so
tests/test_mask_hash_cpu.py can prove that each check rejects a planted fault and names where it sits."""
import math

import numpy as np
import torch

import mask_helpers as MH

# ---------------------------------------------------------------------------------------------- bounds
EMBED_F32_CAP, EMBED_F32_FLOOR = 2e-4, 1e-6                 # absolute; the cap is what test_embed has always used
EMBED_BF16_MAX, EMBED_BF16_MEAN, EMBED_BF16_FLIPS = 4.2e-3, 1.2e-3, 0.02
KERNEL_ENTRY, KERNEL_NORM = 1.3e-5, 5e-6                    # the pair of tests/test_gpu_stgcn.py
BF16_ENTRY = 2.0 ** -8                                      # per entry, relative to that entry, for a bf16-stored result
BF16_NORM = 2.0 ** -9                                       # round-to-nearest: at most half an ulp of every entry


def where(flat, shape):
    return tuple(int(i) for i in np.unravel_index(int(flat), tuple(shape)))


# ---------------------------------------------------------------------------------------------- the mask itself
def mask_check(got, ref, p, what=""):
    """bit for bit: the zero pattern of `got` equals that of keep_mask's `ref`, every survivor carries ONE bit pattern,
    and that pattern is within 1 ulp of the restated scale.  Returns the survivors' value (None if there are none)."""
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref, dtype=np.float32).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gz, rz = got.view(np.uint32) == 0, ref.view(np.uint32) == 0          # (-0.0 is not a zero of the mask)
    bad = np.flatnonzero(gz != rz)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} entries kept / dropped differently, the first at entry "
                           f"{int(bad[0])}: {got[bad[0]]!r} vs {ref[bad[0]]!r}")
    kept = got[~gz].view(np.uint32)
    if kept.size == 0:
        return None
    odd = np.flatnonzero(kept != kept[0])
    assert odd.size == 0, (f"{what}: survivors carry more than one value, the first other one at entry "
                           f"{int(np.flatnonzero(~gz)[odd[0]])}")
    sc = MH.scale(p)
    ulps = abs(int(kept[0]) - int(np.asarray(sc, dtype=np.float32).view(np.uint32)))
    assert ulps <= 1, f"{what}: survivors carry {kept[:1].view(np.float32)[0]!r}, {ulps} ulp from 1 / (1 - p) = {sc!r}"
    return float(kept[:1].view(np.float32)[0])


# ---------------------------------------------------------------------------------------------- embed
def embed_ref(x, idx, bmat, pe, dtype=torch.float64):
    """x (B, T, J, C), idx (K,) or None, bmat (d0 / 2, C), pe (T, d0) or None, all fp32 -> (B, T, K, d0) in `dtype`:
    cat[sin, cos]((2 pi x[:, :, idx]) @ bmat^T) + pe[t]"""
    xs = x if idx is None else x[:, :, idx.long()]
    proj = (2.0 * math.pi * xs.to(dtype)) @ bmat.to(dtype).t()
    out = torch.cat([proj.sin(), proj.cos()], dim=-1)
    if pe is not None:
        out = out + pe.to(dtype)[None, :, None, :]
    return out


def sinusoid(T, d):
    """(T, d) fp32 table, sines in the even columns and cosines in the odd ones (PositionalEncoding)"""
    pe = torch.zeros(T, d)
    pos = torch.arange(0, T).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def embed_inputs(B, T, J, C, d0, seed):
    """x uniform in [-1, 1) (every joint of every frame its own coordinates, so a wrong gather or PE row moves every
    entry), bmat = 10 randn as the model draws it, pe the sinusoid table of exactly T rows"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, T, J, C, generator=g) * 2 - 1
    bmat = torch.randn(d0 // 2, C, generator=g) * 10
    return x, bmat, sinusoid(T, d0)


def _embed_where(flat, shape):
    b, t, k, c = where(flat, shape)
    half = shape[-1] // 2
    return f"clip {b} frame {t} slot {k} column {c} (the {'sine' if c < half else 'cosine'} half, m = {c % half})"


def embed_f32_bound(cpu32, ref64):
    """min(2e-4, max(4 d_cpu, 1e-6)) with d_cpu = the worst deviation of the torch fp32 evaluation on the CPU from fp64"""
    d_cpu = float((cpu32.double() - ref64).abs().max())
    return min(EMBED_F32_CAP, max(4.0 * d_cpu, EMBED_F32_FLOOR)), d_cpu


def embed_f32_check(got, ref64, bound, what=""):
    """every entry within `bound` (absolute); returns the worst error"""
    got = torch.as_tensor(got).detach().cpu()
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got.double() - ref64).abs()
    flat = int(err.argmax())
    e = float(err.flatten()[flat])
    assert e < bound, (f"{what}: error {e:.3g} >= {bound:.3g} at {_embed_where(flat, got.shape)}: "
                       f"{float(got.flatten()[flat]):.7g} vs {float(ref64.flatten()[flat]):.7g}")
    return e


def embed_bf16_check(got, ref64, what="", scale=1.0, keep=None, past_two=False):
    """test_embed's three conditions on a bf16 result: max error < 4.2e-3, mean error < 1.2e-3, at most 2 % of the entries
    differ from the bf16 rounding of fp64.  With `keep` (a keep_mask of the result's shape) and scale = 1 / (1 - p): the
    zero pattern is keep's exactly, and the survivors are held to the first two bounds times `scale`.
    past_two: 4.2e-3 is half a bf16 step below 2 (2^-8) plus 2.9e-4 for the arithmetic.  With the PE added a survivor
    reaches 2 / (1 - p), and unless 1 / (1 - p) is a power of two some land in [2, 4), where half a step is 2^-7: the
    correctly rounded result itself misses 4.2e-3 / (1 - p) there (0.0078 against 0.0047 at p = 0.1).  Only for those
    runs, and only for entries whose reference is >= 2, the bound is 2^-7 + 2.9e-4 / (1 - p); everything else keeps
    4.2e-3 / (1 - p).
    Returns (max, mean, fraction that differs or None)."""
    got = torch.as_tensor(got).detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == ref64.shape, (what, got.dtype, tuple(got.shape))
    g = got.double()
    assert bool(torch.isfinite(g).all()), f"{what}: not finite"
    if keep is not None:
        keep = torch.as_tensor(keep).double()
        # every dropped entry is 0; every survivor is not -- except where the value itself is 0: in frame 0 the PE is exactly
        # 0 or 1, and sin / cos round to -1 in float32 for one argument in ~10^4, so a handful of survivors ARE 0.  A
        # survivor may be 0 only where |reference| <= 1e-3 (5 x the fp32 bound; bf16 holds 1e-3 with 8 bits to spare).
        zp = ((g == 0) != (keep == 0)) & ((keep == 0) | (ref64.abs() > 1e-3))
        assert not bool(zp.any()), (f"{what}: {int(zp.sum())} entries kept / dropped differently, the first at "
                                    f"{_embed_where(int(zp.flatten().int().argmax()), got.shape)}")
        ref64 = ref64 * keep
        sel = keep != 0
    else:
        sel = torch.ones_like(g, dtype=torch.bool)
    err = (g - ref64).abs()
    bound = torch.full_like(err, EMBED_BF16_MAX * scale)
    if past_two:
        bound[ref64.abs() >= 2.0] = 2.0 ** -7 + (EMBED_BF16_MAX - 2.0 ** -8) * scale
    flat = int((err - bound).argmax())
    e_max, e_mean = float(err.flatten()[flat]), float(err[sel].mean()) if bool(sel.any()) else 0.0
    assert e_max < float(bound.flatten()[flat]), (f"{what}: error {e_max:.3g} >= {float(bound.flatten()[flat]):.3g} at "
                                                  f"{_embed_where(flat, got.shape)}: {float(g.flatten()[flat]):.6g} vs "
                                                  f"{float(ref64.flatten()[flat]):.6g}")
    e_max = float(err.max())
    assert e_mean < EMBED_BF16_MEAN * scale, f"{what}: mean error {e_mean:.3g} >= {EMBED_BF16_MEAN * scale:.3g}"
    flips = None
    if keep is None:
        diff = got != ref64.to(torch.bfloat16)
        flips = float(diff.double().mean())
        assert flips <= EMBED_BF16_FLIPS, (f"{what}: {flips:.3%} of the entries differ from the bf16 rounding of fp64, the "
                                           f"first at {_embed_where(int(diff.flatten().int().argmax()), got.shape)}")
    return e_max, e_mean, flips


def bits_equal_check(got, ref, what="", name=_embed_where):
    """bit for bit (fp32 through int32, bf16 through int16, so that -0.0, NaN payloads and index patterns count)"""
    got, ref = torch.as_tensor(got).detach().cpu().contiguous(), torch.as_tensor(ref).detach().cpu().contiguous()
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, tuple(got.shape), tuple(ref.shape))
    view = {4: torch.int32, 2: torch.int16}[got.element_size()]
    bad = got.view(view) != ref.view(view)
    if bool(bad.any()):
        flat = int(bad.flatten().int().argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} entries differ, the first at {name(flat, got.shape)}: "
                             f"{float(got.flatten()[flat])!r} vs {float(ref.flatten()[flat])!r}")


# ---------------------------------------------------------------------------------------------- merge
def merge_ref(x):
    """TemporalMerging: (B, F, K, d) -> (B, F / 2, K, 2 d), out[b, f, k, tp d + c] = x[b, 2 f + tp, k, c]"""
    B, F, K, d = x.shape
    return x.reshape(B, F // 2, 2, K, d).transpose(2, 3).reshape(B, F // 2, K, 2 * d)


def unmerge_ref(y):
    B, f, K, d2 = y.shape
    return y.reshape(B, f, K, 2, d2 // 2).transpose(2, 3).reshape(B, 2 * f, K, d2 // 2)


def _merged_where(flat, shape):
    b, f, k, c = where(flat, shape)
    d = shape[-1] // 2
    return f"clip {b} merged frame {f} (frame {2 * f + c // d} of the pair) slot {k} column {c}"


def _frame_where(flat, shape):
    b, f, k, c = where(flat, shape)
    return f"clip {b} frame {f} slot {k} column {c}"


def merge_check(got, ref, what="", merged=True):
    bits_equal_check(got, ref, what, _merged_where if merged else _frame_where)


def index_tensor(shape, dtype):
    """fp32: every element is its own flat index (exact below 2^24); bf16: the bit pattern (flat index mod 65521)"""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        assert n < 2 ** 24
        return torch.arange(n, dtype=torch.float32).reshape(shape)
    bits = (torch.arange(n, dtype=torch.int64) % 65521).to(torch.int32)
    bits = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(shape)


# ---------------------------------------------------------------------------------------------- seq_embed
def pad_words(x, pad_index):
    """uint32 (B, ceil(T / 32)): bit t % 32 of word t / 32 set iff x[b, t, 0] == pad_index"""
    B, T = x.shape[:2]
    hit = (x[:, :, 0] == pad_index).numpy()
    words = np.zeros((B, (T + 31) // 32), dtype=np.uint32)
    for t in range(T):
        words[:, t // 32] |= hit[:, t].astype(np.uint32) << np.uint32(t % 32)
    return words


def seq_embed_ref(x, W, b, pe, keep, dtype=torch.float64):
    """drop((x W^T + b) sqrt(d) + pe[t]) in `dtype`; keep: keep_mask of (B, T, d) or None"""
    d = W.shape[0]
    out = (x.to(dtype) @ W.to(dtype).t() + b.to(dtype)) * torch.tensor(math.sqrt(d), dtype=dtype)
    if pe is not None:
        out = out + pe.to(dtype)
    return out if keep is None else out * torch.as_tensor(keep).to(dtype)


def seq_embed_grads_ref(dout, x, keep, d, dtype=torch.float64, rows=None):
    """(dW (d, F), db (d)) of seq_embed_ref for the upstream gradient `dout` (already rounded to the storage type);
    rows: a slice of the B T rows to sum over (default all)"""
    g = dout.to(dtype).reshape(-1, d)
    if keep is not None:
        g = g * torch.as_tensor(keep).to(dtype).reshape(-1, d)
    g = g * torch.tensor(math.sqrt(d), dtype=dtype)
    xf = x.to(dtype).reshape(g.shape[0], -1)
    if rows is not None:
        g, xf = g[rows], xf[rows]
    return g.t() @ xf, g.sum(0)


def deviation(a, ref64):
    """(entry, norm): worst entry-wise error relative to the largest reference entry, and the relative error in norm"""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref64).detach().cpu().double()
    diff = a - b
    return (float(diff.abs().max() / b.abs().max().clamp_min(1e-30)), float(diff.norm() / b.norm().clamp_min(1e-30)))


def seq_bounds(cpu32, ref64):
    """(entry, norm) = max(4 d_cpu, K): d_cpu the deviation of the torch fp32 evaluation on the CPU, K the pair above"""
    de, dn = deviation(cpu32, ref64)
    return max(4.0 * de, KERNEL_ENTRY), max(4.0 * dn, KERNEL_NORM)


def seq_check(got, ref64, bounds, what="", bf16_stored=False):
    """entry by entry (relative to the largest reference entry; a bf16-stored result gets 2^-8 |ref| of its own entry on
    top) and in norm (bf16-stored: + 2^-9).  Returns (entry error, norm error); the entry error of a bf16-stored result
    is what is left after its allowance, never below 0."""
    got, ref64 = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref64).detach().cpu().double()
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(got.float()).all()), f"{what}: not finite"
    tol_e, tol_n = bounds
    scale = float(ref64.abs().max().clamp_min(1e-30))
    err = (got.double() - ref64).abs()
    if bf16_stored:
        err = (err - BF16_ENTRY * ref64.abs()).clamp_min(0.0)
        tol_n = tol_n + BF16_NORM
    flat = int(err.argmax())
    e_entry = float(err.flatten()[flat]) / scale
    e_norm = float((got.double() - ref64).norm() / ref64.norm().clamp_min(1e-30))
    at = where(flat, got.shape)
    assert e_entry < tol_e, (f"{what}: entry-wise error {e_entry:.3g} >= {tol_e:.3g} at entry {at}: "
                             f"{float(got.flatten()[flat]):.7g} vs {float(ref64.flatten()[flat]):.7g}")
    assert e_norm < tol_n, f"{what}: norm error {e_norm:.3g} >= {tol_n:.3g} (worst entry {at})"
    return e_entry, e_norm


# ---------------------------------------------------------------------------------------------- max pool
def pool_check(val, grad, ref_val, ref_grad, what=""):
    """value (B, d) and gradient (B, T, d) equal to torch.max's exactly (a NaN equals a NaN)"""
    val, grad = torch.as_tensor(val).detach().cpu().double(), torch.as_tensor(grad).detach().cpu().double()
    ref_val, ref_grad = ref_val.detach().cpu().double(), ref_grad.detach().cpu().double()
    assert val.shape == ref_val.shape and grad.shape == ref_grad.shape, (what, tuple(val.shape), tuple(grad.shape))
    bad = ~((val == ref_val) | (val.isnan() & ref_val.isnan()))
    if bool(bad.any()):
        b, n = where(int(bad.flatten().int().argmax()), val.shape)
        raise AssertionError(f"{what}: value of clip {b} column {n}: {float(val[b, n])!r} vs {float(ref_val[b, n])!r}")
    bad = ~((grad == ref_grad) | (grad.isnan() & ref_grad.isnan()))
    if bool(bad.any()):
        b, t, n = where(int(bad.flatten().int().argmax()), grad.shape)
        got_t = [int(i) for i in torch.nonzero(grad[b, :, n]).flatten()]
        ref_t = [int(i) for i in torch.nonzero(ref_grad[b, :, n]).flatten()]
        raise AssertionError(f"{what}: gradient of clip {b} column {n} lands on frames {got_t}, torch.max's on {ref_t} "
                             f"(first difference at frame {t}: {float(grad[b, t, n])!r} vs {float(ref_grad[b, t, n])!r})")
