"""torch.autograd bindings of the HWGAT HIP kernels (thin: pointers + sizes).

Every function here calls straight into libhwgat_hip.so through `_lib.call`;
nothing falls back to torch arithmetic.  All activations are in the natural
token order (B, F, K, d).
"""
import ctypes
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib
from ._lib import ptr, stream, dtype_code

# Optional live kernel timing (bench.py): when TIMERS is a dict, every launcher call
# is bracketed by HIP events recorded on the stream the kernel is launched on
# (torch's current stream) and the (start, stop) pairs are appended per entry point.
TIMERS = None
_EVENTS = []            # events created (and recorded once, which is what makes the driver allocate them) ahead of a timed region


def prime_events(n):
    """create `n` timing events now: hipEventCreate happens on an event's first record, ~15 us each -- inside a timed
    region that was 14 % of a 11 ms step (HGATE bf16), although the kernels themselves are untouched by it"""
    fresh = [torch.cuda.Event(enable_timing=True) for _ in range(max(0, n - len(_EVENTS)))]
    for e in fresh:
        e.record()
    torch.cuda.synchronize()
    _EVENTS.extend(fresh)


def call(name, *args):
    if TIMERS is None:
        return _lib.call(name, *args)
    e0 = _EVENTS.pop() if _EVENTS else torch.cuda.Event(enable_timing=True)
    e1 = _EVENTS.pop() if _EVENTS else torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.call(name, *args)
    e1.record()
    TIMERS.setdefault(name, []).append((e0, e1))


def TIMERS_ACTIVE():
    return TIMERS is not None


def timers_summary():
    """{entry point: (launches, total_ms)}; synchronises."""
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in (TIMERS or {}).items()}


# ---------------------------------------------------------------- mask rows
def mask_bits(adj: torch.Tensor) -> torch.Tensor:
    """(nW,32,32) 0/1 adjacency (reference model_params.py:373-392) -> the
    (2,nW,32) uint32 rows `hwgat_win_attn_*` consume: [0] adjacency only,
    [1] adjacency AND the last-slot shift mask (no cross-frame attention,
    reference HWGATE.py:169-187)."""
    a = adj.detach().to("cpu", torch.float32)
    if a.dim() != 3 or a.shape[1:] != (32, 32):
        raise ValueError("adjacency must be (nW, 32, 32) (temporal_patch_size 2 x window 16)")
    if not bool(((a == 0) | (a == 1)).all()):
        raise ValueError("adjacency must be a 0/1 matrix")
    live = a != 0
    same_frame = torch.zeros(32, 32, dtype=torch.bool)
    same_frame[:16, :16] = True
    same_frame[16:, 16:] = True
    weights = (2 ** torch.arange(32, dtype=torch.int64))
    plain = (live.to(torch.int64) * weights).sum(-1)
    last = ((live & same_frame).to(torch.int64) * weights).sum(-1)
    bits = torch.stack([plain, last])                               # (2,nW,32) in [0, 2^32)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.contiguous()


def pwin_mask_bits(adj: torch.Tensor, window_size: int) -> torch.Tensor:
    """(nW, 2W, 2W) 0/1 adjacency of an HWGATE with window size W <= 32 (reference model_params.py:373-392) -> the
    (2, nW, 2W) int64 rows `hwgat_pwin_attn_*` consume: bit j of row [s][w][i] = key slot j visible to query slot i
    (slot = tp * W + joint), [0] adjacency only, [1] adjacency AND the last-slot same-frame mask (HWGATE.py:169-187)."""
    W = int(window_size)
    a = adj.detach().to("cpu", torch.float32)
    if not 1 <= W <= 32:
        raise NotImplementedError(f"window_size {W}: the part-window attention kernels take windows of at most 32 "
                                  f"joints (2 x 32 = 64 tokens, one key per lane)")
    n = 2 * W
    if a.dim() != 3 or a.shape[1:] != (n, n):
        raise ValueError(f"adjacency must be (nW, {n}, {n}) (temporal_patch_size 2 x window {W}), got {tuple(a.shape)}")
    if not bool(((a == 0) | (a == 1)).all()):
        raise ValueError("adjacency must be a 0/1 matrix")
    live = a != 0
    tp = torch.arange(n) // W
    same_frame = tp[:, None] == tp[None, :]
    rows = []
    for m in (live, live & same_frame):
        acc = torch.zeros(a.shape[0], n, dtype=torch.int64)
        for j in range(n):                       # OR of single bits: bit 63 (W = 32) is the sign bit of the int64 word
            acc |= m[..., j].to(torch.int64) << j
        rows.append(acc)
    return torch.stack(rows).contiguous()


def blk_mask_bits(adj: torch.Tensor, n_joints: int) -> torch.Tensor:
    """(2*KJ, 2*KJ) 0/1 block adjacency of HGATE (reference model_params.py:460-476) -> the (2,64,2)
    uint32 rows `hwgat_blk_attn_*` consume.  Query slot i = tp*32 + joint; word [s][i][kt] has bit j
    set iff key joint j of frame kt is visible: [0] adjacency only, [1] adjacency AND same frame (the
    last block of a shifted layer, reference HGATE.py:154-172).  Pad slots (joint >= KJ) stay 0."""
    KJ = int(n_joints)
    a = adj.detach().to("cpu", torch.float32)
    if not 1 <= KJ <= 32 or a.shape != (2 * KJ, 2 * KJ):
        raise ValueError("block adjacency must be (2*K, 2*K) with K <= 32 (temporal_patch_size 2)")
    if not bool(((a == 0) | (a == 1)).all()):
        raise ValueError("adjacency must be a 0/1 matrix")
    live = (a != 0).view(2, KJ, 2, KJ)                       # [tp_q][jq][tp_k][jk]
    weights = (2 ** torch.arange(KJ, dtype=torch.int64))
    plain = torch.zeros(2, 32, 2, dtype=torch.int64)
    plain[:, :KJ] = (live.to(torch.int64) * weights).sum(-1)
    last = plain.clone()
    last[0, :, 1] = 0                                        # no cross-frame pairs
    last[1, :, 0] = 0
    bits = torch.stack([plain.view(64, 2), last.view(64, 2)])
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.contiguous()


def band_mask_rows(adj: torch.Tensor, frames: int) -> torch.Tensor:
    """(nW, T*16, T*16) 0/1 adjacency of WGATE (reference model_params.py:209-228) -> the (nW,16) int64
    rows `hwgat_band_attn_*` consume: bit 16*t + j of row [w][i] = key joint j of frame f-1+t visible to
    query joint i of frame f.  The kernel never forms the (T*16)^2 matrix, so the adjacency must have the
    structure the reference builds: block-tridiagonal over frames with the same three 16x16 blocks on
    every frame, and a visible key in every row of the diagonal block.  Anything else raises."""
    a = adj.detach().to("cpu")
    T = int(frames)
    if a.dim() != 3 or a.shape[1] != T * 16 or a.shape[2] != T * 16:
        raise ValueError("WGATE adjacency must be (nW, T*16, T*16)")
    nW = a.shape[0]
    if not bool(((a == 0) | (a == 1)).all()):
        raise ValueError("adjacency must be a 0/1 matrix")
    blk = (a != 0).view(nW, T, 16, T, 16).permute(0, 1, 3, 2, 4)          # [w][fq][fk][i][j]
    fq = torch.arange(T).view(T, 1)
    fk = torch.arange(T).view(1, T)
    off = (fk - fq)
    if bool(blk[:, off.abs() > 1].any()):
        raise NotImplementedError("WGATE HIP backend needs a block-tridiagonal adjacency (frames f-1, f, f+1)")
    rows = torch.zeros(nW, 16, dtype=torch.int64)
    weights = 2 ** torch.arange(16, dtype=torch.int64)
    for t, o in enumerate((-1, 0, 1)):
        sel = blk[:, off == o]                                            # (nW, n, 16, 16)
        if sel.shape[1] == 0:
            continue
        if not bool((sel == sel[:, :1]).all()):
            raise NotImplementedError("WGATE HIP backend needs the same adjacency blocks on every frame")
        rows += (sel[:, 0].to(torch.int64) * weights).sum(-1) << (16 * t)
    if not bool(((rows >> 16) & 0xFFFF).ne(0).all()):
        raise NotImplementedError("every query joint needs a visible key in its own frame")
    return rows.contiguous()


def wband_mask_rows(adj: torch.Tensor, frames: int, window_size: int) -> torch.Tensor:
    """0/1 adjacency of a band model with W = `window_size` <= 32 joints per window and frame -- WGATE's
    (nW, T*W, T*W) (reference model_params.py:209-228) or GATE's (T*K, T*K) with W = K (model_params.py:60-73) -> the
    (nW, 32, 3) int32 words `hwgat_wband_attn_*` consume: bit j of word [w][i][t] = key joint j of frame f-1+t visible
    to query joint i of frame f; rows i >= W stay 0.  The kernel never forms the (T*W)^2 matrix, so the adjacency must be
    block-tridiagonal over frames with the same three W x W blocks on every frame, and every query joint needs a visible
    key in its own frame (its softmax row must not be empty at the clip ends).  The diagonal itself need not be set
    (GATE has no self loops).  Anything else raises with the rule it breaks."""
    W, T = int(window_size), int(frames)
    if not 1 <= W <= 32:
        raise NotImplementedError(f"window_size {W}: the wide band attention kernels take windows of at most 32 joints "
                                  f"(one 32-bit mask word per key frame)")
    a = adj.detach().to("cpu")
    if a.dim() == 2:
        a = a.unsqueeze(0)
    if a.dim() != 3 or a.shape[1] != T * W or a.shape[2] != T * W:
        raise ValueError(f"band adjacency must be (nW, T*W, T*W) or (T*W, T*W) with T*W = {T * W}, got {tuple(adj.shape)}")
    nW = a.shape[0]
    if not bool(((a == 0) | (a == 1)).all()):
        raise ValueError("adjacency must be a 0/1 matrix")
    blk = (a != 0).view(nW, T, W, T, W).permute(0, 1, 3, 2, 4)             # [w][fq][fk][i][j]
    off = torch.arange(T).view(1, T) - torch.arange(T).view(T, 1)          # fk - fq
    if bool(blk[:, off.abs() > 1].any()):
        raise NotImplementedError("the band attention kernels need a block-tridiagonal adjacency (frames f-1, f, f+1)")
    rows = torch.zeros(nW, 32, 3, dtype=torch.int64)
    weights = 2 ** torch.arange(W, dtype=torch.int64)
    for t, o in enumerate((-1, 0, 1)):
        sel = blk[:, off == o]                                             # (nW, n, W, W)
        if sel.shape[1] == 0:
            continue
        if not bool((sel == sel[:, :1]).all()):
            raise NotImplementedError("the band attention kernels need the same adjacency blocks on every frame")
        rows[:, :W, t] = (sel[:, 0].to(torch.int64) * weights).sum(-1)
    if not bool(rows[:, :W, 1].ne(0).all()):
        raise NotImplementedError("every query joint needs a visible key in its own frame")
    return torch.where(rows >= 2 ** 31, rows - 2 ** 32, rows).to(torch.int32).contiguous()


# ---------------------------------------------------------------- embedding
def embed(x, idx, bmat, pe, K, out_dtype=torch.float32, drop_p=0.0, seed=0, seed_base=None):
    """gather + Fourier features + PE (+ dropout) (no gradient: B is frozen, PE a buffer).
    `seed_base` (here and in every function below that takes a dropout seed): None, or a 1-element device tensor whose
    32-bit word the kernel adds to the site seed when it RUNS (include/hwgat_hip.h, "dropout seeds")."""
    B, T, J, C = x.shape
    d0 = bmat.shape[0] * 2
    out = torch.empty(B, T, K, d0, device=x.device, dtype=out_dtype)
    call("hwgat_embed_fwd", ptr(x), ptr(idx), ptr(bmat), ptr(pe), ptr(out),
         B, T, J, K, C, d0, dtype_code(out), seed & 0xFFFFFFFF, float(drop_p), ptr(seed_base), stream())
    return out


# ---------------------------------------------------------------- LayerNorm
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, deterministic=False):
        d = x.shape[-1]
        n = x.numel() // d
        y = torch.empty_like(x)
        mean = torch.empty(n, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        call("hwgat_ln_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd),
             n, d, dtype_code(x), stream())
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.deterministic = bool(deterministic)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        d = x.shape[-1]
        dy = dy.contiguous()
        dg = torch.zeros(2, d, device=x.device, dtype=torch.float32)
        # deterministic: dgamma / dbeta through per-block images added in a fixed order (hwgat_ln_bwd_det)
        dx = ln_backward(dy, x, mean, rstd, gamma, None, dg[0], dg[1], deterministic=ctx.deterministic).dx
        return dx, dg[0], dg[1], None


def layer_norm(x, gamma, beta, deterministic=False):
    """LayerNorm over the last dim; `deterministic`: a bit-reproducible backward (no float atomics)"""
    return _LayerNorm.apply(x.contiguous(), gamma, beta, bool(deterministic))


# ---------------------------------------------------------------- attention
def _tile16_dims(shape, bits, n_heads):
    B, F, K, d = shape
    return B, F, K // 16, n_heads, d // n_heads


def _blk_dims(shape, bits, n_heads):
    B, F, K, d = shape
    return B, F, K, n_heads, d // n_heads


def _pwin_dims(shape, bits, n_heads):
    """(B, F, K, W, n_heads, head_dim) of a 'pwin' launch; W comes from the (2, nW, 2W) mask rows"""
    B, F, K, d = shape
    if bits.dtype != torch.int64 or bits.dim() != 3 or bits.shape[0] != 2 or bits.shape[2] % 2:
        raise ValueError("'pwin' attention needs the (2, nW, 2W) int64 rows of functional.pwin_mask_bits")
    W = bits.shape[2] // 2
    if bits.shape[1] * W != K:
        raise ValueError(f"mask rows are for {bits.shape[1]} windows of {W} joints, activations have {K} joints")
    hd = d // n_heads
    if hd not in (32, 64):
        raise NotImplementedError(f"head_dim {hd}: the part-window attention kernels for window sizes other than 16 "
                                  f"take head_dim 32 or 64")
    return B, F, K, W, n_heads, hd


def _wband_dims(shape, rows, n_heads):
    """(B, F, nW, W, n_heads, head_dim) of a 'wband' launch; nW comes from the (nW, 32, 3) mask words"""
    B, F, K, d = shape
    if rows.dtype != torch.int32 or rows.dim() != 3 or tuple(rows.shape[1:]) != (32, 3):
        raise ValueError("'wband' attention needs the (nW, 32, 3) int32 words of functional.wband_mask_rows")
    nW = rows.shape[0]
    if K % nW or K // nW > 32:
        raise ValueError(f"mask words are for {nW} windows, activations have {K} joints per frame")
    hd = d // n_heads
    if d % n_heads or hd not in (16, 32):
        raise NotImplementedError(f"head_dim {d / n_heads:g}: the wide band attention kernels take head_dim 16 or 32")
    return B, F, nW, K // nW, n_heads, hd


class AttnKind(NamedTuple):
    """one attention kind: entry points `<stem>_fwd[_drop]` / `<stem>_bwd[_drop]` (include/hwgat_hip.h) taking
    qkv, o | (do, dqkv), mask[, thr], *dims(o_shape, mask, n_heads)[, shifted], dtype[, seed, p, seed_base], stream"""
    stem: str
    takes_thr: bool             # the train-mode threshold drop of the part-window models (HWGATE.py:94-100)
    takes_shifted: bool         # the last-slot mask of a shifted layer
    dims: Callable              # (o_shape, mask, n_heads) -> the integer arguments, after checking mask and head_dim
    refusal: str                # what the assertion says when a threshold / shift is given to a kind without one


ATTN_KINDS = {
    # HWGATE part windows, W = 16
    "win": AttnKind("hwgat_win_attn", True, True, _tile16_dims, ""),
    # HWGATE part windows of any other size W <= 32 (W from the mask rows, functional.pwin_mask_bits)
    "pwin": AttnKind("hwgat_pwin_attn", True, True, _pwin_dims, ""),
    # HGATE blocks
    "blk": AttnKind("hwgat_blk_attn", False, True, _blk_dims, "HGATE has no train-mode threshold"),
    # WGATE, W = 16
    "band": AttnKind("hwgat_band_attn", False, False, _tile16_dims, "WGATE has neither threshold nor shift"),
    # GATE, and WGATE with any other W <= 32 (functional.wband_mask_rows)
    "wband": AttnKind("hwgat_wband_attn", False, False, _wband_dims, "the band models have neither threshold nor shift"),
}


def _attn_kind(kind):
    if kind not in ATTN_KINDS:
        raise ValueError(kind)
    return ATTN_KINDS[kind]


def _attn_drop(kind, thr, drop):
    """(seed, p, seed_base) of the attention dropout (reference HWGATE.py:78,112, HGATE.py:78,106, WGATE.py:81,103) or None"""
    if drop is None or float(drop[1]) <= 0.0:
        return None
    if _attn_kind(kind).takes_thr and thr is None:
        raise ValueError("attention dropout is a train-mode operation: it needs the train-mode threshold tensor")
    return int(drop[0]) & 0xFFFFFFFF, float(drop[1]), (drop[2] if len(drop) > 2 else None)


def _attn_launch(direction, kind, qkv, tensors, bits, thr, n_heads, shifted, drop):
    """launch `<stem>_<direction>` of `kind`, or its `_drop` entry when the dropout rate is above 0;
    `tensors` = (o,) for 'fwd', (do, dqkv) for 'bwd'"""
    rec = _attn_kind(kind)
    drop = _attn_drop(kind, thr, drop)
    assert (rec.takes_thr or thr is None) and (rec.takes_shifted or not shifted), rec.refusal
    args = [ptr(qkv), *(ptr(t) for t in tensors), ptr(bits)]
    if rec.takes_thr:
        args.append(ptr(thr))
    args += rec.dims(tensors[0].shape, bits, n_heads)
    if rec.takes_shifted:
        args.append(int(shifted))
    args.append(dtype_code(qkv))
    if drop is None:
        call(f"{rec.stem}_{direction}", *args, stream())
    else:
        call(f"{rec.stem}_{direction}_drop", *args, drop[0], drop[1], ptr(drop[2]), stream())


def attn_fwd(kind, qkv, o, bits, thr, n_heads, shifted, drop=None):
    """launch the attention forward of a model family: 'win' = HWGATE part windows (W = 16), 'pwin' = HWGATE part
    windows of any other size W <= 32 (W from `bits`, functional.pwin_mask_bits), 'blk' = HGATE blocks, 'band' = WGATE
    (W = 16), 'wband' = GATE and WGATE with any other W <= 32 (functional.wband_mask_rows).
    `drop` = (seed, p) or (seed, p, seed_base): attention dropout ('win' / 'pwin': train mode only)"""
    _attn_launch("fwd", kind, qkv, (o,), bits, thr, n_heads, shifted, drop)


def attn_bwd(kind, qkv, do, dqkv, bits, thr, n_heads, shifted, drop=None):
    """the backward of attn_fwd: dqkv from qkv and do, masks regenerated from the same `drop`"""
    _attn_launch("bwd", kind, qkv, (do, dqkv), bits, thr, n_heads, shifted, drop)


ATTN_PROBS_CODE = {"win": 0, "pwin": 1, "blk": 2, "band": 3, "wband": 4}      # HWGAT_ATTN_* of include/hwgat_hip.h


def _attn_probs_geom(kind, qkv, mask, n_heads):
    """(B, F, K, W, nW, n_heads, head_dim) of an attn_probs call, through the kind's own `dims` helper (same refusals)"""
    if qkv.dim() < 4:
        raise ValueError("qkv must be (B, F, K, 3 d) or (B, F, K, 3, nH, hd)")
    B, F, K = qkv.shape[:3]
    d3 = qkv.numel() // max(1, B * F * K)
    dims = _attn_kind(kind).dims((B, F, K, d3 // 3), mask, n_heads)
    if kind in ("win", "band"):
        _, _, nW, nH, hd = dims
        W = 16
    elif kind == "pwin":
        _, _, _, W, nH, hd = dims
        nW = K // W
    elif kind == "blk":
        _, _, _, nH, hd = dims
        W, nW = K, 1
    else:
        _, _, nW, W, nH, hd = dims
    return B, F, K, W, nW, nH, hd


def attn_probs_shape(kind, B, F, K, W, n_heads):
    """shape of the exported probability tensor: pair kinds (B, F/2, nW, nH, 2W, 2W), band kinds (B, nW, nH, F, W, 3, W)"""
    nW = K // W
    if kind in ("win", "pwin", "blk"):
        return (B, F // 2, nW, n_heads, 2 * W, 2 * W)
    return (B, nW, n_heads, F, W, 3, W)


def attn_probs(kind, qkv, mask, n_heads, shifted=False, probs=True, received=True, out=None):
    """the eval-mode attention probabilities of `kind` (a key of ATTN_KINDS) for the qkv tensor (B, F, K, 3 d) its fused
    forward reads and the model's mask rows, written out by hwgat_attn_probs (csrc/attn_probs.hip) -> (probs | None,
    received | None), both fp32.  probs: the reference's attention tensor -- pair kinds ('win', 'pwin', 'blk')
    (B, F/2, nW, nH, n, n) with n = 2 W (in a shifted block window fi holds frames (2 fi + 1) % F, (2 fi + 2) % F:
    explain.window_frames), band kinds ('band', 'wband') (B, nW, nH, F, W, 3, W) with [.., f, i, t, j] = query joint i of
    frame f -> key joint j of frame f - 1 + t (explain.band_to_dense).  received (B, F, K): the head-mean column sums,
    how much attention each joint of each frame of the block's input received; computed without materialising P.
    `out` = (probs buffer | None, received buffer | None): write into these instead of allocating."""
    if not (probs or received):
        raise ValueError("attn_probs: ask for probs, received or both")
    rec = _attn_kind(kind)
    assert rec.takes_shifted or not shifted, rec.refusal
    qkv = qkv.contiguous()
    B, F, K, W, nW, nH, hd = _attn_probs_geom(kind, qkv, mask, n_heads)
    code = ATTN_PROBS_CODE[kind]
    p_buf, r_buf = out if out is not None else (None, None)
    p = r = None
    if probs:
        shape = attn_probs_shape(kind, B, F, K, W, nH)
        p = p_buf if p_buf is not None else torch.empty(shape, device=qkv.device, dtype=torch.float32)
        if tuple(p.shape) != shape or p.dtype != torch.float32:
            raise ValueError(f"probs buffer must be fp32 {shape}, got {p.dtype} {tuple(p.shape)}")
    if received:
        r = r_buf if r_buf is not None else torch.empty(B, F, K, device=qkv.device, dtype=torch.float32)
        if tuple(r.shape) != (B, F, K) or r.dtype != torch.float32:
            raise ValueError(f"received buffer must be fp32 {(B, F, K)}, got {r.dtype} {tuple(r.shape)}")
    call("hwgat_attn_probs", code, ptr(qkv), ptr(mask), ptr(p), ptr(r), B, F, K, W, nH, hd, int(bool(shifted)),
         dtype_code(qkv), stream())
    return p, r


class _Attn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, bits, thr, n_heads, shifted, drop, kind):
        B, F, K, d3 = qkv.shape
        o = torch.empty(B, F, K, d3 // 3, device=qkv.device, dtype=qkv.dtype)
        attn_fwd(kind, qkv, o, bits, thr, n_heads, shifted, drop)
        ctx.save_for_backward(qkv, bits, thr)
        ctx.cfg = (n_heads, int(shifted), drop, kind)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, bits, thr = ctx.saved_tensors
        n_heads, shifted, drop, kind = ctx.cfg
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        attn_bwd(kind, qkv, do, dqkv, bits, thr, n_heads, shifted, drop)
        return dqkv, None, None, None, None, None, None


def band_attention(qkv, rows, n_heads, drop=None):
    """WGATE: qkv (B,F,K,3d) -> o (B,F,K,d); a window = one 16-joint part window over all F frames.
    `drop` = (seed, p[, seed_base]): attention dropout (reference WGATE.py:103)."""
    return _Attn.apply(qkv.contiguous(), rows, None, n_heads, False, _attn_drop("band", None, drop), "band")


def wband_attention(qkv, rows, n_heads, drop=None):
    """GATE / WGATE with a window size other than 16: qkv (B,F,K,3d) -> o (B,F,K,d); a window = W <= 32 joints over all
    F frames, K = nW * W; `rows` = functional.wband_mask_rows(adj, F, W) on the device.
    `drop` = (seed, p[, seed_base]): attention dropout (reference GATE.py:65, WGATE.py:103)."""
    return _Attn.apply(qkv.contiguous(), rows, None, n_heads, False, _attn_drop("wband", None, drop), "wband")


def block_attention(qkv, bits, n_heads, shifted, drop=None):
    """HGATE: qkv (B,F,K,3d) -> o (B,F,K,d); a block = 2 frames x all K joints.
    `drop` = (seed, p[, seed_base]): attention dropout (reference HGATE.py:106)."""
    return _Attn.apply(qkv.contiguous(), bits, None, n_heads, shifted, _attn_drop("blk", None, drop), "blk")


def window_attention(qkv, bits, thr, n_heads, shifted, drop=None):
    """qkv (B,F,K,3d) -> o (B,F,K,d).  `thr`: 1-element fp32 device tensor
    (train mode) or None (eval mode).  `drop` = (seed, p): attention dropout on the
    probabilities (reference HWGATE.py:112), train mode only."""
    return _Attn.apply(qkv.contiguous(), bits, thr, n_heads, shifted, _attn_drop("win", thr, drop), "win")


def part_window_attention(qkv, bits, thr, n_heads, shifted, drop=None):
    """HWGATE with a window size W != 16: qkv (B,F,K,3d) -> o (B,F,K,d); `bits` = functional.pwin_mask_bits(adj, W)
    (on the device), the rest as window_attention."""
    return _Attn.apply(qkv.contiguous(), bits, thr, n_heads, shifted, _attn_drop("pwin", thr, drop), "pwin")


# ---------------------------------------------------------------- merge
class _Merge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, F, K, d = x.shape
        out = torch.empty(B, F // 2, K, 2 * d, device=x.device, dtype=x.dtype)
        call("hwgat_merge", ptr(x), ptr(out), B, F, K, d, 0, dtype_code(x), stream())
        return out

    @staticmethod
    def backward(ctx, dout):
        B, f, K, d2 = dout.shape
        dout = dout.contiguous()
        dx = torch.empty(B, f * 2, K, d2 // 2, device=dout.device, dtype=dout.dtype)
        call("hwgat_merge", ptr(dout), ptr(dx), B, f * 2, K, d2 // 2, 1, dtype_code(dout), stream())
        return dx


def temporal_merge(x):
    return _Merge.apply(x.contiguous())


# ---------------------------------------------------------------- LN + pool
def _pool_tokens(x):
    B, d = x.shape[0], x.shape[-1]
    return B, x.numel() // (B * d), d


def _pool_carry(x, carrier, up, book):
    """(x contiguous, carrier, up) of a pool call.  carrier / up / book (block.fused_block) count only together: a carrier
    that is not shaped like a contiguous x or comes without a book is dropped, and `up` = (seed, p) stays -- the backward
    then makes the masked copy -- only with a carrier and p > 0"""
    xcont = x.contiguous()
    if carrier is not None and (xcont is not x or carrier.shape != x.shape or book is None):
        carrier = None
    if carrier is None or up is None or up[1] <= 0.0:
        up = None
    return xcont, carrier, up


def _pool_forward(x, wt, deterministic):
    """hwgat_ln[w]pool_fwd[_det] -> (mean, rstd, hat): the row statistics and the (B, d) fp32 sum over a clip's tokens
    of xhat, times the token weights `wt` where given"""
    B, n_tok, d = _pool_tokens(x)
    mean = torch.empty(B * n_tok, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    name = "hwgat_lnpool_fwd" if wt is None else "hwgat_lnwpool_fwd"
    wts = () if wt is None else (ptr(wt),)
    if deterministic:      # per-block partial sums added in index order: the same bits on every run
        rows = _lib.lib().hwgat_lnpool_partial_rows(B, n_tok)
        hat = torch.empty(B, d, device=x.device, dtype=torch.float32)
        part = torch.empty(B * rows, d, device=x.device, dtype=torch.float32)
        call(name + "_det", ptr(x), *wts, ptr(hat), ptr(mean), ptr(rstd), B, n_tok, d, dtype_code(x), ptr(part), stream())
    else:
        hat = torch.zeros(B, d, device=x.device, dtype=torch.float32)
        call(name, ptr(x), *wts, ptr(hat), ptr(mean), ptr(rstd), B, n_tok, d, dtype_code(x), stream())
    return mean, rstd, hat


def _pool_backward(ctx, g, x, mean, rstd, wt=None):
    """hwgat_ln[w]pool_bwd_masked for the per-clip upstream gradient g (B, d) -> (dx, dx_masked or None, gdot or None);
    the masked copy is made with ctx.up and registered with the book; gdot (B, n_tok): the weighted pool's
    sum_c g[b][c] xhat[b][t][c]"""
    B, n_tok, d = _pool_tokens(x)
    dx = torch.empty_like(x)
    dxm = torch.empty_like(x) if ctx.up is not None else None
    seed, p = ctx.up if ctx.up else (0, 0.0)
    gdot = None if wt is None else torch.empty(B, n_tok, device=x.device, dtype=torch.float32)
    front = (ptr(g), ptr(x)) if wt is None else (ptr(g), ptr(wt), ptr(x))
    call("hwgat_lnpool_bwd_masked" if wt is None else "hwgat_lnwpool_bwd_masked", *front, ptr(mean), ptr(rstd), ptr(dx),
         *(() if wt is None else (ptr(gdot),)), B, n_tok, d, dtype_code(x), ptr(dxm), seed & 0xFFFFFFFF, float(p),
         ptr(ctx.seed_base), stream())
    if dxm is not None:
        ctx.book.register(dx, dxm)
    return dx, dxm, gdot


class _LnPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, xc=None, up=None, book=None, deterministic=False, seed_base=None):
        # xc / up / book: carrier of the masked gradient for the block that produced x, as _pool_carry resolved them
        ctx.up, ctx.book, ctx.seed_base = up, book, seed_base
        mean, rstd, hat = _pool_forward(x, None, deterministic)
        hat_mean = hat / _pool_tokens(x)[1]
        ctx.save_for_backward(x, gamma, mean, rstd, hat_mean)
        return hat_mean * gamma + beta

    @staticmethod
    def backward(ctx, dfeat):
        x, gamma, mean, rstd, hat_mean = ctx.saved_tensors
        dfeat = dfeat.float()
        g = (dfeat * gamma / _pool_tokens(x)[1]).contiguous()
        dx, dxm, _ = _pool_backward(ctx, g, x, mean, rstd)
        return dx, (dfeat * hat_mean).sum(0), dfeat.sum(0), dxm, None, None, None, None


def ln_mean_pool(x, gamma, beta, carrier=None, up=None, book=None, deterministic=False, seed_base=None):
    """final LayerNorm + mean over all tokens -> (B, d) fp32.  carrier / up / book: see block.fused_block (the last
    block's fc2-dropout mask is applied to its incoming gradient here, once).  `deterministic`: fixed summation order
    (two launches, no atomics), what eval() uses so that two forwards are bit-identical like the reference's."""
    xcont, carrier, up = _pool_carry(x, carrier, up, book)
    return _LnPool.apply(xcont, gamma, beta, carrier, up, book, bool(deterministic), seed_base)


class _LnWeightedPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, w, bias, xc=None, up=None, book=None, deterministic=False, seed_base=None):
        ctx.up, ctx.book, ctx.seed_base = up, book, seed_base
        n_tok = _pool_tokens(x)[1]
        wt = w.detach().reshape(-1).float().contiguous()
        if wt.numel() != n_tok:
            raise ValueError(f"the pool has {wt.numel()} token weights, the activations have {n_tok} tokens per clip")
        mean, rstd, hat = _pool_forward(x, wt, deterministic)
        ctx.save_for_backward(x, gamma, beta, wt, mean, rstd, hat)
        ctx.w_shape = w.shape
        return hat * gamma + (beta * wt.sum() + bias.reshape(()))

    @staticmethod
    def backward(ctx, dfeat):
        x, gamma, beta, wt, mean, rstd, hat = ctx.saved_tensors
        dfeat = dfeat.float()
        dx, dxm, gdot = _pool_backward(ctx, (dfeat * gamma).contiguous(), x, mean, rstd, wt)
        dsum = dfeat.sum(0)                                                 # (d)
        # d w[t] = sum_b sum_c dfeat[b,c] (gamma_c xhat[b,t,c] + beta_c): the kernel did the channel sums per (b, t)
        dw = (gdot.sum(0) + (dsum * beta).sum()).reshape(ctx.w_shape)
        return dx, (dfeat * hat).sum(0), dsum * wt.sum(), dw, dsum.sum().reshape(1), dxm, None, None, None, None


def ln_weighted_pool(x, gamma, beta, w, bias, carrier=None, up=None, book=None, deterministic=False, seed_base=None):
    """final LayerNorm + weighted pool over all tokens (reference GATE.py:208-210, `weightedAvg = nn.Linear(T K, 1)` applied
    along the token axis): feat[b, c] = sum_tok w[tok] LN(x)[b, tok, c] + bias -> (B, d) fp32.  w (n_tok) or (1, n_tok),
    bias (1).  Gradients to x, gamma, beta, w and bias.  carrier / up / book / deterministic / seed_base: as ln_mean_pool.
    Widths 128, 256, 512 and 1024."""
    xcont, carrier, up = _pool_carry(x, carrier, up, book)
    if xcont.shape[-1] not in (128, 256, 512, 1024):
        raise NotImplementedError(f"width {xcont.shape[-1]}: the weighted token pool takes d in 128, 256, 512, 1024")
    return _LnWeightedPool.apply(xcont, gamma, beta, w, bias, carrier, up, book, bool(deterministic), seed_base)


# ---------------------------------------------------------------- fp32 MFMA linears
PRO_NONE, PRO_LN, PRO_DROP, PRO_LN_FOLD = 0, 1, 2, 3
# Formulation switches.  Plain module constants: the product reads no environment variables; the parity tests flip them
# (monkeypatch) to compare the formulations against each other.
# LayerNorm -> Linear pairs (norm1 -> qkv, norm2 -> fc1) run with the normalisation folded into the weights and the
# GEMM epilogue (hwgat_ln_fold + pro 3) when the token count is whole tiles; False keeps the normalising loader (pro 1).
LN_FOLD = True
# Dropout masks in the backward pass: 0 = hashed in every GEMM loader that needs the masked gradient; 1 = the
# LayerNorm backward that produces a gradient also writes its masked copy once (hwgat_ln_bwd_masked) for the block's own
# projection dropout; 2 = also across blocks, for the fc2 dropout of the block that produced this block's input.
MASK_ONCE = 2
# ... for blocks at least this wide: at d = 128 the extra E-sized write costs what the mask loaders cost there
# (measured: WGATE, 8 blocks of d = 128, 1 468 -> 1 441 clips/s with masked copies everywhere)
MASK_ONCE_MIN_D = 256


class CarryBook:
    """Validity records of the dropout-masked gradient copies of ONE forward call.

    A masked copy handed to the producing block through a carrier is only valid if the gradient that block receives IS
    the dx it was made from.  If the tensor has another consumer (an auxiliary loss on a block output, say) autograd adds
    that gradient to dx -- in a new tensor, or in place -- and the copy would miss it.  The consumer therefore registers
    (address, version counter, shape) of its dx under the address of the masked copy; the producer uses the copy only if
    the gradient it got still has exactly that address and version, and otherwise masks the real gradient in its
    loaders.  One book per forward call (held by the HandOver, referenced by the autograd nodes of that call): nothing is
    shared between models or between two forwards of one model."""

    def __init__(self):
        self._rec = {}

    def register(self, dx, dxm):
        if dxm is not None:
            self._rec[dxm.data_ptr()] = (dx.data_ptr(), dx._version, tuple(dx.shape))

    def valid(self, dout, doutm):
        """True iff `doutm` is the registered masked copy of exactly this `dout`"""
        if doutm is None:
            return False
        rec = self._rec.pop(doutm.data_ptr(), None)
        return rec is not None and rec == (dout.data_ptr(), dout._version, tuple(dout.shape))


class WeightPrep:
    """Every derived copy of the block weights a forward (+ backward) call consumes, made by ONE launch
    (hwgat_weight_prep): per block the LayerNorm-folded qkv / fc1 weights with their row sums (hwgat_ln_fold), the
    activation-dtype copies of proj / fc2 (bf16 activations only) and, when a backward will follow, the four transposed
    copies for the dX launches.  The output buffers and the device table are built once per (model, dtype, train) and
    reused: the copies are rewritten by every forward call from the current master weights, and a backward reads the
    copies of its own forward (the weights do not change in between).  `per_block[k]` maps names to tensors."""

    OP_COPY, OP_T, OP_FOLD = 0, 1, 2

    def __init__(self, blocks, dtype, with_transposes):
        import numpy as np
        self.dtype = dtype
        dev = blocks[0].attn.qkv.weight.device
        ent, self.per_block, self._keep = [], [], []
        first = 0

        def add(op, W, out, bias=None, gamma=None, beta=None, s=None, c=None):
            nonlocal first
            N, K = W.shape
            ent.append((W.data_ptr(), 0 if bias is None else bias.data_ptr(), 0 if gamma is None else gamma.data_ptr(),
                        0 if beta is None else beta.data_ptr(), out.data_ptr(), 0 if s is None else s.data_ptr(),
                        0 if c is None else c.data_ptr(), N, K, op, first))
            first += -(-N // 4) if op == self.OP_FOLD else (-(-N // 32)) * (-(-K // 32))

        def fold(lin, norm):
            N, K = lin.weight.shape
            Wf = torch.empty(N, K, device=dev, dtype=dtype)
            sc = torch.empty(2, N, device=dev, dtype=torch.float32)
            add(self.OP_FOLD, lin.weight, Wf, lin.bias, norm.weight, norm.bias, sc[0], sc[1])
            return Wf, sc[0], sc[1]

        def copy(W, transposed):
            N, K = W.shape
            out = torch.empty((K, N) if transposed else (N, K), device=dev, dtype=dtype)
            add(self.OP_T if transposed else self.OP_COPY, W, out)
            return out

        srcs = []
        for blk in blocks:
            lins = (blk.attn.qkv, blk.attn.proj, blk.ff.fc1, blk.ff.fc2)
            srcs += [t for lin in lins for t in (lin.weight, lin.bias)] + [blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias]
            d = {"qkv_f": fold(blk.attn.qkv, blk.norm1), "w1_f": fold(blk.ff.fc1, blk.norm2)}
            if dtype != torch.float32:
                d["wp_c"], d["w2_c"] = copy(blk.attn.proj.weight, False), copy(blk.ff.fc2.weight, False)
            if with_transposes:
                d["wqkvT"], d["wpT"] = copy(blk.attn.qkv.weight, True), copy(blk.attn.proj.weight, True)
                d["w1T"], d["w2T"] = copy(blk.ff.fc1.weight, True), copy(blk.ff.fc2.weight, True)
            self.per_block.append(d)
        self.key = self.signature(blocks, dtype, with_transposes)
        rec = np.dtype([("p", np.uint64, 7), ("i", np.int32, 4)])           # hwgat_prep_entry: 7 pointers, N, K, op, first_block
        assert rec.itemsize == 72
        host = np.zeros(len(ent), dtype=rec)
        for i, e in enumerate(ent):
            host[i]["p"] = e[:7]
            host[i]["i"] = e[7:]
        self.table = torch.from_numpy(host.view(np.uint8).copy()).to(dev)
        self.n, self.total = len(ent), first

    @staticmethod
    def signature(blocks, dtype, with_transposes):
        """what the cached buffers and table were built for: the addresses of every source parameter"""
        ptrs = []
        for blk in blocks:
            for t in (blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj.weight, blk.ff.fc1.weight, blk.ff.fc1.bias,
                      blk.ff.fc2.weight, blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias):
                ptrs.append(t.data_ptr())
        return (dtype, bool(with_transposes), tuple(ptrs))

    def run(self):
        call("hwgat_weight_prep", ptr(self.table), self.n, self.total, 0 if self.dtype == torch.float32 else 1, stream())
        return self


def weight_prep(owner, blocks, dtype, with_transposes):
    """the (cached) WeightPrep of `owner` (a model) for this dtype / mode, run for the current weights; None where the
    masters are not plain fp32 parameters (the per-call kernels then do the work, as before)"""
    ws = [blk.attn.qkv.weight for blk in blocks]
    if not ws or any(w.dtype != torch.float32 or not w.is_cuda for w in ws):
        return None
    key = WeightPrep.signature(blocks, dtype, with_transposes)
    cache = owner.__dict__.setdefault("_weight_prep_cache", {})
    wp = cache.get(key[:2])
    if wp is None or wp.key != key:
        wp = cache[key[:2]] = WeightPrep(blocks, dtype, with_transposes)
    return wp.run()


class HandOver:
    """What one block's epilogues produced for the next block of the same forward call: `of` = the tensor the values
    belong to, `stats` = (mean, rstd) of its rows (from the fc2 epilogue), `carrier` / `up` = the data-less carrier of
    the masked gradient and the (seed, p) of the dropout it masks, `plan[k]` = (produce output statistics, store merged)
    for block k, `book` = the CarryBook of the call.  A local of FamilyModel._run_blocks (models/_family.py); never stored on
    the module."""

    def __init__(self, last_block=-1, deterministic=False):
        self.of = self.stats = self.carrier = self.up = None
        self.plan = {}
        self.last_block = last_block
        self.deterministic = bool(deterministic)
        self.book = CarryBook()
        self.prep = None            # WeightPrep of this call (per_block[k] = the derived weight copies of block k)
        self.seed_base = None       # 1-element device tensor: the base seed of this call's dropout masks (or None)


EPI_BIAS, EPI_BIAS_DROP_RES, EPI_BIAS_GELU_DROP, EPI_GELU_BWD, EPI_NONE, EPI_BIAS_GELU_DROP_G, EPI_MUL_AUX = 0, 1, 2, 3, 4, 5, 6


def can_fuse_row_stats(x):
    """the producing linear's epilogue can deliver the LayerNorm statistics of `x`-shaped output (whole tiles)"""
    return (x.numel() // x.shape[-1]) % 256 == 0


def linear_nt(A, W, bias=None, *, pro=PRO_NONE, ln=None, pro_seed=0, pro_p=0.0, epi=EPI_BIAS,
              res=None, aux=None, epi_seed=0, epi_p=0.0, out=None, stats=False, merge=None, seed_base=None):
    """C[M,N] = pro(A)[M,K] . W[N,K]^T with fused epilogue (see include/hwgat_hip.h).
    Returns C, or (C, C2) for EPI_BIAS_GELU_DROP (C2 = pre-activation) / EPI_BIAS_GELU_DROP_G (C2 = gelu' * mask).
    EPI_BIAS_DROP_RES: `stats=True` also returns (mean, rstd) of the OUTPUT rows, produced by the epilogue
    (no separate pass over C); `merge=(F, K_tok)` stores C in the TemporalMerging layout (B, F/2, K_tok, 2N)
    (HWGATE.py:55-63), statistics then per merged row.  Returns (C, mean, rstd)."""
    K = A.shape[-1]
    M = A.numel() // K
    N = W.shape[0]
    if W.dtype != A.dtype:
        raise TypeError("weight must already be in the activation dtype (cast once per step)")
    if stats or merge is not None:
        if epi != EPI_BIAS_DROP_RES or pro != PRO_NONE or M % 256 or out is not None:
            raise ValueError("row statistics / merged store: EPI_BIAS_DROP_RES, no prologue, M % 256 == 0")
        if merge is not None:
            F, Kt = merge
            C = torch.empty(M // (F * Kt), F // 2, Kt, 2 * N, device=A.device, dtype=A.dtype)
            rows, width = M // 2, 2 * N
        else:
            C = torch.empty(*A.shape[:-1], N, device=A.device, dtype=A.dtype)
            rows, width = M, N
        st = torch.zeros(2, rows, device=A.device, dtype=torch.float32)
        call("hwgat_linear_nt_f32_ex" if A.dtype == torch.float32 else "hwgat_linear_nt_bf16_ex",
             ptr(A), ptr(W), ptr(bias), ptr(C), M, N, K, pro, None, None, None, None,
             pro_seed & 0xFFFFFFFF, float(pro_p), epi, ptr(res), None, None, epi_seed & 0xFFFFFFFF, float(epi_p),
             ptr(st[0]), ptr(st[1]), merge[0] if merge else 0, merge[1] if merge else 0, ptr(seed_base), stream())
        call("hwgat_ln_finalize", ptr(st[0]), ptr(st[1]), rows, width, stream())
        return C, st[0], st[1]
    C = out if out is not None else torch.empty(*A.shape[:-1], N, device=A.device, dtype=A.dtype)
    C2 = torch.empty_like(C) if epi in (EPI_BIAS_GELU_DROP, EPI_BIAS_GELU_DROP_G) else None
    mean = rstd = gamma = beta = None
    if pro in (PRO_LN, PRO_LN_FOLD):
        mean, rstd, gamma, beta = ln
    call("hwgat_linear_nt_f32" if A.dtype == torch.float32 else "hwgat_linear_nt_bf16", ptr(A), ptr(W), ptr(bias), ptr(C), M, N, K, pro, ptr(mean), ptr(rstd),
         ptr(gamma), ptr(beta), pro_seed & 0xFFFFFFFF, float(pro_p), epi, ptr(res), ptr(C2), ptr(aux),
         epi_seed & 0xFFFFFFFF, float(epi_p), ptr(seed_base), stream())
    return (C, C2) if C2 is not None else C


def ln_fold(W, bias, gamma, beta, dtype):
    """(W o gamma in `dtype`, s, c) for pro = PRO_LN_FOLD from the fp32 master weights (hwgat_ln_fold)"""
    N, K = W.shape
    Wf = torch.empty(N, K, device=W.device, dtype=dtype)
    sc = torch.empty(2, N, device=W.device, dtype=torch.float32)
    call("hwgat_ln_fold", ptr(W), ptr(bias), ptr(gamma), ptr(beta), N, K, ptr(Wf), ptr(sc[0]), ptr(sc[1]),
         0 if dtype == torch.float32 else 1, stream())
    return Wf, sc[0], sc[1]


def linear_nt_ln(A, W, bias, ln, *, epi=EPI_BIAS, epi_seed=0, epi_p=0.0, out=None, folded=None, seed_base=None):
    """LN(A) . W^T + bias with the epilogue `epi` (EPI_BIAS or EPI_BIAS_GELU_DROP); W, bias are the fp32 master
    parameters, ln = (mean, rstd, gamma, beta).  Whole-tile token counts take the folded form (no per-element
    normalisation in the GEMM's load path), anything else the normalising loader."""
    mean, rstd, gamma, beta = ln
    M = A.numel() // A.shape[-1]
    if LN_FOLD and M % 128 == 0 and W.dtype == torch.float32 and gamma.dtype == torch.float32:   # hwgat_ln_fold reads fp32 masters
        Wf, s, c = folded if folded is not None else ln_fold(W, bias, gamma, beta, A.dtype)   # `folded`: made by WeightPrep
        return linear_nt(A, Wf, None, pro=PRO_LN_FOLD, ln=(mean, rstd, s, c), epi=epi, epi_seed=epi_seed, epi_p=epi_p, out=out,
                         seed_base=seed_base)
    Wc = W if W.dtype == A.dtype else W.to(A.dtype)
    return linear_nt(A, Wc, bias, pro=PRO_LN, ln=ln, epi=epi, epi_seed=epi_seed, epi_p=epi_p, out=out, seed_base=seed_base)


def _zero_rows_to(t, M, rows):
    """`t` (M rows) followed by zero rows up to `rows`"""
    out = torch.zeros((rows,) + tuple(t.reshape(M, -1).shape[1:]), device=t.device, dtype=t.dtype)
    out[:M] = t.reshape(M, -1)
    return out


def linear_tn(A, Bm, dW, db=None, *, pro_seed=0, pro_p=0.0, ln=None, seed_base=None, deterministic=False, pad_stage=False):
    """dW[N,K] += dropmask(A)[M,N]^T . ln(Bm)[M,K]; db[N] += colsum(dropmask(A)).
    ln = (mean, rstd, gamma, beta) normalises Bm on the fly.
    `deterministic`: the bit-reproducible form (hwgat_linear_tn_*_det: per-split partial images in a zero-filled
    workspace, added in split order; no float atomics).  It takes whole 32-row stages only; `pad_stage` (the fused
    block passes it: a micro-batch of 3 clips of 16 tokens is 48 rows) appends zero rows to A, Bm and the row statistics
    up to the next stage instead of refusing: a zero row of A adds an exact zero to every entry of dW and db, and its
    mask is the mask of a zero."""
    N, K = dW.shape
    M = A.numel() // N
    if deterministic and pad_stage and M % 32:
        rows = (M + 31) // 32 * 32
        A, Bm = _zero_rows_to(A, M, rows), _zero_rows_to(Bm, M, rows)
        if ln is not None:
            ln = (_zero_rows_to(ln[0], M, rows), _zero_rows_to(ln[1], M, rows), ln[2], ln[3])
        M = rows
    if N % 128 or K % 128:
        # 64x64 dW tiles (odd multiples of 64): split images added in a fixed order in every mode -- no float atomics
        need = _lib.lib().hwgat_linear_tn_det_bytes(M, N, K)
        if need <= 0 or (deterministic and M % 32):
            raise NotImplementedError("weight gradients need N, K multiples of 64 (and, deterministic, a token count "
                                      "that is a multiple of 32)")
        mean, rstd, gamma, beta = ln if ln is not None else (None, None, None, None)
        ws = torch.empty(need // 4, device=A.device, dtype=torch.float32)
        call("hwgat_linear_tn_f32_det" if A.dtype == torch.float32 else "hwgat_linear_tn_bf16_det", ptr(A), ptr(Bm), ptr(dW),
             ptr(db), M, N, K, pro_seed & 0xFFFFFFFF, float(pro_p), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(seed_base),
             ptr(ws), need, stream())
        return
    if deterministic:
        need = _lib.lib().hwgat_linear_tn_det_bytes(M, N, K)
        if M % 32 or need <= 0:
            raise NotImplementedError("deterministic weight gradients need a token count that is a multiple of 32 and "
                                      "N, K multiples of 128")
        mean, rstd, gamma, beta = ln if ln is not None else (None, None, None, None)
        ws = torch.zeros(need // 4, device=A.device, dtype=torch.float32)
        call("hwgat_linear_tn_f32_det" if A.dtype == torch.float32 else "hwgat_linear_tn_bf16_det", ptr(A), ptr(Bm), ptr(dW),
             ptr(db), M, N, K, pro_seed & 0xFFFFFFFF, float(pro_p), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(seed_base),
             ptr(ws), need, stream())
        return
    if A.dtype == torch.bfloat16 and ln is None and pro_p == 0.0:
        # plain bf16 operands: M-split partial tiles through a workspace + fixed-order reduction instead of global atomics
        need = _lib.lib().hwgat_linear_tn_bf16_ws_bytes(M, N, K)
        if need > 0:
            ws = torch.empty(need // 4, device=A.device, dtype=torch.float32)
            call("hwgat_linear_tn_bf16_ws", ptr(A), ptr(Bm), ptr(dW), ptr(db), M, N, K, ptr(ws), need, stream())
            return
    mean, rstd, gamma, beta = ln if ln is not None else (None, None, None, None)
    if A.dtype == torch.float32:
        # fp32, 256-aligned outputs and the narrow layers' whole-weight tiles: slabs + fixed-order reduction as well (any prologue)
        need = _lib.lib().hwgat_linear_tn_f32_ws_bytes(M, N, K)
        if need > 0:
            ws = torch.empty(need // 4, device=A.device, dtype=torch.float32)
            call("hwgat_linear_tn_f32_ws", ptr(A), ptr(Bm), ptr(dW), ptr(db), M, N, K, pro_seed & 0xFFFFFFFF, float(pro_p),
                 ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(ws), need, ptr(seed_base), stream())
            return
    call("hwgat_linear_tn_f32" if A.dtype == torch.float32 else "hwgat_linear_tn_bf16", ptr(A), ptr(Bm), ptr(dW), ptr(db), M, N, K, pro_seed & 0xFFFFFFFF,
         float(pro_p), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(seed_base), stream())


def ln_stats(x, gamma, beta):
    """per-row mean / rstd only (consumers normalise on the fly)"""
    d = x.shape[-1]
    n = x.numel() // d
    mean = torch.empty(n, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    call("hwgat_ln_fwd", ptr(x), ptr(gamma), ptr(beta), None, ptr(mean), ptr(rstd), n, d, dtype_code(x), stream())
    return mean, rstd


class LnGrads(NamedTuple):
    """what ln_backward returns; a member its options did not ask for is None"""
    dx: torch.Tensor
    dx_masked: Optional[torch.Tensor]       # with `mask`
    xn: Optional[torch.Tensor]              # with `beta`


def ln_backward(dy, x, mean, rstd, gamma, dres, dgamma, dbeta, mask=None, beta=None, seed_base=None, deterministic=False):
    """dx = dLN(dy) (+ dres); dgamma/dbeta accumulated in place.  mask = (seed, p): also dx_masked = dx * dropout-mask
    (the gradient in front of the dropout that produced this tensor).  `beta` given: ALSO xn = LN(x), for the
    weight-gradient launch of the Linear behind this LayerNorm (hwgat_ln_bwd_xn).
    `deterministic`: dgamma / dbeta through per-block images added in a fixed order (hwgat_ln_bwd_det).  -> LnGrads"""
    d = x.shape[-1]
    dx = torch.empty_like(x)
    dxm = torch.empty_like(x) if mask is not None else None
    xn = torch.empty_like(x) if beta is not None else None
    # the parameter lists of the four entry points are cuts of one: what a restricted form lacks, it does not take
    # (built up in place: this is host time of every block's backward, and the plain form is the most frequent)
    takes_xn = deterministic or beta is not None
    name = "hwgat_ln_bwd"
    args = (ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma))
    if takes_xn:
        args += (ptr(beta),)
    args += (ptr(dres), ptr(dx), ptr(dgamma), ptr(dbeta), x.numel() // d, d, dtype_code(x))
    if takes_xn or mask is not None:
        name = "hwgat_ln_bwd_masked"
        args += (ptr(dxm), (mask[0] if mask else 0) & 0xFFFFFFFF, float(mask[1]) if mask else 0.0)
        if takes_xn:
            name = "hwgat_ln_bwd_xn"
            args += (ptr(xn),)
        args += (ptr(seed_base),)
        if deterministic:
            name = "hwgat_ln_bwd_det"
            need = _lib.lib().hwgat_ln_bwd_det_bytes(d)
            ws = torch.empty(need // 4, device=x.device, dtype=torch.float32)
            args += (ptr(ws), need)
    call(name, *args, stream())
    return LnGrads(dx, dxm, xn)


_LN_IDENTITY = {}


def ln_identity(device, d):
    """(ones, zeros) of width d, fp32: the gamma / beta with which a LayerNorm prologue yields the bare xhat.  Kept per
    device and width; while a stream is being captured nothing is cached (a tensor from a graph's private pool must not
    outlive the capture), the two fills become nodes of that graph instead."""
    key = (device.type, device.index, d)
    if key in _LN_IDENTITY:
        return _LN_IDENTITY[key]
    if torch.cuda.is_current_stream_capturing():
        return torch.ones(d, device=device), torch.zeros(d, device=device)
    # host tensors copied over: the copy has completed when .to() returns, so every stream may read them
    pair = (torch.ones(d).to(device), torch.zeros(d).to(device))
    _LN_IDENTITY[key] = pair
    return pair


def ln_param_grads_from_g(G, db, W, gamma, beta, dW, dgamma, dbeta):
    """dW += G gamma + db (x) beta, dgamma += colsum(W * G), dbeta += db W, with G = dY^T xhat and db = colsum(dY): the
    parameter gradients of a LayerNorm -> Linear pair whose input needs no gradient (hwgat_ln_param_grads_from_g)."""
    N, K = dW.shape
    call("hwgat_ln_param_grads_from_g", ptr(G), ptr(db), ptr(W), ptr(gamma), ptr(beta), ptr(dW), ptr(dgamma), ptr(dbeta),
         N, K, stream())


def dw_wants_xn(x):
    """True where the weight-gradient launch of a LayerNorm -> Linear pair takes LN(x) as a plain operand written by the
    LayerNorm backward (bf16, whole 256-wide tiles: the LDS-DMA kernel gemm_bf16_tn8w.hip) instead of normalising x in its
    loaders."""
    d = x.shape[-1]
    return x.dtype == torch.bfloat16 and d % 256 == 0 and (x.numel() // d) % 128 == 0


def transpose(W, dtype=torch.float32):
    """W^T of a (small) weight, optionally cast to the activation dtype"""
    R, C = W.shape
    out = torch.empty(C, R, device=W.device, dtype=torch.float32)
    call("hwgat_transpose_f32", ptr(W), ptr(out), R, C, stream())
    return out if dtype == torch.float32 else out.to(dtype)


def dropout_mask(shape, seed, p, device, seed_base=None):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    call("hwgat_dropout_mask_f32", ptr(out), out.numel(), seed & 0xFFFFFFFF, float(p), ptr(seed_base), stream())
    return out


# ---------------------------------------------------------------- device-resident dropout seed
SEED_C1, SEED_C2, SEED_C3, SEED_SITE = 0x9E3779B1, 0x85EBCA77, 0x27D4EB2F, 0xC2B2AE35


def seed_base_value(initial, counter, salt):
    """host mirror of what hwgat_seed_set / hwgat_seed_advance leave in state[1]"""
    return (initial * SEED_C1 + counter * SEED_C2 + salt * SEED_C3) & 0xFFFFFFFF


def seed_set(state, counter, initial, salt):
    """state (4 int32 device words) <- {counter, base(counter), initial, salt}: the eager path, all four from host
    integers passed as kernel arguments (no H2D copy, no sync)"""
    call("hwgat_seed_set", ptr(state), counter & 0xFFFFFFFF, initial & 0xFFFFFFFF, salt & 0xFFFFFFFF, stream())


def seed_advance(state):
    """counter += 1 and the new base, on the device: the form a captured train step replays"""
    call("hwgat_seed_advance", ptr(state), stream())


# ---------------------------------------------------------------- Transformer baseline (models/Transformer.py)
EPI_BIAS_RELU_DROP, EPI_RELU_BWD = 7, 8
SEQ_MAX_LEN = 512


def seq_embed(x, Wt, bias, pe, out_dtype, pad_index, drop_p=0.0, seed=0, seed_base=None):
    """frames (B, T, F) fp32 -> (drop((x W^T + b) sqrt(d) + pe[:T]) (B, T, d) in `out_dtype`, key-padding words
    (B, ceil(T/32)) int32 with bit t set iff x[b, t, 0] == pad_index), one launch (hwgat_seq_embed_fwd).  Wt = W^T (F, d)."""
    B, T, F = x.shape
    d = Wt.shape[1]
    out = torch.empty(B, T, d, device=x.device, dtype=out_dtype)
    pad = torch.empty(B, (T + 31) // 32, device=x.device, dtype=torch.int32)
    call("hwgat_seq_embed_fwd", ptr(x), ptr(Wt), ptr(bias), ptr(pe), ptr(out), ptr(pad), B, T, F, d, float(pad_index),
         dtype_code(out), seed & 0xFFFFFFFF, float(drop_p), ptr(seed_base), stream())
    return out, pad


def seq_embed_backward(dout, x, dW, db, drop_p=0.0, seed=0, seed_base=None):
    """dW (d, F) += g^T x, db (d) += colsum(g), g = dout * mask * sqrt(d): fixed-order split sums (bit-reproducible)"""
    F = x.shape[-1]
    d = dout.shape[-1]
    need = _lib.lib().hwgat_seq_embed_bwd_bytes(F, d)
    if need <= 0:
        raise NotImplementedError(f"the frame embedding takes at most 512 input features, got {F}")
    ws = torch.empty(need // 4, device=x.device, dtype=torch.float32)
    call("hwgat_seq_embed_bwd", ptr(dout), ptr(x), ptr(dW), ptr(db), x.numel() // F, F, d, dtype_code(dout),
         seed & 0xFFFFFFFF, float(drop_p), ptr(seed_base), ptr(ws), need, stream())


def seq_attn_forward(qkv, pad, n_heads, drop=None, want_lse=True):
    """qkv (B, T, 3d) -> (o (B, T, d), lse (B, nH, T) fp32 or None); `drop` = (seed, p[, seed_base]) or None"""
    B, T, d3 = qkv.shape
    d = d3 // 3
    o = torch.empty(B, T, d, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(B, n_heads, T, device=qkv.device, dtype=torch.float32) if want_lse else None
    seed, p, base = (int(drop[0]) & 0xFFFFFFFF, float(drop[1]), drop[2] if len(drop) > 2 else None) if drop else (0, 0.0, None)
    call("hwgat_seq_attn_fwd", ptr(qkv), ptr(o), ptr(lse), ptr(pad), B, T, n_heads, d // n_heads, dtype_code(qkv),
         seed, p, ptr(base), stream())
    return o, lse


def seq_attn_backward(qkv, o, do, lse, pad, n_heads, drop=None):
    """dqkv (B, T, 3d) of seq_attn_forward; no atomics (two launches), bit-reproducible"""
    B, T, d3 = qkv.shape
    d = d3 // 3
    dqkv = torch.empty_like(qkv)
    D = torch.empty(B, n_heads, T, device=qkv.device, dtype=torch.float32)
    seed, p, base = (int(drop[0]) & 0xFFFFFFFF, float(drop[1]), drop[2] if len(drop) > 2 else None) if drop else (0, 0.0, None)
    call("hwgat_seq_attn_bwd", ptr(qkv), ptr(o), ptr(do.contiguous()), ptr(lse), ptr(pad), ptr(dqkv), ptr(D), B, T,
         n_heads, d // n_heads, dtype_code(qkv), seed, p, ptr(base), stream())
    return dqkv


class _SeqAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, pad, n_heads, drop):
        o, lse = seq_attn_forward(qkv, pad, n_heads, drop, want_lse=True)
        ctx.save_for_backward(qkv, o, lse, pad)
        ctx.cfg = (n_heads, drop)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, pad = ctx.saved_tensors
        n_heads, drop = ctx.cfg
        return seq_attn_backward(qkv, o, do, lse, pad, n_heads, drop), None, None, None


def seq_attention(qkv, pad, n_heads, drop=None):
    """dense key-padded multi-head attention over the frames of each clip (hwgat_seq_attn_*): qkv (B, T, 3d) in the
    in_proj layout -> o (B, T, d); `pad` from seq_embed; `drop` = (seed, p[, seed_base]) on the probabilities"""
    return _SeqAttn.apply(qkv.contiguous(), pad, int(n_heads), drop if drop and float(drop[1]) > 0.0 else None)


class _SeqMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        B, T, d = x.shape
        out = torch.empty(B, d, device=x.device, dtype=torch.float32)
        idx = torch.empty(B, d, device=x.device, dtype=torch.int32)
        call("hwgat_seq_maxpool_fwd", ptr(x), ptr(out), ptr(idx), B, T, d, dtype_code(x), stream())
        ctx.save_for_backward(idx)
        ctx.shape, ctx.dtype = (B, T, d), x.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, T, d = ctx.shape
        dx = torch.empty(B, T, d, device=dout.device, dtype=ctx.dtype)
        call("hwgat_seq_maxpool_bwd", ptr(dout.float().contiguous()), ptr(idx), ptr(dx), B, T, d, dtype_code(dx), stream())
        return dx


def seq_max_pool(x):
    """max over the frames of (B, T, d) -> (B, d) fp32 (first index of the maximum, as torch.max)"""
    return _SeqMaxPool.apply(x.contiguous())


# ---------------------------------------------------------------- ST-GCN baseline (models/STGCN.py, stgcn_block.py)
# fp32, channels-last (N, T, V, C).  Thin launchers of csrc/stgcn_conv.hip / stgcn_ops.hip; nothing here is differentiable
# by itself (the autograd nodes are in stgcn_block.py).
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
STGCN_MAX_NODES = 32


def _ws(nbytes, device):
    if nbytes <= 0:
        raise NotImplementedError("shape not supported by the GCN baselines' kernels")
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32), nbytes


def pad32(c):
    return (c + 31) // 32 * 32


def stgcn_weight_image(W, mode, cin_pad=None):
    """the k-major image of a conv master weight (C_out, C_in, taps, 1): mode 0 (taps, CinP, C_out) for the forward,
    mode 1 (taps, C_out, CinP) for the input gradient; rows / columns C_in .. CinP are zero"""
    Cout, Cin, taps = W.shape[0], W.shape[1], W.shape[2]
    CinP = cin_pad or Cin
    out = torch.empty((taps, CinP, Cout) if mode == 0 else (taps, Cout, CinP), device=W.device, dtype=torch.float32)
    call("hwgat_stgcn_weight_prep", ptr(W), ptr(out), Cout, Cin, taps, CinP, mode, stream())
    return out


def stgcn_conv(x, wk, bias, stride=1, pad=0):
    """(N, T, V, Cin) -> (N, T_out, V, Cout) with the mode-0 image wk (taps, Cin, Cout)"""
    N, T, V, Cin = x.shape
    taps, _, Cout = wk.shape
    To = (T + 2 * pad - taps) // stride + 1
    out = torch.empty(N, To, V, Cout, device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_conv", ptr(x), ptr(wk), ptr(bias), None, None, ptr(out), N, T, To, V, Cin, Cout, taps, stride, pad, 0,
         stream())
    return out


def stgcn_conv_dx(dy, wkt, t_x, stride=1, pad=0, add=None, mask=None):
    """input gradient (N, t_x, V, CxP) of a convolution from dy (N, T_y, V, Cy) and the mode-1 image wkt (taps, Cy, CxP);
    `add` (+ `mask`): out += add [mask > 0]"""
    N, Ty, V, Cy = dy.shape
    taps, _, Cx = wkt.shape
    out = torch.empty(N, t_x, V, Cx, device=dy.device, dtype=torch.float32)
    call("hwgat_stgcn_conv", ptr(dy), ptr(wkt), None, ptr(add), ptr(mask), ptr(out), N, Ty, t_x, V, Cy, Cx, taps, stride, pad,
         1, stream())
    return out


def stgcn_conv_dw(x, dy, w_shape, stride=1, pad=0):
    """weight gradient in the master layout `w_shape` = (C_out, C_in, taps, 1); x may carry padded channels"""
    N, T, V, CinP = x.shape
    Cout, Cin, taps = w_shape[0], w_shape[1], w_shape[2]
    To = dy.shape[1]
    ws, nbytes = _ws(_lib.lib().hwgat_stgcn_conv_dw_bytes(N * To * V, CinP, Cout, taps), x.device)
    dW = torch.empty(tuple(w_shape), device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_conv_dw", ptr(x), ptr(dy), ptr(dW), N, T, To, V, CinP, Cin, Cout, taps, stride, pad, ptr(ws), nbytes,
         stream())
    return dW


def stgcn_colsum(x):
    C = x.shape[-1]
    M = x.numel() // C
    ws, nbytes = _ws(_lib.lib().hwgat_stgcn_red_bytes(C), x.device)
    out = torch.empty(C, device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_colsum", ptr(x), ptr(out), M, C, ptr(ws), nbytes, stream())
    return out


def stgcn_bn_stats(x, running_mean=None, running_var=None, num_batches=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """batch (mean, rstd) of the columns of x (..., C); the running values are updated on the device"""
    C = x.shape[-1]
    M = x.numel() // C
    if M < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    ws, nbytes = _ws(_lib.lib().hwgat_stgcn_red_bytes(C), x.device)
    st = torch.empty(2, C, device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_bn_stats", ptr(x), M, C, float(eps), float(momentum), ptr(st[0]), ptr(st[1]), ptr(running_mean),
         ptr(running_var), ptr(num_batches), ptr(ws), nbytes, stream())
    return st[0], st[1]


def stgcn_bn_eval_stats(running_mean, running_var, eps=BN_EPS):
    C = running_mean.shape[0]
    st = torch.empty(2, C, device=running_mean.device, dtype=torch.float32)
    call("hwgat_stgcn_bn_eval_stats", ptr(running_mean), ptr(running_var), float(eps), ptr(st[0]), ptr(st[1]), C, stream())
    return st[0], st[1]


def stgcn_bn_apply(x, mean, rstd, gamma, beta, relu, res=None, res_bn=None):
    """relu?(bn(x) + res) ; res_bn = (mean, rstd, gamma, beta) normalises the residual operand too"""
    C = x.shape[-1]
    out = torch.empty_like(x)
    rb = res_bn or (None, None, None, None)
    call("hwgat_stgcn_bn_apply", ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(res), ptr(rb[0]), ptr(rb[1]),
         ptr(rb[2]), ptr(rb[3]), ptr(out), x.numel() // C, C, int(bool(relu)), stream())
    return out


def stgcn_bn_backward(dy, y, x, mean, rstd, gamma, train):
    """(dx, dgamma, dbeta); y = the ReLU output behind this BatchNorm (gates dy) or None"""
    C = x.shape[-1]
    ws, nbytes = _ws(_lib.lib().hwgat_stgcn_red_bytes(C), x.device)
    dx = torch.empty_like(x)
    dg = torch.empty(2, C, device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_bn_bwd", ptr(dy), ptr(y), ptr(x), ptr(mean), ptr(rstd), ptr(gamma), ptr(dx), ptr(dg[0]), ptr(dg[1]),
         x.numel() // C, C, int(bool(train)), ptr(ws), nbytes, stream())
    return dx, dg[0], dg[1]


def stgcn_aggregate(y, A, E):
    """(N, T, V, 3C) -> (N, T, V, C): sum_{k,v} (A o E)[k, v, w] y[.., v, k C + c]"""
    N, T, V, C3 = y.shape
    out = torch.empty(N, T, V, C3 // 3, device=y.device, dtype=torch.float32)
    call("hwgat_stgcn_agg_fwd", ptr(y), ptr(A), ptr(E), ptr(out), N * T, V, C3 // 3, stream())
    return out


def stgcn_aggregate_backward(y, d, A, E, want_dE):
    """(dy, dE or None) of stgcn_aggregate"""
    N, T, V, C3 = y.shape
    dy = torch.empty_like(y)
    dE = ws = None
    nbytes = 0
    if want_dE:
        dE = torch.empty_like(A)
        ws, nbytes = _ws(_lib.lib().hwgat_stgcn_agg_bwd_bytes(N * T), y.device)
    call("hwgat_stgcn_agg_bwd", ptr(y), ptr(d), ptr(A), ptr(E), ptr(dy), ptr(dE), N * T, V, C3 // 3, ptr(ws), nbytes, stream())
    return dy, dE


def stgcn_pool(x, p=0.0, seed=0, seed_base=None):
    """(N, R, C) -> (N, C): mean over R, head dropout (mask of an (N, C) tensor) fused"""
    N, R, C = x.shape
    out = torch.empty(N, C, device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_pool_fwd", ptr(x), ptr(out), N, R, C, seed & 0xFFFFFFFF, float(p), ptr(seed_base), stream())
    return out


def stgcn_pool_backward(dout, R, p=0.0, seed=0, seed_base=None):
    N, C = dout.shape
    dx = torch.empty(N, R, C, device=dout.device, dtype=torch.float32)
    call("hwgat_stgcn_pool_bwd", ptr(dout), ptr(dx), N, R, C, seed & 0xFFFFFFFF, float(p), ptr(seed_base), stream())
    return dx


def stgcn_copy_cols(x, width):
    """the last dimension of x padded with zeros (or cropped) to `width`"""
    C = x.shape[-1]
    out = torch.empty(*x.shape[:-1], width, device=x.device, dtype=torch.float32)
    call("hwgat_stgcn_copy_cols", ptr(x), C, ptr(out), width, x.numel() // C, stream())
    return out


# ---------------------------------------------------------------- DecoupledGCN baseline (models/DecoupledGCN.py, dgcn_block.py)
# fp32, channels-last (N, T, V, C).  Thin launchers of csrc/dgcn_ops.hip; the autograd node is in dgcn_block.py.
def dgcn_aggregate(y, An, groups):
    """(N, T, V, 3C) -> (N, T, V, C): sum_{k,v} An[k, c mod G, v, w] y[.., v, k C + c], An (3, G, V, V)"""
    N, T, V, C3 = y.shape
    out = torch.empty(N, T, V, C3 // 3, device=y.device, dtype=torch.float32)
    call("hwgat_dgcn_agg_fwd", ptr(y), ptr(An), ptr(out), N * T, V, C3 // 3, groups, stream())
    return out


def dgcn_aggregate_backward(y, d, An, groups, want_dAn=True):
    """(dy, dAn or None) of dgcn_aggregate"""
    N, T, V, C3 = y.shape
    dy = torch.empty_like(y)
    dAn = ws = None
    nbytes = 0
    if want_dAn:
        dAn = torch.empty_like(An)
        ws, nbytes = _ws(_lib.lib().hwgat_dgcn_agg_bwd_bytes(N * T, groups), y.device)
    call("hwgat_dgcn_agg_bwd", ptr(y), ptr(d), ptr(An), ptr(dy), ptr(dAn), N * T, V, C3 // 3, groups, ptr(ws), nbytes,
         stream())
    return dy, dAn


def dgcn_gate_sum(h, axis, scale=1.0, g=None, sv=None, st=None, sc=None, m=None, m_scale=0.0):
    """scale * sum over t (axis 0, -> (N, V, C)) or over v (axis 1, -> (N, T, C)) of
    h (g (1 + sv[n, v]) (1 + st[n, t]) (1 + sc[n, c]) + m[n, t, c] m_scale); absent factors are 1, an absent m term 0"""
    N, T, V, C = h.shape
    out = torch.empty(N, V if axis == 0 else T, C, device=h.device, dtype=torch.float32)
    call("hwgat_dgcn_gate_sum", ptr(h), ptr(g), ptr(sv), ptr(st), ptr(sc), ptr(m), float(m_scale), ptr(out), N, T, V, C,
         int(axis), float(scale), stream())
    return out


def dgcn_gate_apply(h, sv, st, sc):
    """h (1 + sv[n, v]) (1 + st[n, t]) (1 + sc[n, c])"""
    N, T, V, C = h.shape
    out = torch.empty_like(h)
    call("hwgat_dgcn_gate_apply", ptr(h), ptr(sv), ptr(st), ptr(sc), ptr(out), N, T, V, C, stream())
    return out


def dgcn_gate_backward(d, sv, st, sc, dm1, dm0):
    """dh = d (1 + sv)(1 + st)(1 + sc) + dm1[n, t, c] (1 + sv) / V + dm0[n, v, c] / T"""
    N, T, V, C = d.shape
    dh = torch.empty_like(d)
    call("hwgat_dgcn_gate_bwd", ptr(d), ptr(sv), ptr(st), ptr(sc), ptr(dm1), ptr(dm0), ptr(dh), N, T, V, C, stream())
    return dh


def dgcn_abs_sum(x, axis, bn=None, fs=None):
    """axis 0: (N, V) = sum_{t,c} |z|; axis 1: (N, T) = sum_{v,c} |z| fs[n, v]; z = x or its BatchNorm read
    bn = (mean, rstd, gamma, beta)"""
    N, T, V, C = x.shape
    b = bn or (None, None, None, None)
    out = torch.empty(N, V if axis == 0 else T, device=x.device, dtype=torch.float32)
    call("hwgat_dgcn_abs_sum", ptr(x), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(fs), ptr(out), N, T, V, C, int(axis),
         stream())
    return out


def dgcn_draw(p, seed, seed_base=None):
    """Bernoulli(p) seeds (1.0 / 0.0) from the hash uniform of (seed + *seed_base, element index)"""
    out = torch.empty_like(p)
    call("hwgat_dgcn_draw", ptr(p), ptr(out), p.numel(), seed & 0xFFFFFFFF, ptr(seed_base), stream())
    return out


def dgcn_mask_spatial(seeds, A):
    """(mask * scale (N, V), scale (1,)) of the spatial DropGraph: joints reached by a seed through A (V, V) are dropped"""
    N, V = seeds.shape
    f = torch.empty_like(seeds)
    scale = torch.empty(1, device=seeds.device, dtype=torch.float32)
    call("hwgat_dgcn_mask_spatial", ptr(seeds), ptr(A), ptr(f), ptr(scale), N, V, stream())
    return f, scale


def dgcn_mask_temporal(seeds, block):
    """(mask * scale (N, T), scale (1,)) of the temporal DropGraph: frames within block // 2 of a seed are dropped"""
    N, T = seeds.shape
    f = torch.empty_like(seeds)
    scale = torch.empty(1, device=seeds.device, dtype=torch.float32)
    call("hwgat_dgcn_mask_temporal", ptr(seeds), ptr(f), ptr(scale), N, T, int(block), stream())
    return f, scale


def dgcn_merge(c, bn, r, res_bn, fs1, ft1, fs2, ft2):
    """relu(bn(c) fs1[n, v] ft1[n, t] + r' fs2[n, v] ft2[n, t]); bn / res_bn = (mean, rstd, gamma, beta), res_bn None: r' = r"""
    N, T, V, C = c.shape
    rb = res_bn or (None, None, None, None)
    out = torch.empty_like(c)
    call("hwgat_dgcn_merge", ptr(c), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(r), ptr(rb[0]), ptr(rb[1]),
         ptr(rb[2]), ptr(rb[3]), ptr(fs1), ptr(ft1), ptr(fs2), ptr(ft2), ptr(out), N, T, V, C, stream())
    return out


def dgcn_merge_backward(dout, out, fs1, ft1, fs2, ft2):
    """(dz1, dz2): dout [out > 0] times the two mask products"""
    N, T, V, C = dout.shape
    dz1, dz2 = torch.empty_like(dout), torch.empty_like(dout)
    call("hwgat_dgcn_merge_bwd", ptr(dout), ptr(out), ptr(fs1), ptr(ft1), ptr(fs2), ptr(ft2), ptr(dz1), ptr(dz2), N, T, V,
         C, stream())
    return dz1, dz2


def dgcn_masked_sum(a, ma, b, mb):
    """a [ma > 0] + b [mb > 0]; a mask that is None passes everything"""
    out = torch.empty_like(a)
    call("hwgat_dgcn_masked_sum", ptr(a), ptr(ma), ptr(b), ptr(mb), ptr(out), a.numel(), stream())
    return out


# ---------------------------------------------------------------- smoothed cross-entropy and evaluation (train.py, evaluate.py)
# Thin launchers of csrc/loss_eval.hip.  logits fp32 (B, C), target int64 (B); `n_valid` is a device int32 (1,) or None (all
# rows): rows at or beyond it are left untouched by the forward and the accumulator and are zero in the backward.
EVAL_ACC_HEADER_WORDS = 5       # n_samples, n_batches, n_invalid (int64), loss_sum_samples, loss_sum_batches (double)

# The four criteria are one body.  `offset` None: the whole batch, `count` its n_valid; else one slice of a zero-padded
# batch, `count` the batch's n_rows (a device int32 (1,) with its real row count) and `offset` the slice's first row in it
# (a host integer): rows of the slice at or beyond n_rows - offset are dead.  target_b (B,) int64 and lam (B,) fp32, slices
# of a mixer's records, make the target a pair; `teacher` (B, C) fp32 with the distillation `state` adds the soft term.
def _ce_check(logits, target, count, offset, target_b, lam, teacher, state):
    if (target_b is None) != (lam is None):
        raise ValueError("target_b and lam come together (a mixer's records) or not at all")
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"logits must be fp32 (B, C), got {logits.dtype} {tuple(logits.shape)}")
    if target.dtype != torch.int64 or target.shape != logits.shape[:1]:
        raise ValueError(f"target must be int64 (B,), got {target.dtype} {tuple(target.shape)}")
    if offset is not None:
        if count is None or count.dtype != torch.int32 or count.numel() != 1:
            raise ValueError("n_rows must be a device int32 tensor of one element")
        if not 0 <= offset < 2 ** 31:
            raise ValueError(f"the slice's offset must be in [0, 2^31), got {offset}")
    if lam is not None:
        if target_b.dtype != torch.int64 or target_b.shape != target.shape:
            raise ValueError(f"target_b must be int64 {tuple(target.shape)}, got {target_b.dtype} {tuple(target_b.shape)}")
        if lam.dtype != torch.float32 or lam.shape != target.shape:
            raise ValueError(f"lam must be fp32 {tuple(target.shape)}, got {lam.dtype} {tuple(lam.shape)}")
    if teacher is not None:
        if teacher.dtype != torch.float32 or teacher.shape != logits.shape:
            raise ValueError(f"teacher must be fp32 {tuple(logits.shape)}, got {teacher.dtype} {tuple(teacher.shape)}")
        _kd_state_check(state)


def _ce_outputs(logits, sliced, paired, taught):
    """the forward's result tuple on three fresh buffers (per-row vectors first, the scalars behind them): loss, row_loss,
    lse, rank, pred; a slice adds correct, live; a pair or a teacher row_loss_b, rank_b; a teacher lse_s, lse_t, row_kd,
    t_pred, kd, agree, t_correct"""
    B, dev = logits.shape[0], logits.device
    nf, ni = (6, 4) if taught else (3, 3) if paired else (2, 2)
    f = torch.empty(nf * B + 1 + taught, device=dev, dtype=torch.float32)
    i = torch.empty(ni * B + sliced, device=dev, dtype=torch.int32)
    out = (f[nf * B:nf * B + 1], f[:B], f[B:2 * B], i[:B], i[B:2 * B])
    if sliced:
        words = torch.empty(3 if taught else 1, device=dev, dtype=torch.int64)
        out += (words[:1], i[ni * B:])
    if paired or taught:
        out += (f[2 * B:3 * B], i[2 * B:3 * B])
    if taught:
        out += (f[3 * B:4 * B], f[4 * B:5 * B], f[5 * B:6 * B], i[3 * B:4 * B], f[6 * B + 1:], words[1:2], words[2:])
    return out


def _ce_entry(sliced, paired, taught):
    """the entry points' stem: each form has its own, named after what it adds"""
    return "hwgat_kd" if taught else "hwgat_mbsce" if paired else "hwgat_bsce" if sliced else "hwgat_sce"


def _ce_forward(logits, target, eps, count, offset=None, target_b=None, lam=None, teacher=None, state=None, out=None):
    _ce_check(logits, target, count, offset, target_b, lam, teacher, state)
    B, C = logits.shape
    sliced, paired, taught = offset is not None, lam is not None, teacher is not None
    if out is None:
        out = _ce_outputs(logits, sliced, paired, taught)
    # the parameter lists of the four entry points are cuts of hwgat_kd_fwd's: what a restricted form lacks, it does not
    # take (built up in place, once, after the choice: this is host time of every step)
    args = (ptr(logits),)
    if taught:
        args += (ptr(teacher),)
    args += (ptr(target),)
    if paired or taught:
        args += (ptr(target_b), ptr(lam))
    args += (ptr(count),)
    if sliced:
        args += (offset,)
    if taught:
        args += (ptr(state),)
    args += (ptr(out[2]), ptr(out[1]), ptr(out[3]), ptr(out[4]), ptr(out[0]))          # lse, row_loss, rank, pred, loss
    if sliced:
        args += (ptr(out[5]), ptr(out[6]))                                                # correct, live
    if paired or taught:
        args += (ptr(out[7]), ptr(out[8])) if paired else (None, None)                    # row_loss_b, rank_b: not written
    if taught:
        args += tuple(map(ptr, out[9:]))                       # lse_s, lse_t, row_kd, t_pred, kd, agree, t_correct
    call(_ce_entry(sliced, paired, taught) + "_fwd", *args, B, C, float(eps), stream())
    return out


def _ce_backward(logits, target, lse, g, eps, count, offset=None, target_b=None, lam=None, teacher=None, state=None,
                 lse_s=None, lse_t=None, out=None):
    _ce_check(logits, target, count, offset, target_b, lam, teacher, state)
    B, C = logits.shape
    sliced, paired, taught = offset is not None, lam is not None, teacher is not None
    dz = torch.empty_like(logits) if out is None else out
    args = (ptr(logits),)
    if taught:
        args += (ptr(teacher),)
    args += (ptr(target),)
    if paired or taught:
        args += (ptr(target_b), ptr(lam))
    args += (ptr(count),)
    if sliced:
        args += (offset,)
    if taught:
        args += (ptr(state), ptr(lse), ptr(lse_s), ptr(lse_t))
    else:
        args += (ptr(lse),)
    call(_ce_entry(sliced, paired, taught) + "_bwd", *args, ptr(g), ptr(dz), B, C, float(eps), stream())
    return dz


def sce_forward(logits, target, eps, n_valid=None, out=None):
    """(loss (1,), row_loss (B,), lse (B,), rank (B,) int32, pred (B,) int32) of the smoothed cross-entropy; `out` takes the
    same five tensors preallocated"""
    return _ce_forward(logits, target, eps, n_valid, out=out)


def sce_backward(logits, target, lse, g, eps, n_valid=None, out=None):
    """d loss / d logits times the device scalar `g` (float32, one element)"""
    return _ce_backward(logits, target, lse, g, eps, n_valid, out=out)


def eval_acc_words(num_classes, k_max, cap):
    """size of the accumulator block of eval_accumulate in 8-byte words (layout: include/hwgat_hip.h)"""
    n = _lib.lib().hwgat_eval_acc_bytes(int(num_classes), int(k_max), int(cap))
    if n < 0:
        raise ValueError(f"no accumulator for num_classes {num_classes}, k_max {k_max}, log capacity {cap}")
    return n // 8


def eval_accumulate(acc, row_loss, rank, pred, target, loss, n_valid, num_classes, k_max, cap):
    """fold one sce_forward into the int64 accumulator block `acc` (eval_acc_words long, zeroed to reset)"""
    if acc.dtype != torch.int64 or acc.numel() < eval_acc_words(num_classes, k_max, cap):
        raise ValueError("the accumulator block must be int64 and eval_acc_words(num_classes, k_max, cap) long")
    call("hwgat_eval_accumulate", ptr(acc), ptr(row_loss), ptr(rank), ptr(pred), ptr(target), ptr(loss), ptr(n_valid),
         row_loss.numel(), int(num_classes), int(k_max), int(cap), stream())


class _SmoothCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, eps, n_valid):
        loss, _, lse, rank, pred = sce_forward(logits, target, eps, n_valid)
        ctx.save_for_backward(logits, target, lse)
        ctx.eps, ctx.n_valid = eps, n_valid
        ctx.mark_non_differentiable(rank, pred)
        return loss.view(()), rank, pred

    @staticmethod
    def backward(ctx, g, _rank, _pred):
        logits, target, lse = ctx.saved_tensors
        g = g.reshape(1).to(torch.float32)                 # stays on the device: nothing is read back
        return sce_backward(logits, target, lse, g, ctx.eps, ctx.n_valid), None, None, None


def smooth_ce(logits, target, eps, n_valid=None):
    """(loss, rank, pred): the batch-mean smoothed cross-entropy as an autograd node (forward two launches, backward one),
    with the detached rank of the target in a stable descending sort and the arg-max (both int32)"""
    return _SmoothCE.apply(logits.float().contiguous(), target.contiguous(), float(eps), n_valid)


class _SlicedCE(torch.autograd.Function):
    """the autograd node of the three slice criteria.  Results: loss, rank, pred, correct; a teacher adds t_pred, kd, agree,
    t_correct.  Only the loss is differentiable, and only with respect to the (student's) logits.  (The whole-batch
    criterion keeps _SmoothCE: its n_valid has other semantics and it has no correct count)"""

    @staticmethod
    def forward(ctx, logits, target, eps, n_rows, offset, target_b, lam, teacher, state):
        out = _ce_forward(logits, target, eps, n_rows, offset, target_b, lam, teacher, state)
        ctx.paired, ctx.taught = lam is not None, teacher is not None
        ctx.save_for_backward(logits, target, out[2], *((target_b, lam) if ctx.paired else ()),
                              *((teacher, state, out[9], out[10]) if ctx.taught else ()))        # out[2]: lse; lse_s, lse_t
        ctx.eps, ctx.n_rows, ctx.offset = eps, n_rows, offset
        # the views that go out are what is marked: a float view left unmarked would carry a grad_fn and keep the node alive
        res = (out[3], out[4], out[5].view(()))            # rank, pred, correct
        if ctx.taught:
            res += (out[12], out[13].view(()), out[14].view(()), out[15].view(()))
        ctx.mark_non_differentiable(*res)
        return (out[0].view(()),) + res

    @staticmethod
    def backward(ctx, g, *_):
        logits, target, lse, *rest = ctx.saved_tensors
        target_b, lam = rest[:2] if ctx.paired else (None, None)
        teacher, state, lse_s, lse_t = rest[-4:] if ctx.taught else (None,) * 4
        g = g.reshape(1).to(torch.float32)                 # stays on the device: nothing is read back
        dz = _ce_backward(logits, target, lse, g, ctx.eps, ctx.n_rows, ctx.offset, target_b, lam, teacher, state, lse_s, lse_t)
        return (dz,) + (None,) * 8


def _needs(form, **members):
    """a restricted launcher refuses what its form cannot do without, instead of quietly becoming a smaller form"""
    missing = [k for k, v in members.items() if v is None]
    if missing:
        raise ValueError(f"{form} needs {' and '.join(missing)}")


# ---- the same loss for one slice of a zero-padded batch
def bsce_forward(logits, target, eps, n_rows, offset, out=None):
    """(loss (1,), row_loss (B,), lse (B,), rank (B,) int32, pred (B,) int32, correct (1,) int64, live (1,) int32) of one
    slice: loss is the live rows' sum over the BATCH's row count (exactly 0 for a slice without live rows), correct the
    number of live rows whose target ranks first; dead rows of the per-row outputs are not written.  `out` takes the same
    seven tensors preallocated"""
    return _ce_forward(logits, target, eps, n_rows, int(offset), out=out)


def bsce_backward(logits, target, lse, g, eps, n_rows, offset, out=None):
    """d loss / d logits of bsce_forward times the device scalar `g`; exactly zero in the dead rows"""
    return _ce_backward(logits, target, lse, g, eps, n_rows, int(offset), out=out)


def batch_sliced_ce(logits, target, eps, n_rows, offset):
    """(loss, rank, pred, correct): a slice's share of the batch-mean smoothed cross-entropy as an autograd node (forward
    three launches, backward one), with the detached rank and arg-max of its live rows and their correct count (int64)"""
    return _SlicedCE.apply(logits.float().contiguous(), target.contiguous(), float(eps), n_rows, int(offset), None, None, None,
                          None)


# ---- the slice criterion with two targets
def mbsce_forward(logits, target, target_b, lam, eps, n_rows, offset, out=None):
    """bsce_forward with two targets and a weight per row: (loss, row_loss, lse, rank, pred, correct, live, row_loss_b,
    rank_b); row_loss is lam l(t) + (1 - lam) l(t_b), rank the dominant label's (t when lam >= 0.5), row_loss_b / rank_b (B,)
    the partner label's own.  `out` takes the same nine tensors preallocated"""
    _needs("mbsce_forward", target_b=target_b, lam=lam)
    return _ce_forward(logits, target, eps, n_rows, int(offset), target_b, lam, out=out)


def mbsce_backward(logits, target, target_b, lam, lse, g, eps, n_rows, offset, out=None):
    """d loss / d logits of mbsce_forward times the device scalar `g`; exactly zero in the dead rows"""
    _needs("mbsce_backward", target_b=target_b, lam=lam)
    return _ce_backward(logits, target, lse, g, eps, n_rows, int(offset), target_b, lam, out=out)


def mixed_sliced_ce(logits, target, target_b, lam, eps, n_rows, offset):
    """(loss, rank, pred, correct): batch_sliced_ce with the pair target -- lam l(target) + (1 - lam) l(target_b) per row,
    rank and correct on the dominant label -- as an autograd node (forward four launches, backward one)"""
    return _SlicedCE.apply(logits.float().contiguous(), target.contiguous(), float(eps), n_rows, int(offset),
                          target_b.contiguous(), lam.contiguous(), None, None)


# ---- the slice criterion with a teacher's logits beside the labels (the state: kd_state / kd_set below)
def kd_forward(logits, teacher, target, target_b, lam, state, eps, n_rows, offset, out=None):
    """mbsce_forward blended with the tempered KL from the teacher's logits: (loss, row_loss, lse, rank, pred, correct, live,
    row_loss_b, rank_b, lse_s, lse_t, row_kd, t_pred, kd, agree, t_correct).  `target_b` and `lam` are both None without a
    mixer (row_loss_b / rank_b are then not written).  `out` takes the same sixteen tensors preallocated"""
    _needs("kd_forward", teacher=teacher, state=state)
    return _ce_forward(logits, target, eps, n_rows, int(offset), target_b, lam, teacher, state, out=out)


def kd_backward(logits, teacher, target, target_b, lam, state, lse, lse_s, lse_t, g, eps, n_rows, offset, out=None):
    """d loss / d logits of kd_forward times the device scalar `g`; exactly zero in the dead rows"""
    _needs("kd_backward", teacher=teacher, state=state, lse_s=lse_s, lse_t=lse_t)
    return _ce_backward(logits, target, lse, g, eps, n_rows, int(offset), target_b, lam, teacher, state, lse_s, lse_t, out=out)


def distilled_sliced_ce(logits, teacher, target, target_b, lam, state, eps, n_rows, offset):
    """(loss, rank, pred, correct, t_pred, kd, agree, t_correct): mixed_sliced_ce (batch_sliced_ce when `target_b` and `lam`
    are None) blended with the tempered KL from `teacher` as (1 - alpha) hard + alpha kd, alpha and tau read from the device
    words of `state` when the kernels run, as an autograd node (forward at most five launches, backward one).  The
    gradient goes to the student's logits only"""
    return _SlicedCE.apply(logits.float().contiguous(), target.contiguous(), float(eps), n_rows, int(offset),
                          None if target_b is None else target_b.contiguous(), None if lam is None else lam.contiguous(),
                          teacher.detach().float().contiguous(), state)


# ---------------------------------------------------------------- train meters (csrc/train_meter.hip, train.TrainMeter)
# The block is int64 words (layout: include/hwgat_hip.h, "train meters"; the slot constants are mirrored in train.py).
def meter_words(log_capacity, history_capacity):
    """size of a meter block in 8-byte words"""
    n = _lib.lib().hwgat_meter_bytes(int(log_capacity), int(history_capacity))
    if n < 0:
        raise ValueError(f"no meter block for log capacity {log_capacity}, history capacity {history_capacity}")
    return n // 8


def _meter_check(block, log_capacity, history_capacity):
    if block.dtype != torch.int64 or block.numel() < meter_words(log_capacity, history_capacity):
        raise ValueError("the meter block must be int64 and meter_words(log_capacity, history_capacity) long")


def meter_fold(block, loss, correct, n_rows, batch_rows, guard_state, log_capacity, history_capacity):
    """fold one step into `block`: loss a one-element fp32 device tensor, correct a one-element int64 one, n_rows a
    one-element int32 one or None (then the host integer `batch_rows` counts), guard_state a GradGuard's fp64 block or
    None.  One launch; nothing is read back"""
    _meter_check(block, log_capacity, history_capacity)
    if loss.dtype != torch.float32 or loss.numel() != 1:
        raise ValueError(f"the step loss must be one fp32 element, got {loss.dtype} {tuple(loss.shape)}")
    if correct.dtype != torch.int64 or correct.numel() != 1:
        raise ValueError(f"the correct count must be one int64 element, got {correct.dtype} {tuple(correct.shape)}")
    if n_rows is not None and (n_rows.dtype != torch.int32 or n_rows.numel() != 1):
        raise ValueError("n_rows must be a device int32 tensor of one element")
    if n_rows is None and not 0 <= int(batch_rows) < 2 ** 31:
        raise ValueError(f"batch_rows must be in [0, 2^31) when there is no n_rows word, got {batch_rows}")
    if guard_state is not None and (guard_state.dtype != torch.float64 or guard_state.numel() < 16):
        raise ValueError("guard_state must be a gradient guard's fp64 block")
    call("hwgat_meter_fold", ptr(block), ptr(loss), ptr(correct), ptr(n_rows), 0 if n_rows is not None else int(batch_rows),
         ptr(guard_state), int(log_capacity), stream())


def meter_close(block, log_capacity, history_capacity):
    """close the epoch: the running words go to the next history slot and are zeroed.  One launch"""
    _meter_check(block, log_capacity, history_capacity)
    call("hwgat_meter_close", ptr(block), int(log_capacity), int(history_capacity), stream())


# ---------------------------------------------------------------- the classifier head (csrc/head.hip)
# logits = feat W^T + bias on the project's own kernels: exact fp32, fixed summation order, so a clip's logits have the same
# bits at any batch size.  Opt-in per model (`model.hip_head = True`, seeding.DeviceSeeds._classify).
HEAD_K_STEP, HEAD_K_MAX, HEAD_N_MAX = 64, 1024, 65536


def head_supported(K):
    """the feature widths the head kernels take: every multiple of 64 from 64 to 1024"""
    return HEAD_K_STEP <= int(K) <= HEAD_K_MAX and int(K) % HEAD_K_STEP == 0


def _head_check(rows, weight, what):
    """`rows` is feat (B, K) or the logits' gradient (B, N); returns (B, N, K)"""
    for name, t in ((what, rows), ("weight", weight)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"head: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"head: {name} must be fp32, got {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"head: {name} must be 2-d, got shape {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"head: {name} must be contiguous")
    N, K = weight.shape
    if rows.shape[1] != (K if what == "feat" else N):
        raise ValueError(f"head: {what} {tuple(rows.shape)} does not match weight (N, K) = {tuple(weight.shape)}")
    if rows.shape[0] < 1 or not 1 <= N <= HEAD_N_MAX:
        raise ValueError(f"head: needs at least one row and 1..{HEAD_N_MAX} classes, got {rows.shape[0]} rows, {N} classes")
    if not head_supported(K):
        raise ValueError(f"head: K = {K} features: the kernels take multiples of {HEAD_K_STEP} up to {HEAD_K_MAX}")
    return rows.shape[0], N, K


def _head_out(out, shape, like, name):
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"head: {name} must be a contiguous fp32 {tuple(shape)} tensor")
    return out


def head_forward(feat, weight, bias=None, out=None):
    """feat (B, K) @ weight (N, K)^T + bias (N,) -> (B, N); one launch"""
    B, N, K = _head_check(feat, weight, "feat")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (N,)):
        raise ValueError(f"head: bias must be fp32 ({N},), got {bias.dtype} {tuple(bias.shape)}")
    y = _head_out(out, (B, N), feat, "out")
    call("hwgat_head_fwd", ptr(feat), ptr(weight), ptr(bias), ptr(y), B, N, K, stream())
    return y


def head_backward_dx(dy, weight, out=None):
    """dy (B, N) @ weight (N, K) -> (B, K); one launch"""
    B, N, K = _head_check(dy, weight, "dy")
    dx = _head_out(out, (B, K), dy, "out")
    call("hwgat_head_bwd_dx", ptr(dy), ptr(weight), ptr(dx), B, N, K, stream())
    return dx


def head_backward_dw(dy, feat, want_db=True, out=None, out_db=None):
    """(dy (B, N)^T @ feat (B, K) -> (N, K), the column sums of dy -> (N,) or None); one launch for both"""
    for name, t in (("dy", dy), ("feat", feat)):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"head: {name} must be a contiguous fp32 matrix")
    if dy.shape[0] != feat.shape[0]:
        raise ValueError(f"head: dy {tuple(dy.shape)} and feat {tuple(feat.shape)} differ in rows")
    (B, N), K = dy.shape, feat.shape[1]
    if B < 1 or not 1 <= N <= HEAD_N_MAX or not head_supported(K):
        raise ValueError(f"head: unsupported gradient shape B = {B}, N = {N}, K = {K}")
    dw = _head_out(out, (N, K), dy, "out")
    db = _head_out(out_db, (N,), dy, "out_db") if want_db else None
    call("hwgat_head_bwd_dw", ptr(dy), ptr(feat), ptr(dw), ptr(db), B, N, K, stream())
    return dw, db


class _HeadLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, weight, bias):
        ctx.save_for_backward(feat, weight)
        ctx.has_bias = bias is not None
        return head_forward(feat, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        feat, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = head_backward_dx(dy, weight) if ctx.needs_input_grad[0] else None
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw, db = head_backward_dw(dy, feat, want_db=ctx.has_bias and ctx.needs_input_grad[2])
        return dx, (dw if ctx.needs_input_grad[1] else None), db


def head_linear(feat, weight, bias=None):
    """the classifier head as ONE autograd node: forward one launch (hwgat_head_fwd); backward hwgat_head_bwd_dw for the
    weight and bias gradients together and hwgat_head_bwd_dx only when `feat` needs a gradient.  feat (B, K) fp32
    contiguous on the device, weight (N, K) fp32, bias (N,) fp32 or None; the gradients are fresh contiguous fp32
    tensors that autograd accumulates as it does nn.Linear's."""
    _head_check(feat, weight, "feat")
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (weight.shape[0],)):
        raise ValueError(f"head: bias must be an fp32 ({weight.shape[0]},) tensor or None")
    return _HeadLinear.apply(feat, weight, bias)


# ---------------------------------------------------------------- streaming recognition (csrc/stream.hip, serve.StreamRecognizer)
# The state block is int64 words (layout: include/hwgat_hip.h, "streaming recognition"): a header, one record per stream and
# the event log; serve.py mirrors the records as numpy dtypes.
STREAM_MAX_STREAMS, STREAM_MAX_CLASSES, STREAM_MAX_LOG = 64, 65536, 1 << 20
STREAM_MAX_FRAMES = 4096                       # HWGAT_AUG_MAX_FRAMES: the longest ring
STREAM_HEADER_WORDS, STREAM_WORDS, STREAM_EVENT_WORDS = 8, 8, 4
STREAM_NPRM = 24                               # HWGAT_AUG_NPRM


def stream_state_words(n_streams, log_capacity):
    """size of a recogniser's state block in 8-byte words"""
    n = _lib.lib().hwgat_stream_state_bytes(int(n_streams), int(log_capacity))
    if n < 0:
        raise ValueError(f"no stream state for {n_streams} streams (1..{STREAM_MAX_STREAMS}) and log capacity "
                         f"{log_capacity} (0..{STREAM_MAX_LOG})")
    return n // 8


def _stream_ring(ring, state, log_capacity):
    if ring.dtype != torch.float32 or ring.dim() != 4:
        raise ValueError(f"the ring must be fp32 (streams, ring_frames, J, C), got {ring.dtype} {tuple(ring.shape)}")
    if state.dtype != torch.int64 or state.numel() < stream_state_words(ring.shape[0], log_capacity):
        raise ValueError("the stream state must be int64 and stream_state_words(n_streams, log_capacity) long")
    return tuple(ring.shape)


def stream_push(ring, state, frames, n_new):
    """append clamp(n_new[s], 0, F) frames of frames (S, F, J, C) fp32 to ring s of ring (S, R, J, C), overwriting the oldest;
    n_new (S,) device int32.  One launch; nothing is read back"""
    S, R, J, C = _stream_ring(ring, state, 0)
    if frames.dtype != torch.float32 or frames.dim() != 4 or (frames.shape[0],) + tuple(frames.shape[2:]) != (S, J, C):
        raise ValueError(f"frames must be fp32 ({S}, push_frames, {J}, {C}), got {frames.dtype} {tuple(frames.shape)}")
    if n_new.dtype != torch.int32 or tuple(n_new.shape) != (S,):
        raise ValueError(f"n_new must be a device int32 tensor of {S} elements")
    call("hwgat_stream_push", ptr(ring), ptr(state), ptr(frames), ptr(n_new), S, R, frames.shape[1], J, C, stream())


def stream_window(ring, state, clip, clip_off, src, prm, window_frames, min_frames, origin, anchors, hands):
    """the newest min(count, window_frames) frames of every ring as the packed clip (S * window_frames, J, C), clip_off
    (S + 1) int32, the eval frame map src (S, src_len) int32 and parameter record prm (S, 24) fp64 that hand_fill / resample
    take, and the ready words in `state`.  One launch"""
    S, R, J, C = _stream_ring(ring, state, 0)
    Wf = int(window_frames)
    if clip.dtype != torch.float32 or clip.numel() < S * Wf * J * C:
        raise ValueError(f"the clip buffer must hold fp32 ({S} * {Wf}, {J}, {C})")
    if clip_off.dtype != torch.int32 or clip_off.numel() != S + 1:
        raise ValueError(f"clip_off must be int32 with {S + 1} elements")
    if src.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != S:
        raise ValueError(f"the frame map must be int32 ({S}, src_len)")
    if prm.dtype != torch.float64 or tuple(prm.shape) != (S, STREAM_NPRM):
        raise ValueError(f"the parameter records must be fp64 ({S}, {STREAM_NPRM})")
    if len(anchors) != 2 or len(hands) != 6:
        raise ValueError("two anchor joints and six hand words (l0, l1, lw, r0, r1, rw)")
    hv = (ctypes.c_int32 * 6)(*[int(h) for h in hands])
    call("hwgat_stream_window", ptr(ring), ptr(state), ptr(clip), ptr(clip_off), ptr(src), ptr(prm), S, R, Wf,
         int(min_frames), src.shape[1], J, C, int(origin), int(anchors[0]), int(anchors[1]), hv, stream())


def stream_decide(state, q, logits, log_capacity):
    """softmax, smoothing and the event rule of every ready stream from logits (S, N) fp32; q (S, N) fp32 is the smoothed
    distribution kept between calls.  One launch"""
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError(f"the logits must be fp32 (streams, classes), got {logits.dtype} {tuple(logits.shape)}")
    S, N = logits.shape
    if q.dtype != torch.float32 or tuple(q.shape) != (S, N):
        raise ValueError(f"q must be fp32 {(S, N)}")
    if state.dtype != torch.int64 or state.numel() < stream_state_words(S, log_capacity):
        raise ValueError("the stream state must be int64 and stream_state_words(n_streams, log_capacity) long")
    call("hwgat_stream_decide", ptr(state), ptr(q), ptr(logits), S, N, int(log_capacity), stream())


# ---------------------------------------------------------------- device-resident clip store (csrc/loader.hip, data.DeviceLoader)
# The loader state is hwgat_loader_state of include/hwgat_hip.h: 8 int32 words and 4 spare int64 words, kept as int64 words.
LOADER_STATE_WORDS = 8
LOADER_MAX_BATCH = 1024                        # HWGAT_LOADER_MAX_BATCH
LOADER_SHUFFLE, LOADER_DROP_LAST, LOADER_TRAIN = 1, 2, 4


def _loader_store(state, frames, clip_off):
    if state.dtype != torch.int64 or state.numel() < LOADER_STATE_WORDS:
        raise ValueError(f"the loader state must be int64 with {LOADER_STATE_WORDS} words")
    if frames.dtype != torch.float32 or frames.dim() != 3:
        raise ValueError(f"the store's frames must be fp32 (store_frames, J, C), got {frames.dtype} {tuple(frames.shape)}")
    if clip_off.dtype != torch.int64 or clip_off.dim() != 1 or clip_off.numel() < 2:
        raise ValueError("the store's clip_off must be int64 (n_clips + 1)")
    return clip_off.numel() - 1


def loader_select(state, frames, clip_off, labels, ids, keys, clip_len, batch_off, y, n_rows, max_frames):
    """the next batch's rows from the loader state: ids / keys / clip_len (B) int32, batch_off (B + 1) int32, y (B) int64,
    n_rows (1) int32; moves the cursor (and the epoch) in `state`.  One launch; nothing is read back"""
    n = _loader_store(state, frames, clip_off)
    B = ids.numel()
    if labels.dtype != torch.int64 or labels.numel() != n:
        raise ValueError(f"labels must be int64 with {n} elements")
    for name, t in (("ids", ids), ("keys", keys), ("clip_len", clip_len)):
        if t.dtype != torch.int32 or t.numel() != B:
            raise ValueError(f"{name} must be int32 with {B} elements")
    if batch_off.dtype != torch.int32 or batch_off.numel() != B + 1:
        raise ValueError(f"batch_off must be int32 with {B + 1} elements")
    if y.dtype != torch.int64 or y.numel() != B:
        raise ValueError(f"y must be int64 with {B} elements")
    if n_rows.dtype != torch.int32 or n_rows.numel() != 1:
        raise ValueError("n_rows must be one int32 word")
    call("hwgat_loader_select", ptr(state), ptr(clip_off), ptr(labels), ptr(ids), ptr(keys), ptr(clip_len), ptr(batch_off),
         ptr(y), ptr(n_rows), n, frames.shape[0], B, int(max_frames), stream())


def loader_draw(state, frames, clip_off, norm, ids, keys, batch_off, clip, masked, src, prm, max_frames, mask_p, ratio,
                shear_std, rotation_std, random_sample, random_shift):
    """the selected rows' raw frames into the packed clip (B * max_frames, J, C), the masked bytes (B * max_frames) uint8,
    the frame map src (B, src_len) int32 and the parameter records prm (B, 24) fp64 that hand_fill / resample take.  One
    launch"""
    n = _loader_store(state, frames, clip_off)
    B, (_, J, C) = ids.numel(), frames.shape
    if norm.dtype != torch.float32 or tuple(norm.shape) != (n, 4):
        raise ValueError(f"norm must be fp32 ({n}, 4)")
    if clip.dtype != torch.float32 or clip.numel() < B * int(max_frames) * J * C:
        raise ValueError(f"the clip buffer must hold fp32 ({B} * {max_frames}, {J}, {C})")
    if masked.dtype != torch.uint8 or masked.numel() < B * int(max_frames):
        raise ValueError(f"the masked bytes must be uint8 with {B} * {max_frames} elements")
    if src.dtype != torch.int32 or src.dim() != 2 or src.shape[0] != B:
        raise ValueError(f"the frame map must be int32 ({B}, src_len)")
    if prm.dtype != torch.float64 or tuple(prm.shape) != (B, STREAM_NPRM):
        raise ValueError(f"the parameter records must be fp64 ({B}, {STREAM_NPRM})")
    if keys.dtype != torch.int32 or keys.numel() != B or batch_off.dtype != torch.int32 or batch_off.numel() != B + 1:
        raise ValueError(f"keys must be int32 ({B}) and batch_off int32 ({B + 1})")
    call("hwgat_loader_draw", ptr(state), ptr(frames), ptr(clip_off), ptr(norm), ptr(ids), ptr(keys), ptr(batch_off),
         ptr(clip), ptr(masked), ptr(src), ptr(prm), n, frames.shape[0], B, int(max_frames), src.shape[1], J, C,
         float(mask_p), float(ratio[0]), float(ratio[1]), float(shear_std), float(rotation_std), int(bool(random_sample)),
         int(bool(random_shift)), stream())


# ---------------------------------------------------------------- Mixup / temporal CutMix (csrc/mix.hip, train.BatchMixer)
# The mixer state is hwgat_mix_state of include/hwgat_hip.h kept as int64 words: word 0 holds seed (low half) and step (high
# half), words 1..4 the fp64 hyper words prob, cutmix_share, mixup_alpha, cutmix_alpha.
MIX_STATE_WORDS = 5
MIX_MAX_BATCH, MIX_ALPHA_MIN = 65536, 0.05     # HWGAT_MIX_MAX_BATCH, HWGAT_MIX_ALPHA_MIN
MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2


def mix_state(device):
    """a zeroed mixer state block on `device` (write it with mix_set before the first draw)"""
    if 8 * MIX_STATE_WORDS != _lib.lib().hwgat_mix_state_bytes():
        raise RuntimeError("the library lays the mixer state out differently from functional.py's constants")
    return torch.zeros(MIX_STATE_WORDS, dtype=torch.int64, device=device)


def _mix_state_check(state):
    if state.dtype != torch.int64 or state.numel() < MIX_STATE_WORDS:
        raise ValueError(f"the mixer state must be int64 with {MIX_STATE_WORDS} words")


def mix_set(state, prob, cutmix_share, mixup_alpha, cutmix_alpha, seed=None, step=0):
    """write the four hyper words and, with a `seed`, the seed and the step counter.  One tiny launch, stream-ordered"""
    _mix_state_check(state)
    if seed is not None and not (0 <= int(seed) < 2 ** 32 and 0 <= int(step) < 2 ** 32):
        raise ValueError(f"seed and step must be in [0, 2^32), got {seed}, {step}")
    call("hwgat_mix_set", ptr(state), float(prob), float(cutmix_share), float(mixup_alpha), float(cutmix_alpha),
         int(seed is not None), 0 if seed is None else int(seed), int(step) if seed is not None else 0, stream())


def _mix_records(B, pairs, partner, lam, seg, mode):
    for name, t, dt, n in (("pairs", pairs, torch.int32, 2 * max(B // 2, 1)), ("partner", partner, torch.int32, B),
                           ("lam", lam, torch.float32, B), ("seg", seg, torch.int32, 2 * B), ("mode", mode, torch.int32, B)):
        if t is not None and (t.dtype != dt or t.numel() != n):
            raise ValueError(f"{name} must be {dt} with {n} elements for a batch of {B}")


def mix_draw(state, y, n_rows, pairs, partner, lam, seg, mode, y_b, T):
    """one step's matching and decisions from the mixer state: pairs (max(B // 2, 1), 2), partner (B), seg (B, 2), mode (B)
    int32, lam (B) fp32, y_b (B) int64 = y[partner]; `n_rows` a device int32 word or None (all B rows are live); advances
    the state's step counter.  One launch; nothing is read back"""
    _mix_state_check(state)
    B = y.numel()
    if y.dtype != torch.int64 or y_b.dtype != torch.int64 or y_b.numel() != B:
        raise ValueError(f"y and y_b must be int64 with {B} elements")
    if n_rows is not None and (n_rows.dtype != torch.int32 or n_rows.numel() != 1):
        raise ValueError("n_rows must be a device int32 tensor of one element")
    _mix_records(B, pairs, partner, lam, seg, mode)
    call("hwgat_mix_draw", ptr(state), ptr(y), ptr(n_rows), ptr(pairs), ptr(partner), ptr(lam), ptr(seg), ptr(mode), ptr(y_b),
         B, int(T), stream())


def mix_apply(x, pairs, lam, seg, mode, n_rows=None):
    """mix the rows of x (B, T, ...) fp32 in place as the records of mix_draw say.  One launch (none for B == 1)"""
    if x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError(f"x must be fp32 (B, T, ...), got {x.dtype} {tuple(x.shape)}")
    B, T = x.shape[:2]
    _mix_records(B, pairs, None, lam, seg, mode)
    if n_rows is not None and (n_rows.dtype != torch.int32 or n_rows.numel() != 1):
        raise ValueError("n_rows must be a device int32 tensor of one element")
    call("hwgat_mix_apply", ptr(x), ptr(pairs), ptr(lam), ptr(seg), ptr(mode), ptr(n_rows), B, T, x[0, 0].numel(), stream())


# ---------------------------------------------------------------- knowledge distillation (csrc/loss_eval.hip, train.Distiller)
# The slice criterion with a teacher's logits beside the labels.  The state is two device floats, alpha and tau.
KD_STATE_WORDS = 2
KD_TAU_MIN, KD_TAU_MAX = 0.25, 32.0            # HWGAT_KD_TAU_MIN, HWGAT_KD_TAU_MAX


def kd_state(device):
    """a zeroed distillation state on `device` (write it with kd_set before the first forward)"""
    if 4 * KD_STATE_WORDS != _lib.lib().hwgat_kd_state_bytes():
        raise RuntimeError("the library lays the distillation state out differently from functional.py's constants")
    return torch.zeros(KD_STATE_WORDS, dtype=torch.float32, device=device)


def _kd_state_check(state):
    if state.dtype != torch.float32 or state.numel() != KD_STATE_WORDS:
        raise ValueError(f"the distillation state must be fp32 with {KD_STATE_WORDS} words")


def kd_set(state, alpha, tau):
    """write alpha and tau.  One tiny launch, stream-ordered"""
    _kd_state_check(state)
    call("hwgat_kd_set", ptr(state), float(alpha), float(tau), stream())


# ---------------------------------------------------------------- input modalities (csrc/modality.hip, modality.Modality)
MOD_KINDS = ("joint", "bone", "motion", "bone_motion")          # HWGAT_MOD_*: the position is the code


def _overlap(a, b):
    """two contiguous tensors share memory"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def modality(x, parent, kind, pad_value=None, out=None):
    """the `kind` view (a name of MOD_KINDS or its code) of the keypoints x (B, T, J, C) fp32: joints, bones over the device
    int32 table `parent` (J,), joint motion or bone motion; `pad_value` marks padded frames by their first word (None: no
    padding).  x is left alone; returns a new tensor, or `out`.  One launch"""
    code = MOD_KINDS.index(kind) if kind in MOD_KINDS else kind
    if isinstance(code, bool) or not isinstance(code, int) or not 0 <= code < len(MOD_KINDS):
        raise ValueError(f"modality: kind must be one of {MOD_KINDS} (or 0..3), got {kind!r}")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"modality: x must be an fp32 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"modality: x must be a non-empty (B, T, J, C) tensor, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("modality: x must be contiguous")
    B, T, J, C = x.shape
    if code in (1, 3):
        if parent is None:
            raise ValueError(f"modality: kind {MOD_KINDS[code]!r} needs the parent table")
        if parent.dtype != torch.int32 or tuple(parent.shape) != (J,):
            raise ValueError(f"modality: parent must be a device int32 tensor of {J} elements, got {parent.dtype} "
                             f"{tuple(parent.shape)}")
    else:
        parent = None
    if out is None:
        ptr(x)                                                    # refuses a CPU or strided x before anything is allocated
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
        raise ValueError(f"modality: out must be a contiguous fp32 {tuple(x.shape)} tensor")
    elif _overlap(x, out):
        raise ValueError("modality: out must not alias x (a frame's neighbours are read after stores)")
    call("hwgat_modality", ptr(x), ptr(parent), ptr(out), B, T, J, C, code, int(pad_value is not None),
         0.0 if pad_value is None else float(pad_value), stream())
    return out


# ---------------------------------------------------------------- score ensemble (csrc/ensemble.hip, ensemble.Ensemble)
ENS_MAX_MEMBERS = 8                                              # HWGAT_ENS_MAX_MEMBERS
ENS_MODES = ("logit", "prob")                                    # HWGAT_ENS_LOGIT, HWGAT_ENS_PROB


def ens_fuse(z, w, mode, out=None):
    """the fused score (B, C) of member logits z (M, B, C) fp32 under the device weights w (M,) fp32: mode 'logit' the
    weighted sum of the logits, 'prob' the log of the weighted mean of the softmaxes.  One launch"""
    if mode not in ENS_MODES:
        raise ValueError(f"ens_fuse: mode must be one of {ENS_MODES}, got {mode!r}")
    for name, t in (("z", z), ("w", w)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"ens_fuse: {name} must be an fp32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if z.dim() != 3 or z.numel() == 0:
        raise ValueError(f"ens_fuse: z must be a non-empty (M, B, C) tensor, got {tuple(z.shape)}")
    if not z.is_contiguous() or not w.is_contiguous():
        raise ValueError("ens_fuse: z and w must be contiguous")
    M, B, C = z.shape
    if not 1 <= M <= ENS_MAX_MEMBERS:
        raise ValueError(f"ens_fuse: 1 to {ENS_MAX_MEMBERS} members, got {M}")
    if tuple(w.shape) != (M,):
        raise ValueError(f"ens_fuse: w must hold {M} weights, got {tuple(w.shape)}")
    if out is None:
        ptr(z)
        out = torch.empty((B, C), device=z.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, C) or not out.is_contiguous():
        raise ValueError(f"ens_fuse: out must be a contiguous fp32 {(B, C)} tensor")
    elif _overlap(z, out):
        raise ValueError("ens_fuse: out must not alias z")
    call("hwgat_ens_fuse", ptr(z), ptr(w), ptr(out), M, B, C, ENS_MODES.index(mode), stream())
    return out
