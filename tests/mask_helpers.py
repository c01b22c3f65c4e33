"""Host restatement of the dropout hash (numpy only), written from the comment and the formulas of csrc/fused_ops.h:

  one 32-bit hash serves an aligned PAIR of elements: h = mix32(seed + seed_base, idx >> 1), the even element takes the
  low 16 bits, the odd one the high 16; an element is kept iff its 16 bits >= thresh(p); survivors carry 1 / (1 - p).

All integer arithmetic wraps at 32 bits; thresh and the scale are evaluated in float32 as on the device.  Nothing here
calls into the library: tests/test_mask_hash_cpu.py pins these functions to vectors worked out by hand, and the GPU tests
hold hwgat_dropout_mask_f32 and the kernels with a fused mask to them."""
import numpy as np

C1, C2, M1, M2 = 0x9E3779B1, 0x85EBCA77, 0x2C1B3C6D, 0x297A2D39
_U32 = np.uint64(0xFFFFFFFF)


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


def mix32(seed, pair):
    """uint32 hash of (32-bit seed, 64-bit pair index); scalars or arrays"""
    seed, pair = _u64(seed) & _U32, _u64(pair)
    lo, hi = pair & _U32, pair >> np.uint64(32)
    # every product of two values below 2^32 fits 64 bits, so masking after each step is the 32-bit wrap
    x = (((lo ^ seed) * np.uint64(C1)) & _U32) + ((hi * np.uint64(C2)) & _U32)
    x &= _U32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(M1)) & _U32
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(M2)) & _U32
    return (x ^ (x >> np.uint64(15))).astype(np.uint32)


def thresh(p):
    """p <= 0 ? 0 : (uint32) min(p * 65536 + 0.5, 65535), every step in float32"""
    p = np.float32(p)
    if p <= np.float32(0):
        return 0
    t = np.float32(p * np.float32(65536.0))
    t = np.float32(t + np.float32(0.5))
    return int(min(t, np.float32(65535.0)))


def scale(p):
    """float32(1) / (float32(1) - float32(p))"""
    return np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(p))


def keep_bits(n, seed, p, seed_base=0, start=0):
    """bool (n,): element start + i survives"""
    th = thresh(p)
    if th == 0:
        return np.ones(n, dtype=bool)
    sd = (int(seed) + int(seed_base)) & 0xFFFFFFFF
    idx = np.arange(start, start + n, dtype=np.uint64)
    h = mix32(sd, idx >> np.uint64(1)).astype(np.uint32)
    half = np.where((idx & np.uint64(1)).astype(bool), h >> np.uint32(16), h & np.uint32(0xFFFF))
    return half >= np.uint32(th)


def keep_mask(shape, seed, p, seed_base=0):
    """float32 array of `shape`: 1 / (1 - p) where the element (row-major flat index) survives, else 0"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64))
    out = np.where(keep_bits(n, seed, p, seed_base), scale(p), np.float32(0.0)).astype(np.float32)
    return out.reshape(shape)
