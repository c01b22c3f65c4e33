"""Host restatement (numpy only) of hwgat_loader_select and hwgat_loader_draw, written from the comment of
include/hwgat_hip.h ("device-resident clip store and train input pipeline"): the Feistel permutation with cycle walking, the
keys, the tagged hashes, the Box-Muller normals, the record and the frame map.  `mix32` is the restated dropout hash of
tests/mask_helpers.py.  Nothing here calls into the library.

The integers a row's floating-point draws decide -- L = int(T * ratio) and start = int((src_len - L) * s) -- are checked to lie
more than 1e-9 from a rounding boundary (`draw_row` asserts it for every row it restates): a difference between a device
integer and this file is then a bug and not an ulp of a libm."""
import numpy as np

from mask_helpers import mix32

TAG_MASK, TAG_SHEAR_ORIGIN, TAG_SHEAR, TAG_ROT_ORIGIN, TAG_ROT = 0x10, 0x20, 0x30, 0x40, 0x50
TAG_RATIO, TAG_MODE, TAG_SUBSET, TAG_CHOICE, TAG_SHIFT, TAG_FLIP = 0x60, 0x70, 0x80, 0x90, 0xA0, 0xB0
NPRM, MAX_FRAMES = 24, 4096
TWO_PI, DEG2RAD = 6.283185307179586, 0.017453292519943295
MARGIN = 1e-9


def feistel_bits(n):
    b = 2
    while (1 << b) < n:
        b += 2
    return b


def feistel(K, n, x):
    """four balanced rounds on feistel_bits(n) bits; x: uint64 array"""
    h = feistel_bits(n) // 2
    m = np.uint64((1 << h) - 1)
    L, R = x >> np.uint64(h), x & m
    for j in range(4):
        L, R = R, L ^ (mix32((int(K) + j) & 0xFFFFFFFF, R).astype(np.uint64) & m)
    return (L << np.uint64(h)) | R


def perm(K, n, x):
    """the keyed bijection of [0, n) at the points x (array of values < n)"""
    x = np.asarray(x, dtype=np.uint64).copy()
    if n <= 1:
        return np.zeros(x.shape, dtype=np.int64)
    y = feistel(K, n, x)
    for _ in range((1 << feistel_bits(n)) - n + 1):
        out = y >= np.uint64(n)
        if not out.any():
            return y.astype(np.int64)
        y[out] = feistel(K, n, y[out])
    raise AssertionError("the walk bound was reached: the round function is no bijection")


def k_perm(seed, epoch):
    return int(mix32(seed, epoch))


def k_row(seed, epoch, ids):
    """the draw key of clip `ids` (scalar or array) in `epoch`"""
    return mix32(int(mix32(seed, (1 << 32) + epoch)), np.asarray(ids, dtype=np.uint64))


def _hash(key, tag, i):
    return mix32((int(key) + tag) & 0xFFFFFFFF, np.asarray(i, dtype=np.uint64))


def uniform(key, tag, i):
    return (_hash(key, tag, i).astype(np.float64) + 0.5) / 4294967296.0


def normal_z(key, tag, i):
    i = np.asarray(i, dtype=np.uint64)
    u1, u2 = uniform(key, tag, 2 * i), uniform(key, tag, 2 * i + 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def normal(loc, scale, key, tag, i):
    return loc + scale * normal_z(key, tag, i)


def clip01(v):
    return np.minimum(np.maximum(v, 0.0), 1.0)


def linspace_int(last, n):
    """numpy.linspace(0, last, n).astype(int), from the header's formula"""
    if n <= 1 or last <= 0:
        return np.zeros(max(n, 0), dtype=np.int64)
    step = np.float64(last) / np.float64(n - 1)
    out = (np.arange(n, dtype=np.float64) * step).astype(np.int64)
    out[-1] = last
    return np.minimum(out, last)


def batches_per_epoch(n_clips, B, world=1, drop_last=False):
    per = n_clips // world if drop_last else -(-n_clips // world)
    nb0 = per // B if drop_last else -(-per // B)
    return nb0, max(nb0, 1)


def select(seed, epoch, cursor, lengths, labels, B, rank=0, world=1, shuffle=True, drop_last=False):
    """one hwgat_loader_select: (dict of the written arrays, (epoch, cursor) afterwards)"""
    n = len(lengths)
    nb0, nb = batches_per_epoch(n, B, world, drop_last)
    limit = nb0 * B * world if drop_last else n
    cursor %= nb
    r = np.arange(B, dtype=np.int64)
    s = (cursor * B + r) * world + rank
    valid = s < limit
    ids = np.full(B, -1, dtype=np.int64)
    if valid.any():
        ids[valid] = perm(k_perm(seed, epoch), n, s[valid]) if shuffle else s[valid]
    keys = np.zeros(B, dtype=np.uint32)
    keys[valid] = k_row(seed, epoch, ids[valid])
    clip_len = np.where(valid, np.asarray(lengths)[np.maximum(ids, 0)], 0).astype(np.int32)
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(clip_len, out=off[1:])
    y = np.where(valid, np.asarray(labels)[np.maximum(ids, 0)], 0).astype(np.int64)
    nxt = (epoch + 1, 0) if cursor + 1 >= nb else (epoch, cursor + 1)
    return dict(ids=ids.astype(np.int32), keys=keys, clip_len=clip_len, batch_off=off, y=y, n_rows=int(valid.sum())), nxt


def rotation(key, C, rotation_std):
    m = np.eye(3)
    if C == 2:
        a = normal(0.0, rotation_std, key, TAG_ROT, 0)
        cs, sn = np.cos(a), np.sin(a)
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = cs, -sn, sn, cs
        return m, float(a)
    t = normal(0.0, rotation_std, key, TAG_ROT, np.arange(3)) * 90.0 * DEG2RAD
    (c0, c1, c2), (s0, s1, s2) = np.cos(t), np.sin(t)
    m[:] = [[c2 * c1, c2 * s1 * s0 - s2 * c0, c2 * s1 * c0 + s2 * s0],
            [s2 * c1, s2 * s1 * s0 + c2 * c0, s2 * s1 * c0 - c2 * s0],
            [-s1, c1 * s0, c1 * c0]]
    return m, t


def _far_from_integer(v, what):
    assert abs(v - np.round(v)) > MARGIN, f"{what} = {v!r} lies within {MARGIN} of an integer: choose another seed"


def draw_row(key, T, norm, C, src_len, train=True, sampling_prob=0.2, frame_augmentation=(0.5, 1.5), shear_std=0.1,
             rotation_std=0.1, random_sample=True, random_shift=True):
    """one row of hwgat_loader_draw: dict(masked sorted frames, prm (24,), src (src_len,), and what path the row took:
    mode in {"empty", "eval", "subset", "choice", "linspace"}, L, pad, flip)"""
    n = src_len
    prm = np.zeros(NPRM)
    prm[3] = 1.0
    prm[[11, 15, 19]] = 1.0
    if T <= 0:
        return dict(masked=np.zeros(0, dtype=np.int64), prm=prm, src=np.zeros(n, dtype=np.int32), mode="empty", L=0,
                    pad=False, flip=False, start=None)
    key = int(key)
    prm[:C] = np.asarray(norm[:C], dtype=np.float64)
    prm[3] = np.float64(norm[3])
    frames = np.arange(T)
    if not train:
        L, mode, masked, aug, flip, s = T, "eval", np.zeros(0, dtype=np.int64), frames, False, 0.5
    else:
        masked = frames[perm(key + TAG_MASK, T, frames) < int(sampling_prob * T)]
        prm[4:4 + C] = clip01(normal(0.5, 0.1, key, TAG_SHEAR_ORIGIN, np.arange(C)))
        prm[7] = normal(0.0, shear_std, key, TAG_SHEAR, 0)
        prm[8:8 + C] = clip01(normal(0.5, 0.1, key, TAG_ROT_ORIGIN, np.arange(C)))
        prm[11:20] = rotation(key, C, rotation_std)[0].reshape(-1)
        flip = int(_hash(key, TAG_FLIP, 0)) < 1 << 31
        prm[20] = 1.0 if flip else 0.0
        lo, hi = frame_augmentation
        ratio = np.float64(hi - lo) * uniform(key, TAG_RATIO, 0) + np.float64(lo)
        _far_from_integer(T * ratio, "T * ratio")
        L = min(max(int(T * ratio), 1), 2 * MAX_FRAMES)
        if random_sample and int(_hash(key, TAG_MODE, 0)) < 1 << 31:
            if ratio <= 1:
                mode, aug = "subset", frames[perm(key + TAG_SUBSET, T, frames) < L]
            else:
                h = _hash(key, TAG_CHOICE, np.arange(L)).astype(np.uint64)
                mode, aug = "choice", np.sort((h * np.uint64(T)) >> np.uint64(32)).astype(np.int64)
        else:
            mode, aug = "linspace", linspace_int(T - 1, L)
        assert len(aug) == L
        s = float(clip01(normal(0.5, 0.1, key, TAG_SHIFT, 0))) if random_shift else 0.5
    pad, start = L <= n, None
    if pad:
        if n - L > 0 and 0.0 < s < 1.0:
            _far_from_integer((n - L) * s, "(src_len - L) * s")
        start = int((n - L) * s)
        t = np.arange(n)
        m = np.where((t >= start) & (t < start + L), t - start, np.where(t < n // 2, 0, L - 1))
    else:
        m = linspace_int(L - 1, n)
    prm[21] = 1.0 if pad else 0.0
    return dict(masked=masked.astype(np.int64), prm=prm, src=np.asarray(aug)[m].astype(np.int32), mode=mode, L=L, pad=pad,
                flip=bool(flip), start=start)


def draw_batch(sel, lengths, norm, C, src_len, train=True, **dist):
    """hwgat_loader_draw for the rows `select` returned: list of draw_row dicts"""
    return [draw_row(sel["keys"][r], int(sel["clip_len"][r]), norm[max(int(sel["ids"][r]), 0)], C, src_len, train, **dist)
            for r in range(len(sel["ids"]))]


def dist_of(transform):
    """the keyword arguments of draw_row from an augment.TrainTransform"""
    return dict(sampling_prob=transform.sampling_prob, frame_augmentation=transform.frame_augmentation,
                shear_std=transform.shear_std, rotation_std=transform.rotation_std,
                random_sample=transform.random_sample, random_shift=transform.random_shift)


# ---------------------------------------------------------------------------------------------- the tests' small dataset
N_CLIPS, JOINTS = 37, 29
LENGTHS = [5 + (i * 43) // 35 for i in range(36)] + [96]      # 5 .. 48 and one long clip


def make_clips(C, seed=7):
    """37 raw clips (T, 29, C) float32 with arbitrary (not dyadic) values: hand frames absent on a pattern, so that the
    spline fill runs, and some frames with a zero origin joint, so that the normalisation takes a later frame"""
    rng = np.random.RandomState(seed + C)
    clips, labels = [], []
    for i, T in enumerate(LENGTHS):
        c = (rng.rand(T, JOINTS, C) * 0.8 + 0.1).astype(np.float32)
        f = np.arange(T)
        c[(f + i) % 5 == 2, 9:19] = 0.0                       # left hand absent
        c[np.isin((f + 2 * i) % 7, (3, 4)), 19:29] = 0.0      # right hand absent
        if i % 3 == 0:
            c[0, 0] = 0.0                                     # the first frame cannot normalise the clip
        if i % 6 == 1 and T > 8:
            c[:2, 3] = 0.0                                    # nor can the first two (an anchor is missing)
        clips.append(c)
        labels.append((i * 5 + 3) % 7)
    return clips, np.asarray(labels, dtype=np.int64)
