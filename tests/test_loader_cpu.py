"""CPU: the host side of the device-resident clip store and loader (csrc/loader.hip, data.DeviceClipStore / DeviceLoader) --
the entry points in the header, the binding and the library, their argument checks before any HIP call, the numpy
restatement of select and draw (tests/loader_helpers.py: the permutation, the rank split, the masked frames, the frame map,
the paths the GPU tests' seed reaches), its distributions against the project's replay of the reference
(augment.TrainTransform.draw), and what the store and the loader refuse before they look at a device."""
import ctypes
import importlib
import random
import re

import numpy as np
import pytest
import torch

import loader_helpers as LH

hw = importlib.import_module("sl-hwgat_amd")
data, augment, HF = hw.data, hw.augment, hw.functional
LOADER_SYMBOLS = {"hwgat_loader_state_bytes", "hwgat_loader_select", "hwgat_loader_draw"}
EINVAL, ESHAPE = -1, -2
SEED = 1234                                                   # the GPU tests' loader seed


def _buf():
    """aligned host memory standing in for a device pointer: never dereferenced, every call below is refused first"""
    keep = (ctypes.c_double * 64)()
    return keep, ctypes.cast(keep, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ header, binding, library
def test_symbols_abi_and_state_record_follow_the_header():
    assert LOADER_SYMBOLS <= set(hw._lib.declared_symbols())
    assert LOADER_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_loader_")}
    L = hw._lib.lib()
    for name in LOADER_SYMBOLS:
        assert getattr(L, name) is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007
    assert L.hwgat_loader_state_bytes() == 64 == data.LOADER_STATE.itemsize == 8 * HF.LOADER_STATE_WORDS
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    assert int(re.search(r"#define\s+HWGAT_LOADER_MAX_BATCH\s+(\d+)", src).group(1)) == HF.LOADER_MAX_BATCH
    for name, want in (("SHUFFLE", HF.LOADER_SHUFFLE), ("DROP_LAST", HF.LOADER_DROP_LAST), ("TRAIN", HF.LOADER_TRAIN)):
        assert int(re.search(r"#define\s+HWGAT_LOADER_" + name + r"\s+(\d+)", src).group(1)) == want
    for name in ("MASK", "SHEAR_ORIGIN", "SHEAR", "ROT_ORIGIN", "ROT", "RATIO", "MODE", "SUBSET", "CHOICE", "SHIFT", "FLIP"):
        got = int(re.search(r"#define\s+HWGAT_LOADER_TAG_" + name + r"\s+(0x[0-9A-Fa-f]+)", src).group(1), 16)
        assert got == getattr(LH, "TAG_" + name), name
    # the numpy record names the fields of the C record, in order
    body = re.search(r"typedef struct \{([^{}]*)\} hwgat_loader_state;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"uint32_t": "<u4", "int32_t": "<i4", "int64_t": "<i8"}
    fields = []
    for typ, names in re.findall(r"(uint32_t|int32_t|int64_t)\s+([^;]+);", body):
        for name in names.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name.strip())
            fields.append((m.group(1), ctype[typ]) + (((int(m.group(2)),),) if m.group(2) else ()))
    assert np.dtype(fields) == data.LOADER_STATE
    assert hw.data is data and "data" in hw.__all__


def test_entry_points_check_their_arguments_without_launching():
    L = hw._lib.lib()
    keep, buf = _buf()
    odd = ctypes.c_void_p(buf.value + 4)
    select, draw = L.hwgat_loader_select, L.hwgat_loader_draw
    # (state, clip_off, labels, ids, keys, clip_len, batch_off, y, n_rows, n_clips, store_frames, batch, max_frames, stream)
    good = [buf] * 9 + [37, 1000, 8, 96, None]
    for i in range(9):
        assert select(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i in (0, 1, 2, 7):                                    # 8-byte words
        assert select(*(good[:i] + [odd] + good[i + 1:])) == EINVAL, i
    for i, bad, rc in ((9, 0, EINVAL), (9, -3, EINVAL), (9, (1 << 30) + 1, ESHAPE), (10, 0, EINVAL), (10, 36, ESHAPE),
                       (11, 0, EINVAL), (11, 1025, ESHAPE), (12, 0, EINVAL), (12, 4097, ESHAPE)):
        assert select(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    # (state, frames, clip_off, norm, ids, keys, batch_off, clip, masked, src, prm, n_clips, store_frames, batch, max_frames,
    #  src_len, J, C, mask_p, ratio_lo, ratio_hi, shear_std, rotation_std, random_sample, random_shift, stream)
    good = [buf] * 11 + [37, 1000, 8, 96, 16, 29, 2, 0.2, 0.5, 1.5, 0.1, 0.1, 1, 1, None]
    for i in range(11):
        assert draw(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i in (0, 2, 10):
        assert draw(*(good[:i] + [odd] + good[i + 1:])) == EINVAL, i
    nan = float("nan")
    for i, bad, rc in ((11, 0, EINVAL), (12, 0, EINVAL), (12, 36, ESHAPE), (13, 0, EINVAL), (13, 1025, ESHAPE),
                       (14, 0, EINVAL), (14, 4097, ESHAPE), (15, 0, EINVAL), (15, (1 << 20) + 1, ESHAPE), (16, 0, EINVAL),
                       (16, 1025, ESHAPE), (17, 1, ESHAPE), (17, 4, ESHAPE), (18, 0.0, ESHAPE), (18, 1.0, ESHAPE),
                       (18, nan, ESHAPE), (19, 0.0, ESHAPE), (19, 1.6, ESHAPE), (20, 2.5, ESHAPE), (20, nan, ESHAPE),
                       (21, -0.1, ESHAPE), (21, nan, ESHAPE), (22, -1.0, ESHAPE), (22, float("inf"), ESHAPE)):
        assert draw(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    del keep


def test_wrappers_refuse_cpu_tensors_and_wrong_buffers():
    n, B, Tm, J, C = 5, 4, 12, 29, 2
    state = torch.zeros(8, dtype=torch.int64)
    frames, off = torch.zeros(40, J, C), torch.zeros(n + 1, dtype=torch.int64)
    labels, norm = torch.zeros(n, dtype=torch.int64), torch.zeros(n, 4)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    ids, keys, clen, boff, y, nrows = i32(B), i32(B), i32(B), i32(B + 1), torch.zeros(B, dtype=torch.int64), i32(1)
    clip, masked = torch.zeros(B * Tm, J, C), torch.zeros(B * Tm, dtype=torch.uint8)
    src, prm = i32(B, 16), torch.zeros(B, 24, dtype=torch.float64)
    sel = lambda **kw: HF.loader_select(**{**dict(state=state, frames=frames, clip_off=off, labels=labels, ids=ids, keys=keys,
                                                  clip_len=clen, batch_off=boff, y=y, n_rows=nrows, max_frames=Tm), **kw})
    drw = lambda **kw: HF.loader_draw(**{**dict(state=state, frames=frames, clip_off=off, norm=norm, ids=ids, keys=keys,
                                                batch_off=boff, clip=clip, masked=masked, src=src, prm=prm, max_frames=Tm,
                                                mask_p=0.2, ratio=(0.5, 1.5), shear_std=0.1, rotation_std=0.1,
                                                random_sample=True, random_shift=True), **kw})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sel()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        drw()
    for kw, msg in ((dict(state=state[:4]), "loader state"), (dict(frames=frames.double()), "frames"),
                    (dict(clip_off=off.int()), "clip_off"), (dict(labels=labels[:3]), "labels"), (dict(keys=keys.long()), "keys"),
                    (dict(batch_off=boff[:B]), "batch_off"), (dict(y=y.int()), "y must"), (dict(n_rows=i32(2)), "n_rows")):
        with pytest.raises(ValueError, match=msg):
            sel(**kw)
    for kw, msg in ((dict(norm=norm[:, :3]), "norm"), (dict(clip=clip[:10]), "clip buffer"), (dict(masked=masked[:5]), "masked"),
                    (dict(src=src.long()), "frame map"), (dict(prm=prm.float()), "parameter records"),
                    (dict(keys=keys[:2]), "keys")):
        with pytest.raises(ValueError, match=msg):
            drw(**kw)


# ------------------------------------------------------------------------------------------ the restatement: select
@pytest.mark.parametrize("n", [1, 2, 3, 37, 64, 1000])
def test_restated_perm_is_a_keyed_bijection(n):
    x = np.arange(n)
    p00 = LH.perm(LH.k_perm(SEED, 0), n, x)
    assert sorted(p00.tolist()) == list(range(n))
    assert np.array_equal(p00, LH.perm(LH.k_perm(SEED, 0), n, x))            # the same (seed, epoch): the same order
    if n >= 37:                                                              # 3! orders or fewer can coincide by chance
        assert not np.array_equal(p00, LH.perm(LH.k_perm(SEED, 1), n, x))
        assert not np.array_equal(p00, LH.perm(LH.k_perm(SEED + 1, 0), n, x))
    assert (1 << LH.feistel_bits(n)) < 4 * n or n == 1                       # the expected walk is below 4 steps
    assert LH.feistel_bits(n) % 2 == 0 and (1 << LH.feistel_bits(n)) >= n


def test_restated_epoch_covers_every_clip_once_and_ranks_split_it():
    lengths, labels = np.asarray(LH.LENGTHS), np.arange(37) % 7
    for shuffle in (False, True):
        seen, state = [], (0, 0)
        for _ in range(LH.batches_per_epoch(37, 8)[1]):
            sel, state = LH.select(SEED, state[0], state[1], lengths, labels, 8, shuffle=shuffle)
            k = sel["n_rows"]
            assert (sel["ids"][:k] >= 0).all() and (sel["ids"][k:] == -1).all() and (sel["clip_len"][k:] == 0).all()
            assert np.array_equal(sel["y"][:k], labels[sel["ids"][:k]]) and (sel["y"][k:] == 0).all()
            assert np.array_equal(np.diff(sel["batch_off"]), sel["clip_len"])
            seen += sel["ids"][:k].tolist()
        assert state == (1, 0) and sorted(seen) == list(range(37))
        assert (seen == list(range(37))) == (not shuffle)
    parts = []
    for rank in (0, 1):
        got, state = [], (0, 0)
        for _ in range(LH.batches_per_epoch(37, 8, world=2)[1]):
            sel, state = LH.select(SEED, state[0], state[1], lengths, labels, 8, rank=rank, world=2)
            got += sel["ids"][:sel["n_rows"]].tolist()
        assert state == (1, 0)
        parts.append(got)
    assert not set(parts[0]) & set(parts[1]) and sorted(parts[0] + parts[1]) == list(range(37))
    # drop_last: full batches only, the same count on every rank
    sel, state = LH.select(SEED, 0, 3, lengths, labels, 8, drop_last=True)
    assert sel["n_rows"] == 8 and state == (1, 0) and LH.batches_per_epoch(37, 8, drop_last=True) == (4, 4)
    # the draw key depends on (seed, epoch, clip) only
    assert np.array_equal(LH.k_row(SEED, 3, np.arange(5)), [LH.k_row(SEED, 3, i) for i in range(5)])
    assert LH.k_row(SEED, 3, 4) != LH.k_row(SEED, 4, 4) and LH.k_row(SEED, 3, 4) != LH.k_row(SEED + 1, 3, 4)


# ------------------------------------------------------------------------------------------ the restatement: draw
def _epoch_rows(C, src_len, epochs=2):
    """every (clip, epoch) row of the GPU tests' store, restated"""
    clips, _ = LH.make_clips(C)
    tf = augment.TrainTransform(src_len)
    norm = np.zeros((len(clips), 4), dtype=np.float32)
    for i, c in enumerate(clips):
        lt, e = tf._normalisation(c)
        norm[i, :C], norm[i, 3] = lt, e
    rows = []
    for ep in range(epochs):
        for i, c in enumerate(clips):
            rows.append((len(c), LH.draw_row(LH.k_row(SEED, ep, i), len(c), norm[i], C, src_len)))
    return rows


def test_restated_rows_are_valid_and_the_seed_reaches_every_path():
    modes, pads, flips = set(), set(), set()
    for C in (2, 3):
        for src_len in (16, 32):
            for T, row in _epoch_rows(C, src_len):            # draw_row asserts the rounding margins of every row
                m = row["masked"]
                assert len(m) == int(0.2 * T) and np.all(np.diff(m) > 0) and (len(m) == 0 or (m[0] >= 0 and m[-1] < T))
                src, L = row["src"], row["L"]
                assert src.min() >= 0 and src.max() < T and 1 <= L <= int(1.5 * T)
                # the augmented clip is sorted and TemporalSample keeps its order inside the placed region (the pad rows
                # around it hold its first or last entry by their own place, not by the region's)
                a, b = (row["start"], row["start"] + L) if row["pad"] else (0, src_len)
                assert 0 <= a < b <= src_len and np.all(np.diff(src[a:b]) >= 0)
                assert row["prm"][21] == (1.0 if L <= src_len else 0.0)
                modes.add(row["mode"]); pads.add(row["pad"]); flips.add(row["flip"])
                M = row["prm"][11:20].reshape(3, 3)
                assert np.allclose(M @ M.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(M) - 1) < 1e-12
                if C == 2:
                    assert row["prm"][2] == row["prm"][6] == row["prm"][10] == 0 and M[2, 2] == 1
            assert modes == {"subset", "choice", "linspace"} and pads == {True, False} and flips == {True, False}, (C, src_len)
            modes, pads, flips = set(), set(), set()
    # eval: EvalTransform.draw's record
    clips, _ = LH.make_clips(2)
    ev = augment.EvalTransform(16)
    for c in (clips[0], clips[-1]):
        rec = ev.draw(c)
        row = LH.draw_row(0, len(c), np.r_[rec.left_top, 0, rec.edge_dist][[0, 1, 2, 3]], 2, 16, train=False)
        want = np.zeros(24)
        augment._params(rec, want)
        assert np.array_equal(row["prm"], want) and np.array_equal(row["src"], rec.src) and len(row["masked"]) == 0
    # the 3-D matrix is augment.euler_xyz_degrees of the three angles
    M, t = LH.rotation(77, 3, 0.1)
    assert np.allclose(M, augment.euler_xyz_degrees(np.rad2deg(t)), atol=1e-15)


# ------------------------------------------------------------------------------------------ distributions vs the reference replay
def _stats_restated(n, T, src_len, seed):
    out = []
    keys = LH.k_row(seed, 0, np.arange(n))
    for k in keys:
        row = LH.draw_row(k, T, np.array([0.1, 0.2, 0, 1.0], dtype=np.float32), 2, src_len)
        p = row["prm"]
        out.append((p[20], p[21], p[7], np.arctan2(p[14], p[11]), p[4], len(np.unique(row["src"])), len(row["masked"])))
    return np.asarray(out)


def _stats_reference(n, T, src_len, seed):
    random.seed(seed)
    np.random.seed(seed)
    clip = (np.random.RandomState(3).rand(T, 29, 2) + 0.5).astype(np.float32)
    tf = augment.TrainTransform(src_len)
    out = []
    for _ in range(n):
        r = tf.draw(clip)
        out.append((float(r.flip), float(r.pad32), r.shear, np.arctan2(r.rot[1, 0], r.rot[0, 0]), r.shear_origin[0],
                    len(np.unique(r.src)), len(r.masked)))
    return np.asarray(out)


def _same_distribution(a, b):
    """every compared quantity within 5 standard errors of the difference, estimated from the two samples"""
    def mean_ok(u, v):
        se = np.sqrt(u.var(ddof=1) / len(u) + v.var(ddof=1) / len(v))
        return abs(u.mean() - v.mean()) <= 5 * se, (u.mean(), v.mean(), se)

    def std_ok(u, v):
        def se_std(w):                                        # delta method: var(s^2) = (m4 - s^4) / n, s = sqrt(s^2)
            d = w - w.mean()
            s2 = d.var()
            return np.sqrt(max((np.mean(d ** 4) - s2 ** 2) / len(w), 0)) / (2 * np.sqrt(s2))
        se = np.sqrt(se_std(u) ** 2 + se_std(v) ** 2)
        return abs(u.std(ddof=1) - v.std(ddof=1)) <= 5 * se, (u.std(ddof=1), v.std(ddof=1), se)

    names = ("flip rate", "pad rate", "shear", "rotation angle", "origin coordinate", "distinct source frames")
    for col, name in enumerate(names):
        ok, what = mean_ok(a[:, col], b[:, col])
        assert ok, ("mean of " + name,) + what
        if col in (2, 3, 4):
            ok, what = std_ok(a[:, col], b[:, col])
            assert ok, ("std of " + name,) + what
    assert np.array_equal(a[:, 6], b[:, 6])                   # int(p T) masked frames, always


def test_distributions_match_the_replay_of_the_reference():
    n, T, src_len = 4000, 40, 32
    ref_a, ref_b = _stats_reference(n, T, src_len, 11), _stats_reference(n, T, src_len, 12)
    _same_distribution(ref_a, ref_b)                          # the yardstick passes on two samples of the reference
    _same_distribution(_stats_restated(n, T, src_len, SEED), ref_a)


# ------------------------------------------------------------------------------------------ the store and the loader on the host
def test_store_refuses_what_draw_refuses_naming_the_clip():
    clips, labels = LH.make_clips(2)
    tf = augment.TrainTransform(16)
    lengths, lab, norm, J, C = data.DeviceClipStore.check(clips, labels, tf)
    assert lengths.tolist() == LH.LENGTHS and (J, C) == (29, 2) and np.array_equal(lab, labels)
    for i in (0, 1, 36):                                      # the host's bits
        lt, e = tf._normalisation(clips[i])
        assert np.array_equal(norm[i], np.array([lt[0], lt[1], 0, e], dtype=np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.DeviceClipStore(clips, labels, "cpu", tf)
    bad = list(clips)
    bad[5] = clips[5][:4]
    with pytest.raises(ValueError, match=r"clip 5: clip of 4 raw frames: KeypointMasking masks"):
        data.DeviceClipStore(bad, labels, "cpu", tf)
    assert data.DeviceClipStore.check(bad, labels, augment.EvalTransform(16))[0][5] == 4      # eval takes short clips
    bad[5] = np.zeros_like(clips[5])
    with pytest.raises(ValueError, match="clip 5: no frame has the origin"):
        data.DeviceClipStore(bad, labels, "cpu", tf)
    bad[5] = clips[5][:, :20]
    with pytest.raises(ValueError, match="clip 5: expected a raw clip"):
        data.DeviceClipStore(bad, labels, "cpu", tf)
    bad[5] = np.concatenate([clips[5], clips[5][:, :3]], axis=1)
    with pytest.raises(ValueError, match=r"clip 5: clip .* does not match the store's \(J, C\)"):
        data.DeviceClipStore(bad, labels, "cpu", tf)
    bad[5] = np.ones((4097, 29, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="clip 5: clip of 4097 raw frames"):
        data.DeviceClipStore(bad, labels, "cpu", tf)
    with pytest.raises(ValueError, match="clip 0: .*TemporalAugmentation keeps"):
        data.DeviceClipStore(clips, labels, "cpu", augment.TrainTransform(16, frame_augmentation=(0.15, 1.5), sampling_prob=0.5))
    with pytest.raises(ValueError, match="device draw takes"):
        data.DeviceClipStore(clips, labels, "cpu", augment.TrainTransform(16, frame_augmentation=(0.5, 2.5)))
    for args, msg in (((clips, labels[:5], tf), "labels"), ((clips, labels.astype(np.float32), tf), "integers"),
                      (([], [], tf), "1 to"), ((clips, labels, None), "transform must be")):
        with pytest.raises(ValueError, match=msg):
            data.DeviceClipStore(*args[:2], "cpu", args[2])


def test_loader_refuses_bad_arguments_on_the_host():
    check = data.DeviceLoader.check
    assert check(37, 8, True, False, 0, 0, 1) == 5 and check(37, 8, True, True, 0, 0, 1) == 4
    assert check(37, 8, True, False, 0, 1, 2) == 3 and check(37, 8, True, True, 0, 1, 2) == 2
    assert check(37, 64, False, False, 0, 0, 1) == 1
    for args, msg in (((37, 0, True, False, 0, 0, 1), "batch_size"), ((37, 1025, True, False, 0, 0, 1), "batch_size"),
                      ((37, 8.0, True, False, 0, 0, 1), "batch_size"), ((37, True, True, False, 0, 0, 1), "batch_size"),
                      ((37, 8, True, False, 0, 2, 2), "rank"), ((37, 8, True, False, 0, -1, 2), "rank"),
                      ((37, 8, True, False, 0, 0, 0), "world"), ((37, 8, True, False, -1, 0, 1), "seed"),
                      ((37, 8, True, False, 1 << 32, 0, 1), "seed"), ((37, 64, True, True, 0, 0, 1), "no full batch")):
        with pytest.raises(ValueError, match=msg):
            check(*args)
    with pytest.raises(ValueError, match="DeviceClipStore"):
        data.DeviceLoader(object(), 8)
