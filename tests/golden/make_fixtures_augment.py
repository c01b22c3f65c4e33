#!/usr/bin/env python3
"""Golden vectors for the device-side train / val-test transforms, from the REFERENCE (development container only).

Run:  python tests/golden/make_fixtures_augment.py        (needs /root/reference)

Imports the reference's `hwgat/dataTransform.py` as-is, builds its train transform (configs.py:93-103) and val / test
transform (configs.py:105-108) without the final WindowCreate (the 29-joint output; the 64-slot layout is the
`parts.part_table(29)` gather, checked against WindowCreate by window_create.npz), and stores data only:

  augment_2d.npz  C = 2, src_len 64;  augment_3d.npz  C = 3, src_len 48
    clips      (total_frames, 29, C) float32 synthetic raw clips in pixel-range coordinates, packed
    off        (n + 1,) int64 frame offsets of the clips
    seed       the value `random.seed` and `np.random.seed` received before the train run
    train      (n, src_len, 29, C) float32: the train transform applied to the clips in order, one seeded run
    eval       (n, src_len, 29, C) float32: the val / test transform
    py_state / np_state   sha256 of random.getstate() / np.random.get_state() after the train run (state_digests)
Hand gaps: leading, trailing, in the middle, absent everywhere, exactly 2 and exactly 3 present frames, none.
"""
import hashlib
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/hwgat"
SEED = 1001                                  # configs.py:55-57
HANDS = ((9, 19, 7), (19, 29, 8))


def state_digests():
    py = hashlib.sha256(repr(random.getstate()).encode()).hexdigest()
    name, keys, pos, has_gauss, gauss = np.random.get_state()
    npd = hashlib.sha256(name.encode() + keys.tobytes() + repr((int(pos), int(has_gauss), float(gauss))).encode())
    return py, npd.hexdigest()


def synth_clip(rng, T, C, left, right):
    """smooth random-walk skeleton of 29 joints; `left` / `right`: per-frame hand presence (bool (T,))"""
    base = np.concatenate([rng.uniform(300, 1600, (29, 1)), rng.uniform(150, 900, (29, 1))]
                          + ([rng.uniform(-400, 400, (29, 1))] if C == 3 else []), axis=1)
    walk = np.cumsum(rng.normal(0, 4.0, (T, 29, C)), axis=0)
    clip = (base[None] + walk).astype(np.float32)
    for (a, e, _), pres in zip(HANDS, (left, right)):
        clip[~pres, a:e] = 0.0
    return clip


def gap_patterns(rng, T):
    """named presence masks for one hand"""
    allp = np.ones(T, bool)
    lead = allp.copy(); lead[:max(1, T // 5)] = False
    trail = allp.copy(); trail[T - max(1, T // 4):] = False
    mid = allp.copy(); mid[T // 3:T // 3 + max(1, T // 6)] = False
    rand = rng.random(T) > 0.35
    none = np.zeros(T, bool)
    two = np.zeros(T, bool); two[rng.choice(T, 2, replace=False)] = True
    three = np.zeros(T, bool); three[np.sort(rng.choice(T, 3, replace=False))] = True
    return dict(all=allp, lead=lead, trail=trail, mid=mid, rand=rand, none=none, two=two, three=three)


def make_clips(C, lengths, seed):
    rng = np.random.default_rng(seed)
    names = ["all", "lead", "trail", "mid", "rand", "none", "two", "three"]
    clips = []
    for i, T in enumerate(lengths):
        pats = gap_patterns(rng, T)
        left = pats[names[i % len(names)]]
        right = pats[names[(3 * i + 1) % len(names)]]
        clip = synth_clip(rng, T, C, left, right)
        if i % 4 == 1:                       # the normalisation frame is not the first one
            clip[:min(3, T - 2), 3] = 0.0
        clips.append(clip)
    return clips


def main():
    sys.path.insert(0, REF)
    import dataTransform as D                # noqa: E402  (the reference, as-is)
    cfg = dict(origin=0, anchors=[3, 4], frame_aug=[0.5, 1.5], p=0.2, shear=0.1, rot=0.1)
    for C, src_len, lengths, name in (
            (2, 64, [5, 6, 9, 17, 30, 48, 63, 64, 65, 80, 96, 120, 128, 150, 200, 240, 300, 40], "augment_2d.npz"),
            (3, 48, [5, 8, 12, 24, 36, 47, 48, 49, 60, 75, 90, 110, 160, 220, 290, 20], "augment_3d.npz")):
        clips = make_clips(C, lengths, seed=C * 7919)
        train = D.Compose([D.KeypointMasking(cfg["p"], HANDS[0][0], HANDS[1][1]),
                           D.HandCorrection(list(HANDS[0]), list(HANDS[1])),
                           D.NormalizeKeypoints(cfg["origin"], cfg["anchors"]),
                           D.ShearTransform(cfg["shear"]),
                           D.RotatationTransform(cfg["rot"]),
                           D.TemporalAugmentation(cfg["frame_aug"], True, True),
                           D.TemporalSample(src_len, True),
                           D.RandomFlip("keypoints")])
        evalt = D.Compose([D.HandCorrection(list(HANDS[0]), list(HANDS[1])),
                           D.NormalizeKeypoints(cfg["origin"], cfg["anchors"]),
                           D.TemporalSample(src_len)])
        random.seed(SEED)
        np.random.seed(SEED)
        tr = np.stack([np.asarray(train(c.copy()), dtype=np.float32) for c in clips])
        py, npd = state_digests()
        ev = np.stack([np.asarray(evalt(c.copy()), dtype=np.float32) for c in clips])
        off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
        path = os.path.join(HERE, name)
        np.savez_compressed(path, clips=np.concatenate(clips), off=off, seed=np.int64(SEED), src_len=np.int64(src_len),
                            train=tr, eval=ev, py_state=np.array(py), np_state=np.array(npd))
        print(f"wrote {path}: {len(clips)} clips, {off[-1]} frames, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
