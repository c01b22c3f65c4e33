#!/usr/bin/env python3
"""Cost of the device-side train transform (sl-hwgat_amd/augment.py), three numbers:

  1. host   `TrainTransform.draw` + `AugmentBatcher` packing / launch, ms per clip (B = 64, T_raw = 128)
  2. device hwgat_aug_hand_fill + hwgat_aug_resample per B = 64 batch at T_raw = src_len in {64, 128, 192} (HIP events)
  3. clips/s of an 8-worker DataLoader (draw in the workers) + AugmentBatcher + bf16 HWGATE TrainStep, against the same
     step on one pre-made device batch

Synthetic raw clips (29 joints, C = 2, pixel-range coordinates, 30 % of the hand frames absent).  The reference's own
transform costs ~30 ms per clip at T_raw = 128 on one CPU core (measured with its Compose; it is not imported here).

  python tools/augment_lab.py [--steps 20] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hw = importlib.import_module("sl-hwgat_amd")
aug = hw.augment
train_mod = importlib.import_module("sl-hwgat_amd.train")


def synth_clip(rng, T, C=2):
    base = np.concatenate([rng.uniform(300, 1600, (29, 1)), rng.uniform(150, 900, (29, 1))], axis=1)[:, :C]
    clip = (base[None] + np.cumsum(rng.normal(0, 4.0, (T, 29, C)), axis=0)).astype(np.float32)
    for a, e in ((9, 19), (19, 29)):
        clip[rng.random(T) < 0.3, a:e] = 0.0
    return clip


class Clips(torch.utils.data.Dataset):
    def __init__(self, n, T, src_len, nc):
        rng = np.random.default_rng(0)
        self.clips = [synth_clip(rng, T) for _ in range(n)]
        self.tf = aug.TrainTransform(src_len)
        self.nc = nc

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        clip = self.clips[i]
        return clip, i % self.nc, self.tf.draw(clip)


def host_cost(dev, B=64, T=128, reps=5):
    ds = Clips(B, T, T, 10)
    batcher = aug.AugmentBatcher(B, T, dev)
    best_draw = best_pack = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        batch = [ds[i] for i in range(B)]
        t1 = time.perf_counter()
        batcher(batch)
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        best_draw, best_pack = min(best_draw, t1 - t0), min(best_pack, t2 - t1)
    return {"draw_ms_per_clip": 1e3 * best_draw / B, "pack_launch_ms_per_clip": 1e3 * best_pack / B,
            "total_ms_per_clip": 1e3 * (best_draw + best_pack) / B}


def device_time(dev, T, B=64, reps=20):
    ds = Clips(B, T, T, 10)
    batch = [ds[i] for i in range(B)]
    clips = [b[0] for b in batch]
    recs = [b[2] for b in batch]
    off = np.concatenate([[0], np.cumsum([r.T for r in recs])]).astype(np.int32)
    x0 = torch.from_numpy(np.concatenate(clips)).to(dev)
    offd = torch.from_numpy(off).to(dev)
    mask = np.zeros(off[-1], np.uint8)
    for a, r in zip(off[:-1], recs):
        mask[a + r.masked] = 1
    maskd = torch.from_numpy(mask).to(dev)
    src = torch.from_numpy(np.stack([r.src for r in recs])).to(dev)
    prm = np.zeros((B, aug.NPRM))
    for i, r in enumerate(recs):
        aug._params(r, prm[i])
    prmd = torch.from_numpy(prm).to(dev)
    out = {}
    for name, gather in (("raw29", None), ("window64", hw.part_table(29).to(dev))):
        times = []
        for _ in range(reps):
            x = x0.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            aug.hand_fill(x, offd, T, masked=maskd)
            aug.resample(x, offd, src, prmd, gather)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        out[name] = {"median_ms": float(np.median(times)), "min_ms": float(np.min(times))}
    return out


def pipeline(dev, steps, B=64, T=128, workers=8, nc=2002):
    torch.manual_seed(1001)
    hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, 2, dev, num_kps=64)
    model = hw.Model(*hp.get_model_params()).to(dev)
    model.use_part_table(hw.part_table(29))
    model.set_activation_dtype(torch.bfloat16)
    model.train()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True)
    step = train_mod.TrainStep(model, opt)
    ds = Clips(B * 8, T, T, nc)
    batcher = aug.AugmentBatcher(B, T, dev)
    x, y = batcher([ds[i] for i in range(B)])
    for _ in range(3):
        step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(x, y)
    torch.cuda.synchronize()
    premade = steps * B / (time.perf_counter() - t0)
    loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True, num_workers=workers, collate_fn=list,
                                         drop_last=True, persistent_workers=True, prefetch_factor=4)
    it, done = iter(loader), 0

    def next_batch():
        nonlocal it
        try:
            return next(it)
        except StopIteration:
            it = iter(loader)
            return next(it)

    for _ in range(3):
        step(*batcher(next_batch()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(*batcher(next_batch()))
        done += B
    torch.cuda.synchronize()
    fed = done / (time.perf_counter() - t0)
    return {"premade_clips_per_s": premade, "augmented_clips_per_s": fed, "ratio": fed / premade,
            "workers": workers, "B": B, "T": T, "model": "HWGATE bf16, 29 joints -> 64 slots"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"host": host_cost(dev), "device": {str(T): device_time(dev, T) for T in (64, 128, 192)},
           "pipeline": pipeline(dev, args.steps),
           "reference_ms_per_clip": {"64": 9.4, "128": 29.8, "192": 61.3, "source": "issue measurement, one core"}}
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
