#!/usr/bin/env python3
"""Batches/s of the train input, two routes, alone and in front of a graphed bf16 train step:

  device  data.DeviceClipStore + data.DeviceLoader (eager launches, and graph=True: one replay per batch)
  host    augment.TrainTransform.draw in the main process on an in-memory list of clips + augment.AugmentBatcher
          (no DataLoader workers: the route a single process has without the device store)

and the step's ceiling on one pre-made batch.  B = 64, 128 raw frames, 29 joints, C = 2, src_len = 128; synthetic clips with
30 % of the hand frames absent.  Wall-clock time around a run of batches with one synchronisation at the end (the host's
work is what is being measured): `--steps` batches in front of a step, 4 x as many for the host route alone and 100 x as
many for the device loader alone, so that every window is a good fraction of a second; median and spread of `--repeats`
runs after a warm-up.

  python tools/loader_lab.py [--model HWGATE|HGATE] [--steps 80] [--repeats 5] [--out profiles/loader_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hw = importlib.import_module("sl-hwgat_amd")
train = importlib.import_module("sl-hwgat_amd.train")
aug, data, optim = hw.augment, hw.data, hw.optim
B, T, J, C, NC = 64, 128, 29, 2, 2002


def synth_clip(rng):
    base = np.concatenate([rng.uniform(300, 1600, (J, 1)), rng.uniform(150, 900, (J, 1))], axis=1)[:, :C]
    clip = (base[None] + np.cumsum(rng.normal(0, 4.0, (T, J, C)), axis=0)).astype(np.float32)
    for a, e in ((9, 19), (19, 29)):
        clip[rng.random(T) < 0.3, a:e] = 0.0
    return clip


def timed(fn, steps, repeats, warmup=5):
    """(median, lowest, highest) batches/s of `repeats` runs of `steps` calls"""
    for _ in range(warmup):
        fn()
    rates = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        rates.append(steps / (time.perf_counter() - t0))
    return statistics.median(rates), min(rates), max(rates)


def make_step(dev, kind):
    torch.manual_seed(1001)
    if kind == "HWGATE":
        hp = hw.HWGATEParams({"src_len": T, "num_class": NC}, C, dev, num_kps=64)
        model = hw.Model(*hp.get_model_params()).to(dev)
        model.use_part_table(hw.part_table(J))
    else:
        hp = hw.HGATEParams({"src_len": T, "num_class": NC}, C, dev)
        model = hw.HGATEModel(*hp.get_model_params()).to(dev)
    model.set_activation_dtype(torch.bfloat16)                # both take the 29 raw joints
    model.train()
    opt = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
    step = train.GraphedTrainStep(model, opt, torch.zeros(B, T, J, C, device=dev),
                                  torch.zeros(B, dtype=torch.int64, device=dev), ragged=True)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="HWGATE", choices=["HWGATE", "HGATE"])
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    clips = [synth_clip(rng) for _ in range(args.clips)]
    labels = np.arange(args.clips) % NC
    tf = aug.TrainTransform(T)
    step = make_step(dev, args.model)

    t0 = time.perf_counter()
    store = data.DeviceClipStore(clips, labels, dev, tf)
    upload_s = time.perf_counter() - t0
    eager = data.DeviceLoader(store, B, seed=1, drop_last=True)
    graphed = data.DeviceLoader(store, B, seed=1, drop_last=True, graph=True)
    bound = data.DeviceLoader(store, B, seed=1, drop_last=True, graph=True)
    bound.bind(step.x, step.y)

    batcher = aug.AugmentBatcher(B, T, dev)
    order = np.random.default_rng(1)

    def host_batch():
        idx = order.integers(0, args.clips, B)
        return batcher([(clips[i], int(labels[i]), tf.draw(clips[i])) for i in idx])

    x0, y0 = host_batch()
    rows = [
        ("device loader alone, eager (4 launches)", timed(eager.next_batch, 100 * args.steps, args.repeats)),
        ("device loader alone, graph (1 replay)", timed(graphed.next_batch, 100 * args.steps, args.repeats)),
        ("host draw + AugmentBatcher alone", timed(host_batch, 4 * args.steps, args.repeats)),
        (f"graphed bf16 {args.model} step on one pre-made batch", timed(lambda: step(x0, y0), args.steps, args.repeats)),
        (f"graphed bf16 {args.model} step fed by the device loader (bound, graph)",
         timed(lambda: (bound.next_batch(), step(step.x, step.y)), args.steps, args.repeats)),
        (f"graphed bf16 {args.model} step fed by host draw + AugmentBatcher",
         timed(lambda: step(*host_batch()), args.steps, args.repeats)),
    ]
    lines = [f"loader_lab: B = {B}, {T} raw frames, J = {J}, C = {C}, src_len = {T}, {args.clips} clips "
             f"({store.nbytes / 2 ** 20:.1f} MiB on the device, uploaded in {upload_s:.2f} s); model {args.model} bf16, "
             f"DeviceAdamW, ragged GraphedTrainStep; {args.steps} batches per run in front of a step, {4 * args.steps} for the host "
             f"route alone, {100 * args.steps} for the device loader alone; median (lowest .. highest) of {args.repeats} runs, "
             f"wall clock",
             f"{'route':<72} {'batches/s':>10} {'lowest':>9} {'highest':>9} {'clips/s':>10} {'ms/batch':>9}"]
    for name, (rate, lo, hi) in rows:
        lines.append(f"{name:<72} {rate:>10.1f} {lo:>9.1f} {hi:>9.1f} {rate * B:>10.0f} {1e3 / rate:>9.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
