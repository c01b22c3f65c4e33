#!/usr/bin/env python3
"""What Mixup / temporal CutMix inside the train step (train.BatchMixer, csrc/mix.hip, hwgat_mbsce_* of csrc/loss_eval.hip)
costs, measured on the device.  Two parts, each a child process of its own under its own time limit (a part that fails
ends the run; nothing is started after it):

  launch  the mixer's and the criterion's launches, each alone, at HWGATE's config 2 (B = 64, T = 128, 67 joints, 2002
          classes): HIP events around replays of ONE graph that holds `--chain` calls back to back, `--launches` per window:
          the device time of a call.  draw; apply with every pair Mixup, every pair CutMix, no pair mixed; the pair
          criterion forward (four launches) and backward against hwgat_bsce_fwd (three) and hwgat_bsce_bwd.
  train   ms per step of train.GraphedTrainStep(ragged=True) with DeviceAdamW inside the graph, HWGATE config 2, fp32 and
          bf16 activations: variant A without a mixer against variant B with BatchMixer(prob=1), two models in one process,
          windows alternated A B A B ..., `--repeats` each; host clock around a window that ends in a synchronise.  The
          spread of a variant is (max - min) / median over its windows.  `--no-mixer` runs variant A alone and never passes
          the `mixer` keyword: that is how the commit before the mixer is measured with this file.

  python tools/mix_lab.py [--only launch] [--no-mixer] [--label NAME] [--txt profiles/mix_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("launch", 180), ("train", 400))                                       # (part, time limit in seconds)
CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                       # bench.py CFG (BASELINE configs[1])


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, importlib.import_module("sl-hwgat_amd.train"), torch.device("cuda:0")


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def part_launch(args):
    torch, hw, train, DEV = _gpu()
    HF = hw.functional
    assert args.launches % args.chain == 0
    c = CFG
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
    y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
    z = torch.randn(c["B"], c["nc"], device=DEV, generator=g)
    rows = torch.full((1,), c["B"], dtype=torch.int32, device=DEV)
    g_up = torch.ones(1, device=DEV)

    def mixer_of(prob, share):
        m = train.BatchMixer(prob=prob, cutmix_share=share, seed=3).bind(DEV, c["B"], c["T"])
        HF.mix_draw(m._state, y, rows, m.pairs, m.partner, m.lam, m.seg, m.mode, m.y_b, c["T"])
        return m

    mixup, cutmix, none = mixer_of(1.0, 0.0), mixer_of(1.0, 1.0), mixer_of(0.0, 0.5)
    fwd = HF.bsce_forward(z, y, 0.01, rows, 0)
    mfwd = HF.mbsce_forward(z, y, mixup.y_b, mixup.lam, 0.01, rows, 0)
    dz = torch.empty_like(z)

    def draw(m):
        return lambda: HF.mix_draw(m._state, y, rows, m.pairs, m.partner, m.lam, m.seg, m.mode, m.y_b, c["T"])

    def apply(m):
        return lambda: HF.mix_apply(x, m.pairs, m.lam, m.seg, m.mode, rows)

    calls = [("mix_draw (32 pairs)", draw(mixup)), ("mix_apply, every pair Mixup", apply(mixup)),
             ("mix_apply, every pair CutMix", apply(cutmix)), ("mix_apply, no pair mixed", apply(none)),
             ("bsce_fwd (3 launches)", lambda: HF.bsce_forward(z, y, 0.01, rows, 0, out=fwd)),
             ("mbsce_fwd (4 launches)", lambda: HF.mbsce_forward(z, y, mixup.y_b, mixup.lam, 0.01, rows, 0, out=mfwd)),
             ("bsce_bwd", lambda: HF.bsce_backward(z, y, fwd[2], g_up, 0.01, rows, 0, out=dz)),
             ("mbsce_bwd", lambda: HF.mbsce_backward(z, y, mixup.y_b, mixup.lam, mfwd[2], g_up, 0.01, rows, 0, out=dz))]
    mb = x.numel() * 4 / 1e6
    print(f"launch [{args.label}]: us per call, {args.launches} calls per window, {args.repeats} windows (median; spread = "
          f"(max - min) / median); device time = replays of a graph of {args.chain} calls; x is {tuple(x.shape)} fp32 = "
          f"{mb:.1f} MB, logits {tuple(z.shape)}")
    for name, fn in calls:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.chain):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches // args.chain):
                graph.replay()
            b.record()
            b.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / args.launches)
        print(f"  {name:30s}  {statistics.median(us):7.2f} us (spread {100 * _spread(us):.1f} %)", flush=True)
    return 0


def part_train(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    c, steps = CFG, args.train_steps
    names = ("A",) if args.no_mixer else ("A", "B")
    print(f"train [{args.label}]: ms per step of train.GraphedTrainStep(ragged=True) with DeviceAdamW inside the graph, HWGATE "
          f"config 2 (B = {c['B']}, T = {c['T']}); A = no mixer" + ("" if args.no_mixer else ", B = BatchMixer(prob=1)") +
          f"; {steps} steps per window, {args.repeats} windows, alternated in one process (median; spread = (max - min) / median)")
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        variants = {}
        for name in names:
            torch.manual_seed(1001)
            hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], DEV, num_kps=c["nW"] * 16, embed_dim=c["d0"])
            model = hw.Model(*hp.get_model_params()).to(DEV)
            model.use_part_table(hw.part_table(c["J"], c["nW"]))
            model.set_activation_dtype(dtype)
            model.train()
            g = torch.Generator(device=DEV).manual_seed(7)
            x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
            y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
            o = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
            kw = dict(mixer=train.BatchMixer(prob=1.0, seed=3)) if name == "B" else {}
            s = train.GraphedTrainStep(model, o, x, y, ragged=True, **kw)
            for _ in range(5):
                s(x, y)
            variants[name] = (s, x, y)
        torch.cuda.synchronize()
        ms = {n: [] for n in variants}
        for _ in range(args.repeats):
            for name, (s, x, y) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    s(x, y)
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
        line = f"  {tag}"
        for name in names:
            line += (f"   {name} {statistics.median(ms[name]):8.3f} ms (spread {100 * _spread(ms[name]):.2f} %; windows " +
                     ", ".join(f"{v:.3f}" for v in ms[name]) + ")")
        if "B" in ms:
            line += f"   B - A {statistics.median(ms['B']) - statistics.median(ms['A']):+.3f} ms"
        print(line + "; loss " + " ".join(f"{n} {float(variants[n][0].loss):.4f}" for n in names), flush=True)
        del variants
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="calls per window (part launch)")
    ap.add_argument("--chain", type=int, default=50, help="calls held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-mixer", action="store_true", help="variant A alone, without the `mixer` keyword (an older commit)")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "mix_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    ap.add_argument("--only", choices=[p for p, _ in PARTS], help="run this part alone (still as a child process)")
    args = ap.parse_args()
    if args.part:
        return {"launch": part_launch, "train": part_train}[args.part](args)
    text, ok = [], True
    for part, limit in PARTS:                                 # this process never opens the GPU: every part is a fresh child
        if args.only not in (None, part) or (args.no_mixer and part == "launch"):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--launches", str(args.launches), "--chain", str(args.chain), "--train-steps", str(args.train_steps),
               "--repeats", str(args.repeats), "--label", args.label] + (["--no-mixer"] if args.no_mixer else [])
        res = subprocess.run(cmd, capture_output=True, text=True)
        text += res.stdout.splitlines()
        print(res.stdout, end="", flush=True)
        if res.returncode != 0:
            ok = False
            text.append(f"part {part} ended with status {res.returncode}; nothing was started after it")
            print(text[-1] + "\n" + res.stderr[-2000:], flush=True)
            break
    with open(args.txt, "a" if args.no_mixer else "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
