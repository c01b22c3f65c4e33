#!/usr/bin/env python3
"""What the fused smoothed cross-entropy and the device-side evaluation loop buy, measured on the device.  Two parts, each a
child process of its own under its own time limit (a part that fails ends the run; nothing is started after it):

  criterion  loss + correct-count, forward and backward, on fp32 logits (64, 2002): train.SmoothedCrossEntropyLoss plus
             TrainStep's argmax line against train.FusedSmoothedCrossEntropyLoss plus its correct().  HIP-event time per
             call over windows of `--iters` eager calls (host-issued, so launch cost is in the figure: that is the point),
             the two variants alternated, two repeats each; and the number of kernels one call launches, counted by
             torch.profiler in a pass of its own after the timing.
  loop       an evaluation loop of 64 batches of HWGATE at BASELINE config 2 (T 128, 67 joints, 2002 classes), B = 4 and
             B = 64, fp32 and bf16 activations, in three variants alternated in one process, two repeats each:
               reference   written like hwgat/utils.py:118-142: eager forward, torch criterion, loss.item(), a full argsort
                           for top-1, .cpu().tolist() per batch
               eager       evaluate.Evaluator(graph=False)
               graphed     evaluate.Evaluator(graph=True)
             clips/s from a host clock around the loop, which ends in the variant's own host read (reference: per batch;
             Evaluator: result()) and a device synchronise.  Inputs are on the device before the clock starts.

  python tools/eval_lab.py [--iters 200] [--txt profiles/eval_lab.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("criterion", 180), ("loop", 420))                                      # (part, time limit in seconds)
CFG = dict(T=128, J=67, nW=5, C=2, d0=128, nc=2002)                             # bench.py CFG (BASELINE configs[1])


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, importlib.import_module("sl-hwgat_amd.train"), torch.device("cuda:0")


def part_criterion(args):
    torch, hw, train, DEV = _gpu()
    B, C = 64, CFG["nc"]
    g = torch.Generator(device=DEV).manual_seed(1)
    z = torch.randn(B, C, device=DEV, generator=g).requires_grad_(True)
    y = torch.randint(0, C, (B,), device=DEV, generator=g)
    crits = {"torch": train.SmoothedCrossEntropyLoss(), "fused": train.FusedSmoothedCrossEntropyLoss()}

    def call(name):
        z.grad = None
        loss = crits[name](z, y) * 0.5                       # a device-side upstream gradient that is not 1, as TrainStep's
        loss.backward()
        return loss.detach(), train._correct(crits[name], z, y)

    def window(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            call(name)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters          # microseconds per call

    for name in crits:                                       # warm-up: code objects, allocator
        for _ in range(20):
            call(name)
    torch.cuda.synchronize()
    us = {name: [] for name in crits}
    for _ in range(2):
        for name in crits:
            us[name].append(window(name))
    launches = {}
    for name in crits:
        try:
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                call(name)
                torch.cuda.synchronize()
            launches[name] = str(sum(1 for e in prof.events() if e.device_type.name == "CUDA" and "Memcpy" not in e.name
                                     and "Memset" not in e.name))
        except Exception as exc:                             # noqa: BLE001
            launches[name] = f"not measured ({type(exc).__name__})"
    lt, ct = call("torch")
    lf, cf = call("fused")
    print(f"criterion: loss + correct-count, forward and backward, logits ({B}, {C}) fp32, eager, {args.iters} calls per window")
    for name in crits:
        a, b = us[name]
        print(f"  {name:6s} {min(a, b):8.1f} us per call (repeats {a:.1f} / {b:.1f}), kernels launched per call: {launches[name]}")
    print(f"  same input: loss {float(lt):.6f} / {float(lf):.6f}, correct {int(ct)} / {int(cf)}")
    return 0


def part_loop(args):
    torch, hw, train, DEV = _gpu()
    evaluate = importlib.import_module("sl-hwgat_amd.evaluate")
    c, n_batches = CFG, 64
    print(f"loop: {n_batches} batches of HWGATE config 2 in eval(), clips/s (host clock, ends in the variant's host read + synchronise)")
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(1001)
        hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], DEV, num_kps=c["nW"] * 16, embed_dim=c["d0"])
        model = hw.Model(*hp.get_model_params()).to(DEV)
        model.use_part_table(hw.part_table(c["J"], c["nW"]))
        model.set_activation_dtype(dtype)
        model.eval()
        crit = train.SmoothedCrossEntropyLoss()
        for B in (4, 64):
            g = torch.Generator(device=DEV).manual_seed(B)
            xs = [torch.rand(B, c["T"], c["J"], c["C"], device=DEV, generator=g) for _ in range(4)]
            ys = [torch.randint(0, c["nc"], (B,), device=DEV, generator=g) for _ in range(4)]
            evs = {"eager": evaluate.Evaluator(model, c["nc"], xs[0], graph=False),
                   "graphed": evaluate.Evaluator(model, c["nc"], xs[0], graph=True)}

            def reference():
                total, acc = 0.0, []
                with torch.no_grad():
                    for i in range(n_batches):
                        out = model(xs[i % 4])
                        total += crit(out, ys[i % 4]).item()
                        pred = torch.argsort(out, dim=-1, descending=True)
                        acc += (pred[:, 0:1] == ys[i % 4].unsqueeze(-1)).any(-1).float().cpu().tolist()
                return total / n_batches, sum(acc) / len(acc)

            def device(ev):
                ev.reset()
                for i in range(n_batches):
                    ev.update(xs[i % 4], ys[i % 4])
                r = ev.result()
                return r["loss"], r["acc"][1]

            variants = {"reference": reference, "eager": lambda: device(evs["eager"]), "graphed": lambda: device(evs["graphed"])}
            got = {k: f() for k, f in variants.items()}          # warm-up of every variant, and what each computes
            torch.cuda.synchronize()
            rate = {k: [] for k in variants}
            for _ in range(2):
                for k, f in variants.items():
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    rate[k].append(n_batches * B / (time.perf_counter() - t0))
            name = "fp32" if dtype == torch.float32 else "bf16"
            for k in variants:
                a, b = rate[k]
                print(f"  {name} B={B:<3d} {k:10s} {max(a, b):9.0f} clips/s (repeats {a:.0f} / {b:.0f}); loss {got[k][0]:.5f}, top-1 {got[k][1]:.4f}")
            del evs
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "eval_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    args = ap.parse_args()
    if args.part:
        return {"criterion": part_criterion, "loop": part_loop}[args.part](args)
    text, ok = [], True
    for part, limit in PARTS:                  # this process never opens the GPU: every part is a fresh child
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--iters", str(args.iters)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        text += res.stdout.splitlines()
        print(res.stdout, end="", flush=True)
        if res.returncode != 0:
            ok = False
            text.append(f"part {part} ended with status {res.returncode}; nothing was started after it")
            print(text[-1] + "\n" + res.stderr[-2000:], flush=True)
            break
    with open(args.txt, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
