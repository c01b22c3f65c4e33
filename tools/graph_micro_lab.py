#!/usr/bin/env python3
"""What micro-batching inside the captured train step buys: train.TrainStep(micro_batch=mb) issued from Python against
train.GraphedTrainStep(micro_batch=mb) replayed, on equal weights, both with optim.DeviceAdamW (eager: two launches after
the last slice; graphed: two nodes of the graph).  Each case is a child process of its own under its own time limit (a
case that fails ends the run; nothing is started after it):

  hgate-bf16    HGATE, bf16, B 64 in 16-clip slices: the host-bound case (a 10-17 ms step issued as 4 x ~400 launches)
  config3       HWGATE BASELINE config 3 (bf16, B 64) in 16-clip slices
  config5-fp32  HWGATE BASELINE config 5 (B 256, T 256, K 112, d 256), fp32, 16-clip slices
  config5-bf16  the same in bf16, 32-clip slices

Per case: the two variants are built one after the other -- the peak of allocated bytes over each one's construction and
first steps is taken relative to what was allocated before it was built -- and then timed in one process, windows
alternated eager, graphed, eager, ..., `--repeats` windows each, host clock around a window that ends in a synchronise.
The spread of a variant is (max - min) / median over its windows.  The hgate-bf16 case also times a third step object,
GraphedTrainStep(micro_batch=16, ragged=True), fed B rows and B - 1 rows in alternating windows: what a short batch costs.

  python tools/graph_micro_lab.py [--only config3] [--repeats 3] [--txt profiles/graph_micro_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                       # bench.py CFG (BASELINE configs[1], [2])
CFG5 = dict(B=256, T=256, J=133, nW=7, C=3, d0=256, nc=2002)                    # bench.py CFG5 (BASELINE configs[4])
CFG_HGATE = dict(B=64, T=128, J=29, K=29, C=2, d0=128, nc=2002)                 # bench.py CFG_HGATE
# case: (kind, config, dtype, micro_batch, steps per window, time limit in seconds)
CASES = {"hgate-bf16": ("hgate", CFG_HGATE, "bf16", 16, 80, 180), "config3": ("hwgate", CFG, "bf16", 16, 40, 180),
         "config5-fp32": ("hwgate", CFG5, "fp32", 16, 2, 300), "config5-bf16": ("hwgate", CFG5, "bf16", 32, 2, 200)}


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def _window(torch, step, x, y, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(x, y)
    torch.cuda.synchronize()
    return steps * x.shape[0] / (time.perf_counter() - t0)


def run_case(name, repeats):
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    train = importlib.import_module("sl-hwgat_amd.train")
    optim = importlib.import_module("sl-hwgat_amd.optim")
    dev = torch.device("cuda:0")
    kind, c, dtype, mb, steps, _ = CASES[name]
    dtype = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=dev, generator=g)
    y = torch.randint(0, c["nc"], (c["B"],), device=dev, generator=g)

    def build(graphed, **kw):
        torch.manual_seed(1001)                              # equal weights
        if kind == "hgate":
            hp = hw.HGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, embed_dim=c["d0"])
            model = hw.HGATEModel(*hp.get_model_params()).to(dev)
        else:
            hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, num_kps=c["nW"] * 16, embed_dim=c["d0"])
            model = hw.Model(*hp.get_model_params()).to(dev)
            model.use_part_table(hw.part_table(c["J"], c["nW"]))
        model.set_activation_dtype(dtype)
        model.train()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        o = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
        if graphed:
            s = train.GraphedTrainStep(model, o, x, y, warmup=1, micro_batch=mb, **kw)
        else:
            s = train.TrainStep(model, o, micro_batch=mb)
        for _ in range(2):
            s(x, y)
        torch.cuda.synchronize()
        print(f"[{name}] {'graphed' if graphed else 'eager'} step built and run twice", file=sys.stderr, flush=True)
        return s, torch.cuda.max_memory_allocated() - before

    variants = {"eager": build(False), "graphed": build(True)}
    rate = {n: [] for n in variants}
    for _ in range(repeats):
        for n, (s, _) in variants.items():
            rate[n].append(_window(torch, s, x, y, steps))
    e, gr = statistics.median(rate["eager"]), statistics.median(rate["graphed"])
    se, sg = _spread(rate["eager"]), _spread(rate["graphed"])
    ahead = "ahead by more than both spreads" if gr / e - 1 > max(se, sg) else "NOT ahead by more than the spread"
    print(f"{name}: B {c['B']} in {variants['graphed'][0].n_slices} slices of {mb}, {steps} steps per window, {repeats} windows "
          f"each, alternated\n"
          f"  eager   {e:9.1f} clips/s (spread {100 * se:.2f} %)  step {1e3 * c['B'] / e:8.2f} ms  peak {variants['eager'][1] / 2 ** 30:7.2f} GiB allocated\n"
          f"  graphed {gr:9.1f} clips/s (spread {100 * sg:.2f} %)  step {1e3 * c['B'] / gr:8.2f} ms  peak {variants['graphed'][1] / 2 ** 30:7.2f} GiB allocated\n"
          f"  graphed / eager {gr / e:.4f}: {ahead}; loss eager {float(variants['eager'][0].loss):.4f} graphed "
          f"{float(variants['graphed'][0].loss):.4f}", flush=True)
    if name == "hgate-bf16":
        del variants
        s, _ = build(True, ragged=True)
        feeds = {"full (n = B)": (x, y), "short (n = B - 1)": (x[:-1], y[:-1])}
        r = {k: [] for k in feeds}
        for _ in range(repeats):
            for k, (xs, ys) in feeds.items():
                s(xs, ys)                                    # the window starts after the row count changed
                r[k].append(xs.shape[0] / _window(torch, s, xs, ys, steps))         # seconds per replay
        full, short = (statistics.median(r[k]) for k in feeds)
        print(f"  ragged=True, one graph: replay fed B rows {1e3 * full:.3f} ms (spread {100 * _spread(r['full (n = B)']):.2f} %), "
              f"fed B - 1 rows {1e3 * short:.3f} ms (spread {100 * _spread(r['short (n = B - 1)']):.2f} %), "
              f"short / full {short / full:.4f}", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "graph_micro_lab.txt"))
    ap.add_argument("--case", choices=list(CASES))
    ap.add_argument("--only", choices=list(CASES), help="run this case alone (still as a child process)")
    args = ap.parse_args()
    if args.case:
        return run_case(args.case, args.repeats)
    text, ok = [], True
    for name in CASES:                                       # this process never opens the GPU: every case is a fresh child
        if args.only not in (None, name):
            continue
        cmd = ["timeout", "-k", "10", str(CASES[name][5]), sys.executable, os.path.abspath(__file__), "--case", name,
               "--repeats", str(args.repeats)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)          # stderr (progress, errors) goes straight through
        text += res.stdout.splitlines()
        print(res.stdout, end="", flush=True)
        if res.returncode != 0:
            ok = False
            text.append(f"case {name} ended with status {res.returncode}; nothing was started after it")
            print(text[-1], flush=True)
            break
    with open(args.txt, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
