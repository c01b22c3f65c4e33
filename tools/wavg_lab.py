#!/usr/bin/env python3
"""What weight averaging (optim.WeightAverage, csrc/weight_avg.hip) costs, measured on the device.  Two parts, each a child
process of its own under its own time limit (a part that fails ends the run; nothing is started after it):

  launch  the averager's advance, update and swap launches over the parameter set of HWGATE at BASELINE config 2, each
          alone: HIP events around replays of ONE graph that holds `--chain` launches back to back, `--launches` per
          window: the device time of a launch.  For update and swap the bytes they move, from shapes (update reads avg and
          src and writes avg: 12 bytes per element; swap reads and writes both: 16), over that time, as a share of the
          8 TB/s HBM peak.  update is timed in its three states: active with a general coefficient, active as the first
          copy (coef 1: src read, avg written, 8 bytes per element), and inactive (every workgroup returns after one word).
  train   clips/s of train.GraphedTrainStep with DeviceAdamW inside the graph at fp32 config 2, variant A without an
          averager against variant B with WeightAverage(decay=0.999), two models in one process, windows alternated
          A B A B ..., `--repeats` each; host clock around a window that ends in a synchronise.  The spread of a variant is
          (max - min) / median over its windows.

  python tools/wavg_lab.py [--only launch] [--launches 400] [--txt profiles/wavg_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("launch", 240), ("train", 420))                                        # (part, time limit in seconds)
CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                       # bench.py CFG (BASELINE configs[1])
HBM_PEAK = 8.0e12


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, importlib.import_module("sl-hwgat_amd.train"), torch.device("cuda:0")


def _model(hw, torch, dev, c, dtype):
    torch.manual_seed(1001)
    hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, num_kps=c["nW"] * 16, embed_dim=c["d0"])
    model = hw.Model(*hp.get_model_params()).to(dev)
    model.use_part_table(hw.part_table(c["J"], c["nW"]))
    model.set_activation_dtype(dtype)
    model.train()
    return model


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def part_launch(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    _lib = importlib.import_module("sl-hwgat_amd._lib")
    assert args.launches % args.chain == 0
    model = _model(hw, torch, DEV, CFG, torch.float32)
    avg = optim.WeightAverage(model, decay=0.999)
    avg.update()                                             # binds, pushes, copies
    with torch.no_grad():
        for p in model.parameters():                         # weights that differ from the average
            p.add_(torch.randn_like(p) * 1e-3)
    n_el = sum(s.numel() for s in avg._shadow)
    aligned = sum(1 for s, t in zip(avg._shadow, avg._live()) if (s.data_ptr() | t.data_ptr()) % 16 == 0)
    st, tb = _lib.ptr(avg._state), _lib.ptr(avg._table)
    words = avg._state

    def advance():
        _lib.call("hwgat_wavg_advance", st, None, _lib.stream())

    def update():
        _lib.call("hwgat_wavg_update", tb, avg._n, st, avg._total, _lib.stream())

    def swap():
        _lib.call("hwgat_wavg_swap", tb, avg._n, avg._total, _lib.stream())

    def both():
        avg.update()

    def put(coef, active):
        words[optim.W_COEF] = coef
        words[optim.W_ACTIVE] = active

    def graph_of(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.chain):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        return graph

    def window(fn, graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter()
        if graph is not None:
            for _ in range(args.launches // args.chain):
                graph.replay()
        else:
            for _ in range(args.launches):
                fn()
        t1 = time.perf_counter()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.launches, (t1 - t0) * 1e6 / args.launches   # us: events, host

    print(f"launch: HWGATE config 2, {len(avg._shadow)} averaged tensors ({aligned} with both addresses 16-byte aligned), "
          f"{n_el} elements, {avg._total} workgroups of {optim.CHUNK} elements; us per launch, {args.launches} launches per "
          f"window, {args.repeats} windows (median; spread = (max - min) / median)")
    # (name, launch, in a graph, bytes per element, (coef, active) put into the state block first or None)
    rows = [("advance", advance, True, 0, None),
            ("update, coef 0.001", update, True, 12, (0.001, 1.0)),
            ("update, coef 1 (the first copy)", update, True, 8, (1.0, 1.0)),
            ("update, inactive", update, True, 0, (0.0, 0.0)),
            ("swap", swap, True, 16, None),
            ("advance + update (WeightAverage.update)", both, False, 12, None)]
    for name, fn, chain, per_el, state in rows:
        if state is not None:
            put(*state)
        graph = graph_of(fn) if chain else None
        fn()
        torch.cuda.synchronize()
        dev = [window(fn, graph)[0] for _ in range(args.repeats)] if graph is not None else None
        eager = [window(fn, None) for _ in range(args.repeats)]
        line = f"  {name:40s}"
        if dev is not None:
            line += f"  device {statistics.median(dev):8.1f} us (spread {100 * _spread(dev):.1f} %)"
        ev, host = [e for e, _ in eager], [h for _, h in eager]
        line += (f"  eager {statistics.median(ev):8.1f} us (spread {100 * _spread(ev):.1f} %)"
                 f"  issue {statistics.median(host):8.1f} us (spread {100 * _spread(host):.1f} %)")
        if per_el and dev is not None:
            us = statistics.median(dev)
            share = per_el * n_el / (us * 1e-6) / HBM_PEAK
            line += (f"  {per_el * n_el / 1e6:.1f} MB: {per_el * n_el / us / 1e6:.2f} TB/s, {100 * share:.1f} % of the 8 TB/s "
                     f"HBM peak ({'at or above' if share >= 0.40 else 'BELOW'} the 0.40 mark)")
        print(line, flush=True)
    return 0


def part_train(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    print("train: clips/s of train.GraphedTrainStep with DeviceAdamW inside the graph at fp32 config 2, A = no averager, "
          "B = WeightAverage(decay=0.999); windows alternated in one process (median; spread = (max - min) / median)")
    variants, c, steps = {}, CFG, args.train_steps
    for name in ("A", "B"):
        model = _model(hw, torch, DEV, c, torch.float32)
        g = torch.Generator(device=DEV).manual_seed(7)
        x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
        y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
        o = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
        if name == "B":
            o.averager = optim.WeightAverage(model, decay=0.999)
        s = train.GraphedTrainStep(model, o, x, y)
        for _ in range(5):
            s(x, y)
        variants[name] = (s, x, y, o)
    torch.cuda.synchronize()
    rate = {n: [] for n in variants}
    for _ in range(args.repeats):
        for name, (s, x, y, _) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s(x, y)
            torch.cuda.synchronize()
            rate[name].append(steps * c["B"] / (time.perf_counter() - t0))
    a, b = statistics.median(rate["A"]), statistics.median(rate["B"])
    avg = variants["B"][3].averager
    for name in ("A", "B"):
        print(f"  {name} windows, ms per step: " + ", ".join(f"{1e3 * c['B'] / r:.3f}" for r in rate[name]))
    print(f"  fp32 config 2  A {a:9.0f} clips/s (spread {100 * _spread(rate['A']):.2f} %)   B {b:9.0f} clips/s "
          f"(spread {100 * _spread(rate['B']):.2f} %)   B / A {b / a:.4f}   step {1e3 * c['B'] / a:.3f} -> "
          f"{1e3 * c['B'] / b:.3f} ms, {steps} steps per window, {args.repeats} windows; loss A "
          f"{float(variants['A'][0].loss):.4f} B {float(variants['B'][0].loss):.4f}; counters {avg.counters()}, "
          f"coefficient {float(avg.coef):.6f}", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="launches per window (part launch)")
    ap.add_argument("--chain", type=int, default=50, help="launches held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps per window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "wavg_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    ap.add_argument("--only", choices=[p for p, _ in PARTS], help="run this part alone (still as a child process)")
    args = ap.parse_args()
    if args.part:
        return {"launch": part_launch, "train": part_train}[args.part](args)
    text, ok = [], True
    for part, limit in PARTS:                                 # this process never opens the GPU: every part is a fresh child
        if args.only not in (None, part):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--launches", str(args.launches), "--chain", str(args.chain), "--train-steps", str(args.train_steps),
               "--repeats", str(args.repeats)]
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
