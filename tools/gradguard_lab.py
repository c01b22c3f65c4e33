#!/usr/bin/env python3
"""What the gradient guard (optim.GradGuard, csrc/grad_guard.hip) costs, measured on the device.  Two parts, each a child
process of its own under its own time limit (a part that fails ends the run; nothing is started after it):

  launch  the guard's partial, finish and scale launches over the real parameter table of HWGATE at BASELINE config 2 and
          at config 5 (random gradients), each alone: HIP events around replays of ONE graph that holds `--chain` launches
          back to back, `--launches` per window: the device time of a launch.  For partial and scale the bytes they move,
          from shapes (partial reads g: 4 bytes per element; scale reads and writes it: 8), over that time, as a share of
          the 8 TB/s HBM peak.  Against them torch.nn.utils.clip_grad_norm_(foreach=True) on the same gradients: HIP
          events around calls issued from Python (the larger of issue time and device time) and, where torch can capture
          it, around replays of a graph of `--chain` calls.
  train   clips/s of train.GraphedTrainStep with DeviceAdamW inside the graph at fp32 config 2 and bf16 config 3, variant
          A without a guard against variant B with GradGuard(max_norm=1, "skip"), two models in one process, windows
          alternated A B A B ..., `--repeats` each; host clock around a window that ends in a synchronise.  The spread of
          a variant is (max - min) / median over its windows.

  python tools/gradguard_lab.py [--only launch] [--launches 400] [--txt profiles/gradguard_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("launch", 300), ("train", 540))                                        # (part, time limit in seconds)
CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                       # bench.py CFG (BASELINE configs[1])
CFG5 = dict(B=256, T=256, J=133, nW=7, C=3, d0=256, nc=2002)                    # bench.py CFG5 (BASELINE configs[4])
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
    for label, c in (("config 2", CFG), ("config 5", CFG5)):
        model = _model(hw, torch, DEV, c, torch.float32)
        shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
        del model
        g = torch.Generator(device=DEV).manual_seed(5)
        ps = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-2
        n_el = sum(p.numel() for p in ps)
        guard = optim.GradGuard()                                # max_norm inf: the scale multiplies by 1, bits unchanged
        optim.clip_grad_norm_(ps, guard)
        table, _ = guard._clip
        st, ws = _lib.ptr(guard._state), _lib.ptr(table.guard_ws)

        def partial():
            _lib.call("hwgat_gguard_partial", _lib.ptr(table.buf), table.n, st, ws, table.total, _lib.stream())

        def finish():
            _lib.call("hwgat_gguard_finish", ws, table.total, st, _lib.stream())

        def scale():
            _lib.call("hwgat_gguard_scale", _lib.ptr(table.buf), table.n, st, table.total, _lib.stream())

        def guard_all():
            optim.clip_grad_norm_(ps, guard)

        def torch_clip():
            torch.nn.utils.clip_grad_norm_(ps, 1e30, foreach=True)

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

        print(f"launch: HWGATE {label}, {len(shapes)} trainable tensors, {n_el} elements, {table.total} workgroups of "
              f"{optim.CHUNK} elements; us per launch, {args.launches} launches per window, {args.repeats} windows "
              f"(median; spread = (max - min) / median)")
        rows = [("partial", partial, True, 4), ("finish", finish, True, 0), ("scale", scale, True, 8),
                ("all three (optim.clip_grad_norm_)", guard_all, False, 12),
                ("torch clip_grad_norm_(foreach=True)", torch_clip, True, 0)]
        for name, fn, chain, per_el in rows:
            graph = None
            if chain:
                try:
                    graph = graph_of(fn)
                except Exception as exc:                          # noqa: BLE001 -- torch's own call may refuse a capture
                    torch.cuda.synchronize()
                    print(f"  {name}: not capturable ({type(exc).__name__}); eager only")
            fn()
            torch.cuda.synchronize()
            dev = [window(fn, graph)[0] for _ in range(args.repeats)] if graph is not None else None
            eager = [window(fn, None) for _ in range(args.repeats)]
            line = f"  {name:36s}"
            if dev is not None:
                line += f"  device {statistics.median(dev):8.1f} us (spread {100 * _spread(dev):.1f} %)"
            ev, host = [e for e, _ in eager], [h for _, h in eager]
            line += (f"  eager {statistics.median(ev):8.1f} us (spread {100 * _spread(ev):.1f} %)"
                     f"  issue {statistics.median(host):8.1f} us (spread {100 * _spread(host):.1f} %)")
            if per_el and dev is not None:
                us = statistics.median(dev)
                line += (f"  {per_el * n_el / 1e6:.1f} MB: {per_el * n_el / us / 1e6:.2f} TB/s, "
                         f"{100 * per_el * n_el / (us * 1e-6) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
            print(line, flush=True)
        del ps, guard
    return 0


def part_train(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    print("train: clips/s of train.GraphedTrainStep with DeviceAdamW inside the graph, A = no guard, B = GradGuard(max_norm=1, "
          "on_nonfinite='skip'); windows alternated in one process (median; spread = (max - min) / median)")
    for label, dtype, steps in (("fp32 config 2", torch.float32, args.train_steps),
                                ("bf16 config 3", torch.bfloat16, 4 * args.train_steps)):
        variants, c = {}, CFG
        for name in ("A", "B"):
            model = _model(hw, torch, DEV, c, dtype)
            g = torch.Generator(device=DEV).manual_seed(7)
            x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
            y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
            o = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
            if name == "B":
                o.guard = optim.GradGuard(max_norm=1.0, on_nonfinite="skip")
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
        guard = variants["B"][3].guard
        print(f"  {label:14s} A {a:9.0f} clips/s (spread {100 * _spread(rate['A']):.2f} %)   B {b:9.0f} clips/s "
              f"(spread {100 * _spread(rate['B']):.2f} %)   B / A {b / a:.4f}   step {1e3 * c['B'] / a:.2f} -> "
              f"{1e3 * c['B'] / b:.2f} ms, {steps} steps per window, {args.repeats} windows; loss A "
              f"{float(variants['A'][0].loss):.4f} B {float(variants['B'][0].loss):.4f}; last norm {float(guard.total_norm):.4f}, "
              f"coefficient {float(guard.clip_coef):.4f}, counters {guard.counters()}", flush=True)
        del variants
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="launches per window (part launch)")
    ap.add_argument("--chain", type=int, default=50, help="launches held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps per fp32 window (bf16: four times as many)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "gradguard_lab.txt"))
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
