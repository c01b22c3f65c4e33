#!/usr/bin/env python3
"""What the HIP classifier head (csrc/head.hip, functional.head_linear) costs against the library head it can replace,
measured on the device.  Two parts, each a child process of its own under its own time limit (a part that fails ends the
run; nothing is started after it):

  kernels  device time per launch of hwgat_head_fwd / hwgat_head_bwd_dx / hwgat_head_bwd_dw against torch's F.linear and
           the three launches of its backward (mm for dX, mm for dW, sum for db), for M in {1, 4, 64, 256}, N in {226, 2002},
           K in {256, 512}.  Both variants run in one process after a warm-up of every shape, windows alternated
           ours / library, `--repeats` windows each, every window shown; HIP events around replays of ONE graph that
           holds `--chain` launches back to back (no host between the kernels: the device time of a launch, the gap to
           the next graph node included), `--calls` launches per window.
  serve    a B = 1 bf16 HWGATE (BASELINE config 2 shapes, 2002 classes) serve.GraphedEval replay with `hip_head` off and
           on: two models with the same weights in one process, windows alternated, HIP events around `--replays` replays.

  python tools/head_lab.py [--calls 2000] [--chain 50] [--txt profiles/head_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("kernels", 300), ("serve", 240))                                       # (part, time limit in seconds)
SHAPES = [(M, N, K) for K in (256, 512) for N in (226, 2002) for M in (1, 4, 64, 256)]
CFG = dict(T=128, J=67, nW=5, C=2, d0=128, nc=2002)                             # bench.py CFG (BASELINE configs[1])


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, torch.device("cuda:0")


def _chain(torch, fn, chain):
    """a graph of `chain` calls of fn back to back; its replay"""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(chain):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph.replay


def _window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls                                       # us per call


def _fmt(v):
    return f"{statistics.median(v):7.2f} [" + " ".join(f"{t:.2f}" for t in v) + "]"


def part_kernels(args):
    torch, hw, DEV = _gpu()
    HF, F = hw.functional, torch.nn.functional
    g = torch.Generator(device=DEV).manual_seed(3)
    assert args.calls % args.chain == 0
    reps = args.calls // args.chain
    print(f"kernels: us per launch (dw+db: per pair of library launches), HIP events around {reps} replays of a graph of "
          f"{args.chain} launches back to back, {args.repeats} windows per variant alternated ours / library in one process; "
          f"median [every window]")
    for M, N, K in SHAPES:
        x = torch.randn(M, K, device=DEV, generator=g)
        w = 0.02 * torch.randn(N, K, device=DEV, generator=g)
        b = 0.1 * torch.randn(N, device=DEV, generator=g)
        dy = torch.randn(M, N, device=DEV, generator=g)
        y, dx, dw, db = (torch.empty(s, device=DEV) for s in ((M, N), (M, K), (N, K), (N,)))
        ours = {"fwd": lambda: HF.head_forward(x, w, b, out=y),
                "dx": lambda: HF.head_backward_dx(dy, w, out=dx),
                "dw+db": lambda: HF.head_backward_dw(dy, x, out=dw, out_db=db)}

        def lib_dw():
            torch.mm(dy.t(), x, out=dw)
            torch.sum(dy, 0, out=db)
        lib = {"fwd": lambda: F.linear(x, w, b), "dx": lambda: torch.mm(dy, w, out=dx), "dw+db": lib_dw}
        for fn in list(ours.values()) + list(lib.values()):                      # warm-up: code objects, the library's choice
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        ours = {k: _chain(torch, fn, args.chain) for k, fn in ours.items()}
        lib = {k: _chain(torch, fn, args.chain) for k, fn in lib.items()}
        # the two variants must agree before their times mean anything (the library's order of summation differs)
        err = float((HF.head_forward(x, w, b) - F.linear(x, w, b)).abs().max())
        res = {(v, k): [] for v in ("ours", "lib") for k in ours}
        for _ in range(args.repeats):
            for k in ours:
                res["ours", k].append(_window(torch, ours[k], reps) / args.chain)
                res["lib", k].append(_window(torch, lib[k], reps) / args.chain)
        print(f"  M {M:3d} N {N:4d} K {K:3d}   (largest |ours - library| of the logits {err:.2e})")
        for k in ours:
            o, l = statistics.median(res["ours", k]), statistics.median(res["lib", k])
            print(f"    {k:6s} ours {_fmt(res['ours', k])}   library {_fmt(res['lib', k])}   ours / library {o / l:.2f}")
    return 0


def part_serve(args):
    torch, hw, DEV = _gpu()
    serve = importlib.import_module("sl-hwgat_amd.serve")
    c = CFG
    runs = {}
    for name, flag in (("off", False), ("on", True)):
        torch.manual_seed(1001)
        hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], DEV, num_kps=c["nW"] * 16, embed_dim=c["d0"])
        model = hw.Model(*hp.get_model_params()).to(DEV)
        model.use_part_table(hw.part_table(c["J"], c["nW"]))
        model.set_activation_dtype(torch.bfloat16)
        model.eval()
        model.hip_head = flag
        x = torch.rand(1, c["T"], c["J"], c["C"], device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        runs[name] = serve.GraphedEval(model, x)
        for _ in range(20):
            runs[name].run()
    torch.cuda.synchronize()
    diff = float((runs["on"].static_out - runs["off"].static_out).abs().max())
    res = {n: [] for n in runs}
    for _ in range(args.repeats):
        for n, ge in runs.items():
            res[n].append(_window(torch, ge.run, args.replays))
    off, on = statistics.median(res["off"]), statistics.median(res["on"])
    print(f"serve: B = 1 bf16 HWGATE (T {c['T']}, {c['nW'] * 16} slots, {c['nc']} classes) GraphedEval replay, us per replay, HIP "
          f"events around {args.replays} replays, {args.repeats} windows per variant alternated; median [every window]")
    print(f"  hip_head off {_fmt(res['off'])}   on {_fmt(res['on'])}   on / off {on / off:.4f}   "
          f"largest |logit difference| {diff:.2e}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000, help="launches per window (part kernels)")
    ap.add_argument("--chain", type=int, default=50, help="launches held by the graph of a window (part kernels)")
    ap.add_argument("--replays", type=int, default=500, help="graph replays per window (part serve)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "head_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    args = ap.parse_args()
    if args.part:
        return {"kernels": part_kernels, "serve": part_serve}[args.part](args)
    text, ok = [], True
    for part, limit in PARTS:                  # this process never opens the GPU: every part is a fresh child
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--calls", str(args.calls), "--chain", str(args.chain), "--replays", str(args.replays), "--repeats", str(args.repeats)]
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
