#!/usr/bin/env python3
"""What knowledge distillation inside the train step (train.Distiller, hwgat_kd_* of csrc/loss_eval.hip) costs, measured
on the device.  Two parts, each a child process of its own under its own time limit (a part that fails ends the run; nothing
is started after it):

  launch  the distilled criterion's calls, each alone, on (64, 2002) fp32 logits beside the mixed criterion's in the same
          process: HIP events around replays of ONE graph that holds `--chain` calls back to back, `--launches` per window:
          the device time of a call.  kd_fwd with a mixer's records (five launches) and without (four), kd_bwd, against
          mbsce_fwd (four), bsce_fwd (three) and their backward.
  train   ms per step at B = 64, T = 128, 29 raw joints, 2002 classes, bf16 activations, three graphs in one process,
          windows alternated S T D S T D ..., `--repeats` each: S the HGATE student's GraphedTrainStep(ragged=True) with
          DeviceAdamW alone, T the HWGATE teacher's (use_part_table(part_table(29))) serve.GraphedEval forward alone, D the
          distilled GraphedTrainStep of the same student with that teacher.  Host clock around a window that ends in a
          synchronise.  The expectation to check is D = S + T; the line ends with D - (S + T).

  python tools/distill_lab.py [--only launch] [--txt profiles/distill_lab.txt]
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
CFG = dict(B=64, T=128, J=29, C=2, d0=128, nc=2002)                             # bench.py CFG_HGATE


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
    y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
    y_b = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
    lam = torch.rand(c["B"], device=DEV, generator=g)
    z = torch.randn(c["B"], c["nc"], device=DEV, generator=g)
    u = 3 * torch.randn(c["B"], c["nc"], device=DEV, generator=g)
    rows = torch.full((1,), c["B"], dtype=torch.int32, device=DEV)
    g_up = torch.ones(1, device=DEV)
    st = HF.kd_state(DEV)
    HF.kd_set(st, 0.5, 4.0)
    fwd = HF.bsce_forward(z, y, 0.01, rows, 0)
    mfwd = HF.mbsce_forward(z, y, y_b, lam, 0.01, rows, 0)
    kfwd = HF.kd_forward(z, u, y, y_b, lam, st, 0.01, rows, 0)
    k1fwd = HF.kd_forward(z, u, y, None, None, st, 0.01, rows, 0)
    dz = torch.empty_like(z)
    calls = [("bsce_fwd (3 launches)", lambda: HF.bsce_forward(z, y, 0.01, rows, 0, out=fwd)),
             ("mbsce_fwd (4 launches)", lambda: HF.mbsce_forward(z, y, y_b, lam, 0.01, rows, 0, out=mfwd)),
             ("kd_fwd, labels (4 launches)", lambda: HF.kd_forward(z, u, y, None, None, st, 0.01, rows, 0, out=k1fwd)),
             ("kd_fwd, pairs (5 launches)", lambda: HF.kd_forward(z, u, y, y_b, lam, st, 0.01, rows, 0, out=kfwd)),
             ("bsce_bwd", lambda: HF.bsce_backward(z, y, fwd[2], g_up, 0.01, rows, 0, out=dz)),
             ("mbsce_bwd", lambda: HF.mbsce_backward(z, y, y_b, lam, mfwd[2], g_up, 0.01, rows, 0, out=dz)),
             ("kd_bwd, labels", lambda: HF.kd_backward(z, u, y, None, None, st, k1fwd[2], k1fwd[9], k1fwd[10], g_up, 0.01, rows, 0,
                                                       out=dz)),
             ("kd_bwd, pairs", lambda: HF.kd_backward(z, u, y, y_b, lam, st, kfwd[2], kfwd[9], kfwd[10], g_up, 0.01, rows, 0,
                                                      out=dz))]
    print(f"launch [{args.label}]: us per call, {args.launches} calls per window, {args.repeats} windows (median; spread = "
          f"(max - min) / median); device time = replays of a graph of {args.chain} calls; logits and teacher {tuple(z.shape)} "
          f"fp32, alpha 0.5, tau 4")
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
    serve = importlib.import_module("sl-hwgat_amd.serve")
    c, steps = CFG, args.train_steps
    ds = {"src_len": c["T"], "num_class": c["nc"]}
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
    y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)

    def student():
        torch.manual_seed(1001)
        hp = hw.HGATEParams(ds, c["C"], DEV, embed_dim=c["d0"])
        m = hw.HGATEModel(*hp.get_model_params()).to(DEV)
        m.set_activation_dtype(torch.bfloat16)
        m.train()
        return m, optim.DeviceAdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4)

    def teacher():
        torch.manual_seed(1002)
        table = hw.part_table(c["J"])
        hp = hw.HWGATEParams(ds, c["C"], DEV, num_kps=table.numel(), embed_dim=c["d0"])
        m = hw.Model(*hp.get_model_params()).to(DEV)
        m.use_part_table(table)
        m.set_activation_dtype(torch.bfloat16)
        return m.eval()

    m_s, o_s = student()
    S = train.GraphedTrainStep(m_s, o_s, x, y, ragged=True)
    T = serve.GraphedEval(teacher(), x)
    m_d, o_d = student()
    distiller = train.Distiller(teacher(), alpha=0.5, temperature=4.0)
    D = train.GraphedTrainStep(m_d, o_d, x, y, ragged=True, distiller=distiller)
    variants = {"S": lambda: S(x, y), "T": T.run, "D": lambda: D(x, y)}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    print(f"train [{args.label}]: ms per step, B = {c['B']}, T = {c['T']}, {c['J']} raw joints, {c['nc']} classes, bf16; S = HGATE "
          f"GraphedTrainStep(ragged=True) with DeviceAdamW, T = HWGATE (part_table({c['J']})) GraphedEval forward, D = the distilled "
          f"step of S with T's model as the teacher; {steps} steps per window, {args.repeats} windows, alternated in one process "
          f"(median; spread = (max - min) / median)")
    ms = {n: [] for n in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
    med = {n: statistics.median(v) for n, v in ms.items()}
    for name in variants:
        print(f"  {name} {med[name]:8.3f} ms (spread {100 * _spread(ms[name]):.2f} %; windows " +
              ", ".join(f"{v:.3f}" for v in ms[name]) + ")", flush=True)
    print(f"  D - (S + T) {med['D'] - med['S'] - med['T']:+.3f} ms; S {c['B'] / med['S'] * 1e3:.0f} clips/s, D "
          f"{c['B'] / med['D'] * 1e3:.0f} clips/s; loss S {float(S.loss):.4f} D {float(D.loss):.4f} kd {float(D.kd):.4f} "
          f"agree {int(D.agree)} of {c['B']}", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="calls per window (part launch)")
    ap.add_argument("--chain", type=int, default=50, help="calls held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="steps per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "distill_lab.txt"))
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
               "--repeats", str(args.repeats), "--label", args.label]
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
