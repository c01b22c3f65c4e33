#!/usr/bin/env python3
"""What the input modalities (csrc/modality.hip) and the score ensemble (csrc/ensemble.hip, ensemble.Ensemble) cost, measured
on the device.  Three parts, each a child process of its own under its own time limit (a part that fails ends the run;
nothing is started after it):

  kernels  the two kernels alone: HIP events around replays of ONE graph that holds `--chain` calls back to back.  The
           modality kernel at B 64, T 128, J 67, C 2 for each kind (the table is the chain over 67 joints); the fuse kernel
           at M 4, B 64, C 2002 in both modes, and -- when the kernel-lab library is there (`python sl-hwgat_amd/build.py
           --lab`) -- the same through it with one wave per row and with a workgroup of 256 per row.
  train    ms per step of a graphed HWGATE bf16 train step (B 64, T 128, 29 raw joints through part_table(29), 2002 classes,
           DeviceAdamW) with `input_modality` unset against set to bone motion: two graphs in one process, windows
           alternated.
  eval     ms per evaluation of a four-member graphed Ensemble (one HWGATE per modality, bf16) against the sum of its
           members' own graphed evaluations, alternated in one process.

  python tools/ensemble_lab.py [--only kernels] [--txt profiles/ensemble_lab.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("kernels", 180), ("train", 300), ("eval", 300))                        # (part, time limit in seconds)
CFG = dict(B=64, T=128, J=29, C=2, d0=128, nc=2002)
LAB = os.path.join(ROOT, "sl-hwgat_amd", "libhwgat_hip_lab.so")


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, torch.device("cuda:0")


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def _device_us(torch, fn, args):
    """us per call of fn: replays of a graph of `chain` calls between two events"""
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
    return statistics.median(us), _spread(us)


def part_kernels(args):
    torch, hw, DEV = _gpu()
    HF = hw.functional
    assert args.launches % args.chain == 0
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(64, 128, 67, 2, device=DEV, generator=g)
    out = torch.empty_like(x)
    table = torch.tensor([max(j - 1, 0) for j in range(67)], dtype=torch.int32, device=DEV)
    mb = 2 * x.numel() * 4 / 1e6
    print(f"kernels [{args.label}]: us per call, {args.launches} calls per window, {args.repeats} windows (median; spread = "
          f"(max - min) / median); device time = replays of a graph of {args.chain} calls")
    print(f"  hwgat_modality, x {tuple(x.shape)} fp32 ({mb:.1f} MB read + written)")
    for kind in HF.MOD_KINDS:
        us, sp = _device_us(torch, lambda: HF.modality(x, table, kind, out=out), args)
        print(f"    {kind:12s} {us:7.2f} us (spread {100 * sp:.1f} %), {mb / us * 1e3:.0f} GB/s", flush=True)
    M, B, C = 4, 64, 2002
    z = torch.randn(M, B, C, device=DEV, generator=g) * 10
    w = torch.full((M,), 0.25, device=DEV)
    fused = torch.empty(B, C, device=DEV)
    print(f"  hwgat_ens_fuse, z {tuple(z.shape)} fp32, equal weights (the library's choice: one wave per row up to 512 "
          f"classes, a workgroup of 256 above)")
    for mode in HF.ENS_MODES:
        us, sp = _device_us(torch, lambda: HF.ens_fuse(z, w, mode, out=fused), args)
        print(f"    {mode:12s} {us:7.2f} us (spread {100 * sp:.1f} %)", flush=True)
    if not os.path.exists(LAB):
        print("  one wave against a workgroup per row at C = 2002: not measured (no kernel-lab library)")
        return 0
    lab = ctypes.CDLL(LAB)
    assert lab.hwgat_is_lab_build() == 1, "not the LAB library: build it with `python sl-hwgat_amd/build.py --lab`"
    lab.hwgat_ens_fuse.argtypes = hw._lib._SIGS["hwgat_ens_fuse"]
    for threads in ("64", "256"):
        os.environ["HWGAT_ENS_THREADS"] = threads
        for code, mode in enumerate(HF.ENS_MODES):
            def fn():
                rc = lab.hwgat_ens_fuse(z.data_ptr(), w.data_ptr(), fused.data_ptr(), M, B, C, code,
                                        torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            us, sp = _device_us(torch, fn, args)
            print(f"    lab, {threads:>3s} lanes per row, {mode:6s} {us:7.2f} us (spread {100 * sp:.1f} %)", flush=True)
    return 0


def _hwgate(torch, hw, DEV, seed, modality_kind=None, train=False):
    c = CFG
    modality = importlib.import_module("sl-hwgat_amd.modality")
    torch.manual_seed(seed)
    table = hw.part_table(c["J"])
    hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], DEV, num_kps=table.numel(), embed_dim=c["d0"])
    m = hw.Model(*hp.get_model_params()).to(DEV)
    m.use_part_table(table)
    m.set_activation_dtype(torch.bfloat16)
    if modality_kind not in (None, "joint"):
        parents = modality.parents_from_edges(hw.STGCNParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"]).edges_, c["J"])
        m.set_input_modality(modality.Modality(modality_kind, parents))
    return m.train() if train else m.eval()


def _alternate(torch, variants, steps, repeats):
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
    return ms


def part_train(args):
    torch, hw, DEV = _gpu()
    train = importlib.import_module("sl-hwgat_amd.train")
    optim = importlib.import_module("sl-hwgat_amd.optim")
    c = CFG
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
    y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
    steps = {}
    for name, kind in (("plain", None), ("bone_motion", "bone_motion")):
        m = _hwgate(torch, hw, DEV, 1001, kind, train=True)
        steps[name] = train.GraphedTrainStep(m, optim.DeviceAdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4), x, y)
    ms = _alternate(torch, {n: (lambda s=s: s(x, y)) for n, s in steps.items()}, args.train_steps, args.repeats)
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(f"train [{args.label}]: ms per graphed HWGATE bf16 train step, B = {c['B']}, T = {c['T']}, {c['J']} raw joints, "
          f"{c['nc']} classes, DeviceAdamW; input_modality unset against bone motion; {args.train_steps} steps per window, "
          f"{args.repeats} windows, alternated in one process (median; spread = (max - min) / median)")
    for name in steps:
        print(f"  {name:12s} {med[name]:8.3f} ms (spread {100 * _spread(ms[name]):.2f} %; windows " +
              ", ".join(f"{v:.3f}" for v in ms[name]) + ")", flush=True)
    print(f"  bone_motion - plain {1e3 * (med['bone_motion'] - med['plain']):+.1f} us", flush=True)
    return 0


def part_eval(args):
    torch, hw, DEV = _gpu()
    serve = importlib.import_module("sl-hwgat_amd.serve")
    ensemble = importlib.import_module("sl-hwgat_amd.ensemble")
    c = CFG
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
    kinds = hw.functional.MOD_KINDS
    alone = [serve.GraphedEval(_hwgate(torch, hw, DEV, 2000 + i, kind), x) for i, kind in enumerate(kinds)]
    together = serve.GraphedEval(ensemble.Ensemble([_hwgate(torch, hw, DEV, 2000 + i, kind) for i, kind in enumerate(kinds)]), x)
    variants = {f"member {kind}": r.run for kind, r in zip(kinds, alone)}
    variants["ensemble"] = together.run
    ms = _alternate(torch, variants, args.train_steps, args.repeats)
    med = {n: statistics.median(v) for n, v in ms.items()}
    print(f"eval [{args.label}]: ms per graphed evaluation, HWGATE bf16, B = {c['B']}, T = {c['T']}, {c['J']} raw joints, {c['nc']} "
          f"classes; the four members alone and a four-member Ensemble (prob mode) of models of the same weights; "
          f"{args.train_steps} evaluations per window, {args.repeats} windows, alternated in one process")
    for name in variants:
        print(f"  {name:20s} {med[name]:8.3f} ms (spread {100 * _spread(ms[name]):.2f} %)", flush=True)
    parts = sum(v for n, v in med.items() if n != "ensemble")
    print(f"  ensemble - sum of its members {1e3 * (med['ensemble'] - parts):+.1f} us (sum {parts:.3f} ms)", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="calls per window (part kernels)")
    ap.add_argument("--chain", type=int, default=50, help="calls held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="steps / evaluations per window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "ensemble_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    ap.add_argument("--only", choices=[p for p, _ in PARTS], help="run this part alone (still as a child process)")
    args = ap.parse_args()
    if args.part:
        return {"kernels": part_kernels, "train": part_train, "eval": part_eval}[args.part](args)
    text, ok, ran = [], True, set()
    for part, limit in PARTS:                                 # this process never opens the GPU: every part is a fresh child
        if args.only not in (None, part):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--launches", str(args.launches), "--chain", str(args.chain), "--train-steps", str(args.train_steps),
               "--repeats", str(args.repeats), "--label", args.label]
        res = subprocess.run(cmd, capture_output=True, text=True)
        text += res.stdout.splitlines()
        print(res.stdout, end="", flush=True)
        ran.add(part)
        if res.returncode != 0:
            ok = False
            text.append(f"part {part} ended with status {res.returncode}; nothing was started after it")
            print(text[-1] + "\n" + res.stderr[-2000:], flush=True)
            break
    text += [f"{part}: not measured" for part, _ in PARTS if part not in ran]
    with open(args.txt, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
