#!/usr/bin/env python3
"""What the HIP optimizers (optim.DeviceAdamW / DeviceSGD / DeviceNAdam, csrc/optim.hip) cost and
buy, measured on the device.  Two parts, each a child process of its own under its own time limit (a part that fails ends
the run; nothing is started after it):

  step   one optimizer step on the trainable parameters of HWGATE at BASELINE config 2 and of HGATE (random gradients),
         once per class (or for the one `--optimizer adamw|sgd|nadam` names): torch's fastest variant of the class against
         the device class, alternated, `--repeats` windows each.  Torch's variant: AdamW(fused=True, capturable=True); SGD(fused=True)
         (with `--momentum`, default 0 as in the reference's call); NAdam(foreach=True, capturable=True) -- it has no
         fused form.
           device   HIP events around replays of ONE graph that holds `--chain` steps back to back (no host between the
                    kernels), `--steps` steps per window: the device time of a step
           eager    HIP events around `--steps` steps issued from Python: the larger of issue time and device time
           issue    perf_counter around the same calls, no synchronise inside the window: the host time of one call
         and for the device class the bytes its step kernel moves, from shapes (AdamW and NAdam: p, g, m, v read; p, m, v
         written: 28 bytes per element; SGD: 12 without momentum, 20 with), over the device time of its step (which
         includes the one-block advance kernel), as a share of the 8 TB/s HBM peak.
  train  clips/s of train.GraphedTrainStep at fp32 config 2, bf16 config 3 and HGATE bf16, variant A (torch's fused AdamW
         issued after every replay: bench.py --graph) against variant B (DeviceAdamW inside the graph), two models in one
         process, windows alternated A B A B ..., `--repeats` each; host clock around a window that ends in a synchronise.
         The spread of a variant is (max - min) / median over its windows.

  python tools/optim_lab.py [--only step] [--optimizer sgd [--momentum 0.9]] [--steps 400] [--txt profiles/optim_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("step", 240), ("train", 540))                                          # (part, time limit in seconds)
CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                       # bench.py CFG (BASELINE configs[1])
CFG_HGATE = dict(B=64, T=128, J=29, K=29, C=2, d0=128, nc=2002)                 # bench.py CFG_HGATE
HBM_PEAK = 8.0e12
CLASSES = ("adamw", "sgd", "nadam")


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, importlib.import_module("sl-hwgat_amd.train"), torch.device("cuda:0")


def _model(hw, torch, dev, kind, dtype):
    torch.manual_seed(1001)
    if kind == "hgate":
        c = CFG_HGATE
        hp = hw.HGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, embed_dim=c["d0"])
        model = hw.HGATEModel(*hp.get_model_params()).to(dev)
    else:
        c = CFG
        hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, num_kps=c["nW"] * 16, embed_dim=c["d0"])
        model = hw.Model(*hp.get_model_params()).to(dev)
        model.use_part_table(hw.part_table(c["J"], c["nW"]))
    model.set_activation_dtype(dtype)
    model.train()
    return model, c


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def _optimizer(torch, optim, args, name, ps):
    """`name` "torch": torch's fastest variant of the chosen class; "device": this backend's class"""
    if args.optimizer == "adamw":
        return (torch.optim.AdamW(ps, lr=5e-4, fused=True, capturable=True) if name == "torch"
                else optim.DeviceAdamW(ps, lr=5e-4))
    if args.optimizer == "sgd":
        return (torch.optim.SGD(ps, lr=5e-4, momentum=args.momentum, fused=True) if name == "torch"
                else optim.DeviceSGD(ps, lr=5e-4, momentum=args.momentum))
    return (torch.optim.NAdam(ps, lr=5e-4, foreach=True, capturable=True) if name == "torch"
            else optim.DeviceNAdam(ps, lr=5e-4))


def part_step(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    assert args.steps % args.chain == 0
    for kind in ("hwgate", "hgate"):
        model, _ = _model(hw, torch, DEV, kind, torch.float32)
        shapes = [tuple(p.shape) for p in model.parameters() if p.requires_grad]
        n_el = sum(p.numel() for p in model.parameters() if p.requires_grad)
        del model
        g = torch.Generator(device=DEV).manual_seed(5)
        opts = {}
        for name in ("torch", "device"):
            ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=g) * 0.05) for s in shapes]
            for p in ps:
                p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-2
            o = _optimizer(torch, optim, args, name, ps)
            for _ in range(20):                                  # warm-up: state, code objects, the table
                o.step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()                       # `chain` steps back to back, for the device time
            if name == "device":
                o.begin_capture()
            with torch.cuda.graph(graph):
                for _ in range(args.chain):
                    o.step()
            keep = o.end_capture() if name == "device" else None
            graph.replay()
            torch.cuda.synchronize()
            opts[name] = (o, graph, keep, ps)

        def window(name, how):
            o, graph, _, _ = opts[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            if how == "device":
                for _ in range(args.steps // args.chain):
                    graph.replay()
            else:
                for _ in range(args.steps):
                    o.step()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / args.steps, (t1 - t0) * 1e6 / args.steps      # us per step: events, host

        res = {(n, h): [] for n in opts for h in ("device", "eager", "issue")}
        for _ in range(args.repeats):
            for name in opts:
                res[name, "device"].append(window(name, "device")[0])
                ev, host = window(name, "eager")
                res[name, "eager"].append(ev)
                res[name, "issue"].append(host)
        n_t = len(shapes)
        blocks = sum(-(-torch.Size(s).numel() // optim.CHUNK) for s in shapes)
        what = args.optimizer + (f" (momentum {args.momentum})" if args.optimizer == "sgd" else "")
        print(f"step: {what}, {kind}, {n_t} trainable tensors, {n_el} elements, {blocks} workgroups of {optim.CHUNK} elements; "
              f"us per optimizer step, {args.steps} steps per window, {args.repeats} windows (median; spread = (max - min) / median)")
        for name in opts:
            line = f"  {name:6s}"
            for how in ("device", "eager", "issue"):
                v = res[name, how]
                line += f"  {how} {statistics.median(v):8.1f} us (spread {100 * _spread(v):.1f} %)"
            print(line)
        dev_us = statistics.median(res["device", "device"])
        per_el = 28 if args.optimizer != "sgd" else (20 if args.momentum else 12)
        nbytes = per_el * n_el
        print(f"  the step kernel moves {nbytes / 1e6:.1f} MB per step ({per_el} bytes per element): over the device time of "
              f"the device class's step {nbytes / dev_us / 1e6:.2f} TB/s, {100 * nbytes / (dev_us * 1e-6) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
        del opts
    return 0


def part_train(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    print("train: clips/s of train.GraphedTrainStep, A = torch AdamW(fused, capturable) issued after the replay, "
          "B = DeviceAdamW inside the graph; windows alternated in one process (median; spread = (max - min) / median)")
    for label, kind, dtype, steps in (("fp32 config 2", "hwgate", torch.float32, args.train_steps),
                                      ("bf16 config 3", "hwgate", torch.bfloat16, 4 * args.train_steps),
                                      ("HGATE bf16", "hgate", torch.bfloat16, 4 * args.train_steps)):
        variants = {}
        for name in ("A", "B"):
            model, c = _model(hw, torch, DEV, kind, dtype)
            g = torch.Generator(device=DEV).manual_seed(7)
            x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=DEV, generator=g)
            y = torch.randint(0, c["nc"], (c["B"],), device=DEV, generator=g)
            ps = [p for p in model.parameters() if p.requires_grad]
            o = torch.optim.AdamW(ps, lr=5e-4, fused=True, capturable=True) if name == "A" else optim.DeviceAdamW(ps, lr=5e-4)
            s = train.GraphedTrainStep(model, o, x, y)
            for _ in range(5):
                s(x, y)
            variants[name] = (s, x, y, c["B"])
        torch.cuda.synchronize()
        rate = {n: [] for n in variants}
        for _ in range(args.repeats):
            for name, (s, x, y, B) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    s(x, y)
                torch.cuda.synchronize()
                rate[name].append(steps * B / (time.perf_counter() - t0))
        a, b = statistics.median(rate["A"]), statistics.median(rate["B"])
        print(f"  {label:14s} A {a:9.0f} clips/s (spread {100 * _spread(rate['A']):.2f} %)   B {b:9.0f} clips/s "
              f"(spread {100 * _spread(rate['B']):.2f} %)   B / A {b / a:.4f}   step {1e3 * variants['A'][3] / a:.2f} -> "
              f"{1e3 * variants['B'][3] / b:.2f} ms, {steps} steps per window, {args.repeats} windows; "
              f"loss A {float(variants['A'][0].loss):.4f} B {float(variants['B'][0].loss):.4f}")
        del variants
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400, help="optimizer steps per window (part step)")
    ap.add_argument("--chain", type=int, default=50, help="optimizer steps held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps per fp32 window (bf16: four times as many)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "optim_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    ap.add_argument("--optimizer", choices=CLASSES, help="class of the step part (default: one step part per class)")
    ap.add_argument("--momentum", type=float, default=0.0, help="SGD momentum of the step part (the reference's call: 0)")
    ap.add_argument("--only", choices=[p for p, _ in PARTS], help="run this part alone (still as child processes)")
    args = ap.parse_args()
    if args.part:
        return {"step": part_step, "train": part_train}[args.part](args)
    text, ok = [], True
    # this process never opens the GPU: every part, and every class of the step part, is a fresh child
    runs = [(part, limit, cls) for part, limit in PARTS if args.only in (None, part)
            for cls in ((args.optimizer,) if args.optimizer else CLASSES if part == "step" else CLASSES[:1])]
    for part, limit, cls in runs:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--steps", str(args.steps), "--chain", str(args.chain), "--train-steps", str(args.train_steps),
               "--repeats", str(args.repeats), "--optimizer", cls, "--momentum", str(args.momentum)]
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
