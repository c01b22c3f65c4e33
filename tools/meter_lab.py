#!/usr/bin/env python3
"""What the train meters (train.TrainMeter, csrc/train_meter.hip) cost and what the epoch loop on top of them saves, measured
on the device.  Three parts, each a child process of its own under its own time limit (a part that fails ends the run;
nothing is started after it):

  launch  the meter's fold and close launches, each alone: HIP events around replays of ONE graph that holds `--chain`
          launches back to back, `--launches` per window: the device time of a launch; and the same launches issued
          eagerly (events and the host's issue time).  fold is timed without and with a guard block and with a step log.
  train   clips/s of train.GraphedTrainStep with DeviceAdamW inside the graph at fp32 config 2, variant A without a meter
          against variant B with TrainMeter(log_capacity=256), two models in one process, windows alternated A B A B ...,
          `--repeats` each; host clock around a window that ends in a synchronise.  The spread of a variant is
          (max - min) / median over its windows.
  loop    a 64-batch train epoch of HGATE and HWGATE, bf16 at B = 4 and fp32 at B = 64: variant R, a loop written like the
          reference's train() (utils.py:93-116: `loss.item()` and the correct count's `.cpu().tolist()` after every
          step) around a GraphedTrainStep(ragged=True), against variant M, train.EpochLoop.train_epoch (the same step
          with a meter, nothing read per batch) plus the one read of the closed epoch.  Two models in one process, windows
          alternated R M R M ..., `--repeats` each; host clock around a window that ends with the numbers on the host.

  python tools/meter_lab.py [--only launch] [--launches 400] [--txt profiles/meter_lab.txt]
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("launch", 180), ("train", 300), ("loop", 400))                         # (part, time limit in seconds)
CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                       # bench.py CFG (BASELINE configs[1])
CFG_HGATE = dict(B=64, T=128, J=29, K=29, C=2, d0=128, nc=2002)                 # bench.py CFG_HGATE


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


def _batch(torch, dev, c, B, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand(B, c["T"], c["J"], c["C"], device=dev, generator=g)
    y = torch.randint(0, c["nc"], (B,), device=dev, generator=g)
    return x, y


def _spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def part_launch(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    assert args.launches % args.chain == 0
    loss = torch.full((), 2.5, dtype=torch.float32, device=DEV)
    correct = torch.full((), 3, dtype=torch.int64, device=DEV)
    n_rows = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    guard = torch.zeros(optim.GUARD_NSTATE, dtype=torch.float64, device=DEV)
    guard[optim.G_TOTAL_NORM] = 1.5

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

    print(f"launch: the meter's launches alone; us per launch, {args.launches} launches per window, {args.repeats} windows "
          f"(median; spread = (max - min) / median); device = replays of a graph of {args.chain} launches")
    plain, logged = train.TrainMeter(0, 1024).bind(DEV), train.TrainMeter(256, 1024).bind(DEV)
    rows = [("fold, row-count word", lambda: plain.fold(loss, correct, n_rows=n_rows)),
            ("fold, constant rows, guard", lambda: plain.fold(loss, correct, batch_rows=64, guard=guard)),
            ("fold, guard and a 256-step log", lambda: logged.fold(loss, correct, n_rows=n_rows, guard=guard)),
            ("close (history of 1024)", plain.close_epoch)]
    for name, fn in rows:
        graph = graph_of(fn)
        dev = [window(fn, graph)[0] for _ in range(args.repeats)]
        eager = [window(fn, None) for _ in range(args.repeats)]
        ev, host = [e for e, _ in eager], [h for _, h in eager]
        print(f"  {name:34s}  device {statistics.median(dev):7.2f} us (spread {100 * _spread(dev):.1f} %)"
              f"  eager {statistics.median(ev):7.2f} us (spread {100 * _spread(ev):.1f} %)"
              f"  issue {statistics.median(host):7.2f} us (spread {100 * _spread(host):.1f} %)", flush=True)
    r = plain.result()
    print(f"  after the run: {r['epochs_closed']} closes, {r['overflow']} past the history; the logged meter holds "
          f"{logged.result()['log_total']} records")
    return 0


def part_train(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    print("train: clips/s of train.GraphedTrainStep with DeviceAdamW inside the graph at fp32 config 2, A = no meter, "
          "B = TrainMeter(log_capacity=256); windows alternated in one process (median; spread = (max - min) / median)")
    variants, steps = {}, args.train_steps
    for name in ("A", "B"):
        model, c = _model(hw, torch, DEV, "hwgate", torch.float32)
        x, y = _batch(torch, DEV, c, c["B"], 7)
        o = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
        meter = train.TrainMeter(log_capacity=256) if name == "B" else None
        s = train.GraphedTrainStep(model, o, x, y, meter=meter)
        for _ in range(5):
            s(x, y)
        variants[name] = (s, x, y, meter)
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
    for name in ("A", "B"):
        print(f"  {name} windows, ms per step: " + ", ".join(f"{1e3 * c['B'] / r:.3f}" for r in rate[name]))
    m = variants["B"][3].result()
    print(f"  fp32 config 2  A {a:9.0f} clips/s (spread {100 * _spread(rate['A']):.2f} %)   B {b:9.0f} clips/s "
          f"(spread {100 * _spread(rate['B']):.2f} %)   B / A {b / a:.4f}   step {1e3 * c['B'] / a:.3f} -> "
          f"{1e3 * c['B'] / b:.3f} ms, {steps} steps per window, {args.repeats} windows; loss A "
          f"{float(variants['A'][0].loss):.4f} B {float(variants['B'][0].loss):.4f}; the meter counted {m['steps']} steps, "
          f"{m['rows']} rows", flush=True)
    return 0


def part_loop(args):
    torch, hw, train, DEV = _gpu()
    optim = importlib.import_module("sl-hwgat_amd.optim")
    n_batches = 64
    print(f"loop: one train epoch of {n_batches} batches, clips/s (host clock; a window ends with the epoch's loss and accuracy "
          "on the host); R = the reference's loop (loss.item() and correct.cpu().tolist() after every replay of a "
          "GraphedTrainStep(ragged=True)), M = train.EpochLoop.train_epoch + one read of the closed epoch; windows alternated "
          "in one process (median; spread = (max - min) / median)")
    for kind in ("hgate", "hwgate"):
        for dtype, B in ((torch.bfloat16, 4), (torch.float32, 64)):
            made = {}
            for name in ("R", "M"):
                model, c = _model(hw, torch, DEV, kind, dtype)
                pool = [_batch(torch, DEV, c, B, 20 + i) for i in range(4)]
                batches = [pool[i % 4] for i in range(n_batches)]
                o = optim.DeviceAdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
                if name == "R":
                    step = train.GraphedTrainStep(model, o, *pool[0], ragged=True)
                    made[name] = (step, batches)
                else:
                    loop = train.EpochLoop(model, o, None, batch_size=B, example=pool[0], num_classes=c["nc"])
                    made[name] = (loop, batches)

            def reference_epoch(step, batches):
                total_loss, hits, rows = 0, [], 0
                for x, y in batches:
                    step(x, y)
                    total_loss += step.loss.item()
                    hits.append(step.correct.cpu().tolist())
                    rows += x.shape[0]
                return total_loss / len(batches), sum(hits) / rows

            def metered_epoch(loop, batches):
                loop.train_epoch(batches)
                h = loop.meter.history()[-1]
                return h["loss"], h["acc"]

            fns = {"R": reference_epoch, "M": metered_epoch}
            for name in fns:                                  # builds the step, warms up
                fns[name](*made[name])
            torch.cuda.synchronize()
            rate, last = {n: [] for n in fns}, {}
            for _ in range(args.repeats):
                for name in fns:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[name] = fns[name](*made[name])
                    torch.cuda.synchronize()
                    rate[name].append(n_batches * B / (time.perf_counter() - t0))
            r, m = statistics.median(rate["R"]), statistics.median(rate["M"])
            tag = "bf16" if dtype == torch.bfloat16 else "fp32"
            print(f"  {kind:6s} {tag} B={B:<3d} R {r:8.0f} clips/s (spread {100 * _spread(rate['R']):.1f} %)   M {m:8.0f} clips/s "
                  f"(spread {100 * _spread(rate['M']):.1f} %)   M / R {m / r:.3f}   per batch {1e3 * B / r:.3f} -> "
                  f"{1e3 * B / m:.3f} ms; last epoch loss R {last['R'][0]:.4f} M {last['M'][0]:.4f}", flush=True)
            del made
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400, help="launches per window (part launch)")
    ap.add_argument("--chain", type=int, default=50, help="launches held by the graph of the device-time windows")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps per window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "meter_lab.txt"))
    ap.add_argument("--part", choices=[p for p, _ in PARTS])
    ap.add_argument("--only", choices=[p for p, _ in PARTS], help="run this part alone (still as a child process)")
    args = ap.parse_args()
    if args.part:
        return {"launch": part_launch, "train": part_train, "loop": part_loop}[args.part](args)
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
