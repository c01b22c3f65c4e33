#!/usr/bin/env python3
"""Headline benchmark: HWGAT training step (fwd + loss + bwd + AdamW) clips/s.

Workload = BASELINE.json configs[1]: B=64 clips per GPU, T=128 frames, J=67 raw
joints -> 5 part windows (K=80), C=2, d_model=128, depths [2,2,4], 2002 classes,
fp32, train mode with the reference defaults (dropout 0.1, stochastic attention
drop).  Inputs are synthetic, resident in HBM before the timed region.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

`--steps K` is the number of timed steps; the result line's `ms_per_step` is their mean wall time.  With
`--dump-outputs DIR` the last timed step's results are written to DIR as .npy files (`dump_outputs`); every input --
weights, clips, labels, dropout seeds -- is seeded, so two runs with the same arguments start from the same data.

A plain run does only what the headline needs: set-up, warm-up, the timed steps (with per-launch HIP events on every
`--timer-every`-th of them, the `kernels` / `roofline` objects), `--dump-outputs`, the JSON line.  `--full` adds the
measurements that take runs of their own (`extra_legs`): the same K steps again without events, the eager kernel timing
of a `--graph` run, the `secondary` configs of the default run and the CPU baseline.

N>1 works both ways: under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`
(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), and as a plain `python bench.py --gpus N`,
where this process -- before it makes any GPU call -- starts N fresh rank processes itself, relays rank 0's
JSON line and exits non-zero if any rank fails (`spawn_ranks`).

Prints ONE JSON line on rank 0 (see README / DESIGN.md section "Measurement").
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CFG = dict(B=64, T=128, J=67, nW=5, C=2, d0=128, nc=2002)                     # BASELINE configs[1] (and [2] in bf16)
CFG5 = dict(B=256, T=256, J=133, nW=7, C=3, d0=256, nc=2002)                  # BASELINE configs[4] "stress"
CFG_HGATE = dict(B=64, T=128, J=29, K=29, C=2, d0=128, nc=2002)               # sibling model HGATE at the headline batch
CFG_WGATE = dict(B=64, T=128, J=64, K=64, C=2, d0=128, nc=2002)               # sibling model WGATE (reference default K=64)
HBM_PEAK = 8.0e12           # B/s, MI355X_MICROARCH.md
F32_MFMA_PEAK = 157.3e12    # FLOP/s


def attn_bytes(E, itemsize, bwd):
    """algorithmic bytes of one fused window-attention launch:
    fwd reads q,k,v + writes o = 4E; bwd reads q,k,v,dO + writes dq,dk,dv = 7E
    (delta is recomputed in-kernel, so o is not re-read: 7E, not 8E)."""
    return (7 if bwd else 4) * E * itemsize


def cpu_baseline_wgate(sample_b=1, steps=2):
    """WGATE oracle (dense (T*16)^2 attention like the reference) on the host cores, eval-mode fwd+bwd"""
    from oracle import wgat_oracle as OW
    c = CFG_WGATE
    cfg = dict(kp_dim=c["C"], temporal_dim=c["T"], num_classes=c["nc"], embed_dim=c["d0"])
    params = {k: v.requires_grad_(k not in ("B", "pos_encoder.pe")) for k, v in OW.synth_params(1, weight_std=0.02, **cfg).items()}
    model = OW.OracleWGAT(params, num_kps=c["K"], temporal_dim=c["T"])
    g = torch.Generator().manual_seed(7)
    x = torch.rand(sample_b, c["T"], c["K"], c["C"], generator=g)
    y = torch.randint(0, c["nc"], (sample_b,), generator=g)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    times = []
    for i in range(steps + 1):
        for p in params.values():
            p.grad = None
        t0 = time.perf_counter()
        OW.smoothed_cross_entropy(model.forward(x), y).backward()
        times.append(time.perf_counter() - t0)
    return {"value": round(sample_b / min(times[1:]), 3), "unit": "clips/s", "cores": torch.get_num_threads(),
            "kind": "port", "sample": f"WGATE oracle eval-mode fwd+bwd, B={sample_b} clip of the same T={c['T']} "
                                      f"K={c['K']} d0={c['d0']} shape, best of {steps} after 1 warm-up"}


def host_cpu():
    """(model string, physical cores, CPUs this process may run on)"""
    model, cores = "unknown", set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as fh:
            for ln in fh:
                if ln.startswith("model name") and model == "unknown":
                    model = ln.split(":", 1)[1].strip()
                elif ln.startswith("physical id"):
                    phys = ln.split(":", 1)[1].strip()
                elif ln.startswith("core id"):
                    core = ln.split(":", 1)[1].strip()
                elif not ln.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
    except OSError:
        pass
    usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return model, (len(cores) or (os.cpu_count() or 1)), usable


def _cpu_cell_worker(idx, cpus, threads, barrier, queue, c, K, steps, go):
    """one of N independent oracle processes of the host-saturating cell: pinned to its own block of CPUs, `threads`
    intra-op threads, eval-mode fwd+bwd on B=2 clips of the workload's shape; reports (start, end, clips) of its timed
    steps on the shared monotonic clock.  Never touches the GPU (torch CPU ops only)."""
    try:
        if cpus and hasattr(os, "sched_setaffinity"):
            os.sched_setaffinity(0, cpus)
        torch.set_num_threads(threads)
        from oracle import hwgat_oracle as O
        cfg = dict(kp_dim=c["C"], temporal_dim=c["T"], num_classes=c["nc"], embed_dim=c["d0"], num_kps=K)
        params = {k: v.requires_grad_(k not in ("B", "pos_encoder.pe"))
                  for k, v in O.synth_params(1, weight_std=0.02, **cfg).items()}
        model = O.OracleHWGAT(params, num_kps=K, temporal_dim=c["T"], drop_rate=0.0)
        g = torch.Generator().manual_seed(7 + idx)
        x = torch.rand(2, c["T"], K, c["C"], generator=g)
        y = torch.randint(0, c["nc"], (2,), generator=g)

        def one():
            for p in params.values():
                p.grad = None
            O.smoothed_cross_entropy(model.forward(x, thresholds=None), y).backward()
        go.wait(timeout=120)                            # the parent finishes its single-process cells first
        one()                                           # warm-up
        barrier.wait(timeout=60)
        t0 = time.monotonic()
        for _ in range(steps):
            one()
        queue.put((idx, t0, time.monotonic(), 2 * steps))
    except Exception as exc:                            # noqa: BLE001 -- reported, never fatal for the bench line
        queue.put((idx, None, None, repr(exc)))


class _SaturatedCell:
    """The multi-process cell of `cpu_baseline`: N independent oracle processes -- N = min(4, physical_cores / 16); the GPU
    box admits at most 6 processes next to an open GPU context and a freshly started torch process counts as one, so N
    stays at 4 -- each with `threads` intra-op threads (16: the winner of every thread sweep so far; round 3 ran 32 per
    process, which the sweep itself shows to be several times slower than 16) and pinned to `threads` CPUs of its own
    quarter of the host (blocks a quarter of the CPU ids apart: separate CCD groups / NUMA nodes).  `start()` launches
    the interpreters (they import torch and build the oracle, then sleep on an event, so the single-process cells are
    not disturbed); `run()` releases them together and returns the aggregate clips/s = all clips of the timed steps /
    (last end - first start) with the per-process rates next to it (contention shows as per-process rates below the
    single-process cell).  4 x 16 threads use half of a 128-core host: that is what the process limit leaves."""

    def __init__(self, c, K, phys, usable, threads=16, steps=2, max_proc=4):
        import multiprocessing as mp
        cores = min(phys, usable)
        self.n_proc = min(max_proc, max(1, cores // threads))
        self.threads = threads
        self.stride = cores // max(self.n_proc, 1)       # CPU ids between the blocks of two processes
        self.steps, self.procs = steps, []
        if self.n_proc < 2:
            return
        ctx = mp.get_context("spawn")                    # fresh interpreters: no GPU state is inherited
        self.barrier, self.queue, self.go = ctx.Barrier(self.n_proc), ctx.Queue(), ctx.Event()
        avail = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
        for i in range(self.n_proc):
            cpus = set(avail[i * self.stride:i * self.stride + self.threads])   # own CCD group / NUMA node, `threads` CPUs of it
            self.procs.append(ctx.Process(target=_cpu_cell_worker, daemon=True,
                                          args=(i, cpus, self.threads, self.barrier, self.queue, c, K, steps, self.go)))

    def start(self):
        for p in self.procs:
            p.start()
        return self

    def run(self, limit_s=40.0):
        if not self.procs:
            return None
        t_begin = time.perf_counter()
        self.go.set()
        got = []
        try:
            while len(got) < self.n_proc and time.perf_counter() - t_begin < limit_s:
                try:
                    got.append(self.queue.get(timeout=0.5))
                except Exception:                        # noqa: BLE001 -- queue.Empty
                    if not any(p.is_alive() for p in self.procs) and self.queue.empty():
                        break
        finally:
            for p in self.procs:                         # exactly the processes started above
                if p.is_alive():
                    p.terminate()
            for p in self.procs:
                p.join(timeout=5)
        ok = [g for g in got if g[1] is not None]
        if 2 * len(ok) < self.n_proc:
            return {"error": f"{len(ok)} of {self.n_proc} workers finished within {limit_s:.0f} s",
                    "details": [str(g[3]) for g in got if g[1] is None][:2]}
        # (workers that did not finish in time still loaded the host while the others were timed: the rate of the finished
        # ones, scaled to all processes, is the aggregate a longer wait would have measured)
        span = max(g[2] for g in ok) - min(g[1] for g in ok)
        return {"clips_per_s": round(sum(g[3] for g in ok) / span * self.n_proc / len(ok), 3), "processes": self.n_proc,
                "finished": len(ok), "threads_per_process": self.threads, "timed_steps": self.steps,
                "per_process_clips_per_s": [round(g[3] / (g[2] - g[1]), 3) for g in sorted(ok)],
                "seconds": round(time.perf_counter() - t_begin, 1)}


def cpu_baseline_saturated(c, K, phys, usable, threads=16, steps=3, limit_s=40.0, max_proc=4):
    return _SaturatedCell(c, K, phys, usable, threads, steps, max_proc).start().run(limit_s)


def cpu_baseline(hgate=False, budget_s=45.0):
    """The oracle (CPU restatement of the reference, cross-checked at 0.95-1.10x the reference's own speed on the
    same cores: BASELINE.md section 3) timed on this box's host cores by the protocol of SURVEY.md 8d: clips of the
    SAME shape as the GPU workload, B=8 and B=2, fwd+bwd in three variants -- (i) the reference's default train mode
    (dropout 0.1 + threshold drop), (ii) train mode with drop_rate 0, (iii) eval()-mode -- median of 3 timed steps
    after 1 warm-up, threads = the fastest of a short sweep (8/16/32/64/all physical cores).  `value` is the FASTEST cell (the
    most favourable to the CPU).  `budget_s` bounds the whole leg: cells are dropped (B=8 variants (i)/(ii) first)
    once the running total says the next one would not fit, and the record says which ran."""
    from oracle import hwgat_oracle as O
    c = dict(CFG_HGATE, nW=None) if hgate else CFG
    K = c["K"] if hgate else c["nW"] * 16
    model_str, phys, usable = host_cpu()
    torch.manual_seed(1001)
    cfg = dict(kp_dim=c["C"], temporal_dim=c["T"], num_classes=c["nc"], embed_dim=c["d0"], num_kps=K)
    params = {k: v.requires_grad_(k not in ("B", "pos_encoder.pe"))
              for k, v in O.synth_params(1, weight_std=0.02, **cfg).items()}
    g = torch.Generator().manual_seed(7)
    thr = [0.5] * 8

    def make(drop):
        if hgate:
            from oracle import hgat_oracle as OH
            return OH.OracleHGAT(params, num_kps=K, temporal_dim=c["T"])
        return O.OracleHWGAT(params, num_kps=K, temporal_dim=c["T"], drop_rate=drop)

    variants = [("eval", 0.0, None), ("train_drop0", 0.0, thr), ("train_drop0.1", 0.1, thr)]
    if hgate:
        variants = variants[:1]                      # the HGATE oracle models neither threshold nor dropout
    t_start = time.perf_counter()
    # thread count: SURVEY 8d says "all physical cores", but on a 128-core host the small per-window ATen ops run
    # SLOWER with 128 threads than with 16-32 (first box measured: 0.9 vs 5.5 clips/s).  The baseline must be the
    # CPU's best, so a short sweep on the cheapest cell picks the thread count; every trial is recorded.
    sweep = {}
    x2 = torch.rand(2, c["T"], K, c["C"], generator=g)
    y2 = torch.randint(0, c["nc"], (2,), generator=g)
    probe = make(0.0)
    for th in sorted({min(8, usable), min(16, usable), min(32, usable), min(64, usable), max(1, min(phys, usable))}):
        torch.set_num_threads(th)
        best = None
        for i in range(2):
            for p in params.values():
                p.grad = None
            t0 = time.perf_counter()
            O.smoothed_cross_entropy(probe.forward(x2), y2).backward()
            dt = time.perf_counter() - t0
            best = dt if (i == 1 or best is None) else best          # the second (warm) pass counts
        sweep[th] = round(2 / best, 3)
        if time.perf_counter() - t_start > budget_s / 4:
            break
    threads = max(sweep, key=sweep.get)
    # the multi-process cell gets the sweep's winner per process; its interpreters come up during the cells below, then sleep
    sat_cell = None if hgate else _SaturatedCell(c, K, phys, usable, threads=threads).start()
    single_budget = budget_s - (10.0 if not hgate else 0.0)     # the host-saturating cell runs last
    torch.set_num_threads(threads)
    cells = {}
    for bsz in (2, 8):
        x = torch.rand(bsz, c["T"], K, c["C"], generator=g)
        y = torch.randint(0, c["nc"], (bsz,), generator=g)
        for name, drop, th in variants:
            model = make(drop)
            est = None
            times = []
            for i in range(4):
                if est is not None and time.perf_counter() - t_start + est > single_budget and i > 1:
                    break
                for p in params.values():
                    p.grad = None
                t0 = time.perf_counter()
                out = model.forward(x) if hgate else model.forward(x, thresholds=th)
                O.smoothed_cross_entropy(out, y).backward()
                times.append(time.perf_counter() - t0)
                est = times[-1]
                if i == 0 and time.perf_counter() - t_start + 3 * est > single_budget and bsz == 8 and name != "eval":
                    times = []
                    break
            timed = sorted(times[1:])
            if timed:
                cells[f"B{bsz}_{name}"] = {"clips_per_s": round(bsz / timed[len(timed) // 2], 3), "timed_steps": len(timed)}
    best = max(cells, key=lambda k: cells[k]["clips_per_s"])
    value, cores = cells[best]["clips_per_s"], threads
    saturated = None
    if not hgate:
        saturated = sat_cell.run(limit_s=50.0)
        if saturated and saturated.get("clips_per_s", 0.0) > value:
            value, cores, best = saturated["clips_per_s"], saturated["processes"] * saturated["threads_per_process"], "host_saturated_eval_B2"
    return {"value": value, "unit": "clips/s", "cores": cores, "kind": "port",
            "cpu_model": model_str, "physical_cores": phys, "usable_cpus": usable,
            "thread_sweep_clips_per_s": {str(k): v for k, v in sweep.items()},
            "sample": f"oracle (torch CPU restatement) fwd+bwd on clips of the same T={c['T']} K={K} C={c['C']} "
                      f"d0={c['d0']} shape: single process, B in (2, 8) x variants (eval, train drop 0, train drop 0.1 = the "
                      f"reference default), median of up to 3 timed steps after 1 warm-up; and the multi-process cell "
                      f"({sat_cell.n_proc if sat_cell else 0} pinned processes x {sat_cell.threads if sat_cell else 0} threads, "
                      f"eval B=2, aggregate); value = fastest ({best})",
            "cells": cells, "host_saturated": saturated, "seconds": round(time.perf_counter() - t_start, 1)}


def visible_gpu_count():
    """GPUs this node exposes, WITHOUT loading the HIP / HSA runtime in this process (the parent of the rank processes
    must stay GPU-free): the *_VISIBLE_DEVICES lists if set, else the KFD topology (nodes with SIMDs are GPUs).
    None = cannot tell (no KFD sysfs): the ranks find out themselves on torch.cuda.set_device()."""
    import glob
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([t for t in v.split(",") if t.strip()])
    nodes = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not nodes:
        return None
    n = 0
    for path in nodes:
        try:
            with open(path) as fh:
                props = dict(ln.split(None, 1) for ln in fh.read().splitlines() if " " in ln)
            n += int(props.get("simd_count", "0")) > 0
        except (OSError, ValueError):
            return None
    return n


def _cpulist(text):
    """'0-15,128-143' -> [0..15, 128..143]"""
    out = []
    for part in text.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        out.extend(range(int(a), int(b or a) + 1))
    return out


def gpu_local_cpus(index, sysfs="/sys"):
    """CPUs of the NUMA node that GPU `index` (HIP order) hangs off, from sysfs ONLY -- no HIP / torch.cuda call, so the
    spawning parent and a rank that has not touched its GPU yet can both use it: KFD topology nodes with SIMDs are the
    GPUs in HIP order (re-mapped through an integer *_VISIBLE_DEVICES list), a node's `domain` / `location_id`
    ((bus << 8) | (device << 3) | function) give its PCI address, and /sys/bus/pci/devices/<address>/local_cpulist names
    the CPUs next to it.  Returns (sorted CPU list, "domain:bus:dev.fn") or (None, reason)."""
    import glob
    gpus = []
    for path in sorted(glob.glob(os.path.join(sysfs, "class/kfd/kfd/topology/nodes/*/properties")),
                       key=lambda q: int(q.split(os.sep)[-2])):
        try:
            with open(path) as fh:
                props = dict(ln.split(None, 1) for ln in fh.read().splitlines() if " " in ln)
            if int(props.get("simd_count", "0")) > 0:
                gpus.append((int(props.get("domain", "0")), int(props["location_id"])))
        except OSError:
            continue            # a node this process may not read (a GPU of the host that is not in this container's device cgroup): not ours
        except (ValueError, KeyError):
            return None, "unreadable KFD topology"
    if not gpus:
        return None, "no KFD topology in sysfs"
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            try:
                gpus = [gpus[int(t)] for t in v.split(",") if t.strip()]
            except (ValueError, IndexError):
                return None, f"{var} is not an integer list"
            break
    if not 0 <= index < len(gpus):
        return None, f"GPU {index} not in the topology ({len(gpus)} GPUs)"
    dom, loc = gpus[index]
    bdf = f"{dom:04x}:{(loc >> 8) & 0xff:02x}:{(loc >> 3) & 0x1f:02x}.{loc & 7}"
    try:
        with open(os.path.join(sysfs, "bus/pci/devices", bdf, "local_cpulist")) as fh:
            cpus = _cpulist(fh.read())
    except (OSError, ValueError):
        return None, f"no local_cpulist for {bdf}"
    return (sorted(cpus), bdf) if cpus else (None, f"empty local_cpulist for {bdf}")


def pin_rank_to_gpu_cpus(local_rank, local_world, sysfs="/sys"):
    """Pin this rank process to its share of the CPUs next to its GPU (with 8 Python ranks on one host the
    step is ~400 launches per 20-100 ms; a rank whose launches are issued from the far socket, or that migrates between
    cores, shows up as launch jitter).  The GPUs of this job that share a NUMA node split that node's CPU list evenly,
    in rank order.  Returns a record for the JSON line; never fatal (an unreadable topology leaves the affinity alone)."""
    if not hasattr(os, "sched_setaffinity"):
        return {"pinned": False, "reason": "no sched_setaffinity"}
    mine, where = gpu_local_cpus(local_rank, sysfs)
    if mine is None:
        return {"pinned": False, "reason": where}
    peers = [r for r in range(local_world) if gpu_local_cpus(r, sysfs)[0] == mine]
    slot = peers.index(local_rank)
    # hyperthread siblings next to each other (a node's list is "64-127,192-255": 192 is the sibling of 64), so that the
    # ranks sharing the node get disjoint PHYSICAL cores, each with both of its threads
    def core_key(c):
        try:
            with open(os.path.join(sysfs, f"devices/system/cpu/cpu{c}/topology/thread_siblings_list")) as fh:
                return (min(_cpulist(fh.read())), c)
        except (OSError, ValueError):
            return (c, c)
    mine = sorted(mine, key=core_key)
    per = len(mine) // len(peers)
    share = set(mine[slot * per:(slot + 1) * per]) & set(os.sched_getaffinity(0))
    if len(share) < 2:
        return {"pinned": False, "reason": f"share of {where}'s CPUs outside this process's affinity mask", "pci": where}
    os.sched_setaffinity(0, share)
    return {"pinned": True, "pci": where, "cpus": len(share), "first_cpu": min(share), "last_cpu": max(share),
            "ranks_sharing_node": len(peers)}


def secondary_run(hw, train_mod, dev, c, label, steps, warmup, micro_batch=None):
    """A second BASELINE config measured in the SAME process right after the headline, so that every driver run of the
    default `python bench.py` also records it: BASELINE configs[2] (the headline shape with bf16 activations / bf16 MFMA
    linears, the HBM-bound variant) and configs[4] (the stress shape, micro-batched) -- the same full train step
    (zero_grad + fwd + loss + bwd + fused AdamW), train mode, inputs resident in HBM.  Returns the object stored under
    `secondary.<name>`; the headline `value` is untouched by it."""
    K = c["nW"] * 16
    HF = hw.functional
    torch.manual_seed(1001)
    hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, num_kps=K, embed_dim=c["d0"])
    model = hw.Model(*hp.get_model_params()).to(dev)
    model.use_part_table(hw.part_table(c["J"], c["nW"]))
    model.set_activation_dtype(torch.bfloat16)
    model.train()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True)
    step = train_mod.TrainStep(model, opt, None, micro_batch=micro_batch)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=dev, generator=g)
    y = torch.randint(0, c["nc"], (c["B"],), device=dev, generator=g)
    for _ in range(warmup):
        step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(x, y)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    n_ev = 2 if micro_batch is None else 1
    HF.TIMERS = store = {}
    for _ in range(n_ev):                                # more steps with per-launch HIP events: kernel durations
        step(x, y)
    timers = HF.timers_summary()
    HF.TIMERS = None
    del store
    rate = c["B"] * steps / elapsed
    e_clip = c["T"] * K * c["d0"]
    b_launch = min(micro_batch or c["B"], c["B"])
    E = b_launch * e_clip
    n_micro = -(-c["B"] // b_launch)
    bytes_clip = 364.0 * e_clip * 2                      # (45 E s per block) x 8 + 4 E s, s = 2
    flops_clip = 3.0 * (16.0 * sum(dep * c["d0"] * 2 ** i for i, dep in enumerate((2, 2, 4))) + 128.0 * 8) * e_clip
    kern = {}
    for name, bwd in (("hwgat_win_attn_fwd", False), ("hwgat_win_attn_bwd", True)):
        n, ms = timers.get(name, (0, 0.0))
        if n:
            ach = attn_bytes(E, 2, bwd) / (ms / n * 1e-3)
            kern[name] = {"bound": "hbm", "achieved": round(ach / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                          "frac": round(ach / HBM_PEAK, 4), "launches": n, "avg_us": round(ms / n * 1e3, 1)}
    for name in ("hwgat_linear_nt_bf16", "hwgat_linear_tn_bf16"):
        n, ms = timers.get(name, (0, 0.0))
        n2, ms2 = timers.get(name + "_ex", (0, 0.0))
        n3, ms3 = timers.get(name + "_ws", (0, 0.0))
        if n + n2 + n3:
            kern[name] = {"launches_per_step": (n + n2 + n3) // n_ev, "ms_per_step": round((ms + ms2 + ms3) / n_ev, 3)}
    return {"value": round(rate, 2), "unit": "clips/s", "dtype": "bf16", "steps": steps, "warmup": warmup,
            "ms_per_step": round(elapsed / steps * 1e3, 3),
            "config": {"workload": f"{label}: HWGAT train step (fwd+loss+bwd+AdamW), B={c['B']}/GPU T={c['T']} "
                                   f"J={c['J']}->K={K} C={c['C']} d_model={c['d0']} depths[2,2,4] classes={c['nc']}, bf16 "
                                   f"activations + bf16 MFMA linears, train-mode drop 0.1"
                                   + (f", micro-batch {b_launch} ({n_micro} slices, gradient accumulation)" if micro_batch else "")},
            "roofline_end_to_end": {"bound": "hbm", "achieved": round(rate * bytes_clip / 1e9, 1), "peak": HBM_PEAK / 1e9,
                                    "unit": "GB/s", "frac": round(rate * bytes_clip / HBM_PEAK, 4), "bytes_per_clip": bytes_clip,
                                    "other_roof": {"bound": "mfma", "achieved": round(rate * flops_clip / 1e12, 1), "peak": 2500.0,
                                                   "unit": "TFLOP/s", "frac": round(rate * flops_clip / 2.5e15, 4)}},
            "kernels": kern, "hip_kernel_ms_per_step": round(sum(v[1] for v in timers.values()) / n_ev, 3),
            "loss": round(float(step.loss), 4)}


def secondary_config3(hw, train_mod, dev, steps=10, warmup=6):
    return secondary_run(hw, train_mod, dev, CFG, "BASELINE configs[2]", steps, warmup)


def secondary_config5(hw, train_mod, dev, steps=2, warmup=1):
    """BASELINE configs[4], the stress shape (B=256 T=256 J=133->K=112 C=3 d0=256), bf16, micro-batch 32: ~0.7 s per step"""
    return secondary_run(hw, train_mod, dev, CFG5, "BASELINE configs[4] (stress)", steps, warmup, micro_batch=32)


def spawn_ranks(n, argv):
    """Parent side of a plain `python bench.py --gpus N` (N > 1): one fresh process per GPU, started BEFORE this
    process has touched the GPU (it never does: devices are counted from the environment / KFD sysfs, never through
    torch.cuda or HIP), each with RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT in its environment -- the same contract
    torch.distributed.run provides.  Rank 0's stdout (exactly one JSON line) is relayed to ours; everything
    else the ranks print goes to stderr.  Any rank failing ends the others and makes this process exit non-zero."""
    import socket
    import subprocess
    dry = os.environ.get("HWGAT_BENCH_DRYRUN") == "1"
    have = None if dry else visible_gpu_count()
    if have is not None and have < n:
        sys.exit(f"bench.py --gpus {n}: only {have} GPU(s) visible on this node")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr))
    failed = None
    pending = set(range(n))
    while pending and failed is None:
        for r in sorted(pending):
            rc = procs[r].poll() if r else None
            if r == 0:
                try:                                        # rank 0 is drained so that its pipe can never fill up
                    out0, _ = procs[0].communicate(timeout=0.2)
                    rc = procs[0].returncode
                except subprocess.TimeoutExpired:
                    rc = None
            if rc is None:
                continue
            pending.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
        time.sleep(0.05)
    if failed is not None:
        for r in pending:                                   # exactly the processes started above
            procs[r].terminate()
        for r in pending:
            try:
                procs[r].wait(timeout=20)
            except subprocess.TimeoutExpired:
                procs[r].kill()
        sys.exit(f"bench.py: rank {failed[0]} exited with code {failed[1]}; run aborted")
    lines = [ln for ln in out0.decode().splitlines() if ln.strip()]
    if len(lines) != 1:
        sys.exit(f"bench.py: rank 0 printed {len(lines)} stdout lines instead of one JSON line")
    rec = json.loads(lines[0])
    if rec.get("n_gpus") != n:
        sys.exit(f"bench.py: rank 0 reports n_gpus={rec.get('n_gpus')}, expected {n}")
    sys.stdout.write(lines[0] + "\n")
    sys.stdout.flush()


def dist_record(dist, world, device_name, step_ms, pin):
    """what the process group actually was, gathered from every rank (collective: all ranks call it): backend, the world
    size torch.distributed reports, every rank's device, the spread of the per-rank step time, every rank's CPU pinning"""
    mine = {"rank": dist.get_rank(), "device": device_name, "step_ms": round(step_ms, 3), "cpu_pin": pin,
            "pid": os.getpid()}
    every = [None] * world
    dist.all_gather_object(every, mine)
    every.sort(key=lambda r: r["rank"])
    steps = [r["step_ms"] for r in every]
    return {"backend": dist.get_backend(), "world_size_seen": dist.get_world_size(), "devices": [r["device"] for r in every],
            "step_ms_min": min(steps), "step_ms_max": max(steps), "cpu_pin": [r["cpu_pin"] for r in every],
            "distinct_processes": len({r["pid"] for r in every})}


DUMP_SAMPLE = 1 << 22       # entries per sampled array of --dump-outputs: 16 MB in float32


def dump_outputs(model, step, out_dir):
    """--dump-outputs DIR: what the last timed train step handed its caller, as DIR/<name>.npy --
    loss.npy (float32, the step's mean loss), correct.npy (float64, correctly classified clips), and of the trainable
    parameters in `named_parameters()` order, flattened and concatenated: params.npy (after the AdamW update) and
    grads.npy (the step's gradients), both float32.  When there are more than DUMP_SAMPLE parameter entries, both hold
    the same fixed sample of them: entries numpy.random.default_rng(0).choice(N, DUMP_SAMPLE, replace=False), sorted
    (a function of N only, so two builds of the same model dump the same entries).  At most ~32 MB in all.
    Call after the timed region; it synchronises and copies to the host."""
    import numpy as np
    ps = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in ps)
    idx = None
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))
        idx_dev = torch.from_numpy(idx).to(ps[0].device)

    def flat(ts):
        v = torch.cat([t.detach().reshape(-1).float() for t in ts])
        return (v if idx is None else v[idx_dev]).cpu().numpy()
    arrays = {
        "loss": np.asarray(float(step.loss), dtype=np.float32),
        "correct": np.asarray(float(step.correct), dtype=np.float64),
        "params": flat(ps),
        "grads": flat([p.grad if p.grad is not None else torch.zeros_like(p) for p in ps]),
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def extra_legs(args, world):
    """What this run measures beyond its headline, each leg after the timed steps: nothing without --full.  With it,
    "timer_free" = the same K steps again without per-launch HIP events (`value_without_kernel_timers`), "graph_timers" =
    two eager steps with events after a --graph run (the replayed graph cannot carry them), "secondary" = BASELINE
    configs[2] / [4] after the default headline on one GPU, "cpu_baseline" = the oracle on the host cores.  Call with
    the final args (after --config 3 has set the dtype)."""
    if not args.full:
        return set()
    legs = set()
    if not args.no_kernel_timers:
        legs.add("graph_timers" if args.graph else "timer_free")
    default_run = (args.config == 2 and args.dtype == "f32" and args.model == "hwgate" and not args.eval_mode
                   and not args.from_host and args.batch is None and args.micro_batch is None and not args.graph
                   and not args.deterministic)
    if world == 1 and default_run and not args.no_secondary:
        legs.add("secondary")
    if world == 1 and not args.no_cpu_baseline and args.config != 5:
        legs.add("cpu_baseline")
    return legs


def dry_run(args, json_fd):
    """HWGAT_BENCH_DRYRUN=1: the launcher / rendezvous / max-over-ranks / one-JSON-line plumbing on the gloo
    backend with no model and no GPU (tests/test_dist_cpu.py); `value` is meaningless."""
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local, local_world = int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    pin = pin_rank_to_gpu_cpus(local, local_world, os.environ.get("HWGAT_BENCH_SYSFS", "/sys")) if world > 1 else None
    if world > 1:
        dist.init_process_group("gloo")
    if os.environ.get("HWGAT_BENCH_DRYRUN_FAIL_RANK") == str(rank):
        sys.exit(3)
    mine = 0.001 * (rank + 1)
    t = torch.tensor([mine], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    info = dist_record(dist, world, f"dry-run device of rank {rank}", mine * 1e3 / max(args.steps, 1), pin) if world > 1 else None
    if rank == 0:
        out = {"metric": "dry-run", "value": 0.0, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "max_elapsed": float(t), "config": {"global_batch": world * CFG["B"], "parallelism": f"dp{world}"},
               "dist": info}
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 5],
                    help="BASELINE config: 2 = fp32 headline (default), 3 = same in bf16, 5 = stress shape")
    ap.add_argument("--model", default="hwgate", choices=["hwgate", "hgate", "wgate"],
                    help="hwgate = the headline model (default); hgate / wgate = the sibling models (SURVEY 8f rank 3) "
                         "at the headline batch / frames / width")
    ap.add_argument("--batch", type=int, default=None, help="clips per GPU (default: the config's)")
    ap.add_argument("--micro-batch", type=int, default=None, help="gradient-accumulation slice (clips)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run what it does not need (see extra_legs): the same K steps without "
                         "per-launch HIP events, the secondary configs of the default run, the CPU baseline; off by default")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary.config3_bf16 / config5_bf16 measurements the default run appends (same process, after the headline)")
    ap.add_argument("--no-kernel-timers", action="store_true", help="skip the per-launch HIP events (A/B runs)")
    ap.add_argument("--timer-every", type=int, default=10,
                    help="record the per-launch HIP events on every N-th step of the timed region (1 = every step).  The "
                         "events cost host time (two records per launch, ~400 launches per step): nothing at the 102 ms "
                         "headline step, but the 10-17 ms sibling-model steps are close to host-bound and a timed step "
                         "runs 1.3-2.3x longer, so the default times 2 of 20 steps")
    ap.add_argument("--eval-mode", action="store_true", help="deterministic fwd+bwd (no dropout / attention drop)")
    ap.add_argument("--deterministic", action="store_true",
                    help="model.deterministic_train = True: every reduction of the step in a fixed order (bit-reproducible "
                         "training like the reference's on one device); slower, never the default headline")
    ap.add_argument("--graph", action="store_true",
                    help="capture the whole train step (seed advance + fwd + loss + bwd + AdamW) in ONE HIP graph and replay it "
                         "per step (train.GraphedTrainStep): same kernels, no per-launch host work; never the default headline")
    ap.add_argument("--from-host", action="store_true",
                    help="feed every step from host samples through collate.PinnedBatcher (pinned staging + async H2D): "
                         "the PCIe-inclusive rate DESIGN.md quotes; never the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (loss, correct count, updated "
                         "parameters and gradients, a fixed sample of the latter two) as DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1: ms_per_step is the mean over the timed steps")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args.gpus, sys.argv[1:])         # nothing above or in there touches the GPU
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={os.environ.get('WORLD_SIZE')}")

    # stdout carries exactly ONE JSON line: native libraries (RCCL prints a version banner on process-group
    # init) write to file descriptor 1 directly, so fd 1 is pointed at stderr for the whole run and the
    # result line goes to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if os.environ.get("HWGAT_BENCH_DRYRUN") == "1":
        return dry_run(args, json_fd)
    # each rank of a multi-GPU job goes to the CPUs next to its own GPU (sysfs only; before this process touches the GPU)
    pin = None
    if world > 1 or os.environ.get("HWGAT_FORCE_PIN") == "1":
        pin = pin_rank_to_gpu_cpus(local, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    # HWGAT_FORCE_DIST=1: run the RCCL path (process group, broadcast, bucketed all-reduce) even at
    # world size 1 -- lets a 1-GPU box rehearse exactly what the N>1 launch executes
    use_dist = world > 1 or os.environ.get("HWGAT_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)

    hw = importlib.import_module("sl-hwgat_amd")
    from importlib import import_module
    train_mod = import_module("sl-hwgat_amd.train")
    dist_mod = import_module("sl-hwgat_amd.dist")
    HF = hw.functional

    if args.config == 3:
        args.dtype = "bf16"
    hgate, wgate = args.model == "hgate", args.model == "wgate"
    base = CFG_HGATE if hgate else CFG_WGATE if wgate else (CFG5 if args.config == 5 else CFG)
    c = dict(base, B=args.batch or base["B"])
    K = c["K"] if (hgate or wgate) else c["nW"] * 16
    if args.config == 5 and args.micro_batch is None:
        args.micro_batch = 16 if args.dtype == "f32" else 32      # activation memory, DESIGN.md section 3
    legs = extra_legs(args, world)
    torch.manual_seed(1001)                                       # reference configs.py:55-59
    if hgate:
        hp = hw.HGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, embed_dim=c["d0"])
        model = hw.HGATEModel(*hp.get_model_params()).to(dev)
    elif wgate:
        hp = hw.WGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, num_kps=K, embed_dim=c["d0"])
        model = hw.WGATEModel(*hp.get_model_params()).to(dev)
    else:
        hp = hw.HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], dev, num_kps=K, embed_dim=c["d0"])
        model = hw.Model(*hp.get_model_params()).to(dev)
        model.use_part_table(hw.part_table(c["J"], c["nW"]))
    if args.dtype == "bf16":
        model.set_activation_dtype(torch.bfloat16)
    model.train(not args.eval_mode)
    model.deterministic_train = bool(args.deterministic)
    dist_mod.broadcast_parameters(model)
    reducer = dist_mod.GradReducer(model.parameters(), always_reduce=use_dist) if use_dist else None
    if args.graph and (args.micro_batch or args.eval_mode or use_dist):
        sys.exit("bench.py --graph: one full-batch train-mode step on one GPU (no --micro-batch / --eval-mode / process group)")
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=args.graph)
    step = train_mod.TrainStep(model, opt, reducer, micro_batch=args.micro_batch)

    g = torch.Generator(device=dev).manual_seed(7 + rank)
    x = torch.rand(c["B"], c["T"], c["J"], c["C"], device=dev, generator=g)
    y = torch.randint(0, c["nc"], (c["B"],), device=dev, generator=g)
    eager_step = step
    if args.graph:
        step = train_mod.GraphedTrainStep(model, opt, x, y)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    if args.from_host:
        batcher = import_module("sl-hwgat_amd.collate").PinnedBatcher(c["B"], (c["T"], c["J"], c["C"]), dev)
        xs, ys = x.cpu(), y.cpu()
        samples = [(xs[i], int(ys[i])) for i in range(c["B"])]          # what a Dataset hands the collate_fn

        def run_step():
            xb, yb = batcher.collate(samples)
            step(xb, yb)
    else:
        def run_step():
            step(x, y)

    for _ in range(args.warmup):
        run_step()
    barrier()
    # per-launch HIP events (kernel durations for the roofline objects) are recorded on every `--timer-every`-th step
    # of the timed region, not on all of them: an event pair costs ~3 us of stream time and 5-10 us of host time, and a
    # step has ~190-400 launches
    store, n_timed = {}, 0
    graph_timers = "graph_timers" in legs                        # per-launch events cannot sit inside a graph replay:
    if args.graph:                                               # the kernel durations come from eager steps AFTER the timed region
        args.no_kernel_timers = True
    if not args.no_kernel_timers:
        # one untimed step with the events on counts the launches of a step; the events the timed region will use are then
        # created BEFORE it (event creation, not recording, was most of what the per-launch timing cost)
        probe = {}
        HF.TIMERS = probe
        run_step()
        HF.TIMERS = None
        per_step = 2 * sum(len(v) for v in probe.values())
        HF.prime_events(per_step * (-(-args.steps // max(1, args.timer_every)) + 1))
        del probe
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        on = not args.no_kernel_timers and i % max(1, args.timer_every) == 0
        HF.TIMERS = store if on else None
        n_timed += on
        run_step()
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:                          # before any later step changes the weights
        dump_outputs(model, step, args.dump_outputs)
    if graph_timers:                                             # the same kernels, launched one by one, with events
        HF.TIMERS = store
        for _ in range(2):
            eager_step(x, y)
        n_timed = 2
    HF.TIMERS = store
    timers = HF.timers_summary()
    HF.TIMERS = None
    n_timed = max(n_timed, 1)
    loss = float(step.loss)
    # the same K steps once more WITHOUT any per-launch HIP events: what the event recording still costs is the
    # difference between the two rates (--full)
    elapsed_plain = None
    if "timer_free" in legs:
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run_step()
        barrier()
        elapsed_plain = time.perf_counter() - t0

    dist_info = None
    if use_dist:                                             # before the MAX: every rank's own step time, device, pinning
        props = torch.cuda.get_device_properties(dev)
        dist_info = dist_record(dist, world, f"{props.name} ({getattr(props, 'gcnArchName', '?')}) cuda:{local}",
                                elapsed / args.steps * 1e3, pin)
    t = torch.tensor([elapsed, elapsed_plain or 0.0], device=dev, dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t[0])
    elapsed_plain = float(t[1]) if elapsed_plain is not None else None

    if rank == 0:
        itemsize = 4 if args.dtype == "f32" else 2
        b_launch = min(args.micro_batch or c["B"], c["B"])            # clips per attention launch
        E = b_launch * c["T"] * K * c["d0"]
        kern = {}
        hip_ms = sum(v[1] for v in timers.values())                  # every timed C-ABI entry point, before any merging below
        attn = "hwgat_blk_attn" if hgate else "hwgat_band_attn" if wgate else "hwgat_win_attn"
        for name, bwd in ((attn + "_fwd", False), (attn + "_bwd", True)):
            n, ms = timers.get(name, (0, 0.0))
            if n:
                avg = ms / n * 1e-3
                ach = attn_bytes(E, itemsize, bwd) / avg
                kern[name] = {"bound": "hbm", "achieved": round(ach / 1e9, 1), "peak": HBM_PEAK / 1e9,
                              "unit": "GB/s", "frac": round(ach / HBM_PEAK, 4), "traffic": None, "traffic_source": None,
                              "launches": n, "avg_us": round(avg * 1e6, 1),
                              "bytes_per_launch": attn_bytes(E, itemsize, bwd)}
        # HBM bytes per launch from stored rocprofv3 PMC passes (FETCH_SIZE x2 correction + WRITE_SIZE, separate passes;
        # the file named in `traffic_source`) -- only valid for the shape they were taken on
        try:
            fname = "r04_sibling_attn_pmc_traffic.json" if (hgate or wgate) else "r04_attn_pmc_traffic.json"   # both dtypes, round-4 binaries
            with open(os.path.join(ROOT, "profiles", fname)) as fh:
                pmc = json.load(fh)
            if args.dtype == "bf16":
                pmc = pmc.get("bf16", {})                             # the bf16 passes (config 3 shape)
            for name in kern:
                rec = pmc.get(name + "_1seg", pmc.get(name))          # band fwd: the shipped 1-segment geometry
                if rec and rec.get("E_bytes", pmc.get("E_bytes")) == E * itemsize:
                    kern[name]["traffic"] = rec["traffic_bytes_per_launch"]
                    kern[name]["traffic_source"] = (f"stored rocprofv3 PMC passes (FETCH_SIZE x2 + WRITE_SIZE) of this kernel at this "
                                                    f"shape, profiles/{fname} -- not measured in this run")
        except (OSError, KeyError):
            pass
        # linears: useful flops per step (fwd + dX + dW = 3 x 16*E*d_i per block) against the dense MFMA peak
        sum_d = 8 * c["d0"] if wgate else sum(dep * c["d0"] * 2 ** i for i, dep in enumerate((2, 2, 4)))
        n_micro = -(-c["B"] // b_launch)
        flops_fwd = 16.0 * E * sum_d * n_micro                        # per step, forward linears
        peak = F32_MFMA_PEAK if args.dtype == "f32" else 2.5e15
        for name, fl in (("hwgat_linear_nt_" + args.dtype, 2 * flops_fwd), ("hwgat_linear_tn_" + args.dtype, flops_fwd)):
            n, ms = timers.get(name, (0, 0.0))
            n2, ms2 = timers.pop(name + "_ex", (0, 0.0))          # the same linears with the statistics / merge epilogue
            n3, ms3 = timers.pop(name + "_ws", (0, 0.0))          # ... and the weight gradients with the workspace reduction
            n, ms = n + n2 + n3, ms + ms2 + ms3
            if n:
                ach = fl * n_timed / (ms * 1e-3)
                kern[name] = {"bound": "mfma", "achieved": round(ach / 1e12, 1), "peak": peak / 1e12,
                              "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": None,
                              "launches": n, "ms_per_step": round(ms / n_timed, 3),
                              "flops_per_step": fl}
        others = {k: {"launches": v[0], "total_ms": round(v[1], 3)} for k, v in timers.items()
                  if k not in kern}
        roof = dict(kern.get(attn + "_bwd", {"bound": "hbm", "achieved": None, "peak": HBM_PEAK / 1e9,
                                                    "unit": "GB/s", "frac": None, "traffic": None}))
        roof["kernel"] = ("blk_attn_bwd_k (fused block graph-attention backward, HGATE)" if hgate
                          else "band_attn_bwd_k (fused band graph-attention backward, WGATE)" if wgate
                          else "win_attn_bwd_k (fused window graph-attention backward)")
        # SURVEY 8(d) "secondary" roofline of the whole step: fwd+bwd flops (linears 16*sum_d*E + dense attention
        # 128*E per block, x3 for fwd + dX + dW) against the dense MFMA peak of the compute dtype -- the bound
        # that binds config 2 in fp32 (the attention kernels above are the HBM-bound part north_star names)
        n_blocks = 8
        e_clip = c["T"] * K * c["d0"]
        flops_clip = 3.0 * (16.0 * sum_d + 128.0 * n_blocks) * e_clip
        bytes_clip = 364.0 * e_clip * itemsize            # (45 E s per block) x 8 + 4 E s
        rate = world * c["B"] * args.steps / elapsed
        e2e_mfma = {"bound": "mfma", "achieved": round(rate * flops_clip / 1e12, 1), "peak": peak / 1e12,
                    "unit": "TFLOP/s", "frac": round(rate * flops_clip / (world * peak), 4), "flops_per_clip": flops_clip}
        e2e_hbm = {"bound": "hbm", "achieved": round(rate * bytes_clip / 1e9, 1), "peak": HBM_PEAK / 1e9,
                   "unit": "GB/s", "frac": round(rate * bytes_clip / (world * HBM_PEAK), 4),
                   "bytes_per_clip": bytes_clip}
        # which roof binds the whole step: fp32 -> fp32 MFMA (869 / 78 clips/s ceilings at
        # configs 2 / 5); bf16 -> HBM (8 385 clips/s at config 3, 1 497 at config 5)
        roof_e2e = dict(e2e_mfma if args.dtype == "f32" else e2e_hbm)
        roof_e2e["other_roof"] = e2e_hbm if args.dtype == "f32" else e2e_mfma
        out = {
            "metric": "clips/sec fwd+bwd at B=64 T=128 J=67; %HBM roofline; 1->8 GPU scaling",
            "value": round(world * c["B"] * args.steps / elapsed, 2), "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "value_without_kernel_timers": (round(world * c["B"] * args.steps / elapsed_plain, 2)
                                            if elapsed_plain else None),
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
            "data": "synthetic" + (", host-fed" if args.from_host else ""),
            "config": {"workload": ("sibling model HGATE at the headline shape" if hgate else
                                    "sibling model WGATE at the headline shape" if wgate else
                                    f"BASELINE configs[{ {2: 1, 3: 2, 5: 4}[args.config] }]")
                                   + (": HGATE" if hgate else ": WGATE" if wgate else ": HWGAT") + " train step (fwd+loss+bwd+AdamW), "
                                   f"B={c['B']}/GPU T={c['T']} J={c['J']}->K={K} C={c['C']} "
                                   f"d_model={c['d0']} " + ("8 blocks" if wgate else "depths[2,2,4]") + f" classes={c['nc']}, "
                                   + ("eval-mode" if args.eval_mode else "train-mode drop 0.1")
                                   + (f", micro-batch {args.micro_batch}" if args.micro_batch else "")
                                   + (", whole step replayed as one HIP graph" if args.graph else "")
                                   + (", deterministic_train (fixed-order reductions, no float atomics)" if args.deterministic else "")
                                   + (", inputs collated from host samples every step (PCIe-inclusive, not the headline)"
                                      if args.from_host else ""),
                       "global_batch": world * c["B"], "parallelism": f"dp{world}"},
            "dist": dist_info, "roofline": roof, "roofline_end_to_end": roof_e2e,
            "kernels": kern, "other_hip_entry_points": others,
            "hip_kernel_ms_per_step": round(hip_ms / n_timed, 3), "kernel_timer_steps": n_timed,
            "loss": round(loss, 4),
        }
        if "secondary" in legs:
            # the headline's model / optimizer / saved activations go first; its numbers above are final
            del step, opt, model
            torch.cuda.empty_cache()
            out["secondary"] = {}
            for name, fn in (("config3_bf16", secondary_config3), ("config5_bf16", secondary_config5)):
                try:
                    out["secondary"][name] = fn(hw, train_mod, dev)
                except Exception as exc:                    # noqa: BLE001 -- the headline above is final and must be printed
                    out["secondary"][name] = {"error": repr(exc)}
                torch.cuda.empty_cache()
        if "cpu_baseline" in legs:
            # after the timed regions; the GPU is idle meanwhile
            out["cpu_baseline"] = cpu_baseline_wgate() if wgate else cpu_baseline(hgate=hgate)
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
