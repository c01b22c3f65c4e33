#!/usr/bin/env python3
"""Cost of the HWGATE part-window attention by window size, two tables:

  1. kernels   forward and backward of one attention launch at B = 64, T = 128, K = 64, d = 128, nH = 2 (head_dim 64),
               W in {8, 16, 32}, fp32 and bf16 storage, train mode (threshold on, no attention dropout): median of HIP
               event times, and the fraction of 8 TB/s against the algorithmic 4 E s (fwd) / 7 E s (bwd) bytes.
               W = 16 runs the hwgat_win_attn_* kernels, the others hwgat_pwin_attn_*.
  2. step      clips/s of the eager full train step (TrainStep, AdamW) of the default HWGATE config (B = 64, T = 128,
               K = 64, C = 2, embed 128) for W in {8, 16, 32}, fp32 and bf16 activations.

  python tools/pwin_lab.py [--iters 20] [--steps 10] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train_mod = importlib.import_module("sl-hwgat_amd.train")
from make_fixtures_window import edge_list  # noqa: E402

DEV = torch.device("cuda:0")
HBM = 8.0e12


def params(W, B=64, T=128, K=64, C=2, nc=2002):
    hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, C, DEV, num_kps=K)
    if W != 16:
        hp.window_size = W
        hp.edges = [edge_list(W, w) for w in range(K // W)]
        hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    return hp


def timed(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def kernel_table(iters):
    B, T, K, d, nH = 64, 128, 64, 128, 2
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        s = torch.tensor([], dtype=dtype).element_size()
        E = B * T * K * d
        qkv = (torch.randn(B, T, K, 3 * d, device=DEV) * 0.5).to(dtype)
        do = torch.randn(B, T, K, d, device=DEV).to(dtype)
        o = torch.empty(B, T, K, d, device=DEV, dtype=dtype)
        dqkv = torch.empty_like(qkv)
        thr = torch.full((1,), 0.3, device=DEV)
        for W in (8, 16, 32):
            hp = params(W)
            kind = "win" if W == 16 else "pwin"
            bits = (HF.mask_bits(hp.adj_mat) if W == 16 else HF.pwin_mask_bits(hp.adj_mat, W)).to(DEV)
            f = timed(lambda: HF.attn_fwd(kind, qkv, o, bits, thr, nH, True), iters)
            b = timed(lambda: HF.attn_bwd(kind, qkv, do, dqkv, bits, thr, nH, True), iters)
            for dirn, ms, nbytes in (("fwd", f, 4 * E * s), ("bwd", b, 7 * E * s)):
                rows.append({"W": W, "dtype": str(dtype).split(".")[-1], "dir": dirn, "kernel": kind, "us": round(ms * 1e3, 1),
                             "roof_frac": round(nbytes / (ms * 1e-3) / HBM, 3)})
                print(f"W={W:2d} {rows[-1]['dtype']:8s} {dirn}  {kind:4s}  {rows[-1]['us']:8.1f} us  "
                      f"{rows[-1]['roof_frac']:.3f} of 8 TB/s", flush=True)
    return rows


def step_table(steps):
    rows = []
    B = 64
    for dtype in (torch.float32, torch.bfloat16):
        for W in (8, 16, 32):
            torch.manual_seed(0)
            hp = params(W)
            model = hw.Model(*hp.get_model_params()).to(DEV).set_activation_dtype(dtype).train()
            opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True)
            step = train_mod.TrainStep(model, opt, None)
            x = torch.rand(B, 128, 64, 2, device=DEV)
            y = torch.randint(0, 2002, (B,), device=DEV)
            for _ in range(3):
                step(x, y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(x, y)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            rows.append({"W": W, "dtype": str(dtype).split(".")[-1], "ms_per_step": round(dt * 1e3, 2),
                         "clips_per_s": round(B / dt, 1)})
            print(f"step W={W:2d} {rows[-1]['dtype']:8s} {rows[-1]['ms_per_step']:8.2f} ms  {rows[-1]['clips_per_s']:8.1f} clips/s",
                  flush=True)
            del model, opt, step
    for r in rows:
        base = next(q for q in rows if q["dtype"] == r["dtype"] and q["W"] == 16)
        r["vs_w16"] = round(r["clips_per_s"] / base["clips_per_s"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernel_table(a.iters)}
    if not a.skip_step:
        out["step"] = step_table(a.steps)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
