#!/usr/bin/env python3
"""Cost of HWGATE stage widths that are odd multiples of 64 (embed_dim 64 / 192), two tables:

  1. kernels   every launch of a stage-0 block that runs a kernel new for these widths, at B = 64, T = 128, K = 64
               (M = 262 144 tokens), d0 in {64, 192}, fp32 and bf16: the 128x64-tile NT linears (qkv, proj, fc2 and the
               dX launches whose output is d wide), the 64x64-tile weight gradients, the LayerNorm statistics pass and
               backward.  Median HIP-event time, and the fraction of the BINDING roof: max(flops / MFMA peak, bytes /
               8 TB/s) over the measured time (peaks 157.3 TF fp32, 2.5 PF bf16 dense; bytes = operands read once +
               output written once).
  2. step      clips/s of the eager train step (TrainStep, AdamW) at B = 64, T = 128, K = 64, C = 2, 2002 classes for
               d0 in {64, 128, 192} (heads (2, 4, 8), the default (4, 8, 16), (3, 6, 12)), fp32 and bf16 activations.

  python tools/width_lab.py [--iters 20] [--steps 10] [--json out.json]
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
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train_mod = importlib.import_module("sl-hwgat_amd.train")

DEV = torch.device("cuda:0")
HBM = 8.0e12
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2.5e15}
HEADS = {64: (2, 4, 8, 16), 128: None, 192: (3, 6, 12, 24)}


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


def row(rows, d0, dt, name, ms, flops, nbytes):
    roof = max(flops / PEAK[dt], nbytes / HBM)
    r = {"d0": d0, "dtype": str(dt).split(".")[-1], "launch": name, "us": round(ms * 1e3, 1),
         "tflops": round(flops / (ms * 1e-3) / 1e12, 1), "tb_s": round(nbytes / (ms * 1e-3) / 1e12, 2),
         "bound": "mfma" if flops / PEAK[dt] > nbytes / HBM else "hbm", "roof_frac": round(roof / (ms * 1e-3), 3)}
    rows.append(r)
    print(f"d0={d0:3d} {r['dtype']:8s} {name:28s} {r['us']:8.1f} us {r['tflops']:7.1f} TF {r['tb_s']:5.2f} TB/s "
          f"{r['bound']:4s} {r['roof_frac']:.3f} of roof", flush=True)


def kernel_table(iters):
    rows = []
    B, T, K = 64, 128, 64
    M = B * (T // 2) * K
    for d0 in (64, 192):
        d, hid = d0, 2 * d0                    # ff_ratio 2 (HWGATEParams)
        for dt in (torch.float32, torch.bfloat16):
            s = torch.tensor([], dtype=dt).element_size()
            x = torch.randn(M, d, device=DEV).to(dt)
            u = torch.randn(M, hid, device=DEV).to(dt)
            g3 = torch.randn(M, 3 * d, device=DEV).to(dt)
            gm, bt = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
            mean, rstd = HF.ln_stats(x, gm, bt)
            Wqkv = torch.randn(3 * d, d, device=DEV) * 0.05
            Wf, sv, cv = HF.ln_fold(Wqkv, None, gm, bt, dt)
            Wp, W2 = (torch.randn(d, d, device=DEV) * 0.05).to(dt), (torch.randn(d, hid, device=DEV) * 0.05).to(dt)
            WqT, W1T = (torch.randn(d, 3 * d, device=DEV) * 0.05).to(dt), (torch.randn(d, hid, device=DEV) * 0.05).to(dt)
            b = torch.zeros(d, device=DEV)
            nt = [("nt qkv (ln-fold)", lambda: HF.linear_nt(x, Wf, None, pro=HF.PRO_LN_FOLD, ln=(mean, rstd, sv, cv)),
                   3 * d, d, 0),
                  ("nt proj (drop+res)", lambda: HF.linear_nt(x, Wp, b, epi=HF.EPI_BIAS_DROP_RES, res=x, epi_seed=1, epi_p=0.1),
                   d, d, 1),
                  ("nt fc2 (drop+res)", lambda: HF.linear_nt(u, W2, b, epi=HF.EPI_BIAS_DROP_RES, res=x, epi_seed=1, epi_p=0.1),
                   d, hid, 1),
                  ("nt dX qkv", lambda: HF.linear_nt(g3, WqT, None, epi=HF.EPI_NONE), d, 3 * d, 0),
                  ("nt dX fc1", lambda: HF.linear_nt(u, W1T, None, epi=HF.EPI_NONE), d, hid, 0)]
            for name, fn, N, Kk, extra in nt:
                ms = timed(fn, iters)
                row(rows, d0, dt, name, ms, 2.0 * M * N * Kk, (M * Kk + M * N * (1 + extra)) * s)
            dws = [("tn dW qkv (ln)", g3, x, 3 * d, d, True), ("tn dW proj", x, x, d, d, False),
                   ("tn dW fc1 (ln)", u, x, hid, d, True), ("tn dW fc2", x, u, d, hid, False)]
            for name, A, Bm, N, Kk, ln in dws:
                dW, db = torch.zeros(N, Kk, device=DEV), torch.zeros(N, device=DEV)
                kw = dict(ln=(mean, rstd, gm, bt)) if ln else {}
                ms = timed(lambda: HF.linear_tn(A, Bm, dW, db, **kw), iters)
                row(rows, d0, dt, name, ms, 2.0 * M * N * Kk, M * (N + Kk) * s)
            for w in (d0, 2 * d0, 4 * d0):
                if w in (128, 256, 512, 1024):
                    continue
                xw = torch.randn(M // (w // d0), w, device=DEV).to(dt)
                n = xw.shape[0]
                gw, bw = torch.ones(w, device=DEV), torch.zeros(w, device=DEV)
                mw, rw = HF.ln_stats(xw, gw, bw)
                ms = timed(lambda: HF.ln_stats(xw, gw, bw), iters)
                row(rows, d0, dt, f"ln stats d={w}", ms, 0.0, n * w * s + 8 * n)
                dgw, dbw = torch.zeros(w, device=DEV), torch.zeros(w, device=DEV)
                ms = timed(lambda: HF.ln_backward(xw, xw, mw, rw, gw, xw, dgw, dbw), iters)
                row(rows, d0, dt, f"ln bwd d={w}", ms, 0.0, 4 * n * w * s + 8 * n)
            del x, u, g3
    return rows


def step_table(steps):
    rows = []
    B = 64
    for dt in (torch.float32, torch.bfloat16):
        for d0 in (64, 128, 192):
            torch.manual_seed(0)
            hp = hw.HWGATEParams({"src_len": 128, "num_class": 2002}, 2, DEV, num_kps=64)
            hp.embed_dim = d0
            if HEADS[d0] is not None:
                hp.num_heads = list(HEADS[d0][:len(hp.depths)])
            model = hw.Model(*hp.get_model_params()).to(DEV).set_activation_dtype(dt).train()
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
            sec = (time.perf_counter() - t0) / steps
            rows.append({"d0": d0, "dtype": str(dt).split(".")[-1], "heads": list(model.num_heads),
                         "ms_per_step": round(sec * 1e3, 2), "clips_per_s": round(B / sec, 1)})
            print(f"step d0={d0:3d} {rows[-1]['dtype']:8s} {rows[-1]['ms_per_step']:8.2f} ms {rows[-1]['clips_per_s']:8.1f} clips/s",
                  flush=True)
            del model, opt, step
    for r in rows:
        base = next(q for q in rows if q["dtype"] == r["dtype"] and q["d0"] == 128)
        r["vs_d128"] = round(r["clips_per_s"] / base["clips_per_s"], 3)
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
        for r in out["step"]:
            print(f"step d0={r['d0']:3d} {r['dtype']:8s} vs d0=128: {r['vs_d128']:.3f}")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
