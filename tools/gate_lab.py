#!/usr/bin/env python3
"""Cost of the GATE model and of WGATE window sizes other than 16, at sizes a user runs (B 64, T 128, d 128, 8 heads,
depth 8; GATE K 29; WGATE K 64 with W 16 and W 32), fp32 and bf16.  Four parts, each a child process of its own under
its own time limit (a part that fails ends the run; nothing is started after it):

  kernels  hwgat_wband_attn_fwd / _bwd (GATE W 29 nW 1; WGATE W 32 nW 2) and, as the yardstick measured in the same run,
           the W = 16 band kernels hwgat_band_attn_* at K 64: median HIP-event time and the share of the 8 TB/s HBM peak
           from the byte model 4 E s forward, 7 E s backward (E = B F K d real tokens x channels, s bytes per element).
  steps    clips/s of the train step (TrainStep, fused AdamW, smoothed CE, dropout at the reference default 0.1), eager
           and graphed: GATE, WGATE W 16 (the yardstick: GATE has 29/64 of its tokens), WGATE W 32.
  dense    the GATE step at T = 32 with the attention done densely in torch (additive 0 / -10000 mask over all T K keys,
           as the reference does) against the same step on the band kernels: the band step must be faster.
  trace    `rocprofv3 --kernel-trace --stats` around a few eager GATE train steps (no timing taken from this run): where
           the step's time goes, kernel by kernel.

  python tools/gate_lab.py [--iters 20] [--steps 10] [--json profiles/gate_lab.json] [--txt profiles/gate_lab.txt]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("kernels", 240), ("steps", 420), ("dense", 180), ("trace", 240))       # (part, time limit in seconds)
HBM = 8.0e12


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return torch, hw, hw.functional, importlib.import_module("sl-hwgat_amd.train"), torch.device("cuda:0")


def timed(torch, fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def part_kernels(args):
    torch, hw, HF, _, DEV = _gpu()
    B, F, nH, hd = 64, 128, 8, 16
    d = nH * hd
    rows = []
    gate_adj = hw.GATEParams({"src_len": F, "num_class": 2}, 2, None).adj_mat
    for dt in (torch.float32, torch.bfloat16):
        es = torch.tensor([], dtype=dt).element_size()
        for name, K, W in (("band W16 K64 (yardstick)", 64, 16), ("wband W32 K64", 64, 32), ("wband W29 K29 (GATE)", 29, 29)):
            nW = K // W
            if W == 29:
                mask = HF.wband_mask_rows(gate_adj, F, 29).to(DEV)
            else:
                hp = hw.WGATEParams({"src_len": F, "num_class": 2}, 2, None, num_kps=K)
                if W != 16:
                    hp.window_size = W
                    hp.edges = [[[i, (i + 1) % W] for i in range(W)] + [[i, (i + 5) % W] for i in range(W)] for _ in range(nW)]
                    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
                mask = (HF.band_mask_rows(hp.adj_mat, F) if W == 16 else HF.wband_mask_rows(hp.adj_mat, F, W)).to(DEV)
            kind = "band" if W == 16 else "wband"
            qkv = torch.randn(B, F, K, 3 * d, device=DEV, dtype=dt)
            o = torch.empty(B, F, K, d, device=DEV, dtype=dt)
            do = torch.randn(B, F, K, d, device=DEV, dtype=dt)
            dqkv = torch.empty_like(qkv)
            E = B * F * K * d
            ms_f = timed(torch, lambda: HF.attn_fwd(kind, qkv, o, mask, None, nH, False), args.iters)
            ms_b = timed(torch, lambda: HF.attn_bwd(kind, qkv, do, dqkv, mask, None, nH, False), args.iters)
            for p, ms, nbytes in (("fwd", ms_f, 4 * E * es), ("bwd", ms_b, 7 * E * es)):
                r = {"table": "kernels", "kernel": name, "dtype": str(dt).split(".")[-1], "pass": p, "us": round(ms * 1e3, 1),
                     "hbm_frac": round(nbytes / (ms * 1e-3) / HBM, 3)}
                rows.append(r)
                print(f"kernel {name:26s} {r['dtype']:8s} {p} {r['us']:9.1f} us  {r['hbm_frac']:.3f} of HBM", flush=True)
    for r in rows:                         # ratio to the yardstick at equal pass / dtype (HBM share: equal bytes per E)
        y = next(q for q in rows if q["kernel"].startswith("band") and q["dtype"] == r["dtype"] and q["pass"] == r["pass"])
        r["vs_band16"] = round(r["hbm_frac"] / y["hbm_frac"], 3)
    return rows


def _model(hw, torch, DEV, which, T, dt, depths=8):
    ds = {"src_len": T, "num_class": 2002}
    if which == "gate":
        hp = hw.GATEParams(ds, 2, DEV)
        hp.depths = depths
        m = hw.GATEModel(*hp.get_model_params())
    else:
        hp = hw.WGATEParams(ds, 2, DEV)
        hp.depths = depths
        if which == "wgate32":
            hp.window_size = 32
            hp.edges = [[[i, (i + 1) % 32] for i in range(32)] + [[i, (i + 5) % 32] for i in range(32)] for _ in range(2)]
            hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
        m = hw.WGATEModel(*hp.get_model_params())
    return m.to(DEV).set_activation_dtype(dt).train()


def _clips_per_s(torch, step, x, y, steps):
    for _ in range(3):
        step(x, y)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step(x, y)
    b.record()
    b.synchronize()
    return x.shape[0] * steps / (a.elapsed_time(b) * 1e-3)


def part_steps(args):
    torch, hw, HF, train, DEV = _gpu()
    B, T = 64, 128
    rows = []
    for dt in (torch.float32, torch.bfloat16):
        for which in ("wgate16", "gate", "wgate32"):
            for graphed in (False, True):
                m = _model(hw, torch, DEV, which, T, dt)
                x = torch.rand(B, T, m.num_kps, 2, device=DEV)
                y = torch.randint(0, 2002, (B,), device=DEV)
                opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
                step = train.GraphedTrainStep(m, opt, x, y) if graphed else train.TrainStep(m, opt, None)
                cps = _clips_per_s(torch, step, x, y, args.steps)
                r = {"table": "steps", "model": which, "dtype": str(dt).split(".")[-1], "graphed": graphed, "clips_per_s": round(cps, 1)}
                rows.append(r)
                print(f"step {which:8s} {r['dtype']:8s} {'graphed' if graphed else 'eager  '} {cps:9.1f} clips/s", flush=True)
                del m, opt, step
                torch.cuda.empty_cache()
    for r in rows:
        y = next(q for q in rows if q["model"] == "wgate16" and q["dtype"] == r["dtype"] and q["graphed"] == r["graphed"])
        r["vs_wgate16"] = round(r["clips_per_s"] / y["clips_per_s"], 3)
    return rows


def part_dense(args):
    """the same GATE step with the attention core replaced by the reference's dense form in torch"""
    torch, hw, HF, train, DEV = _gpu()
    import types
    import torch.nn.functional as tF
    B, T = 64, 32
    rows = []
    for dt in (torch.float32, torch.bfloat16):
        out = {}
        for form in ("band", "dense"):
            m = _model(hw, torch, DEV, "gate", T, dt)
            if form == "dense":
                mask = m.adj_mask.to(dt)                                    # (1, 1, T K, T K) additive 0 / -10000

                def _block(self, h, blk, n_heads, shifted, thr, k, hand, mask=mask):
                    Bq, Fq, K, d = h.shape
                    p = self.drop_rate
                    xn = HF.layer_norm(h, blk.norm1.weight, blk.norm1.bias)
                    qkv = tF.linear(xn, blk.attn.qkv.weight.to(h.dtype), blk.attn.qkv.bias.to(h.dtype))
                    q, kk, v = qkv.view(Bq, Fq * K, 3, n_heads, d // n_heads).permute(2, 0, 3, 1, 4)
                    a = torch.softmax((q * (d // n_heads) ** -0.5) @ kk.transpose(-2, -1) + mask, dim=-1)
                    o = (a @ v).transpose(1, 2).reshape(Bq, Fq, K, d)
                    y = h + tF.dropout(tF.linear(o, blk.attn.proj.weight.to(h.dtype), blk.attn.proj.bias.to(h.dtype)), p, True)
                    z = HF.layer_norm(y, blk.norm2.weight, blk.norm2.bias)
                    u = tF.dropout(tF.gelu(tF.linear(z, blk.ff.fc1.weight.to(h.dtype), blk.ff.fc1.bias.to(h.dtype))), p, True)
                    return y + tF.dropout(tF.linear(u, blk.ff.fc2.weight.to(h.dtype), blk.ff.fc2.bias.to(h.dtype)), p, True)
                m._block = types.MethodType(_block, m)
            x = torch.rand(B, T, 29, 2, device=DEV)
            y = torch.randint(0, 2002, (B,), device=DEV)
            opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
            out[form] = _clips_per_s(torch, train.TrainStep(m, opt, None), x, y, args.steps)
            del m, opt
            torch.cuda.empty_cache()
        r = {"table": "dense", "dtype": str(dt).split(".")[-1], "T": T, "band_clips_per_s": round(out["band"], 1),
             "dense_torch_clips_per_s": round(out["dense"], 1), "band_over_dense": round(out["band"] / out["dense"], 2)}
        rows.append(r)
        print(f"GATE T={T} {r['dtype']:8s} band {out['band']:9.1f} clips/s  dense torch attention {out['dense']:9.1f} clips/s  "
              f"x{r['band_over_dense']:.2f}", flush=True)
    return rows


def part_trace_child(args):
    torch, hw, HF, train, DEV = _gpu()
    m = _model(hw, torch, DEV, "gate", 128, torch.float32)
    x = torch.rand(64, 128, 29, 2, device=DEV)
    y = torch.randint(0, 2002, (64,), device=DEV)
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    step = train.TrainStep(m, opt, None)
    for _ in range(6):
        step(x, y)
    torch.cuda.synchronize()
    return []


def part_trace(args):
    """runs the traced steps under rocprofv3 in a child of this child; returns the top kernels by total time"""
    import csv
    import glob
    import tempfile
    out = tempfile.mkdtemp(prefix="gate_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "gate", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--part", "trace_child"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    if files:
        with open(files[0]) as fh:
            for rec in list(csv.DictReader(fh))[:14]:
                r = {"table": "trace", "kernel": rec.get("Name", "")[:90], "calls": int(rec.get("Calls", 0)),
                     "total_us": round(float(rec.get("TotalDurationNs", 0)) / 1e3, 1), "percent": float(rec.get("Percentage", 0))}
                rows.append(r)
                print(f"trace {r['percent']:6.2f} %  {r['total_us']:11.1f} us  {r['calls']:5d} x  {r['kernel']}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gate_lab.json"))
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "gate_lab.txt"))
    ap.add_argument("--part", default=None, help="(internal) run one part in this process and print its rows as JSON")
    args = ap.parse_args()
    if args.part:
        rows = {"kernels": part_kernels, "steps": part_steps, "dense": part_dense, "trace": part_trace,
                "trace_child": part_trace_child}[args.part](args)
        print("ROWS " + json.dumps(rows), flush=True)
        return 0
    rows, text = [], []
    for part, limit in PARTS:                  # this process never opens the GPU: every part is a fresh child
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part,
               "--iters", str(args.iters), "--steps", str(args.steps)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        for line in res.stdout.splitlines():
            if line.startswith("ROWS "):
                rows += json.loads(line[5:])
            else:
                text.append(line)
                print(line, flush=True)
        if res.returncode != 0:
            text.append(f"part {part} ended with status {res.returncode}; nothing was started after it")
            print(text[-1] + "\n" + res.stderr[-2000:], flush=True)
            break
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
    with open(args.txt, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if rows and not text[-1].startswith("part ") else 1


if __name__ == "__main__":
    sys.exit(main())
