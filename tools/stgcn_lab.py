#!/usr/bin/env python3
"""Cost of the ST-GCN baseline at the size a user runs (B 64, T 128, V 29, C 2, default widths, fp32).  Three parts, each
a child process of its own under its own time limit (a part that fails ends the run; nothing is started after it):

  kernels  every new kernel at the three stage shapes (237 568 rows x 64, 118 784 x 128, 59 392 x 256): median HIP-event
           time, algorithmic flops and bytes from the shapes (the models are in KERNELS below), and the share of the roof
           that applies -- 157.3 TFLOP/s fp32 MFMA for the convolutions, 8 TB/s HBM for everything else.
  steps    clips/s of the train step (zero_grad, forward, smoothed CE, backward, fused AdamW; eager TrainStep and
           GraphedTrainStep) and of the eval forward, alternated in one process with the STOCK path: the same model
           written with torch library ops (conv2d, batch_norm, einsum; channels-first, what a user has today) on the
           same weights.  Warmed, >= 50 timed steps, device events, two repeats for the spread.
  trace    `rocprofv3 --kernel-trace --stats` around a few eager train steps (no timing taken from this run): where the
           step's time goes, kernel by kernel.

  python tools/stgcn_lab.py [--iters 20] [--steps 50] [--json profiles/stgcn_lab.json] [--txt profiles/stgcn_lab.txt]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("kernels", 300), ("steps", 600), ("trace", 300))       # (part, time limit in seconds)
HBM, MFMA = 8.0e12, 157.3e12
B, T, V, NCLASS = 64, 128, 29, 2002
STAGES = ((128, 64), (64, 128), (32, 256))                        # (frames, channels) of the three stages


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
    rows = []
    A = hw.STGCNModel(*hw.STGCNParams({"num_class": 4}, 2).get_model_params()).A.to(DEV)
    E = torch.ones_like(A)
    for Tn, C in STAGES:
        M = B * Tn * V
        x = torch.randn(B, Tn, V, C, device=DEV)
        y3 = torch.randn(B, Tn, V, 3 * C, device=DEV)
        W9 = torch.randn(C, C, 9, 1, device=DEV) / (9 * C) ** 0.5
        W1 = torch.randn(3 * C, C, 1, 1, device=DEV) / C ** 0.5
        bias, gamma = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        k9, k9t = HF.stgcn_weight_image(W9, 0), HF.stgcn_weight_image(W9, 1)
        k1, k1t = HF.stgcn_weight_image(W1, 0), HF.stgcn_weight_image(W1, 1)
        mean, rstd = HF.stgcn_bn_stats(x)
        e = 4 * M * C                                       # bytes of one (M, C) fp32 tensor
        # (name, callable, flops, bytes, roof): algorithmic counts -- every operand once, no halo or re-reads
        KERNELS = (
            ("tconv fwd", lambda: HF.stgcn_conv(x, k9, bias, 1, 4), 2 * M * 9 * C * C, 2 * e, "mfma"),
            ("tconv dX", lambda: HF.stgcn_conv_dx(x, k9t, Tn, 1, 4), 2 * M * 9 * C * C, 2 * e, "mfma"),
            ("tconv dW", lambda: HF.stgcn_conv_dw(x, x, W9.shape, 1, 4), 2 * M * 9 * C * C, 2 * e, "mfma"),
            ("proj fwd", lambda: HF.stgcn_conv(x, k1, None), 2 * M * 3 * C * C, 4 * e, "mfma"),
            ("proj dX", lambda: HF.stgcn_conv_dx(y3, k1t, Tn, 1, 0), 2 * M * 3 * C * C, 4 * e, "mfma"),
            ("proj dW", lambda: HF.stgcn_conv_dw(x, y3, W1.shape, 1, 0), 2 * M * 3 * C * C, 4 * e, "mfma"),
            ("aggregate fwd", lambda: HF.stgcn_aggregate(y3, A, E), 2 * M * 3 * V * C, 4 * e, "hbm"),
            ("aggregate bwd", lambda: HF.stgcn_aggregate_backward(y3, x, A, E, True), 4 * M * 3 * V * C, 7 * e, "hbm"),
            ("bn stats", lambda: HF.stgcn_bn_stats(x), 3 * M * C, e, "hbm"),
            ("bn apply+relu+res", lambda: HF.stgcn_bn_apply(x, mean, rstd, gamma, bias, True, x), 4 * M * C, 3 * e, "hbm"),
            ("bn backward", lambda: HF.stgcn_bn_backward(x, x, x, mean, rstd, gamma, True), 10 * M * C, 7 * e, "hbm"),
            ("colsum (bias grad)", lambda: HF.stgcn_colsum(x), M * C, e, "hbm"),
            ("pool fwd", lambda: HF.stgcn_pool(x.view(B, Tn * V, C)), M * C, e, "hbm"),
        )
        for name, fn, flops, nbytes, roof in KERNELS:
            ms = timed(torch, fn, args.iters)
            share = flops / (ms * 1e-3) / MFMA if roof == "mfma" else nbytes / (ms * 1e-3) / HBM
            r = {"table": "kernels", "kernel": name, "T": Tn, "C": C, "us": round(ms * 1e3, 1), "gflop": round(flops / 1e9, 2),
                 "mbyte": round(nbytes / 1e6, 1), "roof": roof, "share": round(share, 3)}
            if roof == "mfma":
                r["tflops"] = round(flops / (ms * 1e-3) / 1e12, 1)
            rows.append(r)
            print(f"kernel {name:20s} T {Tn:3d} C {C:3d} {r['us']:10.1f} us  {r['gflop']:8.2f} GFLOP {r['mbyte']:8.1f} MB  "
                  f"{share:.3f} of {'MFMA fp32 peak' if roof == 'mfma' else 'HBM'}", flush=True)
    return rows


def stock_model(torch, m):
    """the same network on torch library ops, channels-first, reading the HIP model's own parameters and buffers"""
    import torch.nn.functional as F

    def bn(x, mod, training):
        return F.batch_norm(x, mod.running_mean, mod.running_var, mod.weight, mod.bias, training, mod.momentum, mod.eps)

    def forward(x):
        training = m.training
        N, Tn, Vn, C = x.shape
        h = bn(x.permute(0, 2, 3, 1).reshape(N, Vn * C, Tn), m.data_bn, training)
        h = h.view(N, Vn, C, Tn).permute(0, 2, 3, 1).contiguous()
        for blk, imp in zip(m.st_gcn_networks, m.edge_importance):
            y = F.conv2d(h, blk.gcn.conv.weight, blk.gcn.conv.bias)
            y = y.view(N, 3, -1, y.shape[2], Vn)
            a = torch.einsum("nkctv,kvw->nctw", y, m.A * imp if imp is not None else m.A).contiguous()
            c = F.relu(bn(a, blk.tcn[0], training))
            c = bn(F.conv2d(c, blk.tcn[2].weight, blk.tcn[2].bias, (blk.stride, 1), (4, 0)), blk.tcn[3], training)
            if blk.residual_kind == 1:
                c = c + h
            elif blk.residual_kind == 2:
                c = c + bn(F.conv2d(h, blk.residual[0].weight, blk.residual[0].bias, (blk.stride, 1)), blk.residual[1], training)
            h = F.relu(c)
        feat = F.dropout(h.mean(dim=(2, 3)), m.head.dropout_ratio, training)
        return m.head.classifier(feat)

    return forward


def part_steps(args):
    torch, hw, HF, train, DEV = _gpu()
    x = torch.rand(B, T, V, 2, device=DEV)
    y = torch.randint(0, NCLASS, (B,), device=DEV)
    crit = train.SmoothedCrossEntropyLoss()

    def fresh():
        torch.manual_seed(0)
        m = hw.STGCNModel(*hw.STGCNParams({"num_class": NCLASS}, 2).get_model_params()).to(DEV).train()
        return m, torch.optim.AdamW(m.parameters(), lr=5e-4, fused=True, capturable=True)

    m_e, o_e = fresh()
    m_g, o_g = fresh()
    m_s, o_s = fresh()
    stock = stock_model(torch, m_s)

    def stock_step(xs, ys):
        o_s.zero_grad(set_to_none=True)
        loss = crit(stock(xs), ys)
        loss.backward()
        o_s.step()
        return loss

    legs = {"hip eager": train.TrainStep(m_e, o_e), "hip graphed": train.GraphedTrainStep(m_g, o_g, x, y), "stock torch": stock_step}
    m_ev, _ = fresh()
    m_ev.eval()
    stock_ev = stock_model(torch, m_ev)

    def run(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return B * n / (a.elapsed_time(b) * 1e-3)

    rows = []
    for _ in range(3):                                                  # warm every leg
        for step in legs.values():
            step(x, y)
        with torch.no_grad():
            m_ev(x), stock_ev(x)
    torch.cuda.synchronize()
    for rep in range(2):                                                # alternate the legs, two repeats
        for name, step in legs.items():
            cps = run(lambda: step(x, y), args.steps)
            rows.append({"table": "steps", "leg": "train " + name, "repeat": rep, "clips_per_s": round(cps, 1)})
            print(f"step train {name:12s} repeat {rep}  {cps:9.1f} clips/s  {B / cps * 1e3:8.2f} ms/step", flush=True)
        with torch.no_grad():
            for name, fn in (("hip", lambda: m_ev(x)), ("stock torch", lambda: stock_ev(x))):
                cps = run(fn, args.steps)
                rows.append({"table": "steps", "leg": "eval " + name, "repeat": rep, "clips_per_s": round(cps, 1)})
                print(f"step eval  {name:12s} repeat {rep}  {cps:9.1f} clips/s  {B / cps * 1e3:8.2f} ms/forward", flush=True)
    # the two paths compute the same thing: one train forward on equal weights
    m_a, _ = fresh()
    m_b, _ = fresh()
    m_a.head.dropout_ratio = m_b.head.dropout_ratio = 0.0
    with torch.no_grad():
        d = (m_a(x) - stock_model(torch, m_b)(x)).norm() / m_a(x).norm()
    print(f"hip vs stock train logits, equal weights: relative L2 distance {d.item():.2e}", flush=True)
    rows.append({"table": "steps", "leg": "hip vs stock logits", "rel_l2": float(d)})
    return rows


def part_trace_child(args):
    torch, hw, HF, train, DEV = _gpu()
    m = hw.STGCNModel(*hw.STGCNParams({"num_class": NCLASS}, 2).get_model_params()).to(DEV).train()
    x = torch.rand(B, T, V, 2, device=DEV)
    y = torch.randint(0, NCLASS, (B,), device=DEV)
    step = train.TrainStep(m, torch.optim.AdamW(m.parameters(), lr=5e-4, fused=True, capturable=True))
    for _ in range(4):
        step(x, y)
    torch.cuda.synchronize()
    return []


def part_trace(args):
    """runs the traced steps under rocprofv3 in a child of this child; returns the top kernels by total time"""
    import csv
    import glob
    import tempfile
    out = tempfile.mkdtemp(prefix="stgcn_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "stgcn", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--part", "trace_child"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    if files:
        with open(files[0]) as fh:
            for rec in list(csv.DictReader(fh))[:16]:
                r = {"table": "trace", "kernel": rec.get("Name", "")[:90], "calls": int(rec.get("Calls", 0)),
                     "total_us": round(float(rec.get("TotalDurationNs", 0)) / 1e3, 1), "percent": float(rec.get("Percentage", 0))}
                rows.append(r)
                print(f"trace {r['percent']:6.2f} %  {r['total_us']:11.1f} us  {r['calls']:5d} x  {r['kernel']}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "stgcn_lab.json"))
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "stgcn_lab.txt"))
    ap.add_argument("--part", default=None, help="(internal) run one part in this process and print its rows as JSON")
    args = ap.parse_args()
    if args.part:
        rows = {"kernels": part_kernels, "steps": part_steps, "trace": part_trace,
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
