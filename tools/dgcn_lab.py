#!/usr/bin/env python3
"""Cost of the DecoupledGCN baseline at the size a user runs (B 64, T 128, V 29, C 2, default widths, fp32).  Three parts,
each a child process of its own under its own time limit (a part that fails ends the run; nothing is started after it):

  kernels  every new kernel (csrc/dgcn_ops.hip) at the three stage shapes (237 568 rows x 64, 118 784 x 128,
           59 392 x 256): median HIP-event time, algorithmic bytes from the shapes (every operand once; the models are in
           KERNELS below) and their share of the 8 TB/s HBM figure.
  steps    clips/s of the train step (zero_grad, forward at keep_prob 0.9, smoothed CE, backward, fused AdamW; eager
           TrainStep and GraphedTrainStep) and of the eval forward (eager and GraphedEval), alternated in one process with
           the STOCK path: the same network written with torch library ops (conv2d, batch_norm, einsum, conv1d,
           max_pool1d, torch.bernoulli; channels-first, what a user has today) on the same weights.  Warmed, --steps timed
           steps, device events, two repeats for the spread.
  trace    `rocprofv3 --kernel-trace --stats` around a few eager train steps (no timing taken from this run): where the
           step's time goes, kernel by kernel.

  python tools/dgcn_lab.py [--iters 20] [--steps 50] [--json profiles/dgcn_lab.json] [--txt profiles/dgcn_lab.txt]

--iters: timings per kernel (the median is reported); --steps: timed steps per leg and repeat.  Both results files begin
with the --iters and --steps of the run that wrote them, so a quoted figure can be traced to its command line.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (("kernels", 300), ("steps", 600), ("trace", 300))       # (part, time limit in seconds)
HBM = 8.0e12
B, T, V, NCLASS, G = 64, 128, 29, 2002, 8
STAGES = ((128, 64), (64, 128), (32, 256))                        # (frames, channels) of the three stages


def _gpu():
    import torch
    sys.path.insert(0, ROOT)
    hw = importlib.import_module("sl-hwgat_amd")
    return (torch, hw, hw.functional, importlib.import_module("sl-hwgat_amd.train"),
            importlib.import_module("sl-hwgat_amd.serve"), torch.device("cuda:0"))


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


def _model(hw, DEV, torch):
    torch.manual_seed(0)
    return hw.DecoupledGCNModel(*hw.DecoupledGCNParams({"num_class": NCLASS}, 2).get_model_params()).to(DEV)


def part_kernels(args):
    torch, hw, HF, _, _, DEV = _gpu()
    rows = []
    A = _model(hw, DEV, torch).l1.A.detach()
    for Tn, C in STAGES:
        M = B * Tn * V
        x, d = torch.randn(B, Tn, V, C, device=DEV), torch.randn(B, Tn, V, C, device=DEV)
        y3 = torch.randn(B, Tn, V, 3 * C, device=DEV)
        An = torch.rand(3, G, V, V, device=DEV)
        sv, st, sc = torch.rand(B, V, device=DEV), torch.rand(B, Tn, device=DEV), torch.rand(B, C, device=DEV)
        m1, m0 = torch.randn(B, Tn, C, device=DEV), torch.randn(B, V, C, device=DEV)
        mean, rstd = HF.stgcn_bn_stats(x)
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        bn = (mean, rstd, gamma, beta)
        pv, pt = torch.full((B, V), 0.03, device=DEV), torch.full((B, Tn), 0.01, device=DEV)
        seeds_v, seeds_t = HF.dgcn_draw(pv, 1), HF.dgcn_draw(pt, 2)
        fs, _ = HF.dgcn_mask_spatial(seeds_v, A)
        ft, _ = HF.dgcn_mask_temporal(seeds_t, 41)
        out = HF.dgcn_merge(x, bn, d, None, fs, ft, fs, ft)
        e = 4 * M * C                                       # bytes of one (M, C) fp32 tensor
        small = 4 * B * (V + Tn)
        KERNELS = (
            ("aggregate fwd", lambda: HF.dgcn_aggregate(y3, An, G), 4 * e),
            ("aggregate bwd (dy + dAn)", lambda: HF.dgcn_aggregate_backward(y3, x, An, G, True), 8 * e),
            ("gate sum over T", lambda: HF.dgcn_gate_sum(x, 0, 1.0 / Tn), e),
            ("gate sum over V (s_v)", lambda: HF.dgcn_gate_sum(x, 1, 1.0 / V, sv=sv), e),
            ("gate apply", lambda: HF.dgcn_gate_apply(x, sv, st, sc), 2 * e),
            ("gate grad sum over V", lambda: HF.dgcn_gate_sum(x, 1, 1.0, g=d, sv=sv), 2 * e),
            ("gate grad sum over T", lambda: HF.dgcn_gate_sum(x, 0, 1.0, g=d, st=st, sc=sc, m=m1, m_scale=1.0 / V), 2 * e),
            ("gate backward (dh)", lambda: HF.dgcn_gate_backward(d, sv, st, sc, m1, m0), 2 * e),
            ("drop |x| over (T, C)", lambda: HF.dgcn_abs_sum(x, 0, bn), e),
            ("drop |x| over (V, C)", lambda: HF.dgcn_abs_sum(x, 1, bn, fs), e),
            ("drop draw + spatial mask", lambda: HF.dgcn_mask_spatial(HF.dgcn_draw(pv, 1), A), small),
            ("drop draw + temporal mask", lambda: HF.dgcn_mask_temporal(HF.dgcn_draw(pt, 2), 41), small),
            ("drop merge", lambda: HF.dgcn_merge(x, bn, d, None, fs, ft, fs, ft), 3 * e),
            ("drop merge backward", lambda: HF.dgcn_merge_backward(d, out, fs, ft, fs, ft), 4 * e),
            ("masked sum", lambda: HF.dgcn_masked_sum(x, out, d, None), 4 * e),
        )
        for name, fn, nbytes in KERNELS:
            ms = timed(torch, fn, args.iters)
            share = nbytes / (ms * 1e-3) / HBM
            rows.append({"table": "kernels", "kernel": name, "T": Tn, "C": C, "us": round(ms * 1e3, 1),
                         "mbyte": round(nbytes / 1e6, 2), "share": round(share, 3)})
            print(f"kernel {name:28s} T {Tn:3d} C {C:3d} {ms * 1e3:10.1f} us  {nbytes / 1e6:9.2f} MB  {share:.3f} of HBM", flush=True)
    return rows


def stock_model(torch, m):
    """the same network on torch library ops, channels-first, reading the HIP model's own parameters and buffers (DropGraph
    with torch.bernoulli: the same distribution, not the same draws)"""
    import torch.nn.functional as F

    def bn(x, mod, training):
        return F.batch_norm(x, mod.running_mean, mod.running_var, mod.weight, mod.bias, training, mod.momentum, mod.eps)

    def drop_s(x, keep, A):
        n, c, t, v = x.shape
        a = x.abs().mean(dim=(1, 2)).detach()
        a = a / a.sum() * a.numel()
        M = torch.bernoulli(torch.clamp(a * ((1.0 - keep) / (1 + m.drop_size)), max=1.0)) @ A
        mask = (1 - (M > 0.001).to(x.dtype)).view(n, 1, 1, v)
        return x * mask * mask.numel() / mask.sum()

    def drop_t(x, keep, block):
        n, c, t, v = x.shape
        a = x.abs().mean(dim=(1, 3)).detach()
        a = (a / a.sum() * a.numel()).view(n, 1, t)
        M = torch.bernoulli(torch.clamp(a * ((1.0 - keep) / block), max=1.0))
        mask = (1 - F.max_pool1d(M, block, 1, block // 2)).view(n, 1, t, 1)
        return x * mask * mask.numel() / mask.sum()

    def unit(u, h, keep, training):
        g = u.gcn1
        N, _, Tn, Vn = h.shape
        Co = u.out_channels
        An = (g.decoupled_A / (g.decoupled_A.sum(2, keepdim=True) + 0.001)).repeat(1, Co // g.groups, 1, 1)
        y = torch.einsum("nctv,cd->ndtv", h, g.linear_weight) + g.linear_bias
        y = bn(y, g.bn0, training).view(N, 3, Co, Tn, Vn)
        a = bn(torch.einsum("nkctv,kcvw->nctw", y, An).contiguous(), g.bn, training)
        dn = bn(F.conv2d(h, g.down[0].weight, g.down[0].bias), g.down[1], training) if u.in_channels != Co else h
        y = F.relu(a + dn)
        s = torch.sigmoid(F.conv1d(y.mean(-2), u.conv_sa.weight, u.conv_sa.bias, padding=u.conv_sa.padding))
        y = y * s.unsqueeze(-2) + y
        s = torch.sigmoid(F.conv1d(y.mean(-1), u.conv_ta.weight, u.conv_ta.bias, padding=4))
        y = y * s.unsqueeze(-1) + y
        s = torch.sigmoid(F.linear(F.relu(F.linear(y.mean(-1).mean(-1), u.fc1c.weight, u.fc1c.bias)), u.fc2c.weight,
                                   u.fc2c.bias))
        y = y * s.unsqueeze(-1).unsqueeze(-1) + y
        c = bn(F.conv2d(y, u.tcn1.conv.weight, u.tcn1.conv.bias, (u.stride, 1), (4, 0)), u.tcn1.bn, training)
        r = None
        if u.residual_kind == 1:
            r = h
        elif u.residual_kind == 2:
            r = bn(F.conv2d(h, u.residual.conv.weight, u.residual.conv.bias, (u.stride, 1)), u.residual.bn, training)
        if training and keep != 1.0:
            c = drop_t(drop_s(c, keep, u.A), keep, 41)
            r = drop_t(drop_s(r, keep, u.A), keep, m.block_size)
        return F.relu(c if r is None else c + r)

    def forward(x, keep_prob=0.9):
        training = m.training
        N, Tn, Vn, C = x.shape
        h = bn(x.permute(0, 2, 3, 1).reshape(N, Vn * C, Tn), m.data_bn, training)
        h = h.view(N, Vn, C, Tn).permute(0, 2, 3, 1).contiguous()
        for i, u in enumerate(m.units, start=1):
            h = unit(u, h, keep_prob if i >= 7 else 1.0, training)
        feat = F.dropout(h.mean(dim=(2, 3)), m.head.dropout_ratio, training)
        return m.head.classifier(feat)

    return forward


def part_steps(args):
    torch, hw, HF, train, serve, DEV = _gpu()
    x = torch.rand(B, T, V, 2, device=DEV)
    y = torch.randint(0, NCLASS, (B,), device=DEV)
    crit = train.SmoothedCrossEntropyLoss()

    def fresh():
        m = _model(hw, DEV, torch).train()
        return m, torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)

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
    fast_ev = serve.GraphedEval(m_ev, x)

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
            m_ev(x), stock_ev(x), fast_ev(x)
    torch.cuda.synchronize()
    for rep in range(2):                                                # alternate the legs, two repeats
        for name, step in legs.items():
            cps = run(lambda: step(x, y), args.steps)
            rows.append({"table": "steps", "leg": "train " + name, "repeat": rep, "clips_per_s": round(cps, 1)})
            print(f"step train {name:12s} repeat {rep}  {cps:9.1f} clips/s  {B / cps * 1e3:8.2f} ms/step", flush=True)
        with torch.no_grad():
            for name, fn in (("hip eager", lambda: m_ev(x)), ("hip graphed", lambda: fast_ev(x)),
                             ("stock torch", lambda: stock_ev(x))):
                cps = run(fn, args.steps)
                rows.append({"table": "steps", "leg": "eval " + name, "repeat": rep, "clips_per_s": round(cps, 1)})
                print(f"step eval  {name:12s} repeat {rep}  {cps:9.1f} clips/s  {B / cps * 1e3:8.2f} ms/forward", flush=True)
    # the two paths compute the same thing: one train forward on equal weights without DropGraph (the draws differ)
    m_a, _ = fresh()
    m_b, _ = fresh()
    with torch.no_grad():
        d = (m_a(x, 1.0) - stock_model(torch, m_b)(x, 1.0)).norm() / m_a(x, 1.0).norm()
    print(f"hip vs stock train logits, equal weights, keep_prob 1: relative L2 distance {d.item():.2e}", flush=True)
    rows.append({"table": "steps", "leg": "hip vs stock logits", "rel_l2": float(d)})
    return rows


def part_trace_child(args):
    torch, hw, HF, train, _, DEV = _gpu()
    m = _model(hw, DEV, torch).train()
    x = torch.rand(B, T, V, 2, device=DEV)
    y = torch.randint(0, NCLASS, (B,), device=DEV)
    step = train.TrainStep(m, torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True,
                                                capturable=True))
    for _ in range(4):
        step(x, y)
    torch.cuda.synchronize()
    return []


def part_trace(args):
    """runs the traced steps under rocprofv3 in a child of this child; returns the top kernels by total time"""
    import csv
    import glob
    import tempfile
    out = tempfile.mkdtemp(prefix="dgcn_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "dgcn", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--part", "trace_child"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    rows = []
    if files:
        with open(files[0]) as fh:
            for rec in list(csv.DictReader(fh))[:24]:
                r = {"table": "trace", "kernel": rec.get("Name", "")[:90], "calls": int(rec.get("Calls", 0)),
                     "total_us": round(float(rec.get("TotalDurationNs", 0)) / 1e3, 1), "percent": float(rec.get("Percentage", 0))}
                rows.append(r)
                print(f"trace {r['percent']:6.2f} %  {r['total_us']:11.1f} us  {r['calls']:5d} x  {r['kernel']}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dgcn_lab.json"))
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "dgcn_lab.txt"))
    ap.add_argument("--part", default=None, help="(internal) run one part in this process and print its rows as JSON")
    args = ap.parse_args()
    if args.part:
        rows = {"kernels": part_kernels, "steps": part_steps, "trace": part_trace,
                "trace_child": part_trace_child}[args.part](args)
        print("ROWS " + json.dumps(rows), flush=True)
        return 0
    rows = [{"table": "run", "iters": args.iters, "steps": args.steps}]
    text = [f"run: python tools/dgcn_lab.py --iters {args.iters} --steps {args.steps}"]
    print(text[0], flush=True)
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
    return 0 if len(rows) > 1 and not text[-1].startswith("part ") else 1


if __name__ == "__main__":
    sys.exit(main())
