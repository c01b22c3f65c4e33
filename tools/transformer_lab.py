#!/usr/bin/env python3
"""Cost of the Transformer baseline, three tables:

  1. attention  hwgat_seq_attn_fwd / _bwd at B = 64, 8 heads, head_dim 64, T in {64, 192, 512}, 0 % and ~10 % padded
                keys (tail frames), fp32 and bf16.  Median HIP-event time, and the fraction of the BINDING roof:
                max(flops / MFMA peak, bytes / 8 TB/s) as tools/width_lab.py computes it (peaks 157.3 TF fp32, 2.5 PF
                bf16 dense; flops of the dense T x T products, bytes = operands read once + outputs written once).
  2. step       clips/s of the eager train step (TrainStep, AdamW, smoothed CE) at B = 64, T in {64, 192} with the
                TransformerParams defaults (29 joints, C = 2, 2002 classes), fp32 and bf16 activations, against the same
                step on torch's stock nn.TransformerEncoder (same weights, same function): fp32, and bf16 autocast.
  3. graphed    clips/s of GraphedTrainStep for the backend rows of table 2.

  python tools/transformer_lab.py [--iters 20] [--steps 10] [--json profiles/transformer_lab.json]
"""
import argparse
import importlib
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train_mod = importlib.import_module("sl-hwgat_amd.train")

DEV = torch.device("cuda:0")
HBM = 8.0e12
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2.5e15}


def timed(fn, iters):
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


def attention_rows(iters):
    rows = []
    B, nH, hd = 64, 8, 64
    d = nH * hd
    for dt in (torch.float32, torch.bfloat16):
        es = torch.tensor([], dtype=dt).element_size()
        for T in (64, 192, 512):
            for frac in (0.0, 0.1):
                qkv = torch.randn(B, T, 3 * d, device=DEV, dtype=dt)
                do = torch.randn(B, T, d, device=DEV, dtype=dt)
                x0 = torch.zeros(B, T)
                x0[:, T - int(round(frac * T)):] = -1.0 if frac else 0.0
                words = torch.zeros(B, (T + 31) // 32, dtype=torch.int64)
                for t in range(T):
                    words[:, t // 32] |= (x0[:, t] == -1.0).to(torch.int64) << (t % 32)
                words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).to(DEV)
                o, lse = HF.seq_attn_forward(qkv, words, nH)
                ms_f = timed(lambda: HF.seq_attn_forward(qkv, words, nH), iters)
                ms_b = timed(lambda: HF.seq_attn_backward(qkv, o, do, lse, words, nH), iters)
                for kind, ms, flops, nbytes in (
                        ("fwd", ms_f, 4 * B * nH * T * T * hd, (3 * d + d) * B * T * es + B * nH * T * 4),
                        ("bwd", ms_b, 10 * B * nH * T * T * hd, (3 * d + 2 * d + 3 * d) * B * T * es + 2 * B * nH * T * 4)):
                    roof = max(flops / PEAK[dt], nbytes / HBM)
                    r = {"table": "attention", "dtype": str(dt).split(".")[-1], "T": T, "pad_frac": frac, "pass": kind,
                         "us": round(ms * 1e3, 1), "tflops": round(flops / (ms * 1e-3) / 1e12, 2),
                         "bound": "mfma" if flops / PEAK[dt] > nbytes / HBM else "hbm",
                         "roof_frac": round(roof / (ms * 1e-3), 3)}
                    rows.append(r)
                    print(f"attn {r['dtype']:8s} T={T:3d} pad={frac:.1f} {kind} {r['us']:9.1f} us {r['tflops']:7.2f} TF "
                          f"{r['bound']:4s} {r['roof_frac']:.3f} of roof", flush=True)
    return rows


class TorchTransformer(nn.Module):
    """the same function on torch's stock modules (post-norm, relu, batch_first, key_padding_mask)"""

    def __init__(self, F, nclass, d, nhead, ff, layers, dropout, max_len):
        super().__init__()
        self.encoder = nn.Linear(F, d)
        self.pe = nn.Parameter(torch.zeros(1, max_len, d), requires_grad=False)
        layer = nn.TransformerEncoderLayer(d, nhead, ff, dropout, batch_first=True, norm_first=False)
        self.enc = nn.TransformerEncoder(layer, layers, norm=nn.LayerNorm(d), enable_nested_tensor=False)
        self.drop = nn.Dropout(dropout)
        self.classifier = nn.Linear(d, nclass)
        self.d = d

    def load_from(self, m):
        with torch.no_grad():
            self.encoder.load_state_dict(m.encoder.state_dict())
            self.pe.copy_(m.pos_encoder.pe)
            for a, b in zip(self.enc.layers, m.transformer_encoder.layers):
                a.self_attn.load_state_dict(b.self_attn.state_dict())
                for n in ("linear1", "linear2", "norm1", "norm2"):
                    getattr(a, n).load_state_dict(getattr(b, n).state_dict())
            self.enc.norm.load_state_dict(m.transformer_encoder.norm.state_dict())
            self.classifier.load_state_dict(m.classifier.state_dict())
        return self

    def forward(self, src):
        B, T = src.shape[:2]
        x = src.reshape(B, T, -1)
        pad = x[:, :, 0] == -1
        h = self.drop(self.encoder(x) * self.d ** 0.5 + self.pe[:, :T])
        return self.classifier(self.enc(h, src_key_padding_mask=pad).mean(dim=1))


def step_rows(steps):
    rows = []
    B, nc = 64, 2002
    for T in (64, 192):
        tp = hw.TransformerParams({"src_len": T, "num_class": nc}, 2, DEV)
        g = torch.Generator().manual_seed(T)
        x = torch.rand(B, T, 29, 2, generator=g)
        x[: B // 8, T - T // 10:] = -1.0
        y = torch.randint(0, nc, (B,), generator=g)
        x, y = x.to(DEV), y.to(DEV)
        for dt in (torch.float32, torch.bfloat16):
            name = str(dt).split(".")[-1]
            torch.manual_seed(0)
            m = hw.TransformerModel(*tp.get_model_params()).to(DEV).set_activation_dtype(dt)
            ref = TorchTransformer(58, nc, 512, 8, 2048, 3, 0.1, T).to(DEV).load_from(m)
            m.train()
            ref.train()
            opt = torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True, capturable=True)
            step = train_mod.TrainStep(m, opt)
            ms = timed(lambda: step(x, y), steps)
            ropt = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-4, fused=True)
            crit = train_mod.SmoothedCrossEntropyLoss()

            def torch_step():
                ropt.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                    out = ref(x)
                crit(out, y).backward()
                ropt.step()
            ms_t = timed(torch_step, steps)
            graphed = train_mod.GraphedTrainStep(m, opt, x, y)
            ms_g = timed(lambda: graphed(x, y), steps)
            r = {"table": "step", "dtype": name, "T": T, "B": B, "backend_clips_s": round(B / (ms * 1e-3), 1),
                 "torch_clips_s": round(B / (ms_t * 1e-3), 1), "speedup": round(ms_t / ms, 3),
                 "graphed_clips_s": round(B / (ms_g * 1e-3), 1), "backend_ms": round(ms, 3), "torch_ms": round(ms_t, 3),
                 "graphed_ms": round(ms_g, 3)}
            rows.append(r)
            print(f"step {name:8s} T={T:3d} backend {r['backend_clips_s']:8.1f} clips/s  torch "
                  f"{r['torch_clips_s']:8.1f} clips/s  x{r['speedup']:.2f}  graphed {r['graphed_clips_s']:8.1f} clips/s",
                  flush=True)
            del m, ref, opt, ropt, step, graphed
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "transformer_lab.json"))
    a = ap.parse_args()
    rows = attention_rows(a.iters) + step_rows(a.steps)
    with open(a.json, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
