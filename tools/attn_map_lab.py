#!/usr/bin/env python3
"""Attention-map export (functional.attn_probs, csrc/attn_probs.hip) at the bench shapes, beside the fused forward of the
same kind, in one process: B 64, T 128 -- HWGATE's three stages ('win'), HGATE stage 0 ('blk'), WGATE ('band'), GATE
('wband'), fp32 and bf16 storage.  Per shape: probs only, received only and the forward, timed in alternating rounds with
device events (the median round is reported), each as a fraction of the 8 TB/s HBM roof from its ALGORITHMIC bytes:
q and k read once (2 E), P (4 bytes per entry) and / or received (4 B F K bytes) written once; the forward 4 E.

    python tools/attn_map_lab.py [--out profiles/attn_map_lab.txt] [--batch 64] [--frames 128]     (needs the GPU)
    python tools/attn_map_lab.py --resources                                                       (needs hipcc only)

--resources compiles csrc/attn_probs.hip with -Rpass-analysis=kernel-resource-usage and prints registers, LDS, scratch
and occupancy of every instantiation (scratch must be 0 everywhere); the profile file carries both parts."""
import argparse
import importlib
import importlib.util
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8e12


def resources():
    """[(kernel, VGPRs, SGPRs, scratch bytes / lane, LDS bytes, waves / SIMD)] of csrc/attn_probs.hip"""
    spec = importlib.util.spec_from_file_location("hwgat_build", os.path.join(ROOT, "sl-hwgat_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    src = os.path.join(build.CSRC, "attn_probs.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = subprocess.run([hipcc] + build.FLAGS + ["-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    out = []
    for r in rows:
        t = re.search(r"attn_probs_(pair|band)_kI(f|DF16b)Li(\d+)ELi(\d+)E", r["name"])
        label = f"{t.group(1)}<{'float' if t.group(2) == 'f' else 'bf16'}, HD {t.group(3)}, {'NMAX' if t.group(1) == 'pair' else 'NW'} {t.group(4)}>"
        out.append((label, int(r["VGPRs"]), int(r["TotalSGPRs"]), int(r["ScratchSize"]), int(r["LDS"]), int(r["Occupancy"])))
    return out


def print_resources(put):
    put("kernel-resource-usage of csrc/attn_probs.hip (hipcc --offload-arch=gfx950 -O3):")
    put(f"  {'instantiation':34s} {'VGPRs':>6s} {'SGPRs':>6s} {'scratch':>8s} {'LDS B':>7s} {'waves/SIMD':>11s}")
    rows = resources()
    for label, v, s, sc, lds, occ in rows:
        put(f"  {label:34s} {v:6d} {s:6d} {sc:8d} {lds:7d} {occ:11d}")
    assert rows and all(r[3] == 0 for r in rows), "an instantiation of attn_probs.hip spills to scratch"
    put(f"  {len(rows)} instantiations, 0 bytes of scratch in every one")


def timed(fns, rounds=5, n=20):
    """median over `rounds` of the mean time of n back-to-back calls, the callables alternating within a round"""
    import torch
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / n * 1e-3)
    return [statistics.median(t) for t in times]


def ring_band_rows(HF, W):
    """mask words of a band model whose frame graph is a ring with self loops, the same joint in the neighbouring frames"""
    import torch
    eye = torch.eye(W)
    a = ((eye + torch.roll(eye, 1, 1) + torch.roll(eye, -1, 1)) > 0).float()
    adj = torch.zeros(3, W, 3, W)
    for f in range(3):
        adj[f, :, f, :] = a
        if f:
            adj[f, :, f - 1, :] = eye
            adj[f - 1, :, f, :] = eye
    return HF.wband_mask_rows(adj.reshape(3 * W, 3 * W), 3, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_map_lab.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    lines = []

    def put(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.resources:
        print_resources(put)
        return
    import torch
    from oracle import hwgat_oracle as O
    from oracle import hgat_oracle as G
    from oracle import wgat_oracle as WO
    hw = importlib.import_module("sl-hwgat_amd")
    HF = hw.functional
    if not torch.cuda.is_available():
        raise SystemExit("attn_map_lab measures on the GPU: no device found")
    dev = "cuda:0"
    B, T = args.batch, args.frames
    shapes = [("HWGATE stage 0", "win", T, 64, 2, 64, HF.mask_bits(O.window_adjacency(4)), 16),
              ("HWGATE stage 1", "win", T // 2, 64, 4, 64, HF.mask_bits(O.window_adjacency(4)), 16),
              ("HWGATE stage 2", "win", T // 4, 64, 8, 64, HF.mask_bits(O.window_adjacency(4)), 16),
              ("HGATE stage 0", "blk", T, 29, 2, 64, HF.blk_mask_bits(G.block_adjacency(), 29), 29),
              ("WGATE", "band", T, 64, 8, 16, HF.band_mask_rows(WO.band_adjacency(4, 4), 4), 16),
              ("GATE", "wband", T, 29, 8, 16, ring_band_rows(HF, 29), 29)]
    put(f"attention-map export beside the fused forward, {torch.cuda.get_device_name(0)}, B {B}, T {T}; median of 5 alternating "
        f"rounds of 20 calls; fractions of {HBM / 1e12:.0f} TB/s from algorithmic bytes (2 E + outputs; forward 4 E)")
    put(f"{'shape':15s} {'kind':5s} {'dtype':8s} {'F':>4s} {'K':>3s} {'nH':>3s} {'hd':>3s} | {'probs us':>9s} {'of HBM':>6s} | "
        f"{'received us':>11s} {'of HBM':>6s} | {'forward us':>10s} {'of HBM':>6s} | {'received / forward':>18s}")
    for name, kind, F, K, nH, hd, mask, W in shapes:
        mask = mask.to(dev)
        d = nH * hd
        for dt in (torch.float32, torch.bfloat16):
            qkv = torch.randn(B, F, K, 3 * d, device=dev).to(dt)
            o = torch.empty(B, F, K, d, device=dev, dtype=dt)
            p = torch.empty(HF.attn_probs_shape(kind, B, F, K, W, nH), device=dev)
            r = torch.empty(B, F, K, device=dev)
            E = B * F * K * d * qkv.element_size()
            tp, tr, tf = timed([lambda: HF.attn_probs(kind, qkv, mask, nH, False, True, False, (p, None)),
                                lambda: HF.attn_probs(kind, qkv, mask, nH, False, False, True, (None, r)),
                                lambda: HF.attn_fwd(kind, qkv, o, mask, None, nH, False)])
            put(f"{name:15s} {kind:5s} {str(dt)[6:]:8s} {F:4d} {K:3d} {nH:3d} {hd:3d} | {tp * 1e6:9.1f} "
                f"{(2 * E + p.numel() * 4) / tp / HBM:6.3f} | {tr * 1e6:11.1f} {(2 * E + r.numel() * 4) / tr / HBM:6.3f} | "
                f"{tf * 1e6:10.1f} {4 * E / tf / HBM:6.3f} | {tr / tf:18.2f}")
            del qkv, o, p, r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
