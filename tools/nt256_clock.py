#!/usr/bin/env python3
"""The shader clock the chip holds under the fp32 256-tile NT linear kernel (LAB library): s_memtime at the start and the end of
every persistent workgroup against the launch's wall time (HIP events), for plain launches of the three stages and for a
register-only MFMA loop (tools/mfma_peak.py measures 155 TFLOP/s with that).  What `peak` of the fp32-MFMA roofline is worth
under a real GEMM's LDS / HBM traffic.

    python tools/nt256_clock.py [LAB_LIBRARY]

LAB_LIBRARY: another build's libhwgat_hip_lab.so (same ABI), e.g. the parent commit's for an A/B of the kernel alone.

Second table: cycles per 256 x 256 tile against the 512 K cycles its MFMAs need, K = 128 ... 1 536 at ONE M, N (2 560 tiles, ten
per workgroup), and the least-squares line through them: cycles per tile = fixed + (1 + excess) 512 K.  `fixed` is the epilogue
and the tile boundary, `excess` what the slab loop loses beyond its MFMAs (LABLOG 10.11, 10.13)."""
import ctypes, importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hw = importlib.import_module("sl-hwgat_amd")
HF, L = hw.functional, hw._lib
lab_path = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "sl-hwgat_amd", "libhwgat_hip_lab.so")
lab = ctypes.CDLL(lab_path)
assert lab.hwgat_is_lab_build() == 1, "not the LAB library: build it with `python sl-hwgat_amd/build.py --lab`"
for name, args in L._SIGS.items():
    fn = getattr(lab, name)
    fn.argtypes, fn.restype = args, (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int)
L.lib()
L._lib = lab
lab.hwgat_lab_nt256_stamps.argtypes, lab.hwgat_lab_nt256_stamps.restype = [ctypes.c_void_p], ctypes.c_int
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
st = torch.zeros(256 * 2, device=dev, dtype=torch.int64)


def clock(M, N, K, reps=1):
    """(wall us, median ticks per workgroup, live workgroups) of the plain launch; the median over `reps` stamped launches"""
    A = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.05
    out = torch.empty(M, N, device=dev)
    run = lambda: HF.linear_nt(A, W, None, epi=HF.EPI_NONE, out=out)
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    got = []
    for _ in range(reps):
        st.zero_()
        assert lab.hwgat_lab_nt256_stamps(st.data_ptr()) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        lab.hwgat_lab_nt256_stamps(None)
        s = st.view(256, 2).cpu().double()
        live = s[:, 1] > 0
        # (the counters of different XCDs are not aligned: per-workgroup spans only)
        got.append((e0.elapsed_time(e1) * 1e3, (s[live, 1] - s[live, 0]).median().item(), int(live.sum())))
    got.sort(key=lambda r: r[1])
    return got[len(got) // 2]


print(f"# {lab_path}")
print("fp32 256-tile NT kernel, plain epilogue: shape, wall time, TFLOP/s, s_memtime ticks per workgroup (median), ticks / wall = clock")
for M, N, K in ((163840, 512, 1536), (163840, 512, 512), (327680, 256, 768), (327680, 512, 256), (655360, 256, 128)):
    us, ticks, n_live = clock(M, N, K)
    ghz = ticks / us / 1e3                                       # a workgroup lives for (almost) the whole launch: a lower bound
    print(f"M={M} N={N} K={K}: {us:8.1f} us {2.0 * M * N * K / us / 1e6:6.1f} TF | {n_live} workgroups, median {ticks:.0f} ticks each "
          f"-> >= {ghz:.2f} GHz; 157.3 TF at 2.4 GHz = {157.3 * ghz / 2.4:.1f} TF at this clock", flush=True)

M, N = 327680, 512                                               # 2 560 tiles: ten per workgroup, no tail round
per_wg = (M // 256) * (N // 256) // 256
print(f"\ncycles per tile against 512 K, M={M} N={N} ({per_wg} tiles per workgroup), median of 5 stamped launches")
print("| K | wall us | cycles per tile | MFMA cycles | beyond |")
print("|---|---|---|---|---|")
xs, ys = [], []
for K in (128, 256, 512, 768, 1024, 1536):
    us, ticks, _ = clock(M, N, K, reps=5)
    xs.append(512.0 * K)
    ys.append(ticks / per_wg)
    print(f"| {K} | {us:.1f} | {ys[-1]:.0f} | {xs[-1]:.0f} | {ys[-1] - xs[-1]:.0f} |", flush=True)
n = len(xs)
mx, my = sum(xs) / n, sum(ys) / n
slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
print(f"fit: cycles per tile = {my - slope * mx:.0f} + {slope:.4f} x 512 K   (fixed part, per-K excess {100 * (slope - 1):.2f} %)")
