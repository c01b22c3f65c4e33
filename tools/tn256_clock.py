#!/usr/bin/env python3
"""What a 16-row stage of the fp32 256-tile dW kernel (csrc/gemm_f32_tn256.hip) costs beyond its MFMAs (LAB library): s_memtime at
the start and the end of every workgroup of `gemm_tn256_k`, slab form, at N = K = 512 (four 256 x 256 tiles, 64 M slices: one
round of 256 workgroups) and a sweep of M that gives every workgroup 32 ... 1 280 stages, plain and with LayerNorm on B.

    python tools/tn256_clock.py [LAB_LIBRARY]

LAB_LIBRARY: another build's libhwgat_hip_lab.so (same ABI), e.g. the parent commit's for an A/B of the kernel alone.

Per form: cycles per workgroup (median over the workgroups, then over five stamped launches) beside the 8 192 matrix-pipe cycles
per stage (128 v_mfma_f32_32x32x2_f32 of 64 cycles), and the least-squares line  cycles per workgroup = fixed + per-stage x n_it:
`fixed` is the prologue (two stages fetched with nothing to hide behind), the slab store and the launch skew inside a workgroup,
`per-stage` - 8 192 what the loop loses per stage (LABLOG 10.17)."""
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
lab.hwgat_lab_tn256_stamps.argtypes, lab.hwgat_lab_tn256_stamps.restype = [ctypes.c_void_p], ctypes.c_int
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
N = K = 512
TILES, SPLITS, STAGE_ROWS, STAGE_CYCLES = 4, 64, 16, 8192
GRID = TILES * SPLITS
st = torch.zeros(GRID * 2, device=dev, dtype=torch.int64)


def clock(n_it, ln, reps=5):
    """(wall us, median ticks per workgroup, live workgroups) of one slab-form launch + its reduce; median over `reps` launches"""
    M = SPLITS * STAGE_ROWS * n_it
    assert lab.hwgat_linear_tn_f32_ws_bytes(M, N, K) == SPLITS * TILES * 65536 * 4, "not the 256-tile kernel's one-round split"
    dY = torch.randn(M, N, device=dev, generator=g)
    X = torch.randn(M, K, device=dev, generator=g)
    dW, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    kw = {}
    if ln:
        kw["ln"] = (X.mean(-1), (X.var(-1, unbiased=False) + 1e-5).rsqrt(), torch.randn(K, device=dev, generator=g),
                    torch.randn(K, device=dev, generator=g))
    run = lambda: HF.linear_tn(dY, X, dW, db, **kw)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    got = []
    for _ in range(reps):
        st.zero_()
        assert lab.hwgat_lab_tn256_stamps(st.data_ptr()) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        lab.hwgat_lab_tn256_stamps(None)
        s = st.view(GRID, 2).cpu().double()
        live = s[:, 1] > 0
        # (the counters of different XCDs are not aligned: per-workgroup spans only)
        got.append((e0.elapsed_time(e1) * 1e3, (s[live, 1] - s[live, 0]).median().item(), int(live.sum())))
    got.sort(key=lambda r: r[1])
    return got[len(got) // 2]


print(f"# {lab_path}")
print(f"fp32 256-tile dW kernel, slab form, N = K = {N}: {GRID} workgroups of n_it 16-row stages each; median of 5 stamped launches")
for ln in (False, True):
    print(f"\n{'LayerNorm on B' if ln else 'plain'}")
    print("| n_it | M | wall us (kernel + reduce) | TFLOP/s | cycles per workgroup | 8 192 n_it | beyond | GHz >= |")
    print("|---|---|---|---|---|---|---|---|")
    xs, ys = [], []
    for n_it in (32, 64, 160, 320, 640, 1280):
        us, ticks, n_live = clock(n_it, ln)
        assert n_live == GRID, n_live
        M = SPLITS * STAGE_ROWS * n_it
        xs.append(float(n_it))
        ys.append(ticks)
        print(f"| {n_it} | {M} | {us:.1f} | {2.0 * M * N * K / us / 1e6:.1f} | {ticks:.0f} | {STAGE_CYCLES * n_it} | "
              f"{ticks - STAGE_CYCLES * n_it:.0f} | {ticks / us / 1e3:.2f} |", flush=True)
    n = len(xs)
    mx, my = sum(xs) / n, sum(ys) / n
    slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    print(f"fit: cycles per workgroup = {my - slope * mx:.0f} + {slope:.1f} x n_it   (fixed part; per stage {slope - STAGE_CYCLES:+.1f} "
          f"= {100 * (slope / STAGE_CYCLES - 1):.2f} % over {STAGE_CYCLES})")
