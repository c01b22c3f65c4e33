#!/usr/bin/env python3
"""A/B of the fp32 weight-gradient launches of the narrow layers between TWO builds of the library, in alternating
launches of one process on one GPU: this tree's libhwgat_hip.so against the one given as argv[1] (e.g. the parent
commit's, built in a scratch checkout).  Each launch goes through hwgat_linear_tn_f32_ws with the workspace that build's
own hwgat_linear_tn_f32_ws_bytes asks for (hwgat_linear_tn_f32 where it asks for none), on the stage-0 shapes of the
headline config (B = 64: M = 655 360) with the prologue the fused block uses, plus the plain form, and on the single
256 x 256 tile of the stage-1 projection.  Prints the median time of both builds and the TFLOP/s per case."""
import ctypes
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
dev = "cuda:0"
reps = int(os.environ.get("TN_LAB_REPS", "12"))


def load(path):
    lib = ctypes.CDLL(path)
    for name in ("hwgat_linear_tn_f32_ws_bytes", "hwgat_linear_tn_f32_ws", "hwgat_linear_tn_f32"):
        fn = getattr(lib, name)
        fn.argtypes = hw._lib._SIGS[name]
        fn.restype = ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int
    return lib


libs = [("other", load(sys.argv[1])), ("this", hw._lib.lib())]
p = HF.ptr


def launcher(lib, dY, X, dW, db, seed, pp, ln):
    M, N, K = dY.shape[0], dW.shape[0], dW.shape[1]
    mean, rstd, gamma, beta = ln if ln else (None, None, None, None)
    need = lib.hwgat_linear_tn_f32_ws_bytes(M, N, K)
    ws = torch.empty(max(need // 4, 1), device=dev)

    def go():
        if need > 0:
            rc = lib.hwgat_linear_tn_f32_ws(p(dY), p(X), p(dW), p(db), M, N, K, seed, pp, p(mean), p(rstd), p(gamma), p(beta),
                                            p(ws), need, None, HF.stream())
        else:
            rc = lib.hwgat_linear_tn_f32(p(dY), p(X), p(dW), p(db), M, N, K, seed, pp, p(mean), p(rstd), p(gamma), p(beta), None,
                                         HF.stream())
        assert rc == 0, rc
    return go


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


M0 = 64 * 128 * 80
cases = [("qkv  ", M0, 384, 128, "ln"), ("proj ", M0, 128, 128, "drop"), ("fc1  ", M0, 256, 128, "ln"), ("fc2  ", M0, 128, 256, "drop"),
         ("qkv  ", M0, 384, 128, "plain"), ("proj ", M0, 128, 128, "plain"), ("fc1  ", M0, 256, 128, "plain"),
         ("fc2  ", M0, 128, 256, "plain"), ("proj1", M0 // 2, 256, 256, "drop"), ("proj1", M0 // 2, 256, 256, "plain")]
g = torch.Generator(device=dev).manual_seed(0)
for name, M, N, K, pro in cases:
    dY, X = torch.randn(M, N, device=dev, generator=g), torch.randn(M, K, device=dev, generator=g)
    dW, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    gamma, beta = torch.randn(K, device=dev, generator=g), torch.randn(K, device=dev, generator=g)
    ln = (X.mean(-1), (X.var(-1, unbiased=False) + 1e-5).rsqrt(), gamma, beta) if pro == "ln" else None
    fns = [launcher(lib, dY, X, dW, db, 7, 0.1 if pro == "drop" else 0.0, ln) for _, lib in libs]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[], []]
    for _ in range(reps):                                      # alternating launches
        for i, fn in enumerate(fns):
            times[i].append(timed(fn))
    med = [statistics.median(t) for t in times]
    fl = 2.0 * M * N * K
    print(f"{name} {pro:5s} M={M} N={N:3d} K={K:3d}: other {med[0] * 1e6:7.1f} us {fl / med[0] / 1e12:6.1f} TF | this {med[1] * 1e6:7.1f} us "
          f"{fl / med[1] / 1e12:6.1f} TF | min {min(times[0]) * 1e6:7.1f} / {min(times[1]) * 1e6:7.1f} us", flush=True)
    del dY, X
