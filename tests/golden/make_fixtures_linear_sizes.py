#!/usr/bin/env python3
"""Recorded results of the three workspace-sizing functions of the dW linears (pure host functions, no GPU):

    hwgat_linear_tn_f32_ws_bytes, hwgat_linear_tn_bf16_ws_bytes, hwgat_linear_tn_det_bytes

over the grid M x (N, K) below, written to tests/golden/linear_sizes.txt.  They follow from the M-split rules of the dW
launchers, so the file pins those rules: tests/test_host_cpu.py asserts that the library of the tree returns the same
numbers.

Run:  python tests/golden/make_fixtures_linear_sizes.py [LIBRARY] [COMMIT]

LIBRARY is the libhwgat_hip.so to record (default: the one built in this tree); COMMIT names the commit it was built
from and goes into the file's header.  The committed file was recorded with the library built from the PARENT of the
commit that put the split rule into one function (csrc/gemm_dispatch.h: tn_m_split), i.e. from the four hand-written
copies of the rule.  Regenerate it only with a change that means to alter a split.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "linear_sizes.txt")

MS = (32, 64, 96, 256, 4096, 32 * 301, 65536, 128 * 2003)
NKS = ((64, 64), (128, 128), (192, 192), (384, 128), (128, 384), (256, 256), (512, 256), (256, 512), (768, 768),
       (1536, 512), (512, 1536), (1024, 1024))
FUNCS = ("hwgat_linear_tn_f32_ws_bytes", "hwgat_linear_tn_bf16_ws_bytes", "hwgat_linear_tn_det_bytes")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "sl-hwgat_amd", "libhwgat_hip.so")
    commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"
    lib = ctypes.CDLL(path)
    for f in FUNCS:
        getattr(lib, f).argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
        getattr(lib, f).restype = ctypes.c_int64
    with open(OUT, "w") as fh:
        fh.write("# recorded by tests/golden/make_fixtures_linear_sizes.py from the library built at commit %s\n" % commit)
        fh.write("# (the parent of the commit that introduced tn_m_split)\n")
        fh.write("# M N K " + " ".join(FUNCS) + "\n")
        for M in MS:
            for N, K in NKS:
                fh.write("%d %d %d %s\n" % (M, N, K, " ".join(str(getattr(lib, f)(M, N, K)) for f in FUNCS)))
    print(OUT)


if __name__ == "__main__":
    main()
