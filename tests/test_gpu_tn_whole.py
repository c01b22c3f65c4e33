"""GPU parity of the whole-weight fp32 dW kernel of the narrow layers (csrc/gemm_f32_tnw.hip: one workgroup holds all of
dW, M split over the CUs, partial tiles through workspace slabs) vs fp64 torch: every (N, K) the dispatcher sends there,
at token counts below the ring depth, with uneven M slices and at a full grid; all three prologues; the workspace,
plain and deterministic entry points; accumulation; the ragged tail launch."""
import importlib

import pytest
import torch

from helpers import linear_parity

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
DEV = "cuda:0"
# the bounds of the existing dW tests, copied from tests/test_gpu_gemm.py (TOL: norm-wise; TN_F32: entry-wise and per
# 128 x 128 tile of dW, db norm and entry)
TOL = 2e-5
TN_F32 = dict(tol_entry=3.6e-6, tile=(128, 128), tol_tile=1.9e-6)
SHAPES = [(128, 128), (256, 128), (128, 256), (384, 128)]            # every (N, K) hwgat_linear_tn_f32 routes to the kernel
# 32: two stages, fewer than the ring is deep, one workgroup; 32 * 5; 32 * 257: uneven slices, the last one short;
# 8192: 32 slices of the least depth; 65536: a slice on every CU
MS = [32, 32 * 5, 32 * 257, 8192, 65536]
PROS = ["plain", "drop", "ln"]
# (128 x 128 with the dropout prologue is not sent to this kernel: gemm_tn_k is faster there, and tests/test_gpu_gemm.py has it)
CASES = [(N, K, pro) for N, K in SHAPES for pro in PROS if (N, K, pro) != (128, 128, "drop")]


def _inputs(M, N, K, pro):
    g = torch.Generator(device=DEV).manual_seed(M + 3 * N + K)
    dY = torch.randn(M, N, device=DEV, generator=g)
    X = torch.randn(M, K, device=DEV, generator=g) + 0.3
    dW0 = torch.randn(N, K, device=DEV, generator=g)
    kw, A64, B64 = {}, dY.double(), X.double()
    if pro == "drop":
        kw = dict(pro_seed=9, pro_p=0.1)
        A64 = A64 * HF.dropout_mask((M, N), 9, 0.1, DEV).double()
    elif pro == "ln":
        gamma, beta = torch.randn(K, device=DEV, generator=g), torch.randn(K, device=DEV, generator=g)
        mean = X.mean(-1)
        rstd = (X.var(-1, unbiased=False) + 1e-5).rsqrt()
        kw = dict(ln=(mean, rstd, gamma, beta))
        B64 = torch.nn.functional.layer_norm(B64, (K,), gamma.double(), beta.double())
    return dY, X, dW0, kw, A64.t() @ B64, A64.sum(0)


def _plain_entry(dY, X, dW, db, pro_seed=0, pro_p=0.0, ln=None):
    """hwgat_linear_tn_f32: no workspace (float atomics over the M slices)"""
    N, K = dW.shape
    mean, rstd, gamma, beta = ln if ln is not None else (None, None, None, None)
    HF.call("hwgat_linear_tn_f32", HF.ptr(dY), HF.ptr(X), HF.ptr(dW), HF.ptr(db), dY.shape[0], N, K, pro_seed, float(pro_p),
            HF.ptr(mean), HF.ptr(rstd), HF.ptr(gamma), HF.ptr(beta), None, HF.stream())


@pytest.mark.parametrize("N,K,pro", CASES)
def test_whole_weight_dw_every_entry_point_against_fp64(N, K, pro):
    for M in MS:
        dY, X, dW0, kw, upd, dbr = _inputs(M, N, K, pro)
        tag = f"tn_whole {M}x{N}x{K} {pro}"
        assert hw._lib.lib().hwgat_linear_tn_f32_ws_bytes(M, N, K) > 0       # the dispatcher's answer: slabs of this kernel
        # workspace entry point, onto existing contents: the update against fp64, the same bits on every run
        runs = []
        for _ in range(2):
            dW, db = dW0.clone(), torch.zeros(N, device=DEV)
            HF.linear_tn(dY, X, dW, db, **kw)
            runs.append(dW)
        assert torch.equal(runs[0], runs[1]), tag
        linear_parity((runs[0].double() - dW0.double(), db), (upd, dbr), tol_norm=TOL, **TN_F32, what=tag + " ws")
        # two calls give twice the update
        dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        HF.linear_tn(dY, X, dW, db, **kw)
        HF.linear_tn(dY, X, dW, db, **kw)
        linear_parity((dW, db), (2 * upd, 2 * dbr), tol_norm=TOL, **TN_F32, what=tag + " ws twice")
        # no workspace
        dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        _plain_entry(dY, X, dW, db, **kw)
        linear_parity((dW, db), (upd, dbr), tol_norm=TOL, **TN_F32, what=tag + " plain")
        # deterministic entry point: fp64, and the same bits (dW and db) on every run
        runs = []
        for _ in range(2):
            dW, db = dW0.clone(), torch.zeros(N, device=DEV)
            HF.linear_tn(dY, X, dW, db, deterministic=True, **kw)
            runs.append((dW, db))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), tag
        linear_parity((runs[0][0].double() - dW0.double(), runs[0][1]), (upd, dbr), tol_norm=TOL, **TN_F32, what=tag + " det")


@pytest.mark.parametrize("N,K,pro", CASES)
def test_ragged_token_count_goes_through_the_tail_launch(N, K, pro):
    """M % 32 != 0: the whole stages on this kernel, the last 17 rows on gemm_tn_k's RAGGED launch; nothing is written
    behind dW or db"""
    M = 32 * 9 + 17
    dY, X, _, kw, upd, dbr = _inputs(M, N, K, pro)
    wbuf, bbuf = torch.full((N + 8, K), 777.0, device=DEV), torch.full((N + 64,), 777.0, device=DEV)
    dW, db = wbuf[:N], bbuf[:N]
    dW.zero_()
    db.zero_()
    HF.linear_tn(dY, X, dW, db, **kw)
    linear_parity((dW, db), (upd, dbr), tol_norm=TOL, **TN_F32, what=f"tn_whole ragged {N}x{K} {pro}")
    assert bool((wbuf[N:] == 777.0).all()) and bool((bbuf[N:] == 777.0).all())
