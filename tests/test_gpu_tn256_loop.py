"""GPU parity of the fp32 256-tile dW kernel's stage loop (csrc/gemm_f32_tn256.hip: 16-row stages in a three-slot LDS ring, two
staging register sets, the loop body covers two stages) vs an fp64 product, at the smallest shapes at which the loop can go
wrong: one tile and two (the tile decode); two stages (every look-ahead clamped to the last stage), four, six (the ring wraps
twice) and four M slices of which the last is short; all three prologues; with and without the bias gradient; the slab, the
no-workspace and the deterministic forms; five launches of the slab and the deterministic form give the same bits."""
import functools
import importlib

import pytest
import torch

from helpers import linear_parity

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
DEV = "cuda:0"
# the bounds of tests/test_gpu_tn_whole.py (TOL: norm-wise; TN_F32: entry-wise and per 128 x 128 tile of dW, db norm and entry)
TOL = 2e-5
TN_F32 = dict(tol_entry=3.6e-6, tile=(128, 128), tol_tile=1.9e-6)
SHAPES = [(256, 256), (512, 256)]
# 32: two stages; 64; 96: six stages; 1056: four M slices of 288 rows, the last one 192
MS = [32, 64, 96, 1056]
PROS = ["plain", "ln", "drop"]


@functools.lru_cache(maxsize=None)
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


def _no_ws(dY, X, dW, db, pro_seed=0, pro_p=0.0, ln=None):
    """hwgat_linear_tn_f32: no workspace (float atomics over the M slices)"""
    N, K = dW.shape
    mean, rstd, gamma, beta = ln if ln is not None else (None, None, None, None)
    HF.call("hwgat_linear_tn_f32", HF.ptr(dY), HF.ptr(X), HF.ptr(dW), HF.ptr(db), dY.shape[0], N, K, pro_seed, float(pro_p),
            HF.ptr(mean), HF.ptr(rstd), HF.ptr(gamma), HF.ptr(beta), None, HF.stream())


def _slab(dY, X, dW, db, **kw):
    HF.linear_tn(dY, X, dW, db, **kw)


def _det(dY, X, dW, db, **kw):
    HF.linear_tn(dY, X, dW, db, deterministic=True, **kw)


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("pro", PROS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_stage_loop_every_form_against_fp64(N, K, pro, with_db):
    for M in MS:
        dY, X, dW0, kw, upd, dbr = _inputs(M, N, K, pro)
        assert hw._lib.lib().hwgat_linear_tn_f32_ws_bytes(M, N, K) > 0       # the dispatcher's answer: slabs of this kernel
        for name, entry in (("slab", _slab), ("no workspace", _no_ws), ("deterministic", _det)):
            tag = f"tn256 {M}x{N}x{K} {pro} {'db' if with_db else 'no db'} {name}"
            dW, db = dW0.clone(), (torch.zeros(N, device=DEV) if with_db else None)
            entry(dY, X, dW, db, **kw)
            got, ref = dW.double() - dW0.double(), upd
            if with_db:
                got, ref = (got, db), (upd, dbr)
            linear_parity(got, ref, tol_norm=TOL, **TN_F32, what=tag)


@pytest.mark.parametrize("pro", PROS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_five_launches_of_the_slab_and_the_deterministic_form_give_equal_bits(N, K, pro):
    for M in MS:
        dY, X, dW0, kw, _, _ = _inputs(M, N, K, pro)
        for name, entry in (("slab", _slab), ("deterministic", _det)):
            for with_db in (True, False):
                runs = []
                for _ in range(5):
                    dW, db = dW0.clone(), (torch.zeros(N, device=DEV) if with_db else None)
                    entry(dY, X, dW, db, **kw)
                    runs.append((dW, db))
                tag = f"tn256 {M}x{N}x{K} {pro} {name} {'db' if with_db else 'no db'}"
                assert all(torch.equal(r[0], runs[0][0]) for r in runs[1:]), tag
                # (db of the slab form is added with float atomics over the M slices: one slice, or the deterministic form)
                if with_db and (name == "deterministic" or M <= 96):
                    assert all(torch.equal(r[1], runs[0][1]) for r in runs[1:]), tag + " db"
