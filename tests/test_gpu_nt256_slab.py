"""gemm_nt256_k (fp32 256 x 256 NT linear): the slab pipeline's LDS hand-over at its edges.

The kernel keeps two LDS buffers and ONE barrier per 32-deep K slab: a slab's last chunk already reads the next slab's
first fragments, and a tile's last slab reads the next TILE's.  A misplaced barrier is a race on a buffer, which shows
only for some slab counts and tile walks and not on every run.  So: the smallest K the router sends to this kernel (four
slabs) and an odd slab count (five: successive tiles of a workgroup start in alternating buffers), each on every tile
walk (one tile on one workgroup; one tile on each of 130; two workgroups with two tiles; the un-swizzled tail of the XCD
order; a 128-row remainder launch), every prologue / epilogue pair, and every launch FIVE times on the same inputs: the
kernel has no atomics on C or C2, so any difference between two launches is a race.

Values are checked by test_gpu_gemm's _persistent_loop (fp64 reference, entry-wise parity, the families' tolerances)."""
import pytest
import torch

import test_gpu_gemm as G
from helpers import linear_parity, rel_err

pytestmark = pytest.mark.gpu
HF, DEV = G.HF, G.DEV
REPEAT = 5

# (M, N): tiles of 256 x 256 -> what the 256 persistent workgroups walk
_WALKS = [
    (256 * 130, 256),           # 130 tiles: one each, "no next tile" re-reads its own
    (256 * 129, 512),           # 258 tiles: two workgroups walk two tiles, the rest one
    (256 * 257, 512),           # 514 tiles, 257 % 8 = 1 row blocks: the un-swizzled tail of the XCD order
    (256 * 129 + 128, 512),     # 258 tiles and the 128-row remainder launch
]
_KS = [128, 160]                # four slabs (the smallest K routed here) and five (an odd count)


def _same(a, b):
    if isinstance(a, tuple):
        return all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


def _five_times(monkeypatch):
    """every _nt launch of test_gpu_gemm runs REPEAT times into fresh NaN-filled outputs; all results bit-equal"""
    nt = G._nt

    def launch(A, W, bias=None, **kw):
        first = nt(A, W, bias, **dict(kw))
        for r in range(1, REPEAT):
            again = nt(A, W, bias, **dict(kw))
            assert _same(first, again), f"launch {r} differs from launch 0: a race"
        return first

    monkeypatch.setattr(G, "_nt", launch)


def _blocks(nb):
    return sorted({0, 1, 7, 8, nb // 2, nb - 3, nb - 2, nb - 1})


@pytest.mark.parametrize("pro,epi", G._LOOP_CASES + G._TRAIN_CASES)
@pytest.mark.parametrize("K", _KS)
@pytest.mark.parametrize("M,N", _WALKS)
def test_nt256_slab_counts_and_tile_walks(M, N, K, pro, epi, monkeypatch):
    _five_times(monkeypatch)
    G._persistent_loop(M, N, K, pro, epi, torch.float32, _blocks)


@pytest.mark.parametrize("pro,epi", G._LOOP_CASES + G._TRAIN_CASES)
def test_k96_is_declined_to_the_128_tile_kernel(pro, epi, monkeypatch):
    """K = 96 < 128: hwgat_linear_nt_f32_ex keeps the launch on gemm_nt_k, whatever the tile count"""
    _five_times(monkeypatch)
    G._persistent_loop(256 * 129, 512, 96, pro, epi, torch.float32, _blocks)


@pytest.mark.parametrize("K", _KS)
@pytest.mark.parametrize("M,N,F,Kt", [(256, 256, 2, 128),           # ONE tile on one workgroup: statistics route here below 128 tiles
                                      (256 * 129, 512, 2, 128)])    # 258 tiles
def test_nt256_row_statistics_and_merged_store_at_the_edges(M, N, K, F, Kt):
    """as test_nt_epilogue_row_statistics_and_merged_store: torch.equal against the plain launch, statistics to 1e-5"""
    p = 0.1
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    A = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) * 0.1
    b = torch.randn(N, device=DEV, generator=g)
    res = torch.randn(M, N, device=DEV, generator=g) + 0.7
    kw = dict(epi=HF.EPI_BIAS_DROP_RES, res=res, epi_seed=9, epi_p=p)
    plain = G._nt(A, W, b, **kw)
    ref = res.double() + (A.double() @ W.double().t() + b.double()) * HF.dropout_mask((M, N), 9, p, DEV).double()
    linear_parity(plain, ref, tol_norm=G.TOL, **G.NT_F32, what="nt_f32: drop_res at the slab edges")
    pd = plain.double()
    assert M % (F * Kt) == 0
    Bn = M // (F * Kt)
    want = plain.view(Bn, F // 2, 2, Kt, N).transpose(2, 3).reshape(Bn, F // 2, Kt, 2 * N)
    wd = want.double().view(-1, 2 * N)
    for r in range(REPEAT):
        out, mean, rstd = G._nt(A, W, b, stats=True, **kw)
        assert torch.equal(out, plain), f"launch {r}"
        assert rel_err(mean.cpu(), pd.mean(-1).cpu()) < 1e-5
        assert rel_err(rstd.cpu(), (pd.var(-1, unbiased=False) + 1e-5).rsqrt().cpu()) < 1e-5
        mg, mean2, rstd2 = G._nt(A, W, b, stats=True, merge=(F, Kt), **kw)
        assert mg.shape == want.shape and torch.equal(mg, want), f"launch {r}"
        assert rel_err(mean2.cpu(), wd.mean(-1).cpu()) < 1e-5
        assert rel_err(rstd2.cpu(), (wd.var(-1, unbiased=False) + 1e-5).rsqrt().cpu()) < 1e-5
