"""CPU proof that helpers.tensor_parity / linear_parity have teeth on the linear and LayerNorm families: faults planted in
the best result a kernel can deliver (the fp64 product of the rounded operands, rounded to the storage type) that the old
whole-output norm checks accept must be rejected at the CAPS the GPU tests' entry / row / column bounds have to respect
(bf16-stored outputs: entry 1.2e-2, row and column 1e-2; fp32 outputs: 1e-5 each), with the right metric and index named,
while the unfaulted results pass at the same caps.

Three of the planted faults are so large that the old norm already rejects them (a dW tile that lacks an M slice: ~0.35 of
that tile; a whole dgamma entry off by 5 % against the 1e-4 the fp32 tests use; the shifted dropout mask at the smaller
shape, 1.5e-2 against 6e-3) -- for those the test asserts that, and that the new check names the tile / the entry / the
row, which the norm cannot."""
import pytest
import torch

from helpers import entrywise, linear_parity, rel_err, tensor_parity

BT, TOL = 6e-3, 2e-5                                   # the old norm bounds (tests/test_gpu_gemm.py)
OLD_DW_BF16 = 1e-2                                     # test_tn64_weight_gradients before this file existed
BF16_CAP = dict(tol_entry=1.2e-2, tol_row=1e-2, tol_col=1e-2)
F32_CAP = dict(tol_entry=1e-5, tol_row=1e-5, tol_col=1e-5)
SHAPES = [(512, 256, 128), (1536, 512, 1024)]


def _data(M, N, K, seed):
    """the operands of tests/test_gpu_gemm.py::_data (that module needs a GPU to import)"""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    return A, W, b


def _b(x):
    return x.to(torch.bfloat16)


def _case(M, N, K):
    """(fp64 reference of bf16 operands + fp32 bias, its bf16 rounding = the best a bf16 kernel can store, bias)"""
    A, W, b = _data(M, N, K, 5)
    ref = _b(A).double() @ _b(W).double().t() + b.double()
    return ref, _b(ref.float()).double(), b.double()


def _old_accepts(got, ref, bound=BT):
    e = rel_err(got, ref)
    assert e < bound, e
    return e


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_clean_results_pass_at_the_caps(M, N, K):
    ref, clean, _ = _case(M, N, K)
    errs = tensor_parity(clean, ref, tol_norm=BT, tile=(128, 128), tol_tile=BT, what="clean bf16", **BF16_CAP)
    assert set(errs) == {"norm", "entry", "row", "col", "tile"}
    assert errs["norm"] == pytest.approx(rel_err(clean, ref)) and errs["entry"] == pytest.approx(entrywise(clean, ref))
    assert 1e-3 < errs["entry"] < 6e-3 and 1e-3 < errs["row"] < 5e-3 and 1e-3 < errs["col"] < 5e-3     # the rounding itself
    # a plain fp32 evaluation of the same product at the fp32 caps
    A, W, b = _data(M, N, K, 5)
    errs = tensor_parity(A @ W.t() + b, A.double() @ W.double().t() + b.double(), tol_norm=TOL, what="clean fp32", **F32_CAP)
    assert errs["entry"] < 2e-6 and errs["row"] < 2e-6 and errs["col"] < 2e-6
    # leading dimensions are flattened; a vector gets norm and entry only
    tensor_parity(clean.view(4, M // 4, N), ref.view(4, M // 4, N), tol_norm=BT, **BF16_CAP)
    out = linear_parity((clean, clean.sum(0)), (ref, ref.sum(0)), tol_norm=(BT, 1e-3), tol_entry=(1.2e-2, 1e-3), tol_row=1e-2,
                        tol_col=1e-2, what="pair")
    assert out[1]["row"] is None and out[1]["col"] is None and out[0]["row"] is not None


def test_non_finite_entries_are_named():
    ref, clean, _ = _case(*SHAPES[0])
    bad = clean.clone()
    bad[17, 200] = float("nan")                            # an element a kernel never stored into a poisoned buffer
    with pytest.raises(AssertionError, match=r"not finite: 1 entries, the first at \(17, 200\)"):
        tensor_parity(bad, ref, tol_norm=BT, **BF16_CAP)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_element_set_to_zero_is_rejected(M, N, K):
    ref, clean, _ = _case(M, N, K)
    mag = ref.abs().flatten()
    flat = int((mag - mag.median()).abs().argmin())          # an element of ordinary size: the median |entry|
    i, j = divmod(flat, N)
    bad = clean.clone()
    bad[i, j] = 0.0
    _old_accepts(bad, ref)
    with pytest.raises(AssertionError, match=rf"entry-wise error .*worst entry \({i}, {j}\): 0 vs"):
        tensor_parity(bad, ref, tol_norm=BT, what="zeroed", **BF16_CAP)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_columns_bias_off_by_5_percent_is_rejected(M, N, K):
    ref, clean, b = _case(M, N, K)
    rms = ref.norm().item() / (M * N) ** 0.5
    # the last column whose bias is at least 0.5 and at least half the RMS entry (a smaller one drowns in the product)
    j = int(torch.nonzero(b.abs() >= max(0.5, 0.5 * rms)).max())
    assert abs(b[j]) >= 0.5
    bad = _b((ref + 0.05 * b[j] * torch.nn.functional.one_hot(torch.tensor(j), N)).float()).double()
    _old_accepts(bad, ref)
    assert entrywise(bad, ref) < 1.2e-2                      # too small for the entry check: it takes the column metric
    with pytest.raises(AssertionError, match=rf"column error .*worst column {j},"):
        tensor_parity(bad, ref, tol_norm=BT, what="bias", **BF16_CAP)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_last_row_scaled_by_1_05_is_rejected(M, N, K):
    """what a wrong tail launch for ragged token counts would produce"""
    ref, clean, _ = _case(M, N, K)
    bad = clean.clone()
    bad[M - 1] = _b((ref[M - 1] * 1.05).float()).double()
    _old_accepts(bad, ref)
    with pytest.raises(AssertionError, match=rf"row error .*worst row {M - 1},"):
        tensor_parity(bad, ref, tol_norm=BT, what="tail", tol_entry=1.0, tol_row=1e-2, tol_col=1e-2)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dropout_mask_shifted_by_one_element_in_one_row_of_one_column_block_is_rejected(M, N, K):
    """EPI_BIAS_DROP_RES with the mask of one row moved by one element over one 128-wide column block (a hash indexed with
    the wrong column base): ~18 % of those 128 entries flip between dropped and kept"""
    lin, _, _ = _case(M, N, K)
    g = torch.Generator().manual_seed(M)
    res = _b(torch.randn(M, N, generator=g)).double()
    p = 0.1
    mask = (torch.rand(M, N, generator=g) >= p).double() / (1 - p)
    ref = res + lin * mask
    r, c0 = M // 2 + 1, N - 128
    shifted = mask.clone()
    shifted[r, c0:c0 + 128] = torch.roll(mask[r, c0:c0 + 128], 1)
    bad = _b((res + lin * shifted).float()).double()
    old = rel_err(bad, ref)
    print(f"mask shift ({M}, {N}, {K}): old norm error {old:.3g}")
    # one row of ~1.5-sigma flips against the norm of M rows: the old bound takes it once M * N is large enough
    assert (old < BT) == ((M, N, K) == SHAPES[1]), old
    with pytest.raises(AssertionError, match=rf"(entry-wise|row) error .*\({r}, "):
        tensor_parity(bad, ref, tol_norm=1.0, what="mask", **BF16_CAP)
    with pytest.raises(AssertionError, match=rf"row error .*worst row {r},"):
        tensor_parity(bad, ref, tol_norm=1.0, what="mask", tol_entry=1.0, tol_row=1e-2)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dw_tile_that_lacks_one_of_eight_m_slices_is_rejected(M, N, K):
    """fp32 dW[N, K] from bf16 operands with one 256 x 256 tile (clipped to dW) short of the rows of one M slice"""
    g = torch.Generator().manual_seed(K)
    dY, X = _b(torch.randn(M, N, generator=g)).double(), _b(torch.randn(M, K, generator=g)).double()
    ref = dY.t() @ X
    clean = ref.float().double()
    errs = linear_parity((clean, dY.sum(0).float()), (ref, dY.sum(0)), tol_norm=1e-4, tol_entry=1e-5, tile=(256, 256), tol_tile=1e-4)
    assert errs[0]["tile"] < 1e-6
    tn, tk = (N // 256 - 1) * 256, (K // 256 - 1) * 256 if K >= 256 else 0
    sl = slice(3 * M // 8, 4 * M // 8)
    bad = clean.clone()
    bad[tn:tn + 256, tk:tk + 256] -= (dY[sl, tn:tn + 256].t() @ X[sl, tk:tk + 256]).float()
    # a third of a tile is too much even for the loosest old bound (1e-2) while dW has fewer than ~1000 tiles: the norm
    # sees it, but cannot say where
    assert rel_err(bad, ref) > OLD_DW_BF16
    ti = (tn // 256, tk // 256)
    with pytest.raises(AssertionError, match=rf"tile error .*worst 256 x 256 tile \({ti[0]}, {ti[1]}\)"):
        tensor_parity(bad, ref, tol_norm=1.0, tol_entry=1.0, tile=(256, 256), tol_tile=1e-4, what="dW")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_one_db_entry_scaled_by_1_02_is_rejected(M, N, K):
    g = torch.Generator().manual_seed(N)
    dY = _b(torch.randn(M, N, generator=g)).double()
    ref = dY.sum(0)
    j = int(ref.abs().argmax())
    bad = ref.float().double()
    bad[j] *= 1.02
    _old_accepts(bad, ref, OLD_DW_BF16)                      # the bound test_tn64_weight_gradients held bf16 db to
    with pytest.raises(AssertionError, match="norm error"):
        linear_parity(bad, ref, tol_norm=1e-4, tol_entry=1e-5, what="db")
    with pytest.raises(AssertionError, match=rf"entry-wise error .*worst entry \(0, {j}\)"):
        linear_parity(bad, ref, tol_norm=1.0, tol_entry=1e-5, what="db")


@pytest.mark.parametrize("d", [128, 1024])
def test_one_dgamma_column_scaled_by_1_05_is_rejected(d):
    """bf16 LayerNorm backward at the model's widths had no reference check at all; against the 1e-4 of the fp32 tests a
    whole entry off by 5 % is already visible in the norm (0.05 / sqrt(d) at best) -- the entry check names the column"""
    g = torch.Generator().manual_seed(d)
    n = 1000
    x = (torch.randn(n, d, generator=g) * (0.5 + torch.rand(n, 1, generator=g)) + 3 * torch.randn(n, 1, generator=g)).double()
    dy = torch.randn(n, d, generator=g).double()
    xh = (x - x.mean(1, keepdim=True)) * (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    ref = (dy * xh).sum(0)
    j = int(ref.abs().argmax())
    bad = ref.float().double()
    bad[j] *= 1.05
    assert rel_err(bad, ref) > 1e-4
    with pytest.raises(AssertionError, match=rf"entry-wise error .*worst entry \(0, {j}\)"):
        tensor_parity(bad, ref, tol_norm=1.0, tol_entry=1e-5, what="dgamma")


def test_fp32_row_scaled_by_1_plus_3e_4_is_rejected():
    M, N, K = 512, 256, 128
    A, W, b = _data(M, N, K, 5)
    ref = A.double() @ W.double().t() + b.double()
    bad = (A @ W.t() + b).double()
    bad[M - 1] *= 1 + 3e-4
    _old_accepts(bad, ref, TOL)                              # 3e-4 / sqrt(512) = 1.3e-5 < 2e-5
    with pytest.raises(AssertionError, match=rf"(entry-wise|row) error .*\({M - 1}, "):
        tensor_parity(bad, ref, tol_norm=TOL, what="fp32 row", **F32_CAP)
    with pytest.raises(AssertionError, match=rf"row error .*worst row {M - 1},"):
        tensor_parity(bad, ref, tol_norm=TOL, tol_entry=1.0, tol_row=1e-5, what="fp32 row")


def test_fp32_element_off_by_1e_3_of_the_largest_entry_is_rejected():
    M, N, K = 512, 256, 128
    A, W, b = _data(M, N, K, 5)
    ref = A.double() @ W.double().t() + b.double()
    bad = (A @ W.t() + b).double()
    bad[300, 77] += 1e-3 * ref.abs().max()
    _old_accepts(bad, ref, TOL)
    with pytest.raises(AssertionError, match=r"entry-wise error .*worst entry \(300, 77\)"):
        tensor_parity(bad, ref, tol_norm=TOL, what="fp32 entry", **F32_CAP)
