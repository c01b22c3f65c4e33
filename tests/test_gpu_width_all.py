"""GPU parity at the stage widths that models/HWGATE.py::width_problem accepts and no power-of-two model asks for
(320 ... 960): the LayerNorm row map's edges (row counts around 4 rows per wave and 16 per block, with guard rows behind
every output, and the grid-stride loop past the block caps), the linears at the shapes of widths 320 ("small odd") and
960 ("largest") -- the 128 x 64 NT tile, the 128- and 256-wide NT tiles at K = 64 x odd, the 64 x 64 dW tile up to its
one-split branch -- and whole models at 448 / 896, 576, 704, 832 and 960 against the fp64 oracle
(oracle/hwgat_oracle.py, which test_oracle_golden.py pins to the reference).  References are fp64 torch on the CPU; the
bounds are test_gpu_width.py's and test_gpu_gemm.py's family tables, none of which had to move.

Observed on an MI355X over this module's cases, beside the bound that holds them (entry / row / column, or entry / tile):
  LN64_F32 2.1e-7 / 1.8e-7 of 7.5e-7 / 5.6e-7; LN64_BF16 3.3e-3 / 1.9e-3 of 1e-2 / 8.2e-3; LN64_DG 9.5e-7 of 1.4e-6 (the
  dbeta of 16403 rows of d = 960, atomic order; 1.8e-7 at the row-count edges)
  NT64_F32 1.5e-6 / 1.2e-6 / 9.8e-7 of 1.8e-6 / 1.6e-6 / 1.3e-6 (N 320 K 1280); NT64_F32_GELU 3.7e-6 / 1.0e-6 / 9.4e-7 of
  4.8e-6 / 1.8e-6 / 1.3e-6; NT64_BF16 4.6e-3 / 3.4e-3 / 8.9e-3 of 1.2e-2 / 1e-2 / 1e-2; NT64_BF16_FOLD 8.8e-3 / 3.8e-3 / 8.5e-3
  of 2.3e-2 / 1.5e-2 / 2.4e-2
  test_gpu_gemm's NT_F32 1.5e-6 / 6.5e-7 / 1.7e-6 of 6e-6 / 3.8e-6 / 4.7e-6; NT_F32_GELU 6.7e-6 / 6.2e-7 / 6.6e-7 of 2.2e-5 /
  3e-6 / 2e-6; NT_BF16 4.8e-3 / 3.2e-3 / 9.1e-3 of 1.1e-2 / 1e-2 / 1e-2; NT_BF16_FOLD 1.8e-2 / 3.7e-3 / 9.2e-3 of 3e-2 / 1.2e-2 /
  2e-2 (the 128- and 256-wide tiles at K = 320 and 960; the fp32 fold against test_gpu_gemm._fold_f32's derived bounds)
  TN64_F32 2.0e-6 / 8.3e-7 of 6e-6 / 2.4e-6; TN64_BF16 1.4e-6 / 2.7e-7 of 2.4e-6 / 7.7e-7; TN64_BF16_LN 3.4e-4 / 8.0e-5 of
  6.4e-4 / 9.2e-5
  whole models, fp32: logits 7.0e-7 (eval) / 6.5e-7 (train) of 1e-4, gradients 2.9e-6 / 3.7e-6 of 1e-3; bf16: eval logits
  5.4e-3 of 1e-2, train logits 9.9e-3 of 2e-2 (448 / 896), gradients 8.6e-3 (eval) / 4.7e-2 (train, norm1 of the first of
  704's two blocks: bf16 selector flips in it reach the second block's input; next 2.9e-2 at 448 / 896, the rest under 1e-2)
  of 5e-2; the key third of the qkv bias gradients, whose reference is zero, stays under all of these"""
import functools
import importlib

import pytest
import torch

import test_gpu_gemm as G
import test_gpu_width as W
from helpers import linear_parity, oracle_tie_free_thresholds, rel_err, tensor_parity
from oracle import hwgat_oracle as O

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
DEV = "cuda:0"
SENTINEL, GUARD = -12345.0, 8
DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------ LayerNorm: row-count edges, guarded outputs
def _guarded(rows, cols, dt, fill=float("nan")):
    """(buffer, live view): `rows` live rows (or entries, cols = None) filled with `fill` -- NaN: every element must be
    stored -- and GUARD rows of SENTINEL behind them, which nothing may touch"""
    shape = (rows + GUARD,) if cols is None else (rows + GUARD, cols)
    buf = torch.full(shape, SENTINEL, device=DEV, dtype=dt)
    buf[:rows] = fill
    live = buf[:rows]
    assert live.is_contiguous() and live.data_ptr() % 16 == 0
    return buf, live


def _guard_untouched(buf, rows):
    return bool((buf[rows:] == torch.full_like(buf[rows:], SENTINEL)).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("d", [320, 960])
def test_layernorm_row_count_edges_with_guard_rows(dt, d):
    """16 lanes per row, 4 rows per wave, 16 rows per block: one row, a partial wave, a whole wave, one row into the next
    wave, a block less one row, a whole block, one row into the second block.  Forward, the plain backward and the
    deterministic one through the C entry points, every output with GUARD sentinel rows behind it."""
    par, fam = (W.LN64_F32, "ln64_f32") if dt == torch.float32 else (W.LN64_BF16, "ln64_bf16")
    code = HF.dtype_code(torch.empty(0, dtype=dt))
    need = hw._lib.lib().hwgat_ln_bwd_det_bytes(d)
    for n in (1, 3, 4, 5, 15, 16, 17):
        g = torch.Generator().manual_seed(1000 * d + n)
        x = (torch.randn(n, d, generator=g) * 2 + 0.5).to(dt)
        gm, bt = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
        dy = torch.randn(n, d, generator=g).to(dt)
        dres = torch.randn(n, d, generator=g).to(dt)
        xr = x.double().requires_grad_(True)
        gr, br = gm.double().requires_grad_(True), bt.double().requires_grad_(True)
        yr = torch.nn.functional.layer_norm(xr, (d,), gr, br, 1e-5)
        yr.backward(dy.double())
        want_dx = xr.grad + dres.double()
        xg, gg, bg, dyg, dresg = x.to(DEV), gm.to(DEV), bt.to(DEV), dy.to(DEV), dres.to(DEV)
        ybuf, y = _guarded(n, d, dt)
        mbuf, mean = _guarded(n, None, torch.float32)
        rbuf, rstd = _guarded(n, None, torch.float32)
        HF.call("hwgat_ln_fwd", HF.ptr(xg), HF.ptr(gg), HF.ptr(bg), HF.ptr(y), HF.ptr(mean), HF.ptr(rstd), n, d, code, HF.stream())
        assert _guard_untouched(ybuf, n) and _guard_untouched(mbuf, n) and _guard_untouched(rbuf, n), ("fwd", n)
        tensor_parity(y, yr, tol_norm=W._tol(dt), **par, what=f"{fam}: y d {d} n {n}")
        assert rel_err(mean.cpu(), xr.detach().mean(1)) < W.F32_TOL + (1e-3 if dt != torch.float32 else 0), n
        assert rel_err(rstd.cpu(), (xr.detach().var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-4, n
        for det in (False, True):
            runs = []
            for _ in range(2 if det else 1):
                dxbuf, dx = _guarded(n, d, dt)
                dgbuf, dg = _guarded(d, None, torch.float32, fill=0.0)
                dbbuf, db = _guarded(d, None, torch.float32, fill=0.0)
                if det:
                    ws = torch.empty(need // 4, device=DEV)
                    HF.call("hwgat_ln_bwd_det", HF.ptr(dyg), HF.ptr(xg), HF.ptr(mean), HF.ptr(rstd), HF.ptr(gg), None, HF.ptr(dresg),
                            HF.ptr(dx), HF.ptr(dg), HF.ptr(db), n, d, code, None, 0, 0.0, None, None, HF.ptr(ws), need, HF.stream())
                else:
                    HF.call("hwgat_ln_bwd", HF.ptr(dyg), HF.ptr(xg), HF.ptr(mean), HF.ptr(rstd), HF.ptr(gg), HF.ptr(dresg),
                            HF.ptr(dx), HF.ptr(dg), HF.ptr(db), n, d, code, HF.stream())
                assert _guard_untouched(dxbuf, n) and _guard_untouched(dgbuf, d) and _guard_untouched(dbbuf, d), ("bwd", n, det)
                runs.append((dx, dg.cpu(), db.cpu()))
            dx, dg, db = runs[0]
            if det:
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(dg, runs[1][1]) and torch.equal(db, runs[1][2]), n
            tensor_parity(dx, want_dx, tol_norm=W._tol(dt), **par, what=f"{fam}: dx d {d} n {n} det {det}")
            tensor_parity(dg, gr.grad, tol_norm=1e-4, tol_entry=W.LN64_DG, what=f"ln64_dg: dgamma d {d} {dt} n {n} det {det}")
            tensor_parity(db, br.grad, tol_norm=1e-4, tol_entry=W.LN64_DG, what=f"ln64_dg: dbeta d {d} {dt} n {n} det {det}")


def test_layernorm_grid_stride_past_the_block_caps():
    """d = 960, fp32: the forward launches at most 2048 blocks of 16 rows and the backward at most 1024, so n = cap x 16 + 19
    sends the first 19 rows' waves round the loop a second time.  fp64 on the CPU at the rows where the loop starts,
    wraps and ends, every row against fp64 formed on the device, dgamma / dbeta entry-wise."""
    d, dt = 960, torch.float32
    n_f, n_b = 2048 * 16 + 19, 1024 * 16 + 19
    g = torch.Generator(device=DEV).manual_seed(960)
    x = torch.randn(n_f, d, device=DEV, generator=g) * 2 + 0.5
    gm, bt = 1 + 0.1 * torch.randn(d, device=DEV, generator=g), 0.1 * torch.randn(d, device=DEV, generator=g)
    dy = torch.randn(n_b, d, device=DEV, generator=g)

    def rows_of(n):
        return torch.tensor(sorted({0, 1, 15, 16, n // 2, n - 17, n - 2, n - 1}))

    def ref_fwd(xs, dev):
        return torch.nn.functional.layer_norm(xs.double().to(dev), (d,), gm.double().to(dev), bt.double().to(dev), 1e-5)

    y = torch.full((n_f, d), float("nan"), device=DEV)
    mean, rstd = torch.empty(n_f, device=DEV), torch.empty(n_f, device=DEV)
    HF.call("hwgat_ln_fwd", HF.ptr(x), HF.ptr(gm), HF.ptr(bt), HF.ptr(y), HF.ptr(mean), HF.ptr(rstd), n_f, d, HF.dtype_code(x), HF.stream())
    rows = rows_of(n_f)
    tensor_parity(y[rows.to(DEV)].cpu(), ref_fwd(x[rows.to(DEV)], "cpu"), tol_norm=W.F32_TOL, **W.LN64_F32, what="ln64_f32: grid-stride y, sampled rows")
    tensor_parity(y, ref_fwd(x, DEV), tol_norm=W.F32_TOL, **W.LN64_F32, what="ln64_f32: grid-stride y")
    assert rel_err(mean.cpu(), x.double().mean(1).cpu()) < W.F32_TOL
    assert rel_err(rstd.cpu(), (x.double().var(1, unbiased=False) + 1e-5).rsqrt().cpu()) < 1e-4
    # backward over the first n_b rows
    xb, mb, rb = x[:n_b], mean[:n_b], rstd[:n_b]
    xr = xb.double().requires_grad_(True)
    gr, br = gm.double().requires_grad_(True), bt.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (d,), gr, br, 1e-5).backward(dy.double())        # fp64 on the device: every row
    rows = rows_of(n_b).to(DEV)
    xc = xb[rows].double().cpu().requires_grad_(True)                                   # fp64 on the CPU: the sampled rows
    torch.nn.functional.layer_norm(xc, (d,), gm.double().cpu(), bt.double().cpu(), 1e-5).backward(dy[rows].double().cpu())
    dg_cpu = (dy.double().cpu() * ((xb.double().cpu() - xb.double().cpu().mean(1, keepdim=True))
                                   * (xb.double().cpu().var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt())).sum(0)
    db_cpu = dy.double().cpu().sum(0)
    for det in (False, True):
        dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
        r = HF.ln_backward(dy, xb, mb, rb, gm, None, dg, db, deterministic=det)
        tensor_parity(r.dx[rows].cpu(), xc.grad, tol_norm=W.F32_TOL, **W.LN64_F32, what=f"ln64_f32: grid-stride dx, sampled rows, det {det}")
        tensor_parity(r.dx, xr.grad, tol_norm=W.F32_TOL, **W.LN64_F32, what=f"ln64_f32: grid-stride dx det {det}")
        tensor_parity(dg.cpu(), dg_cpu, tol_norm=1e-4, tol_entry=W.LN64_DG, what=f"ln64_dg: grid-stride dgamma det {det}")
        tensor_parity(db.cpu(), db_cpu, tol_norm=1e-4, tol_entry=W.LN64_DG, what=f"ln64_dg: grid-stride dbeta det {det}")


# ------------------------------------------------------------------ NT linears at the widths' shapes
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", [(320, 320), (960, 320), (320, 1280), (960, 960), (2880, 960)])
def test_nt_n64_at_width_320_and_960_shapes(dt, N, K):
    """proj / qkv / fc2 of widths 320 and 960 on the 128 x 64 tile: three whole row blocks and a 29-row RAGGED tail"""
    W.nt_every_prologue_and_epilogue(dt, N, K, m_ragged=128 * 3 + 29, m_whole=128 * 3)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", [(640, 320), (1280, 320)])
def test_nt_128_wide_tiles_at_k_64_times_odd(dt, N, K):
    """fc1 of width 320 (ff_ratio 2 and 4): N % 128 == 0, so the 128 x 128 tiles of gemm_f32.hip / gemm_bf16.hip with
    K = 5 x 64, held to those kernels' bounds (test_gpu_gemm.py)"""
    W.nt_every_prologue_and_epilogue(dt, N, K, m_ragged=128 * 3 + 29, m_whole=128 * 3, label="nt",
                                     bounds=(G.NT_F32, G.NT_F32_GELU, G.NT_BF16, G.NT_BF16_FOLD))


def _blocks(nb):
    return sorted({0, 1, 7, 8, nb // 2, nb - 3, nb - 2, nb - 1})


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pro,epi", G._LOOP_CASES + G._TRAIN_CASES)
@pytest.mark.parametrize("M,N,K", [(256 * 26, 1280, 320), (256 * 9, 3840, 960)])
def test_nt_256_tiles_at_k_64_times_odd(M, N, K, pro, epi, dt):
    """130 and 135 tiles of 256 x 256: hwgat_linear_nt_*_ex sends these to the 256-wide kernels (N % 256 == 0, K >= 128,
    at least 128 tiles).  K = 320 and 960 are 5 and 15 slabs of 64 in bf16 (10 and 30 of 32 in fp32): the odd slab counts
    start successive tiles of a workgroup in alternating LDS buffers.  K % 128 == 64 is declined by the eight-wave bf16
    kernel, so every pair runs on gemm_nt256_bf16_k."""
    assert N % 256 == 0 and (M // 256) * (N // 256) >= 128 and (K // 64) % 2 == 1
    G._persistent_loop(M, N, K, pro, epi, dt, _blocks)


# ------------------------------------------------------------------ TN weight gradients at the widths' shapes
TN_SHAPES = [(320, 320), (960, 320), (1280, 320), (320, 1280), (960, 960), (2880, 960), (1920, 960), (3840, 960)]
TN_MS = (1024, 1000)


def _tn64_tiles(N, K):
    return (N // 64) * (K // 64)


def test_tn64_shapes_reach_the_one_split_branch():
    """tn64_splits asks for ceil(512 / tiles) splits (fewer for a short M): above 512 tiles one split whatever M is.  Of
    the dW shapes of width 960, qkv (2880 x 960, 675 tiles) and fc1 at ff_ratio 4 (3840 x 960, 900) are above; proj
    (960 x 960, 225) and fc1 at ff_ratio 2 (1920 x 960, 450) are not, and split a long M."""
    lib = hw._lib.lib()
    above = [(N, K) for N, K in TN_SHAPES if _tn64_tiles(N, K) > 512]
    assert above == [(2880, 960), (3840, 960)]
    for N, K in TN_SHAPES:
        one = (N * K + N) * 4                               # the image of one split: dW and db
        for fn in (lib.hwgat_linear_tn_f32_ws_bytes, lib.hwgat_linear_tn_bf16_ws_bytes, lib.hwgat_linear_tn_det_bytes):
            for M in TN_MS + (1 << 20,):
                need = fn(M, N, K)
                assert need >= one and need % one == 0, (M, N, K)
                if (N, K) in above:
                    assert need == one, (M, N, K)
            if (N, K) not in above:
                assert fn(1 << 20, N, K) > one, (N, K)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,K", TN_SHAPES)
def test_tn64_at_width_320_and_960_shapes(dt, N, K):
    if _tn64_tiles(N, K) > 512:
        for M in TN_MS:
            assert hw._lib.lib().hwgat_linear_tn_f32_ws_bytes(M, N, K) == (N * K + N) * 4          # one split
    W.tn64_weight_gradients(dt, N, K, Ms=TN_MS)


def test_tn64_plain_entry_accumulates_at_960_by_320():
    """test_gpu_width.py::test_tn64_plain_entry_accumulates_without_a_workspace at the qkv shape of width 320: 75 tiles, one
    split each, added into a dW / db of ones"""
    M, N, K = 2000, 960, 320
    g = torch.Generator(device=DEV).manual_seed(11)
    A, Bm = torch.randn(M, N, device=DEV, generator=g), torch.randn(M, K, device=DEV, generator=g)
    dw, db = torch.ones(N, K, device=DEV), torch.ones(N, device=DEV)
    HF.call("hwgat_linear_tn_f32", HF.ptr(A), HF.ptr(Bm), HF.ptr(dw), HF.ptr(db), M, N, K, 0, 0.0, None, None, None, None,
            None, HF.stream())
    Ad, Bd = A.double().cpu(), Bm.double().cpu()
    assert rel_err(dw.cpu(), 1 + Ad.T @ Bd) < W.F32_TOL
    assert rel_err(db.cpu(), 1 + Ad.sum(0)) < W.F32_TOL
    linear_parity((dw.cpu(), db.cpu()), (1 + Ad.T @ Bd, 1 + Ad.sum(0)), tol_norm=W.F32_TOL, **W.TN64_F32,
                  what="tn64_f32: plain entry point N 960 K 320")


# ------------------------------------------------------------------ whole models against the fp64 oracle
ORACLE_MODELS = [(448, (7, 14), (1, 1)), (576, (9,), (1,)), (704, (11,), (2,)), (832, (13,), (1,)), (960, (30,), (1,))]
T_, K_, C_, NC_, B_ = 16, 64, 2, 7, 2
# logits / gradients (rel_err per parameter), eval and train: the tolerances of the reference-fixture tests of
# test_gpu_width.py (fp32 1e-4 / 1e-3; bf16 1e-2 eval logits, 2e-2 train logits, 5e-2 gradients)
MODEL_TOL = {torch.float32: dict(eval=1e-4, train=1e-4, grad=1e-3), torch.bfloat16: dict(eval=1e-2, train=2e-2, grad=5e-2)}


def _hp(d0, heads, depths):
    hp = hw.HWGATEParams({"src_len": T_, "num_class": NC_}, C_, None, num_kps=K_)
    hp.num_heads, hp.depths, hp.embed_dim, hp.drop_rate = list(heads), list(depths), d0, 0.0
    return hp


class _Oracle:
    """the fp64 side of one model: parameters, inputs, and `run(thresholds)` -> (logits, {name: gradient})"""

    def __init__(self, d0, heads, depths):
        hp = _hp(d0, heads, depths)
        self.cfg = dict(kp_dim=C_, temporal_dim=T_, num_classes=NC_, embed_dim=d0, depths=tuple(depths), ff_ratio=hp.ff_ratio,
                        use_pe=hp.pe, num_kps=K_, tp=2)
        self.heads, self.depths = heads, depths
        self.params = O.synth_params(100 + d0 // 64, **self.cfg)
        g = torch.Generator().manual_seed(d0)
        self.x = torch.rand(B_, T_, K_, C_, generator=g)
        self.y = torch.randint(0, NC_, (B_,), generator=g)

    def run(self, thr):
        ref_p = {k: v.double().requires_grad_(k not in ("B", "pos_encoder.pe")) for k, v in self.params.items()}
        oracle = O.OracleHWGAT(ref_p, num_kps=K_, temporal_dim=T_, depths=self.depths, num_heads=self.heads)
        ref = oracle.forward(self.x.double(), thresholds=thr)
        O.smoothed_cross_entropy(ref, self.y).backward()
        return ref.detach(), {k: p.grad for k, p in ref_p.items() if p.grad is not None}

    def tie_free_thresholds(self, nominal):
        return oracle_tie_free_thresholds(self.params, self.x, nominal, num_kps=K_, temporal_dim=T_, depths=self.depths,
                                          num_heads=self.heads)


# nominal train-mode thresholds per model, one per block (moved to the nearest gap by oracle_tie_free_thresholds).  Chosen
# on the fp64 oracle alone so that the thresholds move the logits by more than twice the bf16 train tolerance wherever a
# model of this size allows it: 448 / 896 5.1e-2, 576 5.3e-2, 704 4.2e-2, 960 4.9e-2.  The one block of 832 moves them
# by 2.9e-2 at most, whatever the threshold or the weight scale (2.3e-2 ... 3.0e-2 over 0.03 ... 0.5, weight_std 0.08 ...
# 0.16), which is why the test also asserts the distance from the EVAL reference (see there).
NOMINAL_THR = {448: (0.3, 0.1), 576: (0.3,), 704: (0.07, 0.07), 832: (0.04,), 960: (0.1,)}


@functools.lru_cache(maxsize=None)
def _oracle(d0, heads, depths):
    """computed once per model and shared by the fp32 and bf16 cases; nothing in it is written afterwards"""
    o = _Oracle(d0, heads, depths)
    thr, margin = o.tie_free_thresholds(NOMINAL_THR[d0])
    return o, o.run(None), thr, margin, o.run(thr)


def _grad_errors(model, ref_g):
    """{name: rel_err} over every trained parameter, the full gradient.  The key third of a qkv bias has an exactly zero
    gradient (softmax is invariant to it), so a relative error has no scale there: the query and value thirds are
    compared with their reference, and the key third (entry `name [key third]`) is held to the same tolerance on the
    scale of the other two, |got_k| / |ref_qv|."""
    errs = {}
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(ref_g)
    for k, r in ref_g.items():
        a, b = got[k].double().cpu(), r
        if k.endswith("attn.qkv.bias"):
            d = a.numel() // 3
            assert float(b[d:2 * d].abs().max()) < 1e-12 * float(b.abs().max())      # zero in the reference
            errs[k + " [key third]"] = float(a[d:2 * d].norm() / torch.cat([b[:d], b[2 * d:]]).norm())
            a, b = torch.cat([a[:d], a[2 * d:]]), torch.cat([b[:d], b[2 * d:]])
        errs[k] = rel_err(a, b)
    return errs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d0,heads,depths", ORACLE_MODELS)
def test_model_against_fp64_oracle(d0, heads, depths, dtype):
    o, (eval_ref, eval_g), thr, margin, (train_ref, train_g) = _oracle(d0, heads, depths)
    tol = MODEL_TOL[dtype]
    model = hw.Model(*_hp(d0, heads, depths).get_model_params())
    model.load_state_dict(o.params, strict=False)
    model = model.to(DEV).set_activation_dtype(dtype)
    x, y = o.x.to(DEV), o.y.to(DEV)
    tag = f"model d0 {d0} heads {heads} {dtype}"
    # eval mode: logits, then every gradient of the smoothed cross entropy
    model.eval()
    model.zero_grad()
    out = model(x).float()
    O.smoothed_cross_entropy(out, y).backward()
    e_out, e_g = rel_err(out.detach().cpu(), eval_ref), _grad_errors(model, eval_g)
    worst = max(e_g, key=e_g.get)
    print(f"{tag}: eval logits {e_out:.3g}, worst gradient {e_g[worst]:.3g} ({worst})")
    assert e_out < tol["eval"]
    assert e_g[worst] < tol["grad"], worst
    # train mode with the thresholds forced, held to the plain tolerances in both dtypes.  No probability of the oracle is
    # within `margin` (relative) of its block's threshold.  That the thresholds are APPLIED is asserted directly: with
    # dropout off, a model that ignored them would return its eval-mode output, which the assertion above has just held to
    # within tol["eval"] of the eval reference; the train-mode output must be at least half the thresholds' effect away
    # from that reference, and the effect is more than twice tol["eval"], so the two cannot both hold for such a model.
    effect = rel_err(eval_ref, train_ref)
    assert margin > 0 and effect > 2 * tol["eval"], (margin, effect)
    model.train()
    model.threshold_override = list(thr)
    model.zero_grad()
    out = model(x).float()
    O.smoothed_cross_entropy(out, y).backward()
    e_out, e_g = rel_err(out.detach().cpu(), train_ref), _grad_errors(model, train_g)
    away = rel_err(out.detach().cpu(), eval_ref)
    worst = max(e_g, key=e_g.get)
    print(f"{tag}: train logits {e_out:.3g}, from the eval reference {away:.3g} (thresholds' effect {effect:.3g}), worst gradient "
          f"{e_g[worst]:.3g} ({worst}), threshold margin {margin:.3g}")
    assert e_out < tol["train"]
    assert e_g[worst] < tol["grad"], worst
    assert away > effect / 2, (away, effect)
