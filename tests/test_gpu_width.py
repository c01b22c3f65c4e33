"""GPU parity for HWGATE stage widths that are odd multiples of 64 (embed_dim 64 / 192 / 320 / 960): the 128x64-tile NT
linears, the 64x64-tile weight gradients and the LayerNorm kernels through the C-ABI against fp64 torch -- the LayerNorm
family at EVERY accepted width (helpers.ALL_WIDTHS) -- and whole models against tests/golden/width_*.npz
(make_fixtures_width.py) in fp32 and bf16, plus the model modes (deterministic eval / train, GraphedEval,
GraphedTrainStep, attention dropout).  test_gpu_width_all.py runs the same helpers and bounds at the shapes of widths 320
and 960; the observed values below cover its cases too."""
import importlib
import os
import sys

import pytest
import torch

from helpers import ALL_WIDTHS, linear_parity, load_fixture, rel_err, grad_digest_check, tensor_parity
from oracle import hwgat_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_fixtures_window import edge_list  # noqa: E402

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
serve = importlib.import_module("sl-hwgat_amd.serve")
DEV = "cuda:0"
F32_TOL, BF16_TOL = 2e-5, 1e-2
THR = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]
# Entry / row / column bounds of helpers.linear_parity / tensor_parity per kernel family and storage type: 3 x the worst
# error observed on an MI355X against the fp64 reference over this module's cases (in the comments), at or below the caps
# (bf16-stored outputs: entry 1.2e-2, row and column 1e-2; fp32 outputs: 1e-5 each).
# (fp32 at the deepest K of test_gpu_width_all.py, N 320 K 1280: 1.5e-6 / 1.2e-6 / 9.8e-7, under the bounds, which stay;
#  K 960: 1.2e-6 / 7.0e-7 / 6.4e-7)
NT64_F32 = dict(tol_entry=1.8e-6, tol_row=1.6e-6, tol_col=1.3e-6)      # observed 6.0e-7 / 5.5e-7 / 4.4e-7 at K <= 192
# GELU backward and the stored GELU factor (epilogues 3 and 5): erf and exp in fp32 on top of the product -- the fp32 NT
# family holds them to 5e-5 in norm against 2e-5, the caps scale alike (N 320 K 1280: 3.7e-6 / 1.0e-6 / 9.4e-7)
NT64_F32_GELU = dict(tol_entry=4.8e-6, tol_row=1.8e-6, tol_col=1.3e-6)  # observed 1.6e-6 / 6.1e-7 / 4.3e-7 (caps 2.5e-5)
# (bf16 column error: 8.5e-3 at K <= 192, 8.9e-3 at N 960 K 320)
NT64_BF16 = dict(tol_entry=1.2e-2, tol_row=1e-2, tol_col=1e-2)         # observed 4.7e-3 / 5.6e-3 / 8.9e-3: 3 x is above the caps, which hold
# the bf16 folded LayerNorm (prologue 3) cancels mean * s against a product of bf16 operands and rounds W o gamma to bf16
# (the NT family: norm 1.5e-2 against 6e-3, caps 2.5 x); entry at N 960 K 320, column at N 2880 K 960
NT64_BF16_FOLD = dict(tol_entry=2.3e-2, tol_row=1.5e-2, tol_col=2.4e-2)  # observed 8.8e-3 / 4.8e-3 / 8.5e-3 (caps 3e-2 / 2.5e-2)
# weight gradients on 64 x 64 tiles: entry-wise and per tile (db: norm and entry).  From bf16 operands the result is an
# fp32 accumulation of exact bf16 products: norm 1e-4 (2e-3 with the LayerNorm prologue, whose normalised operand is
# formed in fp32 and rounded to bf16), entry caps 5e-5 / 1e-3 = the fp32 cap scaled by the norm ratio to 2e-5.  The worst
# entries are at N 3840 K 960, the worst LayerNorm-prologue tile at N 320 K 320, M 1000.
TN64_F32 = dict(tol_entry=6e-6, tile=(64, 64), tol_tile=2.4e-6)        # observed 2.0e-6 / 8.3e-7
TN64_BF16 = dict(tol_entry=2.4e-6, tile=(64, 64), tol_tile=7.7e-7)     # observed 1.4e-6 / 2.7e-7 (norm 2.5e-7)
TN64_BF16_LN = dict(tol_entry=6.4e-4, tile=(64, 64), tol_tile=9.2e-5)  # observed 3.4e-4 / 8.0e-5 (norm 3.4e-5)
TN_BF16_NORM, TN_BF16_LN_NORM = 1e-4, 2e-3
# LayerNorm at all sixteen widths: y, dx (row check), the masked copy and xn; dgamma / dbeta (norm 1e-4) entry-wise
# (4.7e-7 at n = 1003; 9.5e-7 over the 16403 rows of test_gpu_width_all.py's grid-stride case, atomic order)
LN64_F32 = dict(tol_entry=7.5e-7, tol_row=5.6e-7)                      # observed 2.7e-7 / 1.9e-7
LN64_BF16 = dict(tol_entry=1e-2, tol_row=8.2e-3)                       # observed 3.4e-3 / 2.7e-3
LN64_DG = 1.4e-6                                                       # observed 9.5e-7


def _tol(dt):
    return F32_TOL if dt == torch.float32 else BF16_TOL


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))


def _gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5


# ------------------------------------------------------------------ NT linear, N % 128 == 64
NT_CASES = [(pro, epi) for pro in (0, 1, 2) for epi in range(7)] + [(3, 0), (3, 2), (3, 5)]


def nt_every_prologue_and_epilogue(dt, N, K, m_ragged=300, m_whole=256, bounds=None, label="nt64"):
    """every pair of NT_CASES at one (N, K) through HF.linear_nt against fp64: norm, then entry / row / column with the
    bounds of `bounds` = (fp32, fp32 GELU, bf16, bf16 fold), by default this module's N64 tables"""
    f32_par, f32_gelu, bf16_par, bf16_fold = bounds or (NT64_F32, NT64_F32_GELU, NT64_BF16, NT64_BF16_FOLD)
    g = torch.Generator().manual_seed(N + K)
    for pro, epi in NT_CASES:
        M = m_whole if pro == 3 else m_ragged                         # pro 3 needs whole 128-row tiles; else a ragged tail
        A = torch.randn(M, K, generator=g).double()
        W = (torch.randn(N, K, generator=g) * K ** -0.5).double()
        b = torch.randn(N, generator=g).double()
        res = torch.randn(M, N, generator=g).double()
        aux = torch.randn(M, N, generator=g).double()
        gm, bt = 1 + 0.1 * torch.randn(K, generator=g).double(), 0.1 * torch.randn(K, generator=g).double()
        p_pro, p_epi, s_pro, s_epi = 0.2, 0.25, 11, 12
        Ad, Wd = A.to(dt).double(), W.to(dt).double()                 # the values the kernels see
        resd, auxd = res.to(dt).double(), aux.to(dt).double()
        mean, rstd = Ad.mean(1), (Ad.var(1, unbiased=False) + 1e-5).rsqrt()
        a_in = Ad
        if pro in (1, 3):
            a_in = (Ad - mean[:, None]) * rstd[:, None] * gm + bt
        if pro == 2:
            a_in = Ad * HF.dropout_mask((M, K), s_pro, p_pro, DEV).cpu().double()
        acc = a_in @ Wd.T
        mk = HF.dropout_mask((M, N), s_epi, p_epi, DEV).cpu().double()
        pre = acc + b
        want2 = None
        if epi == 0:
            want = pre
        elif epi == 1:
            want = resd + pre * mk
        elif epi == 2:
            want, want2 = _gelu(pre) * mk, pre
        elif epi == 3:
            want = acc * mk * _gelu_grad(auxd)
        elif epi == 4:
            want = acc
        elif epi == 5:
            want, want2 = _gelu(pre) * mk, _gelu_grad(pre) * mk
        else:
            want = acc * auxd
        kw = dict(epi=epi, res=res.to(dt).to(DEV) if epi == 1 else None, aux=aux.to(dt).to(DEV) if epi in (3, 6) else None,
                  epi_seed=s_epi, epi_p=p_epi if epi in (1, 2, 3, 5) else 0.0)
        Ag = A.to(dt).to(DEV)
        canary = torch.full((M + 160, N), 777.0, device=DEV, dtype=dt)      # rows behind the output: nothing may be written there
        canary[:M] = float("nan")                                           # poisoned: every element must be stored
        poison = canary[:M]
        gf, bf = gm.float().to(DEV), bt.float().to(DEV)
        m32, r32 = mean.float().to(DEV), rstd.float().to(DEV)
        if pro == 3:
            Wf, s, c = HF.ln_fold(W.float().to(DEV), b.float().to(DEV), gf, bf, dt)
            out = HF.linear_nt(Ag, Wf, None, pro=3, ln=(m32, r32, s, c), out=poison, **kw)
        else:
            out = HF.linear_nt(Ag, W.to(dt).to(DEV), b.float().to(DEV), pro=pro, ln=(m32, r32, gf, bf) if pro == 1 else None,
                               pro_seed=s_pro, pro_p=p_pro if pro == 2 else 0.0, out=poison, **kw)
        got, got2 = (out if isinstance(out, tuple) else (out, None))
        assert rel_err(got.float().cpu(), want) < _tol(dt), (pro, epi)
        if want2 is not None:
            assert rel_err(got2.float().cpu(), want2) < _tol(dt), (pro, epi, "C2")
        assert bool((canary[M:] == 777.0).all()), (pro, epi)
        if dt == torch.float32:
            par, fam = (f32_gelu, label + "_f32_gelu") if epi in (3, 5) else (f32_par, label + "_f32")
        else:
            par, fam = (bf16_fold, label + "_bf16_fold") if pro == 3 else (bf16_par, label + "_bf16")
        if dt != torch.float32 and pro in (1, 2):           # the prologue's output is rounded to bf16 before the MFMA
            acc = a_in.float().bfloat16().double() @ Wd.T
            pre = acc + b
            want, want2 = {0: (pre, None), 1: (resd + pre * mk, None), 2: (_gelu(pre) * mk, pre), 3: (acc * mk * _gelu_grad(auxd), None),
                           4: (acc, None), 5: (_gelu(pre) * mk, _gelu_grad(pre) * mk), 6: (acc * auxd, None)}[epi]
        linear_parity(got if got2 is None else (got, got2), want if want2 is None else (want, want2), tol_norm=_tol(dt), **par,
                      what=f"{fam}: N {N} K {K} pro {pro} epi {epi}")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,K", [(64, 64), (192, 64), (576, 192), (64, 192)])
def test_nt_n64_every_prologue_and_epilogue(dt, N, K):
    nt_every_prologue_and_epilogue(dt, N, K)


def test_nt_n64_refuses_the_statistics_epilogue():
    A = torch.randn(256, 64, device=DEV)
    with pytest.raises(RuntimeError):
        HF.linear_nt(A, torch.randn(64, 64, device=DEV), None, epi=HF.EPI_BIAS_DROP_RES, res=A, stats=True)


# ------------------------------------------------------------------ TN weight gradients, 64x64 tiles
def tn64_weight_gradients(dt, N, K, Ms=(4096, 1000)):
    """dW / db of the 64 x 64 tile kernel at one (N, K): plain / dropout / LayerNorm prologues, deterministic and not, each
    launched twice (bit-equal), against fp64 in norm, entry-wise and per tile"""
    lib = hw._lib.lib()
    g = torch.Generator().manual_seed(3 * N + K)
    for M in Ms:
        assert lib.hwgat_linear_tn_det_bytes(M, N, K) > 0
        assert lib.hwgat_linear_tn_f32_ws_bytes(M, N, K) > 0 and lib.hwgat_linear_tn_bf16_ws_bytes(M, N, K) > 0
        A = torch.randn(M, N, generator=g).to(dt)
        Bm = torch.randn(M, K, generator=g).to(dt)
        gm, bt = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        Bd = Bm.double()
        mean, rstd = Bd.mean(1), (Bd.var(1, unbiased=False) + 1e-5).rsqrt()
        for kind in ("plain", "drop", "ln"):
            a = A.double()
            b = Bd
            kw = {}
            if kind == "drop":
                a = a * HF.dropout_mask((M, N), 7, 0.2, DEV).cpu().double()
                kw = dict(pro_seed=7, pro_p=0.2)
            if kind == "ln":
                b = (Bd - mean[:, None]) * rstd[:, None] * gm.double() + bt.double()
                kw = dict(ln=(mean.float().to(DEV), rstd.float().to(DEV), gm.to(DEV), bt.to(DEV)))
            want_w, want_b = a.T @ b, a.sum(0)
            tol_w = tol_b = F32_TOL
            par, fam = TN64_F32, "tn64_f32"
            if dt != torch.float32:
                # fp32 accumulation of exact bf16 products: the reference rounds the masked / normalised operand to bf16 as
                # the kernel does (db sums the masked values before that rounding, as test_bf16_tn_weight_and_bias_grad has it)
                want_w = a.float().bfloat16().double().T @ b.float().bfloat16().double()
                tol_w, tol_b = (TN_BF16_LN_NORM if kind == "ln" else TN_BF16_NORM), TN_BF16_NORM
                par, fam = (TN64_BF16_LN, "tn64_bf16_ln") if kind == "ln" else (TN64_BF16, "tn64_bf16")
            for det in (False, True):
                if det and M % 32:
                    continue
                outs = []
                for _ in range(2):
                    dw, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
                    HF.linear_tn(A.to(DEV), Bm.to(DEV), dw, db, deterministic=det, **kw)
                    outs.append((dw.cpu(), db.cpu()))
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (M, kind, det)
                assert rel_err(outs[0][0], want_w) < tol_w, (M, kind, det)
                assert rel_err(outs[0][1], want_b) < tol_b, (M, kind, det)
                linear_parity(outs[0], (want_w, want_b), tol_norm=(tol_w, tol_b), **par, what=f"{fam}: N {N} K {K} M {M} {kind} det {det}")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,K", [(192, 64), (64, 64), (128, 64), (64, 128), (576, 192), (192, 192)])
def test_tn64_weight_gradients(dt, N, K):
    tn64_weight_gradients(dt, N, K)


def test_tn64_plain_entry_accumulates_without_a_workspace():
    M, N, K = 2000, 192, 64
    A, Bm = torch.randn(M, N, device=DEV), torch.randn(M, K, device=DEV)
    dw, db = torch.ones(N, K, device=DEV), torch.ones(N, device=DEV)
    HF.call("hwgat_linear_tn_f32", HF.ptr(A), HF.ptr(Bm), HF.ptr(dw), HF.ptr(db), M, N, K, 0, 0.0, None, None, None, None,
            None, HF.stream())
    assert rel_err(dw.cpu(), 1 + (A.T @ Bm).cpu().double()) < F32_TOL
    assert rel_err(db.cpu(), 1 + A.sum(0).cpu().double()) < F32_TOL
    linear_parity((dw, db), (1 + A.double().T @ Bm.double(), 1 + A.double().sum(0)), tol_norm=F32_TOL, **TN64_F32,
                  what="tn64_f32: plain entry point")


# ------------------------------------------------------------------ LayerNorm family at the new widths
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", ALL_WIDTHS)
def test_layernorm_new_widths(dt, d):
    g = torch.Generator().manual_seed(d)
    n = 1003
    x = (torch.randn(n, d, generator=g) * 2 + 0.5).to(dt)
    gm, bt = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(n, d, generator=g).to(dt)
    dres = torch.randn(n, d, generator=g).to(dt)
    xr = x.double().requires_grad_(True)
    gr, br = gm.double().requires_grad_(True), bt.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (d,), gr, br, 1e-5)
    yr.backward(dy.double())
    xg, gg, bg = x.to(DEV), gm.to(DEV), bt.to(DEV)
    # forward with y, and statistics only
    y = HF.layer_norm(xg.clone().requires_grad_(True), gg, bg)
    assert rel_err(y.detach().float().cpu(), yr.detach()) < _tol(dt)
    par, fam = (LN64_F32, "ln64_f32") if dt == torch.float32 else (LN64_BF16, "ln64_bf16")
    tensor_parity(y, yr, tol_norm=_tol(dt), **par, what=f"{fam}: y d {d}")
    mean, rstd = HF.ln_stats(xg, gg, bg)
    assert rel_err(mean.cpu(), xr.detach().mean(1)) < F32_TOL + (1e-3 if dt != torch.float32 else 0)
    assert rel_err(rstd.cpu(), (xr.detach().var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-4
    want_dx = xr.grad + dres.double()
    xn_want = yr.detach()
    mk = HF.dropout_mask((n, d), 5, 0.3, DEV).cpu().double()
    for det in (False, True):
        for variant in ("plain", "masked", "xn", "xn_masked"):
            outs = []
            for _ in range(2 if det else 1):
                dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
                kw = dict(deterministic=det)
                if "masked" in variant:
                    kw.update(mask=(5, 0.3))
                if "xn" in variant:
                    kw.update(beta=bg)
                r = HF.ln_backward(dy.to(DEV), xg, mean, rstd, gg, dres.to(DEV), dg, db, **kw)
                outs.append((r, dg.cpu(), db.cpu()))
            r, dg, db = outs[0]
            if det:
                assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2]), variant
            assert (r.dx_masked is not None, r.xn is not None) == ("masked" in variant, "xn" in variant), (variant, det)
            assert rel_err(r.dx.float().cpu(), want_dx) < _tol(dt), (variant, det)
            tensor_parity(r.dx, want_dx, tol_norm=_tol(dt), **par, what=f"{fam}: dx d {d} {variant} det {det}")
            if "masked" in variant:
                assert rel_err(r.dx_masked.float().cpu(), want_dx * mk) < _tol(dt), (variant, det)
                tensor_parity(r.dx_masked, want_dx * mk, tol_norm=_tol(dt), **par, what=f"{fam}: dxm d {d} {variant} det {det}")
            if "xn" in variant:
                assert rel_err(r.xn.float().cpu(), xn_want) < _tol(dt), (variant, det)
                tensor_parity(r.xn, xn_want, tol_norm=_tol(dt), **par, what=f"{fam}: xn d {d} {variant} det {det}")
            assert rel_err(dg, gr.grad) < 1e-4 and rel_err(db, br.grad) < 1e-4, (variant, det)
            tensor_parity(dg, gr.grad, tol_norm=1e-4, tol_entry=LN64_DG, what=f"ln64_dg: dgamma d {d} {dt} {variant} det {det}")
            tensor_parity(db, br.grad, tol_norm=1e-4, tol_entry=LN64_DG, what=f"ln64_dg: dbeta d {d} {dt} {variant} det {det}")
    # no residual
    dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    dx, dxm, xn = HF.ln_backward(dy.to(DEV), xg, mean, rstd, gg, None, dg, db)
    assert dxm is None and xn is None
    assert rel_err(dx.float().cpu(), xr.grad) < _tol(dt)
    tensor_parity(dx, xr.grad, tol_norm=_tol(dt), **par, what=f"{fam}: dx d {d} no residual")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d", ALL_WIDTHS)
def test_ln_mean_pool_new_widths(dt, d):
    g = torch.Generator().manual_seed(d + 1)
    B, n_tok = 3, 200
    x = torch.randn(B, n_tok, d, generator=g).to(dt)
    gm, bt = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    df = torch.randn(B, d, generator=g)
    xr = x.double().requires_grad_(True)
    fr = torch.nn.functional.layer_norm(xr, (d,), gm.double(), bt.double(), 1e-5).mean(1)
    fr.backward(df.double())
    for det in (False, True):
        xg = x.to(DEV).requires_grad_(True)
        f = HF.ln_mean_pool(xg, gm.to(DEV), bt.to(DEV), deterministic=det)
        f.backward(df.to(DEV))
        assert rel_err(f.detach().cpu(), fr.detach()) < _tol(dt)
        assert rel_err(xg.grad.float().cpu(), xr.grad) < _tol(dt)
        par, fam = (LN64_F32, "ln64_f32") if dt == torch.float32 else (LN64_BF16, "ln64_bf16")
        # the pooled output is fp32 whatever x is stored in, and the reference reads the same stored x
        tensor_parity(f, fr, tol_norm=_tol(dt), **LN64_F32, what=f"ln64_f32: pool out d {d} {dt} det {det}")
        tensor_parity(xg.grad, xr.grad, tol_norm=_tol(dt), **par, what=f"{fam}: pool dx d {d} det {det}")
        if det:
            f2 = HF.ln_mean_pool(x.to(DEV), gm.to(DEV), bt.to(DEV), deterministic=True)
            assert torch.equal(f.detach(), f2)


# ------------------------------------------------------------------ whole models vs the reference's fixtures
FIXTURES = ["width_d64.npz", "width_d64_w8.npz", "width_d192.npz", "width_d320.npz", "width_d960.npz"]


def _model_from_fixture(fx, dtype=torch.float32):
    T, K, C, d0, nc, B, seed, W = [int(v) for v in fx["cfg"]]
    hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, C, None, num_kps=K)
    hp.window_size, hp.num_heads, hp.drop_rate, hp.embed_dim = W, [int(h) for h in fx["heads"]], 0.0, d0
    if "depths" in fx:                                                # absent: the reference's default (2, 2, 4)
        hp.depths = [int(v) for v in fx["depths"]]
    hp.edges = [edge_list(W, w) for w in range(K // W)]
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    model = hw.Model(*hp.get_model_params())
    cfg = dict(kp_dim=C, temporal_dim=T, num_classes=nc, embed_dim=d0, depths=tuple(hp.depths), ff_ratio=hp.ff_ratio,
               use_pe=hp.pe, num_kps=K, tp=2)
    model.load_state_dict(O.synth_params(seed, weight_std=0.08, **cfg), strict=False)
    return model.to(DEV).set_activation_dtype(dtype)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_matches_reference_fixture(name):
    fx = load_fixture(name)
    model = _model_from_fixture(fx)
    x = torch.from_numpy(fx["x"]).to(DEV)
    y = torch.from_numpy(fx["y"]).to(DEV)
    crit = train.SmoothedCrossEntropyLoss()
    model.eval()
    with torch.no_grad():
        assert rel_err(model(x).cpu(), fx["eval.logits"]) < 1e-4
    model.zero_grad()
    loss = crit(model(x), y)
    loss.backward()
    assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-4
    grad_digest_check({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, fx, "evalbwd.", 1e-3)
    model.train()
    model.threshold_override = [float(t) for t in fx["train.thr"]]
    model.zero_grad()
    out = model(x)
    loss = crit(out, y)
    loss.backward()
    assert rel_err(out.detach().cpu(), fx["train.logits"]) < 1e-4
    assert abs(loss.item() - float(fx["train.loss"])) < 1e-4
    grad_digest_check({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, fx, "train.", 1e-3)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_bf16_matches_reference_fixture(name):
    fx = load_fixture(name)
    model = _model_from_fixture(fx, torch.bfloat16)
    x = torch.from_numpy(fx["x"]).to(DEV)
    y = torch.from_numpy(fx["y"]).to(DEV)
    crit = train.SmoothedCrossEntropyLoss()
    model.eval()
    with torch.no_grad():
        assert rel_err(model(x).float().cpu(), fx["eval.logits"]) < 1e-2
    model.zero_grad()
    loss = crit(model(x).float(), y)
    loss.backward()
    assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-2 * max(1.0, abs(float(fx["evalbwd.loss"])))
    grad_digest_check({k: p.grad for k, p in model.named_parameters() if p.grad is not None}, fx, "evalbwd.", 5e-2)
    model.train()
    model.threshold_override = [float(t) for t in fx["train.thr"]]
    model.zero_grad()
    out = model(x).float()
    loss = crit(out, y)
    loss.backward()
    assert rel_err(out.detach().cpu(), fx["train.logits"]) < 2e-2
    assert abs(loss.item() - float(fx["train.loss"])) < 2e-2 * max(1.0, abs(float(fx["train.loss"])))


# ------------------------------------------------------------------ model modes
def _small(d0, W=16, dtype=torch.float32, attn_drop=0.0):
    torch.manual_seed(13)
    K = 64
    heads = {64: (2, 4, 8), 192: (3, 6, 12), 320: (5, 10), 960: (15,)}[d0]
    hp = hw.HWGATEParams({"src_len": 32, "num_class": 7}, 2, DEV, num_kps=K)
    hp.window_size, hp.num_heads, hp.embed_dim = W, list(heads), d0
    hp.depths = [2, 2, 4][:len(heads)]                                # 320 / 640 and 960 end at 1024: two stages, one stage
    hp.edges = [edge_list(W, w) for w in range(K // W)]
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    hp.attn_drop_rate = attn_drop
    model = hw.Model(*hp.get_model_params()).to(DEV)
    model.set_activation_dtype(dtype)
    return model


MODES = [(64, 16), (64, 8), (192, 16), (320, 16), (960, 16)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d0,W", MODES)
def test_deterministic_eval_repeats(d0, W, dtype):
    model = _small(d0, W, dtype).eval()
    x = torch.rand(6, 32, 64, 2, device=DEV)
    with torch.no_grad():
        a = model(x)
        junk = torch.randn(1 << 20, device=DEV).sum()
        b = model(x)
    assert junk.isfinite() and torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d0,W", MODES)
def test_deterministic_train_repeats_every_weight(d0, W, dtype):
    model = _small(d0, W, dtype, attn_drop=0.1).train()
    model.deterministic_train = True
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.rand(8, 32, 64, 2, device=DEV, generator=g)
    y = torch.randint(0, 7, (8,), device=DEV, generator=g)
    w0 = {k: v.clone() for k, v in model.state_dict().items()}
    runs = []
    for _ in range(2):
        model.load_state_dict(w0)
        model._drop_calls = 5
        torch.manual_seed(99)
        opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4, fused=True)
        step = train.TrainStep(model, opt, None)
        losses = [step(x, y).clone() for _ in range(3)]
        runs.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
    (l1, w1), (l2, w2) = runs
    assert all(torch.isfinite(v) for v in l1)
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    for n in w1:
        assert torch.equal(w1[n], w2[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d0,W", MODES)
def test_graphed_eval_is_bit_equal_to_eager(d0, W, dtype):
    model = _small(d0, W, dtype).eval()
    x = torch.rand(4, 32, 64, 2, device=DEV)
    fast = serve.GraphedEval(model, x)
    with torch.no_grad():
        want = model(x)
    assert torch.equal(fast(x), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d0,W", MODES)
def test_graphed_train_step_matches_eager_deterministic(d0, W, dtype):
    steps, c0 = 3, 17
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(8, 32, 64, 2, device=DEV, generator=g)
    y = torch.randint(0, 7, (8,), device=DEV, generator=g)
    res = []
    for graphed in (False, True):
        m = _small(d0, W, dtype).train()
        m.deterministic_train = True
        m.threshold_override = THR
        o = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
        m._drop_calls = c0
        s = train.GraphedTrainStep(m, o, x, y) if graphed else train.TrainStep(m, o, None)
        losses = [s(x, y).clone() for _ in range(steps)]
        res.append((losses, [p.detach().clone() for p in m.parameters()]))
    (l1, w1), (l2, w2) = res
    for a, b in zip(l1, l2):
        assert torch.equal(a, b), (float(a), float(b))
    for a, b in zip(w1, w2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("d0,W", MODES)
def test_attention_dropout_trains_and_eval_ignores_it(d0, W):
    x = torch.rand(4, 32, 64, 2, device=DEV)
    y = torch.randint(0, 7, (4,), device=DEV)
    plain = _small(d0, W).eval()
    dropped = _small(d0, W, attn_drop=0.1).eval()
    with torch.no_grad():
        assert torch.equal(plain(x), dropped(x))                  # eval: no attention dropout
    dropped.train()
    dropped.threshold_override = THR
    plain.train()
    plain.threshold_override = THR
    plain.drop_rate = dropped.drop_rate = 0.0
    la = train.SmoothedCrossEntropyLoss()(dropped(x), y)
    lb = train.SmoothedCrossEntropyLoss()(plain(x), y)
    la.backward()
    assert torch.isfinite(la) and float(la.detach()) != float(lb.detach())
    assert all(torch.isfinite(p.grad).all() for p in dropped.parameters() if p.grad is not None)
