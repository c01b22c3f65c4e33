"""CPU: host logic of the backend -- C-ABI exports, drop-in boundary, mask rows."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import hwgat_oracle as O
from helpers import load_fixture, reference_standin

hw = importlib.import_module("sl-hwgat_amd")


def test_library_loads_and_exports_every_declared_symbol():
    names = hw._lib.declared_symbols()
    assert len(names) >= 10
    handle = hw._lib.lib()
    for n in names:
        assert getattr(handle, n) is not None, n
    assert set(names) == set(hw._lib._SIGS), set(names) ^ set(hw._lib._SIGS)
    assert handle.hwgat_abi_version() == hw._lib.header_abi_version() >= 3000


def test_state_dict_contract_matches_reference_keys():
    fx = load_fixture("cfg1.npz")
    hp = hw.HWGATEParams({"src_len": 32, "num_class": 10}, 2, torch.device("cpu"), num_kps=32)
    assert np.array_equal(hp.adj_mat.numpy(), fx["adj"])          # reference get_adj_mat()
    model = hw.Model(*hp.get_model_params())
    sd = model.state_dict()
    want = dict(O.param_shapes(kp_dim=2, temporal_dim=32, num_classes=10, num_kps=32))
    for k, shape in want.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    extra = set(sd) - set(want)
    assert extra == {k[5:] for k in fx if k.startswith("mask.")}  # attn_mask of odd blocks only
    for k in extra:
        assert np.array_equal(sd[k].numpy(), fx["mask." + k]), k
    assert not model.B.requires_grad and torch.equal(sd["pos_encoder.pe"], O.sinusoid_table(32, 128))
    # reference-shaped checkpoints load
    model.load_state_dict(O.synth_params(11, kp_dim=2, temporal_dim=32, num_classes=10, num_kps=32), strict=False)
    # default tuple of the reference (K=64) also builds
    hp64 = hw.HWGATEParams({"src_len": 64, "num_class": 262}, 2, None)
    assert hp64.adj_mat.shape == (4, 32, 32) and len(hp64.get_model_params()) == 16


def test_forward_without_gpu_fails_loudly():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, None, num_kps=32)
    model = hw.Model(*hp.get_model_params())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.rand(1, 16, 32, 2))


def test_mask_rows_equal_reference_masks():
    for nW in (2, 5):
        adj = O.window_adjacency(nW)
        bits = hw.functional.mask_bits(adj).numpy().astype(np.int64) & 0xFFFFFFFF
        key = np.arange(32)
        plain = (bits[0][:, :, None] >> key) & 1
        last = (bits[1][:, :, None] >> key) & 1
        assert np.array_equal(plain, adj.numpy().astype(np.int64))
        sm = O.shift_mask(8, nW).view(4, nW, 32, 32)
        assert np.array_equal(last, (adj * sm[-1]).numpy().astype(np.int64))
        assert np.array_equal(plain, (adj * sm[0]).numpy().astype(np.int64))
    with pytest.raises(ValueError):
        hw.functional.mask_bits(torch.full((1, 32, 32), 0.5))


def test_part_tables():
    fx = load_fixture("window_create.npz")
    idx = hw.part_table(29).numpy()
    assert np.array_equal(fx["raw"][:, idx].astype(np.float32), fx["out"])   # == WindowCreate
    for J, nW in ((27, 2), (67, 5), (133, 7)):
        t = hw.part_table(J).numpy()
        assert t.shape == (nW * 16,) and t.min() >= 0 and t.max() < J
        assert all((t[w * 16:w * 16 + 3] == [0, 1, 2]).all() for w in range(nW))


def test_c_abi_rejects_bad_arguments_without_launching():
    """argument validation happens before any HIP call, so it is testable without a GPU"""
    L = hw._lib.lib()
    import ctypes
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.hwgat_win_attn_fwd(None, p, p, None, 1, 4, 1, 2, 64, 0, 0, None) == -1          # HWGAT_EINVAL
    assert L.hwgat_win_attn_fwd(p, p, p, None, 1, 3, 1, 2, 64, 0, 0, None) == -2             # odd F: HWGAT_ESHAPE
    assert L.hwgat_win_attn_fwd(p, p, p, None, 1, 4, 1, 2, 48, 0, 0, None) == -2             # head_dim 48
    assert L.hwgat_win_attn_bwd(p, p, p, p, None, 1, 4, 1, 2, 64, 0, 7, None) == -3          # HWGAT_EDTYPE
    assert L.hwgat_ln_fwd(p, p, p, p, p, p, 8, 100, 0, None) == -2                           # width 100
    assert L.hwgat_linear_nt_f32(p, p, None, p, 128, 100, 128, 0, None, None, None, None, 0, 0.0, 0,
                                 None, None, None, 0, 0.0, None, None) == -2                        # N % 128 (any M is fine)
    assert L.hwgat_linear_nt_f32(p, p, None, p, 0, 128, 128, 0, None, None, None, None, 0, 0.0, 0,
                                 None, None, None, 0, 0.0, None, None) == -1                        # M <= 0
    assert L.hwgat_linear_nt_f32(p, p, None, p, 128, 128, 128, 1, None, None, None, None, 0, 0.0, 0,
                                 None, None, None, 0, 0.0, None, None) == -1                        # LN prologue w/o stats
    assert L.hwgat_linear_nt_f32(p, p, None, p, 128, 128, 128, 0, None, None, None, None, 0, 0.0, 1,
                                 None, None, None, 0, 1.5, None, None) == -1                        # residual missing / p >= 1
    assert L.hwgat_linear_tn_f32(p, p, p, None, 64, 128, 100, 0, 0.0, None, None, None, None, None, None) == -2
    assert L.hwgat_embed_fwd(p, None, p, None, p, 1, 4, 29, 64, 2, 128, 0, 0, 0.0, None, None) == -2   # J != K without a table
    assert L.hwgat_merge(p, p, 1, 3, 16, 128, 0, 0, None) == -2
    # the LayerNorm family, (width, dtype) left open: a width no kernel takes is HWGAT_ESHAPE, an unknown dtype is
    # HWGAT_EDTYPE whatever the width -- the dtype is looked at first
    ln = {
        "hwgat_ln_fwd": lambda d, t: (p, p, p, p, p, p, 8, d, t, None),
        "hwgat_ln_bwd": lambda d, t: (p,) * 9 + (8, d, t, None),
        "hwgat_ln_bwd_masked": lambda d, t: (p,) * 9 + (8, d, t, p, 1, 0.5, None, None),
        "hwgat_ln_bwd_xn": lambda d, t: (p,) * 10 + (8, d, t, p, 1, 0.5, p, None, None),
        "hwgat_ln_bwd_det": lambda d, t: (p,) * 10 + (8, d, t, p, 1, 0.5, p, None, p, 1 << 30, None),
        "hwgat_lnpool_fwd": lambda d, t: (p, p, p, p, 1, 4, d, t, None),
        "hwgat_lnpool_fwd_det": lambda d, t: (p, p, p, p, 1, 4, d, t, p, None),
        "hwgat_lnpool_bwd": lambda d, t: (p,) * 5 + (1, 4, d, t, None),
        "hwgat_lnpool_bwd_masked": lambda d, t: (p,) * 5 + (1, 4, d, t, p, 1, 0.5, None, None),
    }
    for name, args in ln.items():
        for d in (100, 1088, 0):
            assert getattr(L, name)(*args(d, 0)) == -2, (name, d)
        for d in (100, 128, 192):
            assert getattr(L, name)(*args(d, 9)) == -3, (name, d)
    for t in (0, 9):        # a short workspace of the deterministic form: HWGAT_ESHAPE before anything about the dtype
        assert L.hwgat_ln_bwd_det(*(p,) * 10, 8, 128, t, p, 1, 0.5, p, None, p, 16, None) == -2


EINVAL, ESHAPE = -1, -2
_DUMMY = (ctypes.c_float * 64)()
_P = ctypes.cast(_DUMMY, ctypes.c_void_p)
# prologues / epilogues of csrc/fused_ops.h
PRO_NONE, PRO_LN, PRO_DROP, PRO_LN_FOLD = 0, 1, 2, 3
(EPI_BIAS, EPI_BIAS_DROP_RES, EPI_BIAS_GELU_DROP, EPI_GELU_BWD, EPI_NONE, EPI_BIAS_GELU_DROP_G, EPI_MUL_AUX,
 EPI_BIAS_RELU_DROP, EPI_RELU_BWD) = range(9)
_LN = dict(mean=_P, rstd=_P, gamma=_P, beta=_P)
_STAT = dict(M=256, epi=EPI_BIAS_DROP_RES, res=_P, stat_sum=_P, stat_sq=_P)        # a valid statistics call, then one fault
_NT_ORDER = ("A", "W", "bias", "C", "M", "N", "K", "pro", "mean", "rstd", "gamma", "beta", "pro_seed", "pro_p", "epi", "res",
             "C2", "aux", "epi_seed", "epi_p", "stat_sum", "stat_sq", "merge_F", "merge_K", "seed_base", "stream")
_NT_DEFAULT = dict(A=_P, W=_P, C=_P, M=128, N=128, K=128, pro=PRO_NONE, pro_seed=0, pro_p=0.0, epi=EPI_BIAS, epi_seed=0,
                   epi_p=0.0, merge_F=0, merge_K=0)
_TN_ORDER = ("A", "B", "dW", "db", "M", "N", "K", "pro_seed", "pro_p", "mean", "rstd", "gamma", "beta", "seed_base")
_TN_DEFAULT = dict(A=_P, B=_P, dW=_P, M=64, N=128, K=128, pro_seed=0, pro_p=0.0)
_ONE_IMAGE = (128 * 128 + 128) * 4                                                   # bytes of one dW + db image at N = K = 128

# (over-rides of a valid call, status) -- every case fails a check that runs before the first launch
_NT_CASES = {
    "A_null": (dict(A=None), EINVAL), "W_null": (dict(W=None), EINVAL), "C_null": (dict(C=None), EINVAL),
    "M_zero": (dict(M=0), EINVAL), "N_zero": (dict(N=0), EINVAL), "K_negative": (dict(K=-128), EINVAL),
    "N_not_64": (dict(N=100), ESHAPE),
    "ln_without_stats": (dict(pro=PRO_LN, gamma=_P, beta=_P), EINVAL),
    "ln_fold_without_stats": (dict(pro=PRO_LN_FOLD, mean=_P, rstd=_P), EINVAL),
    "ln_fold_other_epilogue": (dict(pro=PRO_LN_FOLD, epi=EPI_BIAS_DROP_RES, res=_P, **_LN), EINVAL),
    "ln_fold_ragged_M": (dict(pro=PRO_LN_FOLD, M=192, **_LN), ESHAPE),
    "drop_res_without_res": (dict(epi=EPI_BIAS_DROP_RES), EINVAL),
    "gelu_drop_without_C2": (dict(epi=EPI_BIAS_GELU_DROP), EINVAL),
    "gelu_drop_g_without_C2": (dict(epi=EPI_BIAS_GELU_DROP_G), EINVAL),
    "gelu_bwd_without_aux": (dict(epi=EPI_GELU_BWD), EINVAL),
    "mul_aux_without_aux": (dict(epi=EPI_MUL_AUX), EINVAL),
    "relu_bwd_without_aux": (dict(epi=EPI_RELU_BWD), EINVAL),
    "pro_p_negative": (dict(pro=PRO_DROP, pro_p=-0.1), EINVAL), "pro_p_one": (dict(pro=PRO_DROP, pro_p=1.0), EINVAL),
    "epi_p_negative": (dict(epi_p=-0.5), EINVAL), "epi_p_one": (dict(epi_p=1.0), EINVAL),
    "relu_with_ln": (dict(epi=EPI_BIAS_RELU_DROP, pro=PRO_LN, **_LN), EINVAL),
    "relu_bwd_with_dropout_prologue": (dict(epi=EPI_RELU_BWD, aux=_P, pro=PRO_DROP, pro_p=0.5), EINVAL),
    "stat_sum_only": (dict(_STAT, stat_sq=None), EINVAL), "stat_sq_only": (dict(_STAT, stat_sum=None), EINVAL),
    "merge_without_buffers": (dict(_STAT, stat_sum=None, stat_sq=None, merge_F=2, merge_K=4), EINVAL),
    "stat_with_prologue": (dict(_STAT, pro=PRO_LN, **_LN), EINVAL),
    "stat_other_epilogue": (dict(_STAT, epi=EPI_BIAS), EINVAL),
    "stat_M_not_256": (dict(_STAT, M=128), ESHAPE),
    "stat_N_odd_64": (dict(_STAT, N=192), ESHAPE),
    "merge_F_zero": (dict(_STAT, merge_F=0, merge_K=4), EINVAL), "merge_F_odd": (dict(_STAT, merge_F=3, merge_K=4), EINVAL),
    "merge_M_not_whole_clips": (dict(_STAT, merge_F=2, merge_K=3), EINVAL),
}
_TN_CASES = {
    "A_null": (dict(A=None), EINVAL), "B_null": (dict(B=None), EINVAL), "dW_null": (dict(dW=None), EINVAL),
    "M_zero": (dict(M=0), EINVAL), "N_not_128": (dict(N=100), ESHAPE), "K_not_128": (dict(K=100), ESHAPE),
    "ln_without_rstd": (dict(mean=_P, gamma=_P, beta=_P), EINVAL), "pro_p_one": (dict(pro_p=1.0), EINVAL),
}
_DET_CASES = {
    "ws_null": (dict(ws=None), EINVAL), "ws_below_one_image": (dict(ws_bytes=_ONE_IMAGE - 4), ESHAPE),
    "ragged_M": (dict(M=48), ESHAPE),
}


def _nt_ex(dtype, over):
    a = dict(_NT_DEFAULT, **over)
    return getattr(hw._lib.lib(), "hwgat_linear_nt_%s_ex" % dtype)(*[a.get(k) for k in _NT_ORDER])


def _tn(dtype, det, over):
    a = dict(_TN_DEFAULT, **(dict(ws=_P, ws_bytes=_ONE_IMAGE) if det else {}))
    a.update(over)
    order = _TN_ORDER + (("ws", "ws_bytes", "stream") if det else ("stream",))
    return getattr(hw._lib.lib(), "hwgat_linear_tn_%s%s" % (dtype, "_det" if det else ""))(*[a.get(k) for k in order])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(_NT_CASES))
def test_linear_nt_ex_rejects_before_launching(dtype, case):
    """one case per validation rule of hwgat_linear_nt_{f32,bf16}_ex; the pointers are a 64-float dummy, so every case
    is one that returns before a launch (the file also runs on GPU machines)"""
    over, status = _NT_CASES[case]
    assert _nt_ex(dtype, over) == status


def test_linear_nt_ex_k_granule():
    """K is a multiple of 32 (fp32) / 64 (bf16): K = 32 passes the fp32 shape check (and is then stopped by the missing
    LayerNorm statistics, so nothing launches) where bf16 refuses the shape; K = 48 is no fp32 shape either"""
    probe = dict(pro=PRO_LN)
    assert _nt_ex("f32", dict(probe, K=32)) == EINVAL
    assert _nt_ex("f32", dict(probe, K=48)) == ESHAPE
    assert _nt_ex("bf16", dict(probe, K=32)) == ESHAPE
    assert _nt_ex("bf16", dict(probe, K=64)) == EINVAL


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("case", list(_TN_CASES))
def test_linear_tn_rejects_before_launching(dtype, det, case):
    over, status = _TN_CASES[case]
    assert _tn(dtype, det, over) == status


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(_DET_CASES))
def test_linear_tn_det_rejects_before_launching(dtype, case):
    """the deterministic form wants a workspace of at least one image and whole 32-row stages"""
    over, status = _DET_CASES[case]
    assert _tn(dtype, True, over) == status


def test_linear_sizing_functions_return_the_recorded_values():
    """hwgat_linear_tn_{f32,bf16}_ws_bytes and hwgat_linear_tn_det_bytes over the grid of
    tests/golden/make_fixtures_linear_sizes.py: the numbers follow from the M-split rules of the dW launchers, and the
    file was recorded from the library that still carried one hand-written copy of the rule per kernel"""
    L = hw._lib.lib()
    funcs = ("hwgat_linear_tn_f32_ws_bytes", "hwgat_linear_tn_bf16_ws_bytes", "hwgat_linear_tn_det_bytes")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_sizes.txt")) as fh:
        rows = [[int(v) for v in ln.split()] for ln in fh if not ln.startswith("#")]
    assert len(rows) == 8 * 12
    assert any(r[3] > 0 for r in rows) and any(r[4] > 0 for r in rows) and all(r[5] > 0 for r in rows)
    got = [[M, N, K] + [getattr(L, f)(M, N, K) for f in funcs] for M, N, K, *_ in rows]
    assert got == rows, [(g, r) for g, r in zip(got, rows) if g != r][:4]


@pytest.mark.parametrize("family", ["HWGATE", "HGATE", "WGATE"])
def test_checkpoint_interchange_with_the_reference_class(family):
    """state_dict of this backend loads STRICTLY into the reference Model and vice versa
    (SURVEY 8b / 8f-4), for the headline model and the sibling HGATE (8f-3).  The reference side -- constructor
    argument types, adjacency, state_dict layout, derived buffers -- is tests/golden/checkpoint_ref.npz
    (make_fixtures_checkpoint.py); `helpers.reference_standin` rebuilds a module with exactly that structure."""
    fx = load_fixture("checkpoint_ref.npz")
    tag = family + "_T64"
    ref = reference_standin(fx, tag)
    hp = getattr(hw, family + "Params")({"src_len": 64, "num_class": 11}, 2, torch.device("cpu"))
    assert [type(a).__name__ for a in hp.get_model_params()] == fx[tag + ".arg_types"].tolist()
    adj = torch.from_numpy(fx[tag + ".adj_mat"])
    assert hp.adj_mat.dtype == adj.dtype and torch.equal(hp.adj_mat, adj)
    mine = {"HWGATE": hw.Model, "HGATE": hw.HGATEModel, "WGATE": hw.WGATEModel}[family](*hp.get_model_params())
    sd_ref, sd_mine = ref.state_dict(), mine.state_dict()
    assert list(sd_ref.keys()) == list(sd_mine.keys())                       # same keys, same order
    assert all(sd_ref[k].shape == sd_mine[k].shape and sd_ref[k].dtype == sd_mine[k].dtype for k in sd_ref)
    for k in sd_ref:
        if k.endswith("attn_mask") or k == "adj_mask":
            assert torch.equal(sd_ref[k], sd_mine[k]), k                      # derived buffers are identical
    # the PE table is the reference's float32 formula: bit-equal on any one host to oracle.sinusoid_table, which
    # tests/golden/make_fixtures.py asserts against the reference itself.  Against the table recorded on another host
    # the last bits of exp / sin / cos may differ: a few ulp of the largest angle (T - 1 = 63 rad) at most.
    pe = sd_mine["pos_encoder.pe"]
    assert torch.equal(pe, O.sinusoid_table(64, 128))
    pe_err = (pe - sd_ref["pos_encoder.pe"]).abs().max().item()
    assert pe_err <= 8 * 64 * torch.finfo(torch.float32).eps, pe_err
    mine.load_state_dict(sd_ref, strict=True)
    ref.load_state_dict(sd_mine, strict=True)
    assert not mine.B.requires_grad and not ref.B.requires_grad
    assert sum(p.numel() for p in mine.parameters() if p.requires_grad) == \
        sum(p.numel() for p in ref.parameters() if p.requires_grad)


def test_sibling_mask_rows_on_cpu():
    """host-side mask compaction of the sibling models (no GPU needed): HGATE block bits decode back to the
    adjacency; WGATE band rows decode back to the three 16x16 blocks and malformed adjacencies are rejected"""
    from oracle import hgat_oracle as OH, wgat_oracle as OW
    HF = hw.functional
    adj = OH.block_adjacency()
    bits = HF.blk_mask_bits(adj, 29).numpy().astype(np.int64) & 0xFFFFFFFF
    assert bits.shape == (2, 64, 2)
    for tq in range(2):
        for jq in range(29):
            for tk in range(2):
                row = [(int(bits[0, tq * 32 + jq, tk]) >> j) & 1 for j in range(32)]
                assert row[:29] == [int(v) for v in adj[tq * 29 + jq, tk * 29:tk * 29 + 29]] and not any(row[29:])
                last = int(bits[1, tq * 32 + jq, tk])
                assert last == (int(bits[0, tq * 32 + jq, tk]) if tq == tk else 0)
    assert not bits[:, 29:32].any() and not bits[:, 61:64].any()              # pad query slots
    with pytest.raises(ValueError):
        HF.blk_mask_bits(adj * 0.5, 29)
    with pytest.raises(ValueError):
        HF.blk_mask_bits(torch.ones(70, 70), 35)

    T, nW = 5, 2
    band = OW.band_adjacency(T, nW)
    rows = HF.band_mask_rows(band, T)
    assert rows.shape == (nW, 16) and rows.dtype == torch.int64
    pa = OW.part_adjacency()
    for i in range(16):
        r = int(rows[1, i])
        assert [(r >> j) & 1 for j in range(16)] == [int(i == j) for j in range(16)]                 # previous frame
        assert [(r >> (16 + j)) & 1 for j in range(16)] == [int(v) for v in pa[i]]                   # same frame
        assert [(r >> (32 + j)) & 1 for j in range(16)] == [int(i == j) for j in range(16)]          # next frame
    assert HF.band_mask_rows(OW.band_adjacency(1, 1), 1).shape == (1, 16)                            # T = 1: no neighbours
    far = band.clone()
    far[0, 0, 3 * 16] = 1
    with pytest.raises(NotImplementedError):
        HF.band_mask_rows(far, T)
    no_diag = band.clone()
    no_diag[1, 2 * 16 + 4, 2 * 16:3 * 16] = 0
    with pytest.raises(NotImplementedError):
        HF.band_mask_rows(no_diag, T)
    with pytest.raises(ValueError):
        HF.band_mask_rows(band, T + 1)


def test_attention_dropout_is_a_constructor_hyper_parameter():
    """reference HWGATE.py:273 `attn_drop_rate`: accepted by the HWGATE backend (stored, used in train mode only), range
    checked; four site seeds per block (proj, fc1, fc2, attention); the sibling backends take it too (HGATE.py:232,
    WGATE.py:165) with the same range check"""
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, "cpu", num_kps=32)
    hp.attn_drop_rate = 0.1
    m = hw.Model(*hp.get_model_params())
    assert m.attn_drop_rate == 0.1
    assert len(m._seeds(0)) == 4 and len(set(m._seeds(0) + m._seeds(1))) == 8
    hp.attn_drop_rate = 1.0
    with pytest.raises(ValueError):
        hw.Model(*hp.get_model_params())
    with pytest.raises(ValueError):
        hw.functional.window_attention(torch.zeros(1, 2, 16, 3 * 64), torch.zeros(2, 1, 32, dtype=torch.int32), None, 1, False,
                                       drop=(1, 0.1))         # eval mode (no threshold) has no dropout
    for params, cls in ((hw.HGATEParams({"src_len": 16, "num_class": 5}, 2, "cpu"), hw.HGATEModel),
                        (hw.WGATEParams({"src_len": 16, "num_class": 5}, 2, "cpu", num_kps=32), hw.WGATEModel)):
        params.attn_drop_rate = 0.2
        assert cls(*params.get_model_params()).attn_drop_rate == 0.2
        params.attn_drop_rate = -0.1
        with pytest.raises(ValueError):
            cls(*params.get_model_params())


def test_dropout_seeds_differ_per_rank_and_per_call():
    """data-parallel ranks share torch's seed but not dropout masks: rank_salt enters the site seeds"""
    hp = hw.HWGATEParams({"src_len": 32, "num_class": 5}, 2, torch.device("cpu"), num_kps=32)
    torch.manual_seed(1001)
    m = hw.Model(*hp.get_model_params())
    base = m._seeds(3)
    assert len(set(base)) == 4 and m._seeds(3) == base and m._seeds(4) != base
    m.rank_salt = 1
    assert m._seeds(3) != base and len(set(m._seeds(3)) & set(base)) == 0
    m.rank_salt = 0
    m._drop_calls += 1
    assert m._seeds(3) != base
