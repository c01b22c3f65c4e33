"""CPU: the GATE model and WGATE window sizes other than 16 -- mask words, parameters, state_dict contract, refusals,
argument rejection of the new entry points, the integration shim, and the dense restatement of tests/gate_helpers.py
pinned to the reference-made fixtures (tests/golden/make_fixtures_gate.py)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch
from torch import nn

import gate_helpers as GH
from oracle import hwgat_oracle as O
from helpers import load_fixture, rel_err, grad_digest_check
from test_integration_cpu import scratch_tree, _Cfg, load_model            # noqa: F401  (fixture + the reference's lines)

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
TOL = 2e-5
FIXTURES = ["gate_a.npz", "gate_b.npz", "wgate_w32.npz", "wgate_w8.npz"]


def _random_edges(seed, W, n):
    rs = np.random.RandomState(seed)
    out = set()
    while len(out) < n:
        i, j = int(rs.randint(W)), int(rs.randint(W))
        if i != j:
            out.add((min(i, j), max(i, j)))
    return sorted(out)


# ------------------------------------------------------------------------------------------ mask words
def test_mask_words_of_the_gate_graph():
    T = 6
    hp = hw.GATEParams({"src_len": T, "num_class": 5}, 2, None)
    words = HF.wband_mask_rows(hp.adj_mat, T, 29)
    assert words.shape == (1, 32, 3) and words.dtype == torch.int32
    assert np.array_equal(words.numpy(), GH.expected_mask_words(hp.adj_mat, T, 29))
    w = words.numpy().astype(np.int64) & 0xFFFFFFFF
    for i in range(29):
        assert not (w[0, i, 1] >> i) & 1                                   # no self loop: the diagonal bit is clear
        assert w[0, i, 0] == w[0, i, 2] == 1 << i                          # the same joint in the neighbouring frames
        assert w[0, i, 1] != 0
    assert not w[0, 29:].any() and not (w >> 29).any()                     # pad rows and pad key bits stay 0
    assert torch.equal(words, HF.wband_mask_rows(hp.adj_mat.unsqueeze(0), T, 29))


@pytest.mark.parametrize("W,nW", [(8, 4), (29, 1), (32, 2)])
def test_mask_words_of_wgate_windows(W, nW):
    T = 5
    edges = [_random_edges(10 * W + w, W, (3 * W) // 2) for w in range(nW)]
    adj = GH.default_adjacency(edges, W, T, self_loops=True)
    words = HF.wband_mask_rows(adj, T, W)
    assert np.array_equal(words.numpy(), GH.expected_mask_words(adj, T, W))
    # arbitrary, asymmetric blocks: prev != next, no diagonal required
    g = torch.Generator().manual_seed(W)
    diag = (torch.rand(nW, W, W, generator=g) < 0.3).float()
    diag[:, torch.arange(W), (torch.arange(W) + 1) % W] = 1.0             # every row keeps a same-frame key
    prev = (torch.rand(nW, W, W, generator=g) < 0.2).float()
    nxt = (torch.rand(nW, W, W, generator=g) < 0.2).float()
    adj = GH.band_adjacency(diag, prev, nxt, T)
    assert np.array_equal(HF.wband_mask_rows(adj, T, W).numpy(), GH.expected_mask_words(adj, T, W))


def test_mask_words_refuse_what_the_kernel_cannot_do():
    T, W = 6, 29
    adj = hw.GATEParams({"src_len": T, "num_class": 5}, 2, None).adj_mat
    bad = adj.clone()
    bad[0 * W + 3, 4 * W + 3] = 1                                          # frame 0 sees frame 4
    with pytest.raises(NotImplementedError, match="block-tridiagonal"):
        HF.wband_mask_rows(bad, T, W)
    bad = adj.clone()
    bad[3 * W + 2, 3 * W + 9] = 1 - bad[3 * W + 2, 3 * W + 9]              # one frame differs
    with pytest.raises(NotImplementedError, match="same adjacency blocks on every frame"):
        HF.wband_mask_rows(bad, T, W)
    bad = adj.view(T, W, T, W).clone()
    bad[:, 5, :, :] = 0                                                    # joint 5 sees no key of its own frame ...
    for f in range(T - 1):
        bad[f, 5, f + 1, 5] = bad[f + 1, 5, f, 5] = 1                      # ... only itself in the neighbouring frames
    with pytest.raises(NotImplementedError, match="visible key in its own frame"):
        HF.wband_mask_rows(bad.reshape(T * W, T * W), T, W)
    with pytest.raises(NotImplementedError, match="at most 32 joints"):
        HF.wband_mask_rows(torch.zeros(1, 2 * 33, 2 * 33), 2, 33)
    with pytest.raises(ValueError, match="0/1"):
        HF.wband_mask_rows(adj * 0.5, T, W)
    with pytest.raises(ValueError, match="adjacency must be"):
        HF.wband_mask_rows(adj, T + 1, W)


# ------------------------------------------------------------------------------------------ parameters, contract
def test_gate_params_equal_the_reference():
    fx = load_fixture("gate_a.npz")
    hp = hw.GATEParams({"src_len": 32, "num_class": 10}, 2, torch.device("cpu"))
    for k in ("kp_dim", "num_kps", "temporal_dim", "num_classes", "embed_dim", "pe", "depths", "num_heads", "ff_ratio",
              "drop_rate", "attn_drop_rate"):
        assert getattr(hp, k) == fx["hp." + k].item(), k
    assert hp.norm_layer is nn.LayerNorm and hp.device == torch.device("cpu")
    as_set = lambda e: {(min(i, j), max(i, j)) for i, j in np.asarray(e).tolist()}     # noqa: E731
    assert as_set(hp.edges) == as_set(fx["hp.edges"]) and len(hp.edges) == len(fx["hp.edges"])
    tup = hp.get_model_params()
    assert len(tup) == int(fx["hp.tuple_len"]) == 14
    assert tup[:9] == (2, 29, 32, 10, 128, True, 8, 8, 2.0) and tup[9] is hp.adj_mat and tup[10:13] == (0.1, 0.0, nn.LayerNorm)
    # the adjacency the reference built, block by block
    blocks = torch.from_numpy(fx["adj_blocks"]).float()
    assert torch.equal(hp.adj_mat, GH.band_adjacency(blocks[:, 1], blocks[:, 0], blocks[:, 2], 32)[0])
    assert hp.adj_mat.dtype == torch.float32 and not bool(torch.diagonal(hp.adj_mat).any())


@pytest.mark.parametrize("name", ["gate_a.npz", "gate_b.npz"])
def test_gate_state_dict_contract(name):
    fx = load_fixture(name)
    cfg, params, adj = GH.fixture_setup(fx)
    hp = hw.GATEParams({"src_len": cfg["temporal_dim"], "num_class": cfg["num_classes"]}, cfg["kp_dim"], None)
    hp.num_heads, hp.depths, hp.pe = cfg["num_heads"], cfg["depths"], cfg["use_pe"]
    model = hw.GATEModel(*hp.get_model_params())
    sd = model.state_dict()
    assert list(sd) == fx["state.keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == fx["state.shapes"].tolist()
    W = 29
    assert np.array_equal(sd["adj_mask"][0, 0, :2 * W, :2 * W].numpy(), fx["adj_mask_head"])
    assert not model.B.requires_grad
    if cfg["use_pe"]:
        assert torch.equal(sd["pos_encoder.pe"], O.sinusoid_table(cfg["temporal_dim"], 128))
    res = model.load_state_dict(params, strict=False)
    assert not res.unexpected_keys and res.missing_keys == ["adj_mask"]
    assert [n for n, p in model.named_parameters() if p.requires_grad and n.startswith("weightedAvg")] == \
        ["weightedAvg.weight", "weightedAvg.bias"]
    # the reference's init: zero biases everywhere, LayerNorm at identity
    fresh = hw.GATEModel(*hp.get_model_params())
    assert float(fresh.weightedAvg.bias.detach().abs().max()) == 0.0 == float(fresh.head.bias.detach().abs().max())
    assert 0.01 < float(fresh.weightedAvg.weight.detach().std()) < 0.03                # trunc_normal_(std=.02)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.rand(1, cfg["temporal_dim"], 29, cfg["kp_dim"]))


def test_constructor_refusals_name_their_rule():
    T = 4
    hp = hw.GATEParams({"src_len": T, "num_class": 5}, 2, None)

    def build(**over):
        args = dict(zip(("kp_dim", "num_kps", "temporal_dim", "num_classes", "embed_dim", "pe", "depths", "num_heads",
                         "ff_ratio", "adj_mat", "drop_rate", "attn_drop_rate", "norm_layer", "device"), hp.get_model_params()))
        args.update(over)
        return hw.GATEModel(*args.values())
    build(depths=1)
    with pytest.raises(NotImplementedError, match="at most 32 joints"):
        build(num_kps=34, adj_mat=torch.zeros(T * 34, T * 34))
    with pytest.raises(NotImplementedError, match="head_dim 16 or 32"):
        build(num_heads=16)                                                # head_dim 8
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        build(norm_layer=nn.BatchNorm1d)
    with pytest.raises(NotImplementedError, match="adjacency"):
        build(adj_mat=None)
    with pytest.raises(ValueError, match="attn_drop_rate"):
        build(attn_drop_rate=1.0)


def _wgate_params(T, K, W, seed=3):
    hp = hw.WGATEParams({"src_len": T, "num_class": 5}, 2, None, num_kps=K)
    hp.window_size, hp.depths = W, 1
    hp.edges = [[list(e) for e in _random_edges(seed + w, W, W)] for w in range(K // W)]
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    return hp


def test_wgate_window_sizes():
    defaults = hw.WGATEParams({"src_len": 4, "num_class": 5}, 2, None)
    assert defaults.window_size == 16 and defaults.num_kps == 64 and defaults.adj_mat.shape == (4, 64, 64)
    assert hw.WGATEModel(*defaults.get_model_params())._attn_kind == "band"           # W = 16: the kernels it always had
    for W, K in ((32, 64), (8, 32)):
        hp = _wgate_params(4, K, W)
        model = hw.WGATEModel(*hp.get_model_params())
        assert model._attn_kind == "wband" and model.n_windows == K // W and model.window_size == W
        assert tuple(model._mask_bits.shape) == (K // W, 32, 3) and tuple(model.adj_mask.shape) == (K // W, 4 * W, 4 * W)
        assert np.array_equal(model._mask_bits.numpy(), GH.expected_mask_words(hp.adj_mat, 4, W))
    hp = _wgate_params(2, 96, 48)
    with pytest.raises(NotImplementedError, match="at most 32"):
        hw.WGATEModel(*hp.get_model_params())


# ------------------------------------------------------------------------------------------ C ABI
def test_new_entry_points_reject_bad_arguments_without_launching():
    L = hw._lib.lib()
    assert {"hwgat_wband_attn_fwd", "hwgat_wband_attn_bwd", "hwgat_wband_attn_fwd_drop", "hwgat_wband_attn_bwd_drop",
            "hwgat_lnwpool_fwd", "hwgat_lnwpool_fwd_det", "hwgat_lnwpool_bwd_masked"} <= set(hw._lib.declared_symbols())
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (qkv, o, maskrows, B, F, nW, W, nH, hd, dtype, stream)
    assert L.hwgat_wband_attn_fwd(None, p, p, 1, 4, 1, 29, 8, 16, 0, None) == -1
    assert L.hwgat_wband_attn_fwd(p, p, None, 1, 4, 1, 29, 8, 16, 0, None) == -1
    assert L.hwgat_wband_attn_fwd(p, p, p, 1, 4, 1, 33, 8, 16, 0, None) == -2                # W > 32
    assert L.hwgat_wband_attn_fwd(p, p, p, 1, 4, 1, 0, 8, 16, 0, None) == -2                 # W < 1
    assert L.hwgat_wband_attn_fwd(p, p, p, 1, 4, 1, 29, 8, 64, 0, None) == -2                # head_dim 64
    assert L.hwgat_wband_attn_fwd(p, p, p, 1, 0, 1, 29, 8, 16, 0, None) == -2                # F = 0
    assert L.hwgat_wband_attn_fwd(p, p, p, 1, 4, 1, 29, 8, 16, 5, None) == -3                # dtype
    assert L.hwgat_wband_attn_bwd(p, None, p, p, 1, 4, 1, 29, 8, 16, 0, None) == -1
    assert L.hwgat_wband_attn_bwd(p, p, p, p, 1, 4, 0, 29, 8, 16, 0, None) == -2             # nW = 0
    assert L.hwgat_wband_attn_bwd(p, p, p, p, 1, 4, 1, 29, 8, 16, 2, None) == -3
    assert L.hwgat_wband_attn_fwd_drop(p, p, p, 1, 4, 1, 29, 8, 16, 0, 1, 1.0, None, None) == -1      # p >= 1
    assert L.hwgat_wband_attn_fwd_drop(p, p, p, 1, 4, 1, 29, 8, 16, 0, 1, -0.1, None, None) == -1
    assert L.hwgat_wband_attn_bwd_drop(p, p, p, p, 1, 4, 1, 29, 8, 16, 0, 1, 1.5, None, None) == -1
    assert L.hwgat_wband_attn_bwd_drop(p, p, p, p, 1, 4, 1, 40, 8, 16, 0, 1, 0.5, None, None) == -2
    # (x, wtok, xhat_wsum, mean, rstd, B, n_tok, d, dtype[, partial], stream)
    assert L.hwgat_lnwpool_fwd(p, None, p, p, p, 1, 4, 128, 0, None) == -1
    assert L.hwgat_lnwpool_fwd(p, p, p, p, p, 1, 0, 128, 0, None) == -1
    assert L.hwgat_lnwpool_fwd(p, p, p, p, p, 1, 4, 100, 0, None) == -2                      # width 100
    assert L.hwgat_lnwpool_fwd_det(p, p, p, p, p, 1, 4, 128, 9, p, None) == -3
    # (g, wtok, x, mean, rstd, dx, gdot, B, n_tok, d, dtype, dxm, seed, p, seed_base, stream)
    assert L.hwgat_lnwpool_bwd_masked(p, p, p, p, p, p, None, 1, 4, 128, 0, None, 0, 0.0, None, None) == -1
    assert L.hwgat_lnwpool_bwd_masked(p, p, p, p, p, p, p, 1, 4, 128, 0, p, 0, 0.0, None, None) == -1   # masked copy, p = 0
    assert L.hwgat_lnwpool_bwd_masked(p, p, p, p, p, p, p, 1, 4, 96, 0, None, 0, 0.0, None, None) == -2
    # (width, dtype) left open: a width no kernel takes is HWGAT_ESHAPE -- the odd multiples of 64 among them, which only
    # the mean pool has kernels for -- and an unknown dtype is HWGAT_EDTYPE whatever the width
    wpool = {
        "hwgat_lnwpool_fwd": lambda d, t: (p, p, p, p, p, 1, 4, d, t, None),
        "hwgat_lnwpool_fwd_det": lambda d, t: (p, p, p, p, p, 1, 4, d, t, p, None),
        "hwgat_lnwpool_bwd_masked": lambda d, t: (p,) * 7 + (1, 4, d, t, p, 1, 0.5, None, None),
    }
    for name, args in wpool.items():
        for d in (100, 1088, 0, 192):
            assert getattr(L, name)(*args(d, 0)) == -2, (name, d)
        for d in (100, 128, 192):
            assert getattr(L, name)(*args(d, 9)) == -3, (name, d)


def test_gate_backend_resolves_by_file_name_like_the_reference(scratch_tree):      # noqa: F811
    cfg = _Cfg("GATE_AMD", "INCLUDE")
    assert type(cfg.model_params) is hw.GATEParams
    cfg.model_params.depths = 2                            # the (T K)^2 buffer is 14 MB at T = 64; two blocks are enough here
    model = load_model(cfg)
    assert type(model) is hw.GATEModel and model.num_classes == 262 and model.temporal_dim == 64
    sd = model.state_dict()
    assert tuple(sd["adj_mask"].shape) == (1, 1, 64 * 29, 64 * 29) and tuple(sd["weightedAvg.weight"].shape) == (1, 64 * 29)
    assert hw.GATEModel is importlib.import_module("sl-hwgat_amd.models.GATE").Model


# ------------------------------------------------------------------------------------------ the restatement vs the reference
def _sub(t):
    return t[:, ::3, ::5, ::11]


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_forward(name):
    fx = load_fixture(name)
    model, params, cfg, adj = GH.dense_model_from_fixture(fx, torch.float32)
    with torch.no_grad():
        logits = model.forward(torch.from_numpy(fx["x"]), tap=True)
    assert rel_err(logits, fx["eval.logits"]) < TOL
    assert rel_err(model.taps["feat"], fx["eval.feat"]) < TOL
    for b in range(cfg["depths"]):
        assert rel_err(_sub(model.taps[f"block{b}"]), fx[f"eval.block{b}"]) < TOL, b
    last = model.taps[f"block{cfg['depths'] - 1}"]
    assert rel_err(model.taps["block0"][0, :2], fx["eval.block0.full"]) < TOL
    assert rel_err(model.taps["block0"][0, -2:], fx["eval.block0.tail"]) < TOL
    assert rel_err(last[-1, :2], fx["eval.last.full"]) < TOL
    assert rel_err(last[-1, -2:], fx["eval.last.tail"]) < TOL
    if cfg["kind"] == "gate":       # the fixtures tell a weighted pool from a mean pool
        w = params["weightedAvg.weight"]
        assert float(w.max() / w.min()) > 3.0 and float(params["weightedAvg.bias"]) != 0.0
        mean_feat = O.layer_norm(last, params["norm.weight"], params["norm.bias"]).mean(dim=(1, 2))
        assert rel_err(mean_feat, fx["eval.feat"]) > 1e-2


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_backward(name):
    fx = load_fixture(name)
    model, params, cfg, adj = GH.dense_model_from_fixture(fx, torch.float32)
    ps = {k: v.clone().requires_grad_(k not in ("B", "pos_encoder.pe")) for k, v in params.items()}
    model.p = ps
    loss = O.smoothed_cross_entropy(model.forward(torch.from_numpy(fx["x"])), torch.from_numpy(fx["y"]))
    loss.backward()
    assert abs(loss.item() - float(fx["evalbwd.loss"])) < 1e-5
    grads = {k: v.grad for k, v in ps.items() if v.grad is not None}
    if cfg["kind"] == "gate":
        assert "weightedAvg.weight" in grads and "evalbwd.gh.weightedAvg.weight" in fx
    grad_digest_check(grads, fx, "evalbwd.", 2e-4)


def test_restated_attention_is_a_band():
    """the dense restatement gives exactly zero probability outside the adjacency (fp32), GATE's no-self-loop graph
    included -- what the fixture generator asserts on the reference's own softmax"""
    T, W, nH = 6, 29, 2
    adj = hw.GATEParams({"src_len": T, "num_class": 5}, 2, None).adj_mat
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(2, T, W, 3 * 32, generator=g) * 3
    _, p = GH.dense_band_attention(qkv, adj, nH, W, return_probs=True)
    assert float((p * (adj == 0)).max()) == 0.0
    assert torch.allclose(p.sum(-1), torch.ones(()), atol=1e-5)
