"""CPU: the DecoupledGCN baseline -- the DecoupledGCNParams tuple and construction, the adjacency and the reference's
state_dict layout (tests/golden/dgcn_*.npz, make_fixtures_dgcn.py), every refusal, the DecoupledGCN_AMD shim as the
reference resolves it, header <-> bindings <-> exports of the new entry points, and the fp64 restatement of the contract
against every fixture (floor rule for the analytically zero biases, ReLU-mask and seed round trip, non-trivial masks)."""
import ctypes
import importlib
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import dgcn_helpers as DH
from helpers import load_fixture, reference_structure, reference_standin

hw = importlib.import_module("sl-hwgat_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["a", "b", "c", "d"]
E = DH.EDGES_29
NEW_SYMBOLS = {"hwgat_dgcn_agg_fwd", "hwgat_dgcn_agg_bwd_bytes", "hwgat_dgcn_agg_bwd", "hwgat_dgcn_gate_sum",
               "hwgat_dgcn_gate_apply", "hwgat_dgcn_gate_bwd", "hwgat_dgcn_abs_sum", "hwgat_dgcn_draw",
               "hwgat_dgcn_mask_spatial", "hwgat_dgcn_mask_temporal", "hwgat_dgcn_merge", "hwgat_dgcn_merge_bwd",
               "hwgat_dgcn_masked_sum"}


def test_params_tuple_and_construction():
    sp = hw.DecoupledGCNParams({"src_len": 128, "num_class": 2002}, 2, None)
    args = sp.get_model_params()
    assert args[:2] == (2, 29) and args[3:] == (8, 41, 256, 2002, 0, False)
    assert len(args[2]) == 34 and args[2] == E
    m = hw.DecoupledGCNModel(*args)
    assert len(m.units) == 10 and [u.stride for u in m.units] == DH.STRIDES
    assert [(u.in_channels, u.out_channels) for u in m.units] == [(ci, co) for ci, co, _, _ in DH.unit_plan(DH.CONFIGS["a"])]
    assert abs(m.drop_size - 2 * 34 / 29) < 1e-12 and m.drop_size == DH.find_drop_size(29, 34)
    assert m.deterministic_eval and m._seed_state.shape == (4,) and m._drop_calls == 0
    assert m.frames_out(128) == 32 and m.frames_out(13) == 4 and m.frames_out(1) == 1
    assert m.l1.conv_sa.weight.shape == (1, 64, 29) and m.l1.conv_sa.padding == (14,)
    assert hw.DecoupledGCNModel(2, 28, [[0, 1]], 8, 41, 256, 5, 0, False).l1.conv_sa.weight.shape == (1, 64, 27)
    # the reference's initialisation
    w = m.head.classifier.weight.detach()
    assert abs(float(w.std()) - (2.0 / 2002) ** 0.5) < 0.05 * (2.0 / 2002) ** 0.5
    for u in m.units:
        co = u.out_channels
        assert float(u.gcn1.bn.weight.detach().min()) == float(u.gcn1.bn.weight.detach().max()) == pytest.approx(1e-6)
        assert float(u.gcn1.bn0.weight.detach().min()) == 1.0 and float(u.tcn1.bn.weight.detach().max()) == 1.0
        assert float(u.gcn1.linear_bias.detach().min()) == float(u.gcn1.linear_bias.detach().max()) == pytest.approx(1e-6)
        assert abs(float(u.gcn1.linear_weight.detach().std()) / (0.5 / (3 * co)) ** 0.5 - 1) < 0.2
        assert float(u.conv_ta.weight.detach().abs().max()) == 0.0 and float(u.fc2c.weight.detach().abs().max()) == 0.0
        assert float(u.conv_sa.weight.detach().std()) > 0 and float(u.fc1c.weight.detach().std()) > 0 and float(u.fc1c.bias.detach().abs().max()) == 0.0
        assert abs(float(u.tcn1.conv.weight.detach().std()) / (2.0 / (co * 9)) ** 0.5 - 1) < 0.2         # Kaiming, fan-out
        assert not u.A.requires_grad and not u.gcn1.eye_list.requires_grad and u.gcn1.decoupled_A.requires_grad
        assert torch.equal(u.gcn1.eye_list, torch.eye(29).expand(co, 29, 29))
    assert m.set_activation_dtype(torch.float32) is m
    with pytest.raises(NotImplementedError, match="fp32 only"):
        m.set_activation_dtype(torch.bfloat16)


@pytest.mark.parametrize("name", NAMES)
def test_adjacency_and_state_dict_match_reference(name):
    fx = load_fixture(f"dgcn_{name}.npz")
    cfg = DH.CONFIGS[name]
    m = hw.DecoupledGCNModel(*DH.model_args(cfg))
    mod = importlib.import_module("sl-hwgat_amd.models.DecoupledGCN")
    assert np.array_equal(mod.spatial_graph(cfg["V"], cfg["edges"]), fx["A"])               # bit for bit, float64
    for u in m.units:
        assert np.array_equal(u.A.numpy(), fx["A_sum"]) and u.A.dtype == torch.float32
        assert np.array_equal(u.gcn1.decoupled_A.detach().numpy(),
                              np.repeat(fx["A"].astype(np.float32)[:, None], cfg["G"], axis=1))
    sd = m.state_dict()
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [t[:3] for t in reference_structure(fx, "sd")]
    assert [n for n, _ in m.named_parameters()] == fx["sd.params"].tolist()
    assert [p.requires_grad for _, p in m.named_parameters()] == fx["sd.requires_grad"].tolist()
    assert sd["data_bn.num_batches_tracked"].dtype == torch.int64
    ref = reference_standin(fx, "sd")
    m.load_state_dict(ref.state_dict(), strict=True)
    back = ref.load_state_dict(m.state_dict(), strict=True)
    assert not back.missing_keys and not back.unexpected_keys
    for (k, v), (k2, v2) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    # an AdamW state built on either side loads on the other
    o_ref = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=1e-3)
    for p in ref.parameters():
        if p.requires_grad:
            p.grad = torch.ones_like(p)
    o_ref.step()
    o_mine = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    o_mine.load_state_dict(o_ref.state_dict())
    o_ref.load_state_dict(o_mine.state_dict())


@pytest.mark.parametrize("args,rule", [
    ((2, 29, E, 8, 41, 256, 10, 0.0, True), "batch_norm=True"),
    ((0, 29, E, 8, 41, 256, 10, 0.0, False), "in_channels"),
    ((5, 29, E, 8, 41, 256, 10, 0.0, False), "in_channels"),
    ((2, 33, [], 8, 41, 256, 10, 0.0, False), "num_nodes"),
    ((2, 29, E, 3, 41, 256, 10, 0.0, False), "must divide 64"),
    ((2, 29, E, 128, 41, 256, 10, 0.0, False), "must divide 64"),
    ((2, 29, E, 8, 4, 256, 10, 0.0, False), "must be odd"),
    ((2, 29, E, 8, 41, 96, 10, 0.0, False), "multiples of 64 up to 1024"),
    ((2, 29, E, 8, 41, 1088, 10, 0.0, False), "multiples of 64 up to 1024"),
    ((2, 29, None, 8, 41, 256, 10, 0.0, False), "edge list is required"),
    ((2, 20, E, 8, 41, 256, 10, 0.0, False), "edge"),
])
def test_refusals_name_the_rule(args, rule):
    with pytest.raises(NotImplementedError, match=rule):
        hw.DecoupledGCNModel(*args)


def test_accepted_corners_and_forward_refusals():
    for c, g in ((1, 1), (4, 64)):
        hw.DecoupledGCNModel(c, 32, [[0, 1]], g, 3, 1024, 3, 0.0, False)
    m = hw.DecoupledGCNModel(2, 29, E, 8, 41, 64, 3, 0.0, False)
    with pytest.raises(ValueError, match="dropout_ratio"):
        hw.DecoupledGCNModel(2, 29, E, 8, 41, 64, 3, 1.0, False)
    with pytest.raises(ValueError, match=r"expected \(N, T, 29, 2\)"):
        m(torch.zeros(1, 8, 29, 3))
    with pytest.raises(ValueError, match=r"expected \(N, T, 29, 2\)"):
        m(torch.zeros(1, 8, 28, 2))
    for kp in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="keep_prob"):
            m(torch.zeros(2, 8, 29, 2), kp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a CPU tensor never falls back to torch arithmetic
        m(torch.zeros(2, 8, 29, 2))


def test_integration_shim_resolves_like_the_reference(tmp_path, monkeypatch):
    pkg = tmp_path / "hwgat" / "models"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    shims = os.path.join(ROOT, "integration", "models")
    for f in ("DecoupledGCN_AMD.py", "model_params_amd.py"):
        shutil.copy(os.path.join(shims, f), pkg / f)
    (pkg / "model_params.py").write_text("class DecoupledGCNParams:\n    pass\n\n\nfrom models.model_params_amd import *\n")
    monkeypatch.setenv("HWGAT_AMD_ROOT", ROOT)
    monkeypatch.syspath_prepend(str(tmp_path / "hwgat"))
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        monkeypatch.delitem(sys.modules, k)
    try:
        module = importlib.import_module("models.model_params")                                   # configs.py:80
        params = getattr(module, "DecoupledGCN_AMD" + "Params")({"src_len": 64, "num_class": 20}, 3, torch.device("cpu"))
        model = getattr(importlib.import_module("models.DecoupledGCN_AMD"), "Model")(*params.get_model_params())
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            sys.modules.pop(k, None)
    assert type(model) is hw.DecoupledGCNModel and model.in_channels == 3 and model.head.classifier.out_features == 20
    assert type(params) is hw.DecoupledGCNParams


def test_new_entry_points_declared_bound_and_exported():
    assert NEW_SYMBOLS <= set(hw._lib.declared_symbols())
    assert NEW_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_dgcn_")}
    handle = hw._lib.lib()
    for n in NEW_SYMBOLS:
        assert getattr(handle, n) is not None
    assert handle.hwgat_abi_version() == hw._lib.header_abi_version() == 4007
    # argument checks that need no device: null pointers and unsupported shapes are refused before any launch
    assert handle.hwgat_dgcn_agg_fwd(None, None, None, 4, 29, 64, 8, None) == -1
    assert handle.hwgat_dgcn_agg_bwd(None, None, None, None, None, 4, 29, 64, 8, None, 0, None) == -1
    assert handle.hwgat_dgcn_gate_sum(None, None, None, None, None, None, 0.0, None, 2, 4, 29, 64, 0, 1.0, None) == -1
    assert handle.hwgat_dgcn_gate_apply(None, None, None, None, None, 2, 4, 29, 64, None) == -1
    assert handle.hwgat_dgcn_gate_bwd(None, None, None, None, None, None, None, 2, 4, 29, 64, None) == -1
    assert handle.hwgat_dgcn_abs_sum(None, None, None, None, None, None, None, 2, 4, 29, 64, 0, None) == -1
    assert handle.hwgat_dgcn_draw(None, None, 8, 1, None, None) == -1
    assert handle.hwgat_dgcn_mask_spatial(None, None, None, None, 2, 29, None) == -1
    assert handle.hwgat_dgcn_mask_temporal(None, None, None, 2, 8, 5, None) == -1
    assert handle.hwgat_dgcn_merge(*([None] * 15), 2, 4, 29, 64, None) == -1
    assert handle.hwgat_dgcn_merge_bwd(*([None] * 8), 2, 4, 29, 64, None) == -1
    assert handle.hwgat_dgcn_masked_sum(None, None, None, None, None, 8, None) == -1
    assert handle.hwgat_dgcn_agg_bwd_bytes(0, 8) == -1 and handle.hwgat_dgcn_agg_bwd_bytes(32, 0) == -1
    assert handle.hwgat_dgcn_agg_bwd_bytes(32, 8) == 32 * 8 * 3 * 32 * 32 * 4
    assert handle.hwgat_dgcn_agg_bwd_bytes(100000, 4) == 128 * 4 * 3 * 32 * 32 * 4


def test_unsupported_shapes_are_refused_before_any_launch():
    """non-null pointers with a shape outside a kernel's rules: HWGAT_ESHAPE (-2), a bad axis or workspace HWGAT_EINVAL
    (-1), decided on the host before anything is launched (the pointers are never read)"""
    L = hw._lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 20                                                                           # N T V C / 256 past 2^31
    assert L.hwgat_dgcn_agg_fwd(p, p, p, 4, 33, 64, 8, None) == -2                          # V > 32
    assert L.hwgat_dgcn_agg_fwd(p, p, p, 4, 29, 65, 8, None) == -2                          # C % G
    assert L.hwgat_dgcn_agg_fwd(p, p, p, 4, 29, 1 << 17, 1 << 16, None) == -2               # G past the grid's y extent
    assert L.hwgat_dgcn_agg_fwd(p, p, p, 4, 0, 64, 8, None) == -1                           # V = 0
    assert L.hwgat_dgcn_agg_bwd(p, p, p, p, None, 4, 33, 64, 8, None, 0, None) == -2        # V > 32
    assert L.hwgat_dgcn_agg_bwd(p, p, p, p, None, 4, 29, 65, 8, None, 0, None) == -2        # C % G
    assert L.hwgat_dgcn_agg_bwd(p, p, p, p, p, 4, 29, 64, 8, None, 0, None) == -1           # d An without a workspace
    assert L.hwgat_dgcn_agg_bwd(p, p, p, p, p, 4, 29, 64, 8, p, L.hwgat_dgcn_agg_bwd_bytes(4, 8) - 1, None) == -1
    assert L.hwgat_dgcn_gate_sum(p, None, None, None, None, None, 0.0, p, 2, 4, 33, 64, 0, 1.0, None) == -2    # V > 32
    assert L.hwgat_dgcn_gate_sum(p, None, None, None, None, None, 0.0, p, 2, 4, 29, 64, 2, 1.0, None) == -1    # axis 2
    assert L.hwgat_dgcn_gate_sum(p, None, None, None, None, None, 0.0, p, big, big, 29, 64, 0, 1.0, None) == -2
    assert L.hwgat_dgcn_gate_apply(p, p, p, p, p, 2, 4, 33, 64, None) == -2
    assert L.hwgat_dgcn_gate_apply(p, p, p, p, p, big, big, 29, 64, None) == -2
    assert L.hwgat_dgcn_gate_bwd(p, p, p, p, None, None, p, 2, 4, 33, 64, None) == -2
    assert L.hwgat_dgcn_gate_bwd(p, p, p, p, None, None, p, 2, 0, 29, 64, None) == -1       # T = 0
    assert L.hwgat_dgcn_abs_sum(p, None, None, None, None, None, p, 2, 4, 33, 64, 0, None) == -2
    assert L.hwgat_dgcn_abs_sum(p, None, None, None, None, None, p, 2, 4, 29, 64, 3, None) == -1               # axis 3
    assert L.hwgat_dgcn_abs_sum(p, p, None, p, p, None, p, 2, 4, 29, 64, 0, None) == -1     # half a BatchNorm
    assert L.hwgat_dgcn_draw(p, p, 1 << 40, 1, None, None) == -2
    assert L.hwgat_dgcn_mask_spatial(p, p, p, p, 2, 33, None) == -2                         # V > 32
    assert L.hwgat_dgcn_mask_temporal(p, p, p, 2, 8, 4, None) == -2                         # an even block
    assert L.hwgat_dgcn_mask_temporal(p, p, p, 2, 8, 0, None) == -1
    assert L.hwgat_dgcn_merge(*([p] * 15), 2, 4, 33, 64, None) == -2
    assert L.hwgat_dgcn_merge(*([p] * 6), p, None, p, p, *([p] * 5), 2, 4, 29, 64, None) == -1   # half a residual BatchNorm
    assert L.hwgat_dgcn_merge_bwd(*([p] * 8), 2, 4, 33, 64, None) == -2
    assert L.hwgat_dgcn_masked_sum(p, None, p, None, p, 1 << 40, None) == -2


def _params(name):
    cfg = DH.CONFIGS[name]
    m = hw.DecoupledGCNModel(*DH.model_args(cfg))
    return DH.fixture_weights(m.state_dict(), cfg), cfg


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_fixture(name, training):
    fx = load_fixture(f"dgcn_{name}.npz")
    P, cfg = _params(name)
    x, y = DH.fixture_input(fx, cfg)
    tag = "train." if training else "eval."
    rec, log = DH.Record(), []
    logits, loss, grads = DH.grads_of(P, x, y, cfg, training, rec=rec, seeds=DH.all_drop_seeds(cfg), log=log)
    ref = torch.from_numpy(fx[tag + "logits"]).double()
    assert ((logits - ref).norm() / ref.norm()).item() < max(1e-6, 4 * float(fx[f"refdev.{tag}logits"]))
    assert abs(loss.item() - float(fx[tag + "loss"])) < max(1e-6, 4 * float(fx[f"refdev.{tag}loss"])) * max(1.0, abs(loss.item()))
    assert rec.margin >= float(fx["margin"]) * (1 - 1e-3)          # the fixture's margin is the smaller of both modes
    assert len(rec.masks) == 30
    if training:
        for i, h in enumerate(rec.blocks):
            r = torch.from_numpy(fx[f"train.block{i}"]).double()
            # the fixture holds the fp32 reference: its own distance to fp64 (refdev) sets the bound
            assert ((DH.block_samples(h) - r).norm() / r.norm()).item() < max(1e-6, 4 * float(fx[f"refdev.train.block{i}"])), i
        for k, v in rec.stats.items():
            r = torch.from_numpy(np.asarray(fx["train.stat." + k]))
            if not v.is_floating_point():
                assert (v == r).all(), k
            else:
                assert ((v - r).norm() / r.norm()).item() < max(1e-6, 4 * float(fx["refdev.train.stat." + k])), k
        assert len(log) == 16 and DH.masks_are_sound(log)
        for unit, site, p, _, _, _ in log:
            r = torch.from_numpy(fx[f"train.p.{unit}.{site}"]).double()
            assert ((p - r).norm() / r.norm()).item() < max(1e-6, 4 * float(fx[f"refdev.train.p.{unit}.{site}"])), (unit, site)
    else:
        assert not log
    if not cfg["tight"]:
        return
    assert float(fx["margin"]) >= 2e-6
    zero = DH.zero_grad_biases(grads) if training else {}
    assert len(DH.gate_biases(grads)) == 20 and set(rec.terms) == set(DH.gate_biases(grads))
    for n, g in grads.items():
        dev = float(fx[f"refdev.{tag}g.{n}"])
        assert dev < 2e-5, (n, dev)
        tol = max(2e-5, 4.0 * float(fx[f"refdev.{tag}g.{n}"]))
        if n in zero:
            # floor rule: in fp64 these gradients vanish against the matching weight gradient
            assert g.norm().item() < 1e-12 * grads[zero[n]].norm().item(), n
            continue
        if n in rec.terms:                  # a gate bias: the recorded sum of its terms is the fixture's scale
            assert abs(rec.terms[n] - float(fx[tag + "gs." + n])) < 1e-9 * rec.terms[n], n
        DH.digest_check(n, g, fx, tag, tol)


def test_restatement_relu_masks_and_seeds_round_trip():
    """the restatement with its own ReLU masks fed back returns the same gradients; a flipped mask entry or another seed
    pattern changes them"""
    P, cfg = _params("b")
    x, y = DH.make_input(cfg, seed=1)
    seeds = DH.all_drop_seeds(cfg)
    rec = DH.Record()
    _, _, g0 = DH.grads_of(P, x, y, cfg, True, rec=rec, seeds=seeds)
    assert len(rec.masks) == 30 and sum(k.endswith("relu_c") for k in rec.masks) == 10
    _, _, g1 = DH.grads_of(P, x, y, cfg, True, masks=rec.masks, seeds=seeds)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    flipped = {k: v.clone() for k, v in rec.masks.items()}
    flipped["l6.relu"][0, 0, 0, :8] = ~flipped["l6.relu"][0, 0, 0, :8]
    _, _, g2 = DH.grads_of(P, x, y, cfg, True, masks=flipped, seeds=seeds)
    assert not torch.equal(g0["l1.gcn1.linear_weight"], g2["l1.gcn1.linear_weight"])
    other = dict(seeds)
    other[(8, 0)] = seeds[(8, 0)].roll(3, dims=1)
    assert not torch.equal(other[(8, 0)], seeds[(8, 0)])
    _, _, g3 = DH.grads_of(P, x, y, cfg, True, masks=rec.masks, seeds=other)
    assert not torch.equal(g0["l1.gcn1.linear_weight"], g3["l1.gcn1.linear_weight"])
    # keep_prob 1 and eval mode ignore the seeds
    l1 = DH.restate(P, x, cfg, training=True, keep_prob=1.0, seeds=None)
    l2 = DH.restate(P, x, cfg, training=False, seeds=None)
    assert torch.isfinite(l1).all() and torch.isfinite(l2).all()


@pytest.mark.parametrize("name", NAMES)
def test_seed_pattern_masks_are_non_trivial(name):
    """every mask the fixed seed pattern produces drops something and keeps something; with `c`, unit l7 has 24 frames: its
    block-41 drop leaves frames alive and the block-5 skip drop blanks a strict sub-range of clip 0"""
    cfg = DH.CONFIGS[name]
    seeds = DH.all_drop_seeds(cfg)
    A = hw.DecoupledGCNModel(*DH.model_args(cfg)).l1.A.double()
    assert len(seeds) == 16
    for (unit, site), s in seeds.items():
        if site % 2 == 0:
            mask = DH.spatial_mask(s, A)
        else:
            assert float(s[0].sum()) == 1.0 and float(s[1:].sum()) == 0.0
            mask = DH.temporal_mask(s, DH.TCN_DROP_BLOCK if site == 1 else cfg["block"])
        assert 0 < float(mask.sum()) < mask.numel(), (unit, site)
    if name == "c":
        assert seeds[(7, 1)].shape == (2, 24)
        m41, m5 = DH.temporal_mask(seeds[(7, 1)], 41), DH.temporal_mask(seeds[(7, 3)], 5)
        assert 0 < float(m41[0].sum()) < 24 and 24 - 5 <= float(m5[0].sum()) < 24


def test_single_row_batch_norm_is_refused_like_torch():
    P, cfg = _params("a")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        DH.restate(P, torch.rand(1, 1, 29, 2), cfg, training=True, keep_prob=1.0)
