"""CPU: the ST-GCN baseline -- the STGCNParams tuple and construction, the adjacency and the reference's state_dict layout
(tests/golden/stgcn_*.npz, make_fixtures_stgcn.py), every construction-time refusal, the STGCN_AMD shim as the reference
resolves it, header <-> bindings <-> exports of the new entry points, and the fp64 restatement of the contract against
every fixture (with the floor rule for the analytically zero biases and the ReLU-mask round trip)."""
import importlib
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import stgcn_helpers as SH
from helpers import load_fixture, grad_digest_check, reference_structure, reference_standin

hw = importlib.import_module("sl-hwgat_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["a", "b", "c", "d"]
NEW_SYMBOLS = {"hwgat_stgcn_weight_prep", "hwgat_stgcn_conv", "hwgat_stgcn_conv_dw_bytes", "hwgat_stgcn_conv_dw",
               "hwgat_stgcn_red_bytes", "hwgat_stgcn_colsum", "hwgat_stgcn_bn_stats", "hwgat_stgcn_bn_eval_stats",
               "hwgat_stgcn_bn_apply", "hwgat_stgcn_bn_bwd", "hwgat_stgcn_agg_fwd", "hwgat_stgcn_agg_bwd_bytes",
               "hwgat_stgcn_agg_bwd", "hwgat_stgcn_pool_fwd", "hwgat_stgcn_pool_bwd", "hwgat_stgcn_copy_cols"}


def test_params_tuple_and_construction():
    sp = hw.STGCNParams({"src_len": 128, "num_class": 2002}, 2, None)
    args = sp.get_model_params()
    assert args[:3] == (2, 29, 0) and args[4:] == (True, 256, 2002, 0.05, False)
    assert len(args[3]) == 34 and args[3] == SH.EDGES_29
    m = hw.STGCNModel(*args)
    assert len(m.st_gcn_networks) == 10 and len(m.edge_importance) == 10 and m.A.shape == (3, 29, 29)
    assert [b.stride for b in m.st_gcn_networks] == SH.STRIDES
    assert [(b.in_channels, b.out_channels) for b in m.st_gcn_networks] == [(ci, co) for ci, co, _, _ in
                                                                           SH.block_plan(SH.CONFIGS["a"])]
    assert m.deterministic_eval and m._seed_state.shape == (4,) and m._drop_calls == 0
    assert m.frames_out(128) == 32 and m.frames_out(13) == 4 and m.frames_out(1) == 1
    w = m.head.classifier.weight.detach()
    assert abs(float(w.std()) - (2.0 / 2002) ** 0.5) < 0.05 * (2.0 / 2002) ** 0.5          # normal(0, sqrt(2 / n_classes))
    assert all(float(e.detach().min()) == 1.0 == float(e.detach().max()) for e in m.edge_importance)
    assert m.set_activation_dtype(torch.float32) is m
    with pytest.raises(NotImplementedError, match="fp32 only"):
        m.set_activation_dtype(torch.bfloat16)


@pytest.mark.parametrize("name", NAMES)
def test_adjacency_and_state_dict_match_reference(name):
    fx = load_fixture(f"stgcn_{name}.npz")
    m = hw.STGCNModel(*SH.model_args(SH.CONFIGS[name]))
    assert np.array_equal(m.A.numpy(), fx["A"]) and m.A.dtype == torch.float32            # bit for bit
    sd = m.state_dict()
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [t[:3] for t in reference_structure(fx, "sd")]
    assert [n for n, _ in m.named_parameters()] == fx["sd.params"].tolist()
    assert sd["data_bn.num_batches_tracked"].dtype == torch.int64
    ref = reference_standin(fx, "sd")
    m.load_state_dict(ref.state_dict(), strict=True)
    back = ref.load_state_dict(m.state_dict(), strict=True)
    assert not back.missing_keys and not back.unexpected_keys
    for (k, v), (k2, v2) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)
    # an AdamW state built on either side loads on the other
    o_ref = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    for p in ref.parameters():
        p.grad = torch.ones_like(p)
    o_ref.step()
    o_mine = torch.optim.AdamW(m.parameters(), lr=1e-3)
    o_mine.load_state_dict(o_ref.state_dict())
    o_ref.load_state_dict(o_mine.state_dict())


def test_other_graphs_match_an_independent_construction():
    """a 17-joint graph with an off-centre root, isolated joints included: column-normalised adjacency, three partitions"""
    edges = [[0, 1], [1, 2], [4, 5], [4, 6], [6, 7], [2, 4], [9, 10]]
    A = hw.STGCNModel(3, 17, 4, edges, False, 128, 7, 0.05, False).A.double()
    link = torch.eye(17, dtype=torch.float64)
    for i, j in edges:
        link[i, j] = link[j, i] = 1
    assert torch.allclose(A.sum(0), link / link.sum(0), atol=1e-7)                  # the partitions tile D^-1-scaled links
    assert torch.equal(A[0], torch.diag(torch.diag(A[0]))) and float(A[1].diagonal().abs().max()) == 0.0
    assert ((A[1] != 0) & (A[2] != 0)).sum() == 0


@pytest.mark.parametrize("args,rule", [
    ((2, 29, 0, SH.EDGES_29, True, 256, 10, 0.05, True), "batch_norm=True"),
    ((0, 29, 0, SH.EDGES_29, True, 256, 10, 0.05, False), "in_channels"),
    ((5, 29, 0, SH.EDGES_29, True, 256, 10, 0.05, False), "in_channels"),
    ((2, 33, 0, [], True, 256, 10, 0.05, False), "num_nodes"),
    ((2, 29, 0, SH.EDGES_29, True, 96, 10, 0.05, False), "multiples of 64 up to 1024"),
    ((2, 29, 0, SH.EDGES_29, True, 1088, 10, 0.05, False), "multiples of 64 up to 1024"),
    ((2, 29, 29, SH.EDGES_29, True, 256, 10, 0.05, False), "center"),
    ((2, 20, 0, SH.EDGES_29, True, 256, 10, 0.05, False), "edge"),
])
def test_refusals_name_the_rule(args, rule):
    with pytest.raises(NotImplementedError, match=rule):
        hw.STGCNModel(*args)


@pytest.mark.parametrize("ratio", [1.0, -0.1, 1.5])
def test_dropout_ratio_outside_the_unit_interval_is_refused(ratio):
    with pytest.raises(ValueError, match="dropout_ratio"):
        hw.STGCNModel(2, 29, 0, SH.EDGES_29, True, 256, 10, ratio, False)


def test_checkpoint_files_interchange_with_the_reference_layout(tmp_path):
    """checkpoint.save_checkpoint writes the reference's dict layout with the reference's state_dict keys (running
    statistics and num_batches_tracked included); a file written from a reference-shaped model and its AdamW resumes here"""
    ck = importlib.import_module("sl-hwgat_amd.checkpoint")
    fx = load_fixture("stgcn_b.npz")
    cfg = SH.CONFIGS["b"]
    ref, mine = reference_standin(fx, "sd"), hw.STGCNModel(*SH.model_args(cfg))
    mine.load_state_dict(SH.recipe_weights(mine.state_dict(), 5), strict=False)
    opt = ck.get_optimizer(mine)
    sch = ck.get_scheduler(opt)
    for p in mine.parameters():
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    sch.step()
    path = str(tmp_path / "mine.pt")
    ck.save_checkpoint(path, mine, opt, sch, [0.1], [2.0], [0.2], [1.9], 6, 4.5e-4)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert list(raw["model_state_dict"]) == list(ref.state_dict())
    rep = {}
    ck.load_weights_from_pretrained(ref, path, "cpu", rep)
    assert rep == {"unknown": [], "mismatched": [], "missing": []}
    assert all(torch.equal(v, mine.state_dict()[k]) for k, v in ref.state_dict().items())
    opt_r = torch.optim.AdamW(ref.parameters(), lr=5e-4)
    opt_r.load_state_dict(raw["optimizer_state_dict"])
    # the other way round: reference-shaped model + optimizer state -> file -> this backend
    sch_r = torch.optim.lr_scheduler.CosineAnnealingLR(opt_r, T_max=20, last_epoch=-1)
    for p in ref.parameters():
        p.grad = torch.full_like(p, -2e-3)
    opt_r.step()
    sch_r.step()
    path2 = str(tmp_path / "ref.pt")
    torch.save({"model_state_dict": ref.state_dict(), "optimizer_state_dict": opt_r.state_dict(), "train_loss_list": [1.0],
                "val_loss_list": [1.1], "train_acc_list": [0.1], "val_acc_list": [0.2], "epoch": 1,
                "learning_rate": sch_r.get_last_lr()[0], "scheduler": sch_r.state_dict()}, path2)
    other = hw.STGCNModel(*SH.model_args(cfg))
    o2 = ck.get_optimizer(other)
    other, o2, s2, lists, start = ck.load_checkpoint(path2, other, o2, ck.get_scheduler(o2))
    assert start == 2
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in other.state_dict().items())
    st_r, st_m = opt_r.state_dict()["state"], o2.state_dict()["state"]
    assert set(st_r) == set(st_m) and all(torch.equal(st_r[i]["exp_avg"], st_m[i]["exp_avg"]) for i in st_r)


def test_accepted_corners_and_forward_refusals():
    for c in (1, 4):
        hw.STGCNModel(c, 32, 0, [[0, 1]], False, 1024, 3, 0.0, False)
    m = hw.STGCNModel(2, 29, 0, SH.EDGES_29, True, 64, 3, 0.05, False)
    with pytest.raises(ValueError, match=r"expected \(N, T, 29, 2\)"):
        m(torch.zeros(1, 8, 29, 3))
    with pytest.raises(ValueError, match=r"expected \(N, T, 29, 2\)"):
        m(torch.zeros(1, 8, 28, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a CPU tensor never falls back to torch arithmetic
        m(torch.zeros(2, 8, 29, 2))


def test_integration_shim_resolves_like_the_reference(tmp_path, monkeypatch):
    pkg = tmp_path / "hwgat" / "models"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    shims = os.path.join(ROOT, "integration", "models")
    for f in ("STGCN_AMD.py", "model_params_amd.py"):
        shutil.copy(os.path.join(shims, f), pkg / f)
    (pkg / "model_params.py").write_text("class STGCNParams:\n    pass\n\n\nfrom models.model_params_amd import *\n")
    monkeypatch.setenv("HWGAT_AMD_ROOT", ROOT)
    monkeypatch.syspath_prepend(str(tmp_path / "hwgat"))
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        monkeypatch.delitem(sys.modules, k)
    try:
        module = importlib.import_module("models.model_params")                                   # configs.py:80
        params = getattr(module, "STGCN_AMD" + "Params")({"src_len": 64, "num_class": 20}, 3, torch.device("cpu"))
        model = getattr(importlib.import_module("models.STGCN_AMD"), "Model")(*params.get_model_params())   # utils.py:55-59
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            sys.modules.pop(k, None)
    assert type(model) is hw.STGCNModel and model.in_channels == 3 and model.head.classifier.out_features == 20


def test_new_entry_points_declared_bound_and_exported():
    assert NEW_SYMBOLS <= set(hw._lib.declared_symbols())
    assert NEW_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_stgcn_")}
    handle = hw._lib.lib()
    for n in NEW_SYMBOLS:
        assert getattr(handle, n) is not None
    # argument checks that need no device: null pointers and unsupported shapes are refused before any launch
    assert handle.hwgat_stgcn_conv(None, None, None, None, None, None, 1, 4, 4, 29, 64, 64, 9, 1, 4, 0, None) == -1
    assert handle.hwgat_stgcn_bn_stats(None, 8, 64, 1e-5, 0.1, None, None, None, None, None, None, 0, None) == -1
    assert handle.hwgat_stgcn_conv_dw_bytes(928, 48, 64, 9) == -1 and handle.hwgat_stgcn_conv_dw_bytes(928, 64, 64, 9) > 0
    assert handle.hwgat_stgcn_red_bytes(64) == (256 * 2 * 64 + 2 * 64) * 4
    assert handle.hwgat_stgcn_agg_bwd_bytes(32) == 32 * 3 * 32 * 32 * 4


def _params(name):
    cfg = SH.CONFIGS[name]
    m = hw.STGCNModel(*SH.model_args(cfg))
    w = SH.fixture_weights(m.state_dict(), cfg)
    return dict(w, A=m.A.clone()), cfg


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_fixture(name, training):
    fx = load_fixture(f"stgcn_{name}.npz")
    P, cfg = _params(name)
    x, y = SH.fixture_input(fx, cfg)
    tag = "train." if training else "eval."
    rec = SH.Record()
    logits, loss, grads = SH.grads_of(P, x, y, cfg, training, rec=rec)
    ref = torch.from_numpy(fx[tag + "logits"]).double()
    assert ((logits - ref).norm() / ref.norm()).item() < 1e-6
    assert abs(loss.item() - float(fx[tag + "loss"])) < max(1e-6, 4 * float(fx[f"refdev.{tag}loss"])) * max(1.0, abs(loss.item()))
    assert rec.margin >= float(fx["margin"]) * (1 - 1e-3)          # the fixture's margin is the smaller of both modes
    if training:
        for i, h in enumerate(rec.blocks):
            r = torch.from_numpy(fx[f"train.block{i}"]).double()
            # the fixture holds the fp32 reference: its own distance to fp64 (refdev) sets the bound
            assert ((SH.block_samples(h) - r).norm() / r.norm()).item() < max(1e-6, 4 * float(fx[f"refdev.train.block{i}"])), i
        for k, v in rec.stats.items():
            r = torch.from_numpy(np.asarray(fx["train.stat." + k]))
            if not v.is_floating_point():
                assert (v == r).all(), k
            else:
                assert ((v - r).norm() / r.norm()).item() < max(1e-6, 4 * float(fx["refdev.train.stat." + k])), k
    if not cfg["tight"]:
        return
    assert float(fx["margin"]) >= 2e-6
    zero = SH.zero_grad_biases(grads) if training else {}
    for n, g in grads.items():
        dev = float(fx[f"refdev.{tag}g.{n}"])
        assert dev < 2e-5, (n, dev)
        tol = max(2e-5, 4.0 * dev)
        if n in zero:
            # floor rule: in fp64 these gradients vanish against the matching weight gradient
            assert g.norm().item() < 1e-12 * grads[zero[n]].norm().item(), n
            continue
        grad_digest_check({n: g}, fx, tag, tol)


def test_restatement_relu_masks_round_trip():
    """the restatement with its own ReLU masks fed back returns the same gradients, and a flipped mask entry changes them"""
    P, cfg = _params("b")
    x, y = SH.make_input(cfg, seed=1)
    rec = SH.Record()
    _, _, g0 = SH.grads_of(P, x, y, cfg, True, rec=rec)
    assert len(rec.masks) == 20
    _, _, g1 = SH.grads_of(P, x, y, cfg, True, masks=rec.masks)
    assert all(torch.equal(g0[n], g1[n]) for n in g0)
    flipped = {k: v.clone() for k, v in rec.masks.items()}
    site = "st_gcn_networks.5.relu"
    flipped[site][0, 0, 0, :8] = ~flipped[site][0, 0, 0, :8]
    _, _, g2 = SH.grads_of(P, x, y, cfg, True, masks=flipped)
    assert not torch.equal(g0["st_gcn_networks.0.gcn.conv.weight"], g2["st_gcn_networks.0.gcn.conv.weight"])


def test_single_row_batch_norm_is_refused_like_torch():
    P, cfg = _params("a")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        SH.restate(P, torch.rand(1, 1, 29, 2), cfg, training=True)
