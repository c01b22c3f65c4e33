"""CPU: the host side of the score ensemble (csrc/ensemble.hip, functional.ens_fuse, ensemble.Ensemble, ensemble.fit_weights)
-- the entry point in the header, the binding and the library, its argument checks before any HIP call, what an Ensemble and
its weight setter refuse, and the weight search on logits whose best grid point is known."""
import ctypes
import importlib
import re

import pytest
import torch
from torch import nn

import modality_helpers as MH

hw = importlib.import_module("sl-hwgat_amd")
ensemble = importlib.import_module("sl-hwgat_amd.ensemble")
HF = hw.functional
CPU = torch.device("cpu")
EINVAL, ESHAPE = -1, -2


def _buf():
    """aligned host memory standing in for a device pointer: never dereferenced, every call below is refused first"""
    keep = (ctypes.c_double * 64)()
    return keep, ctypes.cast(keep, ctypes.c_void_p)


class Scorer(nn.Module):
    """a member that needs no device: a linear score of the flattened clip"""

    def __init__(self, num_classes=5, temporal_dim=None, features=12):
        super().__init__()
        self.num_classes = num_classes
        if temporal_dim is not None:
            self.temporal_dim = temporal_dim
        self.lin = nn.Linear(features, num_classes)

    def forward(self, x):
        return self.lin(x.flatten(1))


# ------------------------------------------------------------------------------------------ header, binding, library
def test_symbol_abi_and_limits_follow_the_header():
    assert "hwgat_ens_fuse" in hw._lib.declared_symbols() and "hwgat_ens_fuse" in hw._lib._SIGS
    assert set(hw._lib._SIGS) == set(hw._lib.declared_symbols())
    L = hw._lib.lib()
    assert L.hwgat_ens_fuse is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    assert int(re.search(r"#define\s+HWGAT_ENS_MAX_MEMBERS\s+(\d+)", src).group(1)) == HF.ENS_MAX_MEMBERS == 8
    assert int(re.search(r"#define\s+HWGAT_ENS_LOGIT\s+(\d+)", src).group(1)) == HF.ENS_MODES.index("logit") == 0
    assert int(re.search(r"#define\s+HWGAT_ENS_PROB\s+(\d+)", src).group(1)) == HF.ENS_MODES.index("prob") == 1
    assert ensemble.MODES == ("logit", "prob") and ensemble.MAX_MEMBERS == 8


def test_entry_point_checks_its_arguments_without_launching():
    fn = hw._lib.lib().hwgat_ens_fuse
    keep, buf = _buf()
    # (z, w, out, M, B, C, mode, stream)
    good = [buf, buf, buf, 4, 3, 7, 1, None]
    for i in range(3):
        assert fn(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i in (4, 5):
        for bad in (0, -1):
            assert fn(*(good[:i] + [bad] + good[i + 1:])) == EINVAL, (i, bad)
    for M in (0, -1, 9, 64):
        assert fn(*(good[:3] + [M] + good[4:])) == ESHAPE, M
    for mode in (-1, 2):
        assert fn(*(good[:6] + [mode] + good[7:])) == ESHAPE, mode
    del keep


def test_wrapper_refuses_what_the_kernel_cannot_take():
    z, w = torch.zeros(3, 4, 5), torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.ens_fuse(z, w, "prob")
    with pytest.raises(ValueError, match="mode"):
        HF.ens_fuse(z, w, "mean")
    with pytest.raises(TypeError, match="fp32"):
        HF.ens_fuse(z.double(), w, "prob")
    with pytest.raises(TypeError, match="fp32"):
        HF.ens_fuse(z, w.double(), "prob")
    with pytest.raises(ValueError, match=r"\(M, B, C\)"):
        HF.ens_fuse(z[0], w, "prob")
    with pytest.raises(ValueError, match="contiguous"):
        HF.ens_fuse(z.transpose(1, 2), w, "prob")
    with pytest.raises(ValueError, match="members"):
        HF.ens_fuse(torch.zeros(9, 4, 5), torch.ones(9), "prob")
    with pytest.raises(ValueError, match="3 weights"):
        HF.ens_fuse(z, torch.ones(4), "prob")
    with pytest.raises(ValueError, match="out must be"):
        HF.ens_fuse(z, w, "prob", out=torch.zeros(4, 6))
    with pytest.raises(ValueError, match="alias"):
        HF.ens_fuse(z, w, "prob", out=z[1])


# ------------------------------------------------------------------------------------------ Ensemble
def test_ensemble_refusals():
    a, b = Scorer(), Scorer()
    with pytest.raises(ValueError, match="members"):
        ensemble.Ensemble([])
    with pytest.raises(ValueError, match="members"):
        ensemble.Ensemble([Scorer() for _ in range(9)])
    with pytest.raises(ValueError, match="twice"):
        ensemble.Ensemble([a, b, a])
    with pytest.raises(ValueError, match="classes"):
        ensemble.Ensemble([a, Scorer(num_classes=6)])
    with pytest.raises(ValueError, match="nn.Module"):
        ensemble.Ensemble([a, lambda x: x])
    with pytest.raises(ValueError, match="mode"):
        ensemble.Ensemble([a, b], mode="mean")
    with pytest.raises(ValueError, match="frames"):
        ensemble.Ensemble([Scorer(temporal_dim=16), Scorer(temporal_dim=32)])
    with pytest.raises(ValueError, match="cannot tell"):
        ensemble.Ensemble([nn.ReLU()])


def test_ensemble_is_evaluation_only_and_freezes_its_members():
    a, b = Scorer(temporal_dim=16), Scorer()
    assert a.training and all(p.requires_grad for p in a.parameters())
    ens = ensemble.Ensemble([a, b])
    assert list(ens.members) == [a, b] and ens.num_classes == 5 and ens.temporal_dim == 16 and ens.mode == "prob"
    assert not ens.training and not a.training and not b.training
    assert not any(p.requires_grad for p in ens.parameters()) and len(list(ens.parameters())) == 4
    with pytest.raises(RuntimeError, match="evaluation-only"):
        ens.train()
    with pytest.raises(RuntimeError, match="evaluation-only"):
        ens.train(True)
    assert ens.eval() is ens and ens.train(False) is ens and not a.training
    assert not hasattr(ensemble.Ensemble([Scorer(), Scorer()]), "temporal_dim")
    # the weights are a registered buffer (address checks see it) that is in no state dict
    assert [n for n, _ in ens.named_buffers()] == ["weight_buffer"] and "weight_buffer" not in ens.state_dict()
    assert ens.weights == [0.5, 0.5] and ens.weight_buffer.tolist() == [0.5, 0.5] and ens.weight_buffer.dtype == torch.float32
    a.train()
    with pytest.raises(RuntimeError, match="member 0"):
        ens(torch.zeros(2, 12))
    # the class count of the models that do not carry `num_classes`
    ds = {"src_len": 16, "num_class": 7}
    for Model, Params in ((hw.STGCNModel, hw.STGCNParams), (hw.TransformerModel, hw.TransformerParams),
                          (hw.DecoupledGCNModel, hw.DecoupledGCNParams), (hw.HGATEModel, hw.HGATEParams)):
        assert ensemble._num_classes(Model(*Params(ds, 2, CPU).get_model_params())) == 7, Model


def test_weight_setter_validates_then_writes_in_place():
    ens = ensemble.Ensemble([Scorer(), Scorer(), Scorer()], weights=[2, 1, 0])
    assert ens.weights == [2.0, 1.0, 0.0]
    addr = ens.weight_buffer.data_ptr()
    for bad, what in (([1, 1], "3 weights"), ([1, 1, 1, 1], "3 weights"), ([1, -0.5, 1], "finite"),
                      ([1, float("nan"), 1], "finite"), ([1, float("inf"), 1], "finite"), ([0, 0, 0], "positive sum"),
                      (1.0, "numbers")):
        with pytest.raises(ValueError, match=what):
            ens.weights = bad
        assert ens.weights == [2.0, 1.0, 0.0] and ens.weight_buffer.tolist() == [2.0, 1.0, 0.0]
    ens.weights = torch.tensor([0.25, 0.5, 0.25])
    assert ens.weights == [0.25, 0.5, 0.25] and ens.weight_buffer.tolist() == [0.25, 0.5, 0.25]
    assert ens.weight_buffer.data_ptr() == addr
    with pytest.raises(ValueError, match="positive sum"):
        ensemble.Ensemble([Scorer()], weights=[0.0])


# ------------------------------------------------------------------------------------------ the weight search
def _one_hot_logits(pred, C, margin):
    z = torch.zeros(len(pred), C)
    z[torch.arange(len(pred)), torch.tensor(pred)] = margin
    return z


@pytest.mark.parametrize("mode", ["logit", "prob"])
def test_fit_weights_finds_the_known_grid_point(mode):
    """two members over 3 classes and 10 clips with labels 0: member 0 votes class 1 with margin 3 on clips 0-3 and is
    right elsewhere with margin 1; member 1 votes class 2 with margin 3 on clips 4-9 and is right elsewhere with margin 1.
    Logit mode: a clip of the first group is right iff w1 > 3 w0, a clip of the second iff w0 > 3 w1.  Prob mode: with
    softmax([0, 3, 0]) = (.045, .909, .045) and softmax([1, 0, 0]) = (.576, .212, .212) the conditions are
    .364 w1 > .864 w0 and .364 w0 > .864 w1, that is w0 < .297 and w0 > .703.  On the grid of step 0.1 both modes give
    (0.8, 0.2) .. (1, 0) the 6 clips of the second group, (0, 1) .. (0.2, 0.8) the 4 of the first and everything between
    neither.  Best: 6 hits, first at (0.8, 0.2)"""
    y = torch.zeros(10, dtype=torch.int64)
    z0 = _one_hot_logits([1] * 4 + [0] * 6, 3, 1.0)
    z0[:4] *= 3.0
    z1 = _one_hot_logits([0] * 4 + [2] * 6, 3, 1.0)
    z1[4:] *= 3.0
    z = torch.stack([z0, z1])
    w = ensemble.fit_weights(z, y, mode, step=0.1)
    assert w == pytest.approx([0.8, 0.2], abs=1e-12)
    hits = lambda w: int((MH.fuse64(z, w, mode).argmax(-1) == y).sum())
    assert hits([0.8, 0.2]) == 6 and hits([0.7, 0.3]) == 0 and hits([0.2, 0.8]) == 4
    # a coarser grid: (0, 1) has 4 hits, (0.5, 0.5) none, (1, 0) six
    assert ensemble.fit_weights(z, y, mode, step=0.5) == [1.0, 0.0]


@pytest.mark.parametrize("mode", ["logit", "prob"])
def test_fit_weights_breaks_ties_lexicographically(mode):
    # identical members: every grid point scores the same, the first in lexicographic order of the weights wins
    z0 = _one_hot_logits([0, 1, 2, 1], 3, 2.0)
    z = torch.stack([z0, z0.clone(), z0.clone()])
    y = torch.tensor([0, 1, 2, 0])
    assert ensemble.fit_weights(z, y, mode, step=0.25) == [0.0, 0.0, 1.0]
    # member 1 alone is right everywhere, member 0 always wrong with a large margin: (0, 1) has every hit and comes first
    right, wrong = _one_hot_logits([0, 1, 2, 0], 3, 1.0), _one_hot_logits([1, 2, 0, 1], 3, 50.0)
    assert ensemble.fit_weights(torch.stack([wrong, right]), y, mode, step=0.1) == [0.0, 1.0]
    assert ensemble.fit_weights(right[None], y, mode) == [1.0]


def test_fit_weights_refusals():
    z, y = torch.zeros(2, 4, 3), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="mode"):
        ensemble.fit_weights(z, y, "mean")
    with pytest.raises(ValueError, match="labels"):
        ensemble.fit_weights(z, y[:3], "prob")
    with pytest.raises(ValueError, match="labels"):
        ensemble.fit_weights(z[0], y, "prob")
    for step in (0.3, 0.0, -0.5, 2.0):
        with pytest.raises(ValueError, match="step"):
            ensemble.fit_weights(z, y, "prob", step=step)
