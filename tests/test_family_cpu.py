"""CPU: the four graph-attention models (HWGATE, HGATE, WGATE, GATE) stand on one base class (models/_family.py).
What must survive that: the reference classes' `state_dict` key order, shapes and dtypes and their `named_parameters`
order and flags (tests/golden/family_state.npz, from tests/golden/make_fixtures_family.py), every field that
`DeviceSeeds._init_device_seeds` owns on every model of the package, and a construction that is a function of torch's seed
alone."""
import importlib

import pytest
import torch
from torch import nn

from helpers import load_fixture

hw = importlib.import_module("sl-hwgat_amd")
seeding = importlib.import_module("sl-hwgat_amd.seeding")
CPU = torch.device("cpu")
FAMILY = {"hwgate": (hw.Model, hw.HWGATEParams), "hgate": (hw.HGATEModel, hw.HGATEParams),
          "wgate": (hw.WGATEModel, hw.WGATEParams), "gate": (hw.GATEModel, hw.GATEParams)}
BASELINES = {"transformer": (hw.TransformerModel, hw.TransformerParams), "stgcn": (hw.STGCNModel, hw.STGCNParams),
             "dgcn": (hw.DecoupledGCNModel, hw.DecoupledGCNParams)}


def build(name):
    Model, Params = {**FAMILY, **BASELINES}[name]
    hp = Params({"src_len": 32, "num_class": 7}, 2, CPU)
    if name in FAMILY:
        hp.embed_dim = 128
    return Model(*hp.get_model_params())


@pytest.fixture(scope="module")
def reference_structure():
    return load_fixture("family_state.npz")


@pytest.mark.parametrize("name", list(FAMILY))
def test_state_dict_and_parameters_match_the_reference_class(name, reference_structure):
    fx = reference_structure
    model = build(name)
    state = model.state_dict()
    assert list(state) == [str(k) for k in fx[name + ".state.keys"]]
    assert [",".join(str(d) for d in v.shape) for v in state.values()] == [str(s) for s in fx[name + ".state.shapes"]]
    assert [str(v.dtype) for v in state.values()] == [str(s) for s in fx[name + ".state.dtypes"]]
    params = list(model.named_parameters())
    assert [k for k, _ in params] == [str(k) for k in fx[name + ".param.names"]]
    assert [bool(p.requires_grad) for _, p in params] == [bool(f) for f in fx[name + ".param.requires_grad"]]


def test_reference_structure_has_the_recorded_sizes(reference_structure):
    """the reference classes at this configuration have 106 / 106 / 103 / 105 state_dict keys"""
    assert [len(reference_structure[n + ".state.keys"]) for n in FAMILY] == [106, 106, 103, 105]


def _seed_fields():
    """every attribute `_init_device_seeds` sets, derived by calling it on a bare DeviceSeeds module"""
    class Bare(seeding.DeviceSeeds, nn.Module):
        pass
    bare = Bare()
    before = set(vars(bare))
    buffers = set(bare._buffers)
    bare._init_device_seeds()
    return (set(vars(bare)) - before), (set(bare._buffers) - buffers)


@pytest.mark.parametrize("name", list(FAMILY) + list(BASELINES))
def test_every_model_has_every_seed_field_on_the_instance(name):
    attrs, buffers = _seed_fields()
    assert {"_drop_calls", "device_seed_counter", "_call_base", "deterministic_eval", "deterministic_train"} <= attrs
    assert buffers == {"_seed_state"}
    model = build(name)
    assert attrs <= set(vars(model)), sorted(attrs - set(vars(model)))
    assert buffers <= set(model._buffers)
    assert not model.deterministic_train and model.deterministic_eval and model._drop_calls == 0


def test_no_class_level_fallback_for_instance_fields():
    attrs, _ = _seed_fields()
    for cls in [seeding.DeviceSeeds] + [m for m, _ in FAMILY.values()]:
        for klass in cls.__mro__:
            if klass.__module__.startswith("sl-hwgat_amd"):
                assert not (attrs | {"attn_drop_rate"}) & set(vars(klass)), klass


@pytest.mark.parametrize("name", list(FAMILY))
def test_construction_depends_on_the_seed_alone(name):
    states = []
    for _ in range(2):
        torch.manual_seed(5)
        states.append(build(name).state_dict())
    assert list(states[0]) == list(states[1])
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
    torch.manual_seed(6)
    other = build(name).state_dict()
    assert not torch.equal(states[0]["B"], other["B"])


@pytest.mark.parametrize("name", list(FAMILY))
def test_models_share_the_base_and_leave_nn_module_init_to_it(name):
    family = importlib.import_module("sl-hwgat_amd.models._family")
    Model = FAMILY[name][0]
    assert Model.__bases__ == (family.FamilyModel,)
    assert family.FamilyModel.__bases__ == (seeding.DeviceSeeds, nn.Module)
