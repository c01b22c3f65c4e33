"""CPU: the Transformer baseline -- construction and the TransformerParams tuple, the reference's state_dict layout
(tests/golden/transformer_*.npz, make_fixtures_transformer.py), parameter order, every construction-time refusal, the
Transformer_AMD shim as the reference resolves it, and the fp64 restatement of the contract against every fixture."""
import importlib
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import transformer_helpers as TH
from helpers import load_fixture

hw = importlib.import_module("sl-hwgat_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["a", "b", "c"]


def _structure(fx):
    keys, ndim, dims = fx["sd.keys"].tolist(), fx["sd.ndim"].tolist(), fx["sd.dims"].tolist()
    out, at = [], 0
    for k, n, dt in zip(keys, ndim, fx["sd.dtypes"].tolist()):
        out.append((k, tuple(int(d) for d in dims[at:at + n]), dt))
        at += n
    return out


def _standin(fx):
    """an nn.Module with exactly the reference Model's parameters and buffers (names, order, shapes, dtypes)"""
    params = set(fx["sd.params"].tolist())
    root = torch.nn.Module()
    g = torch.Generator().manual_seed(0)
    for key, shape, dt in _structure(fx):
        *path, leaf = key.split(".")
        mod = root
        for part in path:
            if not hasattr(mod, part):
                mod.add_module(part, torch.nn.Module())
            mod = getattr(mod, part)
        if key in params:
            mod.register_parameter(leaf, torch.nn.Parameter(torch.randn(shape, generator=g).to(getattr(torch, dt))))
        else:
            mod.register_buffer(leaf, torch.from_numpy(np.array(fx["sd.buf." + key])))
    return root


def test_params_tuple_and_construction():
    tp = hw.TransformerParams({"src_len": 64, "num_class": 2002}, 2, None)
    assert tp.get_model_params() == (58, 2002, -1, 512, 8, 2048, 3, 0.1, 64, "mean")
    m = hw.TransformerModel(*tp.get_model_params())
    assert m.pool == "mean" and m.d_model == 512 and m.max_len == 64 and len(m.transformer_encoder.layers) == 3
    assert m.deterministic_eval and not m.deterministic_train
    assert m._seed_state.shape == (4,) and m._drop_calls == 0 and not m.device_seed_counter
    tp192 = hw.TransformerParams({"src_len": 192, "num_class": 10}, 3, None)
    assert tp192.get_model_params()[0] == 87 and tp192.get_model_params()[8] == 192


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_matches_reference(name):
    fx = load_fixture(f"transformer_{name}.npz")
    m = hw.TransformerModel(*TH.model_args(TH.CONFIGS[name]))
    sd = m.state_dict()
    assert [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in sd.items()] == _structure(fx)
    assert [n for n, _ in m.named_parameters()] == fx["sd.params"].tolist()
    assert np.array_equal(sd["pos_encoder.pe"].numpy(), fx["sd.buf.pos_encoder.pe"])
    ref = _standin(fx)
    m.load_state_dict(ref.state_dict(), strict=True)
    back = ref.load_state_dict(m.state_dict(), strict=True)
    assert not back.missing_keys and not back.unexpected_keys
    for (k, v), (k2, v2) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(v, v2)


def test_parameters_order_and_init():
    torch.manual_seed(0)
    m = hw.TransformerModel(87, 6, -1, 128, 2, 256, 2, 0.1, 37, "max")
    shapes = [(n, tuple(p.shape)) for n, p in m.named_parameters()]
    assert shapes[0] == ("encoder.weight", (128, 87)) and shapes[-1] == ("classifier.bias", (6,))
    assert shapes[2] == ("transformer_encoder.layers.0.self_attn.in_proj_weight", (384, 128))
    ipb = dict(m.named_parameters())["transformer_encoder.layers.0.self_attn.in_proj_bias"]
    assert float(ipb.detach().abs().max()) == 0.0                     # nn.MultiheadAttention's own init
    w = dict(m.named_parameters())["transformer_encoder.layers.0.linear1.weight"]
    bound = (6.0 / (128 + 256)) ** 0.5                      # xavier_uniform
    w = w.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound


@pytest.mark.parametrize("args,rule", [
    ((58, 10, -1, 512, 4, 2048, 3, 0.1, 64, "mean"), "head_dim"),
    ((58, 10, -1, 512, 16, 2048, 3, 0.1, 64, "mean"), "head_dim"),
    ((58, 10, -1, 96, 1, 2048, 3, 0.1, 64, "mean"), "multiples of 64 up to 1024"),
    ((58, 10, -1, 1088, 17, 2048, 3, 0.1, 64, "mean"), "multiples of 64 up to 1024"),
    ((58, 10, -1, 512, 8, 1000, 3, 0.1, 64, "mean"), "dim_feedforward"),
    ((58, 10, -1, 512, 8, 2048, 3, 0.1, 513, "mean"), "max_len"),
    ((58, 10, -1, 512, 8, 2048, 3, 0.1, 64, "sum"), "pool"),
    ((58, 10, -1, 64, 1, 64, 64, 0.1, 64, "mean"), "num_encoder_layers"),
])
def test_refusals_name_the_rule(args, rule):
    with pytest.raises(NotImplementedError, match=rule):
        hw.TransformerModel(*args)


def test_forward_refusals():
    m = hw.TransformerModel(6, 3, -1, 64, 1, 64, 1, 0.1, 8, "concat")
    with pytest.raises(ValueError, match="max_len"):
        m(torch.zeros(1, 9, 3, 2))
    with pytest.raises(ValueError, match="features per frame"):
        m(torch.zeros(1, 8, 4, 2))
    with pytest.raises(ValueError, match="concat"):
        m(torch.zeros(1, 7, 3, 2))


def test_integration_shim_resolves_like_the_reference(tmp_path, monkeypatch):
    pkg = tmp_path / "hwgat" / "models"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    shims = os.path.join(ROOT, "integration", "models")
    for f in ("Transformer_AMD.py", "model_params_amd.py"):
        shutil.copy(os.path.join(shims, f), pkg / f)
    # the one-line edit INTEGRATION.md asks for, on a stand-in for the reference's model_params.py
    (pkg / "model_params.py").write_text("class TransformerParams:\n    pass\n\n\nfrom models.model_params_amd import *\n")
    monkeypatch.setenv("HWGAT_AMD_ROOT", ROOT)
    monkeypatch.syspath_prepend(str(tmp_path / "hwgat"))
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
        monkeypatch.delitem(sys.modules, k)
    try:
        module = importlib.import_module("models.model_params")                                   # configs.py:80
        params = getattr(module, "Transformer_AMD" + "Params")({"src_len": 64, "num_class": 20}, 2,
                                                               torch.device("cpu"))              # configs.py:81-82
        model = getattr(importlib.import_module("models.Transformer_AMD"), "Model")(*params.get_model_params())   # utils.py:55-59
    finally:
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            sys.modules.pop(k, None)
    assert type(model) is hw.TransformerModel and model.max_len == 64 and model.input_dim == 58


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_fixture(name):
    fx = load_fixture(f"transformer_{name}.npz")
    cfg = TH.CONFIGS[name]
    m = hw.TransformerModel(*TH.model_args(cfg))
    w = TH.recipe_weights(m.state_dict(), cfg["seed"])
    x = torch.from_numpy(fx["x"])
    layers = []
    out = TH.restate(w, x, cfg, per_layer=layers)
    ref = torch.from_numpy(fx["logits"]).double()
    assert ((out - ref).abs().max() / ref.abs().max()).item() < 2e-5
    for i, h in enumerate(layers):
        r = torch.from_numpy(fx[f"layer{i}"]).double()
        assert ((h[:, ::8] - r).abs().max() / r.abs().max()).item() < 2e-5
