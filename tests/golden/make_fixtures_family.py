#!/usr/bin/env python3
"""state_dict / parameter STRUCTURE of the four graph-attention models, from the REFERENCE (development container only).

Run:  python tests/golden/make_fixtures_family.py        (needs /root/reference)

Instantiates the reference's `HWGATE.py`, `HGATE.py`, `WGATE.py` and `GATE.py` classes as they are (same
`timm.trunc_normal_` alias as make_fixtures_hgate.py), each from its `*Params({"src_len": 32, "num_class": 7}, 2, cpu)`
with `embed_dim = 128`, and stores names, shapes, dtypes and flags only -- no weights:

  family_state.npz   per model <m> in (hwgate, hgate, wgate, gate):
      <m>.state.keys / .shapes / .dtypes     list(state_dict()) in order, "a,b,c" shapes, torch dtype names
      <m>.param.names / .requires_grad       named_parameters() in order
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/hwgat"
DATASET, KP_DIM, EMBED_DIM = {"src_len": 32, "num_class": 7}, 2, 128


def import_reference():
    for name in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["timm.models.layers"].trunc_normal_ = torch.nn.init.trunc_normal_
    sys.path.insert(0, REF)
    import importlib
    params = importlib.import_module("models.model_params")
    return {name.lower(): (importlib.import_module("models." + name).Model, getattr(params, name + "Params"))
            for name in ("HWGATE", "HGATE", "WGATE", "GATE")}


def main():
    fx = {}
    for name, (Model, Params) in import_reference().items():
        hp = Params(dict(DATASET), KP_DIM, torch.device("cpu"))
        hp.embed_dim = EMBED_DIM
        model = Model(*hp.get_model_params())
        state = model.state_dict()
        fx[name + ".state.keys"] = np.array(list(state))
        fx[name + ".state.shapes"] = np.array([",".join(str(d) for d in v.shape) for v in state.values()])
        fx[name + ".state.dtypes"] = np.array([str(v.dtype) for v in state.values()])
        fx[name + ".param.names"] = np.array([k for k, _ in model.named_parameters()])
        fx[name + ".param.requires_grad"] = np.array([bool(p.requires_grad) for _, p in model.named_parameters()])
        print(name, len(state), "state_dict keys,", len(fx[name + ".param.names"]), "parameters")
    path = os.path.join(HERE, "family_state.npz")
    np.savez_compressed(path, **fx)
    print("family_state.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
