#!/usr/bin/env python3
"""Golden attention maps of a tiny HWGATE, hooked out of the REFERENCE (development container only).

Run:  python tests/golden/make_fixtures_attn.py        (needs the reference checkout make_fixtures.py imports from)

Imports the reference's `hwgat/models/HWGATE.py` as-is (same `timm.trunc_normal_` alias as make_fixtures.py), loads
`oracle.hwgat_oracle.synth_params` and registers a forward hook on every `blk.attn.softmax` of the model in eval():
in eval mode that module runs exactly once per block (`attn = self.softmax(attn)`, HWGATE.py:111 -- the second call,
HWGATE.py:97, is train mode only), so the hook output IS the probability tensor P of the block, (B f nW, nH, 32, 32).

  attn_maps_hwgate.npz   B 2, T 8, K 32 (two 16-joint windows), C 2, embed_dim 64, depths (2, 2), heads (2, 2):
                         head_dim 32 (stage 0, F 8) and 64 (stage 1, F 4); blocks 1 and 3 are shifted.  Holds the input,
                         the adjacency, the eval logits and `prob{k}` of the four blocks.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import hwgat_oracle as O  # noqa: E402
from make_fixtures import import_reference  # noqa: E402

CFG = dict(B=2, T=8, K=32, C=2, d0=64, depths=(2, 2), heads=(2, 2), nc=5, seed=41)


def main():
    Model, HWGATEParams, _ = import_reference()
    c = CFG
    hp = HWGATEParams({"src_len": c["T"], "num_class": c["nc"]}, c["C"], torch.device("cpu"))
    hp.num_kps, hp.embed_dim = c["K"], c["d0"]
    hp.depths, hp.num_heads = list(c["depths"]), list(c["heads"])
    hp.drop_rate = 0.0
    hp.edges = [hp.edges[0]] * (c["K"] // 16)
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    torch.manual_seed(1004)
    model = Model(*hp.get_model_params())
    cfg = dict(kp_dim=c["C"], temporal_dim=c["T"], num_classes=c["nc"], embed_dim=c["d0"], depths=tuple(hp.depths),
               ff_ratio=hp.ff_ratio, use_pe=hp.pe, num_kps=c["K"], tp=hp.temporal_patch_size)
    res = model.load_state_dict(O.synth_params(c["seed"], weight_std=0.08, **cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith("attn_mask") for k in res.missing_keys), res
    model.eval()
    x = torch.rand(c["B"], c["T"], c["K"], c["C"], generator=torch.Generator().manual_seed(43))
    seen = []
    hooks = [blk.attn.softmax.register_forward_hook(lambda m, i, out: seen.append(out.detach().clone()))
             for stage in model.layers for blk in stage.blocks]
    with torch.no_grad():
        logits = model(x)
    for h in hooks:
        h.remove()
    assert len(seen) == sum(c["depths"]), len(seen)            # one softmax call per block in eval mode
    fx = {"x": x.numpy(), "adj": hp.adj_mat.numpy(), "eval.logits": logits.numpy(),
          "cfg": np.array([c["T"], c["K"], c["C"], c["d0"], c["nc"], c["B"], c["seed"]]),
          "depths": np.array(c["depths"]), "heads": np.array(c["heads"])}
    for k, p in enumerate(seen):
        assert torch.allclose(p.sum(-1), torch.ones(()), atol=1e-5)
        fx[f"prob{k}"] = p.numpy()
    path = os.path.join(HERE, "attn_maps_hwgate.npz")
    np.savez_compressed(path, **fx)
    print("attn_maps_hwgate", os.path.getsize(path) // 1024, "KiB", [tuple(p.shape) for p in seen])


if __name__ == "__main__":
    main()
