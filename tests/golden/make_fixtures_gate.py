#!/usr/bin/env python3
"""Golden vectors for the GATE model and for WGATE with window sizes other than 16, from the REFERENCE
(development container only).

Run:  python tests/golden/make_fixtures_gate.py        (needs /root/reference)

Imports `/root/reference/hwgat/models/GATE.py` and `WGATE.py` as they are (same `timm.trunc_normal_` alias as
make_fixtures.py: init only, overwritten before anything is recorded), loads the deterministic
`tests/gate_helpers.synth_params` set (pool weights O(1 / (T K)), non-uniform, non-zero pool bias), runs seeded inputs
and stores inputs + outputs (data only).

  gate_a.npz     T=32, K=29, B=4, C=2, d=128, 8 heads (head_dim 16), 8 blocks, pe on; 3712 tokens = whole tiles: the
                 backend's fused-linear path.  Default GATEParams graph.
  gate_b.npz     T=5, K=29, B=3, C=3, d=128, 4 heads (head_dim 32), 2 blocks, pe off; ragged token count
  wgate_w32.npz  WGATE, W=32, K=64 (2 windows), T=8, B=2, C=2, 8 heads, 2 blocks; random 32-slot edge lists
  wgate_w8.npz   WGATE, W=8, K=32 (4 windows), T=6, B=3, C=3, 4 heads (head_dim 32), 2 blocks; random 8-slot edge lists

For every recorded input the generator ASSERTS on the reference's own softmax output (a forward hook on its nn.Softmax)
that every probability outside the adjacency is exactly 0: the band form of the kernels hides nothing.
With drop_rate 0 train() == eval() for both models.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/hwgat"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import gate_helpers as GH  # noqa: E402
from make_fixtures import grad_digest  # noqa: E402


def import_reference():
    for name in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["timm.models.layers"].trunc_normal_ = torch.nn.init.trunc_normal_
    sys.path.insert(0, REF)
    from models.GATE import Model as GATE                # noqa
    from models.WGATE import Model as WGATE              # noqa
    from models.model_params import GATEParams, WGATEParams   # noqa
    from losses.SmoothCrossEntropy import SmoothedCrossEntropyLoss  # noqa
    return GATE, WGATE, GATEParams, WGATEParams, SmoothedCrossEntropyLoss


def sub(t):
    return t[:, ::3, ::5, ::11].contiguous().numpy()


def frame_blocks(adj, T, W):
    """(nW, 3, W, W) uint8: the blocks towards frame f-1, f, f+1 of query frame 1 -- and a check that the whole matrix is
    exactly the block-tridiagonal repetition of them"""
    a = adj if adj.dim() == 3 else adj.unsqueeze(0)
    nW = a.shape[0]
    v = a.view(nW, T, W, T, W)
    blocks = torch.stack([v[:, 1, :, 0, :], v[:, 1, :, 1, :], v[:, 1, :, 2, :]], dim=1)
    assert torch.equal(GH.band_adjacency(blocks[:, 1], blocks[:, 0], blocks[:, 2], T), a)
    return blocks.numpy().astype(np.uint8)


def record(model, kind, adj, W, x, y, crit, cfg_row):
    T, K = x.shape[1], x.shape[2]
    fx = {"x": x.numpy(), "y": y.numpy(), "cfg": np.array(cfg_row), "kind": np.array(kind),
          "adj_blocks": frame_blocks(adj, T, W),
          "state.keys": np.array(list(model.state_dict().keys())),
          "state.shapes": np.array([",".join(str(d) for d in v.shape) for v in model.state_dict().values()]),
          "adj_mask_head": model.state_dict()["adj_mask"].reshape(-1, T * W, T * W)[0, :2 * W, :2 * W].numpy()}
    a = adj if adj.dim() == 3 else adj.unsqueeze(0)
    outside = (a == 0)                                     # (nW, T W, T W)
    worst = {"p": 0.0, "n": 0, "vis_min": 10 ** 9, "vis_max": 0}

    def check_softmax(_m, _i, out):                        # the reference's own probabilities
        p = out.detach().view(-1, a.shape[0], *out.shape[1:])          # (B, nW, nH, T W, T W)
        worst["p"] = max(worst["p"], float((p * outside[None, :, None]).max()))
        worst["n"] += 1
    vis = a.sum(-1)
    worst["vis_min"], worst["vis_max"] = int(vis.min()), int(vis.max())
    taps = {}

    def hook(name):
        def fn(_m, _i, out):
            taps[name] = out.detach().reshape(x.shape[0], T, K, -1)
        return fn
    handles = []
    for i, layer in enumerate(model.layers):
        handles.append(layer.register_forward_hook(hook(f"block{i}")))
        handles.append(layer.attn.softmax.register_forward_hook(check_softmax))
    model.eval()
    with torch.no_grad():
        fx["eval.logits"] = model(x).numpy()
        fx["eval.feat"] = model.forward_features(x).numpy()
    for k, v in taps.items():
        fx["eval." + k] = sub(v)
    last = f"block{len(model.layers) - 1}"
    fx["eval.block0.full"] = taps["block0"][0, :2].numpy()        # first / last frames: the clipped band edge
    fx["eval.block0.tail"] = taps["block0"][0, -2:].numpy()
    fx["eval.last.full"] = taps[last][-1, :2].numpy()
    fx["eval.last.tail"] = taps[last][-1, -2:].numpy()
    model.zero_grad()
    loss = crit(model(x), y)
    loss.backward()
    fx["evalbwd.loss"] = np.array(loss.item())
    fx.update({"evalbwd." + k: v for k, v in grad_digest(model).items()})
    for h in handles:
        h.remove()
    assert worst["n"] >= 3 * len(model.layers) and worst["p"] == 0.0, worst   # band == dense, exactly
    print(kind, cfg_row, "largest probability outside the adjacency:", worst["p"], "visible keys per row:",
          worst["vis_min"], "-", worst["vis_max"])
    return fx


def load_synth(model, cfg, seed):
    synth = GH.synth_params(seed, **cfg)
    res = model.load_state_dict(synth, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert res.missing_keys == ["adj_mask"], res.missing_keys


def gate_case(GATE, GATEParams, crit, g, *, T, C, d0, nc, B, heads, depths, pe, seed):
    hp = GATEParams({"src_len": T, "num_class": nc}, C, torch.device("cpu"))
    defaults = {"hp." + k: np.array(getattr(hp, k)) for k in
                ("kp_dim", "num_kps", "temporal_dim", "num_classes", "embed_dim", "pe", "depths", "num_heads",
                 "ff_ratio", "drop_rate", "attn_drop_rate", "edges")}
    defaults["hp.tuple_len"] = np.array(len(hp.get_model_params()))
    hp.embed_dim, hp.num_heads, hp.depths, hp.drop_rate, hp.pe = d0, heads, depths, 0.0, pe
    model = GATE(*hp.get_model_params())
    K = hp.num_kps
    cfg = dict(kp_dim=C, temporal_dim=T, num_kps=K, num_classes=nc, embed_dim=d0, depths=depths, ff_ratio=hp.ff_ratio,
               use_pe=pe, pool="weighted")
    load_synth(model, cfg, seed)
    x = torch.rand(B, T, K, C, generator=g)
    y = torch.randint(0, nc, (B,), generator=g)
    fx = record(model, "gate", hp.adj_mat, K, x, y, crit, [T, K, K, C, d0, nc, B, heads, depths, int(pe), seed])
    fx.update(defaults)
    assert not bool(torch.diagonal(hp.adj_mat).any())      # GATE: a joint does not see itself
    return fx


def random_edges(rs, W, n):
    out = set()
    while len(out) < n:
        i, j = int(rs.randint(W)), int(rs.randint(W))
        if i != j:
            out.add((min(i, j), max(i, j)))
    return [list(e) for e in sorted(out)]


def wgate_case(WGATE, WGATEParams, crit, g, *, T, W, nW, C, d0, nc, B, heads, depths, seed):
    hp = WGATEParams({"src_len": T, "num_class": nc}, C, torch.device("cpu"))
    rs = np.random.RandomState(seed)
    hp.window_size, hp.num_kps = W, nW * W
    hp.embed_dim, hp.num_heads, hp.depths, hp.drop_rate = d0, heads, depths, 0.0
    hp.edges = [random_edges(rs, W, (3 * W) // 2) for _ in range(nW)]         # W-slot edge lists, one per window
    hp.adj_mat = torch.tensor(hp.get_adj_mat(), dtype=torch.float32)
    model = WGATE(*hp.get_model_params())
    K = nW * W
    cfg = dict(kp_dim=C, temporal_dim=T, num_kps=K, num_classes=nc, embed_dim=d0, depths=depths, ff_ratio=hp.ff_ratio,
               use_pe=hp.pe, pool="mean")
    load_synth(model, cfg, seed)
    x = torch.rand(B, T, K, C, generator=g)
    y = torch.randint(0, nc, (B,), generator=g)
    fx = record(model, "wgate", hp.adj_mat, W, x, y, crit, [T, K, W, C, d0, nc, B, heads, depths, int(hp.pe), seed])
    fx["edges"] = np.array(hp.edges)
    return fx


def main():
    GATE, WGATE, GATEParams, WGATEParams, Loss = import_reference()
    torch.manual_seed(1001)
    crit = Loss()
    g = torch.Generator().manual_seed(29)
    out = {
        "gate_a.npz": gate_case(GATE, GATEParams, crit, g, T=32, C=2, d0=128, nc=10, B=4, heads=8, depths=8, pe=True, seed=41),
        "gate_b.npz": gate_case(GATE, GATEParams, crit, g, T=5, C=3, d0=128, nc=7, B=3, heads=4, depths=2, pe=False, seed=42),
        "wgate_w32.npz": wgate_case(WGATE, WGATEParams, crit, g, T=8, W=32, nW=2, C=2, d0=128, nc=10, B=2, heads=8,
                                    depths=2, seed=43),
        "wgate_w8.npz": wgate_case(WGATE, WGATEParams, crit, g, T=6, W=8, nW=4, C=3, d0=128, nc=7, B=3, heads=4,
                                   depths=2, seed=44),
    }
    for name, fx in out.items():
        np.savez_compressed(os.path.join(HERE, name), **fx)
        print(name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")


if __name__ == "__main__":
    main()
