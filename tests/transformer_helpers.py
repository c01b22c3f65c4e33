"""Test helpers of the Transformer baseline: the seeded weight recipe the fixtures and the tests share, and a CPU fp64
restatement of the model's contract (reference hwgat/models/Transformer.py with torch 2.10 padding semantics) written
with torch functional ops."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (name, input_dim C, joints, nclass, d_model, nhead, ff, layers, max_len, pool, T, B, weight seed)
CONFIGS = {
    "a": dict(C=2, K=29, nclass=10, d=512, nhead=8, ff=2048, layers=3, max_len=64, pool="mean", T=64, B=4, seed=51),
    "b": dict(C=3, K=29, nclass=6, d=128, nhead=2, ff=256, layers=2, max_len=37, pool="concat", T=37, B=3, seed=52),
    "c": dict(C=3, K=29, nclass=6, d=128, nhead=2, ff=256, layers=2, max_len=37, pool="max", T=37, B=3, seed=53),
}


def model_args(cfg):
    """the positional tuple of Model(...) for a CONFIGS entry (dropout 0.1 as TransformerParams)"""
    return (cfg["C"] * cfg["K"], cfg["nclass"], -1, cfg["d"], cfg["nhead"], cfg["ff"], cfg["layers"], 0.1,
            cfg["max_len"], cfg["pool"])


def recipe_weights(state_dict, seed):
    """seeded parameter values for every floating entry of `state_dict` except the PE buffer, in its order: weights
    uniform(+-sqrt(3 / fan_in)) (unit-variance activations), biases and LayerNorm shifts small, LayerNorm scales ~1"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in state_dict.items():
        if k.endswith("pos_encoder.pe"):
            continue
        if v.dim() > 1:
            bound = math.sqrt(3.0 / v.shape[1])
            out[k] = (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * bound
        elif ".norm" in k and k.endswith("weight"):
            out[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g, dtype=torch.float64)
        else:
            out[k] = 0.05 * torch.randn(v.shape, generator=g, dtype=torch.float64)
        out[k] = out[k].float()
    return out


def make_input(cfg, seed=7):
    """(B, T, K, C) keypoints in [0, 1) with the padding patterns of the fixtures (pad_index -1 on whole frames):
    clip 0 tail-padded, clip 1 scattered padded frames, clip 2 entirely padded (config a), the rest unpadded"""
    g = torch.Generator().manual_seed(seed)
    B, T = cfg["B"], cfg["T"]
    x = torch.rand(B, T, cfg["K"], cfg["C"], generator=g)
    x[0, T - T // 3:] = -1.0
    x[1, 3::5] = -1.0
    if B >= 4:
        x[2] = -1.0
    y = torch.randint(0, cfg["nclass"], (B,), generator=g)
    return x, y


def positional(d, max_len):
    pe = torch.zeros(max_len, d, dtype=torch.float64)
    position = torch.arange(0, max_len).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d, 2) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def attention(qkv, pad, n_heads, keep=None):
    """fp64 restatement of the key-padded attention: qkv (B, T, 3d), pad (B, T) bool -> o (B, T, d).  `keep`: the
    (B, nH, T, T) dropout factor (0 or 1/(1-p)) on the probabilities, or None.  A query with every key padded gets 0."""
    B, T, d3 = qkv.shape
    d = d3 // 3
    hd = d // n_heads
    q, k, v = qkv.split(d, dim=-1)
    q, k, v = (t.reshape(B, T, n_heads, hd).transpose(1, 2) for t in (q, k, v))
    s = (q * hd ** -0.5) @ k.transpose(-1, -2)
    allpad = pad.all(dim=1)[:, None, None, None]
    kp = pad[:, None, None, :] & ~allpad
    p = torch.softmax(s.masked_fill(kp, float("-inf")), dim=-1) * (~allpad)
    if keep is not None:
        p = p * keep
    return (p @ v).transpose(1, 2).reshape(B, T, d)


def restate(params, x, cfg, pad_index=-1.0, per_layer=None, masks=None):
    """fp64 logits of the Transformer contract for keypoints x (B, T, K, C) and a {state_dict key: tensor} `params`.
    `masks`: None (dropout off) or the train-mode dropout factors (0 or 1/(1-p)) of every site, keyed "embed" (B, T, d)
    and (layer, "attn") (B, nH, T, T), (layer, "drop1") / (layer, "drop2") (B, T, d), (layer, "ff") (B, T, ff).
    `per_layer`: a list that receives every encoder layer's output."""
    mk = (lambda key: masks[key].double()) if masks is not None else (lambda key: 1.0)
    P = {k: v.double() for k, v in params.items()}
    d, nH = cfg["d"], cfg["nhead"]
    B, T = x.shape[0], x.shape[1]
    src = x.reshape(B, T, -1).double()
    pad = src[:, :, 0] == pad_index
    h = (F.linear(src, P["encoder.weight"], P["encoder.bias"]) * math.sqrt(d) + positional(d, cfg["max_len"])[:T]) * mk("embed")
    for i in range(cfg["layers"]):
        pre = f"transformer_encoder.layers.{i}."
        qkv = F.linear(h, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"])
        o = attention(qkv, pad, nH, mk((i, "attn")) if masks is not None else None)
        a = F.linear(o, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"]) * mk((i, "drop1"))
        h = F.layer_norm(h + a, (d,), P[pre + "norm1.weight"], P[pre + "norm1.bias"])
        u = torch.relu(F.linear(h, P[pre + "linear1.weight"], P[pre + "linear1.bias"])) * mk((i, "ff"))
        f = F.linear(u, P[pre + "linear2.weight"], P[pre + "linear2.bias"]) * mk((i, "drop2"))
        h = F.layer_norm(h + f, (d,), P[pre + "norm2.weight"], P[pre + "norm2.bias"])
        if per_layer is not None:
            per_layer.append(h)
    h = F.layer_norm(h, (d,), P["transformer_encoder.norm.weight"], P["transformer_encoder.norm.bias"])
    if cfg["pool"] == "mean":
        feat, head = h.mean(dim=1), "classifier."
    elif cfg["pool"] == "max":
        feat, head = h.max(dim=1).values, "classifier."
    else:
        feat, head = h.reshape(B, -1), "classifier.0."
    return F.linear(feat, P[head + "weight"], P[head + "bias"])


def smoothed_ce(logits, y, smooth=0.01):
    """the reference's SmoothedCrossEntropyLoss (losses/SmoothCrossEntropy.py): (1-eps) NLL + eps (-mean log p)"""
    logp = torch.log_softmax(logits, dim=-1)
    nll = -logp.gather(-1, y.view(-1, 1)).squeeze(1)
    return ((1.0 - smooth) * nll + smooth * (-logp.mean(-1))).mean()


def structure(model):
    """the state_dict structure record of make_fixtures_checkpoint.structure (keys, shapes, dtypes, parameters)"""
    sd = model.state_dict()
    params = dict(model.named_parameters())
    out = {"keys": np.array(list(sd)),
           "ndim": np.array([v.dim() for v in sd.values()], dtype=np.int64),
           "dims": np.array([d for v in sd.values() for d in v.shape], dtype=np.int64),
           "dtypes": np.array([str(v.dtype).replace("torch.", "") for v in sd.values()]),
           "params": np.array(list(params)),
           "requires_grad": np.array([p.requires_grad for p in params.values()])}
    for k, v in sd.items():
        if k not in params:
            out["buf." + k] = v.numpy()
    return out
