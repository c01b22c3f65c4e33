"""Test helpers of the ST-GCN baseline: the fixture configurations, the seeded weight recipe the fixtures and the tests
share, and a CPU fp64 restatement of the model's contract (reference hwgat/models/STGCN.py) written channels-last with
torch tensor ops.  The restatement records the smallest |ReLU input| (the margin) and every ReLU mask, and accepts
explicit masks in their place, so a comparison can be held on one side of every ReLU."""
import math

import torch

from transformer_helpers import smoothed_ce, structure  # noqa: F401  (re-exported)

EDGES_29 = [[2, 0], [1, 0], [0, 3], [0, 4], [3, 5], [4, 6], [5, 7], [6, 8], [7, 9], [9, 10], [9, 11], [11, 12], [11, 13],
            [13, 14], [9, 13], [13, 15], [9, 15], [15, 16], [15, 17], [9, 17], [17, 18], [8, 19], [19, 27], [19, 20],
            [19, 21], [19, 23], [19, 25], [21, 22], [21, 23], [23, 24], [23, 25], [25, 26], [25, 27], [27, 28]]

# tight fixtures a-c (gradients compared tightly: the generator picks the input seed with the largest ReLU margin), wide d
CONFIGS = {
    "a": dict(C=2, V=29, center=0, edges=EDGES_29, importance=True, n_out=256, nclass=10, B=2, T=16, seed=61, tight=True),
    "b": dict(C=3, V=29, center=0, edges=EDGES_29, importance=True, n_out=128, nclass=6, B=2, T=13, seed=62, tight=True),
    "c": dict(C=2, V=29, center=0, edges=EDGES_29, importance=False, n_out=256, nclass=10, B=2, T=16, seed=63, tight=True),
    "d": dict(C=2, V=29, center=0, edges=EDGES_29, importance=True, n_out=256, nclass=10, B=4, T=128, seed=64, tight=False),
}
WIDTHS = [64, 64, 64, 64, 128, 128, 128, 256, 256]
STRIDES = [1, 1, 1, 1, 2, 1, 1, 2, 1, 1]
EPS, MOMENTUM = 1e-5, 0.1


def model_args(cfg, dropout=0.05):
    """the positional tuple of Model(...) for a CONFIGS entry, in STGCNParams.get_model_params() order"""
    return (cfg["C"], cfg["V"], cfg["center"], [list(e) for e in cfg["edges"]], cfg["importance"], cfg["n_out"],
            cfg["nclass"], dropout, False)


def block_plan(cfg):
    """[(C_in, C_out, stride, residual kind)] of the ten blocks; kind in 'none', 'identity', 'conv'"""
    outs = WIDTHS + [cfg["n_out"]]
    ins = [cfg["C"]] + outs[:-1]
    plan = []
    for i, (ci, co, s) in enumerate(zip(ins, outs, STRIDES)):
        plan.append((ci, co, s, "none" if i == 0 else "identity" if ci == co and s == 1 else "conv"))
    return plan


def recipe_weights(state_dict, seed):
    """seeded values for every entry of `state_dict` except the adjacency buffer `A`, in its order: conv / linear weights
    uniform(+-sqrt(3 / fan_in)), biases small, BatchNorm scales ~1 and shifts small but not 0, running means / variances
    away from 0 / 1, edge importances ~1, num_batches_tracked 3 -- nothing the backward multiplies by is trivial"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda shape, s: s * torch.randn(shape, generator=g, dtype=torch.float64)
    out = {}
    for k, v in state_dict.items():
        if k == "A":
            continue
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(3, dtype=torch.int64)
            continue
        if k.endswith("running_mean"):
            t = rn(v.shape, 0.1)
        elif k.endswith("running_var"):
            t = 0.75 + 0.5 * torch.rand(v.shape, generator=g, dtype=torch.float64)
        elif k.startswith("edge_importance"):
            t = 1.0 + rn(v.shape, 0.2)
        elif v.dim() > 1:
            fan_in = v[0].numel()
            t = (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * math.sqrt(3.0 / fan_in)
        elif k.endswith("weight"):            # 1-d weights are BatchNorm scales (data_bn, tcn.0, tcn.3, residual.1)
            t = 1.0 + rn(v.shape, 0.1)
        else:
            t = rn(v.shape, 0.05)
        out[k] = t.float()
    return out


def fixture_weights(state_dict, cfg):
    """recipe_weights with the running statistics of a model that has seen data: every BatchNorm's running mean /
    variance is the batch statistic of a fixed calibration clip (seeded, B 2, T 16, fp64 restatement in train mode),
    moved by a seeded perturbation (mean + 0.1 std randn, variance x uniform(0.75, 1.25)).  Eval-mode activations then
    have the unit scale of train mode instead of whatever arbitrary running values would give them."""
    w = recipe_weights(state_dict, cfg["seed"])
    rec = Record()
    x, _ = make_input(dict(cfg, B=2, T=16), seed=999)
    with torch.no_grad():
        restate(dict(w, A=state_dict["A"]), x, cfg, training=True, rec=rec)
    g = torch.Generator().manual_seed(cfg["seed"] + 1000)
    for pre, (mean, var) in rec.batch.items():
        w[pre + "running_mean"] = (mean + 0.1 * var.sqrt() * torch.randn(mean.shape, generator=g, dtype=torch.float64)).float()
        w[pre + "running_var"] = (var * (0.75 + 0.5 * torch.rand(var.shape, generator=g, dtype=torch.float64))).float()
    return w


def make_input(cfg, seed=7):
    """(B, T, V, C) keypoints in [0, 1) and labels"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(cfg["B"], cfg["T"], cfg["V"], cfg["C"], generator=g)
    y = torch.randint(0, cfg["nclass"], (cfg["B"],), generator=g)
    return x, y


def fixture_input(fx, cfg):
    """(x, y) of a fixture: the stored clip, or make_input from the stored input seed where the clip is not stored"""
    x = torch.from_numpy(fx["x"]) if "x" in fx else make_input(cfg, seed=int(fx["input_seed"]))[0]
    return x, torch.from_numpy(fx["y"]).long()


class Record:
    """what one restatement run leaves behind: ReLU masks by site name, the smallest |ReLU input|, block outputs, the
    updated running statistics ({state_dict key: tensor}) and the pre-activation tensors when `keep_pre`"""

    def __init__(self, keep_pre=False):
        self.masks, self.margin, self.blocks, self.stats, self.pre = {}, float("inf"), [], {}, {} if keep_pre else None
        self.batch = {}                 # BatchNorm prefix -> (batch mean, biased batch variance), train mode


def _relu(v, site, masks, rec):
    if rec is not None:
        rec.margin = min(rec.margin, float(v.detach().abs().min()))
        rec.masks[site] = v.detach() > 0
        if rec.pre is not None:
            rec.pre[site] = v.detach()
    m = masks[site] if masks is not None else (v.detach() > 0)
    return v * m.to(v.dtype)


def batch_norm(x, P, pre, training, rec=None):
    """BatchNorm over every dimension but the last, parameters P[pre + 'weight' ...]; train mode: batch statistics (biased
    variance) and the running values after the step (unbiased variance, momentum 0.1) go to rec.stats"""
    C = x.shape[-1]
    flat = x.reshape(-1, C)
    if training:
        M = flat.shape[0]
        if M < 2:
            raise ValueError("Expected more than 1 value per channel when training")
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
        if rec is not None:
            rec.batch[pre] = (mean.detach(), var.detach())
            rec.stats[pre + "running_mean"] = (1 - MOMENTUM) * P[pre + "running_mean"] + MOMENTUM * mean.detach()
            rec.stats[pre + "running_var"] = (1 - MOMENTUM) * P[pre + "running_var"] + MOMENTUM * var.detach() * M / (M - 1)
            rec.stats[pre + "num_batches_tracked"] = P[pre + "num_batches_tracked"] + 1
    else:
        mean, var = P[pre + "running_mean"], P[pre + "running_var"]
    return (x - mean) / torch.sqrt(var + EPS) * P[pre + "weight"] + P[pre + "bias"]


def temporal_conv(h, W, b, stride):
    """(N, T, V, C) -> (N, (T - 1) // stride + 1, V, C_out) with W (C_out, C, taps, 1), zero padding taps // 2"""
    taps = W.shape[2]
    pad = taps // 2
    N, T, V, C = h.shape
    To = (T + 2 * pad - taps) // stride + 1
    halo = h.new_zeros(N, pad, V, C)
    hp = torch.cat([halo, h, halo], dim=1)
    out = b
    for tap in range(taps):
        out = out + hp[:, tap: tap + stride * (To - 1) + 1: stride] @ W[:, :, tap, 0].T
    return out


def block(x, P, pre, A, E, stride, kind, training, masks=None, rec=None):
    """one ST-GCN block on x (N, T, V, C_in); P: {key: tensor} with keys pre + 'gcn.conv.weight' ...; E None = ones"""
    N, T, V, _ = x.shape
    W = P[pre + "gcn.conv.weight"][:, :, 0, 0]
    Co = W.shape[0] // 3
    y = (x @ W.T + P[pre + "gcn.conv.bias"]).reshape(N, T, V, 3, Co)
    a = torch.einsum("ntvkc,kvw->ntwc", y, A if E is None else A * E)
    h = _relu(batch_norm(a, P, pre + "tcn.0.", training, rec), pre + "tcn.1", masks, rec)
    c = temporal_conv(h, P[pre + "tcn.2.weight"], P[pre + "tcn.2.bias"], stride)
    c = batch_norm(c, P, pre + "tcn.3.", training, rec)
    if kind == "identity":
        c = c + x
    elif kind == "conv":
        r = x[:, ::stride] @ P[pre + "residual.0.weight"][:, :, 0, 0].T + P[pre + "residual.0.bias"]
        c = c + batch_norm(r, P, pre + "residual.1.", training, rec)
    return _relu(c, pre + "relu", masks, rec)


def restate(params, x, cfg, training=False, masks=None, rec=None, head_keep=None, dtype=torch.float64):
    """logits of the ST-GCN contract for keypoints x (B, T, V, C) and a {state_dict key: tensor} `params` (must hold `A`).
    `masks`: {site: bool tensor} used in place of the ReLUs' own decisions; `rec`: a Record; `head_keep`: the head
    dropout factor (B, n_out) (0 or 1 / (1 - p)) or None."""
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    N, T, V, C = x.shape
    h = batch_norm(x.to(dtype).reshape(N, T, V * C), P, "data_bn.", training, rec).reshape(N, T, V, C)
    for i, (ci, co, s, kind) in enumerate(block_plan(cfg)):
        E = P[f"edge_importance.{i}"] if cfg["importance"] else None
        h = block(h, P, f"st_gcn_networks.{i}.", P["A"], E, s, kind, training, masks, rec)
        if rec is not None:
            rec.blocks.append(h.detach())
    feat = h.mean(dim=(1, 2))
    if head_keep is not None:
        feat = feat * head_keep.to(dtype)
    return feat @ P["head.classifier.weight"].T + P["head.classifier.bias"]


def grads_of(params, x, y, cfg, training, masks=None, rec=None, dtype=torch.float64, head_keep=None):
    """(logits, loss, {name: gradient}) of the smoothed-CE loss for every floating entry of `params` that is a parameter
    (running statistics and `A` excluded)"""
    leaves = {}
    for k, v in params.items():
        is_param = v.is_floating_point() and k != "A" and "running_" not in k
        leaves[k] = v.detach().to(dtype).requires_grad_(True) if is_param else v
    logits = restate(leaves, x, cfg, training, masks, rec, head_keep, dtype)
    loss = smoothed_ce(logits, y)
    names = [k for k, v in leaves.items() if torch.is_tensor(v) and v.requires_grad]
    gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return logits.detach(), loss.detach(), {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gs)}


# train-mode biases whose gradient is analytically zero (a per-channel constant in front of a batch-statistics BatchNorm),
# mapped to the weight whose gradient norm is their floor
def zero_grad_biases(names):
    out = {}
    for k in names:
        if k.endswith("tcn.2.bias") or k.endswith("residual.0.bias"):
            out[k] = k[:-4] + "weight"
    return out


def block_samples(h):
    """the strided sample of a block output (B, T, V, C) a fixture stores (coarser for long clips)"""
    long = h.shape[1] > 16
    return h[:, ::(11 if long else 3), ::(7 if long else 4), ::(9 if long else 5)]
