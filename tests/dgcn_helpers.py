"""Test helpers of the DecoupledGCN baseline: the fixture configurations, the seeded weight recipe the fixtures and the
tests share, the deterministic DropGraph seed pattern, and a CPU fp64 restatement of the model's contract (reference
hwgat/models/DecoupledGCN.py) written channels-last with torch tensor ops.  The restatement records the smallest
|ReLU input| (the margin) and every ReLU mask over all 30 ReLUs (the channel gate's included), accepts explicit masks in
their place, and takes explicit DropGraph seeds."""

import torch
import torch.nn.functional as F

import stgcn_helpers as SH
from stgcn_helpers import EDGES_29, Record, make_input, fixture_input, block_samples, smoothed_ce, structure  # noqa: F401

CONFIGS = {
    "a": dict(C=2, V=29, edges=EDGES_29, G=8, block=41, n_out=256, nclass=10, B=2, T=16, seed=71, tight=True),
    "b": dict(C=3, V=29, edges=EDGES_29, G=4, block=3, n_out=128, nclass=6, B=2, T=13, seed=72, tight=True),
    "c": dict(C=2, V=29, edges=EDGES_29, G=8, block=5, n_out=256, nclass=10, B=2, T=48, seed=73, tight=True),
    "d": dict(C=2, V=29, edges=EDGES_29, G=8, block=41, n_out=256, nclass=10, B=4, T=128, seed=74, tight=False),
}
WIDTHS = SH.WIDTHS
STRIDES = SH.STRIDES
KEEP_PROB = 0.9
TCN_DROP_BLOCK = 41          # tcn1's own temporal drop: the TCNUnit default, whatever the constructor's block_size is
FIRST_DROP_UNIT = 7
SITES = ("tcn1 spatial", "tcn1 temporal", "skip spatial", "skip temporal")


def nonzero_margin(v):
    """the smallest |entry| of v among the entries that are not exactly 0.  A DropGraph mask zeroes whole joints and frames
    of both summands of a unit's last ReLU: those inputs are exactly 0 in every precision, the ReLU and its gradient gate
    agree on them whatever the rounding, and they say nothing about how close a comparison is to a flip."""
    a = v.detach().abs()
    a = a[a > 0]
    return float(a.min()) if a.numel() else float("inf")


def _relu(v, site, masks, rec):
    """stgcn_helpers._relu with the margin taken over the non-zero inputs"""
    if rec is not None:
        rec.margin = min(rec.margin, nonzero_margin(v))
        rec.masks[site] = v.detach() > 0
        if rec.pre is not None:
            rec.pre[site] = v.detach()
    m = masks[site] if masks is not None else (v.detach() > 0)
    return v * m.to(v.dtype)


def model_args(cfg, dropout=0.0):
    """the positional tuple of Model(...) for a CONFIGS entry, in DecoupledGCNParams.get_model_params() order"""
    return (cfg["C"], cfg["V"], [list(e) for e in cfg["edges"]], cfg["G"], cfg["block"], cfg["n_out"], cfg["nclass"],
            dropout, False)


def unit_plan(cfg):
    """[(C_in, C_out, stride, residual kind)] of the ten units; kind in 'none', 'identity', 'conv'"""
    return SH.block_plan(cfg)


def find_drop_size(num_nodes, num_edges):
    return 2 * num_edges / num_nodes


def is_constructed(k):
    """state_dict entries that stay as the constructor made them: the frozen lN.A and eye_list"""
    return k == "A" or k.endswith(".A") or k.endswith("eye_list")


def recipe_weights(state_dict, seed):
    """seeded values for every entry of `state_dict`: stgcn_helpers.recipe_weights' rules for everything but the graph
    entries; `decoupled_A` = its constructor value x (1 + 0.2 randn), kept positive; `lN.A` and `eye_list` as constructed"""
    plain = {k: v for k, v in state_dict.items() if not is_constructed(k) and not k.endswith("decoupled_A")}
    out = SH.recipe_weights(plain, seed)
    g = torch.Generator().manual_seed(seed + 500)
    for k, v in state_dict.items():
        if k.endswith("decoupled_A"):
            out[k] = (v.double() * (1.0 + 0.2 * torch.randn(v.shape, generator=g, dtype=torch.float64)).clamp(min=0.2)).float()
        elif is_constructed(k):
            out[k] = v.detach().clone()
    return {k: out[k] for k in state_dict}


def fixture_weights(state_dict, cfg):
    """recipe_weights with the running statistics of a model that has seen data (as stgcn_helpers.fixture_weights): every
    BatchNorm's running mean / variance is the batch statistic of a fixed calibration clip, moved by a seeded perturbation"""
    w = recipe_weights(state_dict, cfg["seed"])
    rec = Record()
    x, _ = make_input(dict(cfg, B=2, T=16), seed=999)
    with torch.no_grad():
        restate(w, x, cfg, training=True, rec=rec, keep_prob=1.0)
    g = torch.Generator().manual_seed(cfg["seed"] + 1000)
    for pre, (mean, var) in rec.batch.items():
        w[pre + "running_mean"] = (mean + 0.1 * var.sqrt() * torch.randn(mean.shape, generator=g, dtype=torch.float64)).float()
        w[pre + "running_var"] = (var * (0.75 + 0.5 * torch.rand(var.shape, generator=g, dtype=torch.float64))).float()
    return w


def drop_seed_pattern(cfg, unit, site, shape):
    """the deterministic DropGraph seeds of draw `site` (0..3, SITES) of unit `unit` (7..10), as a float tensor of `shape`
    ((N, V) spatial, (N, T) or (N, 1, T) temporal).  Spatial: seeded Bernoulli(0.15).  Temporal: one seeded frame among the
    first three of clip 0, none in any other clip -- so a block-41 drop blanks clip 0 from its start (all of it when
    T <= 21) and leaves the other clips alive, and a short block blanks a strict sub-range."""
    g = torch.Generator().manual_seed(cfg["seed"] * 1000 + unit * 10 + site)
    if site % 2 == 0:
        return (torch.rand(shape, generator=g, dtype=torch.float64) < 0.15).to(torch.float64)
    out = torch.zeros(shape, dtype=torch.float64)
    T = shape[-1]
    frame = int(torch.randint(0, min(T, 3), (1,), generator=g))
    out[0, ..., frame] = 1.0
    return out


def all_drop_seeds(cfg, B=None, T=None):
    """{(unit, site): seeds} for a clip batch of the configuration's shape"""
    B, T = B or cfg["B"], T or cfg["T"]
    seeds = {}
    for i, (_, _, s, _) in enumerate(unit_plan(cfg), start=1):
        T = (T - 1) // s + 1
        if i >= FIRST_DROP_UNIT:
            for site in range(4):
                seeds[(i, site)] = drop_seed_pattern(cfg, i, site, (B, cfg["V"]) if site % 2 == 0 else (B, T))
    return seeds


def drop_probability(z, axis, gamma):
    """the Bernoulli probabilities of a DropGraph draw on z (N, T, V, C): axis 'v' -> (N, V), axis 't' -> (N, T)"""
    a = z.detach().abs().mean(dim=(1, 3) if axis == "v" else (2, 3))
    a = a / a.sum() * a.numel()
    return torch.clamp(a * gamma, max=1.0)


def spatial_mask(seeds, A):
    M = seeds.to(A.dtype) @ A
    return 1.0 - (M > 0.001).to(A.dtype)


def temporal_mask(seeds, block):
    pooled = F.max_pool1d(seeds.unsqueeze(1), kernel_size=block, stride=1, padding=block // 2).squeeze(1)
    return 1.0 - pooled


def drop_graph(z, A, keep_prob, drop_size, block, unit, first, seeds, log):
    """DropT(DropS(z)) with the seeds of (unit, first) and (unit, first + 1); `log`: a list that receives
    (unit, site, p, seeds, mask, scale) per draw"""
    p = drop_probability(z, "v", (1.0 - keep_prob) / (1.0 + drop_size))
    s = seeds[(unit, first)].to(z.dtype).reshape(p.shape)
    mask = spatial_mask(s, A)
    scale = mask.numel() / mask.sum()
    if log is not None:
        log.append((unit, first, p, s, mask, scale))
    z = z * mask[:, None, :, None] * scale
    p = drop_probability(z, "t", (1.0 - keep_prob) / block)
    s = seeds[(unit, first + 1)].to(z.dtype).reshape(p.shape)
    mask = temporal_mask(s, block)
    scale = mask.numel() / mask.sum()
    if log is not None:
        log.append((unit, first + 1, p, s, mask, scale))
    return z * mask[:, :, None, None] * scale


def conv_rows(m, W, b):
    """nn.Conv1d(C, 1, ker, padding=(ker - 1) // 2) on m (N, L, C) -> (N, L)"""
    return F.conv1d(m.transpose(1, 2), W, b, padding=(W.shape[2] - 1) // 2)[:, 0]


def normalised_adjacency(DA):
    return DA / (DA.sum(dim=2, keepdim=True) + 0.001)


def _gate_conv(m, P, name, rec):
    """conv_rows of the gate convolution `name`; a Record keeps the absolute sum of the output's gradient entries, the
    terms whose plain sum is the gradient of the convolution's one bias (rec.terms[name + 'bias'])"""
    z = conv_rows(m, P[name + "weight"], P[name + "bias"])
    if rec is not None and z.requires_grad:
        if not hasattr(rec, "terms"):
            rec.terms = {}
        z.register_hook(lambda g: rec.terms.__setitem__(name + "bias", float(g.detach().double().abs().sum())))
    return z


def gates(h, P, pre, masks=None, rec=None):
    """(h3, s_v, s_t, s_c) of the three attention gates on h (N, T, V, C)"""
    s_v = torch.sigmoid(_gate_conv(h.mean(1), P, pre + "conv_sa.", rec))
    h = h * (1.0 + s_v[:, None, :, None])
    s_t = torch.sigmoid(_gate_conv(h.mean(2), P, pre + "conv_ta.", rec))
    h = h * (1.0 + s_t[:, :, None, None])
    se = h.mean(2).mean(1)
    s1 = _relu(se @ P[pre + "fc1c.weight"].T + P[pre + "fc1c.bias"], pre + "relu_c", masks, rec)
    s_c = torch.sigmoid(s1 @ P[pre + "fc2c.weight"].T + P[pre + "fc2c.bias"])
    return h * (1.0 + s_c[:, None, None, :]), s_v, s_t, s_c


def unit(x, P, pre, G, stride, kind, training, drop=None, masks=None, rec=None, log=None):
    """one DecoupledGCN unit on x (N, T, V, C_in); P: {key: tensor} with keys pre + 'gcn1.linear_weight' ...;
    drop: None or (keep_prob, drop_size, block, unit number, {(unit, site): seeds})"""
    N, T, V, Cin = x.shape
    W = P[pre + "gcn1.linear_weight"]
    Co = W.shape[1] // 3
    y = x @ W + P[pre + "gcn1.linear_bias"].reshape(-1)
    y = SH.batch_norm(y, P, pre + "gcn1.bn0.", training, rec).reshape(N, T, V, 3, Co)
    An = normalised_adjacency(P[pre + "gcn1.decoupled_A"]).repeat(1, Co // G, 1, 1)        # channel c: group c mod G
    a = torch.einsum("ntvkc,kcvw->ntwc", y, An)
    a = SH.batch_norm(a, P, pre + "gcn1.bn.", training, rec)
    if Cin != Co:
        dn = x @ P[pre + "gcn1.down.0.weight"][:, :, 0, 0].T + P[pre + "gcn1.down.0.bias"]
        dn = SH.batch_norm(dn, P, pre + "gcn1.down.1.", training, rec)
    else:
        dn = x
    h = _relu(a + dn, pre + "gcn1.relu", masks, rec)
    h3 = gates(h, P, pre, masks, rec)[0]
    c = SH.temporal_conv(h3, P[pre + "tcn1.conv.weight"], P[pre + "tcn1.conv.bias"], stride)
    c = SH.batch_norm(c, P, pre + "tcn1.bn.", training, rec)
    if kind == "identity":
        r = x
    elif kind == "conv":
        r = x[:, ::stride] @ P[pre + "residual.conv.weight"][:, :, 0, 0].T + P[pre + "residual.conv.bias"]
        r = SH.batch_norm(r, P, pre + "residual.bn.", training, rec)
    else:
        r = None
    if drop is not None and training and drop[0] != 1.0:
        keep_prob, drop_size, block, number, seeds = drop
        c = drop_graph(c, P[pre + "A"], keep_prob, drop_size, TCN_DROP_BLOCK, number, 0, seeds, log)
        r = drop_graph(r, P[pre + "A"], keep_prob, drop_size, block, number, 2, seeds, log)
    return _relu(c if r is None else c + r, pre + "relu", masks, rec)


def restate(params, x, cfg, training=False, masks=None, rec=None, head_keep=None, dtype=torch.float64, keep_prob=KEEP_PROB,
            seeds=None, log=None):
    """logits of the DecoupledGCN contract for keypoints x (B, T, V, C) and a {state_dict key: tensor} `params`.
    `masks`: {site: bool tensor} used in place of the ReLUs' own decisions; `rec`: a Record; `head_keep`: the head
    dropout factor (B, n_out) or None; `seeds`: {(unit, site): DropGraph seeds} (needed in train mode with
    keep_prob < 1); `log`: a list that receives every draw's (unit, site, p, seeds, mask, scale)."""
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in params.items()}
    N, T, V, C = x.shape
    h = SH.batch_norm(x.to(dtype).reshape(N, T, V * C), P, "data_bn.", training, rec).reshape(N, T, V, C)
    drop_size = find_drop_size(V, len(cfg["edges"]))
    for i, (ci, co, s, kind) in enumerate(unit_plan(cfg), start=1):
        drop = (keep_prob, drop_size, cfg["block"], i, seeds) if i >= FIRST_DROP_UNIT else None
        h = unit(h, P, f"l{i}.", cfg["G"], s, kind, training, drop, masks, rec, log)
        if rec is not None:
            rec.blocks.append(h.detach())
    feat = h.mean(dim=(1, 2))
    if head_keep is not None:
        feat = feat * head_keep.to(dtype)
    return feat @ P["head.classifier.weight"].T + P["head.classifier.bias"]


def is_trainable(k, v):
    return v.is_floating_point() and "running_" not in k and not is_constructed(k)


def grads_of(params, x, y, cfg, training, masks=None, rec=None, dtype=torch.float64, head_keep=None, keep_prob=KEEP_PROB,
             seeds=None, log=None):
    """(logits, loss, {name: gradient}) of the smoothed-CE loss for every trainable entry of `params`"""
    leaves = {k: (v.detach().to(dtype).requires_grad_(True) if is_trainable(k, v) else v) for k, v in params.items()}
    logits = restate(leaves, x, cfg, training, masks, rec, head_keep, dtype, keep_prob, seeds, log)
    loss = smoothed_ce(logits, y)
    names = [k for k, v in leaves.items() if torch.is_tensor(v) and v.requires_grad]
    gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return logits.detach(), loss.detach(), {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gs)}


# train-mode biases whose gradient is analytically zero (a per-channel constant in front of a batch-statistics BatchNorm),
# mapped to the weight whose gradient norm is their floor
def zero_grad_biases(names):
    out = {}
    for k in names:
        if k.endswith("gcn1.linear_bias"):
            out[k] = k[:-len("linear_bias")] + "linear_weight"
        elif k.endswith("gcn1.down.0.bias") or k.endswith("tcn1.conv.bias") or k.endswith("residual.conv.bias"):
            out[k] = k[:-4] + "weight"
    return out


# The two one-channel gate convolutions (conv_sa, conv_ta) have ONE bias each: d bias = sum_{n, l} dz[n, l], the plain sum
# of the gradient at the convolution's output over terms of both signs.  The value that is left after the cancellation
# says nothing about the size of the rounding error in it; the terms do: an error of relative size e in every term moves
# the sum by at most e x sum |dz[n, l]|.  So a gate bias gradient is judged at the scale of its OWN sum, sum |dz|, which
# the restatement records (Record.terms) and the fixtures carry (<tag>gs.<name>): |got - ref| / sum |dz| against the same
# bound as every other quantity, max(4 x d, K), with d measured at the same scale.  Nothing of another tensor enters.
def gate_biases(names):
    """the gate convolutions' single biases among `names`"""
    return [k for k in names if k.endswith("conv_sa.bias") or k.endswith("conv_ta.bias")]


def gate_bias_error(got, ref, terms):
    """|got - ref| / sum |terms| of a one-entry gate bias gradient, and the cancellation |ref| / sum |terms|"""
    got, ref = float(torch.as_tensor(got).double().reshape(-1)[0]), float(torch.as_tensor(ref).double().reshape(-1)[0])
    return abs(got - ref) / max(terms, 1e-300), abs(ref) / max(terms, 1e-300)


def gradient_floors(names, training):
    """{bias: weight} for every gradient that is compared relative to its weight's gradient norm: the analytically zero
    train-mode biases"""
    return zero_grad_biases(names) if training else {}


def masks_are_sound(log):
    """every DropGraph mask of a run's log drops something and no mask sums to zero"""
    return all(0 < float(mask.sum()) < mask.numel() for _, _, _, _, mask, _ in log)


BN0_BIAS = "gcn1.bn0.bias"


def digest_check(name, g, fx, prefix, tol):
    """helpers.grad_digest_check for one gradient: the norm within `tol`, the +-1 projections of the whole gradient and
    the 48-entry head within 10 x `tol`, as there.  Two departures, both by name.  A gate convolution's one bias (see
    gate_biases) is the one entry against the reference's at the scale of its own sum, fx[<prefix>gs.<name>], within
    `tol`.  The head of a gcn1.bn0.bias gradient nearly cancels (the identity partition's share behind a
    batch-statistics BatchNorm) and is far noisier in the fp32 reference than the gradient's norm: it is held within
    max(10 x tol, 4 x refdev.<prefix>gh.<name>), the reference's own head deviation; its norm and projections stay at
    `tol` and 10 x `tol`."""
    import numpy as np
    from helpers import probe_vectors
    gd = g.detach().double().flatten().cpu()
    head = fx[prefix + "gh." + name]
    if name in gate_biases([name]):
        e, left = gate_bias_error(gd, head, float(fx[prefix + "gs." + name]))
        print(f"{prefix}{name}: {e:.3g} of its terms (bound {tol:.3g}; the sum is {left:.3g} of them)")
        assert gd.numel() == 1 and e < tol, (name, "against the sum of its terms", e)
        return e
    ref_norm = float(fx[prefix + "gn." + name][0])
    scale = max(ref_norm, 1e-12)
    e1 = abs(gd.norm().item() - ref_norm) / scale
    e2 = (gd[:48] - torch.from_numpy(head).double()).norm().item() / \
        max(np.linalg.norm(head), 1e-3 * scale / max(gd.numel(), 1) ** 0.5, 1e-30)
    e3 = float(np.abs(probe_vectors(name, gd.numel()) @ gd.numpy() - fx[prefix + "gp." + name]).max()) / scale
    head_tol = tol * 10
    if name.endswith(BN0_BIAS):
        head_tol = max(head_tol, 4.0 * float(fx[f"refdev.{prefix}gh.{name}"]))
    assert e1 < tol, (name, "norm", e1)
    assert e2 < head_tol, (name, "head", e2)
    assert e3 < tol * 10, (name, "projection", e3)
    return max(e1, e2, e3)
