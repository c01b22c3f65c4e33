"""Dense restatement of the band models' arithmetic for the GATE / wide-window WGATE tests (test side only).

The reference's GATE (hwgat/models/GATE.py) and WGATE with a window size other than 16 (hwgat/models/WGATE.py) form the
attention densely over all T*W tokens of a window and add a 0 / -10000 mask; the kernels under test only ever touch three
key frames.  This file states the dense form once, with the window size W as a parameter (GATE: one window of W = K
joints), in whatever dtype the inputs have (fp64 in the tests), plus GATE's LayerNorm + weighted token pool and the whole
models built from them.  tests/test_gate_cpu.py pins it to the reference-made fixtures tests/golden/gate_*.npz and
wgate_w*.npz; the GPU tests compare the kernels with it.
"""
import numpy as np
import torch

from oracle import hwgat_oracle as O

NEG = -10000.0


# ------------------------------------------------------------------------------------------ adjacencies
def frame_graph(edges, W, self_loops):
    """(W, W) symmetric 0/1 joint graph of one frame from an edge list"""
    a = torch.eye(W) if self_loops else torch.zeros(W, W)
    for i, j in edges:
        a[i, j] = 1.0
        a[j, i] = 1.0
    return a


def band_adjacency(diag, prev, nxt, frames):
    """(nW, T*W, T*W) block-tridiagonal 0/1 matrix: `diag` (nW, W, W) inside a frame, `prev` / `nxt` towards frames
    f-1 / f+1"""
    nW, W, _ = diag.shape
    a = torch.zeros(nW, frames, W, frames, W)
    for f in range(frames):
        a[:, f, :, f, :] = diag
        if f > 0:
            a[:, f, :, f - 1, :] = prev
        if f + 1 < frames:
            a[:, f, :, f + 1, :] = nxt
    return a.reshape(nW, frames * W, frames * W)


def default_adjacency(edge_lists, W, frames, self_loops):
    """what both references build: the joint graph inside a frame (WGATE: + identity, GATE: no self loops), the same
    joint in the neighbouring frames"""
    diag = torch.stack([frame_graph(e, W, self_loops) for e in edge_lists])
    eye = torch.eye(W).expand(len(edge_lists), W, W)
    return band_adjacency(diag, eye, eye, frames)


def expected_mask_words(adj, frames, W):
    """the (nW, 32, 3) words of functional.wband_mask_rows, spelled out entry by entry from query frame 1 of `adj`
    (key frames 0, 1, 2; needs at least 3 frames)"""
    assert frames >= 3
    a = adj if adj.dim() == 3 else adj.unsqueeze(0)
    words = np.zeros((a.shape[0], 32, 3), dtype=np.int64)
    for w in range(a.shape[0]):
        for i in range(W):
            for t in range(3):
                for j in range(W):
                    if a[w, W + i, t * W + j] != 0:
                        words[w, i, t] |= 1 << j
    return np.where(words >= 2 ** 31, words - 2 ** 32, words).astype(np.int32)


# ------------------------------------------------------------------------------------------ attention core
def dense_band_attention(qkv, adj, n_heads, W, attn_keep=None, return_probs=False):
    """natural-order qkv (B,F,K,3d) -> o (B,F,K,d): every window of W joints attends densely over its F*W tokens
    (token = frame * W + joint) with the additive 0 / -10000 mask of `adj` ((nW, F*W, F*W), or (F*W, F*W) for one
    window).  attn_keep: None or the dropout factor (B, nW, nH, F*W, F*W) applied to the probabilities."""
    B, F, K, d3 = qkv.shape
    d, nW = d3 // 3, K // W
    hd = d // n_heads
    a = adj if adj.dim() == 3 else adj.unsqueeze(0)
    mask = torch.where(a != 0, torch.zeros((), dtype=qkv.dtype), torch.full((), NEG, dtype=qkv.dtype))
    t = qkv.reshape(B, F, nW, W, 3, n_heads, hd).permute(4, 0, 2, 5, 1, 3, 6).reshape(3, B, nW, n_heads, F * W, hd)
    s = (t[0] * hd ** -0.5) @ t[1].transpose(-2, -1) + mask[None, :, None]
    p = torch.softmax(s, dim=-1)
    o = (p if attn_keep is None else p * attn_keep) @ t[2]                       # (B, nW, nH, F*W, hd)
    o = o.reshape(B, nW, n_heads, F, W, hd).permute(0, 3, 1, 4, 2, 5).reshape(B, F, K, d)
    return (o, p) if return_probs else o


# ------------------------------------------------------------------------------------------ pool
def ln_weighted_pool(x, gamma, beta, w, bias):
    """feat[b, c] = sum_tok w[tok] LN(x)[b, tok, c] + bias for x (B, ..., d), w with one weight per token"""
    B, d = x.shape[0], x.shape[-1]
    y = O.layer_norm(x.reshape(B, -1, d), gamma, beta)
    return torch.einsum("btc,t->bc", y, w.reshape(-1)) + bias.reshape(())


# ------------------------------------------------------------------------------------------ whole models
class DenseBandModel:
    """functional forward of GATE (pool='weighted', W = K) or WGATE (pool='mean') on a reference-keyed parameter dict"""

    def __init__(self, params, *, adj, W, depths, num_heads, use_pe, pool):
        self.p, self.adj, self.W, self.depths, self.heads, self.use_pe, self.pool = params, adj, W, depths, num_heads, use_pe, pool
        self.taps = {}

    def block(self, x, i):
        P, pre = self.p, f"layers.{i}."
        xn = O.layer_norm(x, P[pre + "norm1.weight"], P[pre + "norm1.bias"])
        qkv = xn @ P[pre + "attn.qkv.weight"].t() + P[pre + "attn.qkv.bias"]
        o = dense_band_attention(qkv, self.adj.to(x.dtype), self.heads, self.W)
        y = x + (o @ P[pre + "attn.proj.weight"].t() + P[pre + "attn.proj.bias"])
        h = O.layer_norm(y, P[pre + "norm2.weight"], P[pre + "norm2.bias"])
        h = O.gelu(h @ P[pre + "ff.fc1.weight"].t() + P[pre + "ff.fc1.bias"])
        return y + (h @ P[pre + "ff.fc2.weight"].t() + P[pre + "ff.fc2.bias"])

    def forward(self, x, tap=False):
        P = self.p
        h = O.fourier_embed(x, P["B"])
        if self.use_pe:
            h = h + P["pos_encoder.pe"][:, :h.shape[1]]
        for i in range(self.depths):
            h = self.block(h, i)
            if tap:
                self.taps[f"block{i}"] = h
        if self.pool == "weighted":
            feat = ln_weighted_pool(h, P["norm.weight"], P["norm.bias"], P["weightedAvg.weight"], P["weightedAvg.bias"])
        else:
            feat = O.layer_norm(h, P["norm.weight"], P["norm.bias"]).mean(dim=(1, 2))
        if tap:
            self.taps["feat"] = feat
        return feat @ P["head.weight"].t() + P["head.bias"]


def param_shapes(*, kp_dim, temporal_dim, num_kps, num_classes, embed_dim, depths, ff_ratio, use_pe, pool):
    """ordered (name, shape) list of the reference state_dict minus the derived `adj_mask` buffer"""
    d, hid = embed_dim, int(embed_dim * ff_ratio)
    out = [("B", (d // 2, kp_dim))]
    if use_pe:
        out.append(("pos_encoder.pe", (1, temporal_dim, 1, d)))
    for i in range(depths):
        pre = f"layers.{i}."
        out += [(pre + "norm1.weight", (d,)), (pre + "norm1.bias", (d,)),
                (pre + "attn.qkv.weight", (3 * d, d)), (pre + "attn.qkv.bias", (3 * d,)),
                (pre + "attn.proj.weight", (d, d)), (pre + "attn.proj.bias", (d,)),
                (pre + "norm2.weight", (d,)), (pre + "norm2.bias", (d,)),
                (pre + "ff.fc1.weight", (hid, d)), (pre + "ff.fc1.bias", (hid,)),
                (pre + "ff.fc2.weight", (d, hid)), (pre + "ff.fc2.bias", (d,))]
    out += [("norm.weight", (d,)), ("norm.bias", (d,))]
    if pool == "weighted":
        out += [("weightedAvg.weight", (1, temporal_dim * num_kps)), ("weightedAvg.bias", (1,))]
    out += [("head.weight", (num_classes, d)), ("head.bias", (num_classes,))]
    return out


def synth_params(seed, *, weight_std=0.08, **cfg):
    """deterministic parameter set (numpy MT19937 stream, one draw per tensor in `param_shapes` order).  The pool
    weights are O(1 / (T K)) and NON-uniform (between 0.25 and 1.75 times 1 / (T K)), the pool bias is not zero: a mean
    pool cannot reproduce the fixtures."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, shape in param_shapes(**cfg):
        if name == "pos_encoder.pe":
            out[name] = O.sinusoid_table(cfg["temporal_dim"], cfg["embed_dim"])
            continue
        if name == "B":
            v = rs.standard_normal(shape) * 10.0
        elif name == "weightedAvg.weight":
            v = (0.25 + 1.5 * rs.random_sample(shape)) / shape[1]
        elif name == "weightedAvg.bias":
            v = np.array([0.03]) + 0.0 * rs.standard_normal(shape)
        elif name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
            v = 1.0 + 0.1 * rs.standard_normal(shape)
        elif name.endswith(".bias"):
            v = 0.05 * rs.standard_normal(shape)
        else:
            v = weight_std * rs.standard_normal(shape)
        out[name] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return out


# ------------------------------------------------------------------------------------------ fixtures
def fixture_setup(fx):
    """(cfg, params, adj) of a tests/golden/gate_*.npz or wgate_w*.npz fixture (make_fixtures_gate.py); `adj` is rebuilt
    from the recorded per-window frame blocks (diag / prev / next)"""
    kind = str(fx["kind"])
    T, K, W, C, d0, nc, B, heads, depths, pe, seed = [int(v) for v in fx["cfg"]]
    cfg = dict(kp_dim=C, temporal_dim=T, num_kps=K, num_classes=nc, embed_dim=d0, depths=depths, ff_ratio=2.0,
               use_pe=bool(pe), pool="weighted" if kind == "gate" else "mean")
    params = synth_params(seed, **cfg)
    blocks = torch.from_numpy(fx["adj_blocks"]).float()                         # (nW, 3, W, W): prev, diag, next
    adj = band_adjacency(blocks[:, 1], blocks[:, 0], blocks[:, 2], T)
    return dict(cfg, kind=kind, W=W, B=B, num_heads=heads), params, adj


def dense_model_from_fixture(fx, dtype=torch.float64):
    cfg, params, adj = fixture_setup(fx)
    params = {k: v.to(dtype) for k, v in params.items()}
    model = DenseBandModel(params, adj=adj, W=cfg["W"], depths=cfg["depths"], num_heads=cfg["num_heads"],
                           use_pe=cfg["use_pe"], pool=cfg["pool"])
    return model, params, cfg, adj
