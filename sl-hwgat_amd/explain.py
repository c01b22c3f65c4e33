"""Attention maps and joint relevance of the graph-attention models (HWGATE at any window size, HGATE, WGATE, GATE).

In the reference the attention probabilities are a tensor (`attn = self.softmax(attn)`, HWGATE.py:111; likewise HGATE,
WGATE, GATE) and a forward hook on `blk.attn.softmax` reads it.  Here a block is one fused autograd node whose attention
kernel keeps P in registers, so there is nothing to hook; `AttentionTap` is the replacement:

    tap = explain.AttentionTap(model, probs=True)
    with tap, torch.no_grad():
        logits = model(x)                       # the same launches as always + one hwgat_attn_probs per tapped block
    tap.probs[k]                                # the tensor the reference hook on block k's softmax would have seen
    tap.received[k]                             # (B, F_k, K): attention received per frame and joint slot
    tap.clip_relevance()                        # (B, T, J): one normalised map per clip

The tap launches `functional.attn_probs` (csrc/attn_probs.hip) on the qkv tensor the block's fused forward just formed,
into static buffers: no host synchronisation, nothing read back, so a `serve.GraphedEval` built inside `with tap:` captures
the tap's launches and replays them.  Eval-mode maps only: no train-mode threshold, no attention dropout.
"""
from typing import Dict, Iterable, Optional

import torch

from . import functional as HF
from .models._family import FamilyModel


def window_frames(F: int, shifted: bool) -> torch.Tensor:
    """(F/2, 2) int64: the frames of the block's INPUT that window fi of a pair kind ('win', 'pwin', 'blk') holds, slot
    tp = 0, 1.  Plain blocks: (2 fi, 2 fi + 1).  Shifted blocks roll the input by -1 frame first (HWGATE.py:197-200), so
    window fi holds ((2 fi + 1) % F, (2 fi + 2) % F): the last window pairs frame F - 1 with frame 0 and takes the
    same-frame mask."""
    F = int(F)
    if F <= 0 or F % 2:
        raise ValueError(f"a frame-pair partition needs an even number of frames, got {F}")
    base = torch.arange(F, dtype=torch.int64).view(F // 2, 2)
    return (base + (1 if shifted else 0)) % F


def band_to_dense(probs: torch.Tensor, F: int, W: int) -> torch.Tensor:
    """scatter a band tensor (B, nW, nH, F, W, 3, W) of functional.attn_probs ('band', 'wband') into the reference's dense
    (B nW, nH, F W, F W) attention tensor (token = frame W + joint); everything outside the band is 0.  A host-side
    helper for tests and small T: the dense tensor grows with T squared."""
    B, nW, nH = probs.shape[:3]
    if tuple(probs.shape[3:]) != (F, W, 3, W):
        raise ValueError(f"expected a (B, nW, nH, {F}, {W}, 3, {W}) band tensor, got {tuple(probs.shape)}")
    dense = torch.zeros(B * nW, nH, F, W, F, W, dtype=probs.dtype, device=probs.device)
    band = probs.reshape(B * nW, nH, F, W, 3, W)
    for f in range(F):
        for t in range(3):
            fk = f - 1 + t
            if 0 <= fk < F:
                dense[:, :, f, :, fk, :] = band[:, :, f, :, t, :]
    return dense.reshape(B * nW, nH, F * W, F * W)


def fold_relevance(received: Dict[int, torch.Tensor], T: int, part_index: Optional[torch.Tensor] = None,
                   num_joints: Optional[int] = None) -> torch.Tensor:
    """{block: (B, F_k, K) received} -> (B, T, J) relevance, plain torch ops: every map is brought from its stage's frame
    count F_k to T by repeating frames and dividing by T / F_k (the sum is conserved), the maps are averaged, the K slots
    are folded onto raw joints with `part_index` (slots of the same joint add; None: J = K slots) and every clip is
    normalised to sum 1."""
    if not received:
        raise ValueError("no attention map recorded: run a forward inside `with tap:` first")
    total = None
    for r in received.values():
        B, Fk, K = r.shape
        if T % Fk:
            raise ValueError(f"a map with {Fk} frames cannot be repeated to {T}")
        rep = T // Fk
        up = r.repeat_interleave(rep, dim=1) / rep
        total = up if total is None else total + up
    rel = total / len(received)
    if part_index is not None:
        idx = part_index.to(device=rel.device, dtype=torch.int64)
        J = int(num_joints) if num_joints is not None else int(idx.max()) + 1
        folded = torch.zeros(rel.shape[0], T, J, dtype=rel.dtype, device=rel.device)
        folded.index_add_(2, idx, rel)
        rel = folded
    return rel / rel.sum(dim=(1, 2), keepdim=True)


class AttentionTap:
    """Context manager that exports the attention maps of a FamilyModel's eval() forward.

    `blocks`: indices into model.block_list() (default: all).  `probs`: keep the full probability tensors
    (functional.attn_probs: pair kinds (B, F/2, nW, nH, n, n), band kinds (B, nW, nH, F, W, 3, W)) in `tap.probs[k]`;
    `received`: keep the (B, F_k, K) head-mean column sums in `tap.received[k]`.  Buffers are allocated on the first
    forward of a shape and reused by every later one, so the addresses a captured graph holds stay valid.  Logits are
    bit-identical with and without the tap, and a model without a tap issues exactly the launches it always did."""

    def __init__(self, model, blocks: Optional[Iterable[int]] = None, probs: bool = False, received: bool = True):
        if not isinstance(model, FamilyModel):
            raise TypeError(f"AttentionTap exports the graph attention of HWGATE, HGATE, WGATE and GATE models; "
                            f"{type(model).__module__.rsplit('.', 1)[-1]} has none (the Transformer's key-padded dense "
                            f"attention is a different tensor, the GCN baselines have no attention at all)")
        if not (probs or received):
            raise ValueError("AttentionTap: ask for probs, received or both")
        n = len(model.block_list())
        chosen = range(n) if blocks is None else sorted({int(k) for k in blocks})
        if any(k < 0 or k >= n for k in chosen):
            raise IndexError(f"blocks must index model.block_list() (0..{n - 1}), got {list(chosen)}")
        self.model, self.blocks = model, tuple(chosen)
        self.want_probs, self.want_received = bool(probs), bool(received)
        self.probs: Dict[int, torch.Tensor] = {}
        self.received: Dict[int, torch.Tensor] = {}
        self._static = {}                  # (block, qkv shape, dtype) -> (probs buffer | None, received buffer | None)
        self._num_joints = None

    def __enter__(self):
        if self.model.training:
            raise RuntimeError("AttentionTap exports eval-mode attention maps: call model.eval() first")
        if self.model.attention_tap is not None:
            raise RuntimeError("the model already has an armed AttentionTap")
        self.model.attention_tap = self
        return self

    def __exit__(self, *exc):
        self.model.attention_tap = None
        return False

    def hook(self, k, n_heads, shifted):
        """what block k of the armed model hands to block.fused_block as `tap`: None for a block that is not selected"""
        if k not in self.blocks:
            return None
        return lambda qkv: self._export(k, qkv, n_heads, shifted)

    def _export(self, k, qkv, n_heads, shifted):
        model = self.model
        if model.training:
            raise RuntimeError("AttentionTap exports eval-mode attention maps: the model was switched to train() while armed")
        key = (k, tuple(qkv.shape), qkv.dtype)
        out = self._static.get(key, (None, None))
        p, r = HF.attn_probs(model._attn_kind, qkv, model._mask_bits, n_heads, shifted, probs=self.want_probs,
                             received=self.want_received, out=out)
        self._static[key] = (p, r)
        if p is not None:
            self.probs[k] = p
        if r is not None:
            self.received[k] = r

    def clip_relevance(self, num_joints: Optional[int] = None) -> torch.Tensor:
        """(B, T, J) joint relevance of the last forward, each clip summing to 1 (fold_relevance); J = the raw joints of
        the model's part table (`num_joints`, or the largest index of the table + 1), or the K slots without one"""
        if not self.want_received:
            raise RuntimeError("clip_relevance needs AttentionTap(received=True)")
        index = self.model.part_index
        if index is not None and num_joints is None:
            if self._num_joints is None or self._num_joints[0] is not index:
                self._num_joints = (index, int(index.max()) + 1)
            num_joints = self._num_joints[1]
        return fold_relevance(self.received, self.model.temporal_dim, index, num_joints)
