"""What HWGATE, HGATE, WGATE and GATE share: one base class on `DeviceSeeds, nn.Module`.

A model of the family is  embedding -> PartAttentionBlocks (block.fused_block, one attention kind from
functional.ATTN_KINDS) -> final LayerNorm + pool -> head.  The base owns the block container, the constructor pieces every
member runs, the block loop with its per-call HandOver and the pool tail; a subclass states its constructor signature and
refusals, its mask builder and extra buffers, and whether its blocks sit in stages (`layers[i].blocks[j]`, widths doubling
through TemporalMerging) or flat (`layers[k]`).  Registration order is the `state_dict` key order and the RNG draw order
of the reference classes, so every helper here registers in the order it is called.
"""
import math
from typing import List, Optional

import torch
from torch import nn

from .. import functional as HF
from ..block import fused_block
from ..seeding import DeviceSeeds


class _Slot(nn.Module):
    """parameter container (no forward of its own)"""


def _sinusoid(max_len, d):
    pe = torch.zeros(max_len, d)
    pos = torch.arange(0, max_len).unsqueeze(1)
    div = torch.exp(torch.arange(0, d, 2) * -(math.log(10000.0) / d))
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe.view(1, max_len, 1, d)


def _additive_mask(adj_mat):
    """the band models' `adj_mask` buffer (WGATE.py:190-196, GATE.py:142): 0 -> -10000, 1 -> 0"""
    return adj_mat.to(torch.float32).masked_fill(adj_mat == 0, float(-10000)).masked_fill(adj_mat == 1, float(0))


class FamilyModel(DeviceSeeds, nn.Module):
    _attn_kind = None           # a key of functional.ATTN_KINDS: set by the subclass (or its constructor, by window size)
    _staged = False             # True: layers[i].blocks[j] with TemporalMerging between stages; False: layers[k]

    def __init__(self, kp_dim, num_kps, temporal_dim, num_classes, embed_dim, pe, depths, num_heads, num_features,
                 drop_rate, attn_drop_rate, ff_ratio, norm_layer) -> None:
        """the fields every member has (`depths` / `num_heads`: lists per stage, or integers for a flat model); the
        subclass has run its own refusals that come first and goes on with _build_input, its blocks and _finish"""
        super().__init__()
        if not 0.0 <= float(attn_drop_rate) < 1.0:
            raise ValueError("attn_drop_rate must be in [0, 1)")
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("norm_layer must be nn.LayerNorm")
        self.kp_dim, self.num_kps, self.temporal_dim = kp_dim, num_kps, temporal_dim
        self.num_classes, self.embed_dim, self.pe = num_classes, embed_dim, pe
        self.depths, self.num_heads = depths, num_heads
        self.drop_rate, self.ff_ratio = float(drop_rate), ff_ratio
        self.attn_drop_rate = float(attn_drop_rate)      # nn.Dropout on the attention probabilities (HWGATE.py:78,112)
        self.num_features = num_features

    # ------------------------------------------------------------ construction
    def _build_input(self):
        self.B = nn.Parameter(torch.normal(0.0, 1.0, (self.embed_dim // 2, self.kp_dim)) * 10, requires_grad=False)
        if self.pe:
            self.pos_encoder = _Slot()
            self.pos_encoder.register_buffer("pe", _sinusoid(self.temporal_dim, self.embed_dim))

    def _new_block(self, d, order=("norm1", "attn", "norm2", "ff"), attn_mask=None):
        """one PartAttentionBlock container of width d; its members are created and registered in `order`
        ('attn_mask' in it registers the buffer, `attn_mask` or None)"""
        hidden = int(d * self.ff_ratio)
        blk = _Slot()
        for name in order:
            if name in ("norm1", "norm2"):
                setattr(blk, name, nn.LayerNorm(d))
            elif name == "attn":
                blk.attn = _Slot()
                blk.attn.qkv = nn.Linear(d, 3 * d)
                blk.attn.proj = nn.Linear(d, d)
            elif name == "ff":
                blk.ff = _Slot()
                blk.ff.fc1 = nn.Linear(d, hidden)
                blk.ff.fc2 = nn.Linear(hidden, d)
            elif name == "attn_mask":
                blk.register_buffer("attn_mask", attn_mask)
            else:
                raise ValueError(name)
        return blk

    def _finish(self, adj_mat, mask_bits, device, **pool_modules):
        """after the blocks: final norm, `pool_modules` (what the pool tail reads besides the norm), head, the Linear
        re-initialisation of the reference (HWGATE.py:333-340) and the option / seed fields"""
        self.norm = nn.LayerNorm(self.num_features)
        for name, module in pool_modules.items():
            setattr(self, name, module)
        self.head = nn.Linear(self.num_features, self.num_classes) if self.num_classes > 0 else nn.Identity()
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                nn.init.zeros_(m.bias)
        self.adj_mat = adj_mat
        # compact mask rows derived from the adjacency (+ shift structure); not part of state_dict
        self.register_buffer("_mask_bits", mask_bits, persistent=False)
        self.part_index: Optional[torch.Tensor] = None           # set by use_part_table()
        self.activation_dtype = torch.float32
        self.threshold_override: Optional[List[float]] = None    # tests: inject train thresholds
        self.attention_tap = None                                # explain.AttentionTap while armed (`with tap:`), else None
        self._init_device_seeds()
        if device is not None:
            self.to(device)

    # ------------------------------------------------------------ options
    def use_part_table(self, index: torch.Tensor):
        """accept raw (B,T,J,C) keypoints and gather joints on the device
        (replaces the host-side WindowCreate transform)."""
        assert index.numel() == self.num_kps
        self.register_buffer("_part_index", index.to(torch.int32).to(self.B.device), persistent=False)
        self.part_index = self._part_index
        return self

    def set_activation_dtype(self, dtype):
        assert dtype in (torch.float32, torch.bfloat16)
        self.activation_dtype = dtype
        return self

    # ------------------------------------------------------------ forward
    def _steps(self):
        """[(blk, n_heads, shifted, want_stats, merge_out)] in execution order: every block but the last feeds a
        LayerNorm (want_stats); the last block of every stage but the last stores merged where its epilogue can"""
        if not self._staged:
            return [(blk, self.num_heads, False, k < self.depths - 1, False) for k, blk in enumerate(self.layers)]
        n_blocks = sum(len(stage.blocks) for stage in self.layers)
        steps = []
        for i, stage in enumerate(self.layers):
            for j, blk in enumerate(stage.blocks):
                steps.append((blk, self.num_heads[i], j % 2 == 1, len(steps) < n_blocks - 1,
                              j == len(stage.blocks) - 1 and i < len(self.layers) - 1))
        return steps

    def block_list(self):
        """every PartAttentionBlock container in execution order (what functional.weight_prep derives the copies of)"""
        return [step[0] for step in self._steps()]

    def _block(self, h, blk, n_heads, shifted, thr, k, hand):
        """one PartAttentionBlock (HWGATE.py:189-221) = one fused autograd node (block.fused_block).  `hand` is the
        HandOver of THIS forward call: what the previous block's epilogues produced for this one (LayerNorm statistics of
        h, the carrier of the dropout-masked gradient) goes in, what this block produces for the next one comes out --
        explicit values held in a local of _run_blocks, nothing stored on the module.  Returns the block output
        (B,F,K,d) -- or, for the last block of a stage when the fc2 epilogue can do it, already in the TemporalMerging
        layout (B,F/2,K,2d) (_run_blocks checks the shape)."""
        p = self.drop_rate if self.training else 0.0
        h = h.contiguous()
        have = hand.stats if hand.of is h else None
        carrier, up = (hand.carrier, hand.up) if (hand.of is h and hand.carrier is not None) else (None, None)
        want, merge = hand.plan.get(k, (False, False))
        seeds = self._site_seeds(k)
        tap = getattr(self, "attention_tap", None)               # a model unpickled from before the field existed has none
        out, st, oc = fused_block(h, thr, blk, self._mask_bits, n_heads, shifted, p, seeds, self._attn_kind,
                                  stats=have, want_stats=want, merge_out=merge, return_stats=True,
                                  carrier=carrier, up=up, carry_out=(want or k == hand.last_block) and not merge,
                                  return_carrier=True, book=hand.book, deterministic=hand.deterministic,
                                  attn_p=self.attn_drop_rate if self.training else 0.0,
                                  prep=hand.prep.per_block[k] if hand.prep is not None else None,
                                  seed_base=hand.seed_base, deterministic_backward=hand.deterministic and self.training,
                                  tap=None if tap is None else tap.hook(k, n_heads, shifted))
        hand.of, hand.stats, hand.carrier, hand.up = out, st, oc, ((seeds[2], p) if oc is not None else None)
        return out

    def _embed(self, x):
        if x.dim() != 4 or x.shape[1] != self.temporal_dim or x.shape[3] != self.kp_dim:
            raise ValueError(f"expected (B,{self.temporal_dim},K,{self.kp_dim}) keypoints, got {tuple(x.shape)}")
        idx = None
        if x.shape[2] != self.num_kps:
            if self.part_index is None:
                raise ValueError(f"got {x.shape[2]} joints, model has {self.num_kps} slots and no part table")
            idx = self.part_index
        x = self._input_view(x.contiguous().float())      # the modality sees the raw joints, in front of the part gather
        pe = self.pos_encoder.pe.view(self.temporal_dim, self.embed_dim) if self.pe else None
        seed_base = self._next_step_seed() if self.training else None     # this call's base seed: _call_base
        p_pe = self.drop_rate if (self.training and self.pe) else 0.0     # Dropout lives in PositionalEncoding
        return HF.embed(x, idx, self.B, pe, self.num_kps, self.activation_dtype, p_pe, self._site_seeds(63)[0],
                        seed_base=seed_base)

    def _run_blocks(self, h, steps):
        """run `steps` (see _steps) on the embedding h of this call; returns (h, the call's HandOver)"""
        hand = HF.HandOver(last_block=len(steps) - 1, deterministic=self._deterministic())
        # every derived copy of the block weights this call needs (LayerNorm folds, bf16 copies, transposes for the backward)
        hand.prep = HF.weight_prep(self, [step[0] for step in steps], self.activation_dtype, torch.is_grad_enabled())
        hand.seed_base = self._call_base if self.training else None       # the copy _embed took (DeviceSeeds._next_step_seed)
        for k, (_, _, _, want_stats, merge_out) in enumerate(steps):
            hand.plan[k] = (want_stats, merge_out)
        draw = self.training and HF.ATTN_KINDS[self._attn_kind].takes_thr     # only the part-window kinds have a threshold drop
        for k, (blk, n_heads, shifted, _, merge_out) in enumerate(steps):
            thr = None
            if draw and self.threshold_override is not None:
                thr = torch.full((1,), float(self.threshold_override[k]), device=h.device)
            elif draw:
                thr = torch.rand(1, device=h.device)          # device RNG, no host sync
            d = h.shape[-1]
            h = self._block(h, blk, n_heads, shifted, thr, k, hand)
            if merge_out and h.shape[-1] == d:
                h = HF.temporal_merge(h)                      # the fc2 epilogue could not store merged (ragged M)
        return h, hand

    def _pool(self, h, hand, pool, *pool_weights):
        """final LayerNorm + `pool` (functional.ln_mean_pool, or ln_weighted_pool with its weights) over the tokens"""
        if hand.of is h and hand.carrier is not None:
            return pool(h, self.norm.weight, self.norm.bias, *pool_weights, carrier=hand.carrier, up=hand.up,
                        book=hand.book, deterministic=hand.deterministic, seed_base=hand.seed_base)
        return pool(h, self.norm.weight, self.norm.bias, *pool_weights, deterministic=hand.deterministic)

    def forward_features(self, x):
        h, hand = self._run_blocks(self._embed(x), self._steps())
        return self._pool(h, hand, HF.ln_mean_pool)

    def forward(self, x):
        feat = self.forward_features(x)
        return self._classify(self.head, feat)
