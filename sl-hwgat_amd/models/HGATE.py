"""HGATE (hierarchical graph attention WITHOUT body-part windows) -- MI355X-native backend.

Drop-in for the reference's `hwgat/models/HGATE.py`: class `Model` takes the same
positional 15-tuple (`HGATEParams.get_model_params()`, no `window_size`), has the same
`forward(x: (B,T,K,C)) -> (B,num_classes)` and the same `state_dict()` keys / shapes -- including the odd
blocks' `attn_mask` buffers of shape (F/2, 2K, 2K) (HGATE.py:154-172) -- so checkpoints interchange.

Relative to HWGATE only the attention core differs: a block is 2 frames x ALL K joints (K <= 32; 29 in
HGATEParams), one (2K, 2K) adjacency for every block, and no train-mode threshold (HGATE.py:84-108).
It runs on `hwgat_blk_attn_fwd/bwd` (csrc/blk_attn.hip); embedding, LayerNorms, the fused linears,
TemporalMerging and the final norm + pool are the kernels HWGATE uses, unchanged.
"""
import torch
from torch import nn

from .. import functional as HF
from ._family import FamilyModel, _Slot
from .HWGATE import _SUPPORTED_WIDTHS


def _last_block_mask(frames, n_joints):
    """value of the reference's `attn_mask` buffer (HGATE.py:154-172): ones, except the last block,
    where only same-frame pairs are allowed."""
    f, K = frames // 2, n_joints
    m = torch.ones(f, 2 * K, 2 * K)
    blk = torch.zeros(2 * K, 2 * K)
    blk[:K, :K] = 1
    blk[K:, K:] = 1
    m[f - 1] = blk
    return m


class Model(FamilyModel):
    _attn_kind = "blk"
    _staged = True

    def __init__(self, kp_dim=26, num_kps=64, temporal_dim=256, num_classes=1000, embed_dim=64,
                 temporal_patch_size=4, pe=False, depths=[2, 2, 6, 2], num_heads=[2, 4, 8, 16],
                 adj_mat=None, drop_rate=0., attn_drop_rate=0., ff_ratio=4., norm_layer=nn.LayerNorm,
                 device=None) -> None:
        if temporal_patch_size != 2:
            raise NotImplementedError("HGATE HIP backend supports temporal_patch_size == 2")
        n_stage = len(depths)
        super().__init__(kp_dim, num_kps, temporal_dim, num_classes, embed_dim, pe, list(depths), list(num_heads),
                         int(embed_dim * 2 ** (n_stage - 1)), drop_rate, attn_drop_rate, ff_ratio, norm_layer)
        if not 1 <= num_kps <= 32:
            raise NotImplementedError("HGATE HIP backend supports at most 32 joints per frame (2 x 32-row MFMA tiles)")
        assert temporal_dim % (2 ** n_stage) == 0, "temporal dimension must be divisible by 2**stages"
        assert embed_dim % 2 == 0
        self.num_layers = n_stage

        self._build_input()
        self.layers = nn.ModuleList()
        for i in range(n_stage):
            d = embed_dim * 2 ** i
            if d not in _SUPPORTED_WIDTHS or d % num_heads[i] or (d // num_heads[i]) not in (32, 64):
                raise NotImplementedError(
                    f"stage width {d} / heads {num_heads[i]} not supported by the HIP kernels: widths must be in "
                    f"{_SUPPORTED_WIDTHS} (the linears tile their output in 128- / 256-column blocks and the LayerNorm "
                    f"row maps exist for these widths; embed_dim = 64, the reference constructor's default that no "
                    f"reference config uses, would need 64-column instantiations -- INTEGRATION.md section 6) and "
                    f"head_dim in (32, 64)")
            stage = _Slot()
            stage.blocks = nn.ModuleList(                # registration order of HGATE.py:150-174 (state_dict key order)
                self._new_block(d, ("norm1", "norm2", "ff", "attn_mask", "attn"),
                                _last_block_mask(temporal_dim // 2 ** i, num_kps) if j % 2 == 1 else None)
                for j in range(depths[i]))
            self.layers.append(stage)

        if adj_mat is None:
            adj_mat = torch.ones(2 * num_kps, 2 * num_kps)
        self._finish(adj_mat, HF.blk_mask_bits(adj_mat, num_kps), device)

    def use_part_table(self, index):
        raise NotImplementedError("HGATE takes the raw (B,T,K,C) joints; there are no part windows to gather")
