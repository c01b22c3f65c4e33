"""WGATE (windowed graph attention WITHOUT hierarchy) -- MI355X-native backend.

Drop-in for the reference's `hwgat/models/WGATE.py`: class `Model` takes the same
positional 15-tuple (`WGATEParams.get_model_params()`: integer `depths` / `num_heads`, no temporal patch
size), has the same `forward(x: (B,T,K,C)) -> (B,num_classes)` and the same `state_dict()` keys / shapes
-- `layers.{i}.<...>` directly (no stages) and the (nW, T*16, T*16) additive `adj_mask` buffer of
WGATE.py:190-196 -- so checkpoints interchange.

An attention window is one W-joint part window over ALL T frames.  The reference forms the dense
(T*W)^2 scores and adds 0 / -10000; its adjacency is block-tridiagonal over frames, so every masked
probability is exactly 0 in fp32 and `hwgat_band_attn_fwd/bwd` (csrc/band_attn.hip, W = 16) or
`hwgat_wband_attn_fwd/bwd` (csrc/wband_attn.hip, any other W <= 32) only ever touch the three
neighbouring key frames.  Embedding, LayerNorms, fused linears and the final norm + pool are the
kernels HWGATE uses, unchanged.  `adj_mask` is kept only for the state_dict contract; the kernels read
the mask rows derived from `adj_mat`.
"""
from torch import nn

from .. import functional as HF
from ._family import FamilyModel, _additive_mask
from .HWGATE import _SUPPORTED_WIDTHS


class Model(FamilyModel):
    _attn_kind = "band"

    def __init__(self, kp_dim=26, num_kps=64, temporal_dim=256, num_classes=1000, embed_dim=64, pe=False,
                 depths=16, num_heads=8, window_size=16, ff_ratio=4., adj_mat=None, drop_rate=0.,
                 attn_drop_rate=0., norm_layer=nn.LayerNorm, device=None) -> None:
        window_size = int(window_size)
        if not 1 <= window_size <= 32:
            raise NotImplementedError(f"window_size {window_size}: the WGATE HIP backend takes part windows of at most 32 "
                                      f"joints (one 32-slot frame per window in the band attention kernels)")
        super().__init__(kp_dim, num_kps, temporal_dim, num_classes, embed_dim, pe, int(depths), int(num_heads),
                         embed_dim, drop_rate, attn_drop_rate, ff_ratio, norm_layer)
        if window_size != 16:
            self._attn_kind = "wband"                  # W = 16 stays on the "band" kernels, unchanged
        if adj_mat is None:
            raise NotImplementedError("WGATE needs its (nW, T*W, T*W) adjacency (the reference dereferences it too)")
        assert num_kps % window_size == 0, "window size and number of kps are incompatible"
        d = embed_dim
        if d not in _SUPPORTED_WIDTHS or d % num_heads or (d // num_heads) not in (16, 32):
            raise NotImplementedError(f"width {d} / heads {num_heads} not supported by the HIP kernels "
                                      "(band attention: head_dim 16 or 32)")
        self.window_size = window_size
        self.n_windows = num_kps // window_size

        # either builder validates the structure its kernel relies on
        rows = (HF.band_mask_rows(adj_mat, temporal_dim) if window_size == 16
                else HF.wband_mask_rows(adj_mat, temporal_dim, window_size))
        if rows.shape[0] != self.n_windows:
            raise ValueError(f"adjacency has {rows.shape[0]} windows, num_kps / window_size = {self.n_windows}")
        self.adj_mask_name = "adj_mask"
        self.register_buffer("adj_mask", _additive_mask(adj_mat))              # (nW, T*W, T*W), WGATE.py:190-196
        self._build_input()
        self.layers = nn.ModuleList(self._new_block(d) for _ in range(self.depths))     # PartAttentionBlock, WGATE.py:150-160
        self._finish(adj_mat, rows, device)
