"""GATE (plain graph-masked attention over all T*K tokens, no windows, no hierarchy) -- MI355X-native backend.

Drop-in for the reference's `hwgat/models/GATE.py`: class `Model` takes the same positional 14-tuple
(`GATEParams.get_model_params()`), has the same `forward(x: (B,T,K,C)) -> (B,num_classes)` and the same
`state_dict()` keys / shapes -- `layers.{i}.<...>`, the (1, 1, T*K, T*K) additive `adj_mask` buffer of GATE.py:142-151
and `weightedAvg.{weight (1, T*K), bias (1)}` -- so checkpoints interchange.

The reference forms dense (T*K)^2 scores per head and adds 0 / -10000; its adjacency (model_params.py:60-73) is
block-tridiagonal over frames -- the joint graph inside a frame, the same joint in frames f-1 and f+1, no self loop --
so every masked probability is exactly 0 in fp32 and `hwgat_wband_attn_fwd/bwd` (csrc/wband_attn.hip) only ever touch
the three neighbouring key frames: a frame of K <= 32 joints is one "window" of the wide band kernels WGATE uses for
window sizes other than 16.  The final norm + `weightedAvg` over the token axis (GATE.py:208-210) is
`functional.ln_weighted_pool`; embedding, LayerNorms and fused linears are the kernels HWGATE uses, unchanged.
`adj_mask` is kept only for the state_dict contract; the kernels read the mask words derived from `adj_mat`.
"""
from torch import nn

from .. import functional as HF
from ._family import FamilyModel, _additive_mask
from .HWGATE import _SUPPORTED_WIDTHS


class Model(FamilyModel):
    _attn_kind = "wband"

    def __init__(self, kp_dim=26, num_kps=29, temporal_dim=256, num_classes=1000, embed_dim=64, pe=False, depths=16,
                 num_heads=8, ff_ratio=4., adj_mat=None, drop_rate=0., attn_drop_rate=0., norm_layer=nn.LayerNorm,
                 device=None) -> None:
        if not 1 <= int(num_kps) <= 32:
            raise NotImplementedError(f"num_kps {num_kps}: the GATE HIP backend takes frames of at most 32 joints (one "
                                      f"32-slot frame in the wide band attention kernels)")
        super().__init__(kp_dim, int(num_kps), temporal_dim, num_classes, embed_dim, pe, int(depths), int(num_heads),
                         embed_dim, drop_rate, attn_drop_rate, ff_ratio, norm_layer)
        if adj_mat is None:
            raise NotImplementedError("GATE needs its (T*K, T*K) adjacency (the reference dereferences it too)")
        d = embed_dim
        if d not in _SUPPORTED_WIDTHS or d % num_heads or (d // num_heads) not in (16, 32):
            raise NotImplementedError(f"width {d} / heads {num_heads} not supported by the HIP kernels (width in "
                                      f"{_SUPPORTED_WIDTHS}; wide band attention: head_dim 16 or 32)")
        self.window_size = self.num_kps                        # one window = all joints of a frame
        self.n_windows = 1

        rows = HF.wband_mask_rows(adj_mat, temporal_dim, self.num_kps)     # validates the structure the kernel relies on
        self.adj_mask_name = "adj_mask"
        self.register_buffer("adj_mask", _additive_mask(adj_mat).unsqueeze(0).unsqueeze(0))    # (1, 1, T*K, T*K), GATE.py:142
        self._build_input()
        self.layers = nn.ModuleList(self._new_block(d) for _ in range(self.depths))     # AttentionBlock, GATE.py:111-116
        # weightedAvg runs over the TOKEN axis (GATE.py:181,210)
        self._finish(adj_mat, rows, device, weightedAvg=nn.Linear(temporal_dim * self.num_kps, 1))

    def forward_features(self, x):
        h, hand = self._run_blocks(self._embed(x), self._steps())
        return self._pool(h, hand, HF.ln_weighted_pool, self.weightedAvg.weight, self.weightedAvg.bias)
