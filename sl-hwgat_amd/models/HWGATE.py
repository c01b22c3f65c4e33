"""HWGAT (hierarchical windowed graph attention) -- MI355X-native backend.

Drop-in for the reference's `hwgat/models/HWGATE.py`: class `Model` takes the
same positional 16-tuple (`HWGATEParams.get_model_params()`), has the same
`forward(x: (B,T,K,C)) -> (B,num_classes)`, is an `nn.Module` that takes part
in autograd, and exposes the same `state_dict()` keys/shapes,
so reference checkpoints load here and vice versa.

Inside, nothing is shared with the reference's formulation: activations stay
in natural (B,F,K,d) order for the whole network, window partition / reverse /
roll never materialise, and the attention core, LayerNorms, embedding, merging
and final pooling run as hand-written gfx950 kernels (libhwgat_hip.so).  There
is no CPU path: constructing on / moving to a CPU device works (parameters are
ordinary tensors) but `forward` needs an MI355X.
"""
import torch
from torch import nn

from .. import functional as HF
from ._family import FamilyModel, _Slot, _sinusoid  # noqa: F401  (tests and tools import _Slot / _sinusoid from here)

_SUPPORTED_WIDTHS = (128, 256, 512, 1024)         # HGATE / WGATE: the widths their kernels take
MAX_WIDTH = 1024                                 # HWGATE: every multiple of 64 up to this (width_problem)


def width_problem(d, hidden, n_heads, window_size):
    """why the HWGATE kernels cannot run a stage of width d, FFN hidden width `hidden` and `n_heads` heads (None: they
    can).  The linears tile their outputs in 64-column blocks, the LayerNorm row maps take every d = 64 n <= 1024, the
    attention kernels head_dim 32 / 64 (and 128 with window_size 16)."""
    if d % 64:
        return f"stage width {d} is not a multiple of 64 (the linears and LayerNorms tile rows in 64-wide blocks)"
    if d > MAX_WIDTH:
        return f"stage width {d} is above {MAX_WIDTH} (the LayerNorm row maps end there)"
    if hidden % 64:
        return f"FFN hidden width int({d} * ff_ratio) = {hidden} is not a multiple of 64"
    if d % n_heads:
        return f"stage width {d} is not divisible by {n_heads} heads"
    hd = d // n_heads
    if window_size == 16 and hd not in (32, 64, 128):
        return f"head_dim {hd} (width {d} / {n_heads} heads): the window attention kernels take head_dim 32, 64 or 128"
    if window_size != 16 and hd not in (32, 64):
        return (f"head_dim {hd} with window_size {window_size}: the part-window attention kernels for window sizes "
                f"other than 16 take head_dim 32 or 64 (128 only with window_size 16)")
    return None


def _last_slot_mask(frames, n_windows, window_size=16):
    """value of the reference's `attn_mask` buffer (HWGATE.py:169-187): all
    ones except the last temporal slot, which is block-diagonal per frame."""
    f, n = frames // 2, 2 * window_size
    m = torch.ones(f, n_windows, n, n)
    blk = torch.zeros(n, n)
    blk[:window_size, :window_size] = 1
    blk[window_size:, window_size:] = 1
    m[f - 1] = blk
    return m.view(f * n_windows, n, n)


class Model(FamilyModel):
    _attn_kind = "win"          # part-window attention (hwgat_win_attn_*); an HWGATE with window_size != 16 sets "pwin"
                                # on the instance (hwgat_pwin_attn_*)
    _staged = True

    def __init__(self, kp_dim=26, num_kps=64, temporal_dim=256, num_classes=1000, embed_dim=64,
                 temporal_patch_size=4, pe=False, depths=[2, 2, 6, 2], num_heads=[2, 4, 8, 16],
                 window_size=16, adj_mat=None, drop_rate=0., attn_drop_rate=0., ff_ratio=4.,
                 norm_layer=nn.LayerNorm, device=None) -> None:
        if temporal_patch_size != 2:
            # the reference's TemporalMerging doubles the width per stage, which is only
            # consistent with temporal_patch_size == 2 (HWGATE.py:61 vs :312)
            raise NotImplementedError(f"HWGAT HIP backend supports temporal_patch_size == 2, got {temporal_patch_size} "
                                      f"(Model() with every constructor default is refused: its default is "
                                      f"temporal_patch_size=4; HWGATEParams passes 2)")
        if not 1 <= window_size <= 32:
            raise NotImplementedError(f"window_size {window_size}: the HWGAT HIP backend takes windows of at most 32 "
                                      f"joints (2 frames x 32 = 64 tokens per window)")
        n_stage = len(depths)
        super().__init__(kp_dim, num_kps, temporal_dim, num_classes, embed_dim, pe, list(depths), list(num_heads),
                         int(embed_dim * 2 ** (n_stage - 1)), drop_rate, attn_drop_rate, ff_ratio, norm_layer)
        assert num_kps % window_size == 0, "window size and number of kps are incompatible"
        assert temporal_dim % (2 ** n_stage) == 0, "temporal dimension must be divisible by 2**stages"
        assert embed_dim % 2 == 0
        self.num_layers = n_stage
        self.window_size = int(window_size)
        self.n_windows = num_kps // window_size
        if window_size != 16:
            self._attn_kind = "pwin"                   # W = 16 stays on the "win" kernels, unchanged

        self._build_input()
        self.layers = nn.ModuleList()
        for i in range(n_stage):
            d = embed_dim * 2 ** i
            why = width_problem(d, int(d * ff_ratio), num_heads[i], window_size)
            if why is not None:
                raise NotImplementedError(f"stage {i}: {why}.  HWGATE takes stage widths d = embed_dim * 2**i that are "
                                          f"multiples of 64 up to {MAX_WIDTH}, with int(d * ff_ratio) a multiple of 64")
            stage = _Slot()
            stage.blocks = nn.ModuleList(
                self._new_block(d, ("norm1", "attn", "norm2", "ff", "attn_mask"),
                                _last_slot_mask(temporal_dim // 2 ** i, self.n_windows, window_size) if j % 2 == 1 else None)
                for j in range(depths[i]))
            self.layers.append(stage)

        if adj_mat is None:
            adj_mat = torch.ones(self.n_windows, 2 * window_size, 2 * window_size)
        bits = HF.mask_bits(adj_mat) if self._attn_kind == "win" else HF.pwin_mask_bits(adj_mat, window_size)
        if bits.shape[1] != self.n_windows:
            raise ValueError(f"adjacency has {bits.shape[1]} windows, num_kps / window_size = {self.n_windows}")
        self._finish(adj_mat, bits, device)
