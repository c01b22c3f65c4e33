"""MI355X (gfx950) backend of the Transformer baseline.

Drop-in for the reference's `hwgat/models/Transformer.py`: class `Model` takes the same positional arguments
(input_dim, nclass, pad_index, d_model, nhead, dim_feedforward, num_encoder_layers, dropout, max_len, pool), as
`TransformerParams.get_model_params()` returns them, and its `state_dict()` has the reference's keys, order, shapes and
dtypes (checkpoints and optimizer state interchange).  The forward runs on HIP kernels only:

    embed      hwgat_seq_embed_fwd: (x W^T + b) sqrt(d) + pe, PE dropout and the key-padding bits in one launch
    layers     seq_layer.encoder_layer: one autograd node per post-norm encoder layer (NT linears with fused epilogues,
               hwgat_seq_attn_* dense key-padded attention, LayerNorm kernels)
    norm+pool  mean: hwgat_lnpool (final LayerNorm + mean over ALL T frames, padded ones included, as the reference);
               max: LayerNorm + hwgat_seq_maxpool; concat: LayerNorm, flattened (B, T d)
    classifier nn.Linear (nn.Sequential(nn.Linear) for concat), as in the other models

Supported: head_dim = d_model / nhead = 64, d_model a multiple of 64 up to 1024, dim_feedforward a multiple of 64,
max_len <= 512, pool in {'mean', 'max', 'concat'}; anything else is refused at construction.
"""
import math

import torch
from torch import nn

from .. import functional as HF
from ..seeding import DeviceSeeds
from ..seq_layer import encoder_layer

POOLS = ("mean", "max", "concat")
EMBED_SITE = 63         # the embed's dropout site: _site_seeds(63)[0]; layer k uses sites 4k .. 4k+3 of _site_seeds(k)
MAX_LAYERS = EMBED_SITE


def shape_problem(input_dim, d_model, nhead, dim_feedforward, max_len, pool, num_layers=1):
    """None, or the message naming the rule a configuration breaks"""
    if pool not in POOLS:
        return f"pool {pool!r}: the Transformer backend pools with one of {POOLS}"
    if d_model % 64 or d_model > 1024 or d_model <= 0:
        return f"d_model {d_model}: the Transformer backend takes multiples of 64 up to 1024"
    if nhead <= 0 or d_model % nhead or d_model // nhead != 64:
        return (f"head_dim {d_model / nhead if nhead else 'undefined'} (d_model {d_model} / nhead {nhead}): the "
                f"sequence attention kernels take head_dim 64 only")
    if dim_feedforward % 64 or dim_feedforward <= 0:
        return f"dim_feedforward {dim_feedforward}: the Transformer backend takes multiples of 64"
    if max_len > HF.SEQ_MAX_LEN or max_len <= 0:
        return f"max_len {max_len}: the sequence attention kernels take at most {HF.SEQ_MAX_LEN} frames"
    if num_layers > MAX_LAYERS or num_layers <= 0:
        return (f"num_encoder_layers {num_layers}: at most {MAX_LAYERS} (dropout site seeds of layers 0 .. 62 and the embed, "
                f"site 63, are disjoint)")
    if input_dim <= 0 or input_dim > 512:
        return f"input_dim {input_dim}: the frame embedding takes 1 to 512 features per frame"
    return None


class PositionalEncoding(nn.Module):
    """the `pe` buffer (1, max_len, d) of the reference's PositionalEncoding; its dropout runs in the embed kernel"""

    def __init__(self, d_model, max_len):
        super().__init__()
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.unsqueeze(0))


class EncoderLayer(nn.Module):
    """parameter container of one reference MyTransformerEncoderLayer (same attribute names, same order); the arithmetic
    is seq_layer.encoder_layer.  nn.MultiheadAttention only holds in_proj_* / out_proj (its forward is never called)."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)


class Encoder(nn.Module):
    def __init__(self, d_model, nhead, dim_feedforward, num_layers, dropout):
        super().__init__()
        self.layers = nn.ModuleList([EncoderLayer(d_model, nhead, dim_feedforward, dropout) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = nn.LayerNorm(d_model)


class Model(DeviceSeeds, nn.Module):
    def __init__(self, input_dim, nclass, pad_index=-1, d_model=512, nhead=8, dim_feedforward=2048, num_encoder_layers=6,
                 dropout=0.1, max_len=512, pool='concat') -> None:
        super().__init__()
        problem = shape_problem(input_dim, d_model, nhead, dim_feedforward, max_len, pool, num_encoder_layers)
        if problem is not None:
            raise NotImplementedError(problem)
        self.model_type = 'MyTransformerClassifier'
        self.input_dim = input_dim
        self.d_model = d_model
        self.nhead = nhead
        self.max_len = max_len
        self.pad_index = pad_index
        self.drop_rate = float(dropout)
        self.encoder = nn.Linear(input_dim, d_model)
        self.pos_encoder = PositionalEncoding(d_model, max_len)
        self.transformer_encoder = Encoder(d_model, nhead, dim_feedforward, num_encoder_layers, dropout)
        self.pool = pool
        if pool == 'concat':
            self.classifier = nn.Sequential(nn.Linear(d_model * max_len, nclass))
        else:
            self.classifier = nn.Linear(d_model, nclass)
        for p in self.parameters():          # the reference's _reset_parameters
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.activation_dtype = torch.float32
        self._init_device_seeds()

    def set_activation_dtype(self, dtype):
        assert dtype in (torch.float32, torch.bfloat16)
        self.activation_dtype = dtype
        return self

    def _embed(self, x):
        seed_base = self._next_step_seed() if self.training else None     # this call's base seed: _call_base
        p = self.drop_rate if self.training else 0.0
        T = x.shape[1]
        pe = self.pos_encoder.pe[0, :T]
        return _Embed.apply(x, self.encoder.weight, self.encoder.bias, pe, self.activation_dtype, self.pad_index, p,
                            self._site_seeds(EMBED_SITE)[0], seed_base)

    def forward_features(self, src):
        B, T = src.shape[0], src.shape[1]
        if getattr(self, "input_modality", None) is not None:
            if src.dim() != 4:
                raise ValueError(f"an input modality needs (B, T, K, C) keypoints, got {tuple(src.shape)}: flattened frames "
                                 "do not say which words are a joint's coordinates")
            src = self._input_view(src.contiguous().float(), pad_value=self.pad_index)   # padded frames keep their marker
        x = src.reshape(B, T, -1)
        if x.shape[2] != self.input_dim:
            raise ValueError(f"expected {self.input_dim} features per frame, got {x.shape[2]} (input {tuple(src.shape)})")
        if T > self.max_len:
            raise ValueError(f"{T} frames: the model was built for at most max_len = {self.max_len}")
        if self.pool == 'concat' and T != self.max_len:
            raise ValueError(f"pool 'concat' needs exactly max_len = {self.max_len} frames, got {T}")
        x = x.contiguous().float()
        h, pad = self._embed(x)
        det = self._deterministic()
        p = self.drop_rate if self.training else 0.0
        seed_base = self._call_base if self.training else None         # the copy _embed took (DeviceSeeds._next_step_seed)
        for k, layer in enumerate(self.transformer_encoder.layers):
            h = encoder_layer(h, pad, layer, self.nhead, p, p, self._site_seeds(k), seed_base, det and self.training)
        norm = self.transformer_encoder.norm
        if self.pool == 'mean':
            return HF.ln_mean_pool(h, norm.weight, norm.bias, deterministic=det)
        hn = HF.layer_norm(h, norm.weight, norm.bias, deterministic=det and self.training)
        if self.pool == 'max':
            return HF.seq_max_pool(hn)
        return hn.reshape(B, T * self.d_model).float()

    def forward(self, src):
        return self._classify(self.classifier, self.forward_features(src))


class _Embed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, pe, dtype, pad_index, p, seed, seed_base):
        out, pad = HF.seq_embed(x, HF.transpose(W), b, pe.contiguous(), dtype, pad_index, p, seed, seed_base)
        ctx.mark_non_differentiable(pad)
        ctx.save_for_backward(x)
        ctx.cfg = (W.shape, p, seed, seed_base)
        return out, pad

    @staticmethod
    def backward(ctx, dout, _dpad):
        (x,) = ctx.saved_tensors
        shape, p, seed, seed_base = ctx.cfg
        dW = torch.zeros(shape, device=x.device, dtype=torch.float32)
        db = torch.zeros(shape[0], device=x.device, dtype=torch.float32)
        HF.seq_embed_backward(dout.contiguous(), x, dW, db, p, seed, seed_base)
        return None, dW, db, None, None, None, None, None, None
