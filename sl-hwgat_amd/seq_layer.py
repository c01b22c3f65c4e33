"""One post-norm Transformer encoder layer (reference hwgat/models/Transformer.py: MyTransformerEncoderLayer, the function of
nn.TransformerEncoderLayer(norm_first=False, activation=relu, batch_first=True)) as a single autograd node whose forward
and backward are sequences of HIP launches only, as block.py does for the HWGATE blocks.

forward  (4 GEMM launches, 1 attention, 2 LayerNorms):
    qkv  = x Wqkv^T + b                        in_proj (hwgat_linear_nt_*, epi 0)
    o    = attention(qkv, key padding)         hwgat_seq_attn_fwd (+ the log-sum-exp rows the backward needs)
    y1   = x + drop1(o Wo^T + b)               bias + dropout + residual in the GEMM epilogue (epi 1)
    x1   = LN1(y1)                             hwgat_ln_fwd
    u    = drop(relu(x1 W1^T + b))             epi 7: what is stored is also the backward's factor (u > 0) / (1 - p)
    y2   = x1 + drop2(u W2^T + b)              epi 1
    out  = LN2(y2)
saved: x, qkv, o, lse, y1, x1, u, y2 and the row statistics; dropout masks are recomputed (hash of seed, index).

backward (4 dW/db GEMMs, 4 dX GEMMs, attention backward, 2 LayerNorm backward launches):
    dy2, dy2m   = LN2 backward, and its copy masked by drop2 (hwgat_ln_bwd_masked)
    du          = dy2m W2 with epi 8 (x (u > 0) / (1 - p))         dW2 += dy2m^T u
    dx1         = du W1 + dy2 (epi 1 as a plain residual add)       dW1 += du^T x1
    dy1, dy1m   = LN1 backward (+ drop1 mask)
    do          = dy1m Wo                                          dWo += dy1m^T o
    dqkv        = hwgat_seq_attn_bwd                               dWqkv += dqkv^T x
    dx          = dqkv Wqkv + dy1
"""
import torch

from . import functional as HF
from ._lib import ptr, stream, dtype_code


def _ln_fwd(x, gamma, beta):
    d = x.shape[-1]
    n = x.numel() // d
    y = torch.empty_like(x)
    mean = torch.empty(n, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    HF.call("hwgat_ln_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), n, d, dtype_code(x), stream())
    return y, mean, rstd


class _EncoderLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad, cfg, w_qkv, b_qkv, w_o, b_o, w_1, b_1, w_2, b_2, g_1, be_1, g_2, be_2):
        n_heads, p, attn_p, seeds, seed_base, det, need_bwd = cfg
        dt = x.dtype
        c = lambda w: w if w.dtype == dt else w.to(dt)
        qkv = HF.linear_nt(x, c(w_qkv), b_qkv)
        drop = (seeds[3], attn_p, seed_base) if attn_p > 0.0 else None
        o, lse = HF.seq_attn_forward(qkv, pad, n_heads, drop, want_lse=need_bwd)
        y1 = HF.linear_nt(o, c(w_o), b_o, epi=HF.EPI_BIAS_DROP_RES, res=x, epi_seed=seeds[0], epi_p=p, seed_base=seed_base)
        x1, m1, r1 = _ln_fwd(y1, g_1, be_1)
        u = HF.linear_nt(x1, c(w_1), b_1, epi=HF.EPI_BIAS_RELU_DROP, epi_seed=seeds[1], epi_p=p, seed_base=seed_base)
        y2 = HF.linear_nt(u, c(w_2), b_2, epi=HF.EPI_BIAS_DROP_RES, res=x1, epi_seed=seeds[2], epi_p=p, seed_base=seed_base)
        out, m2, r2 = _ln_fwd(y2, g_2, be_2)
        ctx.save_for_backward(x, pad, qkv, o, lse, y1, m1, r1, x1, u, y2, m2, r2,
                              w_qkv, w_o, w_1, w_2, g_1, g_2)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, dout):
        (x, pad, qkv, o, lse, y1, m1, r1, x1, u, y2, m2, r2, w_qkv, w_o, w_1, w_2, g_1, g_2) = ctx.saved_tensors
        n_heads, p, attn_p, seeds, seed_base, det, _ = ctx.cfg
        dt = x.dtype
        dout = dout.contiguous()
        if dout.dtype != dt:
            dout = dout.to(dt)
        zeros = lambda t: torch.zeros(t.shape, device=t.device, dtype=torch.float32)
        d_qkv_w, d_qkv_b, d_o_w, d_o_b = zeros(w_qkv), zeros(w_qkv[:, 0]), zeros(w_o), zeros(w_o[:, 0])
        d_1_w, d_1_b, d_2_w, d_2_b = zeros(w_1), zeros(w_1[:, 0]), zeros(w_2), zeros(w_2[:, 0])
        d_g1, d_be1, d_g2, d_be2 = zeros(g_1), zeros(g_1), zeros(g_2), zeros(g_2)

        # the LayerNorm backward kernels make a masked copy only together with a residual gradient: one zero tensor,
        # shared by both LayerNorms of the layer
        zero_res = torch.zeros_like(dout) if p > 0.0 else None

        def ln_bwd(dy, xin, mean, rstd, gamma, dg, db, seed):       # -> dx and its masked copy (p = 0: dx itself)
            r = HF.ln_backward(dy, xin, mean, rstd, gamma, zero_res, dg, db, mask=(seed, p) if p > 0.0 else None,
                               seed_base=seed_base, deterministic=det)
            return r.dx, r.dx if r.dx_masked is None else r.dx_masked

        dy2, dy2m = ln_bwd(dout, y2, m2, r2, g_2, d_g2, d_be2, seeds[2])
        HF.linear_tn(dy2m, u, d_2_w, d_2_b, deterministic=det)
        du = HF.linear_nt(dy2m, HF.transpose(w_2, dt), None, epi=HF.EPI_RELU_BWD, aux=u, epi_p=p)
        HF.linear_tn(du, x1, d_1_w, d_1_b, deterministic=det)
        dx1 = HF.linear_nt(du, HF.transpose(w_1, dt), None, epi=HF.EPI_BIAS_DROP_RES, res=dy2)
        dy1, dy1m = ln_bwd(dx1, y1, m1, r1, g_1, d_g1, d_be1, seeds[0])
        HF.linear_tn(dy1m, o, d_o_w, d_o_b, deterministic=det)
        do = HF.linear_nt(dy1m, HF.transpose(w_o, dt), None)
        drop = (seeds[3], attn_p, seed_base) if attn_p > 0.0 else None
        dqkv = HF.seq_attn_backward(qkv, o, do, lse, pad, n_heads, drop)
        HF.linear_tn(dqkv, x, d_qkv_w, d_qkv_b, deterministic=det)
        dx = HF.linear_nt(dqkv, HF.transpose(w_qkv, dt), None, epi=HF.EPI_BIAS_DROP_RES, res=dy1)
        return (dx, None, None, d_qkv_w, d_qkv_b, d_o_w, d_o_b, d_1_w, d_1_b, d_2_w, d_2_b, d_g1, d_be1, d_g2, d_be2)


def encoder_layer(x, pad, layer, n_heads, p, attn_p, seeds, seed_base=None, deterministic=False):
    """one EncoderLayer container (models/Transformer.py) applied to x (B, T, d): the whole layer is one autograd node.
    `seeds` = the four dropout-site seeds (out_proj, linear1, linear2, attention probabilities), p / attn_p the rates
    (0 in eval), `seed_base` the device word of the step (None in eval)."""
    sa = layer.self_attn
    need_bwd = torch.is_grad_enabled() and (x.requires_grad or layer.linear1.weight.requires_grad)
    cfg = (int(n_heads), float(p), float(attn_p), tuple(int(s) for s in seeds), seed_base, bool(deterministic), need_bwd)
    return _EncoderLayer.apply(x.contiguous(), pad, cfg, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight,
                               sa.out_proj.bias, layer.linear1.weight, layer.linear1.bias, layer.linear2.weight,
                               layer.linear2.bias, layer.norm1.weight, layer.norm1.bias, layer.norm2.weight,
                               layer.norm2.bias)
