"""One ST-GCN block (reference hwgat/models/STGCN.py: STGCN_BLOCK) as a single autograd node whose forward and backward
are sequences of HIP launches only, plus the two small nodes around the stack (the input BatchNorm and the pooled head
dropout).  Activations are fp32, channels-last (N, T, V, C).

forward of a block (C_in -> C_out, temporal stride s):
    y   = x Wg^T + bg                              1x1 conv to 3 C_out channels (hwgat_stgcn_conv, 1 tap)
    a   = sum_{k,v} (A o E)[k,v,w] y[..,v,k,:]     hwgat_stgcn_agg_fwd
    h   = relu(BN1(a))                             hwgat_stgcn_bn_stats + hwgat_stgcn_bn_apply
    c   = tconv9(h; Wt, bt, stride s, pad 4)       hwgat_stgcn_conv, 9 taps
    out = relu(BN2(c) + r)                         r = 0 | x | BNr(x Wr^T + br, stride s)
The projection runs BEFORE the aggregation, as in the reference: the bias then stays a plain per-channel bias (behind the
aggregation it would turn into a per-joint table that feeds d edge_importance), and block 0 (2 or 3 input channels,
zero-padded to 32) needs no kernel of its own.  The price is a 3 C_out wide intermediate instead of 3 C_in.
saved: x (padded), y, a, h, c, rc, out and the six column statistics.

backward: BN backward (gated by the ReLU output) -> conv dW / db / dX -> BN backward -> aggregation backward (dy and
d edge_importance) -> projection dW / db / dX, the residual gradient added in that last launch's epilogue.  Every sum
over rows goes through partial images added in a fixed order: two backward runs are bit-identical.
"""
import torch

from . import functional as HF

RES_NONE, RES_IDENTITY, RES_CONV = 0, 1, 2


def _bn_stats(x, bn, training):
    if training:
        return HF.stgcn_bn_stats(x, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)
    return HF.stgcn_bn_eval_stats(bn.running_mean, bn.running_var, bn.eps)


# The three launch sequences that the ST-GCN block and the DecoupledGCN unit (dgcn_block._Unit) have in common.
def pad_channels(x):
    """x with its channels zero-padded to a multiple of 32 (x itself when they are one)"""
    CinP = HF.pad32(x.shape[3])
    return x if CinP == x.shape[3] else HF.stgcn_copy_cols(x, CinP)


def project(xp, wg, bg):
    """the 1x1 projection of the padded input by the master weight wg (3 C_out, C_in, 1, 1) and bias bg"""
    return HF.stgcn_conv(xp, HF.stgcn_weight_image(wg, 0, xp.shape[3]), bg)


def residual_forward(res, x, xp, wr, br, gr, ber, bnr, stride, training):
    """(r, rbn): the residual operand (None | x | the strided 1x1 convolution of xp) and, for RES_CONV, the (mean, rstd,
    gamma, beta) of its BatchNorm, which the block's last launch applies while it adds"""
    if res == RES_CONV:
        rc = HF.stgcn_conv(xp, HF.stgcn_weight_image(wr, 0, xp.shape[3]), br, stride, 0)
        return rc, _bn_stats(rc, bnr, training) + (gr, ber)
    return (x if res == RES_IDENTITY else None), None


def crop_dx(dx, Cin):
    """the input gradient without the padding channels of pad_channels"""
    return dx if dx.shape[3] == Cin else HF.stgcn_copy_cols(dx, Cin)


class _Block(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, E, wg, bg, g1, b1, wt, bt, g2, b2, wr, br, gr, ber):
        A, stride, res, training, bn1, bn2, bnr = cfg
        Cin = x.shape[3]
        xp = pad_channels(x)
        y = project(xp, wg, bg)
        a = HF.stgcn_aggregate(y, A, E)
        m1, r1 = _bn_stats(a, bn1, training)
        h = HF.stgcn_bn_apply(a, m1, r1, g1, b1, relu=True)
        c = HF.stgcn_conv(h, HF.stgcn_weight_image(wt, 0), bt, stride, wt.shape[2] // 2)
        m2, r2 = _bn_stats(c, bn2, training)
        r, rbn = residual_forward(res, x, xp, wr, br, gr, ber, bnr, stride, training)
        rc, mr, rr = (r, rbn[0], rbn[1]) if rbn else (None, None, None)
        out = HF.stgcn_bn_apply(c, m2, r2, g2, b2, relu=True, res=r, res_bn=rbn)
        ctx.save_for_backward(xp, y, a, h, c, rc, out, m1, r1, m2, r2, mr, rr, E, wg, g1, wt, g2, wr, gr)
        ctx.cfg = (A, stride, res, training, Cin)
        return out

    @staticmethod
    def backward(ctx, dout):
        xp, y, a, h, c, rc, out, m1, r1, m2, r2, mr, rr, E, wg, g1, wt, g2, wr, gr = ctx.saved_tensors
        A, stride, res, training, Cin = ctx.cfg
        dout = dout.contiguous()
        N, T, V, CinP = xp.shape
        pad = wt.shape[2] // 2
        # the last ReLU gates everything behind it: the BatchNorm backward kernels take its output as the gate
        dc, d_g2, d_b2 = HF.stgcn_bn_backward(dout, out, c, m2, r2, g2, training)
        d_wr = d_br = d_gr = d_ber = dx_res = None
        if res == RES_CONV:
            drc, d_gr, d_ber = HF.stgcn_bn_backward(dout, out, rc, mr, rr, gr, training)
            d_wr = HF.stgcn_conv_dw(xp, drc, wr.shape, stride, 0)
            d_br = HF.stgcn_colsum(drc)
            dx_res = HF.stgcn_conv_dx(drc, HF.stgcn_weight_image(wr, 1, CinP), T, stride, 0)
        d_wt = HF.stgcn_conv_dw(h, dc, wt.shape, stride, pad)
        d_bt = HF.stgcn_colsum(dc)
        dh = HF.stgcn_conv_dx(dc, HF.stgcn_weight_image(wt, 1), T, stride, pad)
        da, d_g1, d_b1 = HF.stgcn_bn_backward(dh, h, a, m1, r1, g1, training)
        dy, dE = HF.stgcn_aggregate_backward(y, da, A, E, E is not None and ctx.needs_input_grad[2])
        d_wg = HF.stgcn_conv_dw(xp, dy, wg.shape, 1, 0)
        d_bg = HF.stgcn_colsum(dy)
        wg_t = HF.stgcn_weight_image(wg, 1, CinP)
        if res == RES_IDENTITY:
            dx = HF.stgcn_conv_dx(dy, wg_t, T, 1, 0, add=dout, mask=out)
        else:
            dx = HF.stgcn_conv_dx(dy, wg_t, T, 1, 0, add=dx_res)
        return crop_dx(dx, Cin), None, dE, d_wg, d_bg, d_g1, d_b1, d_wt, d_bt, d_g2, d_b2, d_wr, d_br, d_gr, d_ber


def st_gcn_block(x, block, A, importance=None, training=True):
    """one `models.STGCN.Block` container applied to x (N, T, V, C_in) -> (N, T_out, V, C_out), T_out = (T - 1) // stride + 1.
    `A`: the (3, V, V) adjacency buffer, `importance`: the block's edge_importance parameter or None (ones).
    `training`: batch statistics, and the running values of the block's BatchNorms advance on the device; else the
    running values normalise.  The whole block is one autograd node."""
    if x.dim() != 4 or x.shape[2] != A.shape[1] or x.shape[3] != block.in_channels:
        raise ValueError(f"expected (N, T, {A.shape[1]}, {block.in_channels}), got {tuple(x.shape)}")
    conv, bn1, tconv, bn2 = block.gcn.conv, block.tcn[0], block.tcn[2], block.tcn[3]
    if block.residual_kind == RES_CONV:
        rconv, bnr = block.residual[0], block.residual[1]
        rpar = (rconv.weight, rconv.bias, bnr.weight, bnr.bias)
    else:
        bnr, rpar = None, (None, None, None, None)
    cfg = (A, block.stride, block.residual_kind, bool(training), bn1, bn2, bnr)
    return _Block.apply(x.contiguous().float(), cfg, importance, conv.weight, conv.bias, bn1.weight, bn1.bias,
                        tconv.weight, tconv.bias, bn2.weight, bn2.bias, *rpar)


class _RowsBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, bn, training):
        mean, rstd = _bn_stats(x, bn, training)
        ctx.save_for_backward(x, mean, rstd, gamma)
        ctx.training = training
        return HF.stgcn_bn_apply(x, mean, rstd, gamma, beta, relu=False)

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma = ctx.saved_tensors
        dx, dg, db = HF.stgcn_bn_backward(dy.contiguous(), None, x, mean, rstd, gamma, ctx.training)
        return dx, dg, db, None, None


def batch_norm_rows(x, bn, training=True):
    """BatchNorm over the rows of x (M, C) with the parameters and running statistics of the nn.BatchNorm `bn`"""
    return _RowsBN.apply(x.contiguous().float(), bn.weight, bn.bias, bn, bool(training))


class _Pool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, seed_base):
        ctx.cfg = (x.shape[1], p, seed, seed_base)
        return HF.stgcn_pool(x, p, seed, seed_base)

    @staticmethod
    def backward(ctx, dout):
        R, p, seed, seed_base = ctx.cfg
        return HF.stgcn_pool_backward(dout.contiguous(), R, p, seed, seed_base), None, None, None


def mean_pool(x, p=0.0, seed=0, seed_base=None):
    """(N, R, C) -> (N, C): mean over the R rows of each clip, then dropout p with the hash mask of (seed, seed_base)"""
    return _Pool.apply(x.contiguous(), float(p), int(seed), seed_base)
