"""One DecoupledGCN unit (reference hwgat/models/DecoupledGCN.py: DecoupledGCN_TCN_unit) as a single autograd node whose
forward and backward are sequences of HIP launches, in the style of stgcn_block._Block.  Activations are fp32,
channels-last (N, T, V, C).

forward of a unit (C_in -> C_out, temporal stride s):
    y   = x W + b                                  1x1 conv to 3 C_out channels (hwgat_stgcn_conv, 1 tap)
    yb  = BN0(y)                                   hwgat_stgcn_bn_stats + hwgat_stgcn_bn_apply
    a   = sum_{k,v} An[k, c mod G, v, w] yb[.., v, k C_out + c]          hwgat_dgcn_agg_fwd
    h   = relu(BN(a) + down(x))                    hwgat_stgcn_bn_apply; down = identity | BNd(x Wd + bd)
    m0  = mean_T h                       (N, V, C) hwgat_dgcn_gate_sum, axis 0
    s_v = sigmoid(conv_sa(m0))           (N, V)    tensor ops on (N, V, C)
    m1  = mean_V h (1 + s_v)             (N, T, C) hwgat_dgcn_gate_sum, axis 1
    s_t = sigmoid(conv_ta(m1))           (N, T)    tensor ops on (N, T, C)
    m2  = mean_T (1 + s_t) m1            (N, C)    tensor ops: the third squeeze is a frame mean of the second, so h is
                                                   read three times per unit, not four
    s_c = sigmoid(fc2c(relu(fc1c(m2))))  (N, C)
    h3  = h (1 + s_v)(1 + s_t)(1 + s_c)            hwgat_dgcn_gate_apply (h1, h2 never exist)
    c   = tconv9(h3, stride s)                     hwgat_stgcn_conv, 9 taps
    out = relu(BN2(c) + r)                         r = 0 | x | BNr(x Wr + br, stride s): hwgat_stgcn_bn_apply, or with
                                                   DropGraph (train mode, keep_prob < 1) hwgat_dgcn_merge
DropGraph (`drop_masks`): four draws per unit -- spatial then temporal on BN2(c), spatial then temporal on r -- each the
|.| statistic (hwgat_dgcn_abs_sum, BatchNorm and the spatial factor applied while reading), the probabilities on the
(N, V) / (N, T) statistic (tensor ops), the hash Bernoulli draw (hwgat_dgcn_draw) and the mask with its batch-wide
normaliser (hwgat_dgcn_mask_*).  The masks carry no gradient.

backward: merge / BatchNorm backward -> conv dW / db / dX -> gate backward (two hwgat_dgcn_gate_sum launches for the gate
gradients, the small nets re-run under autograd on their (N, V, C) / (N, T, C) inputs, hwgat_dgcn_gate_bwd for dh) ->
BatchNorm backward -> aggregation backward (dyb, dAn) -> BatchNorm backward -> projection dW / db / dX.  Every sum over
rows goes through partial images added in a fixed order: two backward runs are bit-identical.
"""
import torch

from . import functional as HF
from .stgcn_block import _bn_stats, pad_channels, project, residual_forward, crop_dx, RES_IDENTITY, RES_CONV

TCN_DROP_BLOCK = 41      # the reference's TCNUnit builds its temporal DropGraph with the default block size, always


def conv_rows(m, w, b):
    """nn.Conv1d(C, 1, ker, padding=(ker - 1) // 2) on m (N, L, C) channels-last, as a matmul: -> (N, L)"""
    ker = w.shape[2]
    pad = (ker - 1) // 2
    N, L, C = m.shape
    halo = m.new_zeros(N, pad, C)
    windows = torch.cat([halo, m, halo], dim=1).unfold(1, ker, 1)              # (N, L, C, ker)
    return torch.einsum("nlcj,cj->nl", windows, w[0]) + b


def gate_conv(m, w, b):
    """the spatial (m0, conv_sa) or temporal (m1, conv_ta) gate: sigmoid of the one-channel convolution along the rows"""
    return torch.sigmoid(conv_rows(m, w, b))


def gate_channel(m1, s_t, w1, b1, w2, b2):
    m2 = ((1.0 + s_t).unsqueeze(-1) * m1).mean(dim=1)
    return torch.sigmoid(torch.relu(m2 @ w1.t() + b1) @ w2.t() + b2)


def drop_probability(stat, gamma):
    """the Bernoulli probabilities of a DropGraph draw from the |x| sums over the other dimensions: the statistic is
    normalised to mean 1 over the batch (so the divisor of the mean cancels), scaled by gamma and capped at 1"""
    return torch.clamp(stat / stat.sum() * (stat.numel() * gamma), max=1.0)


def drop_masks(z, bn, A, keep_prob, drop_size, block, seeds, seed_base, injected, tap, tag):
    """(fs (N, V), ft (N, T)): the spatial and then the temporal DropGraph mask of z (its BatchNorm read when `bn`), each
    times its batch-wide normaliser.  `seeds`: the two site seeds; `injected`: {(unit, site): seed tensor} or None."""
    unit, first = tag
    stat = HF.dgcn_abs_sum(z, 0, bn)
    p_s = drop_probability(stat, (1.0 - keep_prob) / (1.0 + drop_size))
    key = (unit, first)
    m_s = injected[key].to(p_s) if injected is not None and key in injected else HF.dgcn_draw(p_s, seeds[0], seed_base)
    fs, scale_s = HF.dgcn_mask_spatial(m_s.contiguous(), A)
    stat = HF.dgcn_abs_sum(z, 1, bn, fs)
    p_t = drop_probability(stat, (1.0 - keep_prob) / block)
    key = (unit, first + 1)
    m_t = injected[key].to(p_t) if injected is not None and key in injected else HF.dgcn_draw(p_t, seeds[1], seed_base)
    ft, scale_t = HF.dgcn_mask_temporal(m_t.contiguous(), block)
    if tap is not None:
        tap.append(dict(unit=unit, site=first, p=p_s, seeds=m_s, scale=scale_s, factor=fs))
        tap.append(dict(unit=unit, site=first + 1, p=p_t, seeds=m_t, scale=scale_t, factor=ft))
    return fs, ft


def _linear_master(lw):
    """the (C_in, 3 C_out) projection as a conv master weight (3 C_out, C_in, 1, 1)"""
    return lw.t().contiguous().view(lw.shape[1], lw.shape[0], 1, 1)


class _Unit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cfg, An, lw, lb, g0, b0, g1, b1, wd, bd, gd, bed, w_sa, b_sa, w_ta, b_ta, w1, bc1, w2, bc2,
                wt, bt, g2, b2, wr, br, gr, ber):
        groups, stride, res, training, bn0, bn1, bnd, bn2, bnr, drop = cfg
        N, T, V, Cin = x.shape
        xp = pad_channels(x)
        CinP = xp.shape[3]
        y = project(xp, _linear_master(lw), lb.reshape(-1).contiguous())
        m0, r0 = _bn_stats(y, bn0, training)
        yb = HF.stgcn_bn_apply(y, m0, r0, g0, b0, relu=False)
        a = HF.dgcn_aggregate(yb, An, groups)
        m1, r1 = _bn_stats(a, bn1, training)
        dn = md = rd = None
        if wd is not None:
            dn = HF.stgcn_conv(xp, HF.stgcn_weight_image(wd, 0, CinP), bd)
            md, rd = _bn_stats(dn, bnd, training)
            h = HF.stgcn_bn_apply(a, m1, r1, g1, b1, relu=True, res=dn, res_bn=(md, rd, gd, bed))
        else:
            h = HF.stgcn_bn_apply(a, m1, r1, g1, b1, relu=True, res=x)
        q0 = HF.dgcn_gate_sum(h, 0, 1.0 / T)
        s_v = gate_conv(q0, w_sa, b_sa)
        q1 = HF.dgcn_gate_sum(h, 1, 1.0 / V, sv=s_v)
        s_t = gate_conv(q1, w_ta, b_ta)
        s_c = gate_channel(q1, s_t, w1, bc1, w2, bc2)
        h3 = HF.dgcn_gate_apply(h, s_v, s_t, s_c)
        c = HF.stgcn_conv(h3, HF.stgcn_weight_image(wt, 0), bt, stride, wt.shape[2] // 2)
        m2, r2 = _bn_stats(c, bn2, training)
        r, rbn = residual_forward(res, x, xp, wr, br, gr, ber, bnr, stride, training)
        rc, mr, rr = (r, rbn[0], rbn[1]) if rbn else (None, None, None)
        fs1 = ft1 = fs2 = ft2 = None
        if drop is not None:
            A, keep_prob, drop_size, block, seeds, seed_base, injected, tap, unit = drop
            if r is None:
                raise NotImplementedError("DropGraph on a unit without a residual path: the reference fails on it too")
            fs1, ft1 = drop_masks(c, (m2, r2, g2, b2), A, keep_prob, drop_size, TCN_DROP_BLOCK, seeds[0:2], seed_base,
                                  injected, tap, (unit, 0))
            fs2, ft2 = drop_masks(r, rbn, A, keep_prob, drop_size, block, seeds[2:4], seed_base, injected, tap, (unit, 2))
            out = HF.dgcn_merge(c, (m2, r2, g2, b2), r, rbn, fs1, ft1, fs2, ft2)
        else:
            out = HF.stgcn_bn_apply(c, m2, r2, g2, b2, relu=True, res=r, res_bn=rbn)
        ctx.save_for_backward(xp, y, yb, a, dn, h, q0, q1, s_v, s_t, s_c, h3, c, rc, out, m0, r0, m1, r1, md, rd, m2, r2, mr,
                              rr, An, lw, g0, g1, wd, gd, w_sa, b_sa, w_ta, b_ta, w1, bc1, w2, bc2, wt, g2, wr, gr,
                              fs1, ft1, fs2, ft2)
        ctx.cfg = (groups, stride, res, training, Cin)
        return out

    @staticmethod
    def backward(ctx, dout):
        (xp, y, yb, a, dn, h, q0, q1, s_v, s_t, s_c, h3, c, rc, out, m0, r0, m1, r1, md, rd, m2, r2, mr, rr, An, lw, g0, g1,
         wd, gd, w_sa, b_sa, w_ta, b_ta, w1, bc1, w2, bc2, wt, g2, wr, gr, fs1, ft1, fs2, ft2) = ctx.saved_tensors
        groups, stride, res, training, Cin = ctx.cfg
        dout = dout.contiguous()
        N, T, V, CinP = xp.shape
        pad = wt.shape[2] // 2
        # ---- the tail: relu(BN2(c) f1 + r' f2), f = 1 without DropGraph
        if fs1 is not None:
            dz1, dz2 = HF.dgcn_merge_backward(dout, out, fs1, ft1, fs2, ft2)
            gate = None
        else:
            dz1 = dz2 = dout
            gate = out
        dc, d_g2, d_b2 = HF.stgcn_bn_backward(dz1, gate, c, m2, r2, g2, training)
        d_wr = d_br = d_gr = d_ber = None
        if res == RES_CONV:
            drc, d_gr, d_ber = HF.stgcn_bn_backward(dz2, gate, rc, mr, rr, gr, training)
            d_wr = HF.stgcn_conv_dw(xp, drc, wr.shape, stride, 0)
            d_br = HF.stgcn_colsum(drc)
        d_wt = HF.stgcn_conv_dw(h3, dc, wt.shape, stride, pad)
        d_bt = HF.stgcn_colsum(dc)
        dh3 = HF.stgcn_conv_dx(dc, HF.stgcn_weight_image(wt, 1), T, stride, pad)
        # ---- the gates.  u = sum_v dh3 h (1 + s_v) carries d s_c (times 1 + s_t, summed over t) and d s_t (times
        # 1 + s_c, summed over c); the nets run again under autograd on their small inputs
        u = HF.dgcn_gate_sum(h, 1, 1.0, g=dh3, sv=s_v)
        # (these sums cancel heavily and their operands are tiny: double costs nothing and keeps the gate nets' gradients
        # at the accuracy of the kernels that feed them)
        u = u.double()
        ds_c = ((1.0 + s_t.double()).unsqueeze(-1) * u).sum(dim=1).float()
        ds_t = ((1.0 + s_c.double()).unsqueeze(1) * u).sum(dim=2).float()
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(True) for t in (q1, s_t, w1, bc1, w2, bc2)]
            dq1_c, ds_t_c, d_w1, d_bc1, d_w2, d_bc2 = torch.autograd.grad(gate_channel(*leaves), leaves, ds_c)
            leaves = [t.detach().requires_grad_(True) for t in (q1, w_ta, b_ta)]
            dq1_t, d_w_ta, d_b_ta = torch.autograd.grad(gate_conv(*leaves), leaves, ds_t + ds_t_c)
        dq1 = (dq1_c + dq1_t).contiguous()
        # d s_v = sum_{t,c} h (dh3 (1 + s_t)(1 + s_c) + dq1 / V)
        ds_v = HF.dgcn_gate_sum(h, 0, 1.0, g=dh3, st=s_t, sc=s_c, m=dq1, m_scale=1.0 / V).double().sum(dim=2).float()
        with torch.enable_grad():
            leaves = [t.detach().requires_grad_(True) for t in (q0, w_sa, b_sa)]
            dq0, d_w_sa, d_b_sa = torch.autograd.grad(gate_conv(*leaves), leaves, ds_v)
        dh = HF.dgcn_gate_backward(dh3, s_v, s_t, s_c, dq1, dq0.contiguous())
        # ---- h = relu(BN(a) + down(x))
        da, d_g1, d_b1 = HF.stgcn_bn_backward(dh, h, a, m1, r1, g1, training)
        d_wd = d_bd = d_gd = d_bed = None
        add, mask = None, None             # what reaches x besides the projection's input gradient
        if wd is not None:
            ddn, d_gd, d_bed = HF.stgcn_bn_backward(dh, h, dn, md, rd, gd, training)
            d_wd = HF.stgcn_conv_dw(xp, ddn, wd.shape, 1, 0)
            d_bd = HF.stgcn_colsum(ddn)
            add = HF.stgcn_conv_dx(ddn, HF.stgcn_weight_image(wd, 1, CinP), T, 1, 0)
            if res == RES_CONV:
                add = HF.stgcn_conv_dx(drc, HF.stgcn_weight_image(wr, 1, CinP), T, stride, 0, add=add)
        elif res == RES_IDENTITY:          # identity down and identity skip: C_in == C_out, no channel padding
            add = HF.dgcn_masked_sum(dh, h, dz2, gate)
        elif res == RES_CONV:
            add = HF.stgcn_conv_dx(drc, HF.stgcn_weight_image(wr, 1, CinP), T, stride, 0, add=dh, mask=h)
        else:
            add, mask = dh, h
        dyb, dAn = HF.dgcn_aggregate_backward(yb, da, An, groups, ctx.needs_input_grad[2])
        dy, d_g0, d_b0 = HF.stgcn_bn_backward(dyb, None, y, m0, r0, g0, training)
        wg = _linear_master(lw)
        d_lw = HF.stgcn_conv_dw(xp, dy, wg.shape, 1, 0).view(wg.shape[0], wg.shape[1]).t().contiguous()
        d_lb = HF.stgcn_colsum(dy).view(1, -1, 1, 1)
        dx = HF.stgcn_conv_dx(dy, HF.stgcn_weight_image(wg, 1, CinP), T, 1, 0, add=add, mask=mask)
        return (crop_dx(dx, Cin), None, dAn, d_lw, d_lb, d_g0, d_b0, d_g1, d_b1, d_wd, d_bd, d_gd, d_bed, d_w_sa, d_b_sa, d_w_ta, d_b_ta,
                d_w1, d_bc1, d_w2, d_bc2, d_wt, d_bt, d_g2, d_b2, d_wr, d_br, d_gr, d_ber)


def normalised_adjacency(decoupled_A):
    """An[k, g, v, w] = A[k, g, v, w] / (sum_v A[k, g, v, w] + 0.001): what the reference's `norm` computes with its
    `eye_list` (A diag(1 / (column sum + 0.001))), assuming eye_list is the identity stack it is constructed as"""
    return decoupled_A / (decoupled_A.sum(dim=2, keepdim=True) + 0.001)


def dgcn_unit(x, unit, training=True, drop=None):
    """one `models.DecoupledGCN.Unit` container applied to x (N, T, V, C_in) -> (N, T_out, V, C_out).  `drop`: None (no
    DropGraph) or (keep_prob, drop_size, block_size, the unit's four site seeds, the call's device base-seed word,
    injected seeds or None, the tap list or None, the unit's number)"""
    V = unit.A.shape[0]
    if x.dim() != 4 or x.shape[2] != V or x.shape[3] != unit.in_channels:
        raise ValueError(f"expected (N, T, {V}, {unit.in_channels}), got {tuple(x.shape)}")
    g, t = unit.gcn1, unit.tcn1
    if unit.in_channels != unit.out_channels:
        bnd, dpar = g.down[1], (g.down[0].weight, g.down[0].bias, g.down[1].weight, g.down[1].bias)
    else:
        bnd, dpar = None, (None, None, None, None)
    if unit.residual_kind == RES_CONV:
        bnr = unit.residual.bn
        rpar = (unit.residual.conv.weight, unit.residual.conv.bias, bnr.weight, bnr.bias)
    else:
        bnr, rpar = None, (None, None, None, None)
    if drop is not None:
        drop = (unit.A,) + tuple(drop)
    cfg = (g.groups, unit.stride, unit.residual_kind, bool(training), g.bn0, g.bn, bnd, t.bn, bnr, drop)
    An = normalised_adjacency(g.decoupled_A)
    return _Unit.apply(x.contiguous().float(), cfg, An, g.linear_weight, g.linear_bias, g.bn0.weight, g.bn0.bias,
                       g.bn.weight, g.bn.bias, *dpar, unit.conv_sa.weight, unit.conv_sa.bias, unit.conv_ta.weight,
                       unit.conv_ta.bias, unit.fc1c.weight, unit.fc1c.bias, unit.fc2c.weight, unit.fc2c.bias,
                       t.conv.weight, t.conv.bias, t.bn.weight, t.bn.bias, *rpar)
