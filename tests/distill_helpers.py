"""The distilled slice criterion (hwgat_kd_fwd / hwgat_kd_bwd of csrc/loss_eval.hip) restated in torch ops, in whatever
dtype the student's logits come in (fp64 for the reference, fp32 for the reference's own deviation).  The hard part is
tests/test_gpu_graph_micro.py's `_rows`, the soft part the textbook form tau^2 sum p (log p - log q) -- on purpose NOT the
form the kernel evaluates.  `kd_ref`'s gradient is the closed form of include/hwgat_hip.h, so that tests/test_distill_cpu.py
can hold it against autograd of `kd_loss`."""
import torch

import test_gpu_graph_micro as GM

EPS, G_UP = GM.EPS, GM.G_UP


def kd_rows(z, u, tau):
    """tau^2 KL(softmax(u / tau) || softmax(z / tau)) per row; a column with p = 0 counts 0"""
    lp, lq = torch.log_softmax(u / tau, dim=-1), torch.log_softmax(z / tau, dim=-1)
    p = lp.exp()
    term = torch.where(p > 0, p * (lp - lq), torch.zeros_like(p))
    return (tau * tau) * term.sum(-1)


def hard_rows(z, y, y_b, lam):
    if lam is None:
        return GM._rows(z, y)
    lam = lam.to(z.dtype)
    return lam * GM._rows(z, y) + (1.0 - lam) * GM._rows(z, y_b)


def kd_loss(z, u, y, y_b, lam, alpha, tau, v, n_rows):
    """(loss, kd) of the slice, differentiable in z: the live rows' sums over the batch's row count"""
    u = u.to(z.dtype)
    lam_v = None if lam is None else lam[:v]
    yb_v = None if y_b is None else y_b[:v]
    rk = kd_rows(z[:v], u[:v], tau)
    hard = hard_rows(z[:v], y[:v], yb_v, lam_v)
    return ((1.0 - alpha) * hard + alpha * rk).sum() / n_rows, rk.sum() / n_rows


def kd_grad(z, u, y, y_b, lam, alpha, tau, v, n_rows, soft_only=False):
    """d loss / d z * G_UP by the closed form: zero in the dead rows"""
    u = u.to(z.dtype)
    C = z.shape[1]
    dz = torch.zeros_like(z)
    zl, ul = z[:v], u[:v]
    hit = torch.zeros_like(zl)
    if lam is None:
        hit.scatter_(1, y[:v].unsqueeze(1), 1.0)
    else:
        lam_v = lam[:v].to(z.dtype)
        hit.scatter_add_(1, y[:v].unsqueeze(1), lam_v.unsqueeze(1))
        hit.scatter_add_(1, y_b[:v].unsqueeze(1), (1.0 - lam_v).unsqueeze(1))
    hard = torch.softmax(zl, -1) - (1.0 - EPS) * hit - EPS / C
    soft = tau * (torch.softmax(zl / tau, -1) - torch.softmax(ul / tau, -1))
    dz[:v] = (G_UP / n_rows) * ((0.0 if soft_only else (1.0 - alpha)) * hard + alpha * soft)
    return dz


def kd_ref(z, u, y, y_b, lam, alpha, tau, v, n_rows):
    """(loss, kd, d loss / d z * G_UP) of the slice in z's dtype"""
    with torch.no_grad():
        loss, kd = kd_loss(z, u, y, y_b, lam, alpha, tau, v, n_rows)
        return loss, kd, kd_grad(z, u, y, y_b, lam, alpha, tau, v, n_rows)
