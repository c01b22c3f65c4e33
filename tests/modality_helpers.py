"""Test helpers of the input modalities and the score ensemble: their contracts (include/hwgat_hip.h, "input modalities" and
"score ensemble") restated with plain torch ops on the CPU, and the parent tables the tests share."""
import torch

KINDS = ("joint", "bone", "motion", "bone_motion")

# the 34 links of the 29-joint upper-body graph (face and arms 0-8, left hand 9-18, right hand 19-28) and the spanning tree
# a breadth-first search from joint 0 with ascending neighbours picks from it, written out by hand
EDGES_29 = [[2, 0], [1, 0], [0, 3], [0, 4], [3, 5], [4, 6], [5, 7], [6, 8], [7, 9], [9, 10], [9, 11], [11, 12], [11, 13],
            [13, 14], [9, 13], [13, 15], [9, 15], [15, 16], [15, 17], [9, 17], [17, 18], [8, 19], [19, 27], [19, 20],
            [19, 21], [19, 23], [19, 25], [21, 22], [21, 23], [23, 24], [23, 25], [25, 26], [25, 27], [27, 28]]
PARENTS_29 = [0, 0, 0, 0, 0, 3, 4, 5, 6, 7, 9, 9, 11, 9, 13, 9, 15, 9, 17, 8, 19, 19, 21, 19, 23, 19, 25, 19, 27]


def identity(J):
    return list(range(J))


def chain(J):
    """joint j hangs on j - 1; joint 0 is the root"""
    return [max(j - 1, 0) for j in range(J)]


def star(J):
    """every joint hangs on the last one, which is the root"""
    return [J - 1] * J


def restate(x, parent, kind, pad_value=None):
    """the `kind` view of x (B, T, J, C) fp32 on the CPU, in fp32: copies and single IEEE subtractions, so a kernel must
    agree bit for bit.  `kind` is a name of KINDS; `parent` a list of J ints (unused by the joint and motion kinds)"""
    assert x.dtype == torch.float32 and x.device.type == "cpu" and x.dim() == 4
    B, T, J, C = x.shape
    if kind == "joint":
        return x.clone()
    padded = x[:, :, 0, 0] == pad_value if pad_value is not None else torch.zeros(B, T, dtype=torch.bool)

    def bones(v):
        p = torch.tensor(parent, dtype=torch.int64)
        b = v - v[:, :, p]
        b[:, :, p == torch.arange(J)] = 0.0                  # a root
        return b

    if kind == "bone":
        out = bones(x)
    else:
        v = x if kind == "motion" else bones(x)
        out = torch.zeros_like(x)
        out[:, :-1] = v[:, 1:] - v[:, :-1]
        before_pad = torch.zeros(B, T, dtype=torch.bool)
        before_pad[:, :-1] = padded[:, 1:]
        out[before_pad] = 0.0
    out[padded] = x[padded]
    return out


def fuse64(z, w, mode):
    """the fused score of member logits z (M, B, C) under weights w (M,), in fp64 from the fp32 values"""
    z, w = z.double().cpu(), torch.as_tensor(w, dtype=torch.float32).double().cpu()
    if mode == "logit":
        return (w.view(-1, 1, 1) * z).sum(0)
    keep = w > 0
    return torch.logsumexp(torch.log(w[keep]).view(-1, 1, 1) + torch.log_softmax(z[keep], dim=-1), dim=0)


def logit_bound(z, w):
    """(M + 1) 2^-24 sum_m |w[m] z[m]| per entry: M roundings of products and M of sums, each at most half an ulp of a
    partial sum that the sum of magnitudes bounds"""
    z, w = z.double().cpu(), torch.as_tensor(w, dtype=torch.float32).double().cpu()
    return (z.shape[0] + 1) * 2.0 ** -24 * (w.view(-1, 1, 1) * z).abs().sum(0)
