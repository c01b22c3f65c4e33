"""A score ensemble on the device: several models, one score.

Skeleton-based recognisers gain most from training one network per input view (modality.Modality: joints, bones, joint
motion, bone motion) and adding the models' scores.  `Ensemble` is that sum as an nn.Module: every member's eval forward on
the same input, their fp32 logits side by side in one static buffer, and one launch of csrc/ensemble.hip (formulas:
include/hwgat_hip.h, "score ensemble") that fuses them.

    ensemble = importlib.import_module("sl-hwgat_amd.ensemble")
    ens = ensemble.Ensemble([joint_model, bone_model, motion_model, bone_motion_model], mode="prob")
    fast = serve.GraphedEval(ens, example)              # or evaluate.Evaluator(ens, ...), serve.StreamRecognizer(ens, ...)
    ens.weights = ensemble.fit_weights(val_logits, val_labels, "prob")       # the next replay reads them: no new capture
    step = train.GraphedTrainStep(student, opt, x, y, distiller=train.Distiller(ens))    # four streams into one model

Each member reads the input through its own `input_modality`, so all of them take the raw joints.  The weights live in a
registered device buffer the fuse kernel reads when it runs.  An ensemble is evaluation-only: the members are put into
eval() with requires_grad_(False) and train(True) raises.
"""
import math
import numbers

import torch
from torch import nn

from . import functional as HF

MODES = HF.ENS_MODES
MAX_MEMBERS = HF.ENS_MAX_MEMBERS


def _num_classes(model):
    """the width of a member's logits: `num_classes` where the model carries it, else its classifier's"""
    n = getattr(model, "num_classes", None)
    if isinstance(n, numbers.Integral) and n > 0:
        return int(n)
    for path in ("head.classifier", "classifier", "head"):
        m = model
        for name in path.split("."):
            m = getattr(m, name, None)
        if isinstance(m, nn.Sequential) and len(m) > 0:
            m = m[-1]
        if isinstance(m, nn.Linear):
            return m.out_features
    raise ValueError(f"Ensemble: cannot tell how many classes {type(model).__name__} scores (no `num_classes`, no "
                     "nn.Linear `head`, `head.classifier` or `classifier`)")


def _checked_weights(weights, M):
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().tolist()
    try:
        w = [float(v) for v in weights]
    except TypeError:
        raise ValueError(f"Ensemble: weights must be {M} numbers, got {weights!r}") from None
    if len(w) != M:
        raise ValueError(f"Ensemble: {M} members need {M} weights, got {len(w)}")
    if any(not math.isfinite(v) or v < 0 for v in w):
        raise ValueError(f"Ensemble: every weight must be finite and >= 0, got {w}")
    if not sum(w) > 0:
        raise ValueError(f"Ensemble: the weights must have a positive sum, got {w}")
    return w


class Ensemble(nn.Module):
    """`members`: 1 to 8 distinct nn.Modules that give (B, num_classes) logits for the same input.  `weights`: one number
    per member (default: equal, summing to 1).  `mode`: 'prob' -- log of the weighted mean of the members' softmaxes, a
    normalised log-distribution when the weights sum to 1 -- or 'logit' -- the weighted sum of the logits."""

    def __init__(self, members, weights=None, mode="prob"):
        super().__init__()
        members = list(members)
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError(f"Ensemble: 1 to {MAX_MEMBERS} members, got {len(members)}")
        for m in members:
            if not isinstance(m, nn.Module):
                raise ValueError(f"Ensemble: a member must be a torch.nn.Module, got {type(m).__name__}")
        if len({id(m) for m in members}) != len(members):
            raise ValueError("Ensemble: the same object is a member twice -- give its weight once")
        if mode not in MODES:
            raise ValueError(f"Ensemble: mode must be one of {MODES}, got {mode!r}")
        classes = [_num_classes(m) for m in members]
        if len(set(classes)) != 1:
            raise ValueError(f"Ensemble: the members score {classes} classes: fusion needs the same classes in the same order")
        frames = {int(m.temporal_dim) for m in members if hasattr(m, "temporal_dim")}
        if len(frames) > 1:
            raise ValueError(f"Ensemble: the members take clips of {sorted(frames)} frames: they must agree")
        if frames:
            self.temporal_dim = frames.pop()
        self.num_classes, self.mode = classes[0], mode
        self.members = nn.ModuleList(m.eval().requires_grad_(False) for m in members)
        M = len(members)
        self._weights = _checked_weights([1.0 / M] * M if weights is None else weights, M)
        dev = next((p.device for m in members for p in m.parameters()), torch.device("cpu"))
        self.register_buffer("weight_buffer", torch.tensor(self._weights, dtype=torch.float32).to(dev), persistent=False)
        self._logit_buffers = {}                 # (rows, device) -> (M, rows, classes); kept: a captured graph holds its address
        self.member_logits = None                # the buffer of the latest forward
        nn.Module.train(self, False)

    def train(self, mode=True):
        if mode:
            raise RuntimeError("Ensemble is evaluation-only: its members stay in eval() (train the members on their own)")
        return super().train(False)

    @property
    def weights(self):
        return list(self._weights)

    @weights.setter
    def weights(self, values):
        """validated on the host, then written to the device buffer in place (stream-ordered): a captured graph reads the
        new weights at its next replay"""
        w = _checked_weights(values, len(self.members))
        self._weights = w
        self.weight_buffer.copy_(torch.tensor(w, dtype=torch.float32), non_blocking=False)

    def forward(self, x):
        M = len(self.members)
        buf = None
        with torch.no_grad():
            for i, member in enumerate(self.members):
                if member.training:
                    raise RuntimeError(f"Ensemble: member {i} is in train() mode -- the members must stay in eval()")
                z = member(x)
                if z.dim() != 2 or z.shape[1] != self.num_classes:
                    raise ValueError(f"Ensemble: member {i} returned {tuple(z.shape)}, expected (B, {self.num_classes}) logits")
                if buf is None:
                    key = (z.shape[0], z.device)
                    buf = self._logit_buffers.get(key)
                    if buf is None:
                        buf = self._logit_buffers[key] = torch.empty((M, z.shape[0], self.num_classes), device=z.device,
                                                                     dtype=torch.float32)
                buf[i].copy_(z)                              # the member's logits as fp32, whatever it computes in
            self.member_logits = buf
            return HF.ens_fuse(buf, self.weight_buffer, self.mode)


def _simplex(M, n):
    """every (k_0, .., k_{M-1}) of non-negative integers summing to n, in lexicographic order"""
    if M == 1:
        yield (n,)
        return
    for k in range(n + 1):
        for rest in _simplex(M - 1, n - k):
            yield (k,) + rest


def fuse_reference(member_logits, weights, mode):
    """the fused score in plain torch ops, in the dtype and on the device of `member_logits` (M, N, C): what the fuse kernel
    computes, for the weight search and for checks"""
    z = member_logits
    w = torch.as_tensor(weights, dtype=z.dtype, device=z.device).view(-1, 1, 1)
    if mode == "logit":
        return (w * z).sum(0)
    keep = (w > 0).view(-1)
    return torch.logsumexp(torch.log(w[keep]) + torch.log_softmax(z[keep], dim=-1), dim=0)


def fit_weights(member_logits, labels, mode, step=0.1):
    """the weights on the simplex grid of spacing `step` (1 / step must be an integer) with the best top-1 accuracy of the
    fused score on member_logits (M, N, C) against labels (N,); ties go to the first grid point in lexicographic order of
    the weight tuples.  Plain torch ops on the tensors' device: a few hundred grid points over a few thousand validation
    clips take about 0.1 s.  Returns a list of M floats summing to 1"""
    if mode not in MODES:
        raise ValueError(f"fit_weights: mode must be one of {MODES}, got {mode!r}")
    z = member_logits
    if z.dim() != 3 or z.shape[0] < 1 or labels.shape != (z.shape[1],):
        raise ValueError(f"fit_weights: member logits (M, N, C) and labels (N,), got {tuple(z.shape)} and {tuple(labels.shape)}")
    n = round(1.0 / float(step)) if step and step > 0 else 0
    if n < 1 or abs(n * float(step) - 1.0) > 1e-9:
        raise ValueError(f"fit_weights: 1 / step must be a positive integer, got step = {step}")
    z = z.double()
    labels = labels.to(z.device)
    best, best_hits = None, -1
    for ks in _simplex(z.shape[0], n):
        w = [k / n for k in ks]
        hits = int((fuse_reference(z, w, mode).argmax(dim=-1) == labels).sum())
        if hits > best_hits:
            best, best_hits = w, hits
    return best
