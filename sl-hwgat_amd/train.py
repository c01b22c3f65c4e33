"""Loss and the fwd+bwd step harness of the hot path (reference hwgat/utils.py:93-116
and hwgat/losses/SmoothCrossEntropy.py), without the per-step host syncs."""
import contextlib
import numbers

import numpy as np
import torch
import torch.nn.functional as tF


class SmoothedCrossEntropyLoss(torch.nn.Module):
    """(1-eps)*NLL + eps*(-mean log p), batch mean; eps 0.01 as in the reference."""

    def __init__(self, smooth_factor: float = 0.01):
        super().__init__()
        self.smooth_factor = smooth_factor

    def forward(self, input, target):
        lp = tF.log_softmax(input.float(), dim=-1)
        nll = -lp.gather(-1, target.unsqueeze(1)).squeeze(1)
        return ((1.0 - self.smooth_factor) * nll + self.smooth_factor * (-lp.mean(-1))).mean()


class FusedSmoothedCrossEntropyLoss(torch.nn.Module):
    """SmoothedCrossEntropyLoss on the HIP kernels of csrc/loss_eval.hip: two launches forward, one backward, instead of
    the ~15 of log_softmax / gather / mean / blend and their backward.  The forward also leaves `last_rank` (the target's
    place in a stable descending sort of the row, int32) and `last_pred` (lowest arg-max index, int32) of its batch on the
    device; `correct()` is the number of rows whose target ranks first.  The rank's tie rule and argmax both prefer the
    lowest index, so that is the `(argmax == target).sum()` of TrainStep without its three launches."""

    def __init__(self, smooth_factor: float = 0.01):
        super().__init__()
        self.smooth_factor = smooth_factor
        self.last_rank = self.last_pred = None

    def forward(self, input, target):
        loss, self.last_rank, self.last_pred = _functional().smooth_ce(input, target, self.smooth_factor)
        return loss

    def correct(self):
        return (self.last_rank == 0).sum()


class BatchSlicedCrossEntropyLoss(torch.nn.Module):
    """The smoothed cross-entropy of a zero-padded batch, slice by slice (hwgat_bsce_fwd / hwgat_bsce_bwd of
    csrc/loss_eval.hip).  The step that owns the batch calls `place(n_rows, offset)` before each slice: `n_rows` is its
    device int32 word with the number of real rows, `offset` the slice's first row in the batch.  The slice's loss is the
    sum over its real rows divided by `n_rows` -- its share of the batch mean, used as returned, without an n_i / n factor;
    a slice of padding only gives exactly 0 and a zero gradient.  `last_rank` / `last_pred` hold the real rows' values
    (the others are not written), `correct()` counts real rows only."""

    def __init__(self, smooth_factor: float = 0.01):
        super().__init__()
        self.smooth_factor = smooth_factor
        self.n_rows, self.offset = None, 0
        self.last_rank = self.last_pred = self._hits = None

    def place(self, n_rows, offset):
        self.n_rows, self.offset = n_rows, int(offset)

    def forward(self, input, target):
        if self.n_rows is None:
            raise RuntimeError("BatchSlicedCrossEntropyLoss: place(n_rows, offset) first -- TrainStep(pad_to=...) and "
                               "GraphedTrainStep(ragged=True) do")
        loss, self.last_rank, self.last_pred, self._hits = _functional().batch_sliced_ce(
            input, target, self.smooth_factor, self.n_rows, self.offset)
        return loss

    def correct(self):
        return self._hits


class MixedCrossEntropyLoss(BatchSlicedCrossEntropyLoss):
    """BatchSlicedCrossEntropyLoss for a batch a `BatchMixer` has mixed (hwgat_mbsce_fwd / hwgat_mbsce_bwd of
    csrc/loss_eval.hip): row r's loss is lam[r] l(y[r]) + (1 - lam[r]) l(y_b[r]), with the mixer's records `lam` and `y_b`
    of the latest draw read at the slice's place, `mixer.y_b[offset:offset + b]`.  A row the mixer left alone has lam 1 and
    the parent's bits.  `last_rank` and `correct()` refer to the dominant label (y[r] when lam[r] >= 0.5, else y_b[r]).
    The step that owns the batch binds the mixer (`bind_mixer`) and calls `place(n_rows, offset)` before each slice."""

    def __init__(self, smooth_factor: float = 0.01, mixer=None):
        super().__init__(smooth_factor)
        self.mixer = mixer

    def bind_mixer(self, mixer):
        if self.mixer is not None and self.mixer is not mixer:
            raise ValueError("MixedCrossEntropyLoss is bound to another BatchMixer: one criterion serves one mixer")
        self.mixer = mixer

    def forward(self, input, target):
        if self.n_rows is None or self.mixer is None or self.mixer.y_b is None:
            raise RuntimeError("MixedCrossEntropyLoss: bind_mixer(mixer), mixer.apply(...) and place(n_rows, offset) first -- "
                               "TrainStep(mixer=...) and GraphedTrainStep(mixer=...) do")
        y_b, lam = self._mixer_slice(input.shape[0])
        loss, self.last_rank, self.last_pred, self._hits = _functional().mixed_sliced_ce(
            input, target, y_b, lam, self.smooth_factor, self.n_rows, self.offset)
        return loss

    def _mixer_slice(self, b):
        """(y_b, lam) of the bound mixer's latest draw at the slice's place, rows [offset, offset + b)"""
        m, o = self.mixer, self.offset
        if m.y_b is None:                                  # the distilled criterion's case: the forward above refuses it itself
            raise RuntimeError(f"{type(self).__name__}: the bound mixer has drawn nothing yet (mixer.apply(...) first)")
        if o + b > m.y_b.shape[0]:
            raise ValueError(f"the slice [{o}, {o + b}) lies outside the mixer's batch of {m.y_b.shape[0]} rows")
        return m.y_b[o:o + b], m.lam[o:o + b]


def _unit(name, v, lo=0.0):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not lo <= v <= 1.0:     # a NaN fails the comparison
        raise ValueError(f"BatchMixer: {name} must be a number in [{lo}, 1], got {v!r}")
    return float(v)


class BatchMixer:
    """Mixup and temporal CutMix of the clips of a batch, inside the train step (csrc/mix.hip; formulas: include/hwgat_hip.h,
    "Mixup and temporal CutMix").  Every step the live rows are matched into random pairs; a pair is mixed with
    probability `prob`, by CutMix with probability `cutmix_share` (frames [t0, t0 + L) of the two clips are swapped), else
    by Mixup (lam a + (1 - lam) b and its mirror), lam from Beta(alpha, alpha).  Targets become the pair (y, y_b) with the
    weight `lam` per row, which `MixedCrossEntropyLoss` takes.

        mixer = train.BatchMixer(mixup_alpha=0.4, cutmix_alpha=1.0, prob=1.0, cutmix_share=0.5, seed=0)
        step = train.GraphedTrainStep(model, opt, x, y, ragged=True, mixer=mixer)
        mixer.prob = 0.0                         # the last epochs unmixed: the next step's launch, no new capture

    The draw is a counter-based hash of (seed, step), `step` a device word every draw advances, so the two launches replay
    in a graph and a run is reproducible.  The hyper-parameters are plain attributes; when one changed, one hwgat_mix_set
    launch carries them to the device before the next step (as `push_hyper` does for the optimizers).  Alphas are limited
    to [0.05, 1] (Joehnk's sampler needs alpha <= 1; below 0.05 its powers leave the doubles).  `seed` and `step` may be set
    before or after `bind` (after it, setting either is one hwgat_mix_set launch); reading `step` after `bind` is a host
    read of the device word.  A mixer serves one batch shape `(B, T)`, fixed by `bind`."""

    def __init__(self, mixup_alpha=0.4, cutmix_alpha=1.0, prob=1.0, cutmix_share=0.5, seed=0):
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.cutmix_share = mixup_alpha, cutmix_alpha, prob, cutmix_share
        self._hyper()
        if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"BatchMixer: seed must be an integer in [0, 2^32), got {seed!r}")
        self._state = self._pushed = None
        self._seed, self._step = int(seed), 0
        self.pairs = self.partner = self.lam = self.seg = self.mode = self.y_b = None
        self.B = self.T = None

    def _hyper(self):
        """the four hyper-parameters, validated, in the order of the device words"""
        return (_unit("prob", self.prob), _unit("cutmix_share", self.cutmix_share),
                _unit("mixup_alpha", self.mixup_alpha, 0.05), _unit("cutmix_alpha", self.cutmix_alpha, 0.05))

    # ---- device side
    def bind(self, device, B, T):
        """allocate the state block and the per-row records for batches of B clips of T frames (once)"""
        if self._state is not None:
            if (self.B, self.T) != (int(B), int(T)):
                raise ValueError(f"BatchMixer is bound to batches of ({self.B}, {self.T}, ...), got ({B}, {T}, ...): a mixer "
                                 "serves one batch shape -- pad short batches (TrainStep(pad_to=...), "
                                 "GraphedTrainStep(ragged=True)) or drop them")
            return self
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("BatchMixer needs an MI355X device; there is no CPU fallback")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("BatchMixer: bind() before capturing")
        HF = _functional()
        if not 1 <= int(B) <= HF.MIX_MAX_BATCH or int(T) < 1:
            raise ValueError(f"BatchMixer: no batch of {B} clips of {T} frames (at most {HF.MIX_MAX_BATCH} clips)")
        hyper = self._hyper()
        self.B, self.T = int(B), int(T)
        i32 = torch.zeros(2 * max(self.B // 2, 1) + 4 * self.B, dtype=torch.int32, device=device)
        npair = 2 * max(self.B // 2, 1)
        self.pairs = i32[:npair].view(-1, 2)
        self.partner, self.mode = i32[npair:npair + self.B], i32[npair + self.B:npair + 2 * self.B]
        self.seg = i32[npair + 2 * self.B:].view(self.B, 2)
        self.lam = torch.ones(self.B, dtype=torch.float32, device=device)
        self.y_b = torch.zeros(self.B, dtype=torch.int64, device=device)
        self._state = HF.mix_state(device)
        HF.mix_set(self._state, *hyper, seed=self.seed, step=self._step)
        self._pushed = hyper
        return self

    @property
    def seed(self):
        return self._seed

    @seed.setter
    def seed(self, v):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v < 2 ** 32:
            raise ValueError(f"BatchMixer: seed must be an integer in [0, 2^32), got {v!r}")
        if self._state is not None:                          # the counter goes on where the device has it
            self._step = self.step
        self._seed = int(v)
        self._write_counter()

    def _write_counter(self):
        """seed, step and the hyper words to the device, when there is one"""
        if self._state is not None:
            self._pushed = self._hyper()
            _functional().mix_set(self._state, *self._pushed, seed=self._seed, step=self._step)

    @property
    def step(self):
        """the number of draws so far: the device word once bound (a host read), else the value the first draw starts at"""
        if self._state is None:
            return self._step
        return int(self._state[:1].cpu().numpy().view(np.uint32)[1])

    @step.setter
    def step(self, c):
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= c < 2 ** 32:
            raise ValueError(f"BatchMixer: step must be an integer in [0, 2^32), got {c!r}")
        self._step = int(c)
        self._write_counter()

    def push_hyper(self):
        """one launch when a hyper-parameter changed since the last one, none otherwise"""
        hyper = self._hyper()
        if self._state is not None and hyper != self._pushed:
            _functional().mix_set(self._state, *hyper)
            self._pushed = hyper

    def apply(self, x, y, n_rows=None):
        """draw + apply: mix x (B, T, ...) fp32 in place and leave the records of the step (`partner`, `lam`, `seg`, `mode`,
        `y_b`, `pairs`) on the device; `n_rows`: the device int32 word with the live row count, or None (all rows)"""
        self.bind(x.device, x.shape[0], x.shape[1])
        if not torch.cuda.is_current_stream_capturing():         # a captured step pushes before each replay instead
            self.push_hyper()
        HF = _functional()
        HF.mix_draw(self._state, y, n_rows, self.pairs, self.partner, self.lam, self.seg, self.mode, self.y_b, self.T)
        HF.mix_apply(x, self.pairs, self.lam, self.seg, self.mode, n_rows)

    def records(self):
        """the latest draw's records as numpy arrays (one sync): partner, lam, seg, mode, y_b, pairs"""
        if self._state is None:
            raise RuntimeError("BatchMixer has drawn nothing yet: its records live on the device of its first step (or bind())")
        return dict(partner=self.partner.cpu().numpy(), lam=self.lam.cpu().numpy(), seg=self.seg.cpu().numpy(),
                    mode=self.mode.cpu().numpy(), y_b=self.y_b.cpu().numpy(), pairs=self.pairs.cpu().numpy())

    # ---- what a warm-up must not leave behind
    def snapshot(self):
        return None if self._state is None else self._state.clone()

    def restore(self, snap):
        if self._state is not None and snap is not None:
            self._state.copy_(snap)

    # ---- for a checkpoint's own extra key: plain Python values
    def state_dict(self):
        return dict(seed=self.seed, step=self.step, prob=float(self.prob), cutmix_share=float(self.cutmix_share),
                    mixup_alpha=float(self.mixup_alpha), cutmix_alpha=float(self.cutmix_alpha))

    def load_state_dict(self, sd):
        prob, share, a_mix, a_cut = (sd[k] for k in ("prob", "cutmix_share", "mixup_alpha", "cutmix_alpha"))
        seed = int(sd["seed"])
        if not 0 <= seed < 2 ** 32:
            raise ValueError(f"BatchMixer: seed {seed} of the state dict is outside [0, 2^32)")
        _unit("prob", prob), _unit("cutmix_share", share), _unit("mixup_alpha", a_mix, 0.05), _unit("cutmix_alpha", a_cut, 0.05)
        self.prob, self.cutmix_share, self.mixup_alpha, self.cutmix_alpha = prob, share, a_mix, a_cut
        self._seed = seed
        self.step = int(sd["step"])                              # writes seed, step and the hyper words when bound


def _check_mixer(mixer, criterion, what):
    """a mixed batch needs the criterion with two targets and a weight per row; returns it bound to the mixer"""
    if not isinstance(mixer, BatchMixer):
        raise ValueError(f"{what}: mixer must be a train.BatchMixer or None, got {type(mixer).__name__}")
    criterion = criterion if criterion is not None else MixedCrossEntropyLoss()
    if not isinstance(criterion, MixedCrossEntropyLoss):
        raise ValueError(f"{what} needs a train.MixedCrossEntropyLoss criterion (a mixed row has two targets and a weight, "
                         f"and every other criterion takes one integer target per row), got {type(criterion).__name__}")
    criterion.bind_mixer(mixer)
    return criterion


def _kd_number(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not lo <= v <= hi:      # a NaN fails the comparison
        raise ValueError(f"Distiller: {name} must be a number in [{lo}, {hi}], got {v!r}")
    return float(v)


class Distiller:
    """Knowledge distillation inside the train step: owns the frozen teacher and the two device words the distilled
    criterion reads (csrc/loss_eval.hip, hwgat_kd_*; formulas: include/hwgat_hip.h).  Every slice of a step the teacher sees
    the very input the student sees (after the mixer, when there is one) in an eval forward without gradients, and the
    slice's loss is (1 - alpha) hard + alpha T^2 KL(softmax(teacher / T) || softmax(student / T)).

        distiller = train.Distiller(teacher, alpha=0.5, temperature=4.0)
        step = train.GraphedTrainStep(student, opt, x, y, ragged=True, distiller=distiller)
        distiller.alpha = 0.0                    # the last epochs on the labels alone: the next replay, no new capture

    `alpha` in [0, 1] and `temperature` in [0.25, 32] are properties; when one changed, one hwgat_kd_set launch carries
    both to the device before the next step (`push_hyper`).  With alpha 0 the kernels do not read the teacher's logits
    and the loss and gradient have the undistilled criterion's bits (the teacher's forward still runs).  The teacher is
    put into eval() with requires_grad_(False) and stays the caller's: its weights are in no state dict of this object."""

    def __init__(self, teacher, alpha=0.5, temperature=4.0):
        if not isinstance(teacher, torch.nn.Module):
            raise ValueError(f"Distiller: teacher must be a torch.nn.Module, got {type(teacher).__name__}")
        self._alpha, self._tau = alpha, temperature
        self._hyper()
        self.teacher = teacher.eval().requires_grad_(False)
        self._state = self._pushed = None
        self.logits = None                       # the teacher's fp32 logits of the latest observe()

    def _hyper(self):
        """(alpha, temperature), validated, in the order of the device words"""
        HF = _functional()
        return (_kd_number("alpha", self._alpha, 0.0, 1.0),
                _kd_number("temperature", self._tau, HF.KD_TAU_MIN, HF.KD_TAU_MAX))

    @property
    def alpha(self):
        return self._alpha

    @alpha.setter
    def alpha(self, v):
        self._alpha = _kd_number("alpha", v, 0.0, 1.0)

    @property
    def temperature(self):
        return self._tau

    @temperature.setter
    def temperature(self, v):
        HF = _functional()
        self._tau = _kd_number("temperature", v, HF.KD_TAU_MIN, HF.KD_TAU_MAX)

    # ---- device side
    def bind(self, device):
        """allocate the two device words (once) and write them"""
        if self._state is not None:
            return self
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("Distiller needs an MI355X device; there is no CPU fallback")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Distiller: bind() before capturing")
        hyper = self._hyper()
        HF = _functional()
        self._state = HF.kd_state(device)
        HF.kd_set(self._state, *hyper)
        self._pushed = hyper
        return self

    @property
    def state(self):
        """the device words (alpha, tau) the criterion's kernels read; None before bind()"""
        return self._state

    def push_hyper(self):
        """one launch when alpha or the temperature changed since the last one, none otherwise (none while unbound)"""
        hyper = self._hyper()                    # validated before any launch
        if self._state is not None and hyper != self._pushed:
            _functional().kd_set(self._state, *hyper)
            self._pushed = hyper

    def observe(self, xs):
        """the teacher's eval forward of one slice, without gradients; keeps its fp32 logits for the criterion"""
        if self.teacher.training:
            raise RuntimeError("Distiller: the teacher is in train() mode -- it must stay in eval() (teacher.eval())")
        with torch.no_grad():
            self.logits = self.teacher(xs).float()
        return self.logits

    def _addresses(self):
        return tuple(t.data_ptr() for t in list(self.teacher.parameters()) + list(self.teacher.buffers()))

    # ---- for a checkpoint's own extra key: plain Python values
    def state_dict(self):
        alpha, tau = self._hyper()
        return dict(alpha=alpha, temperature=tau)

    def load_state_dict(self, sd):
        HF = _functional()
        alpha = _kd_number("alpha", sd["alpha"], 0.0, 1.0)
        tau = _kd_number("temperature", sd["temperature"], HF.KD_TAU_MIN, HF.KD_TAU_MAX)
        self._alpha, self._tau = alpha, tau
        self.push_hyper()


class DistilledCrossEntropyLoss(MixedCrossEntropyLoss):
    """MixedCrossEntropyLoss with a teacher (hwgat_kd_fwd / hwgat_kd_bwd of csrc/loss_eval.hip): a live row's loss is
    (1 - alpha) hard + alpha T^2 KL(teacher || student), `hard` the parent's row loss -- with a bound mixer the mixed one,
    read at the slice's place, without one the single-target loss of BatchSlicedCrossEntropyLoss.  alpha and T are the
    distiller's device words.  The step that owns the batch binds the distiller (`bind_distiller`), calls
    `place(n_rows, offset)` and `distiller.observe(slice)` before each slice.  `correct()`, `last_rank` and `last_pred` are
    the parent's; `last_kd` is the slice's share of the batch-mean KD term, `agree()` the number of live rows whose arg-max
    is the teacher's, `teacher_correct()` the number whose teacher arg-max (`last_teacher_pred`) is the dominant label."""

    def __init__(self, smooth_factor: float = 0.01, mixer=None, distiller=None):
        super().__init__(smooth_factor, mixer)
        self.distiller = distiller
        self.last_kd = self.last_teacher_pred = self._agree = self._t_hits = None

    def bind_distiller(self, distiller):
        if self.distiller is not None and self.distiller is not distiller:
            raise ValueError("DistilledCrossEntropyLoss is bound to another Distiller: one criterion serves one distiller")
        self.distiller = distiller

    def forward(self, input, target):
        d = self.distiller
        if self.n_rows is None or d is None or d.state is None or d.logits is None:
            raise RuntimeError("DistilledCrossEntropyLoss: bind_distiller(distiller), distiller.bind(device), "
                               "distiller.observe(slice) and place(n_rows, offset) first -- TrainStep(distiller=...) and "
                               "GraphedTrainStep(distiller=...) do")
        if tuple(d.logits.shape) != tuple(input.shape):
            raise ValueError(f"the teacher gives logits of shape {tuple(d.logits.shape)} for a slice on which the student gives "
                             f"{tuple(input.shape)}: distillation needs the same classes in the same order")
        y_b, lam = (None, None) if self.mixer is None else self._mixer_slice(input.shape[0])
        (loss, self.last_rank, self.last_pred, self._hits, self.last_teacher_pred, self.last_kd, self._agree,
         self._t_hits) = _functional().distilled_sliced_ce(input, d.logits, target, y_b, lam, d.state, self.smooth_factor,
                                                           self.n_rows, self.offset)
        return loss

    def agree(self):
        return self._agree

    def teacher_correct(self):
        return self._t_hits


def _check_distiller(distiller, criterion, model, reducer, what):
    """a distilled batch needs the criterion that takes the teacher's logits; returns it bound to the distiller"""
    if not isinstance(distiller, Distiller):
        raise ValueError(f"{what}: distiller must be a train.Distiller or None, got {type(distiller).__name__}")
    if distiller.teacher is model:
        raise ValueError(f"{what}: the teacher is the student object -- a model cannot be distilled from itself (the teacher "
                         "is frozen in eval(), the student trains)")
    if reducer is not None:
        raise NotImplementedError("distiller with a reducer: multi-rank distillation is not built")
    criterion = criterion if criterion is not None else DistilledCrossEntropyLoss()
    if not isinstance(criterion, DistilledCrossEntropyLoss):
        raise ValueError(f"{what} needs a train.DistilledCrossEntropyLoss criterion (a distilled row has the teacher's logits "
                         f"beside its labels, and every other criterion takes labels only), got {type(criterion).__name__}")
    criterion.bind_distiller(distiller)
    return criterion


def _check_micro_batch(micro_batch):
    if micro_batch is not None and (isinstance(micro_batch, bool) or not isinstance(micro_batch, numbers.Integral)
                                    or micro_batch < 1):
        raise ValueError(f"micro_batch must be a positive integer or None, got {micro_batch!r}")
    return None if micro_batch is None else int(micro_batch)


def _check_padded(model, criterion, what):
    """a zero-padded batch needs a criterion that knows the real row count and a train forward that keeps clips apart"""
    if not isinstance(criterion, BatchSlicedCrossEntropyLoss):
        raise ValueError(f"{what} needs a train.BatchSlicedCrossEntropyLoss criterion (a batch mean over the real rows "
                         f"only), got {type(criterion).__name__}")
    if not getattr(model, "clips_independent_in_train", False):
        raise ValueError(f"{what}: the train forward of {type(model).__name__} couples the clips of a batch "
                         "(clips_independent_in_train is not set), padding rows would enter its batch statistics")


class _PaddedBatch:
    """static (B, ...) input and target buffers for batches of 1..B rows: the rows, zeros behind them, and the row count in
    the device int32 word `n_rows` (written only when it changed, as evaluate.Evaluator.update does)"""

    def __init__(self, B, x, y):
        self.x = x.new_zeros((B,) + tuple(x.shape[1:]))
        self.y = y.new_zeros((B,))
        self.n_rows = torch.full((1,), B, device=x.device, dtype=torch.int32)
        self.rows = B

    def load(self, x, y):
        n, B = x.shape[0], self.x.shape[0]
        if not 1 <= n <= B or x.shape[1:] != self.x.shape[1:] or y.shape != (n,):
            raise ValueError(f"built for 1 to {B} clips of {tuple(self.x.shape[1:])}, got {tuple(x.shape)} with targets "
                             f"{tuple(y.shape)}")
        if x.data_ptr() != self.x.data_ptr():
            self.x[:n].copy_(x, non_blocking=True)
        if y.data_ptr() != self.y.data_ptr():
            self.y[:n].copy_(y, non_blocking=True)
        if n != self.rows:
            self.x[n:].zero_()                               # rows a longer batch left behind
            self.y[n:].zero_()
            self.n_rows.fill_(n)
            self.rows = n


def _run_slices(model, criterion, x, y, mb, weighted=True, n_rows=None, distiller=None):
    """forward, loss and backward of x / y in slices of `mb` rows, gradients accumulating; (loss, correct) summed in slice
    order.  `weighted`: the slice's mean loss times n_i / n.  `n_rows`: the batch is zero-padded, the criterion is told
    each slice's place and returns its share of the mean as it is.  Nothing of a slice outlives its backward but the sums.
    `distiller`: its teacher sees each slice before the student does, and the criterion's three distillation sums
    (kd, agree, teacher_correct) are left, summed the same way, in `criterion.step_sums`."""
    n = x.shape[0]
    total = correct = sums = None
    for i in range(0, n, mb):
        xs, ys = x[i:i + mb], y[i:i + mb]
        if n_rows is not None:
            criterion.place(n_rows, i)
        if distiller is not None:
            distiller.observe(xs)
        out = model(xs)
        loss = criterion(out, ys)
        if weighted:
            loss = loss * (xs.shape[0] / n)
        loss.backward()
        total = loss.detach() if total is None else total + loss.detach()
        c = _correct(criterion, out, ys)
        correct = c if correct is None else correct + c
        if distiller is not None:
            part = (criterion.last_kd, criterion.agree(), criterion.teacher_correct())
            sums = part if sums is None else tuple(a + b for a, b in zip(sums, part))
        del out, loss, c
    if distiller is not None:
        criterion.step_sums = sums
    return total, correct


def _correct(criterion, out, y):
    """correct-count of the batch the criterion has just seen: its own when it keeps one, else the argmax line"""
    if hasattr(criterion, "correct"):
        return criterion.correct()
    return (out.detach().argmax(-1) == y).sum()


def _guard_of(optimizer):
    """the GradGuard of a device optimizer that carries one, else None"""
    import importlib
    if isinstance(optimizer, importlib.import_module(__package__ + ".optim").DeviceOptimizer):
        return optimizer.guard
    return None


class TrainStep:
    """zero_grad -> forward -> loss -> backward (-> bucketed all-reduce) -> optimizer.

    Unlike utils.train (utils.py:109,114) nothing here reads a value back to the
    host: loss and correct-count stay on the device until the caller asks.

    `micro_batch`: process the batch in slices of that many clips and accumulate gradients
    (same mean-loss gradient).  Activations saved for backward are 10*E floats per block
    (DESIGN.md section 3); BASELINE config 5 (B=256, T=256, K=112, d0=256) would need ~600 GB
    in one piece, 16-clip slices need ~38 GB.

    `pad_to=B`: every batch of 1..B clips is zero-padded to B rows and runs as B rows, sliced by `micro_batch` as
    a full batch would be; the real row count sits in the device word `n_rows` and the criterion -- a
    `BatchSlicedCrossEntropyLoss`, the default then -- takes the mean over the real rows only, so loss, `correct` and the
    gradient are those of the real rows (a padding row has finite activations and an exactly zero upstream gradient:
    DESIGN.md section 6o).  This is what `GraphedTrainStep(ragged=True)` captures, run eagerly: the two agree bit for bit
    under `deterministic_train`.  Models whose train forward couples clips (ST-GCN, DecoupledGCN) are refused.  `None`
    (the default): the batch runs as it comes.

    `meter`: a `TrainMeter`; every call ends with its fold launch (after the optimizer's and the averager's), which adds
    the step's loss, correct count and row count -- and the verdict and norm of the device optimizer's guard -- to the
    meter's device words.  `None` (the default): the launch sequence is what it has always been.

    `mixer`: a `BatchMixer`; every call starts with its two launches, which mix the whole batch -- the padded buffer, or a
    copy of `x`: never the caller's tensor -- before any slicing, so partners may sit in different micro-batches.  The
    criterion is a `MixedCrossEntropyLoss` (the default then; anything else is refused) and is told each slice's place,
    with `pad_to` or without (the row count is then a constant word).  BatchNorm models take a mixer without `pad_to`.
    Without `pad_to` the mixer is bound to the first batch's `(B, T)` and every later batch must have that many rows (a
    short last batch raises: drop it, or use `pad_to`).
    `None` (the default): nothing changes.

    `distiller`: a `Distiller`; before each slice's student forward its teacher runs an eval forward of the same slice
    (after the mixer, when there is one) and the criterion -- a `DistilledCrossEntropyLoss`, the default then; anything
    else is refused -- blends the labels' loss with the KL from the teacher's logits.  It is told each slice's place with
    `pad_to` or without (the row count is then a constant word).  `kd`, `agree` and `teacher_correct` hold the step's
    slice sums beside `loss` and `correct`.  A `reducer` is refused.  `None` (the default): nothing changes."""

    def __init__(self, model, optimizer=None, reducer=None, criterion=None, micro_batch=None, pad_to=None, meter=None,
                 mixer=None, distiller=None):
        self.model, self.opt, self.reducer, self.meter, self.mixer = model, optimizer, reducer, meter, mixer
        self.distiller = distiller
        self.kd = self.agree = self.teacher_correct = None
        self.pad_to, self._pad, self._all_rows = pad_to, None, None     # _all_rows: (n, the constant word holding n)
        if distiller is not None:
            criterion = _check_distiller(distiller, criterion, model, reducer, "TrainStep(distiller=...)")
        if mixer is not None:
            criterion = _check_mixer(mixer, criterion, "TrainStep(mixer=...)")
        if pad_to is not None:
            if isinstance(pad_to, bool) or not isinstance(pad_to, numbers.Integral) or pad_to < 1:
                raise ValueError(f"pad_to must be a positive integer or None, got {pad_to!r}")
            _check_micro_batch(micro_batch)
            if reducer is not None:
                raise NotImplementedError("pad_to with a reducer: ranks with different row counts need a weighted mean")
            criterion = criterion or BatchSlicedCrossEntropyLoss()
            _check_padded(model, criterion, "TrainStep(pad_to=...)")
        self.criterion = criterion or SmoothedCrossEntropyLoss()
        self.micro_batch = micro_batch
        self.loss = None
        self.correct = None

    @property
    def n_rows(self):
        """the device int32 word with the latest batch's real row count (`pad_to` only; None before the first call)"""
        return None if self._pad is None else self._pad.n_rows

    def __call__(self, x, y):
        if self.pad_to is not None:
            if self._pad is None:
                self._pad = _PaddedBatch(int(self.pad_to), x, y)
            self._pad.load(x, y)
            x, y = self._pad.x, self._pad.y
        n = x.shape[0]
        place = self.n_rows
        if self.mixer is not None or self.distiller is not None:
            if self.pad_to is None:                          # a buffer of the step's own, and the constant row count
                if self.mixer is not None:
                    x = x.detach().clone()
                if self._all_rows is None or self._all_rows[0] != n:
                    self._all_rows = (n, torch.full((1,), n, device=x.device, dtype=torch.int32))
                place = self._all_rows[1]
        if self.mixer is not None:
            self.mixer.apply(x, y, self.n_rows)
        if self.distiller is not None:
            self.distiller.bind(x.device).push_hyper()
        mb = self.micro_batch if self.micro_batch and self.micro_batch < n else n
        n_acc = (n + mb - 1) // mb
        if self.reducer is not None:
            self.reducer.zero_grad(n_acc)
        elif self.opt is not None:
            self.opt.zero_grad(set_to_none=True)
        total, correct = _run_slices(self.model, self.criterion, x, y, mb, weighted=place is None, n_rows=place,
                                     **({} if self.distiller is None else dict(distiller=self.distiller)))
        if self.distiller is not None:
            self.kd, self.agree, self.teacher_correct = self.criterion.step_sums
        if self.reducer is not None:
            self.reducer.finish()
        if self.opt is not None:
            self.opt.step()
        self.loss, self.correct = total, correct
        if self.meter is not None:
            self.meter.fold(total, correct, n_rows=self.n_rows, batch_rows=n, guard=_guard_of(self.opt))
        return self.loss


class GraphedTrainStep:
    """The train step -- seed advance, forward, loss, backward and, with a device optimizer (`optim.DeviceAdamW`,
    `optim.DeviceSGD`, `optim.DeviceNAdam`), the optimizer step --
    captured ONCE in a HIP graph and replayed per call: one graph launch instead of ~400 kernels issued one by one from Python
    (reference loop: hwgat/utils.py:93-116, which issues its ~40 ATen ops per block the same way).  Why it matters here: the bf16 steps
    of the sibling models are 10-17 ms, within 10 % of what one Python thread can issue, and a node runs 8 such ranks
    (SURVEY 8e); a replay needs no host work between kernels.

    What makes the capture possible (round 4): nothing in a step depends on a host value that changes between steps.
    The dropout seed lives on the device (`model._seed_state`; every seeded kernel adds the step's base seed, which
    hwgat_seed_advance -- the first node of the graph -- rewrites), the train-mode thresholds of HWGATE.py:96 are drawn
    by torch's graph-safe device generator, and every C-ABI launch goes to torch's current stream, so HIP stream capture
    records it like torch's own kernels.  Capture follows the torch.cuda.graphs recipe (warm-up on a side stream, then
    `torch.cuda.graph`), in THIS process: nothing is re-launched or exec'ed.

    The optimizer.  With an `optim.DeviceOptimizer` (AdamW / Adam, SGD, NAdam: every optimizer type of the reference) the
    step is two more nodes of the graph (hwgat_opt_advance and hwgat_opt_step with the class's `kind`): its
    hyper-parameters are fp64 device words that the kernels read when they run, so `__call__` only
    pushes the param groups' values when they changed (hwgat_opt_set, one tiny launch, e.g. after
    `scheduler.step()`) and replays; the optimizer's Python `step` is not entered, and a replay is the whole train step.
    The kernels and their inputs are the eager step's, so a replay and an eager TrainStep step agree bit for bit under
    `deterministic_train`, with any scheduler (tests/test_gpu_optim.py, tests/test_gpu_optim_family.py).  The warm-up's
    traces in the optimizer are undone through its `snapshot_state` / `restore_state`, DeviceSGD's private
    "stepped before" words included: the first replay of a fresh SGD with momentum sets its buffers to the gradient.

    Clipping and divergence.  A device optimizer that carries an `optim.GradGuard` (`optimizer.guard`) issues the guard's
    three launches in front of its own two, so they are nodes of the graph as well: every replay clips the gradients by
    their global norm and, in the guard's "skip" mode, leaves weights, state and step counts alone when a gradient holds
    a NaN or an Inf.  The norm, the coefficient and the counters stay in device words (`guard.total_norm`,
    `guard.clip_coef`, `guard.counters()`); a new `guard.max_norm` reaches the next replay like a new lr.  With a
    `reducer` the guard runs after `reducer.finish()`: each rank sees the all-reduced gradients and so the same norm.
    The warm-up leaves the guard's counters where they were (zero for a new guard).

    Weight averaging.  A device optimizer that carries an `optim.WeightAverage` (`optimizer.averager`) issues the
    averager's two launches behind its own, so every replay also updates the EMA / SWA of the weights, once per replay
    whatever `micro_batch` is, and not at all when the guard skipped the step.  The warm-up leaves the averages and their
    counters as they were.  While the averaged weights are swapped in (`averager.is_applied`) a call raises.

    With any other optimizer the step stays out of the graph and is issued right after the replay, so that it reads the
    param groups' hyper-parameters when it runs: a float lr captured in the graph would be frozen there (an lr scheduler
    would change nothing), and a tensor lr is read by torch's fused AdamW as float32 -- the float lr rounded, updates that
    differ from the eager step's.  Out of the graph it is the eager step's own call on the gradients the replay wrote,
    so the same bit-equality holds.  That optimizer must be AdamW / Adam(fused=True, capturable=True): its step counts
    live on the device, and nothing in the step waits on the host.

    Micro-batches.  `micro_batch=mb` captures the step `TrainStep(micro_batch=mb)` takes: the static batch runs in slices
    `x[i:i+mb]` (a shorter last one at its own shape), each with its own forward, loss `criterion(out_i, y_i) * (n_i / n)`
    and backward, the later ones accumulating into the gradient tensors the first one left -- the tensors the optimizer
    table, the guard and `_grads` hold -- and the optimizer (and guard) once after the last.  `loss` / `correct` are the
    slice sums in slice order; `n_slices` forwards advance the dropout counter `n_slices` times, so slice j of replay k
    draws what the eager step's slice j of step k draws, and a BatchNorm model normalises and advances its running
    statistics per slice, as the eager step does.  A slice's saved activations are released inside the capture before the
    next slice's forward (nothing of a slice is kept but the running sums), so the graph's pool holds one slice's
    activations: that is what lets BASELINE config 5 into a graph at all.  `None` or a value >= the batch is the
    unsliced step, node for node.  With a `reducer` it raises: RCCL inside a capture is untested.

    Short batches.  `ragged=True` makes the step built for B rows take any 1 <= n <= B: `__call__` copies the n rows, zeroes
    the rest, writes n into the device int32 word `n_rows` (only when n changed) and replays the same graph.  The criterion
    must be a `BatchSlicedCrossEntropyLoss` (the default then): it is told each slice's place in the batch and takes the
    mean over the real rows, so loss, `correct` and the gradients are the n real clips' (DESIGN.md section 6o has the
    argument).  A replay costs the same whatever n is.  Models whose train forward couples the clips of a batch
    (`clips_independent_in_train` False: ST-GCN, DecoupledGCN) are refused.  `TrainStep(pad_to=B)` is the same computation
    issued eagerly.

    Meters.  `meter=TrainMeter(...)` makes the meter's fold the last launch of the step and so the last node of the graph,
    behind the optimizer's and the averager's, once per replay whatever `micro_batch` is: it adds the summed `loss` and
    `correct`, the ragged step's `n_rows` word (else the static batch size) and the guard's verdict and norm to the
    meter's device words, so a training loop reads its epoch's numbers once (`meter.close_epoch()`, `meter.history()`)
    instead of `loss` / `correct` after every replay.  With an optimizer that stays out of the graph the fold is still
    captured, after the backward.  The warm-up leaves the meter as it found it.  `None` (the default): the captured node
    sequence is what it has always been.

    Mixing.  `mixer=BatchMixer(...)` makes the mixer's two launches (hwgat_mix_draw, hwgat_mix_apply) the first nodes of
    the graph, in front of the first forward: every replay matches the live rows of the static batch into pairs and mixes
    the static input buffer in place, once, before any slicing (partners may sit in different micro-batches).  The
    criterion must be a `MixedCrossEntropyLoss` (the default then), which is told each slice's place with `ragged` or
    without (the row count is then a constant word).  The mixer's hyper-parameters are device words: `mixer.prob = 0.0`
    reaches the next replay like a new lr.  The warm-up leaves the mixer's step counter where it was: with `mixer.step = c`
    before construction, replay k draws what the eager step draws in its k-th call from the same `c`.  A replay rewrites
    `step.x`; a caller that stages its batches there (`loader.bind(step.x, step.y)`) writes a fresh batch before every
    replay anyway.  BatchNorm models take a mixer without `ragged`.  `None` (the default): nothing changes.

    Distillation.  `distiller=Distiller(teacher, ...)` makes the teacher's eval forward of each slice and the distilled
    criterion's launches (hwgat_kd_fwd, hwgat_kd_bwd) nodes of the same graph: per slice the teacher's forward on the
    static input (behind the mixer's launches, when there is a mixer), then the student's forward, the criterion -- a
    `DistilledCrossEntropyLoss`, the default then; anything else is refused -- and the backward.  The criterion is told
    each slice's place with `ragged` or without (the row count is then a constant word).  alpha and the temperature are
    device words: `distiller.alpha = 0.0` reaches the next replay like a new lr, and from then on the replays leave the
    weights the undistilled step leaves.  `kd`, `agree` and `teacher_correct` are static device tensors with the slice sums
    in slice order, like `loss` and `correct`; the meter's loss is the step's total loss.  The teacher's parameters and
    buffers must not be reallocated after the capture either; the warm-up leaves nothing behind in the teacher, and no
    replay writes to it.  The teacher must not be the student, and a `reducer` is refused.  `None` (the default): the
    captured node sequence is what it has always been.

    Inputs are copied into static buffers; `loss` / `correct` are static device tensors rewritten by every replay.
    Shapes are fixed at capture.  Parameters must not be reallocated afterwards (same rule as serve.GraphedEval).
    The warm-up's traces in the model's buffers (BatchNorm running statistics) are undone like those in the weights.
    With `model._drop_calls = c` before construction, replay k (1-based) draws exactly the masks the eager TrainStep
    draws in its k-th step from the same `c` (tests/test_gpu_graph.py).  Each forward hands its kernels a per-call copy of
    the base seed (seeding.DeviceSeeds._next_step_seed); in the graph that copy is a node after the seed advance."""

    def __init__(self, model, optimizer, x, y, criterion=None, warmup=2, reducer=None, micro_batch=None, ragged=False,
                 meter=None, mixer=None, distiller=None):
        import importlib
        HF = importlib.import_module(__package__ + ".functional")
        micro_batch = _check_micro_batch(micro_batch)
        if micro_batch is not None and reducer is not None:
            raise NotImplementedError("micro_batch with a reducer: the all-reduce inside a capture is untested")
        if distiller is not None:
            criterion = _check_distiller(distiller, criterion, model, reducer, "GraphedTrainStep(distiller=...)")
        if mixer is not None:
            criterion = _check_mixer(mixer, criterion, "GraphedTrainStep(mixer=...)")
        if ragged:
            if reducer is not None:
                raise NotImplementedError("ragged with a reducer: ranks with different row counts need a weighted mean")
            criterion = criterion or BatchSlicedCrossEntropyLoss()
            _check_padded(model, criterion, "GraphedTrainStep(ragged=True)")
        if not x.is_cuda:
            raise ValueError("GraphedTrainStep needs device inputs")
        if not model.training:
            raise ValueError("GraphedTrainStep captures the train() step: call model.train() first")
        self.in_graph = isinstance(optimizer, importlib.import_module(__package__ + ".optim").DeviceOptimizer)
        for grp in optimizer.param_groups:
            if not self.in_graph and not grp.get("capturable", False):
                raise ValueError("the optimizer must be built with capturable=True (its step count then lives on the device)")
        self.model, self.opt, self.reducer, self.meter, self.mixer = model, optimizer, reducer, meter, mixer
        self.distiller = distiller
        self.kd = self.agree = self.teacher_correct = None
        self.criterion = criterion or SmoothedCrossEntropyLoss()
        self.ragged, self._pad = bool(ragged), None
        if self.ragged:
            self._pad = _PaddedBatch(x.shape[0], x, y)
            self._pad.load(x.detach(), y.detach())
            self.x, self.y = self._pad.x, self._pad.y
        else:
            self.x, self.y = x.detach().clone(), y.detach().clone()
        B = x.shape[0]
        # the word the criterion is placed with: the ragged step's row count, or -- for a mixer without it -- the constant B
        self._place = self.n_rows
        if mixer is not None:
            mixer.bind(x.device, B, x.shape[1]).push_hyper()  # state and records exist before the capture
            if self._place is None:
                self._place = torch.full((1,), B, device=x.device, dtype=torch.int32)
        if distiller is not None:
            distiller.bind(x.device).push_hyper()            # the two words exist before the capture
            if self._place is None:
                self._place = torch.full((1,), B, device=x.device, dtype=torch.int32)
        self.micro_batch = micro_batch if micro_batch is not None and micro_batch < B else B
        self.n_slices = (B + self.micro_batch - 1) // self.micro_batch
        start = int(model._drop_calls)
        dev = x.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        # warm-up (allocator, weight-prep caches, optimizer state) on a side stream with the weights and the optimizer
        # state put back afterwards, so that capture changes nothing the caller can observe
        keep_p = [p.detach().clone() for p in model.parameters()]
        keep_b = [b.clone() for b in model.buffers()]
        if self.in_graph:                                # also the words the optimizer keeps to itself (DeviceSGD's)
            keep_state = optimizer.snapshot_state()
        else:
            keep_state = {p: {k: v.clone() for k, v in st.items() if torch.is_tensor(v)} for p, st in optimizer.state.items()}
        keep_meter = None if meter is None else meter.bind(dev).snapshot()   # the block exists before the capture
        keep_mixer = None if mixer is None else mixer.snapshot()
        keep_x = None if mixer is None else self.x.clone()   # the warm-up mixes the static batch in place
        keep_t = None if distiller is None else [b.clone() for b in distiller.teacher.buffers()]
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self._one()
                if mixer is not None:
                    self.x.copy_(keep_x)
        torch.cuda.current_stream(dev).wait_stream(side)
        with torch.no_grad():
            for p, q in zip(model.parameters(), keep_p):
                p.copy_(q)
            for b, q in zip(model.buffers(), keep_b):    # BatchNorm running statistics and batch counts
                b.copy_(q)
            if self.in_graph:                            # state back to what it was, fresh where it is new
                optimizer.restore_state(keep_state)
            else:
                for p, st in optimizer.state.items():    # moments / step counters: back to what they were (zero if new)
                    for k, v in st.items():
                        if torch.is_tensor(v):
                            if p in keep_state and k in keep_state[p]:
                                v.copy_(keep_state[p][k])
                            else:
                                v.zero_()
            if meter is not None:                        # the warm-up's folds never happened
                meter.restore(keep_meter)
            if mixer is not None:                        # nor its draws: the step counter is where the caller left it
                mixer.restore(keep_mixer)
            if distiller is not None:                    # an eval forward writes no buffer; should one, it is undone
                for b, q in zip(distiller.teacher.buffers(), keep_t):
                    b.copy_(q)
        del keep_p, keep_b, keep_state, keep_meter, keep_mixer, keep_x, keep_t
        model.device_seed_counter = True                 # from here on the device counts the steps itself
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        if self.in_graph:
            optimizer.push_hyper()
            optimizer.begin_capture()
        try:
            with torch.cuda.graph(self.graph):
                self.loss, self.correct = self._one(step=self.in_graph)
        finally:
            # the table the captured optimizer launches read: uploaded now (capture executed nothing), owned by this object
            self._opt_table = optimizer.end_capture() if self.in_graph else None
        # capture executed nothing: put the device counter where the host mirror says the caller left it
        model._drop_calls = start
        HF.seed_set(model._seed_state, start, torch.initial_seed(), getattr(model, "rank_salt", 0))
        self._addr = self._addresses()
        # the static gradients every replay writes: what the optimizer step after a replay reads (put back on the
        # parameters per call, in case something -- an eager step's zero_grad(set_to_none=True) -- detached them)
        self._grads = [(p, p.grad) for p in model.parameters() if p.grad is not None]

    @property
    def n_rows(self):
        """the device int32 word with the latest batch's real row count (`ragged` only, else None)"""
        return None if self._pad is None else self._pad.n_rows

    def _one(self, step=True):
        self.opt.zero_grad(set_to_none=True)
        if self.mixer is not None:                       # once, on the whole static batch, before any slicing
            self.mixer.apply(self.x, self.y, self.n_rows)
        if self.n_slices == 1 and self._place is None:   # the unsliced step, node for node what it has always been
            out = self.model(self.x)
            loss = self.criterion(out, self.y)
            loss.backward()
            if self.reducer is not None:
                self.reducer.finish()
            if step:
                self.opt.step()
            return self._fold(loss.detach(), _correct(self.criterion, out, self.y))
        loss, correct = _run_slices(self.model, self.criterion, self.x, self.y, self.micro_batch, weighted=self._place is None,
                                    n_rows=self._place, **({} if self.distiller is None else dict(distiller=self.distiller)))
        if self.distiller is not None:                   # static tensors of the graph's pool, like loss and correct
            self.kd, self.agree, self.teacher_correct = self.criterion.step_sums
        if step:                                         # once, after the last slice (no reducer here: refused above)
            self.opt.step()
        return self._fold(loss, correct)

    def _fold(self, loss, correct):
        """the meter's launch, the last of the step: once per step, on the sums the step returns"""
        if self.meter is not None:
            self.meter.fold(loss, correct, n_rows=self.n_rows, batch_rows=self.x.shape[0],
                            guard=_guard_of(self.opt) if self.in_graph else None)
        return loss, correct

    def _addresses(self):
        own = tuple(t.data_ptr() for t in list(self.model.parameters()) + list(self.model.buffers()))
        return own if self.distiller is None else own + self.distiller._addresses()

    def __call__(self, x, y):
        if not self.model.training:
            raise ValueError("GraphedTrainStep replays the train() step: call model.train() first")
        if not self.ragged and (x.shape != self.x.shape or y.shape != self.y.shape):
            raise ValueError(f"captured for {tuple(self.x.shape)} / {tuple(self.y.shape)}, got {tuple(x.shape)} / {tuple(y.shape)}")
        if self._addresses() != self._addr:
            raise RuntimeError("a parameter or buffer of the model" + (" or of the teacher" if self.distiller is not None else "")
                               + " was reallocated after the capture: capture again")
        averager = getattr(self.opt, "averager", None)
        if averager is not None:                         # a replay bypasses the optimizer's step() and its check
            averager._refuse_applied("a GraphedTrainStep replay")
        if self.ragged:
            self._pad.load(x, y)                         # the rows, zeros behind them, the row count when it changed
        else:
            if x.data_ptr() != self.x.data_ptr():
                self.x.copy_(x, non_blocking=True)
            if y.data_ptr() != self.y.data_ptr():
                self.y.copy_(y, non_blocking=True)
        if self.in_graph:
            self.opt.push_hyper()                        # launches only when a param group's values changed
        if self.mixer is not None:
            self.mixer.push_hyper()                      # likewise
        if self.distiller is not None:
            if self.distiller.teacher.training:
                raise RuntimeError("Distiller: the teacher is in train() mode -- the captured step holds its eval() forward")
            self.distiller.push_hyper()                  # likewise
        self.graph.replay()
        self.model._drop_calls += self.n_slices          # host mirror of the device counter (model._seeds() in tests)
        for p, g in self._grads:
            if p.grad is not g:
                p.grad = g
        if self.in_graph:
            self.opt._opt_called = True                  # what torch's LR schedulers look for before their first step
        else:
            self.opt.step()                              # on the gradients the replay wrote, with the current lr
        return self.loss


# ---------------------------------------------------------------------------------------------------- train meters
# The meter block of csrc/train_meter.hip in 8-byte words; the constants mirror HWGAT_METER_* of include/hwgat_hip.h
METER_LOG_TOTAL, METER_CLOSED, METER_OVERFLOW = 0, 1, 2
METER_RUN, METER_NRUN = 4, 12
METER_LOG = METER_RUN + METER_NRUN
(METER_R_STEPS, METER_R_ROWS, METER_R_CORRECT, METER_R_LOSS_SUM, METER_R_FINITE_STEPS, METER_R_NONFINITE_LOSS,
 METER_R_SKIPPED, METER_R_LAST_LOSS, METER_R_MAX_LOSS, METER_R_MAX_GRAD_NORM) = range(10)
METER_MAX_CAPACITY = 1 << 24
_METER_INTS = (("steps", METER_R_STEPS), ("rows", METER_R_ROWS), ("correct", METER_R_CORRECT),
               ("finite_steps", METER_R_FINITE_STEPS), ("nonfinite_loss", METER_R_NONFINITE_LOSS),
               ("skipped", METER_R_SKIPPED))


def _meter_entry(words):
    """METER_NRUN int64 words (the running words, or a closed epoch) as a dict: the raw words under their own names, and
    `loss` = loss_sum / finite_steps (utils.py:116's total_loss / num_batches when every loss is finite), `acc` = correct /
    rows (its sum(train_acc) / len(train_acc))"""
    w = np.ascontiguousarray(words, dtype=np.int64)
    f64, f32 = w.view(np.float64), w.view(np.float32)         # an fp32 word sits in the low four bytes: index 2 i
    d = {name: int(w[i]) for name, i in _METER_INTS}
    d.update(loss_sum=float(f64[METER_R_LOSS_SUM]), last_loss=float(f32[2 * METER_R_LAST_LOSS]),
             max_loss=float(f32[2 * METER_R_MAX_LOSS]), max_grad_norm=float(f64[METER_R_MAX_GRAD_NORM]))
    d["loss"] = d["loss_sum"] / max(d["finite_steps"], 1)
    d["acc"] = d["correct"] / max(d["rows"], 1)
    return d


class TrainMeter:
    """What a training loop reports per epoch, summed on the device (csrc/train_meter.hip): the reference's train()
    reads `loss.item()` and the correct predictions back after every batch (utils.py:109-114); a meter handed to
    `GraphedTrainStep` / `TrainStep` (`meter=`) folds them in with one launch at the end of every step -- a node of the
    graph -- and the host reads when it wants to.

        meter = train.TrainMeter(log_capacity=256)
        step = train.GraphedTrainStep(model, opt, x, y, ragged=True, meter=meter)
        for x, y in loader: step(x, y)          # nothing is read back
        meter.close_epoch()                      # the running words become the next entry of history()
        meter.history()[-1]["loss"], meter.history()[-1]["acc"]

    The running words of the open epoch: steps, rows (real rows), correct, loss_sum (fp64, one addition per step in step
    order: bit for bit Python's `total += loss.item()`), finite_steps, nonfinite_loss (steps with a NaN or Inf loss: counted,
    not added), skipped (steps the optimizer's GradGuard turned into a no-op), last_loss, max_loss (over the finite
    losses), max_grad_norm (the largest norm the guard reported; a NaN norm never counts, an Inf one does).
    `log_capacity` > 0 also keeps the latest that many steps' (loss, correct, rows, grad_norm) in a ring: the loss curve
    per step without a sync.  `history_capacity` closed epochs are kept; a close past it overwrites the last entry and is
    counted (`overflow`).

    The block is allocated by `bind(device)` or the first `fold`, never inside a capture."""

    def __init__(self, log_capacity=0, history_capacity=1024):
        for name, v in (("log_capacity", log_capacity), ("history_capacity", history_capacity)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v <= METER_MAX_CAPACITY:
                raise ValueError(f"TrainMeter: {name} must be an integer in [0, {METER_MAX_CAPACITY}], got {v!r}")
        self.log_capacity, self.history_capacity = int(log_capacity), int(history_capacity)
        self._block = None           # device block, int64 words
        self._loaded = None          # the words of a load_state_dict() that came before the device block existed

    @property
    def words(self):
        """length of the block in 8-byte words"""
        return METER_LOG + 2 * self.log_capacity + METER_NRUN * self.history_capacity

    # ---- device side
    def bind(self, device):
        """allocate the block on `device` (once; a meter serves one device)"""
        device = torch.device(device)
        if self._block is None:
            if device.type != "cuda":
                raise RuntimeError("TrainMeter needs an MI355X device; there is no CPU fallback")
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TrainMeter: fold once (or bind()) before capturing")
            HF = _functional()
            if HF.meter_words(self.log_capacity, self.history_capacity) != self.words:
                raise RuntimeError("TrainMeter: the library lays the block out differently from train.py's constants")
            self._block = torch.zeros(self.words, dtype=torch.int64, device=device)
            if self._loaded is not None:
                self._block.copy_(torch.from_numpy(self._loaded))
                self._loaded = None
        elif self._block.device != device and not (device.index is None and self._block.device.type == device.type):
            raise ValueError(f"TrainMeter lives on {self._block.device}, the step on {device}")
        return self

    def fold(self, loss, correct, n_rows=None, batch_rows=None, guard=None):
        """one launch: add a step.  `loss` its fp32 device word, `correct` its int64 one; the row count is the device
        int32 word `n_rows` or, without one, the host integer `batch_rows`; `guard` an `optim.GradGuard` (or its fp64
        block) whose skip verdict and norm of this step are recorded, or None"""
        if n_rows is None and batch_rows is None:
            raise ValueError("TrainMeter.fold: give the row count, as the device word n_rows or the integer batch_rows")
        self.bind(loss.device)
        state = guard
        if guard is not None and not torch.is_tensor(guard):
            state = guard.bind(loss.device)._bound()
        _functional().meter_fold(self._block, loss, correct, n_rows, 0 if batch_rows is None else batch_rows, state,
                                 self.log_capacity, self.history_capacity)

    def close_epoch(self):
        """one launch: the running words become the next closed epoch and start again from zero; the step log goes on"""
        if self._block is None:
            raise RuntimeError("TrainMeter has folded nothing yet: its block lives on the device of its first step (or bind())")
        _functional().meter_close(self._block, self.log_capacity, self.history_capacity)

    def reset(self):
        """everything back to zero: running words, step log, closed epochs"""
        self._loaded = None
        if self._block is not None:
            self._block.zero_()

    # ---- what a warm-up must not leave behind
    def snapshot(self):
        return None if self._block is None else self._block.clone()

    def restore(self, snap):
        if self._block is not None:
            if snap is None:
                self._block.zero_()
            else:
                self._block.copy_(snap)

    # ---- readouts: each is ONE host read
    def _host(self):
        if self._block is not None:
            return self._block.cpu().numpy()
        return np.zeros(self.words, dtype=np.int64) if self._loaded is None else self._loaded.copy()

    def result(self):
        """the open epoch so far, as a dict (see the class docstring; `loss` and `acc` as the reference computes them)"""
        return self._result(self._host())

    @staticmethod
    def _result(h):
        d = _meter_entry(h[METER_RUN:METER_LOG])
        d.update(log_total=int(h[METER_LOG_TOTAL]), epochs_closed=int(h[METER_CLOSED]), overflow=int(h[METER_OVERFLOW]))
        return d

    def _history(self, h):
        kept = min(int(h[METER_CLOSED]), self.history_capacity)
        base = METER_LOG + 2 * self.log_capacity
        return [_meter_entry(h[base + i * METER_NRUN:base + (i + 1) * METER_NRUN]) for i in range(kept)]

    def history(self):
        """the closed epochs, oldest first, one dict each; after an overflow the last one is the latest close"""
        return self._history(self._host())

    def step_log(self):
        """the logged steps in step order: dicts of step (its number since the last reset, from 0), loss, correct, rows,
        grad_norm; the latest `log_capacity` of them"""
        h = self._host()
        total, cap = int(h[METER_LOG_TOTAL]), self.log_capacity
        ring = h[METER_LOG:METER_LOG + 2 * cap]
        f32, i32 = ring.view(np.float32), ring.view(np.int32)
        out = []
        for r in range(max(0, total - cap), total):
            s = 4 * (r % cap)
            out.append(dict(step=r, loss=float(f32[s]), correct=int(i32[s + 1]), rows=int(i32[s + 2]),
                            grad_norm=float(f32[s + 3])))
        return out

    # ---- for a checkpoint's own extra key: plain Python values, the words as integers (exact for the fp64 sums too)
    def state_dict(self):
        h = self._host()
        kept = min(int(h[METER_CLOSED]), self.history_capacity)
        base = METER_LOG + 2 * self.log_capacity
        return dict(log_capacity=self.log_capacity, history_capacity=self.history_capacity,
                    head=[int(v) for v in h[:METER_LOG]], log=[int(v) for v in h[METER_LOG:base]],
                    history=[int(v) for v in h[base:base + kept * METER_NRUN]])

    def load_state_dict(self, sd):
        if (int(sd["log_capacity"]), int(sd["history_capacity"])) != (self.log_capacity, self.history_capacity):
            raise ValueError(f"TrainMeter.load_state_dict: the file's meter has capacities ({sd['log_capacity']}, "
                             f"{sd['history_capacity']}), this one ({self.log_capacity}, {self.history_capacity})")
        head, log, hist = list(sd["head"]), list(sd["log"]), list(sd["history"])
        base = METER_LOG + 2 * self.log_capacity
        if len(head) != METER_LOG or len(log) != 2 * self.log_capacity or len(hist) % METER_NRUN or base + len(hist) > self.words:
            raise ValueError("TrainMeter.load_state_dict: the word lists do not fit this meter's block")
        h = np.zeros(self.words, dtype=np.int64)
        h[:base] = head + log
        h[base:base + len(hist)] = hist
        if self._block is None:
            self._loaded = h
        else:
            self._block.copy_(torch.from_numpy(h))


def _functional():
    import importlib
    return importlib.import_module(__package__ + ".functional")


# ---------------------------------------------------------------------------------------------------- the epoch loop
class EarlyStopper:
    """Stop when the validation accuracy has stopped rising (the rule of the reference's utils.EarlyStopper).  The best
    accuracy starts at 0.  `early_stop(acc)`: an accuracy above the best becomes the best and clears the count; any
    other accuracy below best + `min_delta` adds one to the count, and the call that brings the count to `patience`
    answers True.  (With `min_delta` 0 an accuracy equal to the best does neither.)"""

    def __init__(self, patience=1, min_delta=0):
        self.patience, self.min_delta = patience, min_delta
        self.counter, self.max_validation_acc = 0, 0.0

    def early_stop(self, validation_acc):
        if validation_acc > self.max_validation_acc:
            self.max_validation_acc, self.counter = validation_acc, 0
            return False
        if validation_acc < self.max_validation_acc + self.min_delta:
            self.counter += 1
            return self.counter >= self.patience
        return False


class EpochBook:
    """The bookkeeping of run_epochs (utils.py:242-290) without a model or a GPU: the four per-epoch lists, the best
    validation loss and accuracy, which checkpoint files an epoch writes and whether the run stops.

    `record(epoch, train_loss, train_acc, val_loss, val_acc)` appends to the lists and returns `(suffixes, stop)`:
    "best_loss" on a validation loss strictly below the best so far (9999 at the start), "best_acc" on a validation
    accuracy strictly above the best so far (0.0 at the start), and str(epoch) when `epoch > 0 and epoch % save_interval
    == 0`, in that order; `stop` is the early stopper's answer to the validation accuracy (False without one).
    `EpochBook.resumed(lists, ...)` is the book of a run that goes on from a checkpoint's lists: the best values are the
    lists' min / max, or 99999 / 0.0 when they are empty (utils.py:246-250)."""

    def __init__(self, save_interval=100, early_stopper=None):
        if isinstance(save_interval, bool) or not isinstance(save_interval, numbers.Integral) or save_interval < 1:
            raise ValueError(f"save_interval must be a positive integer, got {save_interval!r}")
        self.save_interval, self.early_stopper = int(save_interval), early_stopper
        self.train_loss_list, self.val_loss_list, self.train_acc_list, self.val_acc_list = [], [], [], []
        self.best_val_loss, self.best_val_acc = 9999, 0.0

    @classmethod
    def resumed(cls, lists, save_interval=100, early_stopper=None):
        """`lists`: [train_loss, val_loss, train_acc, val_acc], the order checkpoint.load_checkpoint returns"""
        book = cls(save_interval, early_stopper)
        book.train_loss_list, book.val_loss_list, book.train_acc_list, book.val_acc_list = (list(v) for v in lists)
        book.best_val_acc = 0.0 if len(book.val_acc_list) < 1 else max(book.val_acc_list)
        book.best_val_loss = 99999 if len(book.val_acc_list) < 1 else min(book.val_loss_list)
        return book

    @property
    def lists(self):
        return [self.train_loss_list, self.val_loss_list, self.train_acc_list, self.val_acc_list]

    def record(self, epoch, train_loss, train_acc, val_loss, val_acc):
        self.train_loss_list.append(train_loss)
        self.train_acc_list.append(train_acc)
        self.val_loss_list.append(val_loss)
        self.val_acc_list.append(val_acc)
        suffixes = []
        if val_loss < self.best_val_loss:
            self.best_val_loss = val_loss
            suffixes.append("best_loss")
        if val_acc > self.best_val_acc:
            self.best_val_acc = val_acc
            suffixes.append("best_acc")
        if epoch > 0 and epoch % self.save_interval == 0:
            suffixes.append(str(epoch))
        stop = bool(self.early_stopper is not None and self.early_stopper.early_stop(val_acc))
        return suffixes, stop


class _NoSchedule:
    """stands in for `scheduler=None`: nothing to step, nothing to save"""

    def step(self):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


class EpochLoop:
    """The reference's run_epochs (utils.py:240-290) on this package's pieces: per epoch one pass over the train batches
    through a train step with a `TrainMeter` (nothing is read back per batch), `scheduler.step()`, one pass over the
    validation batches through an `evaluate.Evaluator`, the four lists, the checkpoints and the early stop.

        loop = train.EpochLoop(model, opt, sched, batch_size=64, example=(x0, y0), num_classes=C, out_prefix="out/run1")
        loop.run(train_batches, val_batches, epochs=100)

    `example`: one (x, y) batch of `batch_size` rows; it fixes the shapes the step and the evaluator are built for.
    `graph=True`: the train step is a `GraphedTrainStep(ragged=True, meter=...)`, the evaluator replays a graph as well;
    `graph=False`: `TrainStep(pad_to=batch_size, meter=...)` and an eager evaluator.  Both are built at the first batch.
    Models whose train forward couples the clips of a batch (`clips_independent_in_train` False: ST-GCN, DecoupledGCN)
    cannot be padded: for them the loop builds the unpadded step and raises a ValueError at the first train batch that has
    not `batch_size` rows (drop the last batch: `drop_last=True`); nothing falls back to another path.
    `k`: the validation accuracy is top-k.  `out_prefix`: the reference's cfg.save_model_path -- files
    `{out_prefix}_best_loss.pt`, `_best_acc.pt`, `_{epoch}.pt` through checkpoint.save_checkpoint; None writes nothing.
    `lr`: the value recorded under 'learning_rate' (the reference's cfg.lr); default: the first param group's lr now.
    `eval_averaged=True` evaluates on the optimizer's averaged weights (`optimizer.averager.applied()`).
    `meter`: a `TrainMeter` of the caller's (say, one with a step log); `evaluator`: anything with reset() / update(x, y) /
    result() -> {"loss", "acc": {k: ...}} in the Evaluator's place.  `mixer`: a `BatchMixer` handed to the train step (which
    then uses a `MixedCrossEntropyLoss`); its state goes into the checkpoints.  `distiller`: a `Distiller` handed to the
    train step (which then uses a `DistilledCrossEntropyLoss`); alpha and the temperature go into the checkpoints, the
    teacher's weights do not.  Validation is untouched.

    `run(train_batches, val_batches, epochs, start_epoch=None)`: two re-iterable sources of (x, y) batches, on the CPU
    (copied with non_blocking=True; pinning is the loader's business, see collate.PinnedBatcher) or on the device.
    `epochs` has the reference's meaning: the loop runs `range(start_epoch, epochs + 1)`, so a fresh run with epochs=2
    trains three epochs.  `start_epoch=None` goes on where `resume()` (or nothing: 0) left it.

    Train numbers are the meter's: loss = sum of the step losses / steps with a finite loss, acc = correct / real rows.
    Validation loss is the sum of batch means / batches, as utils.py:131,142.

    `resume(path)` loads a checkpoint of this loop (checkpoint.load_checkpoint): weights, optimizer, scheduler, the four
    lists, `start_epoch = epoch + 1`, best values from the lists; and from the file's 'extra' key the guard's, the
    averager's, the meter's, the mixer's and the distiller's state, the model's dropout counter and its input modality
    (which must be the model's current one: `resume` refuses another), so dropout masks and the mixer's draws go on where
    they stopped.  Torch's
    device generator state is NOT carried: it draws HWGATE's train-mode window thresholds (HWGATE.py:96), so a resumed
    HWGATE run draws other thresholds than the uninterrupted one would have."""

    def __init__(self, model, optimizer, scheduler, batch_size, example, num_classes, smooth_factor=0.01, k=1, graph=True,
                 micro_batch=None, out_prefix=None, save_interval=100, early_stopper=None, lr=None, eval_averaged=False,
                 meter=None, evaluator=None, mixer=None, distiller=None):
        if distiller is not None:
            _check_distiller(distiller, None, model, None, "EpochLoop(distiller=...)")
        if isinstance(batch_size, bool) or not isinstance(batch_size, numbers.Integral) or batch_size < 1:
            raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
        x, y = example
        if x.shape[0] != batch_size or y.shape != (batch_size,):
            raise ValueError(f"the example batch must have batch_size = {batch_size} rows, got {tuple(x.shape)} with "
                             f"targets {tuple(y.shape)}")
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
            raise ValueError(f"k must be a positive integer, got {k!r}")
        if eval_averaged and getattr(optimizer, "averager", None) is None:
            raise ValueError("eval_averaged needs an optimizer that carries an optim.WeightAverage (optimizer.averager)")
        meter = TrainMeter() if meter is None else meter
        if meter.history_capacity < 1:
            raise ValueError("the loop reads each epoch from the meter's history: history_capacity must be at least 1")
        self.model, self.opt, self.scheduler = model, optimizer, scheduler if scheduler is not None else _NoSchedule()
        self.batch_size, self.example, self.num_classes = int(batch_size), (x, y), int(num_classes)
        self.smooth_factor, self.k, self.graph = float(smooth_factor), int(k), bool(graph)
        self.micro_batch = _check_micro_batch(micro_batch)
        self.out_prefix, self.eval_averaged = out_prefix, bool(eval_averaged)
        self.lr = _plain_lr(optimizer.param_groups[0]["lr"]) if lr is None else lr
        self.meter, self.evaluator, self.step, self.mixer = meter, evaluator, None, mixer
        self.distiller = distiller
        self.book = EpochBook(save_interval, early_stopper)
        self.start_epoch = 0
        self.padded = bool(getattr(model, "clips_independent_in_train", False))
        self.written = []            # the files of the latest run(), in the order they were written

    # ---- the pieces, built at the first batch (on the device the model lives on)
    def _device(self):
        return next(self.model.parameters()).device

    def _on_device(self, x, y):
        dev = self._device()
        if x.device != dev:
            x = x.to(dev, non_blocking=True)
        if y.device != dev:
            y = y.to(dev, non_blocking=True)
        return x, y

    def _build_step(self):
        x, y = self._on_device(*self.example)
        self.model.train()
        if self.distiller is not None:
            crit = DistilledCrossEntropyLoss(self.smooth_factor)
        elif self.mixer is not None:
            crit = MixedCrossEntropyLoss(self.smooth_factor)
        elif self.padded:
            crit = BatchSlicedCrossEntropyLoss(self.smooth_factor)
        else:
            crit = FusedSmoothedCrossEntropyLoss(self.smooth_factor)
        extra = {} if self.mixer is None else dict(mixer=self.mixer)      # without one the calls are what they were
        if self.distiller is not None:
            extra["distiller"] = self.distiller
        if self.graph:
            self.step = GraphedTrainStep(self.model, self.opt, x, y, criterion=crit, micro_batch=self.micro_batch,
                                         ragged=self.padded, meter=self.meter, **extra)
        else:
            self.step = TrainStep(self.model, self.opt, criterion=crit, micro_batch=self.micro_batch,
                                  pad_to=self.batch_size if self.padded else None, meter=self.meter, **extra)

    def _build_evaluator(self):
        import importlib
        evaluate = importlib.import_module(__package__ + ".evaluate")
        x, _ = self._on_device(*self.example)
        self.model.eval()
        self.evaluator = evaluate.Evaluator(self.model, self.num_classes, x, k_max=self.k, smooth_factor=self.smooth_factor,
                                            graph=self.graph)

    # ---- one epoch's two halves
    def train_epoch(self, train_batches):
        """one pass over the train batches and the meter's close; reads nothing back"""
        self.model.train()
        for x, y in train_batches:
            if not self.padded and x.shape[0] != self.batch_size:
                raise ValueError(f"{type(self.model).__name__} couples the clips of a train batch, so a batch cannot be "
                                 f"padded: every train batch must have batch_size = {self.batch_size} rows, got "
                                 f"{x.shape[0]} -- build the loader with drop_last=True")
            if self.step is None:
                self._build_step()
            self.step(*self._on_device(x, y))
        if self.step is None:
            raise ValueError("the train source gave no batch")
        self.meter.close_epoch()

    def validate(self, val_batches):
        """(val_loss, val_acc): one pass through the evaluator, one host read"""
        if self.evaluator is None:
            self._build_evaluator()
        self.model.eval()
        self.evaluator.reset()
        averaged = self.opt.averager.applied() if self.eval_averaged else contextlib.nullcontext()
        with averaged:
            for x, y in val_batches:
                self.evaluator.update(*self._on_device(x, y))
            r = self.evaluator.result()
        return r["loss"], r["acc"][self.k]

    # ---- checkpoints
    def _extra(self):
        guard, averager = _guard_of(self.opt), getattr(self.opt, "averager", None)
        extra = dict(guard=None if guard is None else guard.state_dict(),
                     averager=None if averager is None else averager.state_dict(),
                     meter=self.meter.state_dict(), drop_calls=int(getattr(self.model, "_drop_calls", 0)))
        if self.mixer is not None:
            extra["mixer"] = self.mixer.state_dict()
        if self.distiller is not None:
            extra["distiller"] = self.distiller.state_dict()
        modality = getattr(self.model, "input_modality", None)
        if modality is not None:                                   # without one the entry is absent, as it always was
            extra["modality"] = modality.state()
        return extra

    def _save(self, suffix, epoch):
        import importlib
        checkpoint = importlib.import_module(__package__ + ".checkpoint")
        path = f"{self.out_prefix}_{suffix}.pt"
        b = self.book
        checkpoint.save_checkpoint(path, self.model, self.opt, self.scheduler, b.train_acc_list, b.train_loss_list,
                                   b.val_acc_list, b.val_loss_list, epoch, self.lr, extra=self._extra())
        self.written.append(path)

    def resume(self, path):
        """go on from a checkpoint this loop wrote; returns the epoch the next run() starts at"""
        import importlib
        checkpoint = importlib.import_module(__package__ + ".checkpoint")
        dev = self._device()
        extra = checkpoint.read_extra(path, device=dev)
        modality = getattr(self.model, "input_modality", None)
        have, want = extra.get("modality"), None if modality is None else modality.state()
        if have != want:                                          # before anything is loaded: a refusal changes nothing
            raise ValueError(f"{path} was trained on the input modality {have}, the model reads {want}: set the model's "
                             "input_modality to the checkpoint's (modality.Modality.from_state) before resuming")
        _, _, _, lists, start = checkpoint.load_checkpoint(path, self.model, self.opt, self.scheduler, device=dev)
        guard, averager = _guard_of(self.opt), getattr(self.opt, "averager", None)
        if guard is not None and extra.get("guard") is not None:
            guard.load_state_dict(extra["guard"])
        if averager is not None and extra.get("averager") is not None:
            averager.load_state_dict(extra["averager"])
        if extra.get("meter") is not None:
            self.meter.load_state_dict(extra["meter"])
        if self.mixer is not None and extra.get("mixer") is not None:
            self.mixer.load_state_dict(extra["mixer"])
        if self.distiller is not None and extra.get("distiller") is not None:
            self.distiller.load_state_dict(extra["distiller"])
        if "drop_calls" in extra and hasattr(self.model, "_drop_calls"):
            self.model._drop_calls = int(extra["drop_calls"])
            if self.model._seed_state.is_cuda:           # the device counter a captured step advances by itself
                _functional().seed_set(self.model._seed_state, self.model._drop_calls, torch.initial_seed(),
                                       getattr(self.model, "rank_salt", 0))
        self.book = EpochBook.resumed(lists, self.book.save_interval, self.book.early_stopper)
        self.start_epoch = int(start)
        return self.start_epoch

    # ---- the loop
    def run(self, train_batches, val_batches, epochs, start_epoch=None):
        """epochs `start_epoch` .. `epochs`, both included (the reference's range(start_epoch, epochs + 1)); returns the
        book.  Ends early when the early stopper says so"""
        start = self.start_epoch if start_epoch is None else int(start_epoch)
        self.written = []
        for epoch in range(start, int(epochs) + 1):
            self.train_epoch(train_batches)
            self.scheduler.step()
            val_loss, val_acc = self.validate(val_batches)
            tr = self.meter.history()[-1]
            suffixes, stop = self.book.record(epoch, tr["loss"], tr["acc"], val_loss, val_acc)
            if self.out_prefix is not None:
                for suffix in suffixes:
                    self._save(suffix, epoch)
            self.start_epoch = epoch + 1
            if stop:
                break
        return self.book


def _plain_lr(v):
    return float(v.item()) if torch.is_tensor(v) else v
