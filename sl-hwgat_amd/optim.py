"""The reference's optimizer types on HIP kernels (reference: hwgat/utils.py:73-84 builds `Class(model.parameters(),
lr=cfg.lr)` for cfg.optimizer_type 'adamw' / 'adam' / 'nadam' / 'sgd', utils.py:93-116 steps it): DeviceAdamW (AdamW and
Adam), DeviceSGD and DeviceNAdam, all on csrc/optim.hip.  One launch updates every parameter tensor of the model from a
table of one record type in device memory, and every hyper-parameter is a device word the kernels read when they run, so
`train.GraphedTrainStep` captures any of these optimizers' step inside its graph: a replay is the whole train step, under
any torch LR scheduler.

The state is torch's: `param_groups` carry the keys of the torch class, `state[p]` is what that class keeps ({"step": 0-d
fp32 device tensor, "exp_avg", "exp_avg_sq"} for AdamW, the same plus "mu_product" for NAdam, {"momentum_buffer"} for SGD
with momentum, nothing for SGD without), and those ARE the tensors the kernels read and write (a caller may seat them
itself before the first step, e.g. as views of one flat arena), so `state_dict()` interchanges with the torch class (and
the reference's) in both directions and `checkpoint.save_checkpoint` / `load_checkpoint` work unchanged.  There is no CPU
fallback: the objects can be built, inspected and (de)serialised on CPU tensors, `step()` on them raises.

`GradGuard` (csrc/grad_guard.hip) is what a step inside a graph has no other place for: clipping by the global gradient
norm, as torch.nn.utils.clip_grad_norm_ does it, and a verdict on NaN / Inf gradients, both computed and kept on the
device.  Attached to a device optimizer (`opt.guard = GradGuard(max_norm=1.0, on_nonfinite="skip")`) it runs between the
backward and the update in every `step()` and in every replay; `clip_grad_norm_(parameters, guard)` runs it alone.

`WeightAverage` (csrc/weight_avg.hip) keeps an EMA or the equal-weight mean (SWA) of a model's weights in shadow tensors
on the device.  Attached to a device optimizer (`opt.averager = WeightAverage(model, decay=0.999)`) it is updated behind
the optimizer's own launches in every `step()` and in every replay, a step the guard skipped not counted;
`with avg.applied(): ...` exchanges averages and weights in place, so every captured graph stays valid.
"""
import contextlib
import ctypes
import math
import struct

import torch

from ._lib import call, ptr, stream

CHUNK = 4096            # HWGAT_OPTIM_CHUNK: elements per workgroup of a step kernel
NHYPER = 8              # HWGAT_OPTIM_NHYPER: fp64 words per group
NDERIVED = 16           # HWGAT_OPT_NDERIVED: fp32 words per table entry
# hwgat_opt_entry: p, g, s0, s1, w0, w1 (pointers), n (int64), group, first_block (int32)
ENTRY = struct.Struct("<6QqIi")
ENTRY_BYTES = ENTRY.size
KIND_ADAMW, KIND_SGD, KIND_NADAM = range(3)     # HWGAT_OPT_ADAMW / _SGD / _NADAM


GUARD_NSTATE = 16       # HWGAT_GGUARD_NSTATE: fp64 words of a guard's state block, at the HWGAT_GGUARD_* slots:
G_MAX_NORM, G_NORM_TYPE, G_MODE, G_TOTAL_NORM, G_CLIP_COEF, G_NONFINITE, G_SKIP, G_STEPS, G_CLIPPED, G_SKIPPED = range(10)
_COUNTERS = ("steps", "clipped", "skipped")

WAVG_NSTATE = 16        # HWGAT_WAVG_NSTATE: fp64 words of an averager's state block, at the HWGAT_WAVG_* slots:
W_MODE, W_DECAY, W_WARMUP, W_START, W_EVERY, W_STEPS_SEEN, W_N_AVERAGED, W_COEF, W_ACTIVE = range(9)
# hwgat_wavg_entry: avg, src (pointers), n (int64), first_block, pad (int32)
WAVG_ENTRY = struct.Struct("<QQqii")
WAVG_ENTRY_BYTES = WAVG_ENTRY.size
_WAVG_COUNTERS = ("steps_seen", "n_averaged")


def build_table(records, chunk=CHUNK):
    """records: (p, g, s0, s1, w0, w1 addresses -- 0 for an unused one --, n, group) per tensor that has a gradient, n > 0.
    Returns (the packed hwgat_opt_entry array as bytes, [first_block per entry], total_blocks): entry i owns
    ceil(n_i / chunk) workgroups from first_block_i on."""
    blob, first, total = bytearray(), [], 0
    for rec in records:
        n = rec[-2]
        if n <= 0:
            raise ValueError("an empty tensor has no table entry")
        first.append(total)
        blob += ENTRY.pack(*rec, total)
        total += (n + chunk - 1) // chunk
    if total >= 2 ** 31:
        raise ValueError("more workgroups than one launch holds")
    return bytes(blob), first, total


class _Table:
    """one device table + its derived block; `records` is what the device holds (or, while `pending`, will hold).
    `guard_ws`: a gradient guard's workspace for this table, two fp64 words per workgroup"""

    def __init__(self, capacity, device, nderived=NDERIVED):
        self.capacity = capacity
        self.buf = torch.zeros(max(1, capacity) * ENTRY_BYTES, dtype=torch.uint8, device=device)
        self.derived = torch.zeros(max(1, capacity) * nderived, dtype=torch.float32, device=device)
        self.records, self.n, self.total, self.pending = None, 0, 0, None
        self.guard_ws = None

    def reserve_guard_ws(self, blocks):
        if self.guard_ws is None or self.guard_ws.numel() < 2 * blocks:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("a gradient guard's workspace would be allocated inside a capture: begin_capture() first")
            self.guard_ws = torch.empty(2 * max(1, blocks), dtype=torch.float64, device=self.buf.device)

    def upload(self, blob):
        self.buf[:len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
        self.pending = None


class GradGuard:
    """Clip gradients by their global norm and detect non-finite ones, on the device (csrc/grad_guard.hip).

    `max_norm`: torch.nn.utils.clip_grad_norm_'s; every gradient is multiplied in place by
    min(1, max_norm / (total_norm + 1e-6)).  inf (the default) measures only: the coefficient is 1.
    `norm_type`: 2 or inf.
    `on_nonfinite`: "propagate" is torch's behaviour -- a NaN norm gives a NaN coefficient, NaN gradients and, after the
    step, NaN weights; "skip" turns a step whose gradients hold a NaN or an Inf into a no-op: the gradients are left
    unscaled (so they can be inspected) and a guarded optimizer writes no parameter, no state and no step count.
    All three are plain attributes and may be changed at any time; the new values reach the device, and so a captured
    graph, with the next `push()` (which `DeviceOptimizer.push_hyper()` and so every step and replay issues).

    Results stay on the device, in one fp64 block that every run rewrites: `total_norm`, `clip_coef` and `nonfinite` are
    0-d float64 views of it (reading one is the caller's host sync, at the time of its choosing), `counters()` reads
    {steps, clipped, skipped} in one copy.  The sum of squares is accumulated in fp64 in a fixed order: the norm depends on
    the gradients' values and sizes alone, not on their alignment, and repeats bit for bit."""

    _MODES = ("propagate", "skip")

    def __init__(self, max_norm=float("inf"), norm_type=2.0, on_nonfinite="propagate"):
        self.max_norm, self.norm_type, self.on_nonfinite = max_norm, norm_type, on_nonfinite
        self._config()
        self._state = None           # device block, GUARD_NSTATE fp64
        self._held = None            # the config the device holds
        self._loaded = None          # counters of a load_state_dict() that came before the device block existed
        self._clip = (None, None)    # clip_grad_norm_'s own table and the addresses it was built from

    def _config(self):
        """(max_norm, norm_type, skip) as the `set` entry point takes them; refuses what the kernels do not do"""
        max_norm, norm_type = float(self.max_norm), float(self.norm_type)
        if not max_norm >= 0.0:
            raise ValueError(f"GradGuard: max_norm must be >= 0, got {self.max_norm}")
        if norm_type != 2.0 and norm_type != math.inf:
            raise ValueError(f"GradGuard: norm_type 2 or inf, got {self.norm_type}")
        if self.on_nonfinite not in self._MODES:
            raise ValueError(f"GradGuard: on_nonfinite {self.on_nonfinite!r}: one of {list(self._MODES)}")
        return max_norm, norm_type, int(self.on_nonfinite == "skip")

    # ---- device side
    def bind(self, device):
        """allocate the state block on `device` (once; a guard serves one device)"""
        device = torch.device(device)
        if self._state is None:
            if device.type != "cuda":
                raise RuntimeError("GradGuard needs an MI355X device; there is no CPU fallback")
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradGuard: run it once (or bind() and push()) before capturing")
            self._state = torch.zeros(GUARD_NSTATE, dtype=torch.float64, device=device)
            if self._loaded is not None:
                self._put_counters(self._loaded)
                self._loaded = None
        elif self._state.device != device:
            raise ValueError(f"GradGuard lives on {self._state.device}, the gradients on {device}")
        return self

    def push(self, device=None):
        """make the device hold the current config: one `set` launch when it changed"""
        if device is not None:
            self.bind(device)
        cfg = self._config()
        if cfg != self._held:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GradGuard: the config changed inside a capture; push() before it")
            call("hwgat_gguard_set", ptr(self._bound()), *cfg, stream())
            self._held = cfg

    def _bound(self):
        if self._state is None:
            raise RuntimeError("GradGuard has not run yet: its results live on the device of its first step (or bind())")
        return self._state

    def _measure_and_scale(self, table):
        """partial, finish, scale over `table` (a filled _Table with its workspace reserved)"""
        st, s = ptr(self._state), stream()
        call("hwgat_gguard_partial", ptr(table.buf), table.n, st, ptr(table.guard_ws), table.total, s)
        call("hwgat_gguard_finish", ptr(table.guard_ws), table.total, st, s)
        call("hwgat_gguard_scale", ptr(table.buf), table.n, st, table.total, s)

    # ---- readouts
    @property
    def total_norm(self):
        return self._bound()[G_TOTAL_NORM]

    @property
    def clip_coef(self):
        return self._bound()[G_CLIP_COEF]

    @property
    def nonfinite(self):
        return self._bound()[G_NONFINITE]

    def counters(self):
        """{steps, clipped, skipped} so far: one host read"""
        if self._state is None:
            return dict(self._loaded or dict.fromkeys(_COUNTERS, 0))
        return {k: int(v) for k, v in zip(_COUNTERS, self._state[G_STEPS:G_SKIPPED + 1].tolist())}

    def _put_counters(self, values):
        self._state[G_STEPS:G_SKIPPED + 1].copy_(torch.tensor([float(values[k]) for k in _COUNTERS], dtype=torch.float64))

    # ---- what a warm-up must not leave behind: the results and the counters (the config is the caller's)
    def snapshot(self):
        return None if self._state is None else self._state[G_TOTAL_NORM:].clone()

    def restore(self, snap):
        if self._state is not None:
            if snap is None:
                self._state[G_TOTAL_NORM:].zero_()
            else:
                self._state[G_TOTAL_NORM:].copy_(snap)

    # ---- for a checkpoint's own extra key (the reference's nine keys stay as they are)
    def state_dict(self):
        return dict(max_norm=float(self.max_norm), norm_type=float(self.norm_type), on_nonfinite=self.on_nonfinite,
                    **self.counters())

    def load_state_dict(self, sd):
        keep = (self.max_norm, self.norm_type, self.on_nonfinite)
        self.max_norm, self.norm_type, self.on_nonfinite = sd["max_norm"], sd["norm_type"], sd["on_nonfinite"]
        try:
            self._config()
        except ValueError:
            self.max_norm, self.norm_type, self.on_nonfinite = keep
            raise
        values = {k: int(sd.get(k, 0)) for k in _COUNTERS}
        if self._state is None:
            self._loaded = values
        else:
            self._put_counters(values)


@torch.no_grad()
def clip_grad_norm_(parameters, guard):
    """torch.nn.utils.clip_grad_norm_(parameters, guard.max_norm, guard.norm_type) on the guard's three launches, for the
    gradients of an optimizer that is not a DeviceOptimizer (a torch optimizer stepped after a GraphedTrainStep replay --
    e.g. from its `register_step_pre_hook` --, an eager loop).  Returns `guard.total_norm`, a 0-d float64 device tensor:
    nothing is read back.  The gradients must be contiguous float32 tensors on one device; in "skip" mode the caller
    decides what a set `guard.nonfinite` means for its own optimizer."""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None and p.grad.numel() > 0]
    if not grads:
        raise ValueError("clip_grad_norm_: no gradients")
    for g in grads:
        if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous():
            raise ValueError("clip_grad_norm_ needs contiguous float32 gradients")
        if not g.is_cuda:
            raise RuntimeError("clip_grad_norm_ needs gradients on an MI355X device; there is no CPU fallback")
        if g.device != grads[0].device:
            raise ValueError("clip_grad_norm_ needs all gradients on one device")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("clip_grad_norm_ is an eager call; inside a capture attach the guard to a DeviceOptimizer")
    guard.push(grads[0].device)
    key = tuple((g.data_ptr(), g.numel()) for g in grads)
    table, held = guard._clip
    if key != held:
        if table is None or table.capacity < len(grads):
            table = _Table(len(grads), grads[0].device, nderived=0)
        blob, _, table.total = build_table([(0, a, 0, 0, 0, 0, n, 0) for a, n in key])
        table.n = len(grads)
        table.upload(blob)
        table.reserve_guard_ws(table.total)
        guard._clip = (table, key)
    guard._measure_and_scale(table)
    return guard.total_norm


class WeightAverage:
    """An exponential moving average (EMA) or the equal-weight running mean (SWA) of a model's weights, kept and updated
    on the device (csrc/weight_avg.hip), as torch.optim.swa_utils.AveragedModel keeps it -- without a second model: the
    averages live in fp32 shadow tensors beside the weights, and `swap()` / `applied()` exchange the two IN PLACE, so no
    address changes and every captured graph (train.GraphedTrainStep, serve.GraphedEval, evaluate.Evaluator) stays valid and
    simply sees the averaged weights while they are swapped in.

    `mode`: "ema" -- avg += (1 - decay) (p - avg), torch's get_ema_multi_avg_fn(decay) -- or "swa" -- the equal-weight
    mean, avg += (p - avg) / (n_averaged + 1), AveragedModel's default.  The first update copies the weights in both.
    `warmup`: EMA with the decay min(decay, (1 + n_averaged) / (10 + n_averaged)), so that early averages are not
    dominated by the initial weights.
    `start`, `every`: the update is due at the steps s (counted from 1, skipped steps not counted) with s > start and
    (s - start) % every == 0.
    `buffers`: also average `running_mean` / `running_var` of every BatchNorm module.  No other buffer (adjacency, masks,
    seeds, `num_batches_tracked`) is ever held.
    All five config values are plain attributes and may be changed at any time; they reach the device, and so a captured
    graph, with the next `push()` (which `DeviceOptimizer.push_hyper()` and so every step and replay issues).

    Attached to a device optimizer (`opt.averager = WeightAverage(model)`) the average is updated by two launches behind
    the optimizer's own in every `step()` and, as two more nodes of the graph, in every GraphedTrainStep replay; under a
    `GradGuard` in "skip" mode a skipped step is not averaged in and not counted -- the verdict is a device word, the host
    never learns it.  With any other optimizer call `update()` after its step.  `n_averaged`, `steps_seen` and `coef` are
    0-d float64 device views (reading one is the caller's host sync).  One table serves eager steps and every capture: it
    holds weight and shadow addresses only, no gradient's.

    While the averages are swapped in (`is_applied`), `update()`, `DeviceOptimizer.step()` and a GraphedTrainStep call
    raise: a step would train the averages.  Data-parallel runs need nothing extra: the ranks hold equal weights after
    every step, so they hold equal averages.  There is no CPU fallback: the object can be built, inspected and
    (de)serialised on a CPU model; everything that launches raises there."""

    _MODES = ("ema", "swa")

    def __init__(self, model, mode="ema", decay=0.999, warmup=False, start=0, every=1, buffers=True):
        self.model = model
        self.mode, self.decay, self.warmup, self.start, self.every = mode, decay, warmup, start, every
        self.buffers = bool(buffers)
        self._config()
        # (state_dict key, owner, attribute): a model.to() replaces a buffer object, so the live tensor is looked up
        self._slots = [(name, p, None) for name, p in model.named_parameters() if p.is_floating_point()]
        if self.buffers:
            for mname, m in model.named_modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    for attr in ("running_mean", "running_var"):
                        if getattr(m, attr, None) is not None:
                            self._slots.append((f"{mname}.{attr}" if mname else attr, m, attr))
        keys = set(model.state_dict().keys())
        for key, t in zip(self.keys(), self._live()):
            if key not in keys:
                raise ValueError(f"WeightAverage: {key!r} is no key of the model's state_dict()")
            if t.dtype != torch.float32:
                raise ValueError(f"WeightAverage needs float32 weights, {key!r} is {t.dtype}")
        if not self._slots:
            raise ValueError("WeightAverage: the model has nothing to average")
        self._shadow = [t.detach().clone(memory_format=torch.contiguous_format) for t in self._live()]
        self._state = None           # device block, WAVG_NSTATE fp64
        self._table = None           # device table, one WAVG_ENTRY per non-empty tensor
        self._n = self._total = 0
        self._key = None             # the addresses the table was built from
        self._held = None            # the config the device holds
        self._loaded = None          # counters of a load_state_dict() that came before the device block existed
        self.is_applied = False

    def keys(self):
        """the state_dict keys of the averaged tensors, in table order"""
        return [s[0] for s in self._slots]

    def _live(self):
        return [(o if attr is None else getattr(o, attr)).detach() for _, o, attr in self._slots]

    def _config(self):
        """(mode, decay, warmup, start, every) as the `set` entry point takes them; refuses what the kernels do not do"""
        if self.mode not in self._MODES:
            raise ValueError(f"WeightAverage: mode {self.mode!r}: one of {list(self._MODES)}")
        decay = float(self.decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightAverage: decay must be in [0, 1), got {self.decay}")
        for name in ("start", "every"):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or int(v) < (1 if name == "every" else 0):
                raise ValueError(f"WeightAverage: {name} must be an integer >= {1 if name == 'every' else 0}, got {v!r}")
        return self._MODES.index(self.mode), decay, int(bool(self.warmup)), int(self.start), int(self.every)

    # ---- device side
    def bind(self, device=None):
        """allocate the state block and the table on the model's device and move the shadows there (once)"""
        if self._state is not None:
            if device is not None and torch.device(device) != self._state.device:
                raise ValueError(f"WeightAverage lives on {self._state.device}, not on {device}")
            return self
        live = self._live()
        if not all(t.is_cuda for t in live):
            raise RuntimeError("WeightAverage needs the model on an MI355X device; there is no CPU fallback")
        dev = live[0].device
        if any(t.device != dev for t in live) or (device is not None and torch.device(device) != dev):
            raise ValueError("WeightAverage needs all weights on one device, the optimizer's")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightAverage: bind() (or one eager update) before capturing")
        self._shadow = [s if s.device == dev else s.to(dev) for s in self._shadow]
        self._table = torch.zeros(len(self._slots) * WAVG_ENTRY_BYTES, dtype=torch.uint8, device=dev)
        self._state = torch.zeros(WAVG_NSTATE, dtype=torch.float64, device=dev)
        if self._loaded is not None:
            self._put_counters(self._loaded)
            self._loaded = None
        self._check_table(live)
        return self

    def _bound(self):
        if self._state is None:
            raise RuntimeError("WeightAverage has not run yet: its results live on the device of its first update (or bind())")
        return self._state

    def _check_table(self, live=None):
        """the table against the current addresses: a tuple compare, packed and uploaded (in place) only on change"""
        live = self._live() if live is None else live
        key = tuple(t.data_ptr() for t in live)
        if key == self._key:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightAverage: a weight was reallocated before a capture; run one eager update() first")
        blob, total, n = bytearray(), 0, 0
        for t, s in zip(live, self._shadow):
            if not t.is_contiguous() or t.shape != s.shape or t.device != s.device:
                raise ValueError("WeightAverage needs contiguous weights that keep their shape and device")
            if t.numel() == 0:
                continue
            blob += WAVG_ENTRY.pack(s.data_ptr(), t.data_ptr(), t.numel(), total, 0)
            total += (t.numel() + CHUNK - 1) // CHUNK
            n += 1
        if total >= 2 ** 31:
            raise ValueError("more workgroups than one launch holds")
        if blob:
            self._table[:len(blob)].copy_(torch.frombuffer(blob, dtype=torch.uint8))
        self._n, self._total, self._key = n, total, key

    def push(self, device=None):
        """make the device hold the current config: one `set` launch when it changed"""
        cfg = self._config()
        self.bind(device)
        if cfg != self._held:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("WeightAverage: the config changed inside a capture; push() before it")
            call("hwgat_wavg_set", ptr(self._state), *cfg, stream())
            self._held = cfg

    def _refuse_applied(self, what):
        if self.is_applied:
            raise RuntimeError(f"{what} while the averaged weights are swapped in (WeightAverage.is_applied): swap() back first")

    def _issue(self, guard=None):
        """advance and update on the current stream; `guard`: the GradGuard whose skip verdict decides whether the step counts"""
        self._check_table()
        if self._n:
            call("hwgat_wavg_advance", ptr(self._state), None if guard is None else ptr(guard._bound()), stream())
            call("hwgat_wavg_update", ptr(self._table), self._n, ptr(self._state), self._total, stream())

    @torch.no_grad()
    def update(self, guard=None):
        """take the current weights into the average: two launches on the current stream, capturable (bind() and push()
        before the capture).  For an optimizer that is not a DeviceOptimizer, or a loop written by hand"""
        self._refuse_applied("WeightAverage.update()")
        self.push()
        self._issue(guard)

    @torch.no_grad()
    def swap(self):
        """exchange the averaged and the live weights in place: one launch.  Every forward re-derives its weight images
        from the weights, so the next one, eager or replayed, runs on what is swapped in"""
        self.bind()
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightAverage.swap() is an eager call: the host has to know which weights are live")
        self._check_table()
        if self._n:
            call("hwgat_wavg_swap", ptr(self._table), self._n, self._total, stream())
        self.is_applied = not self.is_applied

    @contextlib.contextmanager
    def applied(self):
        """`with avg.applied(): ...`: the body runs on the averaged weights; they are swapped back out on any exit"""
        self._refuse_applied("WeightAverage.applied()")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ---- readouts
    @property
    def n_averaged(self):
        return self._bound()[W_N_AVERAGED]

    @property
    def steps_seen(self):
        return self._bound()[W_STEPS_SEEN]

    @property
    def coef(self):
        return self._bound()[W_COEF]

    def counters(self):
        """{steps_seen, n_averaged} so far: one host read"""
        if self._state is None:
            return dict(self._loaded or dict.fromkeys(_WAVG_COUNTERS, 0))
        return {k: int(v) for k, v in zip(_WAVG_COUNTERS, self._state[W_STEPS_SEEN:W_N_AVERAGED + 1].tolist())}

    def _put_counters(self, values):
        self._state[W_STEPS_SEEN:W_N_AVERAGED + 1].copy_(
            torch.tensor([float(values[k]) for k in _WAVG_COUNTERS], dtype=torch.float64))

    # ---- what a warm-up must not leave behind: the shadows and the result words (the config is the caller's)
    @torch.no_grad()
    def snapshot(self):
        return ([s.clone() for s in self._shadow], None if self._state is None else self._state[W_STEPS_SEEN:].clone())

    @torch.no_grad()
    def restore(self, snap):
        """None: an averager that was attached after the snapshot becomes a fresh one, its shadows the current weights"""
        shadows, words = (self._live(), None) if snap is None else snap
        for s, q in zip(self._shadow, shadows):
            s.copy_(q)
        if self._state is not None:
            if words is None:
                self._state[W_STEPS_SEEN:].zero_()
            else:
                self._state[W_STEPS_SEEN:].copy_(words)

    # ---- (de)serialisation
    @torch.no_grad()
    def model_state_dict(self):
        """the model's state_dict() -- its keys, its order -- with clones of the averaged values in place of the live
        ones: `torch.save({"model_state_dict": avg.model_state_dict()}, path)` is a weights file of the averaged model"""
        sd = self.model.state_dict()
        for key, s, t in zip(self.keys(), self._shadow, self._live()):
            sd[key] = (t if self.is_applied else s).detach().clone()
        return sd

    @torch.no_grad()
    def state_dict(self):
        """config, counters and the shadows by state_dict key; for a checkpoint's own extra key"""
        self._refuse_applied("WeightAverage.state_dict()")
        return dict(mode=self.mode, decay=float(self.decay), warmup=bool(self.warmup), start=int(self.start),
                    every=int(self.every), buffers=self.buffers, **self.counters(),
                    shadows={k: s.detach().clone() for k, s in zip(self.keys(), self._shadow)})

    @torch.no_grad()
    def load_state_dict(self, sd):
        """the loaded values go INTO the live shadow tensors and device words: no address changes"""
        self._refuse_applied("WeightAverage.load_state_dict()")
        names = ("mode", "decay", "warmup", "start", "every")
        shadows = sd["shadows"]
        if list(shadows.keys()) != self.keys():
            raise ValueError("WeightAverage.load_state_dict: the file averages other tensors than this object "
                             f"({len(shadows)} against {len(self._slots)}; `buffers` must match)")
        for (k, q), s in zip(shadows.items(), self._shadow):
            if tuple(q.shape) != tuple(s.shape):
                raise ValueError(f"WeightAverage.load_state_dict: {k!r} has shape {tuple(q.shape)}, expected {tuple(s.shape)}")
        keep = tuple(getattr(self, k) for k in names)
        for k in names:
            setattr(self, k, sd[k])
        try:
            self._config()
        except ValueError:
            for k, v in zip(names, keep):
                setattr(self, k, v)
            raise
        for q, s in zip(shadows.values(), self._shadow):
            s.copy_(q.to(dtype=torch.float32))
        values = {k: int(sd.get(k, 0)) for k in _WAVG_COUNTERS}
        if self._state is None:
            self._loaded = values
        else:
            self._put_counters(values)


class DeviceOptimizer(torch.optim.Optimizer):
    """What the device optimizers share: the fp32 / one-device checks, the fp64 hyper-parameter block with its host
    mirror (`push_hyper`), the device table keyed by the (parameter, gradient) addresses, `begin_capture` / `end_capture`,
    `load_state_dict` into the live tensors, and `snapshot_state` / `restore_state`.  A subclass names its `kind` of the
    three entry points (hwgat_opt_set / hwgat_opt_advance / hwgat_opt_step), says which tensors a parameter's state
    consists of and where they go in a table record, and turns a param group into the eight words of its hyper block.

    `step()`: pushes the param-group values that differ from what the device holds (one tiny `set` launch per changed
    group), revalidates the table against the current addresses -- a tuple compare; rebuilt and uploaded only on change --
    then issues `advance` and `step`.  A parameter whose grad is None is skipped and gets no state, as in torch.

    Capturing `step()` in a HIP graph: the gradients of a capture come from the graph's pool, so the table the graph's
    launches read is a new one.  `begin_capture()` (before the capture; allocates it) ... the capture, with `step()`
    inside ... `end_capture()` (after it; uploads the table -- capture executes nothing, so that is early enough -- and
    returns it: keep the returned object alive as long as the graph).  Hyper-parameters must be on the device before the
    capture (`push_hyper()`), and before each replay call `push_hyper()` again: it launches only when something changed.
    `train.GraphedTrainStep` does all of this.

    `guard`: a `GradGuard` or None (the default).  It is an attribute of the optimizer, not a param-group key and not part
    of `state[p]`: `state_dict()` is the torch class's with or without one.  With a guard, `step()` issues the guard's
    partial, finish and scale launches over the same table and hands `advance` and `step` the guard's state block, which
    then do nothing when the guard decided to skip; without one it issues exactly `advance` and `step`.

    `averager`: a `WeightAverage` or None (the default), an attribute like `guard` and as little a part of `state_dict()`.
    With one, `step()` issues the averager's `advance` and `update` launches after its own (handing them the guard's state
    block when there is a guard, so a skipped step is not averaged in), `push_hyper()` pushes its config, and
    `snapshot_state` / `restore_state` cover its shadows and result words; `step()` raises while the averaged weights are
    swapped in.  Without one the launches are exactly those above."""

    _KIND = None                         # the `kind` argument of the entry points
    _STATE_KEYS = ()                     # state[p], in torch's order
    _SCALAR_KEYS = ()                    # those of them that are one fp32 word
    _PRIVATE_KEYS = ()                   # per-tensor device words that are not part of state[p] / state_dict()
    _INITIAL = {}                        # fresh value of a key; 0 when absent
    _CAPTURABLE = True                   # the torch class has a `capturable` key
    _REFILL_ON_LOAD = True               # a load without state for a live parameter exposes its zeroed tensors again

    def __init__(self, params, defaults):
        self._dev = None
        self._live = {}              # parameter -> {key: tensor}: the tensors the device tables point at
        self._key = None             # what the eager table was built from
        self._table = None
        self._capture = None
        self._hyper = None           # device block, NHYPER fp64 per group
        self._held = []              # host mirror of it, one tuple per group
        self.guard = None            # a GradGuard, or None
        self.averager = None         # a WeightAverage, or None
        super().__init__(params, defaults)

    @property
    def _name(self):
        return type(self).__name__

    # ---- construction-time checks
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32:
                raise ValueError(f"{self._name} needs float32 parameters, got {p.dtype}")
        self._key = self._dev = None

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _device(self):
        if self._dev is not None:
            return self._dev
        ps = self._params()
        if not ps or not all(p.is_cuda for p in ps):
            raise RuntimeError(f"{self._name}.step needs its parameters on an MI355X device; there is no CPU fallback")
        if any(p.device != ps[0].device for p in ps):
            raise ValueError(f"{self._name} needs all parameters on one device")
        self._dev = ps[0].device                 # checked once per set of parameters
        return self._dev

    # ---- hyper-parameters
    @staticmethod
    def _hyper_words(vals):
        """the NHYPER doubles of a group's device block (the header's layout for this kind), from a `_group_values` tuple"""
        raise NotImplementedError

    @staticmethod
    def _decode_hyper(row):
        """a group's values as `device_hyper()` reports them, from its NHYPER words"""
        raise NotImplementedError

    def push_hyper(self):
        """make the device block hold what `param_groups` say: one `set` launch per group that changed; and the guard's
        and the averager's config, when there is one and it changed"""
        if self.guard is not None:
            self.guard.push(self._device())
        if self.averager is not None:
            self.averager.push(self._device())
        n = len(self.param_groups)
        if self._hyper is None or self._hyper.numel() < n * NHYPER:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._name}: take one eager step (or push_hyper()) before capturing")
            self._hyper = torch.zeros(n * NHYPER, dtype=torch.float64, device=self._device())
            self._held = [None] * n
        for i, group in enumerate(self.param_groups):
            vals = self._group_values(group)
            if vals != self._held[i]:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(f"{self._name}: a hyper-parameter changed inside a capture; push_hyper() before it")
                words = (ctypes.c_double * NHYPER)(*self._hyper_words(vals))
                call("hwgat_opt_set", ptr(self._hyper), i, self._KIND, words, stream())
                self._held[i] = vals

    def device_hyper(self):
        """what the device block holds, read back: per group the values of `_decode_hyper`"""
        return [self._decode_hyper(r) for r in self._hyper.cpu().view(-1, NHYPER).tolist()[:len(self.param_groups)]]

    # ---- state and table
    def _wants_state(self, group):
        return True

    def _fresh(self, p, key):
        shape = () if key in self._SCALAR_KEYS or key in self._PRIVATE_KEYS else p.shape
        return torch.full(shape, self._INITIAL.get(key, 0.0), dtype=torch.float32, device=p.device)

    def _reset(self, live):
        for k, t in live.items():
            t.fill_(self._INITIAL.get(k, 0.0))

    def _state_of(self, p, create):
        st = self.state[p]
        if len(st) == 0:
            if not create:
                raise RuntimeError(f"{self._name}: a parameter would get its state inside a capture; warm up with one eager step")
            if p in self._live:                  # had state before (a load_state_dict without it): same tensors, fresh
                live = self._live[p]
                self._reset(live)
            else:
                live = {k: self._fresh(p, k) for k in self._STATE_KEYS + self._PRIVATE_KEYS}
                self._live[p] = live
            st.update((k, live[k]) for k in self._STATE_KEYS)
        elif p not in self._live:                # state seated by the caller (e.g. views of a flat arena): adopt it
            live = {k: st[k] for k in self._STATE_KEYS}
            for k, t in live.items():
                ok = t.dtype == torch.float32 and t.device == p.device
                ok = ok and (t.numel() == 1 if k in self._SCALAR_KEYS else t.shape == p.shape and t.is_contiguous())
                if not ok:
                    raise ValueError(f"{self._name}: state tensors must be float32 on the parameter's device, the arrays "
                                     "contiguous and of its shape, the scalars one element")
            live.update((k, self._fresh(p, k)) for k in self._PRIVATE_KEYS)
            self._live[p] = live
        return st

    def _record(self, p, g, live, gi):
        """one table record, (addresses ..., n, group); `live` is None for a tensor without state"""
        raise NotImplementedError

    def table_records(self, create=True):
        """the table record of every non-empty parameter that has a gradient, in group order; creates the state of a
        parameter the first time it has one"""
        recs = []
        for gi, group in enumerate(self.param_groups):
            wants = self._wants_state(group)
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if g.is_sparse:
                    raise ValueError(f"{self._name} does not support sparse gradients")
                if g.dtype != torch.float32 or not g.is_contiguous() or not p.is_contiguous() or g.shape != p.shape:
                    raise ValueError(f"{self._name} needs contiguous float32 parameters and gradients of one shape")
                if wants:
                    self._state_of(p, create)
                recs.append(self._record(p, g, self._live[p] if wants else None, gi))
        return recs

    def _address_key(self):
        return tuple((p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in self._params())

    def _fill(self, table, defer):
        recs = self.table_records(create=not defer)
        table.records = recs
        table.n = len(recs)
        if recs:
            blob, _, table.total = build_table(recs)
            if defer:
                table.pending = blob
            else:
                table.upload(blob)

    def begin_capture(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("begin_capture() goes before the capture")
        self._capture = _Table(len(self._params()), self._device())
        if self.guard is not None:           # as many partials as the table can have workgroups at the most
            self._capture.reserve_guard_ws(sum(-(-p.numel() // CHUNK) for p in self._params()))

    def end_capture(self):
        """upload the table the captured launches read; returns it (the graph's owner keeps it alive)"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("end_capture() goes after the capture")
        table, self._capture = self._capture, None
        if table is not None and table.pending is not None:
            table.upload(table.pending)
        return table

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._device()
        if self.averager is not None:
            self.averager._refuse_applied(f"{self._name}.step()")
        self.push_hyper()
        if torch.cuda.is_current_stream_capturing():
            table = self._capture
            if table is None:
                raise RuntimeError(f"{self._name}: begin_capture() before a capture that holds step()")
            if table.records is None:
                self._fill(table, defer=True)
            elif self.table_records(create=False) != table.records:   # a later step of the same capture: same tensors
                raise RuntimeError(f"{self._name}: the steps of one capture must see the same parameters and gradients")
        else:
            key = self._address_key()
            if self._table is None or self._table.capacity < len(self._params()):
                self._table, self._key = _Table(len(self._params()), dev), None
            table = self._table
            if key != self._key:
                self._fill(table, defer=False)
                self._key = key
        if table.n:
            gs = None
            if self.guard is not None:
                table.reserve_guard_ws(table.total)
                self.guard._measure_and_scale(table)
                gs = ptr(self.guard._state)
            call("hwgat_opt_advance", self._KIND, ptr(table.buf), table.n, ptr(self._hyper), ptr(table.derived), gs, stream())
            call("hwgat_opt_step", self._KIND, ptr(table.buf), table.n, ptr(table.derived), table.total, gs, stream())
        if table.n and self.averager is not None:            # after the update, and only of a step the guard let happen
            self.averager._issue(self.guard)
        return loss

    # ---- what a warm-up must not leave behind (train.GraphedTrainStep): every state tensor and private word
    @torch.no_grad()
    def snapshot_state(self):
        """clones of every tensor of `state` and of every private per-tensor word, for `restore_state`"""
        snap = {}
        for p, st in self.state.items():
            snap[p] = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
        for p, live in self._live.items():
            snap.setdefault(p, {}).update((k, live[k].clone()) for k in self._PRIVATE_KEYS)
        if self.guard is not None:
            snap[self.guard] = self.guard.snapshot()
        if self.averager is not None:
            snap[self.averager] = self.averager.snapshot()
        return snap

    @torch.no_grad()
    def restore_state(self, snap):
        """put back what `snapshot_state` saw, in place; a tensor that did not exist then becomes a fresh one (zero; 1 for
        NAdam's mu_product; "never stepped" for SGD's private word), so that state created since looks newly made"""
        def put(p, k, t):
            if p in snap and k in snap[p]:
                t.copy_(snap[p][k])
            else:
                t.fill_(self._INITIAL.get(k, 0.0))
        for p, st in self.state.items():
            for k, v in st.items():
                if torch.is_tensor(v):
                    put(p, k, v)
        for p, live in self._live.items():
            for k in self._PRIVATE_KEYS:
                put(p, k, live[k])
        if self.guard is not None:           # its results and counters; zero when it first ran after the snapshot
            self.guard.restore(snap.get(self.guard))
        if self.averager is not None:        # its shadows and result words; a fresh one when it came after the snapshot
            self.averager.restore(snap.get(self.averager))

    # ---- (de)serialisation: the loaded values go INTO the live tensors, whose addresses device tables (a captured
    # graph's among them) hold
    def _loaded(self, st):
        """{key: value} of the live tensors, from one parameter's loaded state; None when that state holds nothing a
        step would use"""
        return {k: (torch.as_tensor(st.get(k, self._INITIAL.get(k, 0.0)), dtype=torch.float32).reshape(())
                    if k in self._SCALAR_KEYS else st[k]) for k in self._STATE_KEYS}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._group_values(group)
            if self._CAPTURABLE:
                group["capturable"] = True
            for p in group["params"]:
                st, live = self.state.get(p), self._live.get(p)
                new = self._loaded(st) if st else None
                if new is None:
                    if st is not None:
                        del self.state[p]
                    if live is not None:         # the file has no state for it: fresh state in the same tensors
                        self._reset(live)
                        if self._REFILL_ON_LOAD:
                            self.state[p].update((k, live[k]) for k in self._STATE_KEYS)
                    continue
                if live is None:
                    live = {k: torch.as_tensor(t).detach().to(device=p.device, dtype=torch.float32).contiguous().clone()
                            for k, t in new.items()}
                    live.update((k, self._fresh(p, k)) for k in self._PRIVATE_KEYS if k not in new)
                    self._live[p] = live
                else:
                    for k, src in new.items():
                        dst = live[k]
                        dst.copy_(torch.as_tensor(src).to(device=dst.device, dtype=torch.float32).reshape(dst.shape))
                st.update((k, live[k]) for k in self._STATE_KEYS)
        self._key = None


class DeviceAdamW(DeviceOptimizer):
    """torch.optim.AdamW (decoupled_weight_decay=True) or Adam (False) with amsgrad = maximize = False on fp32
    parameters, the HWGAT_OPT_ADAMW kind of the entry points (csrc/optim.hip).  See DeviceOptimizer for `step()` and for
    capturing it in a HIP graph."""

    _KIND = KIND_ADAMW
    _STATE_KEYS = ("step", "exp_avg", "exp_avg_sq")
    _SCALAR_KEYS = ("step",)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True,
                 amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError("DeviceAdamW: amsgrad=True is not supported")
        if maximize:
            raise ValueError("DeviceAdamW: maximize=True is not supported")
        if not 0.0 <= float(lr):
            raise ValueError(f"invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"invalid epsilon: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"invalid weight_decay: {weight_decay}")
        # exactly the keys torch's own class writes into a state_dict, whatever the torch version
        like = torch.optim.AdamW if decoupled_weight_decay else torch.optim.Adam
        defaults = dict(like([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        capturable=True, decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)

    @staticmethod
    def _group_values(group):
        if group.get("amsgrad", False):
            raise ValueError("DeviceAdamW: amsgrad=True is not supported")
        if group.get("maximize", False):
            raise ValueError("DeviceAdamW: maximize=True is not supported")
        b1, b2 = group["betas"]
        return (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                bool(group.get("decoupled_weight_decay", True)))

    @staticmethod
    def _hyper_words(vals):
        """{lr, beta1, beta2, eps, weight_decay, coupled, 0, 0}"""
        return (*vals[:5], 0.0 if vals[5] else 1.0, 0.0, 0.0)

    @staticmethod
    def _decode_hyper(r):
        """{lr, betas, eps, weight_decay, decoupled_weight_decay}"""
        return dict(lr=r[0], betas=(r[1], r[2]), eps=r[3], weight_decay=r[4], decoupled_weight_decay=r[5] == 0.0)

    def _record(self, p, g, live, gi):
        """(p, g, m, v, step, 0 addresses, n, group)"""
        return (p.data_ptr(), g.data_ptr(), live["exp_avg"].data_ptr(), live["exp_avg_sq"].data_ptr(),
                live["step"].data_ptr(), 0, p.numel(), gi)


def _refuse_unsupported(name, group):
    if group.get("maximize", False):
        raise ValueError(f"{name}: maximize=True is not supported")
    if group.get("differentiable", False):
        raise ValueError(f"{name}: differentiable=True is not supported")


class DeviceSGD(DeviceOptimizer):
    """torch.optim.SGD with maximize = False on fp32 parameters, the HWGAT_OPT_SGD kind of the entry points
    (csrc/optim.hip).  `state[p]` is torch's: {"momentum_buffer"} in a group whose momentum is not 0, nothing
    otherwise.  Torch's SGD keeps no step count; that a tensor's FIRST buffer is the gradient itself (torch clones it,
    whatever the dampening) is decided on the device from a private per-tensor word, which is not part of `state_dict()`:
    a buffer the caller seats before the first step is storage and counts as never stepped, one that arrives through
    `load_state_dict` counts as stepped.  A group whose momentum moves between 0 and non-zero is given (or stops using)
    its buffers at the next eager `step()`; after a capture that is refused, because the captured table cannot change."""

    _KIND = KIND_SGD
    _STATE_KEYS = ("momentum_buffer",)
    _PRIVATE_KEYS = ("stepped",)
    _CAPTURABLE = False
    _REFILL_ON_LOAD = False              # no buffer in the file: torch would clone the next gradient, and so does this

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False,
                 differentiable=False):
        defaults = dict(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3).defaults)
        defaults.update(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                        maximize=bool(maximize), differentiable=bool(differentiable))
        self._group_values(defaults)
        self._captured_momentum = None   # per group, whether the last captured table has buffers
        super().__init__(params, defaults)

    @staticmethod
    def _group_values(group):
        _refuse_unsupported("DeviceSGD", group)
        lr, mom, damp, wd = (float(group[k]) for k in ("lr", "momentum", "dampening", "weight_decay"))
        if not 0.0 <= lr:
            raise ValueError(f"invalid learning rate: {lr}")
        if not 0.0 <= mom:
            raise ValueError(f"invalid momentum value: {mom}")
        if not 0.0 <= wd:
            raise ValueError(f"invalid weight_decay value: {wd}")
        if group["nesterov"] and (mom <= 0.0 or damp != 0.0):
            raise ValueError("nesterov momentum requires a momentum and zero dampening")
        return (lr, mom, damp, wd, bool(group["nesterov"]))

    @staticmethod
    def _hyper_words(vals):
        """{lr, momentum, dampening, weight_decay, nesterov, 0, 0, 0}"""
        return (*vals[:4], 1.0 if vals[4] else 0.0, 0.0, 0.0, 0.0)

    def push_hyper(self):
        if self._captured_momentum is not None:
            now = [float(g["momentum"]) != 0.0 for g in self.param_groups]
            if now != self._captured_momentum:
                raise ValueError("DeviceSGD: a group's momentum moved between 0 and non-zero after a capture, and the "
                                 "captured table has no momentum buffer for it (or one it must no longer use): capture again")
        super().push_hyper()

    def end_capture(self):
        table = super().end_capture()
        if table is not None and table.records is not None:
            self._captured_momentum = [float(g["momentum"]) != 0.0 for g in self.param_groups]
        return table

    @staticmethod
    def _decode_hyper(r):
        """{lr, momentum, dampening, weight_decay, nesterov}"""
        return dict(lr=r[0], momentum=r[1], dampening=r[2], weight_decay=r[3], nesterov=r[4] != 0.0)

    def _wants_state(self, group):
        return float(group["momentum"]) != 0.0

    def _record(self, p, g, live, gi):
        """(p, g, momentum buffer, 0, stepped word, 0 addresses, n, group); the buffer and the word 0 without momentum"""
        if live is None:
            return (p.data_ptr(), g.data_ptr(), 0, 0, 0, 0, p.numel(), gi)
        return (p.data_ptr(), g.data_ptr(), live["momentum_buffer"].data_ptr(), 0, live["stepped"].data_ptr(), 0,
                p.numel(), gi)

    def _address_key(self):
        return super()._address_key() + tuple(self._wants_state(g) for g in self.param_groups)

    def _loaded(self, st):
        if st.get("momentum_buffer") is None:
            return None
        return {"momentum_buffer": st["momentum_buffer"], "stepped": 1.0}


class DeviceNAdam(DeviceOptimizer):
    """torch.optim.NAdam (both values of decoupled_weight_decay) with maximize = False on fp32 parameters, the
    HWGAT_OPT_NADAM kind of the entry points (csrc/optim.hip).  `state[p]` is that of a capturable torch NAdam: {"step", "mu_product": 0-d fp32 device tensors, "exp_avg", "exp_avg_sq"}."""

    _KIND = KIND_NADAM
    _STATE_KEYS = ("step", "mu_product", "exp_avg", "exp_avg_sq")
    _SCALAR_KEYS = ("step", "mu_product")
    _INITIAL = {"mu_product": 1.0}

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum_decay=4e-3,
                 decoupled_weight_decay=False, maximize=False, differentiable=False):
        defaults = dict(torch.optim.NAdam([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, momentum_decay=momentum_decay,
                        decoupled_weight_decay=bool(decoupled_weight_decay), maximize=bool(maximize), capturable=True,
                        differentiable=bool(differentiable))
        self._group_values(defaults)
        super().__init__(params, defaults)

    @staticmethod
    def _group_values(group):
        _refuse_unsupported("DeviceNAdam", group)
        lr, eps, wd, md = (float(group[k]) for k in ("lr", "eps", "weight_decay", "momentum_decay"))
        b1, b2 = (float(b) for b in group["betas"])
        if not 0.0 <= lr:
            raise ValueError(f"invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"invalid epsilon: {eps}")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"invalid betas: {group['betas']}")
        if not 0.0 <= wd:
            raise ValueError(f"invalid weight_decay: {wd}")
        if not 0.0 <= md:
            raise ValueError(f"invalid momentum_decay: {md}")
        return (lr, b1, b2, eps, wd, md, bool(group.get("decoupled_weight_decay", False)))

    @staticmethod
    def _hyper_words(vals):
        """{lr, beta1, beta2, eps, weight_decay, coupled, momentum_decay, 0}"""
        return (*vals[:5], 0.0 if vals[6] else 1.0, vals[5], 0.0)

    @staticmethod
    def _decode_hyper(r):
        """{lr, betas, eps, weight_decay, momentum_decay, decoupled_weight_decay}"""
        return dict(lr=r[0], betas=(r[1], r[2]), eps=r[3], weight_decay=r[4], momentum_decay=r[6],
                    decoupled_weight_decay=r[5] == 0.0)

    def _record(self, p, g, live, gi):
        """(p, g, m, v, step, mu_product addresses, n, group)"""
        return (p.data_ptr(), g.data_ptr(), live["exp_avg"].data_ptr(), live["exp_avg_sq"].data_ptr(),
                live["step"].data_ptr(), live["mu_product"].data_ptr(), p.numel(), gi)
