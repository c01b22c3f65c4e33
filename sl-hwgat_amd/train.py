"""Loss and the fwd+bwd step harness of the hot path (reference hwgat/utils.py:93-116
and hwgat/losses/SmoothCrossEntropy.py), without the per-step host syncs."""
import numbers

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
        import importlib
        HF = importlib.import_module(__package__ + ".functional")
        loss, self.last_rank, self.last_pred = HF.smooth_ce(input, target, self.smooth_factor)
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
        import importlib
        HF = importlib.import_module(__package__ + ".functional")
        if self.n_rows is None:
            raise RuntimeError("BatchSlicedCrossEntropyLoss: place(n_rows, offset) first -- TrainStep(pad_to=...) and "
                               "GraphedTrainStep(ragged=True) do")
        loss, self.last_rank, self.last_pred, self._hits = HF.batch_sliced_ce(input, target, self.smooth_factor,
                                                                              self.n_rows, self.offset)
        return loss

    def correct(self):
        return self._hits


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


def _run_slices(model, criterion, x, y, mb, weighted=True, n_rows=None):
    """forward, loss and backward of x / y in slices of `mb` rows, gradients accumulating; (loss, correct) summed in slice
    order.  `weighted`: the slice's mean loss times n_i / n.  `n_rows`: the batch is zero-padded, the criterion is told
    each slice's place and returns its share of the mean as it is.  Nothing of a slice outlives its backward but the sums."""
    n = x.shape[0]
    total = correct = None
    for i in range(0, n, mb):
        xs, ys = x[i:i + mb], y[i:i + mb]
        if n_rows is not None:
            criterion.place(n_rows, i)
        out = model(xs)
        loss = criterion(out, ys)
        if weighted:
            loss = loss * (xs.shape[0] / n)
        loss.backward()
        total = loss.detach() if total is None else total + loss.detach()
        c = _correct(criterion, out, ys)
        correct = c if correct is None else correct + c
        del out, loss, c
    return total, correct


def _correct(criterion, out, y):
    """correct-count of the batch the criterion has just seen: its own when it keeps one, else the argmax line"""
    if hasattr(criterion, "correct"):
        return criterion.correct()
    return (out.detach().argmax(-1) == y).sum()


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
    (the default): the batch runs as it comes."""

    def __init__(self, model, optimizer=None, reducer=None, criterion=None, micro_batch=None, pad_to=None):
        self.model, self.opt, self.reducer = model, optimizer, reducer
        self.pad_to, self._pad = pad_to, None
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
        mb = self.micro_batch if self.micro_batch and self.micro_batch < n else n
        n_acc = (n + mb - 1) // mb
        if self.reducer is not None:
            self.reducer.zero_grad(n_acc)
        elif self.opt is not None:
            self.opt.zero_grad(set_to_none=True)
        total, correct = _run_slices(self.model, self.criterion, x, y, mb, weighted=self.pad_to is None, n_rows=self.n_rows)
        if self.reducer is not None:
            self.reducer.finish()
        if self.opt is not None:
            self.opt.step()
        self.loss, self.correct = total, correct
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
    step is two more nodes of the graph (the class's `advance` and `step` entry points, e.g. hwgat_optim_advance and
    hwgat_optim_step): its hyper-parameters are fp64 device words that the kernels read when they run, so `__call__` only
    pushes the param groups' values when they changed (its `set` entry point, one tiny launch, e.g. after
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

    Inputs are copied into static buffers; `loss` / `correct` are static device tensors rewritten by every replay.
    Shapes are fixed at capture.  Parameters must not be reallocated afterwards (same rule as serve.GraphedEval).
    The warm-up's traces in the model's buffers (BatchNorm running statistics) are undone like those in the weights.
    With `model._drop_calls = c` before construction, replay k (1-based) draws exactly the masks the eager TrainStep
    draws in its k-th step from the same `c` (tests/test_gpu_graph.py).  Each forward hands its kernels a per-call copy of
    the base seed (seeding.DeviceSeeds._next_step_seed); in the graph that copy is a node after the seed advance."""

    def __init__(self, model, optimizer, x, y, criterion=None, warmup=2, reducer=None, micro_batch=None, ragged=False):
        import importlib
        HF = importlib.import_module(__package__ + ".functional")
        micro_batch = _check_micro_batch(micro_batch)
        if micro_batch is not None and reducer is not None:
            raise NotImplementedError("micro_batch with a reducer: the all-reduce inside a capture is untested")
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
        self.model, self.opt, self.reducer = model, optimizer, reducer
        self.criterion = criterion or SmoothedCrossEntropyLoss()
        self.ragged, self._pad = bool(ragged), None
        if self.ragged:
            self._pad = _PaddedBatch(x.shape[0], x, y)
            self._pad.load(x.detach(), y.detach())
            self.x, self.y = self._pad.x, self._pad.y
        else:
            self.x, self.y = x.detach().clone(), y.detach().clone()
        B = x.shape[0]
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
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self._one()
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
        del keep_p, keep_b, keep_state
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
        if self.n_slices == 1 and not self.ragged:       # the unsliced step, node for node what it has always been
            out = self.model(self.x)
            loss = self.criterion(out, self.y)
            loss.backward()
            if self.reducer is not None:
                self.reducer.finish()
            if step:
                self.opt.step()
            return loss.detach(), _correct(self.criterion, out, self.y)
        loss, correct = _run_slices(self.model, self.criterion, self.x, self.y, self.micro_batch, weighted=not self.ragged,
                                    n_rows=self.n_rows)
        if step:                                         # once, after the last slice (no reducer here: refused above)
            self.opt.step()
        return loss, correct

    def _addresses(self):
        return tuple(t.data_ptr() for t in list(self.model.parameters()) + list(self.model.buffers()))

    def __call__(self, x, y):
        if not self.model.training:
            raise ValueError("GraphedTrainStep replays the train() step: call model.train() first")
        if not self.ragged and (x.shape != self.x.shape or y.shape != self.y.shape):
            raise ValueError(f"captured for {tuple(self.x.shape)} / {tuple(self.y.shape)}, got {tuple(x.shape)} / {tuple(y.shape)}")
        if self._addresses() != self._addr:
            raise RuntimeError("a parameter or buffer of the model was reallocated after the capture: capture again")
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
