"""Evaluation forward captured in a HIP graph.

The reference evaluates with `model.eval(); model(x)` (hwgat/utils.py:119-134): ~280 kernel launches per forward here.  At
the training batch that is hidden behind the GPU time; at serving batches (B = 1 .. 8) the forward is launch-bound -- the host
issues launches slower than the GPU retires them.  `GraphedEval` records the eval forward of a model ONCE for a fixed input
shape (HIP stream capture through torch.cuda.graphs: every launch of the forward goes to torch's current stream, so the C-ABI
launches are captured like torch's own) and replays it per call: one graph launch instead of ~280 kernel launches.  The
eval forward is bit-reproducible, so a replay returns exactly the eager result.

    hw = importlib.import_module("sl-hwgat_amd")
    serve = importlib.import_module("sl-hwgat_amd.serve")
    fast = serve.GraphedEval(model, torch.empty(1, 128, 80, 2, device=dev))
    logits = fast(x)          # x: same shape / dtype / device as the example

The weights are read at replay time (the graph holds the launches, not the values): an optimizer step or load_state_dict
between calls is seen by the next replay, as long as no parameter is reallocated.  The graph holds raw ADDRESSES -- of the
parameters and of the derived weight copies (functional.WeightPrep) -- so a reallocated parameter (`model.to()`,
`load_state_dict(assign=True)`) would make a replay read stale or recycled memory: `GraphedEval` keeps the WeightPrep
objects it captured alive, compares the addresses of every source parameter with the captured ones on each call and
raises "capture again" on a mismatch.

`StreamRecognizer` puts live input in front of that graph and a decision behind it: raw keypoint frames of several streams
go into device ring buffers, and one replay per step pushes the new frames, cuts every stream's window, applies the eval
transform, runs the forward and decides whether a sign was seen (csrc/stream.hip).
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import augment
from . import functional as HF


class GraphedEval:
    """`tail`, when given, is a callable that takes the static logits and is captured right after the forward (warmed up with
    it, too): whatever it launches replays with the graph, and what it returns is kept as `static_tail`.  `run()` replays
    in place for such callers -- they fill `static_in` themselves and read the static results.  With `graph=False` nothing is
    captured: `run()` issues the same forward and tail eagerly on the same static buffers, under the same train() check
    (the partner of an A/B measurement, evaluate.Evaluator(graph=False)).

    `head` is the mirror of `tail`: a callable that takes `static_in` and is captured right in front of the forward.  What it
    launches fills `static_in` on the device (StreamRecognizer: ring push, window, hand fill, resample), so such a caller
    copies nothing into `static_in` itself.  `None` (the default) captures exactly the forward (+ tail)."""

    def __init__(self, model, example, warmup=2, tail=None, graph=True, head=None):
        if model.training:
            raise ValueError("GraphedEval captures the eval() forward: call model.eval() first")
        if not example.is_cuda:
            raise ValueError("the example input must live on the GPU")
        self.model, self.tail, self.head = model, tail, head
        self.static_in = example.detach().clone()
        self.static_tail = None
        self.graph = None
        if not graph:
            self._forward()
            return
        side = torch.cuda.Stream(device=example.device)
        side.wait_stream(torch.cuda.current_stream(example.device))
        with torch.cuda.stream(side):                         # warm-up off the default stream, as torch.cuda.graphs asks
            for _ in range(max(1, warmup)):
                self._forward()
        torch.cuda.current_stream(example.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._forward()
        # the derived weight copies the captured launches read and rewrite: referenced here so that a later eager forward,
        # which may replace the model's cache entry, cannot hand their memory back to the allocator under the graph
        # (of the model itself and, for a model made of models -- ensemble.Ensemble --, of every module below it)
        self._preps = dict(model.__dict__.get("_weight_prep_cache", {}))
        for name, sub in model.named_modules():
            if sub is not model and "_weight_prep_cache" in sub.__dict__:
                self._preps.update({(name,) + key: wp for key, wp in sub.__dict__["_weight_prep_cache"].items()})
        self._captured = self._addresses()

    def _forward(self):
        with torch.no_grad():
            if self.head is not None:
                self.head(self.static_in)
            self.static_out = self.model(self.static_in)
            if self.tail is not None:
                self.static_tail = self.tail(self.static_out)

    def _addresses(self):
        """addresses of everything the captured launches take by pointer from the model"""
        m = self.model
        sig = ()
        for sub in m.modules():                               # the model itself first; an ensemble's members after it
            if hasattr(sub, "block_list"):
                sig += HF.WeightPrep.signature(sub.block_list(), sub.activation_dtype, False)[2]
        rest = tuple(t.data_ptr() for t in list(m.parameters()) + list(m.buffers()))
        return sig, rest

    def check(self):
        """what a replay relies on: no parameter reallocated since the capture, the model still in eval()"""
        if self.graph is not None and self._addresses() != self._captured:
            raise RuntimeError("a parameter or buffer of the model was reallocated after the capture (model.to(), "
                               "load_state_dict(assign=True), ...): the graph holds the old addresses -- capture again")
        if self.model.training:
            raise RuntimeError("the model was switched to train() after the capture; GraphedEval replays the eval() forward")

    def run(self):
        """forward (+ tail) on what `static_in` holds now, results in `static_out` / `static_tail`; synchronises nothing"""
        self.check()
        self._replay()

    def _replay(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self._forward()

    def __call__(self, x):
        """logits for `x` (shape / dtype of the captured example); the result is a fresh tensor"""
        if x.shape != self.static_in.shape or x.dtype != self.static_in.dtype:
            raise ValueError(f"captured for {tuple(self.static_in.shape)} {self.static_in.dtype}, got {tuple(x.shape)} {x.dtype}")
        self.check()
        self.static_in.copy_(x, non_blocking=True)
        self._replay()
        return self.static_out.clone()


# the records of the state block (include/hwgat_hip.h, "streaming recognition") as numpy sees them
STREAM_HEADER = np.dtype([("log_count", "<i8"), ("overflow", "<i8"), ("alpha", "<f4"), ("threshold", "<f4"),
                          ("hold", "<i4"), ("blank_class", "<i4"), ("spare", "<i8", (4,))])
STREAM_WORDS = np.dtype([("head", "<i4"), ("count", "<i4"), ("frames_seen", "<i8"), ("ready", "<i4"), ("win_len", "<i4"),
                         ("top", "<i4"), ("run", "<i4"), ("conf", "<f4"), ("fired", "<i4"), ("evals", "<i8"),
                         ("events", "<i8"), ("spare", "<i8")])
STREAM_EVENT = np.dtype([("frames_seen", "<i8"), ("evaluation", "<i8"), ("stream", "<i4"), ("cls", "<i4"), ("conf", "<f4"),
                         ("pad", "<i4")])
assert (STREAM_HEADER.itemsize, STREAM_WORDS.itemsize, STREAM_EVENT.itemsize) == \
    (8 * HF.STREAM_HEADER_WORDS, 8 * HF.STREAM_WORDS, 8 * HF.STREAM_EVENT_WORDS)


class StreamEvent(NamedTuple):
    """one recognised sign: the stream, the frames that stream had received, its 0-based ready evaluation, class, confidence"""
    stream: int
    frames_seen: int
    evaluation: int
    cls: int
    conf: float


class StreamRecognizer:
    """Live recognition on `n_streams` keypoint streams: raw (joints, coords) frames go into device ring buffers and every
    `step` replays ONE graph -- ring push, window cut + eval transform record (hwgat_stream_push / _window), the hand fill and
    the resampler of augment.py into the model's static input, the eval forward, and the decision rule on the logits
    (hwgat_stream_decide: softmax, exponential smoothing, "the same top class `hold` evaluations in a row at `threshold`").
    Nothing is read back until `poll`.

        rec = serve.StreamRecognizer(model, n_streams=4, window_frames=192, ring_frames=256, push_frames=8, coords=2)
        while True:
            frames, counts = grab()             # (4, 8, 29, 2) float32, (4,) new frames per stream in [0, 8]
            rec.step(frames, counts)
            for ev in rec.poll()["events"]:
                print(ev.stream, ev.cls, ev.conf)

    `model` is any of the seven models taking (B, T, K, C) in eval(), or an ensemble.Ensemble of them; T =
    `model.temporal_dim` is the clip length the window is resampled to.  `out_joints=None` hands the model the raw joints (HWGATE with `use_part_table(part_table(29))`); a
    gather table hands it that layout.  A stream is ready once it holds `min_frames` frames and a frame whose origin and
    anchor joints are non-zero (with anchors a positive finite distance apart); a stream that is not ready gets a benign
    input row and its decision state does not move.  `alpha`, `threshold`, `hold`, `blank_class` live in device words
    (`set_decision`): changing them needs no new capture.  The log holds the events between two polls; `poll` empties it.

    `graph=False` issues the same launches eagerly on the same buffers (identical bits).  `step` and `push` synchronise
    nothing: host input goes through two pinned staging buffers used in turn, and a call waits only for the upload that
    read its buffer two calls ago.  Call everything from one thread, on one stream."""

    def __init__(self, model, n_streams, window_frames, ring_frames, push_frames, joints=29, coords=2, out_joints=None,
                 min_frames=1, alpha=0.5, threshold=0.6, hold=3, blank_class=-1, log_capacity=1024,
                 hands=(9, 19, 7, 19, 29, 8), origin_idx=0, anchor_points=(3, 4), graph=True):
        if model.training:
            raise ValueError("StreamRecognizer captures the eval() forward: call model.eval() first")
        if not hasattr(model, "temporal_dim"):
            raise ValueError("the model must take (B, T, K, C) clips and carry `temporal_dim`")
        if len(hands) != 6:
            raise ValueError("hands: (left first, left end, left wrist, right first, right end, right wrist)")
        S, Wf, R, F, J, C = (int(v) for v in (n_streams, window_frames, ring_frames, push_frames, joints, coords))
        self.src_len = int(model.temporal_dim)
        base = augment._Base(self.src_len, tuple(hands[:3]), tuple(hands[3:]), origin_idx, anchor_points)
        self.hands, self.norm_idx = base.hands, tuple(int(j) for j in base.norm_idx)
        if not 1 <= S <= HF.STREAM_MAX_STREAMS:
            raise ValueError(f"n_streams in [1, {HF.STREAM_MAX_STREAMS}], got {n_streams}")
        if not 1 <= R <= HF.STREAM_MAX_FRAMES:
            raise ValueError(f"ring_frames in [1, {HF.STREAM_MAX_FRAMES}], got {ring_frames}")
        if not 1 <= Wf <= R or not 1 <= F <= R:
            raise ValueError(f"window_frames and push_frames in [1, ring_frames = {R}], got {window_frames} and {push_frames}")
        if C not in (2, 3) or J < self.hands[4] or max(self.norm_idx + (self.hands[2], self.hands[5])) >= J or \
                min(self.norm_idx) < 0:
            raise ValueError(f"frames of {J} joints x {C} coordinates do not hold the hands {self.hands} and the "
                             f"origin / anchors {self.norm_idx} (coords in (2, 3))")
        if int(min_frames) < 1 or not 0 <= int(log_capacity) <= HF.STREAM_MAX_LOG:
            raise ValueError(f"min_frames >= 1 and log_capacity in [0, {HF.STREAM_MAX_LOG}]")
        self.n_streams, self.window_frames, self.ring_frames, self.push_frames = S, Wf, R, F
        self.joints, self.coords, self.min_frames, self.log_capacity = J, C, int(min_frames), int(log_capacity)
        self._decision = self._checked_decision(dict(alpha=0.5, threshold=0.6, hold=3, blank_class=-1),
                                                alpha, threshold, hold, blank_class)
        dev = next(model.parameters()).device                 # every host check has passed: the first look at the device
        if dev.type != "cuda":
            raise ValueError("the model must live on the GPU: StreamRecognizer keeps its rings on the model's device")
        self.device = dev
        self._gather = None
        if out_joints is not None:
            g = torch.as_tensor(out_joints, dtype=torch.int32).reshape(-1)
            if int(g.min()) < 0 or int(g.max()) >= J:
                raise ValueError(f"gather table entries must be joint indices in [0, {J})")
            self._gather = g.to(dev)
        J_out = J if self._gather is None else self._gather.numel()

        # static device buffers: everything a replay reads or writes
        self._in_bytes = S * F * J * C * 4
        self._in = torch.zeros(self._in_bytes + S * 4, dtype=torch.uint8, device=dev)
        self._frames = self._in[:self._in_bytes].view(torch.float32).view(S, F, J, C)
        self._counts = self._in[self._in_bytes:].view(torch.int32)
        self._pinned = [torch.zeros(self._in.numel(), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._uploaded = [None, None]
        self._slot = 0
        self.ring = torch.zeros((S, R, J, C), dtype=torch.float32, device=dev)
        self.state = torch.zeros(HF.stream_state_words(S, self.log_capacity), dtype=torch.int64, device=dev)
        self._words = self.state[HF.STREAM_HEADER_WORDS:HF.STREAM_HEADER_WORDS + S * HF.STREAM_WORDS].view(S, HF.STREAM_WORDS)
        self.clip = torch.zeros((S * Wf, J, C), dtype=torch.float32, device=dev)
        self.clip_off = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        self.frame_map = torch.zeros((S, self.src_len), dtype=torch.int32, device=dev)
        self.params = torch.zeros((S, HF.STREAM_NPRM), dtype=torch.float64, device=dev)
        self._ws = torch.empty(int(_lib.lib().hwgat_aug_hand_fill_ws_bytes(S * Wf)), dtype=torch.uint8, device=dev)
        self._hv = augment.ctypes_int32_6(*self.hands)
        self.q = None                                         # (S, classes) fp32, sized by the first logits
        self._write_decision()
        self._runner = GraphedEval(model, torch.zeros((S, self.src_len, J_out, C), dtype=torch.float32, device=dev),
                                   tail=self._tail, graph=graph, head=self._head)
        self.reset()                                          # warm-up and capture ran on empty rings

    # ------------------------------------------------------------ what the graph holds
    def _head(self, static_in):
        S, Wf, J, C = self.n_streams, self.window_frames, self.joints, self.coords
        HF.stream_push(self.ring, self.state, self._frames, self._counts)
        HF.stream_window(self.ring, self.state, self.clip, self.clip_off, self.frame_map, self.params, Wf, self.min_frames,
                         self.norm_idx[0], self.norm_idx[1:], self.hands)
        HF.call("hwgat_aug_hand_fill", _lib.ptr(self.clip), _lib.ptr(self.clip_off), None, S, S * Wf, Wf, J, C, self._hv,
                _lib.ptr(self._ws), self._ws.numel(), None, _lib.stream())
        HF.call("hwgat_aug_resample", _lib.ptr(self.clip), _lib.ptr(self.clip_off), _lib.ptr(self.frame_map),
                _lib.ptr(self.params), _lib.ptr(self._gather), _lib.ptr(static_in), S, self.src_len, J, static_in.shape[2], C,
                _lib.stream())

    def _tail(self, logits):
        z = logits.float().contiguous()
        if z.dim() != 2 or z.shape[0] != self.n_streams:
            raise ValueError(f"the model returned {tuple(z.shape)}, expected ({self.n_streams}, classes) logits")
        if self.q is None:                                    # the first warm-up call, never inside a capture
            self.q = torch.zeros_like(z)
        HF.stream_decide(self.state, self.q, z, self.log_capacity)
        return z

    # ------------------------------------------------------------ decision parameters (device words)
    @staticmethod
    def _checked_decision(cur, alpha=None, threshold=None, hold=None, blank_class=None):
        new = dict(cur)
        for k, v in (("alpha", alpha), ("threshold", threshold), ("hold", hold), ("blank_class", blank_class)):
            if v is not None:
                new[k] = v
        if not 0.0 <= float(new["alpha"]) <= 1.0:
            raise ValueError(f"alpha in [0, 1], got {new['alpha']}")
        if int(new["hold"]) != new["hold"] or int(new["hold"]) < 1:
            raise ValueError(f"hold must be an integer >= 1, got {new['hold']}")
        if int(new["blank_class"]) != new["blank_class"] or int(new["blank_class"]) < -1:
            raise ValueError(f"blank_class must be a class index or -1, got {new['blank_class']}")
        return dict(alpha=float(new["alpha"]), threshold=float(new["threshold"]), hold=int(new["hold"]),
                    blank_class=int(new["blank_class"]))

    def _write_decision(self):
        d = self._decision
        words = np.concatenate([np.array([d["alpha"], d["threshold"]], dtype=np.float32).view(np.int64),
                                np.array([d["hold"], d["blank_class"]], dtype=np.int32).view(np.int64)])
        self.state[2:4].copy_(torch.from_numpy(words))

    def set_decision(self, alpha=None, threshold=None, hold=None, blank_class=None):
        """change the rule's parameters; the next replay reads them (no new capture)"""
        self._decision = self._checked_decision(self._decision, alpha, threshold, hold, blank_class)
        self._write_decision()

    # ------------------------------------------------------------ input
    @staticmethod
    def check_counts(counts, n_streams, push_frames):
        """host counts as int32 (n_streams,), each in [0, push_frames]"""
        cn = np.asarray(counts.numpy() if isinstance(counts, torch.Tensor) else counts)
        if cn.shape != (n_streams,) or cn.dtype.kind not in "iu":
            raise ValueError(f"counts must hold {n_streams} integers, got {cn.dtype} {cn.shape}")
        if (cn < 0).any() or (cn > push_frames).any():
            raise ValueError(f"counts must lie in [0, {push_frames}], got {cn.tolist()}")
        return cn.astype(np.int32)

    def _load(self, frames, counts):
        S, F, J, C = self.n_streams, self.push_frames, self.joints, self.coords
        f_dev = isinstance(frames, torch.Tensor) and frames.is_cuda
        c_dev = isinstance(counts, torch.Tensor) and counts.is_cuda
        if not isinstance(frames, torch.Tensor):
            frames = np.asarray(frames, dtype=np.float32)
        if tuple(frames.shape) != (S, F, J, C):
            raise ValueError(f"frames must be ({S}, {F}, {J}, {C}), got {tuple(frames.shape)}")
        if c_dev and tuple(counts.shape) != (S,):
            raise ValueError(f"counts must hold {S} integers, got {tuple(counts.shape)}")
        cn = None if c_dev else self.check_counts(counts, S, F)
        if f_dev:
            self._frames.copy_(frames, non_blocking=True)
        if c_dev:
            self._counts.copy_(counts, non_blocking=True)     # no host check possible: the kernel clamps to [0, F]
        if f_dev and c_dev:
            return
        s = self._slot
        self._slot = 1 - s
        if self._uploaded[s] is not None:
            self._uploaded[s].synchronize()                   # the upload that last read this pinned buffer has finished
        hb = self._pinned[s].numpy()
        if not c_dev:
            hb[self._in_bytes:].view(np.int32)[:] = cn
        if not f_dev:
            hb[:self._in_bytes].view(np.float32).reshape(S, F, J, C)[:] = \
                frames.numpy() if isinstance(frames, torch.Tensor) else frames
        lo, hi = (0 if not f_dev else self._in_bytes), (self._in.numel() if not c_dev else self._in_bytes)
        self._in[lo:hi].copy_(self._pinned[s][lo:hi], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._uploaded[s] = ev

    def step(self, frames, counts):
        """append counts[s] of the frames (S, F, J, C) to stream s and evaluate every stream: one upload, one graph replay"""
        self._runner.check()
        self._load(frames, counts)
        self._runner._replay()

    def push(self, frames, counts):
        """append only: one eager launch, no evaluation"""
        self._load(frames, counts)
        HF.stream_push(self.ring, self.state, self._frames, self._counts)

    # ------------------------------------------------------------ results
    @property
    def logits(self):
        """the static (S, classes) fp32 logits of the last step"""
        return self._runner.static_tail

    @property
    def model_input(self):
        """the model's static input (S, T, J_out, C) of the last step"""
        return self._runner.static_in

    def poll(self):
        """ONE device-to-host read (synchronises): {"events": [StreamEvent] since the last poll, in emission order,
        "overflow": events the full log could not take, and per stream (numpy, length S) "ready", "top", "conf", "run",
        "count", "frames_seen", "evals", "n_events"}"""
        host = self.state.cpu().numpy()
        S, H = self.n_streams, HF.STREAM_HEADER_WORDS
        head = host[:H].view(STREAM_HEADER)[0]
        words = host[H:H + S * HF.STREAM_WORDS].view(STREAM_WORDS)
        n = min(max(int(head["log_count"]), 0), self.log_capacity)
        log = host[H + S * HF.STREAM_WORDS:].view(STREAM_EVENT)[:n]
        events = [StreamEvent(int(e["stream"]), int(e["frames_seen"]), int(e["evaluation"]), int(e["cls"]), float(e["conf"]))
                  for e in log]
        overflow = int(head["overflow"])
        if n or overflow:
            self.state[0:2].zero_()                           # the log is empty again (stream-ordered, no wait)
        out = {"events": events, "overflow": overflow}
        for key, field in (("ready", "ready"), ("top", "top"), ("conf", "conf"), ("run", "run"), ("count", "count"),
                           ("frames_seen", "frames_seen"), ("evals", "evals"), ("n_events", "events")):
            out[key] = words[field].copy()
        return out

    def reset(self, streams=None):
        """clear the rings and the decision state of all streams or of the listed ones; the log and the rule's parameters
        stay.  Synchronises nothing"""
        if streams is None:
            self.ring.zero_()
            self._words.zero_()
            if self.q is not None:
                self.q.zero_()
            return
        idx = sorted({int(s) for s in streams})
        if idx and not (0 <= idx[0] and idx[-1] < self.n_streams):
            raise ValueError(f"streams in [0, {self.n_streams}), got {idx}")
        if not idx:
            return
        t = torch.tensor(idx, dtype=torch.int64, device=self.device)
        self.ring.index_fill_(0, t, 0.0)
        self._words.index_fill_(0, t, 0)
        if self.q is not None:
            self.q.index_fill_(0, t, 0.0)
