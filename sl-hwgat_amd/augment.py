"""Device-side train / val-test transforms (reference hwgat/configs.py:93-108, hwgat/dataTransform.py).

The reference runs `train_transform` in DataLoader workers on the CPU; its `HandCorrection` refits a scipy spline for
every missing frame, joint and coordinate and costs ~30 ms per clip at 128 raw frames, which caps the input pipeline
below the speed of the training step.  Here the work is split in two halves:

  host    `TrainTransform.draw(clip)` / `EvalTransform.draw(clip)` consume Python `random` and `np.random` with the
          same calls, arguments and order as the reference's `Compose` and return a small picklable `AugRecord`
          (masked frames, normalisation, shear / rotation / flip parameters, the composed frame map).  Cheap: run it
          in the DataLoader workers.
  device  `AugmentBatcher` packs raw clips + records into pinned memory, uploads them on a side stream and launches
          `hwgat_aug_hand_fill` (masking + the spline hand fill) and `hwgat_aug_resample` (normalise, shear, rotate,
          temporal resampling, flip, optional WindowCreate gather) on the consumer stream.

With the same RNG state the result equals the reference's output clip for clip, to fp32 rounding.  The training loop:

    tf = TrainTransform(src_len)
    class DS(torch.utils.data.Dataset):
        def __getitem__(self, i):
            clip = load(i).astype(np.float32)                  # raw (T, 29, C)
            return clip, label(i), tf.draw(clip)               # draw in the worker
    loader = DataLoader(DS(), batch_size=B, shuffle=True, num_workers=8, collate_fn=list)
    batcher = AugmentBatcher(B, max_frames, dev)               # main process
    for batch in loader:
        x, y = batcher(batch)                                  # (B, src_len, 29, C) fp32 on the device
        step(x, y)

Deliberate deviations from the reference: a hand counts as absent everywhere when every coordinate is zero (the
reference tests `np.sum == 0`); the errors the reference hits (fewer than 5 raw frames: IndexError in KeypointMasking;
no frame with origin and both anchors non-zero: UnboundLocalError in NormalizeKeypoints) are raised by `draw` as
`ValueError` with a message.
"""
import ctypes
import random
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

NPRM = 24                   # HWGAT_AUG_NPRM
MAX_FRAMES = 4096           # HWGAT_AUG_MAX_FRAMES
ctypes_int32_6 = ctypes.c_int32 * 6


class AugRecord(NamedTuple):
    """Per-clip parameters of one transform application (everything the device needs besides the raw clip)."""
    T: int                      # raw frames
    masked: np.ndarray          # sorted frames whose hands KeypointMasking zeroes (empty: eval)
    left_top: np.ndarray        # (C,) float32 NormalizeKeypoints
    edge_dist: np.float32
    shear_origin: np.ndarray    # (C,) float64
    shear: float
    rot_origin: np.ndarray      # (C,) float64
    rot: np.ndarray             # (C, C) float64, applied as x @ rot
    flip: bool
    pad32: bool                 # TemporalSample padded the clip (fp32 buffer): the flip acts on rounded values
    src: np.ndarray             # (src_len,) int32 raw frame of every output frame
    hands: Tuple[int, ...]      # (left first, left end, left wrist, right first, right end, right wrist)


def euler_xyz_degrees(thetas) -> np.ndarray:
    """rotation matrix of extrinsic x-y-z Euler angles in degrees (scipy Rotation.from_euler("xyz", degrees=True))"""
    a, b, c = np.deg2rad(np.asarray(thetas, dtype=np.float64))
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return rz @ ry @ rx


class _Base:
    def __init__(self, src_len, left_slice, right_slice, origin_idx, anchor_points):
        l0, l1, lw = left_slice
        r0, r1, rw = right_slice
        if not (0 <= l0 < l1 <= r0 < r1) or lw in range(l0, r1) or rw in range(l0, r1):
            raise ValueError("hand slices: left [l0, l1) before right [r0, r1), adjacent, wrists outside both")
        if l1 != r0:
            raise ValueError("KeypointMasking zeroes joints [left first, right end): the hands must be adjacent")
        if len(anchor_points) != 2:
            raise ValueError("NormalizeKeypoints takes exactly two anchor points")
        self.src_len = int(src_len)
        self.hands = (l0, l1, lw, r0, r1, rw)
        self.norm_idx = [origin_idx, anchor_points[0], anchor_points[1]]
        if any(l0 <= j < r1 for j in self.norm_idx):
            raise ValueError("origin / anchor joints must lie outside the hands")

    def _check(self, clip):
        clip = np.asarray(clip, dtype=np.float32)
        if clip.ndim != 3 or clip.shape[2] not in (2, 3) or clip.shape[1] < self.hands[4]:
            raise ValueError(f"expected a raw clip (T, J >= {self.hands[4]}, C in (2, 3)), got {clip.shape}")
        if clip.shape[0] > MAX_FRAMES:
            raise ValueError(f"clip of {clip.shape[0]} raw frames: the device hand fill supports up to {MAX_FRAMES}")
        return clip

    def _normalisation(self, clip):
        """left_top / edge_dist of the first frame whose origin and anchors are fully non-zero, in the clip's dtype
        (dataTransform.py:96-109); those joints are never masked or hand-corrected, so the raw clip decides"""
        o, a0, a1 = self.norm_idx
        ok = np.all(clip[:, self.norm_idx] != 0, axis=(1, 2))
        if not ok.any():
            raise ValueError("no frame has the origin and both anchor joints non-zero: the clip cannot be normalised "
                             "(the reference raises UnboundLocalError in NormalizeKeypoints)")
        kp = clip[int(np.argmax(ok))]
        unit = np.linalg.norm(kp[a0] - kp[a1])
        left_top = kp[o] - 3 * unit
        left_top[1] = kp[o][1] - 2 * unit
        return left_top, 6 * unit

    def _temporal_sample(self, L, random_shift):
        """TemporalSample (dataTransform.py:300-326) as a map from output frame to input frame"""
        n = self.src_len
        if L <= n:
            s = np.clip(np.random.normal(loc=0.5, scale=0.1, size=1), 0, 1)[0] if random_shift else 0.5
            start = int((n - L) * s)
            t = np.arange(n)
            inside = (t >= start) & (t < start + L)
            # rows outside the placed clip keep the pad they were created with: first frame in the front half
            return np.where(inside, t - start, np.where(t < n // 2, 0, L - 1)), True
        return np.linspace(0, L - 1, num=n).astype(int), False


class TrainTransform(_Base):
    """Host half of the reference's train transform (configs.py:93-103); defaults are configs.py:14-25."""

    def __init__(self, src_len, left_slice=(9, 19, 7), right_slice=(19, 29, 8), origin_idx=0, anchor_points=(3, 4),
                 frame_augmentation=(0.5, 1.5), sampling_prob=0.2, shear_std=0.1, rotation_std=0.1,
                 random_sample=True, random_shift=True):
        super().__init__(src_len, left_slice, right_slice, origin_idx, anchor_points)
        self.frame_augmentation = tuple(frame_augmentation)
        self.sampling_prob, self.shear_std, self.rotation_std = sampling_prob, shear_std, rotation_std
        self.random_sample, self.random_shift = random_sample, random_shift

    def draw(self, clip) -> AugRecord:
        clip = self._check(clip)
        T, C = clip.shape[0], clip.shape[2]
        # KeypointMasking: a sorted sample of int(p T) frames
        n_mask = int(self.sampling_prob * T)
        masked = sorted(random.sample(list(range(T)), n_mask))
        if n_mask == 0:
            raise ValueError(f"clip of {T} raw frames: KeypointMasking masks int({self.sampling_prob} * T) = 0 frames "
                             "(the reference raises IndexError); train clips need at least "
                             f"{int(np.ceil(1 / self.sampling_prob))} frames")
        left_top, edge_dist = self._normalisation(clip)
        # ShearTransform: origin, then the shear
        shear_origin = np.clip(np.random.normal(loc=0.5, scale=0.1, size=C), 0, 1)
        shear = np.random.normal(loc=0, scale=self.shear_std, size=1)[0]
        # RotatationTransform: origin, then the angle (C = 2) or three Euler angles in units of 90 degrees (C = 3)
        rot_origin = np.clip(np.random.normal(loc=0.5, scale=0.1, size=C), 0, 1)
        if C == 2:
            ang = np.random.normal(loc=0, scale=self.rotation_std, size=1)[0]
            cs, sn = np.cos(ang), np.sin(ang)
            rot = np.array([[cs, -sn], [sn, cs]])
        else:
            rot = euler_xyz_degrees(np.random.normal(loc=0, scale=self.rotation_std, size=3) * 90)
        # TemporalAugmentation: a frame-rate ratio, then random (sorted) or evenly spaced frames
        lo, hi = self.frame_augmentation
        ratio = (hi - lo) * random.uniform(0, 1) + lo
        L = int(T * ratio)
        if random.uniform(0, 1) < 0.5 and self.random_sample:
            if ratio <= 1:
                aug = sorted(random.sample(list(range(T)), L))
            else:
                aug = sorted(random.choices(list(range(T)), k=L))
            aug = np.asarray(aug, dtype=np.int64)
        else:
            aug = np.linspace(0, T - 1, num=L).astype(int)
        m, pad32 = self._temporal_sample(L, self.random_shift)
        flip = random.uniform(0, 1) <= 0.5
        return AugRecord(T, np.asarray(masked, dtype=np.int64), left_top, edge_dist, shear_origin, float(shear),
                         rot_origin, rot, bool(flip), pad32, aug[m].astype(np.int32), self.hands)


class EvalTransform(_Base):
    """Host half of the reference's val / test transform (configs.py:105-108): hand correction, normalise, centred
    TemporalSample.  Draws nothing."""

    def __init__(self, src_len, left_slice=(9, 19, 7), right_slice=(19, 29, 8), origin_idx=0, anchor_points=(3, 4)):
        super().__init__(src_len, left_slice, right_slice, origin_idx, anchor_points)

    def draw(self, clip) -> AugRecord:
        clip = self._check(clip)
        T, C = clip.shape[0], clip.shape[2]
        left_top, edge_dist = self._normalisation(clip)
        m, pad32 = self._temporal_sample(T, False)
        zero = np.zeros(C)
        return AugRecord(T, np.zeros(0, dtype=np.int64), left_top, edge_dist, zero, 0.0, zero, np.eye(C), False,
                         pad32, m.astype(np.int32), self.hands)


def _params(rec: AugRecord, out: np.ndarray):
    """the HWGAT_AUG_NPRM doubles of include/hwgat_hip.h"""
    C = len(rec.left_top)
    out[:] = 0.0
    out[0:C] = rec.left_top
    out[3] = rec.edge_dist
    out[4:4 + C] = rec.shear_origin
    out[7] = rec.shear
    out[8:8 + C] = rec.rot_origin
    m = np.eye(3)
    m[:C, :C] = rec.rot
    out[11:20] = m.reshape(-1)
    out[20] = 1.0 if rec.flip else 0.0
    out[21] = 1.0 if rec.pad32 else 0.0


def hand_fill(x: torch.Tensor, clip_off: torch.Tensor, max_frames: int, masked: Optional[torch.Tensor] = None,
              hands=(9, 19, 7, 19, 29, 8), tap: Optional[torch.Tensor] = None):
    """hwgat_aug_hand_fill on device tensors, in place: x (total_frames, J, C) fp32, clip_off (n+1) int32,
    masked (total_frames) uint8 or None; tap: None or an fp64 tensor shaped like x"""
    total, J, C = x.shape
    ws = torch.empty(int(_lib.lib().hwgat_aug_hand_fill_ws_bytes(total)), dtype=torch.uint8, device=x.device)
    hv = (ctypes_int32_6)(*hands)
    _lib.call("hwgat_aug_hand_fill", _lib.ptr(x), _lib.ptr(clip_off), _lib.ptr(masked), clip_off.numel() - 1, total,
              int(max_frames), J, C, hv, _lib.ptr(ws), ws.numel(), _lib.ptr(tap), _lib.stream())


def resample(x: torch.Tensor, clip_off: torch.Tensor, src: torch.Tensor, prm: torch.Tensor,
             gather: Optional[torch.Tensor] = None) -> torch.Tensor:
    """hwgat_aug_resample on device tensors: returns (n, src_len, J_out, C) fp32"""
    total, J, C = x.shape
    n, src_len = src.shape
    J_out = J if gather is None else gather.numel()
    out = torch.empty((n, src_len, J_out, C), dtype=torch.float32, device=x.device)
    _lib.call("hwgat_aug_resample", _lib.ptr(x), _lib.ptr(clip_off), _lib.ptr(src), _lib.ptr(prm), _lib.ptr(gather),
              _lib.ptr(out), n, src_len, J, J_out, C, _lib.stream())
    return out


def _align(n, a=256):
    return (n + a - 1) // a * a


class AugmentBatcher:
    """Ragged raw clips + `AugRecord`s -> the model's input batch on the device.

    `__call__(samples)`, samples a list of (raw clip (T, J, C) float32, label, record), returns (x, y): x (n, src_len,
    J_out, C) fp32 and y (n,) int64, fresh device tensors.  `out_joints=None` keeps the J raw joints (HWGATE with
    `use_part_table(part_table(29))`, HGATE); a gather table (e.g. `part_table(29)`, 64 slots) returns that layout
    (WindowCreate, for a model without a part table).

    Everything a batch needs (per-clip parameters, frame maps, mask bytes, labels, the packed clips) is written into one
    pinned staging buffer and uploaded with one copy on a side stream; the kernels run on the stream that is current at
    the call.  Slot reuse follows `collate.PinnedBatcher`: at the start of every call an event recorded on the consumer
    stream covers what was enqueued since the previous call (that call's kernels and the step that read its batch);
    a slot's device buffer is overwritten only after the event recorded one call after the slot was handed out, and its
    pinned buffer only after its previous upload finished.  Call it from the thread that enqueues the training step."""

    def __init__(self, batch_size: int, max_frames: int, device, out_joints=None, depth: int = 2):
        if depth < 2:
            raise ValueError("depth >= 2 (double buffering)")
        if not 0 < max_frames <= MAX_FRAMES:
            raise ValueError(f"max_frames in [1, {MAX_FRAMES}]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("AugmentBatcher runs the transform on an MI355X device; there is no CPU fallback")
        self.batch_size, self.max_frames, self.depth = batch_size, max_frames, depth
        self.gather = None
        if out_joints is not None:
            g = torch.as_tensor(out_joints, dtype=torch.int32).reshape(-1)
            self._gather_max = int(g.max())
            if int(g.min()) < 0:
                raise ValueError("gather table entries must be non-negative joint indices")
            self.gather = g.to(self.device)
        self._cap = 0
        self._host = [None] * depth
        self._dev = [None] * depth
        self._stream = torch.cuda.Stream(self.device)
        self._ready = [None] * depth
        self._consumed = [None] * depth
        self._slot = 0
        self._last = None

    def _layout(self, n, src_len, total, J, C):
        o, lay = 0, {}
        for name, nbytes in (("prm", n * NPRM * 8), ("off", (n + 1) * 4), ("src", n * src_len * 4), ("y", n * 8),
                             ("mask", total), ("x", total * J * C * 4)):
            lay[name] = (o, nbytes)
            o = _align(o + nbytes)
        return lay, o

    def _ensure(self, nbytes, src_len, J, C):
        if nbytes <= self._cap:
            return
        # size for a full batch of max_frames clips (grows only if a later batch has a longer src_len / more joints)
        _, cap = self._layout(self.batch_size, src_len, self.batch_size * self.max_frames, J, C)
        cap = max(cap, nbytes)
        torch.cuda.synchronize(self.device)        # nothing in flight reads the old buffers
        self._host = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(self.depth)]
        self._dev = [torch.empty(cap, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self._ready = [None] * self.depth
        self._consumed = [None] * self.depth
        self._last = None
        self._cap = cap

    def __call__(self, samples: Sequence):
        n = len(samples)
        if not 0 < n <= self.batch_size:
            raise ValueError(f"batch of {n} clips (staging holds 1..{self.batch_size})")
        clips = [np.asarray(s[0], dtype=np.float32) for s in samples]
        recs = [s[2] for s in samples]
        J, C = clips[0].shape[1], clips[0].shape[2]
        src_len, hands = len(recs[0].src), recs[0].hands
        for clip, rec in zip(clips, recs):
            if clip.ndim != 3 or clip.shape[1:] != (J, C) or clip.shape[0] != rec.T:
                raise ValueError(f"clip {clip.shape} does not match its record (T={rec.T}) or the batch's (J, C)")
            if len(rec.src) != src_len or rec.hands != hands:
                raise ValueError("all records of a batch must come from one transform (src_len, hand slices)")
            if rec.T > self.max_frames:
                raise ValueError(f"clip of {rec.T} raw frames > max_frames {self.max_frames}")
        if self.gather is not None and self._gather_max >= J:
            raise ValueError(f"gather table names joint {self._gather_max}, clips have {J}")
        lengths = np.array([r.T for r in recs], dtype=np.int64)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lengths, out=off[1:])
        total = int(off[-1])
        lay, nbytes = self._layout(n, src_len, total, J, C)
        self._ensure(nbytes, src_len, J, C)

        s = self._slot
        self._slot = (s + 1) % self.depth
        cur = torch.cuda.current_stream(self.device)
        if self._last is not None:
            ev = torch.cuda.Event()               # covers the kernels + step that consumed the previous call's slot
            ev.record(cur)
            self._consumed[self._last] = ev
        if self._ready[s] is not None:
            self._ready[s].synchronize()          # the previous upload FROM this pinned buffer has finished
        hb = self._host[s].numpy()

        def view(name, dtype, shape):
            o, nb = lay[name]
            return hb[o:o + nb].view(dtype).reshape(shape)

        prm = view("prm", np.float64, (n, NPRM))
        view("off", np.int32, (n + 1,))[:] = off
        srcv = view("src", np.int32, (n, src_len))
        yv = view("y", np.int64, (n,))
        mask = view("mask", np.uint8, (total,))
        xv = view("x", np.float32, (total, J, C))
        mask[:] = 0
        for i, (clip, rec) in enumerate(zip(clips, recs)):
            a = int(off[i])
            _params(rec, prm[i])
            srcv[i] = rec.src
            yv[i] = int(samples[i][1])
            mask[a + rec.masked] = 1
            xv[a:a + rec.T] = clip
        self._last = s
        dev = self._dev[s]
        if self._consumed[s] is not None:
            self._stream.wait_event(self._consumed[s])      # the kernels / step that read this device buffer are done
        with torch.cuda.stream(self._stream):
            dev[:nbytes].copy_(self._host[s][:nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._ready[s] = ev
        cur.wait_event(ev)

        base = dev.data_ptr()
        p = {k: base + o for k, (o, _) in lay.items()}
        has_mask = any(len(r.masked) for r in recs)
        lib = _lib.lib()
        ws = torch.empty(int(lib.hwgat_aug_hand_fill_ws_bytes(total)), dtype=torch.uint8, device=self.device)
        st = cur.cuda_stream
        _lib.call("hwgat_aug_hand_fill", p["x"], p["off"], p["mask"] if has_mask else None, n, total,
                  int(lengths.max()), J, C, ctypes_int32_6(*hands), ws.data_ptr(), ws.numel(), None, st)
        J_out = J if self.gather is None else self.gather.numel()
        x = torch.empty((n, src_len, J_out, C), dtype=torch.float32, device=self.device)
        _lib.call("hwgat_aug_resample", p["x"], p["off"], p["src"], p["prm"], _lib.ptr(self.gather), x.data_ptr(), n,
                  src_len, J, J_out, C, st)
        o, nb = lay["y"]
        y = dev[o:o + nb].view(torch.int64).clone()
        return x, y
