"""Device-resident clip store and in-graph train input pipeline (csrc/loader.hip).

`augment.AugmentBatcher` takes raw clips and `AugRecord`s that DataLoader workers drew on the CPU, packs them in a Python
loop over the batch and uploads them: nothing about a batch is known to the device until the host has built it.  Keypoint
datasets are small (tens of thousands of clips of ~100 frames x 29-67 joints: a GB or two), so here the whole dataset is
uploaded once (`DeviceClipStore`) and "the next batch" is four launches with no host input (`DeviceLoader`):

    hwgat_loader_select   the batch's clip ids (a keyed Feistel permutation of the epoch), labels, lengths, offsets
    hwgat_loader_draw     the raw frames into the packed batch, the masked frames, the augmentation record, the frame map
    hwgat_aug_hand_fill   } the kernels AugmentBatcher runs, unchanged
    hwgat_aug_resample    }

Seed, epoch and cursor are device words, so the four launches replay as one HIP graph (`graph=True`).  The draw has the
distributions of `TrainTransform.draw` (the reference's train transform) but its own counter-based random numbers, keyed by
(seed, epoch, clip id): clip i in epoch e gets the same augmentation however it is batched or split over ranks.  The
formulas are in include/hwgat_hip.h; tests/loader_helpers.py restates them in numpy.

    store = data.DeviceClipStore(clips, labels, dev, augment.TrainTransform(src_len))
    loader = data.DeviceLoader(store, 64, seed=1, graph=True)
    step = train.GraphedTrainStep(model, opt, x0, y0, ragged=True)
    loader.bind(step.x, step.y)                       # the loader writes the step's own buffers: no copy
    for epoch in range(epochs):
        for x, y in loader:
            step(x, y)
"""
import numbers

import numpy as np
import torch

from . import _lib
from . import augment
from . import functional as HF

# hwgat_loader_state of include/hwgat_hip.h as numpy sees it
LOADER_STATE = np.dtype([("seed", "<u4"), ("epoch", "<u4"), ("cursor", "<i4"), ("n_clips", "<i4"), ("batch", "<i4"),
                         ("rank", "<i4"), ("world", "<i4"), ("flags", "<i4"), ("spare", "<i8", (4,))])
assert LOADER_STATE.itemsize == 8 * HF.LOADER_STATE_WORDS
MAX_CLIPS, MAX_WORLD = 1 << 30, 1 << 20
_CHUNK_BYTES = 32 << 20


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _same_geometry(a, b):
    return a.hands == b.hands and list(a.norm_idx) == list(b.norm_idx)


def _check_train_lengths(transform, lengths, first=0):
    """what TrainTransform.draw refuses per clip, for every length at once; the index of the clip is named"""
    if not isinstance(transform, augment.TrainTransform):
        return
    p, (lo, hi) = transform.sampling_prob, transform.frame_augmentation
    if not (0.0 < p < 1.0) or not (0.0 < lo <= hi <= 2.0) or transform.shear_std < 0 or transform.rotation_std < 0:
        raise ValueError("the device draw takes 0 < sampling_prob < 1, 0 < frame_augmentation[0] <= [1] <= 2 and "
                         "non-negative standard deviations")
    for i, T in enumerate(lengths):
        T = int(T)
        if int(p * T) == 0:
            raise ValueError(f"clip {first + i}: clip of {T} raw frames: KeypointMasking masks int({p} * T) = 0 frames "
                             f"(the reference raises IndexError); train clips need at least {int(np.ceil(1 / p))} frames")
        if int(T * lo) < 1:
            raise ValueError(f"clip {first + i}: clip of {T} raw frames: TemporalAugmentation keeps int(T * {lo}) = 0 frames")


class DeviceClipStore:
    """All raw clips of a dataset in device memory: `frames` (total_frames, J, C) fp32 one clip after another, `clip_off`
    (n + 1) int64, `labels` (n) int64 and `norm` (n, 4) fp32 = NormalizeKeypoints' left_top[0..2], edge_dist, computed once
    on the host by the transform's `_normalisation` (the origin and anchor joints are never masked or hand-corrected, so the
    raw clip decides, and the device record has the host's bits).

    `clips`: a sequence of raw (T, J, C) arrays, all with the same (J, C); `transform`: an `augment.TrainTransform` or
    `EvalTransform` -- it supplies the hand slices, the normalisation joints, `src_len` and the distribution parameters, and
    is the default transform of the loaders built on the store.  Everything `transform.draw` refuses per clip is refused
    here once, with the same `ValueError`s and the clip's index in front.  The clips go up in chunks through two pinned
    buffers.  `nbytes`: device bytes held; `len(store)`: clips; `max_frames`: the longest clip."""

    @staticmethod
    def check(clips, labels, transform):
        """the host half: (lengths (n) int64, labels (n) int64, norm (n, 4) float32, J, C), or a ValueError"""
        if not isinstance(transform, (augment.TrainTransform, augment.EvalTransform)):
            raise ValueError("transform must be an augment.TrainTransform or augment.EvalTransform")
        n = len(clips)
        if n == 0 or n > MAX_CLIPS:
            raise ValueError(f"a store holds 1 to {MAX_CLIPS} clips, got {n}")
        if len(labels) != n:
            raise ValueError(f"{n} clips but {len(labels)} labels")
        lab = np.asarray(labels)
        if lab.ndim != 1 or lab.dtype.kind not in "iu":
            raise ValueError(f"labels must be {n} integers, got {lab.dtype} {lab.shape}")
        lengths = np.zeros(n, dtype=np.int64)
        norm = np.zeros((n, 4), dtype=np.float32)
        J = C = None
        for i, clip in enumerate(clips):
            try:
                c = transform._check(clip)
                if c.shape[0] < 1:
                    raise ValueError("a clip needs at least one frame")
                if J is None:
                    J, C = c.shape[1], c.shape[2]
                elif c.shape[1:] != (J, C):
                    raise ValueError(f"clip {c.shape} does not match the store's (J, C) = ({J}, {C})")
                left_top, edge = transform._normalisation(c)
            except ValueError as e:
                raise ValueError(f"clip {i}: {e}") from None
            lengths[i] = c.shape[0]
            norm[i, :C] = left_top
            norm[i, 3] = edge
        if max(transform.norm_idx + [transform.hands[2], transform.hands[5]]) >= J:
            raise ValueError(f"clips of {J} joints do not hold the wrists and the origin / anchor joints")
        _check_train_lengths(transform, lengths)
        return lengths, lab.astype(np.int64), norm, J, C

    def __init__(self, clips, labels, device, transform):
        lengths, lab, norm, J, C = self.check(clips, labels, transform)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceClipStore keeps the clips on an MI355X device; there is no CPU fallback")
        self.transform, self.joints, self.coords = transform, J, C
        self.lengths = lengths
        self.max_frames = int(lengths.max())
        off = np.zeros(len(lengths) + 1, dtype=np.int64)
        np.cumsum(lengths, out=off[1:])
        self.total_frames = int(off[-1])
        self.frames = torch.empty((self.total_frames, J, C), dtype=torch.float32, device=self.device)
        self.clip_off = torch.from_numpy(off).to(self.device)
        self.labels = torch.from_numpy(lab).to(self.device)
        self.norm = torch.from_numpy(norm).to(self.device)
        self._upload(clips, off)

    def _upload(self, clips, off):
        """clips -> frames in chunks of whole clips through two pinned buffers used in turn"""
        row = self.joints * self.coords
        cap = max(_CHUNK_BYTES // (4 * row), self.max_frames)             # frames per chunk
        pinned = [torch.empty((cap, self.joints, self.coords), dtype=torch.float32, pin_memory=True) for _ in range(2)]
        done = [None, None]
        flat = self.frames
        i, slot, n = 0, 0, len(clips)
        while i < n:
            j = i
            while j < n and off[j + 1] - off[i] <= cap:
                j += 1
            if done[slot] is not None:
                done[slot].synchronize()                                  # the copy that last read this pinned buffer
            hb = pinned[slot].numpy()
            for k in range(i, j):
                hb[off[k] - off[i]:off[k + 1] - off[i]] = np.asarray(clips[k], dtype=np.float32)
            flat[off[i]:off[j]].copy_(pinned[slot][:off[j] - off[i]], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            done[slot] = ev
            i, slot = j, 1 - slot
        for ev in done:
            if ev is not None:
                ev.synchronize()

    def __len__(self):
        return len(self.lengths)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.frames, self.clip_off, self.labels, self.norm))


class DeviceLoader:
    """(x, y) train or eval batches from a `DeviceClipStore` with no host input per batch.

    `transform`: default the store's; another one (say an `EvalTransform` on a store built with a `TrainTransform`) must
    have the store's hand slices and normalisation joints.  A `TrainTransform` draws (masking, shear, rotation, temporal
    augmentation, flip); an `EvalTransform` draws nothing.  `shuffle`: a new keyed permutation of the clips per epoch;
    `drop_last`: only full batches; `rank` / `world`: sample s of the epoch's order goes to rank s % world; every rank has
    the same number of batches.  `out_joints`: the gather table, as in `AugmentBatcher`.

    `len(loader)`: batches per epoch.  `for x, y in loader` runs from the current cursor to the epoch's end and yields the
    loader's STATIC buffers `x` (B, src_len, J_out, C) fp32 and `y` (B,) int64 -- for a short last batch the views `x[:n]`,
    `y[:n]`; the rows behind are zeros with label 0; a batch without any row (a rank's share can end early) is not yielded.
    The host mirrors the cursor, so it knows n without a read-back; `n_rows` is the device word.  `graph=True` captures the
    four launches once, at the first batch (warm-up on a side stream); each batch is then one replay.  `bind(x, y)` makes
    the loader write caller-owned buffers -- `step.x, step.y` of a `GraphedTrainStep`, whose `__call__` then sees its own
    `data_ptr` and copies nothing; bind before the first batch of a graphed loader.  `records()` reads back the last
    batch's ids, masked frames, frame maps and parameter records.  `state_dict()` / `load_state_dict()` carry seed, epoch
    and cursor: a resumed run continues the same sequence.  Kernels run on the current stream; use one stream, one
    thread."""

    @staticmethod
    def check(n_clips, batch_size, shuffle, drop_last, seed, rank, world):
        """the argument checks, without a device: batches per epoch"""
        if not _is_int(batch_size) or not 1 <= batch_size <= HF.LOADER_MAX_BATCH:
            raise ValueError(f"batch_size in [1, {HF.LOADER_MAX_BATCH}], got {batch_size!r}")
        if not _is_int(world) or not 1 <= world <= MAX_WORLD or not _is_int(rank) or not 0 <= rank < world:
            raise ValueError(f"world in [1, {MAX_WORLD}] and rank in [0, world), got rank {rank!r} of {world!r}")
        if not _is_int(seed) or not 0 <= seed < 1 << 32:
            raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
        per = n_clips // world if drop_last else -(-n_clips // world)
        nb = per // batch_size if drop_last else -(-per // batch_size)
        if nb < 1:
            raise ValueError(f"{n_clips} clips over {world} ranks give no full batch of {batch_size} (drop_last)")
        return nb

    def __init__(self, store, batch_size, transform=None, shuffle=True, drop_last=False, seed=0, rank=0, world=1,
                 out_joints=None, graph=False):
        if not isinstance(store, DeviceClipStore):
            raise ValueError("store must be a data.DeviceClipStore")
        tf = store.transform if transform is None else transform
        if not isinstance(tf, (augment.TrainTransform, augment.EvalTransform)):
            raise ValueError("transform must be an augment.TrainTransform or augment.EvalTransform")
        if not _same_geometry(tf, store.transform):
            raise ValueError("the loader's transform must have the store's hand slices and normalisation joints")
        if tf is not store.transform:
            _check_train_lengths(tf, store.lengths)
        self._nb = self.check(len(store), batch_size, shuffle, drop_last, seed, rank, world)
        self.store, self.transform, self.batch_size = store, tf, int(batch_size)
        self.train = isinstance(tf, augment.TrainTransform)
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        self.src_len = int(tf.src_len)
        dev, B, J, C, Tm = store.device, self.batch_size, store.joints, store.coords, store.max_frames
        if B * Tm >= (1 << 31) - 1:
            raise ValueError(f"batch_size * max_frames = {B * Tm} does not fit the packed batch's int32 offsets")
        self.device = dev
        self._gather = None
        if out_joints is not None:
            g = torch.as_tensor(out_joints, dtype=torch.int32).reshape(-1)
            if int(g.min()) < 0 or int(g.max()) >= J:
                raise ValueError(f"gather table entries must be joint indices in [0, {J})")
            self._gather = g.to(dev)
        self.out_joints = J if self._gather is None else self._gather.numel()
        self._limit = self._nb * B * self.world if self.drop_last else len(store)
        self._seed, self._epoch, self._cursor = int(seed), 0, 0
        self._last_n = 0
        # static device buffers: everything a batch reads or writes
        self.state = torch.zeros(HF.LOADER_STATE_WORDS, dtype=torch.int64, device=dev)
        self.ids = torch.zeros(B, dtype=torch.int32, device=dev)
        self.keys = torch.zeros(B, dtype=torch.int32, device=dev)
        self.clip_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.batch_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        self.n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
        self.clip = torch.zeros((B * Tm, J, C), dtype=torch.float32, device=dev)
        self.masked = torch.zeros(B * Tm, dtype=torch.uint8, device=dev)
        self.frame_map = torch.zeros((B, self.src_len), dtype=torch.int32, device=dev)
        self.params = torch.zeros((B, augment.NPRM), dtype=torch.float64, device=dev)
        self._ws = torch.empty(int(_lib.lib().hwgat_aug_hand_fill_ws_bytes(B * Tm)), dtype=torch.uint8, device=dev)
        self._hv = augment.ctypes_int32_6(*tf.hands)
        self.x = torch.zeros((B, self.src_len, self.out_joints, C), dtype=torch.float32, device=dev)
        self.y = torch.zeros(B, dtype=torch.int64, device=dev)
        self.want_graph, self.graph = bool(graph), None
        self._launched = False
        self._write_state()

    # ------------------------------------------------------------ state words
    def _write_state(self):
        rec = np.zeros(1, dtype=LOADER_STATE)
        rec["seed"], rec["epoch"], rec["cursor"] = self._seed, self._epoch & 0xFFFFFFFF, self._cursor
        rec["n_clips"], rec["batch"], rec["rank"], rec["world"] = len(self.store), self.batch_size, self.rank, self.world
        rec["flags"] = (HF.LOADER_SHUFFLE if self.shuffle else 0) | (HF.LOADER_DROP_LAST if self.drop_last else 0) | \
            (HF.LOADER_TRAIN if self.train else 0)
        self.state.copy_(torch.from_numpy(rec.view(np.int64).copy()))

    def state_dict(self):
        return {"seed": self._seed, "epoch": self._epoch, "cursor": self._cursor}

    def load_state_dict(self, sd):
        seed, epoch, cursor = int(sd["seed"]), int(sd["epoch"]), int(sd["cursor"])
        if not 0 <= seed < 1 << 32 or epoch < 0 or not 0 <= cursor < self._nb:
            raise ValueError(f"seed in [0, 2^32), epoch >= 0 and cursor in [0, {self._nb}), got {sd!r}")
        self._seed, self._epoch, self._cursor = seed, epoch, cursor
        self._write_state()

    @property
    def epoch(self):
        return self._epoch

    @property
    def cursor(self):
        return self._cursor

    def __len__(self):
        return self._nb

    def rows_of(self, cursor):
        """real rows of batch `cursor` of an epoch on this rank (host arithmetic, the kernel's rule)"""
        first = cursor * self.batch_size * self.world + self.rank          # the sample of row 0; row r adds r * world
        return int(min(max(-(-(self._limit - first) // self.world), 0), self.batch_size))

    # ------------------------------------------------------------ the launches
    def bind(self, x, y):
        """write into the caller's buffers from now on: x (B, src_len, J_out, C) fp32 and y (B,) int64 on the loader's device"""
        if self.graph is not None:
            raise RuntimeError("the loader's graph holds the addresses of its buffers: bind before the first batch")
        if x.dtype != torch.float32 or tuple(x.shape) != tuple(self.x.shape) or x.device != self.x.device or \
                not x.is_contiguous():
            raise ValueError(f"x must be a contiguous fp32 {tuple(self.x.shape)} tensor on {self.x.device}, got {x.dtype} "
                             f"{tuple(x.shape)} on {x.device}")
        if y.dtype != torch.int64 or tuple(y.shape) != tuple(self.y.shape) or y.device != self.y.device or \
                not y.is_contiguous():
            raise ValueError(f"y must be a contiguous int64 {tuple(self.y.shape)} tensor on {self.y.device}")
        self.x, self.y = x, y

    def _launch(self):
        st, tf, B, Tm = self.store, self.transform, self.batch_size, self.store.max_frames
        HF.loader_select(self.state, st.frames, st.clip_off, st.labels, self.ids, self.keys, self.clip_len, self.batch_off,
                         self.y, self.n_rows, Tm)
        if self.train:
            dist = (tf.sampling_prob, tf.frame_augmentation, tf.shear_std, tf.rotation_std, tf.random_sample, tf.random_shift)
        else:
            dist = (0.5, (1.0, 1.0), 0.0, 0.0, False, False)              # never read: the state's train flag is off
        HF.loader_draw(self.state, st.frames, st.clip_off, st.norm, self.ids, self.keys, self.batch_off, self.clip,
                       self.masked, self.frame_map, self.params, Tm, *dist)
        HF.call("hwgat_aug_hand_fill", _lib.ptr(self.clip), _lib.ptr(self.batch_off), _lib.ptr(self.masked), B, B * Tm, Tm,
                st.joints, st.coords, self._hv, _lib.ptr(self._ws), self._ws.numel(), None, _lib.stream())
        HF.call("hwgat_aug_resample", _lib.ptr(self.clip), _lib.ptr(self.batch_off), _lib.ptr(self.frame_map),
                _lib.ptr(self.params), _lib.ptr(self._gather), _lib.ptr(self.x), B, self.src_len, st.joints, self.out_joints,
                st.coords, _lib.stream())

    def _capture(self):
        dev = self.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                         # warm-up off the default stream, as torch.cuda.graphs asks
            self._launch()
        torch.cuda.current_stream(dev).wait_stream(side)
        self._write_state()                                   # the warm-up moved the cursor: back to the mirror's
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._launch()

    def next_batch(self):
        """launch the next batch into `x` / `y`; returns its real row count (host arithmetic).  Synchronises nothing"""
        if self.want_graph:
            if self.graph is None:
                self._capture()
            self.graph.replay()
        else:
            self._launch()
        self._launched = True
        n = self.rows_of(self._cursor)
        self._cursor += 1
        if self._cursor >= self._nb:
            self._cursor, self._epoch = 0, self._epoch + 1
        self._last_n = n
        return n

    def __iter__(self):
        while True:
            n = self.next_batch()
            if n == self.batch_size:
                yield self.x, self.y
            elif n > 0:
                yield self.x[:n], self.y[:n]
            if self._cursor == 0:
                return

    # ------------------------------------------------------------ read-back
    def records(self):
        """ONE synchronising read of the last batch: {"n_rows", "ids" (B), "y" (B), "clip_len" (B), "batch_off" (B + 1),
        "keys" (B) uint32, "masked": per row the sorted masked frames, "src" (B, src_len), "prm" (B, 24)} as numpy"""
        if not self._launched:
            raise RuntimeError("no batch has been launched yet")
        off = self.batch_off.cpu().numpy()
        msk = self.masked.cpu().numpy()
        B = self.batch_size
        return {"n_rows": int(self.n_rows.item()), "ids": self.ids.cpu().numpy(), "y": self.y.cpu().numpy(),
                "clip_len": self.clip_len.cpu().numpy(), "batch_off": off,
                "keys": self.keys.cpu().numpy().view(np.uint32),
                "masked": [np.flatnonzero(msk[off[r]:off[r + 1]]).astype(np.int64) for r in range(B)],
                "src": self.frame_map.cpu().numpy(), "prm": self.params.cpu().numpy()}
