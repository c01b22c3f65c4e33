"""CPU: the host side of streaming recognition (csrc/stream.hip, serve.StreamRecognizer, GraphedEval's `head`) -- the entry
points in the header, the binding and the library, the records of the state block, the argument checks of every entry point
before any HIP call, and what the recogniser refuses before it looks at a device."""
import ctypes
import importlib
import inspect
import re

import numpy as np
import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
serve = importlib.import_module("sl-hwgat_amd.serve")
HF = hw.functional
CPU = torch.device("cpu")
STREAM_SYMBOLS = {"hwgat_stream_state_bytes", "hwgat_stream_push", "hwgat_stream_window", "hwgat_stream_decide"}
HANDS = (ctypes.c_int32 * 6)(9, 19, 7, 19, 29, 8)
EINVAL, ESHAPE = -1, -2


def _model(train=False):
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 7}, 2, CPU, num_kps=64)
    m = hw.Model(*hp.get_model_params()).use_part_table(hw.part_table(29))
    return m.train() if train else m.eval()


def _buf():
    """aligned host memory standing in for a device pointer: never dereferenced, every call below is refused first"""
    keep = (ctypes.c_double * 64)()
    return keep, ctypes.cast(keep, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ header, binding, library
def test_symbols_abi_and_records_follow_the_header():
    assert STREAM_SYMBOLS <= set(hw._lib.declared_symbols())
    assert STREAM_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_stream_")}
    L = hw._lib.lib()
    for name in STREAM_SYMBOLS:
        assert getattr(L, name) is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    assert int(re.search(r"#define\s+HWGAT_STREAM_MAX_STREAMS\s+(\d+)", src).group(1)) == HF.STREAM_MAX_STREAMS == 64
    assert int(re.search(r"#define\s+HWGAT_STREAM_MAX_CLASSES\s+(\d+)", src).group(1)) == HF.STREAM_MAX_CLASSES
    assert re.search(r"#define\s+HWGAT_STREAM_MAX_LOG\s+\(1 << 20\)", src) and HF.STREAM_MAX_LOG == 1 << 20
    assert int(re.search(r"#define\s+HWGAT_AUG_MAX_FRAMES\s+(\d+)", src).group(1)) == HF.STREAM_MAX_FRAMES
    assert int(re.search(r"#define\s+HWGAT_AUG_NPRM\s+(\d+)", src).group(1)) == HF.STREAM_NPRM
    # the numpy records name the fields of the C records, in order
    ctype = {"int32_t": "<i4", "int64_t": "<i8", "float": "<f4"}
    for struct, dt in (("hwgat_stream_header", serve.STREAM_HEADER), ("hwgat_stream_words", serve.STREAM_WORDS),
                       ("hwgat_stream_event", serve.STREAM_EVENT)):
        body = re.search(r"typedef struct \{([^{}]*)\} " + struct + ";", src).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for typ, names in re.findall(r"(int32_t|int64_t|float)\s+([^;]+);", body):
            for name in names.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name.strip())
                fields.append((m.group(1), ctype[typ]) + (((int(m.group(2)),),) if m.group(2) else ()))
        assert np.dtype(fields) == dt, struct
    assert (serve.STREAM_HEADER.itemsize, serve.STREAM_WORDS.itemsize, serve.STREAM_EVENT.itemsize) == (64, 64, 32)
    assert (HF.STREAM_HEADER_WORDS, HF.STREAM_WORDS, HF.STREAM_EVENT_WORDS) == (8, 8, 4)


def test_state_size_follows_the_layout():
    L = hw._lib.lib()
    for S, cap in ((1, 0), (3, 5), (64, 1024), (8, 1 << 20)):
        assert L.hwgat_stream_state_bytes(S, cap) == 64 + 64 * S + 32 * cap
        assert HF.stream_state_words(S, cap) * 8 == 64 + 64 * S + 32 * cap
    for S, cap in ((0, 4), (-1, 4), (65, 4), (3, -1), (3, (1 << 20) + 1)):
        assert L.hwgat_stream_state_bytes(S, cap) == EINVAL
        with pytest.raises(ValueError, match="no stream state"):
            HF.stream_state_words(S, cap)


def test_every_entry_point_checks_its_arguments_without_launching():
    L = hw._lib.lib()
    keep, buf = _buf()
    odd = ctypes.c_void_p(buf.value + 4)
    push, window, decide = L.hwgat_stream_push, L.hwgat_stream_window, L.hwgat_stream_decide
    # (ring, state, frames, n_new, S, R, F, J, C, stream)
    good = [buf, buf, buf, buf, 3, 32, 5, 29, 2, None]
    for i in range(4):                                        # null pointers
        assert push(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    assert push(*(good[:1] + [odd] + good[2:])) == EINVAL      # the state holds 8-byte words
    for i, bad, rc in ((4, 0, EINVAL), (4, -1, EINVAL), (4, 65, ESHAPE), (5, 0, EINVAL), (5, 4097, ESHAPE),
                       (6, 0, EINVAL), (6, 33, ESHAPE),       # F > R: a push would overwrite itself
                       (7, 0, EINVAL), (7, 1025, ESHAPE), (8, 1, ESHAPE), (8, 4, ESHAPE)):
        assert push(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    # (ring, state, clip, clip_off, src, prm, S, R, Wf, min_frames, src_len, J, C, origin, a0, a1, hands, stream)
    good = [buf, buf, buf, buf, buf, buf, 3, 32, 24, 1, 16, 29, 2, 0, 3, 4, HANDS, None]
    for i in (0, 1, 2, 3, 4, 5, 16):
        assert window(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    assert window(*(good[:1] + [odd] + good[2:])) == EINVAL
    assert window(*(good[:5] + [odd] + good[6:])) == EINVAL    # fp64 records
    for i, bad, rc in ((6, 0, EINVAL), (6, 65, ESHAPE), (7, 0, EINVAL), (7, 4097, ESHAPE), (8, 0, EINVAL),
                       (8, 33, ESHAPE),                       # Wf > R
                       (9, 0, EINVAL), (10, 0, EINVAL), (11, 0, EINVAL), (12, 4, ESHAPE),
                       (13, -1, ESHAPE), (13, 29, ESHAPE), (13, 9, ESHAPE),      # the origin: outside the frame, in a hand
                       (14, 28, ESHAPE), (15, 19, ESHAPE), (15, 30, ESHAPE)):
        assert window(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    assert window(*(good[:11] + [20] + good[12:])) == ESHAPE   # the hands do not fit a frame of 20 joints
    # (state, q, logits, S, N, log_capacity, stream)
    good = [buf, buf, buf, 3, 7, 16, None]
    for i in range(3):
        assert decide(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    assert decide(*([odd] + good[1:])) == EINVAL
    for i, bad, rc in ((3, 0, EINVAL), (3, 65, ESHAPE), (4, 0, EINVAL), (4, 65537, ESHAPE), (5, -1, EINVAL),
                       (5, (1 << 20) + 1, ESHAPE)):
        assert decide(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    del keep


def test_wrappers_refuse_cpu_tensors_and_wrong_buffers():
    S, R, F, J, C, N = 3, 32, 5, 29, 2, 7
    ring = torch.zeros(S, R, J, C)
    state = torch.zeros(HF.stream_state_words(S, 4), dtype=torch.int64)
    frames, n_new = torch.zeros(S, F, J, C), torch.zeros(S, dtype=torch.int32)
    clip, off = torch.zeros(S * 24, J, C), torch.zeros(S + 1, dtype=torch.int32)
    src, prm = torch.zeros(S, 16, dtype=torch.int32), torch.zeros(S, 24, dtype=torch.float64)
    q, z = torch.zeros(S, N), torch.zeros(S, N)
    hands = (9, 19, 7, 19, 29, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.stream_push(ring, state, frames, n_new)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.stream_window(ring, state, clip, off, src, prm, 24, 1, 0, (3, 4), hands)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.stream_decide(state, q, z, 4)
    with pytest.raises(ValueError, match="ring"):
        HF.stream_push(ring.double(), state, frames, n_new)
    with pytest.raises(ValueError, match="stream state"):
        HF.stream_push(ring, state[:8], frames, n_new)
    with pytest.raises(ValueError, match="frames"):
        HF.stream_push(ring, state, frames[:, :, :28], n_new)
    with pytest.raises(ValueError, match="n_new"):
        HF.stream_push(ring, state, frames, n_new.long())
    with pytest.raises(ValueError, match="clip buffer"):
        HF.stream_window(ring, state, clip[:10], off, src, prm, 24, 1, 0, (3, 4), hands)
    with pytest.raises(ValueError, match="clip_off"):
        HF.stream_window(ring, state, clip, off[:S], src, prm, 24, 1, 0, (3, 4), hands)
    with pytest.raises(ValueError, match="frame map"):
        HF.stream_window(ring, state, clip, off, src.long(), prm, 24, 1, 0, (3, 4), hands)
    with pytest.raises(ValueError, match="parameter records"):
        HF.stream_window(ring, state, clip, off, src, prm.float(), 24, 1, 0, (3, 4), hands)
    with pytest.raises(ValueError, match="logits"):
        HF.stream_decide(state, q, z.double(), 4)
    with pytest.raises(ValueError, match="q must"):
        HF.stream_decide(state, q[:, :5], z, 4)
    with pytest.raises(ValueError, match="stream state"):
        HF.stream_decide(state, q, z, 5)


# ------------------------------------------------------------------------------------------ the recogniser on the host
def test_recognizer_refuses_before_any_device_work():
    kw = dict(n_streams=3, window_frames=24, ring_frames=32, push_frames=5)
    with pytest.raises(ValueError, match=r"model\.eval\(\)"):
        serve.StreamRecognizer(_model(train=True), **kw)
    model = _model()
    with pytest.raises(ValueError, match="must live on the GPU"):
        serve.StreamRecognizer(model, **kw)
    # hand slices and anchors: the messages of augment._Base
    with pytest.raises(ValueError, match="hand slices: left"):
        serve.StreamRecognizer(model, hands=(19, 29, 7, 9, 19, 8), **kw)
    with pytest.raises(ValueError, match="hand slices: left"):
        serve.StreamRecognizer(model, hands=(9, 19, 12, 19, 29, 8), **kw)
    with pytest.raises(ValueError, match="the hands must be adjacent"):
        serve.StreamRecognizer(model, hands=(9, 18, 7, 19, 29, 8), **kw)
    with pytest.raises(ValueError, match="exactly two anchor points"):
        serve.StreamRecognizer(model, anchor_points=(3, 4, 5), **kw)
    with pytest.raises(ValueError, match="origin / anchor joints must lie outside the hands"):
        serve.StreamRecognizer(model, anchor_points=(3, 12), **kw)
    with pytest.raises(ValueError, match="origin / anchor joints must lie outside the hands"):
        serve.StreamRecognizer(model, origin_idx=20, **kw)
    with pytest.raises(ValueError, match="hands:"):
        serve.StreamRecognizer(model, hands=(9, 19, 7), **kw)
    for bad in (dict(n_streams=0), dict(n_streams=65), dict(ring_frames=4097), dict(window_frames=33), dict(push_frames=33),
                dict(window_frames=0), dict(push_frames=0)):
        with pytest.raises(ValueError, match="in \\["):
            serve.StreamRecognizer(model, **dict(kw, **bad))
    for bad in (dict(coords=4), dict(joints=28), dict(anchor_points=(3, 29)), dict(min_frames=0), dict(log_capacity=-1),
                dict(alpha=1.5), dict(hold=0), dict(hold=2.5), dict(blank_class=-2)):
        with pytest.raises(ValueError):
            serve.StreamRecognizer(model, **dict(kw, **bad))


def test_counts_are_checked_on_the_host():
    check = serve.StreamRecognizer.check_counts
    got = check([0, 5, 3], 3, 5)
    assert got.dtype == np.int32 and got.tolist() == [0, 5, 3]
    assert check(torch.tensor([1, 2, 0]), 3, 5).tolist() == [1, 2, 0]
    assert check(np.array([5, 5, 5], dtype=np.int64), 3, 5).tolist() == [5, 5, 5]
    for bad in ([0, 6, 1], [-1, 0, 0], np.array([0, 1 << 40, 0])):
        with pytest.raises(ValueError, match=r"lie in \[0, 5\]"):
            check(bad, 3, 5)
    for bad in ([0, 1], [[0, 1, 2]], [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError, match="counts must hold 3 integers"):
            check(bad, 3, 5)


def test_graphed_eval_takes_a_head_that_defaults_to_none():
    sig = inspect.signature(serve.GraphedEval.__init__)
    assert list(sig.parameters) == ["self", "model", "example", "warmup", "tail", "graph", "head"]
    assert sig.parameters["head"].default is None and sig.parameters["tail"].default is None
    assert list(inspect.signature(serve.StreamRecognizer.__init__).parameters) == [
        "self", "model", "n_streams", "window_frames", "ring_frames", "push_frames", "joints", "coords", "out_joints",
        "min_frames", "alpha", "threshold", "hold", "blank_class", "log_capacity", "hands", "origin_idx", "anchor_points", "graph"]
