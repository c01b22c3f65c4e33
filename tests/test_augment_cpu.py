"""CPU: host half of the device-side transforms (sl-hwgat_amd/augment.py) against the reference's fixtures.

`TrainTransform.draw` / `EvalTransform.draw` must consume the RNG exactly as the reference's Compose does, and the
drawn records, applied by a test-local numpy + scipy restatement, must reproduce the reference's outputs."""
import hashlib
import importlib
import pickle
import random

import numpy as np
import pytest

from helpers import load_fixture

aug = importlib.import_module("sl-hwgat_amd").augment


def state_digests():
    py = hashlib.sha256(repr(random.getstate()).encode()).hexdigest()
    name, keys, pos, has_gauss, gauss = np.random.get_state()
    npd = hashlib.sha256(name.encode() + keys.tobytes() + repr((int(pos), int(has_gauss), float(gauss))).encode())
    return py, npd.hexdigest()


def clips_of(fx):
    off = fx["off"]
    return [fx["clips"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def draw_train(fx):
    tf = aug.TrainTransform(int(fx["src_len"]))
    random.seed(int(fx["seed"]))
    np.random.seed(int(fx["seed"]))
    return [tf.draw(c) for c in clips_of(fx)]


def fill_hand(x, a, e, w, splrep, splev):
    """HandCorrection of one hand, restated: wrist outside the present span, spline (k=2, s=0) through it"""
    present = np.any(x[:, a:e] != 0, axis=(1, 2))
    if not present.any():
        x[:, a:e] = x[:, w:w + 1]
        return
    idx = np.flatnonzero(present)
    x[:idx[0], a:e] = x[:idx[0], w:w + 1]
    x[idx[-1] + 1:, a:e] = x[idx[-1] + 1:, w:w + 1]
    miss = np.setdiff1d(np.arange(idx[0], idx[-1] + 1), idx)
    if len(miss) == 0 or len(idx) < 3:
        return
    for j in range(a, e):
        for c in range(x.shape[2]):
            x[miss, j, c] = splev(miss, splrep(idx, x[idx, j, c].astype(np.float64), k=2))


def apply_record(clip, rec):
    from scipy.interpolate import splev, splrep
    x = np.array(clip, dtype=np.float32)
    l0, l1, lw, r0, r1, rw = rec.hands
    if len(rec.masked):
        x[rec.masked, l0:r1] = 0.0
    fill_hand(x, l0, l1, lw, splrep, splev)
    fill_hand(x, r0, r1, rw, splrep, splev)
    v = ((x - rec.left_top) / rec.edge_dist).astype(np.float64)
    v = v - rec.shear_origin
    v[..., 1] = v[..., 0] * rec.shear + v[..., 1]
    v = v + rec.shear_origin
    v = (v - rec.rot_origin) @ rec.rot + rec.rot_origin
    out = v[rec.src]
    if rec.pad32:
        out = out.astype(np.float32)
    if rec.flip:
        out[..., 0] = 1 - out[..., 0]
    return out.astype(np.float32)


@pytest.mark.parametrize("name", ["augment_2d.npz", "augment_3d.npz"])
def test_train_draw_replays_reference_rng_stream(name):
    fx = load_fixture(name)
    recs = draw_train(fx)
    assert state_digests() == (str(fx["py_state"]), str(fx["np_state"]))
    assert len(recs) == len(fx["train"])
    assert all(len(r.src) == int(fx["src_len"]) for r in recs)
    assert any(r.flip for r in recs) and not all(r.flip for r in recs)
    pickle.loads(pickle.dumps(recs))                      # records travel from DataLoader workers


@pytest.mark.parametrize("name", ["augment_2d.npz", "augment_3d.npz"])
def test_train_records_reproduce_reference_outputs(name):
    pytest.importorskip("scipy")
    fx = load_fixture(name)
    recs = draw_train(fx)
    for i, (clip, rec) in enumerate(zip(clips_of(fx), recs)):
        ref = fx["train"][i]
        got = apply_record(clip, rec)
        assert np.all(np.abs(got - ref) <= 1e-5 * np.maximum(1, np.abs(ref))), i


@pytest.mark.parametrize("name", ["augment_2d.npz", "augment_3d.npz"])
def test_eval_records_reproduce_reference_outputs(name):
    pytest.importorskip("scipy")
    fx = load_fixture(name)
    tf = aug.EvalTransform(int(fx["src_len"]))
    before = state_digests()
    recs = [tf.draw(c) for c in clips_of(fx)]
    assert state_digests() == before                      # the eval transform draws nothing
    for i, (clip, rec) in enumerate(zip(clips_of(fx), recs)):
        ref = fx["eval"][i]
        got = apply_record(clip, rec)
        assert np.all(np.abs(got - ref) <= 1e-5 * np.maximum(1, np.abs(ref))), i


def test_euler_matrix_matches_scipy():
    pytest.importorskip("scipy")
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    for _ in range(20):
        th = rng.normal(0, 0.1, 3) * 90
        np.testing.assert_allclose(aug.euler_xyz_degrees(th), Rotation.from_euler("xyz", th, degrees=True).as_matrix(),
                                   rtol=0, atol=1e-14)


def test_short_clip_raises():
    clip = np.ones((4, 29, 2), np.float32)
    with pytest.raises(ValueError, match="KeypointMasking"):
        aug.TrainTransform(64).draw(clip)
    aug.TrainTransform(64).draw(np.ones((5, 29, 2), np.float32))


@pytest.mark.parametrize("tf", [aug.TrainTransform(32), aug.EvalTransform(32)])
def test_clip_without_normalisation_frame_raises(tf):
    clip = np.ones((20, 29, 3), np.float32)
    clip[::2, 0] = 0.0
    clip[1::2, 4, 1] = 0.0                 # every frame misses the origin or one coordinate of an anchor
    with pytest.raises(ValueError, match="normalised"):
        tf.draw(clip)


def test_eval_record_is_identity_transform():
    rng = np.random.default_rng(0)
    clip = rng.uniform(1, 100, (70, 29, 2)).astype(np.float32)
    rec = aug.EvalTransform(64).draw(clip)
    assert not rec.flip and rec.shear == 0 and np.array_equal(rec.rot, np.eye(2))
    assert np.array_equal(rec.src, np.linspace(0, 69, num=64).astype(int))
    rec = aug.EvalTransform(64).draw(clip[:10])
    start = (64 - 10) // 2
    assert np.array_equal(rec.src[start:start + 10], np.arange(10))
    assert (rec.src[:start] == 0).all() and (rec.src[start + 10:] == 9).all()
