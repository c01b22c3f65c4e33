"""GPU: the device-side transforms -- hwgat_aug_hand_fill against scipy's splrep / splev, and the whole train / eval
path through `AugmentBatcher` against the reference-generated fixtures (augment_{2d,3d}.npz)."""
import importlib
import random

import numpy as np
import pytest
import torch

from helpers import load_fixture

hw = importlib.import_module("sl-hwgat_amd")
aug = hw.augment
DEV = torch.device("cuda:0")
HANDS = (9, 19, 7, 19, 29, 8)

pytestmark = pytest.mark.gpu


def clips_of(fx):
    off = fx["off"]
    return [fx["clips"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def train_records(fx):
    tf = aug.TrainTransform(int(fx["src_len"]))
    random.seed(int(fx["seed"]))
    np.random.seed(int(fx["seed"]))
    return [tf.draw(c) for c in clips_of(fx)]


def run_batched(batcher, clips, recs, chunk):
    xs, ys = [], []
    for i in range(0, len(clips), chunk):
        x, y = batcher([(c, k, r) for k, (c, r) in enumerate(zip(clips[i:i + chunk], recs[i:i + chunk]), start=i)])
        xs.append(x)
        ys.append(y)
    return torch.cat(xs), torch.cat(ys)


def close(got, ref):
    ref = torch.as_tensor(ref)
    return bool(((got.cpu() - ref).abs() <= 1e-5 * ref.abs().clamp_min(1)).all())


# ---- hwgat_aug_hand_fill vs scipy -------------------------------------------------------------------------------

def presence_cases(rng):
    """(T, left presence, right presence, masked frames) covering every edge case of HandCorrection"""
    out = []
    for n_pres in (3, 4, 5, 7, 16, 33, 64, 100, 257, 600, 1024):
        T = n_pres + int(rng.integers(1, max(2, n_pres // 2) + 1)) + 2
        left = np.zeros(T, bool)
        left[np.sort(rng.choice(T, n_pres, replace=False))] = True
        right = rng.random(T) > 0.3
        out.append((T, left, right, np.sort(rng.choice(T, T // 5, replace=False))))
    T = 40
    base = np.ones(T, bool)
    lead, trail, mid = base.copy(), base.copy(), base.copy()
    lead[:7] = False
    trail[-5:] = False
    mid[10:19] = False
    none = np.zeros(T, bool)
    two, three, one = none.copy(), none.copy(), none.copy()
    two[[5, 30]] = True
    three[[4, 17, 33]] = True
    one[20] = True
    adjacent = none.copy()
    adjacent[[10, 11, 12]] = True                      # 3 present, no gap between them
    parity = none.copy()
    parity[[0, 2, 4, 8, 10, 11, 20, 22, 39]] = True    # interior knots on integer frames
    empty = np.zeros(0, np.int64)
    out += [(T, lead, trail, empty), (T, mid, none, empty), (T, two, three, empty), (T, one, adjacent, empty),
            (T, parity, base, empty), (T, three, two, np.array([4, 9, 25])), (T, lead, mid, np.arange(0, T, 3)),
            (T, base, base, np.arange(T))]
    return out


def make_batch(rng, C, cases):
    clips = []
    for T, left, right, _ in cases:
        clip = rng.uniform(-900, 1900, (T, 29, C)).astype(np.float32)
        clip[~left, 9:19] = 0.0
        clip[~right, 19:29] = 0.0
        clips.append(clip)
    return clips


def expected_fill(clip, masked):
    """HandCorrection restated with scipy: (filled fp32 clip, fp64 spline values, spline-element mask, series scale)"""
    from scipy.interpolate import splev, splrep
    x = clip.copy()
    if len(masked):
        x[masked, 9:29] = 0.0
    v64 = np.zeros(x.shape)
    where = np.zeros(x.shape, bool)
    scale = np.ones(x.shape)
    for a, e, w in ((9, 19, 7), (19, 29, 8)):
        present = np.any(x[:, a:e] != 0, axis=(1, 2))
        if not present.any():
            x[:, a:e] = x[:, w:w + 1]
            continue
        idx = np.flatnonzero(present)
        x[:idx[0], a:e] = x[:idx[0], w:w + 1]
        x[idx[-1] + 1:, a:e] = x[idx[-1] + 1:, w:w + 1]
        miss = np.setdiff1d(np.arange(idx[0], idx[-1] + 1), idx)
        if len(miss) == 0 or len(idx) < 3:
            continue
        for j in range(a, e):
            for c in range(x.shape[2]):
                y = x[idx, j, c].astype(np.float64)
                val = splev(miss, splrep(idx, y, k=2))
                v64[miss, j, c] = val
                where[miss, j, c] = True
                scale[miss, j, c] = max(1.0, np.abs(y).max())
                x[miss, j, c] = val
    return x, v64, where, scale


@pytest.mark.parametrize("C", [2, 3])
def test_hand_fill_matches_scipy_splrep(C):
    pytest.importorskip("scipy")
    rng = np.random.default_rng(40 + C)
    cases = presence_cases(rng)
    clips = make_batch(rng, C, cases)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])])
    masked = np.zeros(off[-1], np.uint8)
    for (_, _, _, m), a in zip(cases, off[:-1]):
        masked[a + m] = 1
    x = torch.from_numpy(np.concatenate(clips)).to(DEV)
    tap = torch.full(x.shape, float("nan"), dtype=torch.float64, device=DEV)
    aug.hand_fill(x, torch.from_numpy(off.astype(np.int32)).to(DEV), max(len(c) for c in clips),
                  masked=torch.from_numpy(masked).to(DEV), tap=tap)
    got, got64 = x.cpu().numpy(), tap.cpu().numpy()
    for i, (clip, case) in enumerate(zip(clips, cases)):
        want, v64, where, scale = expected_fill(clip, case[3])
        g, g64 = got[off[i]:off[i + 1]], got64[off[i]:off[i + 1]]
        assert np.array_equal(np.isfinite(g64), where), i                      # the tap marks exactly the spline
        assert np.all(np.abs(g64[where] - v64[where]) <= 1e-9 * scale[where]), i
        ulp = np.spacing(np.abs(want[where]).astype(np.float32))
        assert np.all(np.abs(g[where] - want[where]) <= ulp), i
        assert np.array_equal(g[~where].view(np.uint32), want[~where].view(np.uint32)), i   # bit-equal elsewhere


def test_hand_fill_rejects_too_long_clips():
    x = torch.zeros((aug.MAX_FRAMES + 1, 29, 2), device=DEV)
    off = torch.tensor([0, aug.MAX_FRAMES + 1], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        aug.hand_fill(x, off, aug.MAX_FRAMES + 1)


# ---- the whole path against the reference fixtures -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["augment_2d.npz", "augment_3d.npz"])
def test_batcher_train_and_eval_match_reference(name):
    fx = load_fixture(name)
    clips = clips_of(fx)
    recs = train_records(fx)
    ev = [aug.EvalTransform(int(fx["src_len"])).draw(c) for c in clips]
    raw = aug.AugmentBatcher(8, 300, DEV)
    win = aug.AugmentBatcher(8, 300, DEV, out_joints=hw.part_table(29))
    for records, ref in ((recs, fx["train"]), (ev, fx["eval"])):
        x29, y = run_batched(raw, clips, records, 8)
        x64, _ = run_batched(win, clips, records, 7)
        assert x29.shape == ref.shape and x64.shape == (*ref.shape[:2], 64, ref.shape[3])
        assert torch.equal(y.cpu(), torch.arange(len(clips)))
        assert close(x29, ref)
        assert torch.equal(x64, x29[:, :, hw.part_table(29).long().to(DEV)])


def test_batcher_runs_are_bitwise_reproducible():
    fx = load_fixture("augment_2d.npz")
    clips, recs = clips_of(fx), train_records(fx)
    b = aug.AugmentBatcher(18, 300, DEV, depth=3)
    x0, _ = run_batched(b, clips, recs, 18)
    x1, _ = run_batched(b, clips, recs, 18)
    x2, _ = run_batched(aug.AugmentBatcher(5, 300, DEV), clips, recs, 5)
    assert torch.equal(x0, x1) and torch.equal(x0, x2)


class _Clips(torch.utils.data.Dataset):
    def __init__(self, clips, tf):
        self.clips, self.tf = clips, tf

    def __len__(self):
        return len(self.clips)

    def __getitem__(self, i):
        clip = self.clips[i].astype(np.float32)
        return clip, i, self.tf.draw(clip)


def test_dataloader_workers_draw_and_batches_do_not_mix_clips():
    fx = load_fixture("augment_3d.npz")
    ds = _Clips(clips_of(fx), aug.TrainTransform(int(fx["src_len"])))
    loader = torch.utils.data.DataLoader(ds, batch_size=5, shuffle=True, num_workers=2, collate_fn=list,
                                         generator=torch.Generator().manual_seed(0))
    batcher = aug.AugmentBatcher(5, 300, DEV)
    one = aug.AugmentBatcher(1, 300, DEV)
    seen = []
    for batch in loader:
        x, y = batcher(batch)
        singles = torch.cat([one([s])[0] for s in batch])
        assert torch.equal(x, singles)
        assert torch.equal(y.cpu(), torch.tensor([s[1] for s in batch]))
        seen += [s[1] for s in batch]
    assert sorted(seen) == list(range(len(ds)))


@pytest.mark.parametrize("model_kind", ["hwgate_f32", "hwgate_bf16", "hgate"])
def test_train_step_fed_by_batcher(model_kind):
    train_mod = importlib.import_module("sl-hwgat_amd.train")
    fx = load_fixture("augment_2d.npz")
    T, C, nc = int(fx["src_len"]), 2, 7
    torch.manual_seed(0)
    if model_kind == "hgate":
        hp = hw.HGATEParams({"src_len": T, "num_class": nc}, C, DEV)
        model = hw.HGATEModel(*hp.get_model_params()).to(DEV)
    else:
        hp = hw.HWGATEParams({"src_len": T, "num_class": nc}, C, DEV, num_kps=64)
        model = hw.Model(*hp.get_model_params()).to(DEV)
        model.use_part_table(hw.part_table(29))
        if model_kind == "hwgate_bf16":
            model.set_activation_dtype(torch.bfloat16)
    model.train()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=5e-4)
    step = train_mod.TrainStep(model, opt)
    clips, recs = clips_of(fx), train_records(fx)
    batcher = aug.AugmentBatcher(6, 300, DEV)
    losses = []
    for i in range(0, 18, 6):
        x, y = batcher([(c, k % nc, r) for k, (c, r) in enumerate(zip(clips[i:i + 6], recs[i:i + 6]), start=i)])
        step(x, y)
        losses.append(float(step.loss))
    assert all(np.isfinite(losses)), losses
