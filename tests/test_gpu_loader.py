"""GPU: the device-resident clip store and loader (csrc/loader.hip: hwgat_loader_select / _draw; data.DeviceClipStore,
data.DeviceLoader).  The device's ids, labels, offsets, masked frames and frame maps must equal the numpy restatement of
tests/loader_helpers.py exactly and its fp64 records to 1e-12 (entries are O(1) and come from a handful of fp64 libm calls a
few ulp wide each: about 100 times that); the batch must be bit-equal to what augment.AugmentBatcher makes of the same
records; a clip's record must not depend on how it is batched; a graphed loader must equal the eager one; and a graphed
train step fed by the loader must be reproducible run to run."""
import functools
import importlib

import numpy as np
import pytest
import torch

import loader_helpers as LH

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
train = importlib.import_module("sl-hwgat_amd.train")
data, augment, optim = hw.data, hw.augment, hw.optim
DEV = torch.device("cuda:0")
SEED, B, NC = 1234, 8, 7                                      # tests/test_loader_cpu.py proves this seed reaches every path
PRM_ATOL = 1e-12
THRESHOLDS = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]       # HWGATE.py:96 draws these at random


@functools.lru_cache(maxsize=None)
def the_store(C):
    clips, labels = LH.make_clips(C)
    store = data.DeviceClipStore(clips, labels, DEV, augment.TrainTransform(16))
    return clips, labels, store


def _records_to_samples(clips, rec, n, hands):
    """(clip, label, AugRecord) of the first n rows from a loader's read-back"""
    out = []
    for r in range(n):
        p, i = rec["prm"][r], int(rec["ids"][r])
        C = clips[i].shape[2]
        out.append((clips[i], int(rec["y"][r]),
                    augment.AugRecord(len(clips[i]), rec["masked"][r], p[:C].astype(np.float32), np.float32(p[3]), p[4:4 + C].copy(),
                                      float(p[7]), p[8:8 + C].copy(), p[11:20].reshape(3, 3)[:C, :C].copy(), bool(p[20]),
                                      bool(p[21]), rec["src"][r].copy(), hands)))
    return out


def _assert_batch_equals_restatement(rec, want_sel, want_rows):
    for k in ("ids", "y", "clip_len", "batch_off", "keys"):
        assert np.array_equal(rec[k], want_sel[k]), k
    assert rec["n_rows"] == want_sel["n_rows"]
    for r, row in enumerate(want_rows):
        assert np.array_equal(rec["masked"][r], row["masked"]), (r, "masked")
        assert np.array_equal(rec["src"][r], row["src"]), (r, row["mode"], "src")
        d = np.abs(rec["prm"][r] - row["prm"]).max()
        assert d <= PRM_ATOL, (r, d)


# ------------------------------------------------------------------------------------------ the store
def test_store_holds_the_clips_and_the_hosts_normalisation():
    clips, labels, store = the_store(2)
    assert len(store) == 37 and store.max_frames == 96 and store.total_frames == sum(LH.LENGTHS)
    assert store.nbytes == store.total_frames * 29 * 2 * 4 + 38 * 8 + 37 * 8 + 37 * 16
    assert torch.equal(store.frames.cpu(), torch.from_numpy(np.concatenate(clips)))
    assert store.clip_off.cpu().tolist() == np.r_[0, np.cumsum(LH.LENGTHS)].tolist()
    assert torch.equal(store.labels.cpu(), torch.from_numpy(labels))
    tf = store.transform
    for i in (0, 1, 7, 36):
        lt, e = tf._normalisation(clips[i])
        assert store.norm[i].cpu().tolist() == [float(lt[0]), float(lt[1]), 0.0, float(e)]


# ------------------------------------------------------------------------------------------ train batches
@pytest.mark.parametrize("src_len", [16, 32])
@pytest.mark.parametrize("C", [2, 3])
def test_two_epochs_equal_the_restatement_and_the_batcher(C, src_len):
    clips, labels, store = the_store(C)
    tf = augment.TrainTransform(src_len)
    loader = data.DeviceLoader(store, B, transform=tf, seed=SEED)
    batcher = augment.AugmentBatcher(B, store.max_frames, DEV)
    norm = store.norm.cpu().numpy()
    assert len(loader) == 5
    state, modes = (0, 0), set()
    for step in range(10):
        n = loader.next_batch()
        rec = loader.records()
        sel, state = LH.select(SEED, state[0], state[1], LH.LENGTHS, labels, B)
        rows = LH.draw_batch(sel, LH.LENGTHS, norm, C, src_len, True, **LH.dist_of(tf))
        _assert_batch_equals_restatement(rec, sel, rows)
        modes |= {r["mode"] for r in rows}
        assert n == rec["n_rows"] == (5 if step % 5 == 4 else 8) and (loader.epoch, loader.cursor) == state
        # the same kernels on the same inputs: only max_frames is the capacity instead of the batch maximum
        x_ref, y_ref = batcher(_records_to_samples(clips, rec, n, tf.hands))
        assert torch.equal(loader.x[:n], x_ref) and torch.equal(loader.y[:n], y_ref)
        assert not loader.x[n:].any().item() and not loader.y[n:].any().item()
        assert torch.isfinite(loader.x).all().item()
    assert modes == {"subset", "choice", "linspace", "empty"}


@pytest.mark.parametrize("C", [2, 3])
def test_eval_mode_equals_the_batcher_on_eval_records(C):
    clips, labels, store = the_store(C)
    for src_len in (16, 32):
        ev = augment.EvalTransform(src_len)
        loader = data.DeviceLoader(store, B, transform=ev, shuffle=False)
        batcher = augment.AugmentBatcher(B, store.max_frames, DEV)
        seen = 0
        for x, y in loader:
            n = x.shape[0]
            samples = [(clips[i], int(labels[i]), ev.draw(clips[i])) for i in range(seen, seen + n)]
            x_ref, y_ref = batcher(samples)
            assert torch.equal(x, x_ref) and torch.equal(y, y_ref)
            rec = loader.records()
            assert rec["ids"][:n].tolist() == list(range(seen, seen + n)) and all(len(m) == 0 for m in rec["masked"])
            seen += n
        assert seen == 37 and (loader.epoch, loader.cursor) == (1, 0)


# ------------------------------------------------------------------------------------------ a clip's record is its own
def _by_clip(loader, epochs=2):
    """{(epoch, clip id): (masked, src, prm, x row)} over whole epochs"""
    out = {}
    for ep in range(epochs):
        assert loader.epoch == ep
        for x, y in loader:
            rec = loader.records()
            xs = x.cpu()
            for r in range(x.shape[0]):
                out[(ep, int(rec["ids"][r]))] = (rec["masked"][r], rec["src"][r].copy(), rec["prm"][r].copy(), xs[r].clone())
    return out


def test_a_clips_record_does_not_depend_on_batching_or_ranks():
    _, _, store = the_store(2)
    whole = _by_clip(data.DeviceLoader(store, 8, seed=SEED))
    assert sorted(whole) == [(e, i) for e in range(2) for i in range(37)]
    parts = [_by_clip(data.DeviceLoader(store, 5, seed=SEED)),
             {**_by_clip(data.DeviceLoader(store, 4, seed=SEED, rank=0, world=2)),
              **_by_clip(data.DeviceLoader(store, 4, seed=SEED, rank=1, world=2))}]
    for other in parts:
        assert sorted(other) == sorted(whole)
        for key, (m, s, p, x) in whole.items():
            om, os_, op, ox = other[key]
            assert np.array_equal(m, om) and np.array_equal(s, os_) and np.array_equal(p, op) and torch.equal(x, ox), key
    # another seed or epoch: another record
    assert any(not np.array_equal(whole[(0, i)][2], whole[(1, i)][2]) for i in range(37))
    ordered = data.DeviceLoader(store, 8, seed=SEED, shuffle=False)
    ids = []
    for x, _ in ordered:
        ids += ordered.records()["ids"][:x.shape[0]].tolist()
    assert ids == list(range(37))
    full = data.DeviceLoader(store, 8, seed=SEED, drop_last=True)
    assert len(full) == 4 and [x.shape[0] for x, _ in full] == [8] * 4 and (full.epoch, full.cursor) == (1, 0)


# ------------------------------------------------------------------------------------------ graph, state
def test_graphed_loader_equals_eager_and_state_resumes():
    _, _, store = the_store(2)
    eager = data.DeviceLoader(store, B, seed=SEED)
    graphed = data.DeviceLoader(store, B, seed=SEED, graph=True)
    resumed, tail = None, []
    for step in range(10):
        if step == 7:                                         # mid-epoch: a fresh loader goes on from here
            sd = eager.state_dict()
            assert sd == {"seed": SEED, "epoch": 1, "cursor": 2} == graphed.state_dict()
            resumed = data.DeviceLoader(store, B, seed=0, graph=True)
            resumed.load_state_dict(sd)
        n, ng = eager.next_batch(), graphed.next_batch()
        assert n == ng and torch.equal(eager.x, graphed.x) and torch.equal(eager.y, graphed.y)
        assert torch.equal(eager.n_rows, graphed.n_rows) and torch.equal(eager.frame_map, graphed.frame_map)
        assert torch.equal(eager.params, graphed.params) and torch.equal(eager.ids, graphed.ids)
        assert torch.equal(eager.state, graphed.state)
        if resumed is not None:
            tail.append((eager.x.clone(), eager.y.clone(), n))
    assert graphed.graph is not None and eager.graph is None
    got = [(x.clone(), y.clone()) for x, y in resumed]
    assert len(got) == 3 == len(tail)
    for (x, y), (xe, ye, n) in zip(got, tail):
        assert x.shape[0] == n and torch.equal(x, xe[:n]) and torch.equal(y, ye[:n])
    with pytest.raises(RuntimeError, match="bind before the first batch"):
        graphed.bind(torch.zeros_like(graphed.x), torch.zeros_like(graphed.y))
    with pytest.raises(ValueError, match="x must be"):
        eager.bind(torch.zeros(B, 16, 29, 3, device=DEV), eager.y)


# ------------------------------------------------------------------------------------------ feeding the graphed step
def _hwgate():
    torch.manual_seed(11)
    hp = hw.HWGATEParams({"src_len": 16, "num_class": NC}, 2, DEV, num_kps=64)
    model = hw.Model(*hp.get_model_params()).use_part_table(hw.part_table(29)).to(DEV)
    model.train()
    model.threshold_override = THRESHOLDS
    model.deterministic_train = True
    return model


def _train_run(loader_seed):
    _, _, store = the_store(2)
    model = _hwgate()
    opt = optim.DeviceAdamW(list(model.parameters()), lr=1e-3)
    meter = train.TrainMeter()
    loader = data.DeviceLoader(store, B, seed=loader_seed, graph=True)
    step = train.GraphedTrainStep(model, opt, torch.zeros(B, 16, 29, 2, device=DEV),
                                  torch.zeros(B, dtype=torch.int64, device=DEV), ragged=True, meter=meter)
    loader.bind(step.x, step.y)
    losses = []
    for _ in range(2):
        for x, y in loader:
            assert x.data_ptr() == step.x.data_ptr() and y.data_ptr() == step.y.data_ptr()       # nothing is copied
            step(x, y)
            losses.append(step.loss.clone())
        meter.close_epoch()
    return torch.stack(losses).cpu(), [p.detach().cpu().clone() for p in model.parameters()], meter.history()


def test_graphed_step_fed_by_the_loader_is_reproducible():
    loss_a, w_a, hist_a = _train_run(SEED)
    loss_b, w_b, hist_b = _train_run(SEED)
    assert loss_a.numel() == 10 and torch.isfinite(loss_a).all().item()
    assert torch.equal(loss_a, loss_b) and all(torch.equal(p, q) for p, q in zip(w_a, w_b))
    assert [(h["rows"], h["steps"]) for h in hist_a] == [(37, 5), (37, 5)] == [(h["rows"], h["steps"]) for h in hist_b]
    loss_c, w_c, _ = _train_run(SEED + 1)
    assert not torch.equal(loss_a, loss_c) and any(not torch.equal(p, q) for p, q in zip(w_a, w_c))


def test_epoch_loop_runs_on_a_train_and_an_eval_loader():
    _, _, store = the_store(2)
    model = _hwgate()
    opt = optim.DeviceAdamW(list(model.parameters()), lr=1e-3)
    loader = data.DeviceLoader(store, B, seed=SEED, graph=True)
    eval_loader = data.DeviceLoader(store, B, transform=augment.EvalTransform(16), shuffle=False, graph=True)
    example = (torch.zeros(B, 16, 29, 2, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV))
    loop = train.EpochLoop(model, opt, None, batch_size=B, example=example, num_classes=NC)
    # `epochs` has the reference's meaning, range(start_epoch, epochs + 1): epochs 1 and 2
    book = loop.run(loader, eval_loader, 2, start_epoch=1)
    for lst in book.lists:
        assert len(lst) == 2 and all(np.isfinite(v) for v in lst)
    assert [h["rows"] for h in loop.meter.history()] == [37, 37]
    assert (loader.epoch, loader.cursor) == (2, 0) == (eval_loader.epoch, eval_loader.cursor)
