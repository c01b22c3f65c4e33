"""GPU: streaming recognition (csrc/stream.hip: hwgat_stream_push / _window / _decide; serve.StreamRecognizer and the `head`
hook of serve.GraphedEval).

The rings are held against a host deque, the model's static input against the host route -- augment.EvalTransform.draw on
the mirror's window, packed and transformed by augment.AugmentBatcher -- with torch.equal on dyadic-grid inputs (every
fp32 square and sum of the normalisation is exact there, so numpy's summation order cannot enter), and the decision words
against a numpy fp64 restatement of the rule, written below from its description.

Measured on an MI355X:
  ARBITRARY_ULPS  the arbitrary-value case (C = 3) differs from the host route by at most 4 ulp on this input: numpy's fp32
                  dot of three squares is not the sequential sum the kernel forms (about one `unit` in ten differs by a
                  rounding, and `x - left_top` cancels); the bound is four times that: 16 ulp.
  q               the smoothed distribution is within 6.6e-8 of the fp64 restatement; it is held to the bound the softmax of
                  tests/test_gpu_loss_eval.py is held to: max(2e-5, 4 x the deviation of the same rule in fp32 numpy).
"""
import functools
import importlib
from collections import deque

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
serve = importlib.import_module("sl-hwgat_amd.serve")
aug = hw.augment
HF = hw.functional
DEV = torch.device("cuda:0")

S, F, WF, R, J, T, NC = 3, 5, 24, 32, 29, 16, 7
N_RAW = 64                                       # raw frames generated per stream
# frames per stream and step.  Stream 0: padded maps (5, 10, 15), linspace maps (19, 24), the saturated window, ring wrap
# (> 32 frames); stream 1: zeros in between, 20 and 21 frames; stream 2: nothing at first, then one frame that cannot be normalised
COUNTS = [(5, 3, 0), (5, 0, 1), (5, 5, 0), (4, 2, 0), (5, 5, 2), (3, 0, 5), (5, 5, 5), (5, 1, 0), (2, 5, 5), (5, 5, 3)]
ARBITRARY_ULPS = 4 * 4                           # four times the largest distance seen (header)
Q_FLOOR = 2e-5                                   # tests/test_gpu_loss_eval.py: FLOOR


# ------------------------------------------------------------------------------------------ inputs, built once
@functools.lru_cache(maxsize=None)
def raw_streams(C, dyadic=True):
    """(S, N_RAW, J, C) float32: multiples of 2^-8 in (0, 1) or arbitrary values; some hand frames are absent (the spline fill
    runs) and every seventh frame has a zero origin joint (the search for the first normalisable frame runs)"""
    rng = np.random.default_rng(10 * C + dyadic)
    if dyadic:
        x = rng.integers(1, 256, size=(S, N_RAW, J, C)).astype(np.float32) / np.float32(256)
    else:
        x = (rng.standard_normal((S, N_RAW, J, C)) * 0.37 + 0.5).astype(np.float32)
        x[x == 0] = 1.0
    f = np.arange(N_RAW)
    x[:, f % 4 == 1, 9:19] = 0
    x[:, (f % 5 == 2) | (f % 5 == 3), 19:29] = 0
    x[:, f % 7 == 0, 0] = 0
    x.setflags(write=False)
    return x


def make_model(C, batch=S, bf16=False):
    hp = hw.HWGATEParams({"src_len": T, "num_class": NC}, C, DEV, num_kps=64)
    model = hw.Model(*hp.get_model_params()).use_part_table(hw.part_table(29))
    if bf16:
        model.set_activation_dtype(torch.bfloat16)
    return model.eval()


class Feeder:
    """cuts the raw streams into (S, F, J, C) blocks and mirrors every ring in a deque"""

    def __init__(self, data, n_streams=S, push=F):
        self.data, self.S, self.F = data, n_streams, push
        self.pos = [0] * n_streams
        self.mirror = [deque(maxlen=R) for _ in range(n_streams)]

    def block(self, counts):
        frames = np.full((self.S, self.F) + self.data.shape[2:], 7.5, dtype=np.float32)      # slots past the count: never read
        for s, c in enumerate(counts):
            new = self.data[s, self.pos[s]:self.pos[s] + c]
            assert len(new) == c
            frames[s, :c] = new
            self.mirror[s].extend(new)
            self.pos[s] += c
        return frames

    def window(self, s):
        m = list(self.mirror[s])[-WF:]
        return np.stack(m) if m else None


def host_record(window):
    """(AugRecord, its HWGAT_AUG_NPRM doubles) of the host route, or None where the host route refuses the window"""
    if window is None:
        return None
    try:
        rec = aug.EvalTransform(T).draw(window)
    except ValueError:
        return None
    prm = np.zeros(aug.NPRM)
    aug._params(rec, prm)
    return rec, prm


def ulp_distance(a, b):
    """largest distance of two fp32 tensors in units in the last place"""
    def order(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((order(a) - order(b)).abs().max())


def words_of(state, n_streams=S):
    h = HF.STREAM_HEADER_WORDS
    host = state.cpu().numpy()
    return host[:h].view(serve.STREAM_HEADER)[0], host[h:h + n_streams * HF.STREAM_WORDS].view(serve.STREAM_WORDS)


def log_of(state, n_streams=S):
    host = state.cpu().numpy()
    head = host[:HF.STREAM_HEADER_WORDS].view(serve.STREAM_HEADER)[0]
    log = host[HF.STREAM_HEADER_WORDS + n_streams * HF.STREAM_WORDS:].view(serve.STREAM_EVENT)
    return [(int(e["stream"]), int(e["frames_seen"]), int(e["evaluation"]), int(e["cls"])) for e in log[:int(head["log_count"])]]


def as_input(frames, kind):
    """the three ways frames reach `step`: numpy, a pinned tensor, a device tensor"""
    if kind == 0:
        return frames
    t = torch.from_numpy(frames)
    return t.pin_memory() if kind == 1 else t.to(DEV)


# ------------------------------------------------------------------------------------------ the ring
def test_ring_equals_a_host_deque_and_a_garbage_count_is_clamped():
    C = 2
    data = raw_streams(C)
    ring = torch.zeros((S, R, J, C), device=DEV)
    state = torch.zeros(HF.stream_state_words(S, 0), dtype=torch.int64, device=DEV)
    feed = Feeder(data)
    for counts in COUNTS:
        HF.stream_push(ring, state, torch.from_numpy(feed.block(counts)).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV))

    def check():
        _, w = words_of(state)
        host = ring.cpu().numpy()
        for s in range(S):
            assert w["frames_seen"][s] == feed.pos[s] and w["count"][s] == len(feed.mirror[s]) == min(feed.pos[s], R)
            assert w["head"][s] == feed.pos[s] % R
            slots = (w["head"][s] - w["count"][s] + np.arange(w["count"][s])) % R
            assert np.array_equal(host[s, slots], np.stack(feed.mirror[s])) if len(slots) else True
        return host
    check()
    assert max(feed.pos) > R and min(feed.pos) < R              # one ring wrapped, one did not fill
    # a count word that is garbage: clamped to [0, F]; nothing but the F next slots of that ring is written
    before = ring.cpu().numpy().copy()
    block = feed.block((F, 0, 3))
    HF.stream_push(ring, state, torch.from_numpy(block).to(DEV), torch.tensor([1 << 30, -(1 << 30), 3], dtype=torch.int32, device=DEV))
    after = check()
    _, w = words_of(state)
    changed = np.zeros((S, R), dtype=bool)
    for s, c in enumerate((F, 0, 3)):
        changed[s, (w["head"][s] - c + np.arange(c)) % R] = True
    assert np.array_equal(after[~changed], before[~changed])


# ------------------------------------------------------------------------------------------ the model's input
def run_parity(C, gathered, dyadic):
    """the scripted sequence through a graphed recogniser; per step and ready stream the device's row, frame map and record
    beside the host route's"""
    table = hw.part_table(29) if gathered else None
    rec = serve.StreamRecognizer(make_model(C), S, WF, R, F, joints=J, coords=C, out_joints=table)
    batcher = aug.AugmentBatcher(S, N_RAW, DEV, out_joints=table)
    feed = Feeder(raw_streams(C, dyadic))
    out, lengths, not_ready = [], set(), 0
    for k, counts in enumerate(COUNTS):
        rec.step(as_input(feed.block(counts), k % 3), list(counts) if k % 2 else torch.tensor(counts, device=DEV))
        st = rec.poll()
        windows = [feed.window(s) for s in range(S)]
        L = [0 if w is None else len(w) for w in windows]
        assert rec.clip_off.tolist() == [0] + np.cumsum(L).tolist()
        assert st["count"].tolist() == [len(m) for m in feed.mirror] and st["frames_seen"].tolist() == feed.pos
        host = [host_record(w) for w in windows]
        assert st["ready"].tolist() == [int(h is not None) for h in host]
        ready = [s for s in range(S) if host[s] is not None]
        not_ready += S - len(ready)
        if not ready:
            continue
        x_host, _ = batcher([(windows[s], 0, host[s][0]) for s in ready])
        assert torch.isfinite(rec.model_input).all() and torch.isfinite(rec.logits).all()
        for i, s in enumerate(ready):
            lengths.add(L[s])
            out.append((k, s, rec.model_input[s].clone(), x_host[i], rec.frame_map[s].cpu().numpy(), host[s][0].src,
                        rec.params[s].cpu().numpy(), host[s][1]))
    # the sequence reaches every path of the frame map, the saturated window and the wrap
    assert min(lengths) < T < max(lengths) == WF and any(T < n < WF for n in lengths) and max(feed.pos) > R and not_ready >= 3
    return out


@pytest.mark.parametrize("gathered", [False, True], ids=["raw29", "table64"])
@pytest.mark.parametrize("C", [2, 3])
def test_model_input_equals_the_host_route_on_dyadic_values(C, gathered):
    for k, s, x_dev, x_host, map_dev, map_host, prm_dev, prm_host in run_parity(C, gathered, True):
        assert np.array_equal(map_dev, map_host), (k, s)
        assert np.array_equal(prm_dev, prm_host), (k, s, prm_dev, prm_host)
        assert torch.equal(x_dev, x_host), (k, s, ulp_distance(x_dev, x_host))


def test_model_input_on_arbitrary_values_is_within_the_measured_bound():
    seen = 0
    for k, s, x_dev, x_host, map_dev, map_host, _, _ in run_parity(3, False, False):
        assert np.array_equal(map_dev, map_host), (k, s)
        seen = max(seen, ulp_distance(x_dev, x_host))
    print(f"arbitrary values: largest distance to the host route {seen} ulp")
    assert seen <= ARBITRARY_ULPS, seen


def test_frame_map_for_every_window_length():
    C = 2
    rec = serve.StreamRecognizer(make_model(C), 1, WF, R, 1, joints=J, coords=C)
    data = raw_streams(C)
    maps, lens = [], []
    for k in range(WF + 3):
        rec.step(data[:1, k:k + 1], [1])
        maps.append(rec.frame_map[0].clone())
        lens.append(rec.clip_off.clone())
    tf = aug.EvalTransform(T)
    for k in range(WF + 3):
        L = min(k + 1, WF)
        want, _ = tf._temporal_sample(L, False)
        assert lens[k].tolist() == [0, L]
        assert np.array_equal(maps[k].cpu().numpy(), want.astype(np.int32)), (L, maps[k].tolist(), want.tolist())


# ------------------------------------------------------------------------------------------ streams that are not ready
def test_a_stream_that_is_not_ready_moves_nothing_and_disturbs_nobody():
    C = 2
    data = raw_streams(C)
    model = make_model(C)
    blind = np.array(data)
    blind[1, :, 0] = 0                                        # stream 1 never shows its origin joint
    runs = {}
    for name, src, counts, graph in (("plain", data, (5, 5, 5), False), ("empty", data, (5, 0, 5), True),
                                     ("blind", blind, (5, 5, 5), False)):
        rec = serve.StreamRecognizer(model, S, WF, R, F, joints=J, coords=C, threshold=0.0, hold=1, graph=graph)
        feed = Feeder(src)
        rows = []
        for _ in range(6):
            rec.step(feed.block(counts), list(counts))
            assert torch.isfinite(rec.model_input).all() and torch.isfinite(rec.logits).all() and torch.isfinite(rec.q).all()
            assert torch.isfinite(rec.params).all()
            rows.append((rec.model_input.clone(), rec.logits.clone()))
        runs[name] = (rows, rec.poll(), rec)
    st = runs["plain"][1]
    assert st["ready"].tolist() == [1, 1, 1] and st["evals"].tolist() == [6, 6, 6] and st["n_events"].min() >= 1
    for name in ("empty", "blind"):
        rows, st, rec = runs[name]
        assert st["ready"].tolist() == [1, 0, 1]
        for key in ("top", "run", "evals", "n_events"):       # the decision words of stream 1 never moved
            assert st[key][1] == 0, key
        assert st["conf"][1] == 0.0 and not rec.q[1].any()
        assert all(ev.stream != 1 for ev in st["events"]) and len(st["events"]) == len(runs["plain"][1]["events"]) - int(
            sum(ev.stream == 1 for ev in runs["plain"][1]["events"]))
        assert st["count"][1] == (0 if name == "empty" else min(6 * F, R))
        for (x, z), (x0, z0) in zip(rows, runs["plain"][0]):
            for s in (0, 2):
                assert torch.equal(x[s], x0[s]) and torch.equal(z[s], z0[s])
        _, w = words_of(rec.state)
        assert w["fired"][1] == 0 and w["win_len"][1] == (0 if name == "empty" else WF)
    assert not runs["empty"][0][-1][0][1].any()               # an empty clip resamples to zeros
    # the benign record of a stream that is not ready
    prm = runs["blind"][2].params[1].cpu().numpy()
    assert prm[:3].tolist() == [0, 0, 0] and prm[3] == 1.0


# ------------------------------------------------------------------------------------------ the decision rule
STEPS = 30
# per stream: (class, peak probability, steps).  Stream 0: a long run, then two more; stream 1: a run, a break of three
# steps, the run again, then a class too faint for the first threshold; stream 2: the blank class around one real sign
SCRIPT = [[(2, 0.90, 12), (4, 0.85, 10), (2, 0.90, 8)],
          [(3, 0.90, 6), (5, 0.80, 3), (3, 0.90, 8), (1, 0.50, 13)],
          [(0, 0.90, 14), (6, 0.80, 5), (0, 0.90, 11)]]
# (alpha, threshold, hold, blank_class) and the step from which they hold: changed through the device words mid-way
RULES = [(0, (0.5, 0.6, 3, 0)), (22, (0.5, 0.45, 2, 0))]
SCRIPT_SEED = 0                                  # chosen so that the restatement decides nothing by a hair (asserted below)


def rule_at(t):
    return [r for t0, r in RULES if t0 <= t][-1]


@functools.lru_cache(maxsize=None)
def scripted_logits():
    """(STEPS, S, NC) fp32 logits whose softmax puts `peak` on the scripted class and unequal shares on the others"""
    rng = np.random.default_rng(SCRIPT_SEED)
    z = np.zeros((STEPS, S, NC), dtype=np.float32)
    for s, runs in enumerate(SCRIPT):
        # a fixed, evenly spaced ranking of the classes that are not on top; the scripted classes rank highest, in order of
        # appearance, so that a class that leaves the top settles above the others and passes none of them on its way down
        tops = list(dict.fromkeys(cls for cls, _, _ in runs))
        others = [c for c in range(NC) if c not in tops]
        share = np.zeros(NC)
        share[tops + [others[i] for i in rng.permutation(len(others))]] = np.arange(NC + 1.0, 1.0, -1.0)
        t = 0
        for cls, peak, n in runs:
            for _ in range(n):
                w = np.delete(share, cls) * rng.uniform(0.99, 1.01, NC - 1)
                p = np.insert((1 - peak) * w / w.sum(), cls, peak)
                z[t, s] = np.log(p) + rng.uniform(-1, 1)      # the softmax does not see a shift of the row
                t += 1
        assert t == STEPS
    return z


def restate(z, dtype=np.float64):
    """the rule for one stream, from its description: z (STEPS, NC) logits -> per step (q, top, conf, run, fired, event)"""
    q, prev, run, fired, out = None, None, 0, False, []
    for t, row in enumerate(z):
        alpha, threshold, hold, blank = rule_at(t)
        row = row.astype(dtype)
        e = np.exp(row - row.max())
        p = e / e.sum()
        q = p if q is None else dtype(1 - alpha) * q + dtype(alpha) * p
        top = int(np.argmax(q))                               # the lowest index of the maximum
        conf = q[top]
        if prev is not None and top == prev:
            run += 1
        else:
            run, fired = 1, False
        event = run >= hold and conf >= threshold and not fired and top != blank
        fired = fired or event
        prev = top
        out.append((q.copy(), top, float(conf), run, fired, bool(event)))
    return out


class Scripted(torch.nn.Module):
    """returns row `step` of a device table and advances the device counter: a forward without any kernel of this project"""

    def __init__(self, table):
        super().__init__()
        self.table = torch.nn.Parameter(table, requires_grad=False)
        self.register_buffer("step", torch.zeros(1, dtype=torch.int64, device=table.device))
        self.temporal_dim = T

    def forward(self, x):
        out = torch.index_select(self.table, 0, self.step)[0]
        self.step.add_(1)
        return out


def test_decision_follows_the_restated_rule():
    z = scripted_logits()
    want = [restate(z[:, s]) for s in range(S)]
    want32 = [restate(z[:, s], np.float32) for s in range(S)]
    # the scripts decide nothing by a hair: no confidence near a threshold, no two entries of q near a tie
    for s in range(S):
        for t, (q, top, conf, run, fired, event) in enumerate(want[s]):
            assert abs(conf - rule_at(t)[1]) > 1e-3, (s, t, conf)
            gaps = np.abs(q[:, None] - q[None, :])[~np.eye(NC, dtype=bool)]
            assert gaps.min() > 1e-3, (s, t, np.sort(q))
    events = [(t, s, want[s][t][1]) for t in range(STEPS) for s in range(S) if want[s][t][5]]
    by_stream = [[(t, c) for t, s_, c in events if s_ == s] for s in range(S)]
    # what the scripts are there to show
    assert [c for _, c in by_stream[0]] == [2, 4, 2] and by_stream[0][0][0] == 2          # once in a run of twelve
    assert [c for _, c in by_stream[1]][:2] == [3, 3] and by_stream[1][1][0] >= 9          # again after the broken run
    assert [c for _, c in by_stream[1]][2:] == [1] and by_stream[1][2][0] == 22            # the lowered threshold lets it through
    assert [c for _, c in by_stream[2]] == [6]                                             # never the blank class
    assert len(events) == 7
    q_dev = max(float(np.abs(want32[s][t][0] - want[s][t][0]).max()) for s in range(S) for t in range(STEPS))
    q_bound = max(Q_FLOOR, 4 * q_dev)

    table = torch.from_numpy(np.concatenate([z, np.zeros((4, S, NC), dtype=np.float32)])).to(DEV)
    data = raw_streams(2)
    cap = 3
    results = {}
    for graph, log_capacity, polled in ((True, cap, False), (False, 64, True)):
        model = Scripted(table).eval()
        a, thr, hold, blank = rule_at(0)
        rec = serve.StreamRecognizer(model, S, WF, R, 1, joints=J, coords=2, alpha=a, threshold=thr, hold=hold,
                                     blank_class=blank, log_capacity=log_capacity, graph=graph)
        model.step.zero_()                                    # warm-up and capture advanced the counter
        rec.push(data[:, 1:2], [1, 1, 1])                     # frame 1 can be normalised: every stream is ready from step 0 on
        captured = rec._runner.graph
        qs, states, got = [], [], []
        for t in range(STEPS):
            if t and rule_at(t) != rule_at(t - 1):
                a, thr, hold, blank = rule_at(t)
                rec.set_decision(alpha=a, threshold=thr, hold=hold, blank_class=blank)
            rec.step(data[:, 2 + t:3 + t], [1, 1, 1])
            qs.append(rec.q.clone())
            states.append(rec.state.clone())
            if polled:
                st = rec.poll()
                assert st["overflow"] == 0
                got += [(t, ev.stream, ev.cls) for ev in st["events"]]
                for ev in st["events"]:                       # the first frame was pushed before step 0
                    assert ev.frames_seen == t + 2 and ev.evaluation == t
                    assert abs(ev.conf - want[ev.stream][t][2]) <= q_bound
        assert rec._runner.graph is captured                  # the new rule needed no new capture
        results[graph] = (qs, states, got, rec)
    worst = 0.0
    for graph, (qs, states, got, rec) in results.items():
        for t in range(STEPS):
            _, w = words_of(states[t])
            q = qs[t].cpu().numpy()
            for s in range(S):
                wq, top, conf, run, fired, _ = want[s][t]
                worst = max(worst, float(np.abs(q[s] - wq).max()))
                assert np.abs(q[s] - wq).max() <= q_bound and abs(w["conf"][s] - conf) <= q_bound
                assert (w["top"][s], w["run"][s], w["fired"][s], w["evals"][s], w["ready"][s]) == (top, run, int(fired), t + 1, 1)
                assert w["events"][s] == sum(1 for tt, c in by_stream[s] if tt <= t)
    print(f"q: largest distance to the fp64 restatement {worst:.2e} (bound {q_bound:.2e}, fp32 numpy deviates {q_dev:.2e})")
    # polled every step: every event, in order of step and stream
    assert results[False][2] == events
    # never polled, three slots: the log is intact up to its capacity and the rest is counted
    rec = results[True][3]
    assert [(s, c) for s, _, _, c in log_of(rec.state)] == [(s, c) for _, s, c in events[:cap]]
    assert [e for _, _, e, _ in log_of(rec.state)] == [t for t, _, _ in events[:cap]]
    st = rec.poll()
    assert st["overflow"] == len(events) - cap and [(ev.stream, ev.cls) for ev in st["events"]] == [(s, c) for _, s, c in events[:cap]]
    assert st["n_events"].tolist() == [len(b) for b in by_stream]
    again = rec.poll()                                        # the poll emptied the log
    assert again["events"] == [] and again["overflow"] == 0


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_graph_and_eager_agree_reset_and_reallocation(bf16):
    C = 2
    data = raw_streams(C)
    model = make_model(C, bf16=bf16)
    kw = dict(joints=J, coords=C, threshold=0.0, hold=2, alpha=0.5)
    recs = [serve.StreamRecognizer(model, S, WF, R, F, graph=g, **kw) for g in (True, True, False)]
    feeds = [Feeder(data) for _ in recs]
    for counts in COUNTS:
        for rec, feed in zip(recs, feeds):
            rec.step(feed.block(counts), list(counts))
    a = recs[0]
    assert log_of(a.state)                                    # something was recognised: the logs below are not empty
    for b in recs[1:]:
        for name in ("state", "ring", "q", "logits", "model_input", "clip_off", "frame_map", "params"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    # reset of one stream: it behaves as new, the others are untouched
    keep = {name: getattr(a, name).clone() for name in ("state", "ring", "q")}
    a.reset(streams=[1])
    _, w = words_of(a.state)
    _, w0 = words_of(keep["state"])
    assert w[1] == np.zeros((), dtype=serve.STREAM_WORDS) and not a.ring[1].any() and not a.q[1].any()
    for s in (0, 2):
        assert w[s] == w0[s] and torch.equal(a.ring[s], keep["ring"][s]) and torch.equal(a.q[s], keep["q"][s])
    assert log_of(a.state) == log_of(keep["state"])
    fresh = serve.StreamRecognizer(model, S, WF, R, F, graph=False, **kw)
    late, new = Feeder(data), Feeder(data)
    late.pos = list(feeds[0].pos)
    late.pos[1] = 0                                           # stream 1 of the reset recogniser starts over
    for counts in COUNTS[:4]:
        a.step(late.block(counts), list(counts))
        fresh.step(new.block(counts), list(counts))
        assert torch.equal(a.logits[1], fresh.logits[1]) and torch.equal(a.q[1], fresh.q[1])
        assert torch.equal(a.model_input[1], fresh.model_input[1])
    _, w = words_of(a.state)
    _, wf = words_of(fresh.state)
    assert w[1] == wf[1] and w["evals"][0] == len(COUNTS) + 4
    ev_a = [e[1:] for e in log_of(a.state) if e[0] == 1][-int(wf["events"][1]):] if wf["events"][1] else []
    assert ev_a == [e[1:] for e in log_of(fresh.state) if e[0] == 1]
    # a reallocated parameter: the graph holds the old address
    p = model.head.weight
    p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="capture again"):
        a.step(Feeder(data).block(COUNTS[0]), list(COUNTS[0]))
    model.train()
    with pytest.raises(RuntimeError, match=r"train\(\)"):
        fresh.step(Feeder(data).block(COUNTS[0]), list(COUNTS[0]))
    model.eval()
