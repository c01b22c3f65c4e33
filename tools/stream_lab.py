#!/usr/bin/env python3
"""per-step latency of streaming recognition (serve.StreamRecognizer) beside the graphed forward alone and the host route,
HWGATE at the headline shape (src_len 128, 2002 classes, 29 raw joints through part_table(29)), window 192 frames, one new
frame per stream and step, S = 1 and 8 streams, fp32 and bf16.  Writes profiles/stream_lab.txt (or the path given).

Every figure is the median over REPEATS timed loops of LOOP iterations after a warm-up loop, host wall clock with the
synchronising call inside the loop; "device" figures are HIP-event times around the replay alone."""
import importlib, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hw = importlib.import_module("sl-hwgat_amd")
serve = importlib.import_module("sl-hwgat_amd.serve")
aug = hw.augment
dev = torch.device("cuda:0")
T, NC, J, C, WF, R, F = 128, 2002, 29, 2, 192, 256, 1
REPEATS, LOOP = 7, 40
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stream_lab.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clock(fn):
    """median microseconds per call of fn (which synchronises itself) over REPEATS loops"""
    for _ in range(LOOP):
        fn()
    per = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(LOOP):
            fn()
        per.append((time.perf_counter() - t0) / LOOP * 1e6)
    return statistics.median(per), min(per), max(per)


def device_us(fn):
    """median HIP-event microseconds of fn (enqueue only) over REPEATS x LOOP calls"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPEATS * LOOP)]
    for _ in range(LOOP):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


say(f"stream_lab: HWGATE src_len {T}, {NC} classes, {J} joints x {C}, window {WF}, ring {R}, {F} new frame per stream and step")
say(f"median [min .. max] of {REPEATS} loops of {LOOP} calls, microseconds per call; {torch.cuda.get_device_name(0)}")
rng = np.random.default_rng(0)
for dt in (torch.float32, torch.bfloat16):
    torch.manual_seed(0)
    hp = hw.HWGATEParams({"src_len": T, "num_class": NC}, C, dev, num_kps=64)
    model = hw.Model(*hp.get_model_params()).use_part_table(hw.part_table(29)).eval()
    model.set_activation_dtype(dt)
    for S in (1, 8):
        raw = rng.integers(1, 256, size=(S, WF + 8, J, C)).astype(np.float32) / np.float32(256)     # exact in every fp32 sum
        rec = serve.StreamRecognizer(model, S, WF, R, F, joints=J, coords=C)
        for k in range(WF):                                   # saturate the windows: every stream ready, L = WF
            rec.push(raw[:, k:k + 1], [1] * S)
        frames, counts = raw[:, WF:WF + 1], [1] * S
        rec.step(frames, counts)
        assert rec.poll()["ready"].all()
        x = rec.model_input.clone()

        def stream_step():
            rec.step(frames, counts)
            rec.poll()
        t_stream = clock(stream_step)
        d_stream = device_us(rec._runner._replay)

        fast = serve.GraphedEval(model, x)

        def graph_only():
            fast(x)
            torch.cuda.synchronize()
        t_graph = clock(graph_only)
        d_graph = device_us(fast._replay)

        tf, batcher = aug.EvalTransform(T), aug.AugmentBatcher(S, WF, dev)
        windows = [np.ascontiguousarray(raw[s, 1:WF + 1]) for s in range(S)]

        def host_route():
            samples = [(w, 0, tf.draw(w)) for w in windows]
            xb, _ = batcher(samples)
            return torch.softmax(fast(xb).float(), -1).cpu()
        t_host = clock(host_route)
        assert torch.equal(batcher([(w, 0, tf.draw(w)) for w in windows])[0], x)      # the same input as the device route

        def draw_only():
            [tf.draw(w) for w in windows]
        t_draw = clock(draw_only)
        name = "fp32" if dt == torch.float32 else "bf16"
        say(f"{name} S={S}:")
        say(f"  StreamRecognizer.step + poll      {t_stream[0]:8.1f} [{t_stream[1]:8.1f} .. {t_stream[2]:8.1f}]   replay on the device {d_stream:8.1f}")
        say(f"  GraphedEval alone, ready clip     {t_graph[0]:8.1f} [{t_graph[1]:8.1f} .. {t_graph[2]:8.1f}]   replay on the device {d_graph:8.1f}")
        say(f"  host route (draw+batch+graph+cpu) {t_host[0]:8.1f} [{t_host[1]:8.1f} .. {t_host[2]:8.1f}]   of which EvalTransform.draw {t_draw[0]:8.1f}")
        say(f"  added by streaming: device {d_stream - d_graph:+8.1f} (push, window, hand fill, resample, decide inside the graph), "
            f"host {t_stream[0] - t_graph[0] - (d_stream - d_graph):+8.1f} (pinned upload, the poll's read and decode)")
        # which stage: the same launches issued eagerly, every entry point between two HIP events (functional.TIMERS); an
        # event pair costs a few microseconds itself, so these say where the added device time goes, not how much it is
        eager = serve.StreamRecognizer(model, S, WF, R, F, joints=J, coords=C, graph=False)
        for k in range(WF):
            eager.push(raw[:, k:k + 1], [1] * S)
        eager.step(frames, counts)
        hw.functional.prime_events(2 * 400 * LOOP)
        hw.functional.TIMERS = {}
        for _ in range(LOOP):
            eager.step(frames, counts)
        torch.cuda.synchronize()
        timers, hw.functional.TIMERS = hw.functional.TIMERS, None
        stages = ("hwgat_stream_push", "hwgat_stream_window", "hwgat_aug_hand_fill", "hwgat_aug_resample", "hwgat_stream_decide")
        per = {n: statistics.median(a.elapsed_time(b) * 1e3 for a, b in timers[n]) for n in stages}
        say("  per stage, eager, between HIP events: " + ", ".join(f"{n.split('_', 1)[1]} {per[n]:.1f}" for n in stages)
            + f" (sum {sum(per.values()):.1f})")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
