"""CPU: `bench.py --dump-outputs DIR` writes what the last timed train step computed -- loss, correct count, updated
parameters, gradients -- as float32 / float64 .npy files, whole when small and as a fixed sample when large, and
`--steps` below 1 is refused before anything runs."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _model_and_step(seed=0, sizes=((40, 30), (30,), (7, 3))):
    g = torch.Generator().manual_seed(seed)
    model = torch.nn.Module()
    for i, s in enumerate(sizes):
        p = torch.nn.Parameter(torch.randn(s, generator=g))
        p.grad = torch.randn(s, generator=g)
        model.register_parameter(f"p{i}", p)
    model.register_parameter("frozen", torch.nn.Parameter(torch.ones(5), requires_grad=False))
    step = types.SimpleNamespace(loss=torch.tensor(1.25), correct=torch.tensor(3))
    return model, step


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_the_whole_step_output_when_small(tmp_path):
    bench = _bench()
    model, step = _model_and_step()
    bench.dump_outputs(model, step, str(tmp_path / "d"))
    out = _load(tmp_path / "d")
    assert set(out) == {"loss", "correct", "params", "grads"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert float(out["loss"]) == 1.25 and float(out["correct"]) == 3.0
    trainable = [p for p in model.parameters() if p.requires_grad]
    np.testing.assert_array_equal(out["params"], torch.cat([p.detach().flatten() for p in trainable]).numpy())
    np.testing.assert_array_equal(out["grads"], torch.cat([p.grad.flatten() for p in trainable]).numpy())


def test_dump_of_a_large_model_is_a_fixed_sample_within_the_size_cap(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 500)
    model, step = _model_and_step()
    for d in ("a", "b"):
        bench.dump_outputs(model, step, str(tmp_path / d))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a["params"].shape == a["grads"].shape == (500,)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])                     # same entries, same values, run after run
    trainable = [p for p in model.parameters() if p.requires_grad]
    full = torch.cat([p.detach().flatten() for p in trainable]).numpy()
    idx = np.sort(np.random.default_rng(0).choice(full.size, 500, replace=False))
    np.testing.assert_array_equal(a["params"], full[idx])
    # the real cap keeps a dump of any model within 64 MB
    assert 2 * bench.DUMP_SAMPLE * 4 + 16 <= 64 * 2 ** 20


def test_steps_below_one_are_refused():
    env = dict(os.environ, HWGAT_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
