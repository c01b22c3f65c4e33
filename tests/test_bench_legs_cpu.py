"""CPU: a plain `bench.py` run measures only its headline; the legs that take runs of their own (the timer-free repeat
of the timed steps, the eager kernel timing of a --graph run, the secondary configs, the CPU baseline) run only with
--full, and there exactly where they ran before the option existed."""
import importlib.util
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _args(**kw):
    """bench.py's argument defaults, as main() leaves them before extra_legs (--config 3 implies bf16)"""
    a = dict(full=False, config=2, dtype="f32", model="hwgate", batch=None, micro_batch=None, no_cpu_baseline=False,
             no_secondary=False, no_kernel_timers=False, eval_mode=False, deterministic=False, graph=False,
             from_host=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_a_plain_run_has_no_extra_legs():
    legs = _bench().extra_legs
    for kw in ({}, dict(config=3, dtype="bf16"), dict(config=5, micro_batch=16), dict(model="hgate"), dict(graph=True),
               dict(from_host=True), dict(deterministic=True)):
        assert legs(_args(**kw), 1) == set(), kw
    assert legs(_args(), 2) == set()


def test_full_runs_the_legs_the_other_options_leave_on():
    legs = _bench().extra_legs
    assert legs(_args(full=True), 1) == {"timer_free", "secondary", "cpu_baseline"}
    assert legs(_args(full=True, no_secondary=True, no_cpu_baseline=True), 1) == {"timer_free"}
    assert legs(_args(full=True, no_kernel_timers=True), 1) == {"secondary", "cpu_baseline"}
    assert legs(_args(full=True, graph=True), 1) == {"graph_timers", "cpu_baseline"}
    assert legs(_args(full=True, config=3, dtype="bf16"), 1) == {"timer_free", "cpu_baseline"}
    assert legs(_args(full=True, config=5, micro_batch=16), 1) == {"timer_free"}
    assert legs(_args(full=True, model="wgate"), 1) == {"timer_free", "cpu_baseline"}
    assert legs(_args(full=True, eval_mode=True), 1) == {"timer_free", "cpu_baseline"}
    assert legs(_args(full=True), 2) == {"timer_free"}                 # secondary and CPU legs are one-GPU only


def test_full_is_an_option_of_the_command_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout
