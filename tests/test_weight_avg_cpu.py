"""CPU: host logic of optim.WeightAverage (csrc/weight_avg.hip) -- the new entry points in the header, the binding and the
library, their argument checks, what is and is not shadowed, argument errors, both state dicts, that everything that
launches raises on CPU tensors, that an averager changes nothing of an optimizer's state_dict(), and
checkpoint.get_device_optimizer(weight_average=...)."""
import copy
import ctypes
import importlib
import io
import math
import re

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
optim = importlib.import_module("sl-hwgat_amd.optim")
ck = hw.checkpoint
CPU = torch.device("cpu")
WAVG_SYMBOLS = {f"hwgat_wavg_{what}" for what in ("set", "advance", "update", "swap")}
OPTIMIZERS = [(optim.DeviceAdamW, torch.optim.AdamW, dict(lr=2e-3, weight_decay=0.05)),
              (optim.DeviceSGD, torch.optim.SGD, dict(lr=2e-3, momentum=0.9)),
              (optim.DeviceNAdam, torch.optim.NAdam, dict(lr=2e-3))]


def _hwgate():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, CPU, num_kps=32)
    return hw.Model(*hp.get_model_params())


def _stgcn():
    hp = hw.STGCNParams({"src_len": 32, "num_class": 7}, 2, CPU)
    return hw.STGCNModel(*hp.get_model_params())


def test_symbols_abi_and_constants_follow_the_header():
    assert WAVG_SYMBOLS <= set(hw._lib.declared_symbols())
    assert WAVG_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_wavg_")}
    assert not any(n.startswith(("hwgat_gguard_", "hwgat_optim_", "hwgat_sgd_", "hwgat_nadam_")) for n in WAVG_SYMBOLS)
    L = hw._lib.lib()
    for name in WAVG_SYMBOLS:                                # exported by the library that was built
        assert getattr(L, name) is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+HWGAT_WAVG_(\w+)\s+(\d+)", src)}
    assert slots.pop("NSTATE") == optim.WAVG_NSTATE
    assert slots.pop("ENTRY_BYTES") == optim.WAVG_ENTRY_BYTES == optim.WAVG_ENTRY.size == 32
    mine = dict(MODE=optim.W_MODE, DECAY=optim.W_DECAY, WARMUP=optim.W_WARMUP, START=optim.W_START, EVERY=optim.W_EVERY,
                STEPS_SEEN=optim.W_STEPS_SEEN, N_AVERAGED=optim.W_N_AVERAGED, COEF=optim.W_COEF, ACTIVE=optim.W_ACTIVE)
    assert slots == mine and sorted(mine.values()) == list(range(9)) and max(mine.values()) < optim.WAVG_NSTATE
    assert int(re.search(r"#define\s+HWGAT_OPTIM_CHUNK\s+(\d+)", src).group(1)) == optim.CHUNK


def test_entry_points_refuse_bad_arguments_without_launching():
    L = hw._lib.lib()
    buf = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)      # 16-byte aligned host memory: never dereferenced
    nan, inf = math.nan, math.inf
    assert L.hwgat_wavg_set(None, 0, 0.9, 0, 0, 1, None) == -1
    for mode in (-1, 2, 7):
        assert L.hwgat_wavg_set(buf, mode, 0.9, 0, 0, 1, None) == -1, mode
    for decay in (-0.1, 1.0, 1.5, nan, inf, -inf):
        assert L.hwgat_wavg_set(buf, 0, decay, 0, 0, 1, None) == -1, decay
    for start in (-1, -2 ** 40):
        assert L.hwgat_wavg_set(buf, 0, 0.9, 0, start, 1, None) == -1, start
    for every in (0, -1, -2 ** 40):
        assert L.hwgat_wavg_set(buf, 0, 0.9, 0, 0, every, None) == -1, every
    assert L.hwgat_wavg_advance(None, None, None) == -1
    assert L.hwgat_wavg_advance(None, buf, None) == -1
    update, swap = L.hwgat_wavg_update, L.hwgat_wavg_swap
    assert update(None, 1, buf, 1, None) == -1
    assert update(buf, 1, None, 1, None) == -1
    assert update(ctypes.c_void_p(buf.value + 4), 1, buf, 1, None) == -1     # records hold 8-byte words
    for n in (0, -1):
        assert update(buf, n, buf, 1, None) == -1
        assert swap(buf, n, 1, None) == -1
    for blocks in (0, -1):
        assert update(buf, 1, buf, blocks, None) == -1
        assert swap(buf, 1, blocks, None) == -1
    assert swap(None, 1, 1, None) == -1
    assert swap(ctypes.c_void_p(buf.value + 4), 1, 1, None) == -1


def test_construction_and_what_is_shadowed():
    model = _hwgate()
    avg = optim.WeightAverage(model)
    assert (avg.mode, avg.decay, avg.warmup, avg.start, avg.every, avg.buffers) == ("ema", 0.999, False, 0, 1, True)
    assert not avg.is_applied
    names = [n for n, _ in model.named_parameters()]
    assert avg.keys() == names and len(names) > 0           # HWGATE: parameters only, though it has buffers
    assert len(list(model.buffers())) > 0
    for s, (_, p) in zip(avg._shadow, model.named_parameters()):
        assert s.dtype == torch.float32 and torch.equal(s, p.detach()) and s.data_ptr() != p.data_ptr()
        assert not s.requires_grad
    assert avg.counters() == dict(steps_seen=0, n_averaged=0)

    model = _stgcn()
    params = [n for n, _ in model.named_parameters()]
    stats = [k for k in model.state_dict() if k.endswith(("running_mean", "running_var"))]
    assert len(stats) >= 4 and "A" in model.state_dict()
    assert any(k.endswith("num_batches_tracked") for k in model.state_dict())
    with_b = optim.WeightAverage(model, buffers=True)
    without = optim.WeightAverage(model, buffers=False)
    assert without.keys() == params
    assert with_b.keys()[:len(params)] == params and sorted(with_b.keys()[len(params):]) == sorted(stats)
    for a in (with_b, without):
        assert "A" not in a.keys() and not any(k.endswith("num_batches_tracked") for k in a.keys())
        assert set(a.keys()) <= set(model.state_dict())
    sd = model.state_dict()
    for k, s in zip(with_b.keys(), with_b._shadow):
        assert torch.equal(s, sd[k]) and s.data_ptr() != sd[k].data_ptr()


def test_argument_errors():
    model = _hwgate()
    for bad in (dict(mode="mean"), dict(mode=None), dict(mode=0), dict(decay=1.0), dict(decay=-0.1), dict(decay=math.nan),
                dict(start=-1), dict(start=0.5), dict(every=0), dict(every=-3), dict(every=1.5), dict(every=True)):
        with pytest.raises(ValueError):
            optim.WeightAverage(model, **bad)
    optim.WeightAverage(model, mode="swa", decay=0.0, warmup=True, start=3, every=2, buffers=False)
    avg = optim.WeightAverage(model)
    avg.decay = 1.0                                          # a bad value set later is refused when it is next used
    with pytest.raises(ValueError, match="decay"):
        avg.push()
    half = copy.deepcopy(model).half()
    with pytest.raises(ValueError, match="float32"):
        optim.WeightAverage(half)
    with pytest.raises(ValueError, match="nothing to average"):
        optim.WeightAverage(torch.nn.ReLU())


def test_everything_that_launches_raises_on_cpu():
    model = _hwgate()
    avg = optim.WeightAverage(model)
    before = [p.detach().clone() for p in model.parameters()]
    for launch in (avg.bind, avg.push, avg.update, avg.swap):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            launch()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with avg.applied():
            raise AssertionError("the body must not run")
    assert not avg.is_applied
    for name in ("n_averaged", "steps_seen", "coef"):
        with pytest.raises(RuntimeError, match="not run yet"):
            getattr(avg, name)
    assert all(torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))
    assert all(torch.equal(s, q) for s, q in zip(avg._shadow, before))
    # through an optimizer as well
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    holder = torch.nn.ParameterList([p])
    for cls, _, kw in OPTIMIZERS:
        o = cls([p], **kw)
        o.averager = optim.WeightAverage(holder)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            o.step()
        assert torch.equal(p.detach(), torch.zeros(4))


def test_state_dict_round_trip_on_cpu():
    torch.manual_seed(3)
    model = _stgcn()
    avg = optim.WeightAverage(model, mode="swa", decay=0.5, warmup=True, start=2, every=3)
    for s in avg._shadow:
        s.copy_(torch.randn_like(s))
    sd = avg.state_dict()
    assert {k: sd[k] for k in ("mode", "decay", "warmup", "start", "every", "buffers", "steps_seen", "n_averaged")} == dict(
        mode="swa", decay=0.5, warmup=True, start=2, every=3, buffers=True, steps_seen=0, n_averaged=0)
    assert list(sd["shadows"]) == avg.keys()
    assert all(v.data_ptr() != s.data_ptr() for v, s in zip(sd["shadows"].values(), avg._shadow))     # clones
    fh = io.BytesIO()
    torch.save(dict(sd, steps_seen=11, n_averaged=3), fh)
    fh.seek(0)
    back = torch.load(fh, weights_only=True)
    other = optim.WeightAverage(_stgcn())
    addresses = [s.data_ptr() for s in other._shadow]
    other.load_state_dict(back)
    assert (other.mode, other.decay, other.warmup, other.start, other.every) == ("swa", 0.5, True, 2, 3)
    assert other.counters() == dict(steps_seen=11, n_averaged=3)
    assert [s.data_ptr() for s in other._shadow] == addresses            # into the live tensors
    assert all(torch.equal(a, b) for a, b in zip(other._shadow, avg._shadow))
    again = other.state_dict()
    assert again["steps_seen"] == 11 and again["n_averaged"] == 3
    assert all(torch.equal(again["shadows"][k], sd["shadows"][k]) for k in sd["shadows"])
    # refused loads change nothing
    with pytest.raises(ValueError, match="decay"):
        other.load_state_dict(dict(back, decay=2.0))
    assert other.decay == 0.5
    with pytest.raises(ValueError, match="buffers"):
        optim.WeightAverage(_stgcn(), buffers=False).load_state_dict(back)
    wrong = dict(back, shadows={k: (torch.zeros(2, 3, 5, 7, 11) if i == 0 else v) for i, (k, v) in enumerate(back["shadows"].items())})
    with pytest.raises(ValueError, match="shape"):
        other.load_state_dict(wrong)


@pytest.mark.parametrize("build", [_hwgate, _stgcn], ids=["hwgate", "stgcn"])
def test_model_state_dict_has_the_models_keys_order_and_dtypes(build):
    model = build()
    avg = optim.WeightAverage(model)
    for s in avg._shadow:
        s.fill_(0.25)
    own, got = model.state_dict(), avg.model_state_dict()
    assert list(got.keys()) == list(own.keys())
    assert type(got) is type(own)
    shadowed = set(avg.keys())
    for k in own:
        assert got[k].dtype == own[k].dtype and got[k].shape == own[k].shape, k
        if k in shadowed:
            assert bool((got[k] == 0.25).all()) and got[k].data_ptr() not in [s.data_ptr() for s in avg._shadow], k
        else:
            assert torch.equal(got[k], own[k]), k
    fresh = build()
    fresh.load_state_dict(got)                               # strict: the same keys
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, got[k]), k


def test_averaged_weights_file_loads_through_load_weights_from_pretrained(tmp_path):
    model = _hwgate()
    avg = optim.WeightAverage(model)
    for s in avg._shadow:
        s.mul_(0.5)
    path = tmp_path / "averaged.pt"
    torch.save({"model_state_dict": avg.model_state_dict()}, path)
    report = {}
    fresh = ck.load_weights_from_pretrained(_hwgate(), str(path), report=report)
    assert report == dict(unknown=[], mismatched=[], missing=[])
    for (k, p), s in zip(fresh.named_parameters(), avg._shadow):
        assert torch.equal(p.detach(), s), k


@pytest.mark.parametrize("cls, like, kw", OPTIMIZERS, ids=["adamw", "sgd", "nadam"])
def test_an_averager_is_no_part_of_the_optimizers_state_dict(cls, like, kw):
    torch.manual_seed(0)
    theirs = [torch.nn.Parameter(torch.randn(s)) for s in ((3, 5), (7,))]
    o_t = like(theirs, **kw)
    for _ in range(2):
        for p in theirs:
            p.grad = torch.full_like(p, 0.25)
        o_t.step()
    mine = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone()) for p in theirs])
    plain, averaged = cls(list(mine), **kw), cls(list(mine), **kw)
    assert plain.averager is None
    averaged.averager = optim.WeightAverage(mine, decay=0.9)
    for o in (plain, averaged):
        o.load_state_dict(copy.deepcopy(o_t.state_dict()))
    a, b, t = plain.state_dict(), averaged.state_dict(), o_t.state_dict()
    assert a.keys() == b.keys() == t.keys()
    assert b["param_groups"][0].keys() == a["param_groups"][0].keys() == t["param_groups"][0].keys()
    assert "averager" not in averaged.param_groups[0] and "averager" not in averaged.defaults
    assert b["state"].keys() == t["state"].keys()
    for k in t["state"]:
        assert b["state"][k].keys() == a["state"][k].keys() == t["state"][k].keys()
        for name, v in t["state"][k].items():
            assert torch.equal(torch.as_tensor(b["state"][k][name]).float(), torch.as_tensor(v).float()), name
    # snapshot / restore with an averager that has not run: the shadows come back, nothing breaks
    snap = averaged.snapshot_state()
    for s in averaged.averager._shadow:
        s.zero_()
    averaged.restore_state(snap)
    assert all(torch.equal(s, p.detach()) for s, p in zip(averaged.averager._shadow, mine))
    assert averaged.averager.counters() == dict(steps_seen=0, n_averaged=0)


def test_get_device_optimizer_attaches_an_averager():
    model = _hwgate()
    for kind in ("adamw", "adam", "nadam", "sgd"):
        assert ck.get_device_optimizer(model, optimizer_type=kind).averager is None
        o = ck.get_device_optimizer(model, optimizer_type=kind, weight_average={})
        assert isinstance(o.averager, optim.WeightAverage) and o.averager.model is model and o.guard is None
        assert (o.averager.mode, o.averager.decay) == ("ema", 0.999)
        o = ck.get_device_optimizer(model, optimizer_type=kind, max_grad_norm=1.0,
                                    weight_average=dict(mode="swa", start=5, every=2))
        assert (o.averager.mode, o.averager.start, o.averager.every) == ("swa", 5, 2) and o.guard is not None
        plain = ck.get_device_optimizer(model, optimizer_type=kind)
        assert o.state_dict().keys() == plain.state_dict().keys()
        assert o.param_groups[0].keys() == plain.param_groups[0].keys()
    with pytest.raises(ValueError, match="decay"):
        ck.get_device_optimizer(model, weight_average=dict(decay=1.0))
