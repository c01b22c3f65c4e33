"""CPU: host logic of optim.DeviceSGD and optim.DeviceNAdam -- their hwgat_opt_entry records, state_dict interchange
with torch.optim.SGD / torch.optim.NAdam (the reference's cfg.optimizer_type 'sgd' / 'nadam', hwgat/utils.py:73-84),
argument errors, checkpoint.get_device_optimizer."""
import ctypes
import importlib
import re

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
optim = importlib.import_module("sl-hwgat_amd.optim")
ck = hw.checkpoint
CHUNK = optim.CHUNK
NEW_SYMBOLS = {f"hwgat_opt_{what}" for what in ("set", "advance", "step")}
KINDS = [(optim.DeviceSGD, "SGD"), (optim.DeviceNAdam, "NADAM")]
SIZES = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1]


def _header_struct_bytes(name):
    """sizeof(`name`) from the header's own text, laid out by ctypes with the C rules"""
    with open(hw._lib.HEADER) as fh:
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", fh.read()).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [n.strip() for n in decl.split(",")]
        base = names[0].rsplit(None, 1)[0] if "*" not in names[0] else names[0][:names[0].rindex("*") + 1]
        names[0] = names[0][len(base):].strip()
        ctype = ctypes.c_void_p if "*" in base else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[base.strip()]
        fields += [(n, ctype) for n in names]
    return ctypes.sizeof(type("E", (ctypes.Structure,), {"_fields_": fields})), [n for n, _ in fields]


def test_symbols_constants_and_record_size_follow_the_header():
    assert NEW_SYMBOLS <= set(hw._lib.declared_symbols())
    assert NEW_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_opt_")}
    assert not any(n.startswith(("hwgat_optim_", "hwgat_sgd_", "hwgat_nadam_")) for n in hw._lib._SIGS)
    L = hw._lib.lib()
    for name in NEW_SYMBOLS:                                 # exported by the library that was built
        assert getattr(L, name) is not None
    size, names = _header_struct_bytes("hwgat_opt_entry")
    assert names == ["p", "g", "s0", "s1", "w0", "w1", "n", "group", "first_block"]
    assert optim.ENTRY_BYTES == optim.ENTRY.size == size == 64
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    assert "hwgat_optim_entry" not in src                    # one record, one derived width
    assert int(re.search(r"#define\s+HWGAT_OPT_NDERIVED\s+(\d+)", src).group(1)) == optim.NDERIVED == 16
    assert (optim.CHUNK, optim.NHYPER) == (4096, 8)
    for cls, name in KINDS:
        assert cls._KIND == int(re.search(rf"HWGAT_OPT_{name}\s*=\s*(\d+)", src).group(1))


def test_entry_points_refuse_bad_arguments_without_launching():
    L = hw._lib.lib()
    buf = ctypes.cast((ctypes.c_double * 16)(), ctypes.c_void_p)     # host memory: never dereferenced by a refused call
    advance, step = L.hwgat_opt_advance, L.hwgat_opt_step
    for cls, _ in KINDS:
        kind = cls._KIND
        assert L.hwgat_opt_set(None, 0, kind, buf, None) == -1
        assert L.hwgat_opt_set(buf, 0, kind, None, None) == -1
        assert L.hwgat_opt_set(buf, -1, kind, buf, None) == -1
        for guard in (buf, None):                            # a NULL guard is not what is refused: the other argument is
            assert advance(kind, buf, 0, buf, buf, guard, None) == -1
            assert advance(kind, buf, -1, buf, buf, guard, None) == -1
            assert advance(kind, None, 1, buf, buf, guard, None) == -1
            assert advance(kind, buf, 1, None, buf, guard, None) == -1
            assert advance(kind, buf, 1, buf, None, guard, None) == -1
            assert step(kind, buf, 1, buf, 0, guard, None) == -1
            assert step(kind, buf, 1, buf, -1, guard, None) == -1
            assert step(kind, buf, 0, buf, 1, guard, None) == -1
            assert step(kind, buf, 1, None, 1, guard, None) == -1
            assert step(kind, None, 1, buf, 1, guard, None) == -1
    for bad in (-1, 3):
        assert L.hwgat_opt_set(buf, 0, bad, buf, None) == -1
        assert advance(bad, buf, 1, buf, buf, None, None) == -1
        assert step(bad, buf, 1, buf, 1, None, None) == -1


def test_hyper_words_are_the_device_layout_and_decode_back():
    """SGD {lr, momentum, dampening, weight_decay, nesterov, 0, 0, 0}; NAdam {lr, beta1, beta2, eps, weight_decay, coupled,
    momentum_decay, 0}, `coupled` the inverse of decoupled_weight_decay"""
    p = torch.nn.Parameter(torch.zeros(4))
    cases = [(optim.DeviceSGD, dict(lr=3e-2, momentum=0.8, dampening=0.0, weight_decay=0.02, nesterov=True),
              (3e-2, 0.8, 0.0, 0.02, 1.0, 0.0, 0.0, 0.0)),
             (optim.DeviceSGD, dict(lr=3e-2, momentum=0.8, dampening=0.25, weight_decay=0.02, nesterov=False),
              (3e-2, 0.8, 0.25, 0.02, 0.0, 0.0, 0.0, 0.0)),
             (optim.DeviceNAdam, dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02, momentum_decay=5e-3,
                                      decoupled_weight_decay=True), (3e-4, 0.8, 0.95, 1e-6, 0.02, 0.0, 5e-3, 0.0)),
             (optim.DeviceNAdam, dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02, momentum_decay=5e-3,
                                      decoupled_weight_decay=False), (3e-4, 0.8, 0.95, 1e-6, 0.02, 1.0, 5e-3, 0.0))]
    for cls, kw, want in cases:
        o = cls([p], **kw)
        words = o._hyper_words(o._group_values(o.param_groups[0]))
        assert len(words) == optim.NHYPER == 8 and all(type(w) is float for w in words)
        assert tuple(words) == want, kw
        assert o._decode_hyper(list(words)) == kw


def _two_groups(cls, **kw):
    params = [torch.nn.Parameter(torch.zeros(n)) for n in SIZES] + [torch.nn.Parameter(torch.zeros(7))]
    opt = cls([{"params": params[:2]}, {"params": params[2:], "lr": 3e-4}], **kw)
    for p in params[:-1]:
        p.grad = torch.ones_like(p)
    return params, opt


def _check_packing(recs):
    blob, first, total = optim.build_table(recs)
    blocks = [-(-n // CHUNK) for n in SIZES]
    assert blocks == [1, 1, 1, 1, 2]
    assert first == [sum(blocks[:i]) for i in range(len(blocks))] and total == sum(blocks)
    assert len(blob) == len(recs) * optim.ENTRY_BYTES
    for i, r in enumerate(recs):                             # every record reads back field by field
        assert optim.ENTRY.unpack_from(blob, i * optim.ENTRY_BYTES) == r + (first[i],)


def test_sgd_table_records_prefix_sums_and_skipped_parameters():
    params, opt = _two_groups(optim.DeviceSGD, momentum=0.9)
    recs = opt.table_records()                               # the last parameter has no gradient: no entry, no state
    assert len(recs) == len(SIZES) and params[-1] not in opt.state
    assert [r[6] for r in recs] == SIZES and [r[7] for r in recs] == [0, 0, 1, 1, 1]
    for r, p in zip(recs, params):
        st = opt.state[p]
        assert st.keys() == {"momentum_buffer"} and st["momentum_buffer"].shape == p.shape
        assert r[:4] == (p.data_ptr(), p.grad.data_ptr(), st["momentum_buffer"].data_ptr(), 0) and r[4] != 0 and r[5] == 0
    assert len({r[4] for r in recs}) == len(recs)            # every tensor its own "stepped before" word
    _check_packing(recs)
    params[1].grad = None                                    # a gradient that goes away leaves the table, keeps its state
    recs2 = opt.table_records()
    assert [r[6] for r in recs2] == [1, CHUNK - 1, CHUNK, CHUNK + 1] and params[1] in opt.state
    assert optim.build_table(recs2)[1] == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        optim.build_table([(8, 8, 8, 0, 8, 0, 0, 0)])
    # momentum 0 in one group: its tensors get null state pointers and NO state, as in torch
    params, opt = _two_groups(optim.DeviceSGD, momentum=0.9)
    opt.param_groups[0]["momentum"] = 0.0
    recs = opt.table_records()
    assert all(r[2:6] == (0, 0, 0, 0) for r in recs[:2]) and all(r[2] != 0 and r[4] != 0 for r in recs[2:])
    assert params[0] not in opt.state and params[1] not in opt.state and params[2] in opt.state
    params, opt = _two_groups(optim.DeviceSGD)               # the reference's call: no momentum anywhere, no state at all
    recs = opt.table_records()
    assert [r[6] for r in recs] == SIZES and all(r[2:6] == (0, 0, 0, 0) for r in recs) and len(opt.state) == 0
    assert opt.state_dict()["state"] == {}
    _check_packing(recs)


def test_nadam_table_records_prefix_sums_and_skipped_parameters():
    params, opt = _two_groups(optim.DeviceNAdam)
    recs = opt.table_records()
    assert len(recs) == len(SIZES) and params[-1] not in opt.state
    assert [r[6] for r in recs] == SIZES and [r[7] for r in recs] == [0, 0, 1, 1, 1]
    for r, p in zip(recs, params):
        st = opt.state[p]
        assert list(st.keys()) == ["step", "mu_product", "exp_avg", "exp_avg_sq"]
        assert r[:6] == (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                         st["step"].data_ptr(), st["mu_product"].data_ptr())
        for k, v in (("step", 0.0), ("mu_product", 1.0)):
            assert st[k].shape == () and st[k].dtype == torch.float32 and float(st[k]) == v
        assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())
    _check_packing(recs)


@pytest.mark.parametrize("cls, like, kw", [(optim.DeviceSGD, torch.optim.SGD, dict(lr=1e-2, momentum=0.9)),
                                           (optim.DeviceSGD, torch.optim.SGD, dict(lr=1e-2)),
                                           (optim.DeviceNAdam, torch.optim.NAdam, dict(lr=1e-3)),
                                           (optim.DeviceNAdam, torch.optim.NAdam, dict(decoupled_weight_decay=True))],
                         ids=["sgd-momentum", "sgd", "nadam", "nadam-decoupled"])
def test_param_group_keys_are_torchs(cls, like, kw):
    mine = cls([torch.nn.Parameter(torch.zeros(3))], **kw)
    theirs = like([torch.nn.Parameter(torch.zeros(3))], **kw)
    assert list(mine.param_groups[0].keys()) == list(theirs.param_groups[0].keys())
    assert mine.state_dict()["param_groups"][0].keys() == theirs.state_dict()["param_groups"][0].keys()
    for k, v in theirs.param_groups[0].items():
        if k not in ("params", "capturable"):
            assert mine.param_groups[0][k] == v, k
    if cls is optim.DeviceNAdam:
        assert mine.param_groups[0]["capturable"] is True
    else:
        assert "capturable" not in mine.param_groups[0]


CASES = [("sgd", optim.DeviceSGD, torch.optim.SGD, dict(lr=2e-3, momentum=0.9, weight_decay=0.05), {"momentum_buffer"}),
         ("nadam", optim.DeviceNAdam, torch.optim.NAdam, dict(lr=2e-3, weight_decay=0.05),
          {"step", "mu_product", "exp_avg", "exp_avg_sq"})]


def _same_layout(a, b, keys):
    assert a["param_groups"][0].keys() == b["param_groups"][0].keys()
    assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == keys
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.shape == y.shape, (k, name)
            assert torch.equal(x.float(), y.float()), (k, name)


@pytest.mark.parametrize("name, cls, like, kw, keys", CASES, ids=[c[0] for c in CASES])
def test_state_dict_interchanges_with_torch_and_survives_a_checkpoint(tmp_path, name, cls, like, kw, keys):
    torch.manual_seed(0)
    shapes = [(3, 5), (7,), (2, 2, 2), (4,)]
    theirs = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    o_t = like(theirs, **kw)
    for _ in range(2):
        for p in theirs[:-1]:                                # the last one never gets a gradient (the frozen `B`)
            p.grad = torch.full_like(p, 0.25)
        o_t.step()
    mine = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    o_m = cls(mine)
    # torch -> device class: values arrive in fp32 tensors of the right shapes
    o_m.load_state_dict(o_t.state_dict())
    assert o_m.param_groups[0]["lr"] == 2e-3 and o_m.param_groups[0]["weight_decay"] == 0.05
    assert 3 not in o_m.state_dict()["state"] and mine[-1] not in o_m.state           # no gradient, no state
    for p, q in zip(mine[:-1], theirs[:-1]):
        st = o_m.state[p]
        assert st.keys() == keys
        for k in keys:
            assert st[k].dtype == torch.float32 and torch.equal(st[k], o_t.state[q][k].float()), k
        if name == "nadam":
            assert st["step"].shape == () and float(st["step"]) == 2.0 and st["mu_product"].shape == ()
            assert 0.0 < float(st["mu_product"]) < 1.0
        else:
            assert float(o_m._live[p]["stepped"]) == 1.0     # a loaded buffer counts as stepped ...
            assert "stepped" not in st                       # ... and the word is no part of the state
    # device class -> torch on CPU -> back
    sd = o_m.state_dict()
    o_t2 = like([torch.nn.Parameter(p.detach().clone()) for p in theirs])
    o_t2.load_state_dict(sd)
    _same_layout(sd, o_t2.state_dict(), keys)
    o_m2 = cls([torch.nn.Parameter(p.detach().clone()) for p in theirs])
    o_m2.load_state_dict(o_t2.state_dict())
    _same_layout(sd, o_m2.state_dict(), keys)
    # a second load goes INTO the live tensors (a captured graph's table holds their addresses)
    def addresses():
        return [t.data_ptr() for p in mine[:-1] for t in o_m._live[p].values()]
    live = addresses()
    assert all(o_m.state[p][k].data_ptr() == o_m._live[p][k].data_ptr() for p in mine[:-1] for k in keys)
    o_m.load_state_dict(o_m2.state_dict())
    assert live == addresses()
    assert all(o_m.state[p][k].data_ptr() == o_m._live[p][k].data_ptr() for p in mine[:-1] for k in keys)
    _same_layout(sd, o_m.state_dict(), keys)
    # checkpoint.save_checkpoint -> load_checkpoint, unchanged code
    model = torch.nn.ParameterList(mine)
    sched = ck.get_scheduler(o_m)                            # (writes 'initial_lr' into the param group)
    sd = o_m.state_dict()
    path = str(tmp_path / "ck.pt")
    ck.save_checkpoint(path, model, o_m, sched, [0.1], [1.0], [0.2], [2.0], 3, 2e-3)
    model2 = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in shapes])
    o_m3 = cls(list(model2.parameters()))
    sched3 = ck.get_scheduler(o_m3)
    _, o_back, _, lists, epoch = ck.load_checkpoint(path, model2, o_m3, sched3)
    assert epoch == 4 and lists == [[1.0], [2.0], [0.1], [0.2]]
    _same_layout(sd, o_back.state_dict(), keys)
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), model2.parameters()))


def test_sgd_load_without_a_buffer_marks_the_tensor_fresh():
    p = torch.nn.Parameter(torch.zeros(4))
    o = optim.DeviceSGD([p], momentum=0.9)
    t = torch.optim.SGD([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, momentum=0.9)
    t.param_groups[0]["params"][0].grad = torch.ones(4)
    t.step()
    o.load_state_dict(t.state_dict())
    word, buf = o._live[p]["stepped"], o._live[p]["momentum_buffer"]
    assert float(word) == 1.0 and torch.equal(buf, torch.ones(4))
    fresh = torch.optim.SGD([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, momentum=0.9)
    o.load_state_dict(fresh.state_dict())                    # no momentum_buffer in it
    assert p not in o.state and o.state_dict()["state"] == {}
    assert o._live[p]["stepped"] is word and float(word) == 0.0
    p.grad = torch.ones(4)
    o.table_records()                                        # the next step's table: the same tensors again
    assert o.state[p]["momentum_buffer"] is buf and float(word) == 0.0


def test_snapshot_and_restore_cover_state_and_private_words():
    for cls, kw in ((optim.DeviceSGD, dict(momentum=0.9)), (optim.DeviceNAdam, {})):
        old, new = torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(4))
        o = cls([old, new], **kw)
        old.grad = torch.ones(4)
        o.table_records()
        for t in o._live[old].values():
            t.fill_(3.0)
        snap = o.snapshot_state()
        new.grad = torch.ones(4)
        o.table_records()                                    # `new` gets its state after the snapshot
        for q in (old, new):
            for t in o._live[q].values():
                t.fill_(7.0)
        o.restore_state(snap)
        assert all(bool((t == 3.0).all()) for t in o._live[old].values())
        for k, t in o._live[new].items():                    # fresh: zero, NAdam's mu_product one
            assert bool((t == (1.0 if k == "mu_product" else 0.0)).all()), k


def test_argument_errors():
    p = torch.nn.Parameter(torch.zeros(4))
    for cls in (optim.DeviceSGD, optim.DeviceNAdam):
        with pytest.raises(ValueError, match="maximize"):
            cls([p], maximize=True)
        with pytest.raises(ValueError, match="differentiable"):
            cls([p], differentiable=True)
        for dtype in (torch.bfloat16, torch.float64, torch.float16):
            with pytest.raises(ValueError, match="float32"):
                cls([torch.nn.Parameter(torch.zeros(4, dtype=dtype))])
        o = cls([p])
        with pytest.raises(ValueError, match="float32"):
            o.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.bfloat16))]})
        emb = torch.nn.Embedding(8, 4, sparse=True)
        o = cls(emb.parameters())
        emb(torch.tensor([1, 2])).sum().backward()
        assert emb.weight.grad.is_sparse
        with pytest.raises(ValueError, match="sparse"):
            o.table_records()
        o = cls([p])
        o.param_groups[0]["maximize"] = True                 # e.g. out of a loaded state_dict
        with pytest.raises(ValueError, match="maximize"):
            o._group_values(o.param_groups[0])
        for bad in (dict(lr=-1.0), dict(weight_decay=-0.1)):
            with pytest.raises(ValueError):
                cls([p], **bad)
    for bad in (dict(momentum=-0.5), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            optim.DeviceSGD([p], **bad)
    optim.DeviceSGD([p], nesterov=True, momentum=0.9)
    for bad in (dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            optim.DeviceNAdam([p], **bad)


@pytest.mark.parametrize("cls", [optim.DeviceSGD, optim.DeviceNAdam])
def test_step_on_cpu_parameters_raises(cls):
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cls([p]).step()
    assert torch.equal(p.detach(), torch.zeros(4))


def test_get_device_optimizer_and_get_optimizer():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, torch.device("cpu"), num_kps=32)
    model = hw.Model(*hp.get_model_params())
    n_all = len(list(model.parameters()))
    for kind, cls, like in (("adamw", optim.DeviceAdamW, torch.optim.AdamW), ("adam", optim.DeviceAdamW, torch.optim.Adam),
                            ("nadam", optim.DeviceNAdam, torch.optim.NAdam), ("sgd", optim.DeviceSGD, torch.optim.SGD)):
        o = ck.get_device_optimizer(model, lr=3e-4, optimizer_type=kind)
        assert type(o) is cls and isinstance(o, optim.DeviceOptimizer) and len(o.param_groups) == 1
        grp = o.param_groups[0]
        assert len(grp["params"]) == n_all and grp["params"][0] is model.B          # ALL parameters, `B` is entry 0
        want = like(list(model.parameters()), lr=3e-4).param_groups[0]               # what utils.get_optimizer would give
        assert grp.keys() == want.keys()
        for k, v in want.items():
            if k not in ("params", "capturable"):
                assert grp[k] == v, (kind, k)
        assert ("capturable" not in grp) if kind == "sgd" else grp["capturable"] is True
    assert ck.get_device_optimizer(model).param_groups[0]["lr"] == 5e-4
    assert type(ck.get_device_optimizer(model)) is optim.DeviceAdamW
    with pytest.raises(ValueError, match="optimizer_type"):
        ck.get_device_optimizer(model, optimizer_type="rmsprop")
    # get_optimizer: what it returned before, and the keyword still refuses the two types
    for kind in ("nadam", "sgd"):
        with pytest.raises(ValueError, match="device_step"):
            ck.get_optimizer(model, optimizer_type=kind, device_step=True)
    for kind, cls in (("adamw", torch.optim.AdamW), ("adam", torch.optim.Adam), ("nadam", torch.optim.NAdam),
                      ("sgd", torch.optim.SGD)):
        o = ck.get_optimizer(model, lr=3e-4, optimizer_type=kind)
        assert type(o) is cls and len(o.param_groups) == 1 and len(o.param_groups[0]["params"]) == n_all
    assert isinstance(ck.get_optimizer(model, device_step=True), optim.DeviceAdamW)
