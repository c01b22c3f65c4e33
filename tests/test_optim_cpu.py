"""CPU: host logic of optim.DeviceAdamW -- the device table's layout, state_dict interchange with torch.optim.AdamW (the
reference's optimizer, hwgat/utils.py:71-82), argument errors, checkpoint.get_optimizer's new keyword."""
import ctypes
import importlib
import re

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
optim = importlib.import_module("sl-hwgat_amd.optim")
ck = hw.checkpoint
CHUNK = optim.CHUNK
NEW_SYMBOLS = {"hwgat_opt_set", "hwgat_opt_advance", "hwgat_opt_step"}


def _header_struct_bytes():
    """sizeof(hwgat_opt_entry) from the header's own text, laid out by ctypes with the C rules"""
    with open(hw._lib.HEADER) as fh:
        body = re.search(r"typedef struct \{([^}]*)\}\s*hwgat_opt_entry;", fh.read()).group(1)
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
    size, names = _header_struct_bytes()
    assert names == ["p", "g", "s0", "s1", "w0", "w1", "n", "group", "first_block"]
    assert optim.ENTRY_BYTES == optim.ENTRY.size == size == 64
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    assert "hwgat_optim_entry" not in src                    # the one record serves all three optimizers
    for name, val in (("OPTIM_CHUNK", optim.CHUNK), ("OPTIM_NHYPER", optim.NHYPER), ("OPT_NDERIVED", optim.NDERIVED)):
        assert int(re.search(rf"#define\s+HWGAT_{name}\s+(\d+)", src).group(1)) == val
    assert (optim.CHUNK, optim.NHYPER, optim.NDERIVED) == (4096, 8, 16)
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"HWGAT_OPT_(ADAMW|SGD|NADAM)\s*=\s*(\d+)", src)}
    assert kinds == dict(ADAMW=optim.KIND_ADAMW, SGD=optim.KIND_SGD, NADAM=optim.KIND_NADAM) == dict(ADAMW=0, SGD=1, NADAM=2)
    assert optim.DeviceAdamW._KIND == kinds["ADAMW"]


def test_entry_points_refuse_bad_arguments_without_launching():
    L = hw._lib.lib()                                        # bad arguments are refused before any HIP call
    buf = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)      # host memory: never dereferenced by a refused call
    kind = optim.KIND_ADAMW
    assert L.hwgat_opt_set(None, 0, kind, buf, None) == -1
    assert L.hwgat_opt_set(buf, 0, kind, None, None) == -1
    assert L.hwgat_opt_set(buf, -1, kind, buf, None) == -1
    for bad in (-1, 3):
        assert L.hwgat_opt_set(buf, 0, bad, buf, None) == -1
    advance, step = L.hwgat_opt_advance, L.hwgat_opt_step
    for guard in (buf, None):                                # a NULL guard is not what is refused: the other argument is
        assert advance(kind, buf, 0, buf, buf, guard, None) == -1
        assert advance(kind, buf, -1, buf, buf, guard, None) == -1
        for i in range(3):                                   # each non-nullable pointer in turn
            args = [buf, buf, buf]
            args[i] = None
            assert advance(kind, args[0], 1, args[1], args[2], guard, None) == -1, i
        assert step(kind, buf, 0, buf, 1, guard, None) == -1
        assert step(kind, buf, 1, buf, 0, guard, None) == -1
        assert step(kind, buf, 1, buf, -1, guard, None) == -1
        assert step(kind, None, 1, buf, 1, guard, None) == -1
        assert step(kind, buf, 1, None, 1, guard, None) == -1
        for bad in (-1, 3):
            assert advance(bad, buf, 1, buf, buf, guard, None) == -1
            assert step(bad, buf, 1, buf, 1, guard, None) == -1


def test_hyper_words_are_the_device_layout_and_decode_back():
    """{lr, beta1, beta2, eps, weight_decay, coupled, 0, 0}: `coupled` is the inverse of decoupled_weight_decay"""
    p = torch.nn.Parameter(torch.zeros(4))
    for decoupled, coupled in ((True, 0.0), (False, 1.0)):
        o = optim.DeviceAdamW([p], lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02, decoupled_weight_decay=decoupled)
        words = o._hyper_words(o._group_values(o.param_groups[0]))
        assert len(words) == optim.NHYPER == 8 and all(type(w) is float for w in words)
        assert tuple(words) == (3e-4, 0.8, 0.95, 1e-6, 0.02, coupled, 0.0, 0.0)
        assert o._decode_hyper(list(words)) == dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02,
                                                    decoupled_weight_decay=decoupled)


SIZES = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1]


def test_table_builder_prefix_sums_and_skipped_parameters():
    params = [torch.nn.Parameter(torch.zeros(n)) for n in SIZES] + [torch.nn.Parameter(torch.zeros(7))]
    opt = optim.DeviceAdamW([{"params": params[:2]}, {"params": params[2:], "lr": 3e-4}])
    for p in params[:-1]:
        p.grad = torch.ones_like(p)
    recs = opt.table_records()                               # the last parameter has no gradient: no entry, no state
    assert len(recs) == len(SIZES) and params[-1] not in opt.state
    assert [r[6] for r in recs] == SIZES and [r[7] for r in recs] == [0, 0, 1, 1, 1]
    for r, p in zip(recs, params):
        st = opt.state[p]
        assert r[:6] == (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                         st["step"].data_ptr(), 0)
        assert st["step"].shape == () and st["step"].dtype == torch.float32 and float(st["step"]) == 0.0
    blob, first, total = optim.build_table(recs)
    blocks = [-(-n // CHUNK) for n in SIZES]
    assert blocks == [1, 1, 1, 1, 2]
    assert first == [sum(blocks[:i]) for i in range(len(blocks))] and total == sum(blocks)
    assert len(blob) == len(recs) * optim.ENTRY_BYTES
    for i, r in enumerate(recs):                             # every record reads back field by field
        assert optim.ENTRY.unpack_from(blob, i * optim.ENTRY_BYTES) == r + (first[i],)
    params[1].grad = None                                    # a gradient that goes away leaves the table, keeps its state
    recs2 = opt.table_records()
    assert [r[6] for r in recs2] == [1, CHUNK - 1, CHUNK, CHUNK + 1] and params[1] in opt.state
    assert optim.build_table(recs2)[1] == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        optim.build_table([(8, 8, 8, 8, 8, 0, 0, 0)])       # an empty tensor
    blocks = 2 ** 30                                         # 2^31 workgroups are more than one launch holds
    assert optim.build_table([(8, 8, 8, 8, 8, 0, blocks * CHUNK, 0), (8, 8, 8, 8, 8, 0, (blocks - 1) * CHUNK, 0)])[2] == 2 ** 31 - 1
    with pytest.raises(ValueError, match="one launch"):
        optim.build_table([(8, 8, 8, 8, 8, 0, blocks * CHUNK, 0)] * 2)


def _stepped_torch_adamw(params, **kw):
    o = torch.optim.AdamW(params, **kw)
    for p in params[:-1]:                                    # the last one never gets a gradient (the frozen `B`)
        p.grad = torch.full_like(p, 0.25)
    o.step()
    o.step()
    return o


def _same_layout(a, b):
    assert a["param_groups"][0].keys() == b["param_groups"][0].keys()
    assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.shape == y.shape, (k, name)
            assert torch.equal(x.float(), y.float()), (k, name)


def test_state_dict_interchanges_with_torch_adamw_and_survives_a_checkpoint(tmp_path):
    torch.manual_seed(0)
    shapes = [(3, 5), (7,), (2, 2, 2), (4,)]
    theirs = [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    o_t = _stepped_torch_adamw(theirs, lr=2e-3, weight_decay=0.05)
    mine = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    o_m = optim.DeviceAdamW(mine)
    assert o_m.state_dict()["param_groups"][0].keys() == o_t.state_dict()["param_groups"][0].keys()
    # torch -> DeviceAdamW: values arrive, the step count becomes the 0-d fp32 tensor the kernels read
    o_m.load_state_dict(o_t.state_dict())
    assert o_m.param_groups[0]["lr"] == 2e-3 and o_m.param_groups[0]["weight_decay"] == 0.05
    assert 3 not in o_m.state_dict()["state"]                # no gradient, no state
    for p, q in zip(mine[:-1], theirs[:-1]):
        st = o_m.state[p]
        assert st["step"].dtype == torch.float32 and st["step"].shape == () and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], o_t.state[q]["exp_avg"]) and torch.equal(st["exp_avg_sq"], o_t.state[q]["exp_avg_sq"])
    # DeviceAdamW -> torch on CPU -> back
    sd = o_m.state_dict()
    o_t2 = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in theirs])
    o_t2.load_state_dict(sd)
    _same_layout(sd, o_t2.state_dict())
    o_m2 = optim.DeviceAdamW([torch.nn.Parameter(p.detach().clone()) for p in theirs])
    o_m2.load_state_dict(o_t2.state_dict())
    _same_layout(sd, o_m2.state_dict())
    # a second load goes INTO the live tensors (a captured graph's table holds their addresses)
    live = [o_m.state[p]["exp_avg"].data_ptr() for p in mine[:-1]] + [o_m.state[p]["step"].data_ptr() for p in mine[:-1]]
    o_m.load_state_dict(o_m2.state_dict())
    assert live == [o_m.state[p]["exp_avg"].data_ptr() for p in mine[:-1]] + [o_m.state[p]["step"].data_ptr() for p in mine[:-1]]
    _same_layout(sd, o_m.state_dict())
    # checkpoint.save_checkpoint -> load_checkpoint, unchanged code
    model = torch.nn.ParameterList(mine)
    sched = ck.get_scheduler(o_m)                            # (writes 'initial_lr' into the param group)
    sd = o_m.state_dict()
    path = str(tmp_path / "ck.pt")
    ck.save_checkpoint(path, model, o_m, sched, [0.1], [1.0], [0.2], [2.0], 3, 2e-3)
    model2 = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in shapes])
    o_m3 = optim.DeviceAdamW(list(model2.parameters()))
    sched3 = ck.get_scheduler(o_m3)
    _, o_back, _, lists, epoch = ck.load_checkpoint(path, model2, o_m3, sched3)
    assert epoch == 4 and lists == [[1.0], [2.0], [0.1], [0.2]]
    _same_layout(sd, o_back.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), model2.parameters()))


def test_argument_errors():
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="amsgrad"):
        optim.DeviceAdamW([p], amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.DeviceAdamW([p], maximize=True)
    for dtype in (torch.bfloat16, torch.float64, torch.float16):
        with pytest.raises(ValueError, match="float32"):
            optim.DeviceAdamW([torch.nn.Parameter(torch.zeros(4, dtype=dtype))])
    o = optim.DeviceAdamW([p])
    with pytest.raises(ValueError, match="float32"):
        o.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2, dtype=torch.bfloat16))]})
    emb = torch.nn.Embedding(8, 4, sparse=True)
    o = optim.DeviceAdamW(emb.parameters())
    emb(torch.tensor([1, 2])).sum().backward()
    assert emb.weight.grad.is_sparse
    with pytest.raises(ValueError, match="sparse"):
        o.table_records()
    o = optim.DeviceAdamW([p])
    o.param_groups[0]["amsgrad"] = True                      # e.g. out of a loaded state_dict
    with pytest.raises(ValueError, match="amsgrad"):
        o._group_values(o.param_groups[0])
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-0.1)):
        with pytest.raises(ValueError):
            optim.DeviceAdamW([p], **bad)


def test_step_on_cpu_parameters_raises():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optim.DeviceAdamW([p]).step()
    assert torch.equal(p.detach(), torch.zeros(4))


def test_get_optimizer_keyword():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 5}, 2, torch.device("cpu"), num_kps=32)
    model = hw.Model(*hp.get_model_params())
    n_all = len(list(model.parameters()))
    for kind, decoupled, wd in (("adamw", True, 1e-2), ("adam", False, 0.0)):
        o = ck.get_optimizer(model, lr=3e-4, optimizer_type=kind, device_step=True)
        assert isinstance(o, optim.DeviceAdamW) and len(o.param_groups) == 1
        grp = o.param_groups[0]
        assert len(grp["params"]) == n_all and grp["params"][0] is model.B          # ALL parameters, `B` is entry 0
        assert grp["lr"] == 3e-4 and grp["decoupled_weight_decay"] is decoupled and grp["weight_decay"] == wd
        assert grp["capturable"] is True
    for kind in ("nadam", "sgd"):
        with pytest.raises(ValueError, match="device_step"):
            ck.get_optimizer(model, optimizer_type=kind, device_step=True)
    # without the keyword: exactly what it returned before
    for kind, cls in (("adamw", torch.optim.AdamW), ("adam", torch.optim.Adam), ("nadam", torch.optim.NAdam),
                      ("sgd", torch.optim.SGD)):
        o = ck.get_optimizer(model, lr=3e-4, optimizer_type=kind)
        assert type(o) is cls and len(o.param_groups) == 1 and len(o.param_groups[0]["params"]) == n_all
        want = cls(list(model.parameters()), lr=3e-4)
        assert {k: v for k, v in o.param_groups[0].items() if k != "params"} == \
            {k: v for k, v in want.param_groups[0].items() if k != "params"}
    assert ck.get_optimizer(model, fused=False).param_groups[0]["fused"] is False
