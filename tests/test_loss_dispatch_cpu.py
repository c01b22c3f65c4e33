"""CPU: the launchers of the cross-entropy family (sce_* / bsce_* / mbsce_* / kd_* of functional.py) go to the entry point
and pass the argument list that include/hwgat_hip.h declares, for each of the input forms: the whole batch without and
with n_valid, a slice, a slice with a pair target, a slice with a teacher (without and with a pair).  `call`, `ptr` and
`stream` are replaced by recorders, so nothing is launched and the tensors are host tensors; the expected tuples below are
literals read off the header's parameter lists (P = a pointer argument, S = the stream).  The entry point a call goes to is
what the per-entry-point timers of bench.py and the launch counts of the GPU tests are keyed by."""
import importlib

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional

P, S = "ptr", "stream"
B, C, EPS, OFF = 6, 10, 0.25, 3


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(HF, "call", lambda name, *args: rec.append((name,) + args))
    monkeypatch.setattr(HF, "ptr", lambda t: None if t is None else P)
    monkeypatch.setattr(HF, "stream", lambda: S)
    return rec


def _inputs():
    return dict(z=torch.zeros(B, C), u=torch.zeros(B, C), y=torch.zeros(B, dtype=torch.int64),
                y_b=torch.zeros(B, dtype=torch.int64), lam=torch.ones(B), n=torch.zeros(1, dtype=torch.int32),
                st=torch.zeros(HF.KD_STATE_WORDS), lse=torch.zeros(B), g=torch.ones(1))


TAIL = (B, C, EPS, S)
FWD = {
    # logits, target, n_valid, lse, row_loss, rank, pred, loss
    "batch": ("hwgat_sce_fwd", (P, P, None, P, P, P, P, P) + TAIL, 5),
    "batch n_valid": ("hwgat_sce_fwd", (P, P, P, P, P, P, P, P) + TAIL, 5),
    # logits, target, n_rows, offset, lse, row_loss, rank, pred, loss, correct, live
    "slice": ("hwgat_bsce_fwd", (P, P, P, OFF, P, P, P, P, P, P, P) + TAIL, 7),
    # logits, target, target_b, lam, n_rows, offset, lse, row_loss, rank, pred, loss, correct, live, row_loss_b, rank_b
    "slice pair": ("hwgat_mbsce_fwd", (P, P, P, P, P, OFF, P, P, P, P, P, P, P, P, P) + TAIL, 9),
    # logits, teacher, target, target_b, lam, n_rows, offset, state, lse, row_loss, rank, pred, loss, correct, live,
    # row_loss_b, rank_b, lse_s, lse_t, row_kd, t_pred, kd, agree, t_correct
    "slice teacher": ("hwgat_kd_fwd", (P, P, P, None, None, P, OFF, P, P, P, P, P, P, P, P, None, None, P, P, P, P, P, P, P)
                      + TAIL, 16),
    "slice teacher pair": ("hwgat_kd_fwd", (P, P, P, P, P, P, OFF, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P) + TAIL, 16),
}
BWD = {
    # logits, target, n_valid, lse, g, dlogits
    "batch": ("hwgat_sce_bwd", (P, P, None, P, P, P) + TAIL),
    "batch n_valid": ("hwgat_sce_bwd", (P, P, P, P, P, P) + TAIL),
    # logits, target, n_rows, offset, lse, g, dlogits
    "slice": ("hwgat_bsce_bwd", (P, P, P, OFF, P, P, P) + TAIL),
    # logits, target, target_b, lam, n_rows, offset, lse, g, dlogits
    "slice pair": ("hwgat_mbsce_bwd", (P, P, P, P, P, OFF, P, P, P) + TAIL),
    # logits, teacher, target, target_b, lam, n_rows, offset, state, lse, lse_s, lse_t, g, dlogits
    "slice teacher": ("hwgat_kd_bwd", (P, P, P, None, None, P, OFF, P, P, P, P, P, P) + TAIL),
    "slice teacher pair": ("hwgat_kd_bwd", (P, P, P, P, P, P, OFF, P, P, P, P, P, P) + TAIL),
}


def _forward(form, t):
    if form.startswith("batch"):
        return HF.sce_forward(t["z"], t["y"], EPS, t["n"] if "n_valid" in form else None)
    pair = (t["y_b"], t["lam"]) if "pair" in form else (None, None)
    if "teacher" in form:
        return HF.kd_forward(t["z"], t["u"], t["y"], *pair, t["st"], EPS, t["n"], OFF)
    if "pair" in form:
        return HF.mbsce_forward(t["z"], t["y"], *pair, EPS, t["n"], OFF)
    return HF.bsce_forward(t["z"], t["y"], EPS, t["n"], OFF)


def _backward(form, t):
    if form.startswith("batch"):
        return HF.sce_backward(t["z"], t["y"], t["lse"], t["g"], EPS, t["n"] if "n_valid" in form else None)
    pair = (t["y_b"], t["lam"]) if "pair" in form else (None, None)
    if "teacher" in form:
        return HF.kd_backward(t["z"], t["u"], t["y"], *pair, t["st"], t["lse"], t["lse"], t["lse"], t["g"], EPS, t["n"], OFF)
    if "pair" in form:
        return HF.mbsce_backward(t["z"], t["y"], *pair, t["lse"], t["g"], EPS, t["n"], OFF)
    return HF.bsce_backward(t["z"], t["y"], t["lse"], t["g"], EPS, t["n"], OFF)


@pytest.mark.parametrize("form", list(FWD))
def test_forward_entry_arguments_and_result(calls, form):
    name, args, members = FWD[form]
    out = _forward(form, _inputs())
    assert calls == [(name,) + args]                                     # one call
    assert type(calls[0][-2]) is float and ("slice" not in form or type(calls[0][args.index(OFF) + 1]) is int)
    assert isinstance(out, tuple) and len(out) == members
    loss, row_loss, lse, rank, pred = out[:5]
    assert loss.shape == (1,) and loss.dtype == torch.float32
    assert all(v.shape == (B,) and v.dtype == torch.float32 for v in (row_loss, lse) + out[7:8] + out[9:12])
    assert all(v.shape == (B,) and v.dtype == torch.int32 for v in (rank, pred) + out[8:9] + out[12:13])
    if members > 5:
        assert out[5].shape == (1,) and out[5].dtype == torch.int64 and out[6].shape == (1,) and out[6].dtype == torch.int32
    if members == 16:
        assert out[13].shape == (1,) and out[13].dtype == torch.float32
        assert all(v.shape == (1,) and v.dtype == torch.int64 for v in out[14:])
    # no two members share memory
    spans = sorted((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size()) for v in out)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("form", list(BWD))
def test_backward_entry_arguments_and_result(calls, form):
    name, args = BWD[form]
    t = _inputs()
    dz = _backward(form, t)
    assert calls == [(name,) + args]                                     # one call
    assert dz.shape == (B, C) and dz.dtype == torch.float32 and dz.data_ptr() != t["z"].data_ptr()


def test_out_is_used_as_given(calls):
    t = _inputs()
    given = HF.bsce_forward(t["z"], t["y"], EPS, t["n"], OFF)
    assert HF.bsce_forward(t["z"], t["y"], EPS, t["n"], OFF, out=given) is given
    dz = torch.zeros(B, C)
    assert HF.bsce_backward(t["z"], t["y"], t["lse"], t["g"], EPS, t["n"], OFF, out=dz) is dz
    assert [c[0] for c in calls] == ["hwgat_bsce_fwd", "hwgat_bsce_fwd", "hwgat_bsce_bwd"]


@pytest.mark.parametrize("form,results", [("batch", 3), ("slice", 4), ("slice pair", 4), ("slice teacher", 8),
                                          ("slice teacher pair", 8)])
def test_autograd_entries_keep_their_results_and_launch_once_each_way(calls, form, results):
    t = _inputs()
    z = t["z"].requires_grad_()
    pair = (t["y_b"], t["lam"]) if "pair" in form else (None, None)
    if form == "batch":
        out = HF.smooth_ce(z, t["y"], EPS)
    elif "teacher" in form:
        out = HF.distilled_sliced_ce(z, t["u"], t["y"], *pair, t["st"], EPS, t["n"], OFF)
    elif "pair" in form:
        out = HF.mixed_sliced_ce(z, t["y"], *pair, EPS, t["n"], OFF)
    else:
        out = HF.batch_sliced_ce(z, t["y"], EPS, t["n"], OFF)
    assert len(out) == results and out[0].shape == () and out[0].requires_grad
    assert not any(v.requires_grad for v in out[1:])
    assert all(v.shape == () for v in out[3:4] + out[5:])                # correct; kd, agree, t_correct
    out[0].backward()
    assert calls == [(FWD[form][0],) + FWD[form][1], (BWD[form][0],) + BWD[form][1]]
    assert z.grad.shape == (B, C)


def test_refusals(calls):
    t = _inputs()
    z, u, y, y_b, lam, n, st = (t[k] for k in ("z", "u", "y", "y_b", "lam", "n", "st"))
    for pair in ((y_b, None), (None, lam)):
        with pytest.raises(ValueError, match="target_b and lam come together"):
            HF.kd_forward(z, u, y, *pair, st, EPS, n, OFF)
        with pytest.raises(ValueError, match="target_b and lam come together"):
            HF.kd_backward(z, u, y, *pair, st, t["lse"], t["lse"], t["lse"], t["g"], EPS, n, OFF)
    with pytest.raises(ValueError, match=r"logits must be fp32 \(B, C\)"):
        HF.sce_forward(z.double(), y, EPS)
    with pytest.raises(ValueError, match=r"logits must be fp32 \(B, C\)"):
        HF.sce_forward(z[0], y, EPS)
    with pytest.raises(ValueError, match=r"target must be int64 \(B,\)"):
        HF.sce_backward(z, y.int(), t["lse"], t["g"], EPS)
    with pytest.raises(ValueError, match=r"target must be int64 \(B,\)"):
        HF.bsce_forward(z, y[:-1], EPS, n, OFF)
    for bad_n in (None, n.long(), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="n_rows must be a device int32 tensor of one element"):
            HF.bsce_forward(z, y, EPS, bad_n, OFF)
    for bad_off in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="the slice's offset must be in"):
            HF.mbsce_backward(z, y, y_b, lam, t["lse"], t["g"], EPS, n, bad_off)
    for bad_b in (y_b.int(), y_b[:-1]):
        with pytest.raises(ValueError, match="target_b must be int64"):
            HF.mbsce_forward(z, y, bad_b, lam, EPS, n, OFF)
    for bad_lam in (lam.double(), lam[:-1]):
        with pytest.raises(ValueError, match="lam must be fp32"):
            HF.kd_forward(z, u, y, y_b, bad_lam, st, EPS, n, OFF)
    for bad_u in (u.double(), u[:, :-1]):
        with pytest.raises(ValueError, match="teacher must be fp32"):
            HF.kd_forward(z, bad_u, y, None, None, st, EPS, n, OFF)
    for bad_st in (st.double(), torch.zeros(HF.KD_STATE_WORDS + 1)):
        with pytest.raises(ValueError, match="the distillation state must be fp32"):
            HF.kd_backward(z, u, y, None, None, bad_st, t["lse"], t["lse"], t["lse"], t["g"], EPS, n, OFF)
    # the pair form without its pair and the teacher form without its teacher do not quietly become a smaller form
    for pair in ((None, None), (y_b, None), (None, lam)):
        with pytest.raises(ValueError, match="mbsce_forward needs"):
            HF.mbsce_forward(z, y, *pair, EPS, n, OFF)
        with pytest.raises(ValueError, match="mbsce_backward needs"):
            HF.mbsce_backward(z, y, *pair, t["lse"], t["g"], EPS, n, OFF)
    with pytest.raises(ValueError, match="kd_forward needs teacher"):
        HF.kd_forward(z, None, y, y_b, lam, st, EPS, n, OFF)
    with pytest.raises(ValueError, match="kd_backward needs state and lse_t"):
        HF.kd_backward(z, u, y, y_b, lam, None, t["lse"], t["lse"], None, t["g"], EPS, n, OFF)
    # an unpaired record is refused before a bad tensor is looked at, as a bad tensor is before a bad record of a later kind
    with pytest.raises(ValueError, match="target_b and lam come together"):
        HF.kd_forward(z.double(), u, y, y_b, None, st, EPS, n, OFF)
    with pytest.raises(ValueError, match="n_rows must be"):
        HF.kd_forward(z, u.double(), y, y_b.int(), lam, st, EPS, None, OFF)
    with pytest.raises(ValueError, match="target_b must be"):
        HF.kd_forward(z, u.double(), y, y_b.int(), lam, st, EPS, n, OFF)
    assert calls == []
