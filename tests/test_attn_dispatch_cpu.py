"""CPU: functional.attn_fwd / attn_bwd launch the entry point and the argument list that include/hwgat_hip.h declares for
every attention kind, direction and dropout state.  `call`, `ptr` and `stream` are replaced by recorders, so nothing is
launched; the expected tuples below are literals read off the header's parameter lists (P = a pointer argument, S = the
stream), not computed by the table under test."""
import importlib

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional

P, S = "ptr", "stream"
F32, BF16 = 0, 1
SEED, RATE = 7, 0.25


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(HF, "call", lambda name, *args: rec.append((name,) + args))
    monkeypatch.setattr(HF, "ptr", lambda t: None if t is None else P)
    monkeypatch.setattr(HF, "stream", lambda: S)
    return rec


def _case(kind):
    """(o shape, mask, n_heads, shifted) of the case of `kind`"""
    return {
        "win": ((2, 4, 64, 128), torch.zeros(2, 4, 32, dtype=torch.int32), 4, True),
        "band": ((2, 4, 64, 128), torch.zeros(4, 16, dtype=torch.int64), 4, False),
        "blk": ((2, 4, 29, 128), torch.zeros(2, 64, 2, dtype=torch.int32), 4, True),
        "pwin8": ((2, 4, 32, 128), torch.zeros(2, 4, 16, dtype=torch.int64), 4, True),       # 4 windows of W = 8
        "pwin32": ((2, 4, 32, 128), torch.zeros(2, 1, 64, dtype=torch.int64), 4, False),     # one window of W = 32
        "wband8": ((2, 4, 32, 128), torch.zeros(4, 32, 3, dtype=torch.int32), 4, False),
        "wband32": ((2, 4, 32, 128), torch.zeros(1, 32, 3, dtype=torch.int32), 4, False),
    }[kind]


# the integer arguments between the pointers and the dropout triple, from the header: [.., shifted], dtype
INTS = {
    "win": (2, 4, 4, 4, 32, 1, F32),              # B, F, nW, nH, hd, shifted, dtype
    "band": (2, 4, 4, 4, 32, F32),                # B, F, nW, nH, hd, dtype
    "blk": (2, 4, 29, 4, 32, 1, F32),             # B, F, KJ, nH, hd, shifted, dtype
    "pwin8": (2, 4, 32, 8, 4, 32, 1, F32),        # B, F, K, W, nH, hd, shifted, dtype
    "pwin32": (2, 4, 32, 32, 4, 32, 0, F32),
    "wband8": (2, 4, 4, 8, 4, 32, F32),           # B, F, nW, W, nH, hd, dtype
    "wband32": (2, 4, 1, 32, 4, 32, F32),
}
STEM = {"win": "hwgat_win_attn", "band": "hwgat_band_attn", "blk": "hwgat_blk_attn", "pwin8": "hwgat_pwin_attn",
        "pwin32": "hwgat_pwin_attn", "wband8": "hwgat_wband_attn", "wband32": "hwgat_wband_attn"}
TAKES_THR = ("win", "pwin8", "pwin32")


def _launch(case, direction, drop, dtype=torch.float32):
    kind = case.rstrip("0123456789")
    shape, mask, n_heads, shifted = _case(case)
    qkv = torch.zeros(*shape[:3], 3 * shape[3], dtype=dtype)
    thr = torch.zeros(1) if (case in TAKES_THR and drop is not None) else None
    if direction == "fwd":
        HF.attn_fwd(kind, qkv, torch.zeros(shape, dtype=dtype), mask, thr, n_heads, shifted, drop)
    else:
        HF.attn_bwd(kind, qkv, torch.zeros(shape, dtype=dtype), torch.zeros_like(qkv), mask, thr, n_heads, shifted, drop)
    return thr


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("case", list(INTS))
def test_plain_entry_and_arguments(calls, case, direction):
    _launch(case, direction, None)
    tensors = (P, P) if direction == "fwd" else (P, P, P)                 # qkv, o | qkv, dO, dqkv
    thr = (None,) if case in TAKES_THR else ()                            # eval mode: a NULL threshold pointer
    assert calls == [(f"{STEM[case]}_{direction}",) + tensors + (P,) + thr + INTS[case] + (S,)]


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("case", list(INTS))
def test_dropout_entry_and_arguments(calls, case, direction):
    base = torch.zeros(1, dtype=torch.int32)
    _launch(case, direction, (SEED, RATE, base))
    tensors = (P, P) if direction == "fwd" else (P, P, P)
    thr = (P,) if case in TAKES_THR else ()
    assert calls == [(f"{STEM[case]}_{direction}_drop",) + tensors + (P,) + thr + INTS[case] + (7, 0.25, P, S)]
    assert type(calls[0][-4]) is int and type(calls[0][-3]) is float


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_dropout_without_seed_base_and_zero_rate(calls, direction):
    _launch("blk", direction, (SEED + 2 ** 32, RATE))                     # the seed is taken modulo 2^32, no base: NULL
    assert calls[-1][0] == f"hwgat_blk_attn_{direction}_drop" and calls[-1][-4:] == (7, 0.25, None, S)
    _launch("blk", direction, (SEED, 0.0, None))                          # p = 0: the plain entry
    assert calls[-1][0] == f"hwgat_blk_attn_{direction}" and calls[-1][-2:] == (F32, S)


def test_dtype_code_follows_qkv(calls):
    _launch("band", "fwd", None, torch.bfloat16)
    assert calls == [("hwgat_band_attn_fwd", P, P, P, 2, 4, 4, 4, 32, BF16, S)]


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_refusals(calls, direction):
    def run(kind, case, thr=None, shifted=False, drop=None):
        shape, mask, n_heads, _ = _case(case)
        qkv = torch.zeros(*shape[:3], 3 * shape[3])
        if direction == "fwd":
            HF.attn_fwd(kind, qkv, torch.zeros(shape), mask, thr, n_heads, shifted, drop)
        else:
            HF.attn_bwd(kind, qkv, torch.zeros(shape), torch.zeros_like(qkv), mask, thr, n_heads, shifted, drop)

    with pytest.raises(ValueError, match="^nope$"):
        run("nope", "win")
    for kind, case in (("win", "win"), ("pwin", "pwin8")):
        with pytest.raises(ValueError, match="attention dropout is a train-mode operation"):
            run(kind, case, drop=(SEED, RATE, None))
    for kind, case, msg in (("blk", "blk", "HGATE has no train-mode threshold"),
                            ("band", "band", "WGATE has neither threshold nor shift"),
                            ("wband", "wband8", "the band models have neither threshold nor shift")):
        with pytest.raises(AssertionError, match=msg):
            run(kind, case, thr=torch.zeros(1))
    for kind, case, msg in (("band", "band", "WGATE has neither threshold nor shift"),
                            ("wband", "wband8", "the band models have neither threshold nor shift")):
        with pytest.raises(AssertionError, match=msg):
            run(kind, case, shifted=True)
    assert calls == []


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_shape_checks_of_the_table_run_in_both_directions(calls, direction):
    """the mask / head_dim checks of 'pwin' and 'wband' keep their exception types and messages"""
    def run(kind, shape, mask, n_heads):
        qkv = torch.zeros(*shape[:3], 3 * shape[3])
        if direction == "fwd":
            HF.attn_fwd(kind, qkv, torch.zeros(shape), mask, None, n_heads, False)
        else:
            HF.attn_bwd(kind, qkv, torch.zeros(shape), torch.zeros_like(qkv), mask, None, n_heads, False)

    with pytest.raises(ValueError, match=r"'pwin' attention needs the \(2, nW, 2W\) int64 rows"):
        run("pwin", (2, 4, 32, 128), torch.zeros(2, 4, 16, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="mask rows are for 4 windows of 8 joints, activations have 24 joints"):
        run("pwin", (2, 4, 24, 128), torch.zeros(2, 4, 16, dtype=torch.int64), 4)
    with pytest.raises(NotImplementedError, match="head_dim 16: the part-window attention kernels"):
        run("pwin", (2, 4, 32, 128), torch.zeros(2, 4, 16, dtype=torch.int64), 8)
    with pytest.raises(ValueError, match=r"'wband' attention needs the \(nW, 32, 3\) int32 words"):
        run("wband", (2, 4, 32, 128), torch.zeros(4, 32, 2, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="mask words are for 3 windows, activations have 32 joints per frame"):
        run("wband", (2, 4, 32, 128), torch.zeros(3, 32, 3, dtype=torch.int32), 4)
    with pytest.raises(NotImplementedError, match="head_dim 64: the wide band attention kernels take head_dim 16 or 32"):
        run("wband", (2, 4, 32, 128), torch.zeros(4, 32, 3, dtype=torch.int32), 2)
    assert calls == []


def test_table_has_the_five_kinds():
    assert set(HF.ATTN_KINDS) == {"win", "pwin", "blk", "band", "wband"}
    assert {k: (r.takes_thr, r.takes_shifted) for k, r in HF.ATTN_KINDS.items()} == {
        "win": (True, True), "pwin": (True, True), "blk": (False, True), "band": (False, False), "wband": (False, False)}
