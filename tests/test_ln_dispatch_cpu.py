"""CPU: functional.ln_backward, ln_mean_pool and ln_weighted_pool launch the entry point and the argument list that
include/hwgat_hip.h declares, for every combination of their options, and ln_backward returns exactly the members its
options ask for.  `call`, `ptr` and `stream` are replaced by recorders, so nothing is launched; the expected tuples below
are literals read off the header's parameter lists (P = a pointer argument, S = the stream).  The entry point a call goes
to is what the per-entry-point timers of bench.py and the launch counts of the GPU tests are keyed by."""
import importlib

import pytest
import torch

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional

P, S = "ptr", "stream"
F32, BF16 = 0, 1
N, D = 6, 128
WS_BYTES = 1024 * 2 * D * 4                 # hwgat_ln_bwd_det_bytes(128)
B, N_TOK = 2, 5
SEED, RATE = 7, 0.25


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(HF, "call", lambda name, *args: rec.append((name,) + args))
    monkeypatch.setattr(HF, "ptr", lambda t: None if t is None else P)
    monkeypatch.setattr(HF, "stream", lambda: S)
    return rec


# (deterministic, beta, mask) -> the entry point and its arguments after  dy, x, mean, rstd, gamma
LN_BWD = {
    # dres, dx, dgamma, dbeta, N, d, dtype, stream
    (False, False, False): ("hwgat_ln_bwd", (P, P, P, P, N, D, F32, S)),
    # dres, dx, dgamma, dbeta, N, d, dtype, dx_masked, mask_seed, mask_p, seed_base, stream
    (False, False, True): ("hwgat_ln_bwd_masked", (P, P, P, P, N, D, F32, P, 7, 0.25, P, S)),
    # beta, dres, dx, dgamma, dbeta, N, d, dtype, dx_masked, mask_seed, mask_p, xn, seed_base, stream
    (False, True, False): ("hwgat_ln_bwd_xn", (P, P, P, P, P, N, D, F32, None, 0, 0.0, P, P, S)),
    (False, True, True): ("hwgat_ln_bwd_xn", (P, P, P, P, P, N, D, F32, P, 7, 0.25, P, P, S)),
    # beta, dres, dx, dgamma, dbeta, N, d, dtype, dx_masked, mask_seed, mask_p, xn, seed_base, ws, ws_bytes, stream
    (True, False, False): ("hwgat_ln_bwd_det", (None, P, P, P, P, N, D, F32, None, 0, 0.0, None, P, P, WS_BYTES, S)),
    (True, False, True): ("hwgat_ln_bwd_det", (None, P, P, P, P, N, D, F32, P, 7, 0.25, None, P, P, WS_BYTES, S)),
    (True, True, False): ("hwgat_ln_bwd_det", (P, P, P, P, P, N, D, F32, None, 0, 0.0, P, P, P, WS_BYTES, S)),
    (True, True, True): ("hwgat_ln_bwd_det", (P, P, P, P, P, N, D, F32, P, 7, 0.25, P, P, P, WS_BYTES, S)),
}


def _ln_backward(det, with_beta, with_mask, dtype=torch.float32, dres=True, seed_base=True):
    x = torch.zeros(N, D, dtype=dtype)
    stat, vec = torch.zeros(N), torch.zeros(D)
    return x, HF.ln_backward(x, x, stat, stat, vec, x if dres else None, vec, vec,
                             mask=(SEED + 2 ** 32, RATE) if with_mask else None, beta=vec if with_beta else None,
                             seed_base=torch.zeros(1, dtype=torch.int32) if seed_base else None, deterministic=det)


@pytest.mark.parametrize("det,with_beta,with_mask", list(LN_BWD))
def test_ln_backward_entry_arguments_and_result(calls, det, with_beta, with_mask):
    x, out = _ln_backward(det, with_beta, with_mask)
    name, rest = LN_BWD[(det, with_beta, with_mask)]
    assert calls == [(name, P, P, P, P, P) + rest]                       # one launch
    if name != "hwgat_ln_bwd":                                           # mask_seed, mask_p follow dx_masked
        at = 14 + (name != "hwgat_ln_bwd_masked")
        assert type(calls[0][at]) is int and type(calls[0][at + 1]) is float
    assert isinstance(out, HF.LnGrads) and out._fields == ("dx", "dx_masked", "xn")
    assert (out.dx_masked is not None, out.xn is not None) == (with_mask, with_beta)
    for t in out:
        assert t is None or (t.shape == x.shape and t.dtype == x.dtype)
    assert len({t.data_ptr() for t in out if t is not None} | {x.data_ptr()}) == 2 + with_mask + with_beta


def test_ln_backward_optional_pointers_and_dtype(calls):
    _ln_backward(False, False, False, dtype=torch.bfloat16, dres=False)
    assert calls.pop() == ("hwgat_ln_bwd", P, P, P, P, P, None, P, P, P, N, D, BF16, S)
    _ln_backward(False, False, True, seed_base=False)                     # no device seed word: NULL
    assert calls.pop() == ("hwgat_ln_bwd_masked", P, P, P, P, P, P, P, P, P, N, D, F32, P, 7, 0.25, None, S)
    _ln_backward(True, False, False, dres=False, seed_base=False)
    assert calls.pop() == ("hwgat_ln_bwd_det", P, P, P, P, P, None, None, P, P, P, N, D, F32, None, 0, 0.0, None, None, P,
                           WS_BYTES, S)


@pytest.mark.parametrize("det", [False, True])
def test_layer_norm_backward_goes_through_ln_backward(calls, det):
    x = torch.zeros(N, D, requires_grad=True)
    HF.layer_norm(x, torch.ones(D), torch.zeros(D), deterministic=det).sum().backward()
    # x, gamma, beta, y, mean, rstd, N, d, dtype, stream
    assert calls[0] == ("hwgat_ln_fwd", P, P, P, P, P, P, N, D, F32, S)
    if det:                                                               # no beta, no residual gradient, no seed word
        assert calls[1:] == [("hwgat_ln_bwd_det", P, P, P, P, P, None, None, P, P, P, N, D, F32, None, 0, 0.0, None, None, P,
                              WS_BYTES, S)]
    else:
        assert calls[1:] == [("hwgat_ln_bwd", P, P, P, P, P, None, P, P, P, N, D, F32, S)]


# ---- the final LayerNorm + token pool
def _pool(weighted, det, up=None, dtype=torch.float32):
    x = torch.zeros(B, N_TOK, D, dtype=dtype, requires_grad=True)
    gamma, beta = torch.ones(D), torch.zeros(D)
    kw = dict(deterministic=det, seed_base=torch.zeros(1, dtype=torch.int32) if up else None)
    if up:
        kw.update(carrier=torch.zeros(1).expand(x.shape), up=up, book=HF.CarryBook())
    if weighted:
        return HF.ln_weighted_pool(x, gamma, beta, torch.zeros(1, N_TOK), torch.zeros(1), **kw)
    return HF.ln_mean_pool(x, gamma, beta, **kw)


POOL_FWD = {
    # x, xhat_sum, mean, rstd, B, n_tok, d, dtype, [partial,] stream
    (False, False): ("hwgat_lnpool_fwd", P, P, P, P, B, N_TOK, D, F32, S),
    (False, True): ("hwgat_lnpool_fwd_det", P, P, P, P, B, N_TOK, D, F32, P, S),
    # x, wtok, xhat_wsum, mean, rstd, B, n_tok, d, dtype, [partial,] stream
    (True, False): ("hwgat_lnwpool_fwd", P, P, P, P, P, B, N_TOK, D, F32, S),
    (True, True): ("hwgat_lnwpool_fwd_det", P, P, P, P, P, B, N_TOK, D, F32, P, S),
}
POOL_BWD = {
    # g, x, mean, rstd, dx, B, n_tok, d, dtype, dx_masked, mask_seed, mask_p, seed_base, stream
    (False, False): ("hwgat_lnpool_bwd_masked", P, P, P, P, P, B, N_TOK, D, F32, None, 0, 0.0, None, S),
    (False, True): ("hwgat_lnpool_bwd_masked", P, P, P, P, P, B, N_TOK, D, F32, P, 7, 0.25, P, S),
    # g, wtok, x, mean, rstd, dx, gdot, B, n_tok, d, dtype, dx_masked, mask_seed, mask_p, seed_base, stream
    (True, False): ("hwgat_lnwpool_bwd_masked", P, P, P, P, P, P, P, B, N_TOK, D, F32, None, 0, 0.0, None, S),
    (True, True): ("hwgat_lnwpool_bwd_masked", P, P, P, P, P, P, P, B, N_TOK, D, F32, P, 7, 0.25, P, S),
}


@pytest.mark.parametrize("weighted,det", list(POOL_FWD))
def test_pool_forward_entry_and_arguments(calls, weighted, det):
    feat = _pool(weighted, det)
    assert calls == [POOL_FWD[(weighted, det)]]
    assert feat.shape == (B, D) and feat.dtype == torch.float32


@pytest.mark.parametrize("weighted,with_up", list(POOL_BWD))
def test_pool_backward_entry_and_arguments(calls, weighted, with_up):
    _pool(weighted, False, up=(SEED + 2 ** 32, RATE) if with_up else None).sum().backward()
    assert calls[1:] == [POOL_BWD[(weighted, with_up)]]
    assert type(calls[1][-4]) is int and type(calls[1][-3]) is float


def test_pool_up_counts_only_with_carrier_book_and_rate(calls):
    """`up` without a carrier, a carrier without a book, a carrier of another shape and a zero rate: no masked copy"""
    x = torch.zeros(B, N_TOK, D, requires_grad=True)
    gamma, beta, car = torch.ones(D), torch.zeros(D), torch.zeros(1).expand(B, N_TOK, D)
    for kw in (dict(up=(SEED, RATE), book=HF.CarryBook()), dict(carrier=car, up=(SEED, RATE)),
               dict(carrier=car[:1], up=(SEED, RATE), book=HF.CarryBook()), dict(carrier=car, up=(SEED, 0.0), book=HF.CarryBook())):
        del calls[:]
        HF.ln_mean_pool(x, gamma, beta, **kw).sum().backward()
        assert calls[1:] == [POOL_BWD[(False, False)]], list(kw)


def test_pool_dtype_code_and_width_refusal(calls):
    _pool(False, True, dtype=torch.bfloat16)
    assert calls.pop() == ("hwgat_lnpool_fwd_det", P, P, P, P, B, N_TOK, D, BF16, P, S)
    with pytest.raises(NotImplementedError, match="width 192: the weighted token pool takes d in 128, 256, 512, 1024"):
        HF.ln_weighted_pool(torch.zeros(B, N_TOK, 192), torch.ones(192), torch.zeros(192), torch.zeros(N_TOK), torch.zeros(1))
    assert calls == []
