"""CPU: the host side of the attention-map export (csrc/attn_probs.hip, functional.attn_probs, explain) -- the two entry
points in the header, the binding and the library, the element counts, every refusal of hwgat_attn_probs before a pointer
is looked at, and the plain-torch helpers of explain (window_frames, band_to_dense, fold_relevance, AttentionTap's
refusals)."""
import ctypes
import importlib

import pytest
import torch

from oracle import hwgat_oracle as O
from oracle import wgat_oracle as WO

hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
EX = hw.explain
CPU = torch.device("cpu")
SYMBOLS = {"hwgat_attn_probs", "hwgat_attn_probs_numel"}
EINVAL, ESHAPE, EDTYPE = -1, -2, -3
WIN, PWIN, BLK, BAND, WBAND = 0, 1, 2, 3, 4


def _buf():
    """aligned host memory standing in for a device pointer: never dereferenced, every call below is refused first"""
    keep = (ctypes.c_double * 64)()
    return keep, ctypes.cast(keep, ctypes.c_void_p)


def test_symbols_and_abi_follow_the_header():
    assert SYMBOLS <= set(hw._lib.declared_symbols())
    assert SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_attn_probs")}
    L = hw._lib.lib()
    for name in SYMBOLS:
        assert getattr(L, name) is not None
    assert L.hwgat_attn_probs_numel.restype is ctypes.c_int64
    assert L.hwgat_abi_version() == hw._lib.header_abi_version() == 4007
    assert HF.ATTN_PROBS_CODE == {"win": WIN, "pwin": PWIN, "blk": BLK, "band": BAND, "wband": WBAND}
    assert list(HF.ATTN_PROBS_CODE) == list(HF.ATTN_KINDS)


@pytest.mark.parametrize("kind,code,B,F,K,W,nH", [("win", WIN, 2, 4, 32, 16, 2), ("pwin", PWIN, 3, 6, 21, 7, 4),
                                                  ("blk", BLK, 2, 4, 29, 29, 2), ("band", BAND, 2, 5, 32, 16, 8),
                                                  ("wband", WBAND, 2, 5, 58, 29, 2)])
def test_numel(kind, code, B, F, K, W, nH):
    shape = HF.attn_probs_shape(kind, B, F, K, W, nH)
    nW = K // W
    assert shape == ((B, F // 2, nW, nH, 2 * W, 2 * W) if code <= BLK else (B, nW, nH, F, W, 3, W))
    assert hw._lib.lib().hwgat_attn_probs_numel(code, B, F, K, W, nH) == torch.Size(shape).numel()


def test_numel_past_32_bits_and_refused_shapes():
    L = hw._lib.lib()
    assert L.hwgat_attn_probs_numel(WIN, 512, 128, 64, 16, 8) == 512 * 64 * 4 * 8 * 1024      # 2^30: still an int
    assert L.hwgat_attn_probs_numel(PWIN, 4096, 128, 64, 32, 8) == 4096 * 64 * 2 * 8 * 4096   # 2^36
    for bad in ((5, 2, 4, 32, 16, 2), (WIN, 2, 3, 32, 16, 2), (PWIN, 2, 4, 30, 7, 2), (WBAND, 2, 4, 33, 33, 2)):
        assert L.hwgat_attn_probs_numel(*bad) == 0


GOOD = dict(kind=PWIN, B=2, F=4, K=14, W=7, nH=2, hd=32, shifted=1, dtype=0)


def _call(probs=True, received=True, **over):
    a = dict(GOOD, **over)
    keep, p = _buf()
    return hw._lib.lib().hwgat_attn_probs(a["kind"], p, p, p if probs else None, p if received else None, a["B"], a["F"],
                                          a["K"], a["W"], a["nH"], a["hd"], a["shifted"], a["dtype"], None)


@pytest.mark.parametrize("over,rc", [
    (dict(probs=False, received=False), EINVAL),                  # both outputs NULL
    (dict(kind=5), ESHAPE), (dict(kind=-1), ESHAPE),              # unknown kind
    (dict(F=3), ESHAPE), (dict(kind=WIN, K=32, W=16, F=5), ESHAPE), (dict(kind=BLK, K=7, F=1), ESHAPE),   # odd F, pair kinds
    (dict(K=15), ESHAPE), (dict(kind=WBAND, K=30, W=7, hd=16), ESHAPE),                                   # K % W != 0
    (dict(K=33, W=33), ESHAPE), (dict(kind=WBAND, K=33, W=33, hd=16), ESHAPE), (dict(W=0), ESHAPE),       # W outside 1..32
    (dict(hd=128), ESHAPE), (dict(kind=BLK, K=7, hd=128), ESHAPE), (dict(kind=WIN, K=32, W=16, hd=16), ESHAPE),
    (dict(kind=BAND, K=32, W=16, hd=64), ESHAPE), (dict(kind=WBAND, hd=64), ESHAPE),                      # head_dim per kind
    (dict(kind=WIN, K=32, W=8), ESHAPE), (dict(kind=BAND, K=32, W=8, hd=16), ESHAPE), (dict(kind=BLK, K=14), ESHAPE),
    (dict(B=0), ESHAPE), (dict(nH=0), ESHAPE),
    (dict(dtype=2), EDTYPE), (dict(dtype=-1), EDTYPE),            # unknown dtype
])
def test_refusals_before_any_pointer_is_touched(over, rc):
    assert _call(**over) == rc


def test_shapes_are_checked_before_pointers():
    """a bad shape with NULL everywhere is a shape refusal; a good shape with a NULL input is the pointer refusal"""
    L = hw._lib.lib()
    assert L.hwgat_attn_probs(PWIN, None, None, None, None, 2, 3, 14, 7, 2, 32, 0, 0, None) == ESHAPE
    keep, p = _buf()
    assert L.hwgat_attn_probs(PWIN, None, p, p, p, 2, 4, 14, 7, 2, 32, 0, 0, None) == EINVAL
    assert L.hwgat_attn_probs(PWIN, p, None, p, p, 2, 4, 14, 7, 2, 32, 0, 0, None) == EINVAL


def test_functional_refuses_through_the_kinds_own_dims_helper():
    qkv = torch.zeros(2, 4, 14, 3 * 2 * 48)
    bits = HF.pwin_mask_bits(torch.ones(2, 14, 14), 7)
    with pytest.raises(NotImplementedError, match="head_dim 48"):
        HF.attn_probs("pwin", qkv, bits, 2)
    with pytest.raises(ValueError, match="windows of 7 joints"):
        HF.attn_probs("pwin", torch.zeros(2, 4, 21, 3 * 64), bits, 2)
    with pytest.raises(ValueError):
        HF.attn_probs("pwin", qkv, bits, 2, probs=False, received=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # a CPU tensor never reaches the library
        HF.attn_probs("pwin", torch.zeros(2, 4, 14, 3 * 64), bits, 2)


# ------------------------------------------------------------------------------------------ explain: plain torch
@pytest.mark.parametrize("F", [2, 4, 10])
@pytest.mark.parametrize("shifted", [False, True])
def test_window_frames_is_the_roll_and_the_partition(F, shifted):
    frames = EX.window_frames(F, shifted)
    assert frames.shape == (F // 2, 2) and frames.dtype == torch.int64
    idx = torch.arange(F, dtype=torch.float32).view(1, F, 1, 1).expand(1, F, 16, 1)       # every token carries its frame
    x = torch.roll(idx, -1, 1) if shifted else idx
    win = O.to_windows(x.contiguous())                                                    # (1, f, 1, 32, 1)
    assert torch.equal(win[0, :, 0, :16, 0].long(), frames[:, :1].expand(F // 2, 16))
    assert torch.equal(win[0, :, 0, 16:, 0].long(), frames[:, 1:].expand(F // 2, 16))
    with pytest.raises(ValueError):
        EX.window_frames(5, False)


@pytest.mark.parametrize("F,W,nW", [(1, 16, 2), (4, 16, 2), (5, 3, 1)])
def test_band_to_dense_inverts_the_band_cut(F, W, nW):
    g = torch.Generator().manual_seed(F * 10 + W)
    B, nH = 2, 2
    if W == 16:
        adj = WO.band_adjacency(F, nW, torch.float64)
    else:
        eye = torch.eye(F)
        tri = ((eye + torch.roll(eye, 1, 1) + torch.roll(eye, -1, 1)) > 0).double()
        tri[0, F - 1] = tri[F - 1, 0] = 0
        adj = torch.kron(tri, torch.ones(W, W, dtype=torch.float64)).unsqueeze(0)
    s = torch.randn(B, nW, nH, F * W, F * W, generator=g, dtype=torch.float64)
    dense = torch.softmax(s + WO.additive_mask(adj)[None, :, None], dim=-1)              # 0 outside the adjacency in fp64
    for w in range(adj.shape[0]):
        assert bool((dense[:, w][:, :, adj[w] == 0] == 0).all())
    d6 = dense.view(B, nW, nH, F, W, F, W)
    band = torch.zeros(B, nW, nH, F, W, 3, W, dtype=torch.float64)
    for f in range(F):
        for t in range(3):
            if 0 <= f - 1 + t < F:
                band[:, :, :, f, :, t, :] = d6[:, :, :, f, :, f - 1 + t, :]
    back = EX.band_to_dense(band, F, W)
    assert back.shape == (B * nW, nH, F * W, F * W)
    assert torch.equal(back.view_as(dense), dense)
    with pytest.raises(ValueError):
        EX.band_to_dense(band, F + 1, W)


def test_fold_relevance_conserves_the_sum():
    g = torch.Generator().manual_seed(3)
    B, T, K = 2, 8, 6
    received = {0: torch.rand(B, 8, K, generator=g, dtype=torch.float64), 1: torch.rand(B, 4, K, generator=g, dtype=torch.float64),
                3: torch.rand(B, 2, K, generator=g, dtype=torch.float64)}
    mean_total = sum(r.sum((1, 2)) for r in received.values()) / 3
    # through upsampling: before the normalisation a map keeps its sum; after it every clip sums to 1
    one = EX.fold_relevance({1: received[1]}, T)
    assert one.shape == (B, T, K)
    assert torch.allclose(one * received[1].sum((1, 2)).view(B, 1, 1), received[1].repeat_interleave(2, 1) / 2, atol=1e-15)
    rel = EX.fold_relevance(received, T)
    assert torch.allclose(rel.sum((1, 2)), torch.ones(B, dtype=torch.float64), atol=1e-14)
    up = sum(r.repeat_interleave(T // r.shape[1], 1) / (T // r.shape[1]) for r in received.values()) / 3
    assert torch.allclose(up.sum((1, 2)), mean_total, atol=1e-13)
    assert torch.allclose(rel, up / mean_total.view(B, 1, 1), atol=1e-15)
    # through folding slots onto joints: slots of the same joint add, nothing is lost
    index = torch.tensor([0, 2, 2, 1, 0, 4], dtype=torch.int32)
    folded = EX.fold_relevance(received, T, index)
    assert folded.shape == (B, T, 5)
    assert torch.allclose(folded.sum((1, 2)), torch.ones(B, dtype=torch.float64), atol=1e-14)
    assert torch.allclose(folded[..., 0], rel[..., 0] + rel[..., 4], atol=1e-15)
    assert torch.allclose(folded[..., 2], rel[..., 1] + rel[..., 2], atol=1e-15)
    assert bool((folded[..., 3] == 0).all())
    assert EX.fold_relevance(received, T, index, num_joints=7).shape == (B, T, 7)
    with pytest.raises(ValueError):
        EX.fold_relevance({}, T)
    with pytest.raises(ValueError):
        EX.fold_relevance({0: torch.rand(B, 3, K)}, T)


def _hwgate():
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 7}, 2, CPU, num_kps=64)
    return hw.Model(*hp.get_model_params())


def test_attention_tap_refusals_and_restore():
    for Model, Params in ((hw.TransformerModel, hw.TransformerParams), (hw.STGCNModel, hw.STGCNParams)):
        other = Model(*Params({"src_len": 32, "num_class": 7}, 2, CPU).get_model_params())
        with pytest.raises(TypeError, match="attention"):
            EX.AttentionTap(other)
    model = _hwgate()
    n = len(model.block_list())
    with pytest.raises(ValueError):
        EX.AttentionTap(model, probs=False, received=False)
    with pytest.raises(IndexError):
        EX.AttentionTap(model, blocks=[n])
    tap = EX.AttentionTap(model.train(), blocks=[0, n - 1])
    with pytest.raises(RuntimeError, match="eval"):
        with tap:
            pass
    assert model.attention_tap is None
    model.eval()
    before = dict(vars(model))
    with tap:
        assert model.attention_tap is tap
        assert tap.hook(1, 2, False) is None and callable(tap.hook(0, 2, False))
        with pytest.raises(RuntimeError, match="already"):
            with EX.AttentionTap(model):
                pass
    assert model.attention_tap is None and dict(vars(model)).keys() == before.keys()
    with pytest.raises(ValueError, match="no attention map"):
        tap.clip_relevance()


def test_a_model_without_a_tap_hands_none_to_the_block(monkeypatch):
    """the seam is one default-None argument of block.fused_block: unarmed, the block gets None and calls nothing"""
    family = importlib.import_module("sl-hwgat_amd.models._family")
    seen = []

    def fake(h, *a, **kw):
        seen.append(kw.get("tap", "missing"))
        raise KeyboardInterrupt            # stop before any kernel: there is no GPU here

    monkeypatch.setattr(family, "fused_block", fake)
    model = _hwgate().eval()
    hand = HF.HandOver()
    h = torch.zeros(1, 16, 64, 128)
    with pytest.raises(KeyboardInterrupt):
        model._block(h, model.block_list()[0], 2, False, None, 0, hand)
    with EX.AttentionTap(model, blocks=[0]):
        with pytest.raises(KeyboardInterrupt):
            model._block(h, model.block_list()[0], 2, False, None, 0, hand)
    assert seen[0] is None and callable(seen[1])
