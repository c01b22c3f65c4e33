"""GPU: the fused block whose input needs no gradient (the first block: x comes from the parameter-free embedding) forms
norm1's and qkv's parameter gradients from G = dqkv^T xhat (hwgat_ln_param_grads_from_g) instead of a dX GEMM and a
LayerNorm-backward pass.  The same call with x.requires_grad_(True) takes the LayerNorm-backward path; both go against
an fp64 evaluation of the same block: oracle/hwgat_oracle.py's block with the masks the kernels hash
(hwgat_dropout_mask_f32) put in place of its random dropout, and a threshold no probability comes close to."""
import functools
import importlib

import pytest
import torch

from oracle import hwgat_oracle as O
from helpers import linear_parity, tensor_parity, tie_free_threshold

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
fb = importlib.import_module("sl-hwgat_amd.block")
HF = hw.functional
DEV = "cuda:0"
# the bounds of the kernels that deliver these gradients, copied from the tests of those kernels:
TOL = 2e-5                                                             # tests/test_gpu_gemm.py (norm-wise, fp32 outputs)
TN_F32 = dict(tol_entry=3.6e-6, tile=(128, 128), tol_tile=1.9e-6)      # tests/test_gpu_gemm.py: dW entry-wise / per tile, db entry-wise
LN_DG = 5.8e-6                                                         # tests/test_gpu_kernels.py, test_layernorm_model_widths_every_output_against_fp64:
#                                                                        dgamma / dbeta entry-wise (norm-wise F32_TOL = 2e-5 there)
D, HEADS, P, SEEDS = 128, 2, 0.1, (11, 22, 33, 44)
SHAPES = [(2, 4, 32), (7, 16, 32)]                                     # B, F, K: 256 tokens; 32 * 7 * 16 tokens (no power of two)
QKV = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias")   # what the new path computes differently


class _MaskedOracle(O.OracleHWGAT):
    """the oracle with its dropout sites (proj, fc1, fc2, in call order) multiplying by given masks"""

    def __init__(self, params, masks, **kw):
        super().__init__(params, **kw)
        self._masks = list(masks)

    def _drop(self, t):
        return t * self._masks.pop(0)


def _unmasked_p0(qkv):
    B, F, K, _ = qkv.shape
    hd = D // HEADS
    w = O.to_windows(qkv).reshape(B, F // 2, K // 16, 32, 3, HEADS, hd).permute(4, 0, 1, 2, 5, 3, 6)
    return torch.softmax((w[0] * hd ** -0.5) @ w[1].transpose(-2, -1), dim=-1)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """block, inputs and the fp64 parameter gradients of one shape: computed once, shared by the tests, never modified"""
    B, F, K = shape
    torch.manual_seed(5 + B)
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 3}, 2, DEV, num_kps=K)
    model = hw.Model(*hp.get_model_params()).to(DEV)
    blk = model.layers[0].blocks[0]
    g = torch.Generator().manual_seed(B * F * K)
    for n, q in blk.named_parameters():
        v = torch.randn(q.shape, generator=g) * (0.3 if "norm" in n else 0.1)
        q.data.copy_(v + 1.0 if n.endswith("norm1.weight") or n.endswith("norm2.weight") else v)
    x = torch.randn(B, F, K, D, generator=g) * (0.5 + torch.rand(B, F, K, 1, generator=g)) + torch.randn(B, F, K, 1, generator=g)
    cot = torch.randn(B, F, K, D, generator=g)
    hid = blk.ff.fc1.weight.shape[0]
    m1 = HF.dropout_mask((B, F, K, D), SEEDS[0], P, DEV).cpu().double()
    m2 = HF.dropout_mask((B, F, K, hid), SEEDS[1], P, DEV).cpu().double()
    m3 = HF.dropout_mask((B, F, K, D), SEEDS[2], P, DEV).cpu().double()
    pre = "layers.0.blocks.0."
    ref_p = {pre + n: q.detach().cpu().double().requires_grad_(True) for n, q in blk.named_parameters()}
    x64 = x.double()
    qkv64 = O.layer_norm(x64, ref_p[pre + "norm1.weight"], ref_p[pre + "norm1.bias"]) @ ref_p[pre + "attn.qkv.weight"].t() \
        + ref_p[pre + "attn.qkv.bias"]
    thr, margin = tie_free_threshold(_unmasked_p0(qkv64.detach()), 0.2)
    assert margin > 1e-4, (thr, margin)                               # fp32 scores are ~1e-6 off: the selector cannot flip
    # (the proj site drops in the window layout, HWGATE.py:115-116 before :207)
    oracle = _MaskedOracle(dict(ref_p, B=torch.zeros(1, dtype=torch.float64)), [O.to_windows(m1), m2, m3], num_kps=K, temporal_dim=F)
    out64, _ = oracle.block(x64, 0, 0, HEADS, thr)
    out64.backward(cot.double())
    ref = {n[len(pre):]: q.grad for n, q in ref_p.items()}
    return dict(model=model, blk=blk, x=x.to(DEV), cot=cot.to(DEV), thr=torch.tensor([thr], device=DEV), ref=ref,
                out=out64.detach())


def _call(c, x, det):
    return fb.fused_block(x, c["thr"], c["blk"], c["model"]._mask_bits, HEADS, False, P, SEEDS, kind="win",
                          deterministic=det, deterministic_backward=det)


def _run(c, need_dx, det, timers=None):
    for q in c["blk"].parameters():
        q.grad = None
    x = c["x"].clone().requires_grad_(need_dx)
    out = _call(c, x, det)
    HF.TIMERS = timers
    try:
        out.backward(c["cot"])
    finally:
        HF.TIMERS = None
    return out.detach(), x.grad, {n: q.grad.clone() for n, q in c["blk"].named_parameters()}


def _check_grads(grads, ref, what):
    assert len(grads) == len(ref) == 12
    for n, got in grads.items():
        if "norm" in n:
            tensor_parity(got, ref[n], tol_norm=TOL, tol_entry=LN_DG, what=f"{what}: {n}")
        else:
            linear_parity(got, ref[n], tol_norm=TOL, **TN_F32, what=f"{what}: {n}")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_parameter_gradients_of_both_paths_against_fp64(shape, det):
    """all 12 parameter gradients, with and without an input gradient, at the bounds of the kernels that deliver them;
    without one the input gradient is None, the d_xn GEMM and norm1's LayerNorm backward are not launched"""
    c = _case(shape)
    t_old, t_new = {}, {}
    out_old, dx_old, g_old = _run(c, True, det, t_old)
    out_new, dx_new, g_new = _run(c, False, det, t_new)
    if det:                                       # (the default forward adds its row statistics in arrival order)
        assert torch.equal(out_old, out_new)
    for out in (out_old, out_new):
        tensor_parity(out, c["out"], tol_norm=TOL, tol_entry=1e-5, what="block output")
    assert dx_old is not None and dx_new is None
    count = lambda t, *names: sum(len(t.get(n, ())) for n in names)
    assert count(t_new, "hwgat_ln_param_grads_from_g") == 1 and count(t_old, "hwgat_ln_param_grads_from_g") == 0
    assert count(t_new, "hwgat_linear_nt_f32", "hwgat_linear_nt_f32_ex") == count(t_old, "hwgat_linear_nt_f32", "hwgat_linear_nt_f32_ex") - 1
    assert count(t_new, "hwgat_ln_bwd", "hwgat_ln_bwd_det") == count(t_old, "hwgat_ln_bwd", "hwgat_ln_bwd_det") - 1 == 1
    _check_grads(g_old, c["ref"], f"{shape} det {det} with dx")
    _check_grads(g_new, c["ref"], f"{shape} det {det} without dx")


@pytest.mark.parametrize("shape", SHAPES)
def test_untouched_gradients_keep_their_bits_and_the_new_path_repeats_its_own(shape):
    """deterministic forward and backward: the gradients the change does not touch (eight, and the qkv bias, which both
    paths take from the same column sum) are bit-equal between the two paths, and the path without an input gradient
    returns the same bits on every run (all 12)"""
    c = _case(shape)
    _, _, g_old = _run(c, True, True)
    _, _, g_new = _run(c, False, True)
    _, _, g_again = _run(c, False, True)
    for n in g_old:
        if n not in QKV:
            assert torch.equal(g_old[n], g_new[n]), n
        assert torch.equal(g_new[n], g_again[n]), n
    # the bias gradient is the same column sum of the same launch geometry in both paths
    assert torch.equal(g_old["attn.qkv.bias"], g_new["attn.qkv.bias"])


def test_graphed_replay_equals_the_eager_call_bit_for_bit():
    """forward + backward without an input gradient captured in a HIP graph (deterministic mode): no host sync, no
    host-dependent value on the path -- a replay writes the eager call's bits"""
    c = _case(SHAPES[1])
    out_e, _, g_e = _run(c, False, True)
    params = list(c["blk"].parameters())
    names = [n for n, _ in c["blk"].named_parameters()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(_call(c, c["x"], True), params, c["cot"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _call(c, c["x"], True)
        grads = torch.autograd.grad(out, params, c["cot"])
    for t in (out,) + tuple(grads):
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), out_e)
    for n, got in zip(names, grads):
        assert torch.equal(got, g_e[n]), n


@pytest.mark.parametrize("N,K", [(384, 128), (100, 32), (5, 64)])
def test_ln_param_grads_from_g_against_fp64_and_accumulates(N, K):
    """the launch itself, at row counts that do not divide into its 8 row groups: sums of N terms per column in fp32
    (bound: the LayerNorm family's dgamma / dbeta and the dW entry bounds), adding to what the outputs already hold"""
    g = torch.Generator(device=DEV).manual_seed(N + K)
    G, W = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, K, device=DEV, generator=g)
    db, gamma, beta = (torch.randn(n, device=DEV, generator=g) for n in (N, K, K))
    dW0, dg0, db0 = (torch.randn(s, device=DEV, generator=g) for s in ((N, K), (K,), (K,)))
    dW, dg, dbt = dW0.clone(), dg0.clone(), db0.clone()
    HF.ln_param_grads_from_g(G, db, W, gamma, beta, dW, dg, dbt)
    G6, W6, d6 = G.double(), W.double(), db.double()
    tensor_parity(dW, dW0.double() + G6 * gamma.double() + d6[:, None] * beta.double(), tol_norm=TOL, tol_entry=TN_F32["tol_entry"],
                  what="from_g: dW")
    tensor_parity(dg, dg0.double() + (W6 * G6).sum(0), tol_norm=TOL, tol_entry=LN_DG, what="from_g: dgamma")
    tensor_parity(dbt, db0.double() + d6 @ W6, tol_norm=TOL, tol_entry=LN_DG, what="from_g: dbeta")
