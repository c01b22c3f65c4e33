"""The opt-in HIP classifier head (csrc/head.hip, functional.head_linear, DeviceSeeds._classify; reference: the `head` /
`classifier` nn.Linear of every model, hwgat/models/HWGATE.py:331,372) on the device.

Parity is entry by entry against the product formed on the CPU in float64, with a DERIVED bound.  With u = 2^-24 and n
the length of the reduction,

    |got - ref64| <= 1.01 (n + 2) u S + n 2^-126

where S is the same product over absolute values (Y: |x| |w|^T + |b|, n = K; dX: |dY| |w|, n = N; dW: |dY|^T |x|, n = M;
db: sum |dY|, n = M).  This is the standard bound of any fixed-order fp32 fused-multiply-add chain (the 1.01 keeps it
above the exact constant gamma_{n+1} up to the largest N, the floor covers flushed subnormals); a dropped k-slice or a
wrong row misses it by orders of magnitude.  torch's own fp32 CPU F.linear / mm stays within 0.38 of it on these inputs.

Measured on an MI355X (test 1's own print-out, the largest |got - ref64| / bound over the eleven shapes): Y 0.018, dX 0.255,
dW 0.392, db 0.215 (at K = 320 and 960 alone: Y 0.003, dX 0.130, dW 0.349, db 0.215; db over the nine other shapes 0.200);
the model logits of test 6 at most 0.003."""
import functools
import importlib

import pytest
import torch

import stgcn_helpers as SH
import transformer_helpers as TH
from test_gpu_graph import _batch, _build

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
optim = importlib.import_module("sl-hwgat_amd.optim")
train = importlib.import_module("sl-hwgat_amd.train")
DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 64), (1, 5, 64), (3, 15, 128), (16, 16, 64), (17, 17, 192), (4, 226, 512), (64, 2002, 512),
          (65, 33, 1024), (130, 100, 256), (17, 17, 320), (5, 226, 960)]     # the last two: K = 64 x odd above 192
CASES = [(s, True) for s in SHAPES] + [(SHAPES[1], False), (SHAPES[6], False)]
CASE_IDS = ["x".join(map(str, s)) + ("" if b else "-nobias") for s, b in CASES]
INVARIANCE_SHAPES = [(64, 2002, 512), (17, 17, 192), (17, 17, 320), (17, 33, 960)]
U = 2.0 ** -24
SENTINEL, PAD = -12345.0, 8


# ------------------------------------------------------------------------------------------ inputs, reference, bound
@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """seeded on the CPU; shared, never written"""
    M, N, K = shape
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    x = torch.randn(M, K, generator=g)
    w = 0.02 * torch.randn(N, K, generator=g)
    b = 0.1 * torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    if N > 7:
        w[7] *= 1e3
    if M > 2:
        x[2] = 0
    return x, w, b, dy


def _dense64(a, b):
    """a (I, R) times b (R, J) in float64 with every product formed: no library kernel between a non-finite operand and
    the result (small shapes only)"""
    return (a.double()[:, :, None] * b.double()[None, :, :]).sum(1)


def _products(x, w, b, dy, mm=torch.matmul):
    """{output: (float64 value, the same product over absolute values, reduction length)}"""
    M, K = x.shape
    N = w.shape[0]
    x, w, dy = x.double(), w.double(), dy.double()
    b = torch.zeros(N, dtype=torch.float64) if b is None else b.double()
    return {"Y": (mm(x, w.t()) + b, mm(x.abs(), w.abs().t()) + b.abs(), K),
            "dX": (mm(dy, w), mm(dy.abs(), w.abs()), N),
            "dW": (mm(dy.t(), x), mm(dy.abs().t(), x.abs()), M),
            "db": (dy.sum(0), dy.abs().sum(0), M)}


@functools.lru_cache(maxsize=None)
def _reference(shape, with_bias):
    x, w, b, dy = _inputs(shape)
    return _products(x, w, b if with_bias else None, dy)


def _bound(S, n):
    return 1.01 * (n + 2) * U * S + n * 2.0 ** -126


def _within_bound(got, ref, S, n, what, where=None):
    """entry by entry; `where` restricts the comparison (the finite entries of a non-finite case); returns the worst ratio"""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if where is None:
        where = torch.ones_like(ref, dtype=torch.bool)
    err, bound = (got - ref).abs()[where], _bound(S, n)[where]
    assert bool(torch.isfinite(got[where]).all()), what
    ratio = float((err / bound).max()) if err.numel() else 0.0
    print(f"{what}: n = {n}, largest |got - ref64| {float(err.max()) if err.numel() else 0.0:.3e}, largest err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


# ------------------------------------------------------------------------------------------ the three kernels, guarded
def _guarded(*shape):
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((PAD + n + PAD,), SENTINEL, device=DEV)
    view = buf[PAD:PAD + n].view(*shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return buf, view


def _kernels(x, w, b, dy, guarded=False):
    """the three direct kernel calls on device tensors; {output: tensor} and {output: (buffer, written length)}"""
    (M, K), N = x.shape, w.shape[0]
    shapes = {"Y": (M, N), "dX": (M, K), "dW": (N, K), "db": (N,)}
    bufs, out = {}, {}
    for k, s in shapes.items():
        bufs[k], out[k] = _guarded(*s) if guarded else (None, None)
    out["Y"] = HF.head_forward(x, w, b, out=out["Y"])
    out["dX"] = HF.head_backward_dx(dy, w, out=out["dX"])
    out["dW"], db = HF.head_backward_dw(dy, x, want_db=b is not None, out=out["dW"], out_db=out["db"] if b is not None else None)
    written = {k: (bufs[k], out[k].numel() if k != "db" or b is not None else 0) for k in shapes} if guarded else None
    out["db"] = db
    torch.cuda.synchronize()
    return out, written


@functools.lru_cache(maxsize=None)
def _device_run(shape, with_bias):
    x, w, b, dy = (t.to(DEV) for t in _inputs(shape))
    return _kernels(x, w, b if with_bias else None, dy, guarded=True)


# ------------------------------------------------------------------------------------------ 1, 2: parity and guards
@pytest.mark.parametrize("shape,with_bias", CASES, ids=CASE_IDS)
def test_kernels_against_float64(shape, with_bias):
    out, _ = _device_run(shape, with_bias)
    ref = _reference(shape, with_bias)
    assert (out["db"] is None) == (not with_bias)
    for name in ("Y", "dX", "dW") + (("db",) if with_bias else ()):
        _within_bound(out[name], *ref[name], f"{shape} {'bias' if with_bias else 'no bias'} {name}")


@pytest.mark.parametrize("shape,with_bias", CASES, ids=CASE_IDS)
def test_nothing_outside_the_outputs_is_written(shape, with_bias):
    out, written = _device_run(shape, with_bias)
    for name, (buf, n) in written.items():
        assert bool((buf[:PAD] == SENTINEL).all()), (name, "before")
        assert bool((buf[PAD + n:] == SENTINEL).all()), (name, "after" if n else "a NULL db was written")
        if n:
            assert not bool((buf[PAD:PAD + n] == SENTINEL).any()), (name, "an output entry was left unwritten")


# ------------------------------------------------------------------------------------------ 3: batch invariance
@pytest.mark.parametrize("shape", INVARIANCE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_do_not_depend_on_the_batch_and_runs_repeat(shape):
    M = shape[0]
    x, w, b, dy = (t.to(DEV) for t in _inputs(shape))
    full, _ = _kernels(x, w, b, dy)
    for m in (0, 15, 16, M - 1):
        assert torch.equal(HF.head_forward(x[m:m + 1], w, b)[0], full["Y"][m]), ("Y", m)
        assert torch.equal(HF.head_backward_dx(dy[m:m + 1].contiguous(), w)[0], full["dX"][m]), ("dX", m)
    parts = torch.cat([HF.head_forward(x[:3], w, b), HF.head_forward(x[3:], w, b)])
    assert torch.equal(parts, full["Y"])
    parts = torch.cat([HF.head_backward_dx(dy[:3], w), HF.head_backward_dx(dy[3:], w)])
    assert torch.equal(parts, full["dX"])
    again, _ = _kernels(x, w, b, dy)
    for name in ("Y", "dX", "dW", "db"):
        assert torch.equal(again[name], full[name]), name
    # and the guarded run of test 1 (other buffers, same inputs) has the same bits
    for name, t in _device_run(shape, True)[0].items():
        assert torch.equal(t, full[name]), name


# ------------------------------------------------------------------------------------------ 4: non-finite inputs
@pytest.mark.parametrize("inf_in_dy", [False, True], ids=["x-inf-w-nan", "and-dy-inf"])
def test_non_finite_inputs_propagate_as_in_the_dense_product(inf_in_dy):
    shape = (17, 17, 192)
    x, w, b, dy = (t.clone() for t in _inputs(shape))
    x[2, 5] = float("inf")
    w[7, 9] = float("nan")
    if inf_in_dy:
        dy[4, 3] = float("inf")
    ref = _products(x, w, b, dy, mm=_dense64)
    out, _ = _kernels(*(t.to(DEV) for t in (x, w, b, dy)))
    hit = 0
    for name in ("dX", "dW", "db") if inf_in_dy else ("Y", "dX", "dW", "db"):
        r, S, n = ref[name]
        got = out[name].cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(r)), (name, "nan mask")
        assert torch.equal(torch.isinf(got), torch.isinf(r)), (name, "inf mask")
        assert torch.equal(got[torch.isinf(r)].double(), r[torch.isinf(r)]), (name, "sign of an infinity")
        hit += int((~torch.isfinite(r)).sum())
        _within_bound(out[name], r, S, n, f"non-finite {name}", where=torch.isfinite(r))
    assert hit > 0


# ------------------------------------------------------------------------------------------ 5: the autograd node
@pytest.mark.parametrize("shape", [(17, 17, 192), (4, 226, 512)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_autograd_node_is_the_three_kernels(shape, with_bias):
    x, w, b, dy = (t.to(DEV) for t in _inputs(shape))
    direct, _ = _kernels(x, w, b if with_bias else None, dy)
    feat, weight = x.clone().requires_grad_(True), torch.nn.Parameter(w.clone())
    bias = torch.nn.Parameter(b.clone()) if with_bias else None
    y = HF.head_linear(feat, weight, bias)
    assert torch.equal(y.detach(), direct["Y"])
    y.backward(dy)
    assert torch.equal(feat.grad, direct["dX"]) and torch.equal(weight.grad, direct["dW"])
    assert feat.grad.is_contiguous() and weight.grad.is_contiguous() and weight.grad.dtype == torch.float32
    if with_bias:
        assert torch.equal(bias.grad, direct["db"])
    # a feature tensor that needs no gradient gets none (hwgat_head_bwd_dx is not launched); the others are unchanged
    launched = []
    real = HF.head_backward_dx
    feat2, weight2 = x.clone(), torch.nn.Parameter(w.clone())
    bias2 = torch.nn.Parameter(b.clone()) if with_bias else None
    y2 = HF.head_linear(feat2, weight2, bias2)
    HF.head_backward_dx = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        y2.backward(dy)
    finally:
        HF.head_backward_dx = real
    assert feat2.grad is None and not launched
    assert torch.equal(weight2.grad, direct["dW"]) and (not with_bias or torch.equal(bias2.grad, direct["db"]))
    # autograd accumulates a second backward as it does for nn.Linear
    HF.head_linear(feat2, weight2, bias2).backward(dy)
    assert torch.equal(weight2.grad, direct["dW"] + direct["dW"])


# ------------------------------------------------------------------------------------------ 6: models, eval
@functools.lru_cache(maxsize=None)
def _stgcn_weights(name):
    """computed once (a float64 restatement on the CPU calibrates the running statistics), shared, never written"""
    cfg = SH.CONFIGS[name]
    return SH.fixture_weights(hw.STGCNModel(*SH.model_args(cfg)).state_dict(), cfg)


def _stgcn(name="b", dropout=0.0):
    """test_gpu_stgcn._model at the smallest configuration of the ST-GCN tests"""
    cfg = SH.CONFIGS[name]
    m = hw.STGCNModel(*SH.model_args(cfg, dropout))
    m.load_state_dict(_stgcn_weights(name), strict=False)
    x, y = SH.make_input(cfg)
    return m.to(DEV), m.head.classifier, x.to(DEV), y.to(DEV)


def _transformer(name):
    cfg = TH.CONFIGS[name]
    m = hw.TransformerModel(*TH.model_args(cfg))
    m.load_state_dict(TH.recipe_weights(m.state_dict(), cfg["seed"]), strict=False)
    x, y = TH.make_input(cfg)
    return m.to(DEV), m.classifier, x.to(DEV), y.to(DEV)


def _hwgate(dtype):
    m = _build(dtype)
    with torch.no_grad():
        m.head.bias.normal_(0, 0.1, generator=torch.Generator(device=DEV).manual_seed(5))    # _finish zeroes it
    x, y = _batch(m)
    return m, m.head, x, y


EVAL_MODELS = {"hwgate-fp32": lambda: _hwgate(torch.float32), "hwgate-bf16": lambda: _hwgate(torch.bfloat16),
               "stgcn": _stgcn, "transformer-mean": lambda: _transformer("a")}


@pytest.mark.parametrize("name", list(EVAL_MODELS))
def test_model_eval_logits_are_the_float64_product_of_its_features(name):
    model, linear, x, _ = EVAL_MODELS[name]()
    model.eval()
    model.hip_head = True
    calls = []
    real = HF.head_linear
    HF.head_linear = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        with torch.no_grad():
            out, again = model(x), model(x)
            feat = model.forward_features(x)
    finally:
        HF.head_linear = real
    assert len(calls) == 2                                     # the head kernels ran, not the library
    assert feat.dtype == torch.float32 and out.shape == (x.shape[0], linear.out_features)
    assert torch.equal(out, again)
    ref = _products(feat.cpu(), linear.weight.detach().cpu(), linear.bias.detach().cpu(), torch.zeros(out.shape))["Y"]
    _within_bound(out, *ref, f"{name} logits")


def test_transformer_concat_head_stays_on_its_module(monkeypatch):
    model, classifier, x, _ = _transformer("b")
    assert isinstance(classifier, torch.nn.Sequential)

    def refuse(*a, **k):
        raise AssertionError("functional.head_linear must not be reached")
    monkeypatch.setattr(HF, "head_linear", refuse)
    model.eval()
    model.hip_head = True
    with torch.no_grad():
        out = model(x)
    assert out.shape == (x.shape[0], TH.CONFIGS["b"]["nclass"]) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------ 7: models, train
TRAIN_MODELS = {"hwgate-fp32": lambda: _hwgate(torch.float32), "hwgate-bf16": lambda: _hwgate(torch.bfloat16),
                "stgcn": lambda: _stgcn("b", dropout=0.05)}


@pytest.mark.parametrize("name", list(TRAIN_MODELS))
def test_whole_train_step_with_the_head_is_bit_equal_eager_and_graphed(name):
    """hip_head + deterministic_train + DeviceAdamW, three steps with a CosineAnnealingLR step after each: the same kernels
    run on the same bits eager and replayed, so every loss and every weight is equal"""
    steps, c0 = 3, 17
    runs = []
    for graphed in (False, True):
        torch.manual_seed(11)
        m, _, x, y = TRAIN_MODELS[name]()
        m.train()
        m.hip_head = True
        m.deterministic_train = True
        o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=20)
        m._drop_calls = c0
        calls = []
        real = HF.head_linear
        HF.head_linear = lambda *a, **k: calls.append(1) or real(*a, **k)
        try:
            s = train.GraphedTrainStep(m, o, x, y) if graphed else train.TrainStep(m, o, None)
            losses = []
            for _ in range(steps):
                losses.append(s(x, y).clone())
                sched.step()
        finally:
            HF.head_linear = real
        assert calls                                           # eager: once per step; graphed: at capture
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (le, we), (lg, wg) = runs
    print(name, "losses", [float(v) for v in le])
    for k in range(steps):
        assert torch.equal(le[k], lg[k]), (k, float(le[k]), float(lg[k]))
    assert float(le[-1]) < float(le[0])
    for n in we:
        assert torch.equal(we[n], wg[n]), n


# ------------------------------------------------------------------------------------------ 8: off means off
@pytest.mark.parametrize("name", ["hwgate-fp32", "stgcn"])
def test_switch_off_never_reaches_the_head_kernels(name, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("functional.head_linear must not be reached")
    monkeypatch.setattr(HF, "head_linear", refuse)
    m, _, x, y = TRAIN_MODELS[name]()
    assert m.hip_head is False
    m.train()
    o = optim.DeviceAdamW(list(m.parameters()), lr=5e-4)
    loss = train.TrainStep(m, o, None)(x, y)
    assert bool(torch.isfinite(loss))
    m.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(m(x)).all())
