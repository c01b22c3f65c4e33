"""GPU: the train-mode contract one layer above the kernels -- which dropout masks a backward regenerates when train
forwards interleave, what a graphed step does under an lr schedule, and the host mirror of the device seed counter.

Every seeded kernel hashes site seed + a base-seed word it reads from the device when it runs, and a backward
regenerates the proj / fc2 / attention / LayerNorm-backward masks instead of storing them.  So the word a backward reads
must be the one its OWN forward used, not the one a later train forward wrote (seeding.DeviceSeeds._next_step_seed: a
per-call copy).  All comparisons are bitwise under `deterministic_train` unless a test says otherwise; the Transformer
case is also anchored to the fp64 restatement (tests/transformer_helpers.py)."""
import importlib

import pytest
import torch

import transformer_helpers as TH
from test_gpu_graph import _build as _gate_model
from test_gpu_transformer import _model as _transformer_model, _rel
from test_gpu_window_size import _small as _pwin_model

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
ck = importlib.import_module("sl-hwgat_amd.checkpoint")
DEV = torch.device("cuda:0")
THR = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]       # HWGATE.py:96 draws these at random in train mode
C0 = 17
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["hwgate16", "hwgate8", "hgate", "wgate", "transformer"]
TR_CFG = dict(TH.CONFIGS["b"], B=32)                      # (deterministic weight gradients: B T a multiple of 32)
crit = train.SmoothedCrossEntropyLoss()


def _setup(kind, dtype):
    """a fresh model in train() with drop 0.1 and attention dropout 0.1 at every site, `deterministic_train`, and two
    different batches A and B on the device.  The builders are seeded: two calls give the same weights."""
    if kind == "transformer":
        m, _, _ = _transformer_model("b", dtype)
        batches = [TH.make_input(TR_CFG, seed=s) for s in (7, 8)]
        batches = [(x.to(DEV), y.to(DEV)) for x, y in batches]
    else:
        if kind == "hwgate8":
            m = _pwin_model(8, dtype)                     # K = 64, the part-window ('pwin') kernels
        else:
            m = _gate_model(dtype, "hwgate" if kind == "hwgate16" else kind)
            m.attn_drop_rate = 0.1
        g = torch.Generator(device=DEV).manual_seed(5)
        batches = [(torch.rand(8, m.temporal_dim, m.num_kps, m.kp_dim, device=DEV, generator=g),
                    torch.randint(0, 7, (8,), device=DEV, generator=g)) for _ in range(2)]
        if kind.startswith("hwgate"):
            m.threshold_override = THR
    assert m.drop_rate == 0.1 and (kind == "transformer" or m.attn_drop_rate == 0.1)
    m.train()
    m.deterministic_train = True
    return m, batches[0], batches[1]


def _grads(m):
    return [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]


def _same(ga, gb):
    return len(ga) == len(gb) and all((a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))
                                      for a, b in zip(ga, gb))


def _reference(m, A, B):
    """one forward + backward per call, nothing in between: call A at counter C0, call B at C0 + 1 -> [(logits, grads)]"""
    out = []
    for c, (x, y) in ((C0, A), (C0 + 1, B)):
        m.zero_grad(set_to_none=True)
        m._drop_calls = c
        logits = m(x)
        crit(logits, y).backward()
        out.append((logits.detach().clone(), _grads(m)))
    m.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_backward_after_a_later_train_forward_uses_its_own_masks(kind, dtype, order):
    """forward A, forward B, then the two backwards in either order: each gives the gradients of its call alone"""
    m, A, B = _setup(kind, dtype)
    ref = _reference(m, A, B)
    assert not torch.equal(ref[0][0], ref[1][0])
    m._drop_calls = C0
    outs = [m(A[0]), m(B[0])]
    assert m._drop_calls == C0 + 2
    for k in range(2):
        assert torch.equal(outs[k].detach(), ref[k][0]), k
    losses = [crit(outs[0], A[1]), crit(outs[1], B[1])]
    for k in ((0, 1) if order == "AB" else (1, 0)):
        losses[k].backward()
        assert _same(_grads(m), ref[k][1]), k
        m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_eval_forward_between_forward_and_backward(kind, dtype):
    m, A, B = _setup(kind, dtype)
    ref = _reference(m, A, B)
    m._drop_calls = C0
    loss = crit(m(A[0]), A[1])
    m.eval()
    with torch.no_grad():
        m(B[0])
    m.train()
    assert m._drop_calls == C0 + 1                        # an eval forward draws no masks
    loss.backward()
    assert _same(_grads(m), ref[0][1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_backward_of_two_summed_train_forwards(kind, dtype):
    """(ce(model(xA)) + ce(model(xB))).backward() == GA + GB up to the order of the two accumulations (1e-5 relative per
    parameter; a backward with the other call's masks is off by O(p))"""
    m, A, B = _setup(kind, dtype)
    (_, ga), (_, gb) = _reference(m, A, B)
    m._drop_calls = C0
    (crit(m(A[0]), A[1]) + crit(m(B[0]), B[1])).backward()
    names = [n for n, _ in m.named_parameters()]
    for n, g, a, b in zip(names, _grads(m), ga, gb):
        if a is None:
            assert g is None and b is None, n
            continue
        want = a.double() + b.double()
        err = float((g.double() - want).norm()) / max(float(want.norm()), 1e-30)
        assert err <= 1e-5, (n, err)


def test_interleaved_transformer_backward_against_fp64():
    """fp32: forward A, forward B, backward A against the fp64 restatement with call A's masks, rebuilt on the host side
    from `_seeds()` at A's counter (as test_gpu_transformer.test_train_dropout_sites_against_fp64 does)"""
    m, w, _ = _transformer_model("b", torch.float32)
    m.train()
    cfg = TR_CFG
    x, y = TH.make_input(cfg, seed=7)
    xb, _ = TH.make_input(cfg, seed=8)
    m._drop_calls = C0
    logits = m(x.to(DEV))
    m(xb.to(DEV))
    crit(logits, y.to(DEV)).backward()
    m._drop_calls = C0 + 1                                # the counter call A ran at
    B, T, d, nH, ff, p = cfg["B"], cfg["T"], cfg["d"], cfg["nhead"], cfg["ff"], m.drop_rate
    mask = lambda shape, seed: HF.dropout_mask(shape, seed, p, DEV).double().cpu()
    masks = {"embed": mask((B, T, d), m._seeds(63)[0])}
    for k in range(cfg["layers"]):
        s = m._seeds(k)
        masks[(k, "drop1")], masks[(k, "ff")] = mask((B, T, d), s[0]), mask((B, T, ff), s[1])
        masks[(k, "drop2")], masks[(k, "attn")] = mask((B, T, d), s[2]), mask((B, nH, T, T), s[3])
    ref_p = {k: v.double().requires_grad_(True) for k, v in w.items()}
    ref = TH.restate(ref_p, x, cfg, masks=masks)
    assert _rel(logits.detach(), ref.detach()) < 1e-4, _rel(logits.detach(), ref.detach())
    TH.smoothed_ce(ref, y).backward()
    for n, q in m.named_parameters():
        e = _rel(q.grad, ref_p[n].grad, 1e-3 * ref_p[n].grad.norm().item() + 1e-30)
        assert e < 1e-3, (n, e)


def _float_lr_chain(steps, lr=5e-4):
    """the lr of each step of a plain float-lr AdamW under checkpoint.get_scheduler (host arithmetic only)"""
    opt = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=lr)
    sch = ck.get_scheduler(opt)
    out = []
    for _ in range(steps):
        out.append(float(opt.param_groups[0]["lr"]))
        opt.step()                                        # (no gradients: no update; keeps the step order torch expects)
        sch.step()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["hwgate16", "hgate", "wgate", "transformer"])
def test_graphed_step_follows_the_lr_schedule(kind, dtype):
    """GraphedTrainStep given a float-lr AdamW(fused, capturable) with CosineAnnealingLR stepped between replays takes
    the steps an eager TrainStep takes with the same float-lr optimizer and schedule: losses and weights bit-equal, and
    the lr of each step is the float-lr chain's, exactly.

    Why the optimizer step runs after the replay and is not captured: a captured float lr is frozen into the graph,
    and a tensor lr does not match the float one.  Measured on the MI355X (torch 2.10 ROCm, 3 x 4099 fp32 parameters,
    4 fused AdamW steps): the fused kernel reads a tensor lr as a float32 word -- a float64 tensor lr is refused
    ("expected scalar type Float but found Double") -- and a float32 5e-4 changed 44 of the 12 297 entries against the
    float 5e-4 (the updates equal those of the Python float of the float32 value: only the rounding differs)."""
    steps = 6
    runs = []
    for graphed in (False, True):
        m, (x, y), _ = _setup(kind, dtype)
        opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
        sch = ck.get_scheduler(opt)
        m._drop_calls = C0
        step = train.GraphedTrainStep(m, opt, x, y) if graphed else train.TrainStep(m, opt, None)
        losses, lrs = [], []
        for _ in range(steps):
            lrs.append(opt.param_groups[0]["lr"])
            losses.append(step(x, y).clone())
            sch.step()
        runs.append((losses, lrs, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (le, lre, we), (lg, lrg, wg) = runs
    want = _float_lr_chain(steps)
    assert want[-1] < 0.9 * want[0]                       # the schedule moves the lr within these steps
    assert lre == lrg == want
    for k in range(steps):
        assert torch.equal(le[k], lg[k]), (k, float(le[k]), float(lg[k]))
    for n in we:
        assert torch.equal(we[n], wg[n]), n


def test_seed_mirror_after_graph_replays_then_an_eager_step():
    """two replays of a captured step, then one eager step on the same model: the host mirror `_seeds()` still names the
    masks the kernels draw, and the eager step's gradients are those of an eager-only model at the same counter.  A
    replay after that still trains; one after model.eval() is refused."""
    m, (x, y), _ = _setup("hwgate16", torch.float32)
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    m._drop_calls = C0
    graphed = train.GraphedTrainStep(m, opt, x, y)
    graphed(x, y)
    graphed(x, y)
    assert m._drop_calls == C0 + 2
    m.zero_grad(set_to_none=True)
    train.TrainStep(m, None, None)(x, y)                  # no optimizer: the gradients stay
    assert m._drop_calls == C0 + 3
    for k in (0, 5):
        for site, eff in zip(m._site_seeds(k), m._seeds(k)):
            a = HF.dropout_mask((4096,), eff, 0.3, DEV)
            b = HF.dropout_mask((4096,), site, 0.3, DEV, seed_base=m._seed_state[1:2])
            assert torch.equal(a, b), (k, site)
    got = _grads(m)
    ref, _, _ = _setup("hwgate16", torch.float32)
    ref.load_state_dict(m.state_dict())                   # the weights after the two replays
    ref._drop_calls = C0 + 2
    train.TrainStep(ref, None, None)(x, y)
    assert _same(got, _grads(ref))
    # the eager step's zero_grad detached nothing the replays need: a replay after it still updates the weights
    m.zero_grad(set_to_none=True)
    w = [p.detach().clone() for p in m.parameters()]
    graphed(x, y)
    assert sum(not torch.equal(a, p) for a, p in zip(w, m.parameters())) > len(w) // 2
    m.eval()
    with pytest.raises(ValueError, match="train"):
        graphed(x, y)
