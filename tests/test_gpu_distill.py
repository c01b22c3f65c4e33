"""GPU: knowledge distillation inside the train step (hwgat_kd_* of csrc/loss_eval.hip, train.Distiller,
train.DistilledCrossEntropyLoss, the `distiller=` of TrainStep / GraphedTrainStep / EpochLoop).

The kernels are held against tests/distill_helpers.py in fp64 with the bound of tests/test_gpu_mix.py for the same file's
kernels: max(FLOOR, 4 x the fp32 helper's own deviation from fp64).  Graph against eager is `torch.equal` throughout, under
`deterministic_train`: a replay issues the eager step's kernels on the eager step's inputs.

Worst deviations measured (WORST_kd lines, MI355X): see DESIGN.md section 6y."""
import importlib
import math

import pytest
import torch

import distill_helpers as DH
import stgcn_helpers as SH
import test_gpu_graph_micro as GM
from helpers import rel_err

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
optim = importlib.import_module("sl-hwgat_amd.optim")
DEV = torch.device("cuda:0")
EPS, G_UP, FLOOR = GM.EPS, GM.G_UP, GM.FLOOR
# (b, C, floats the logits sit past a 16-byte boundary); the row kernel stages rows of up to 4096 columns
KERNEL_CASES = GM.KERNEL_CASES + [(4, 5, 0), (3, 67, 1), (2, 4095, 1), (2, 4096, 0), (2, 4100, 0)]
HYPER = [(0.5, 0.25), (0.5, 1.0), (1.0, 4.0), (0.3, 32.0)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stable_rank(z, t):
    zt = z.gather(-1, t.unsqueeze(1))
    cols = torch.arange(z.shape[1]).unsqueeze(0)
    return ((z > zt) | ((z == zt) & (cols < t.unsqueeze(1)))).sum(-1)


def _lowest_argmax(u):
    cols = torch.arange(u.shape[1]).unsqueeze(0).expand_as(u)
    return torch.where(u == u.max(-1, keepdim=True).values, cols, u.shape[1]).min(-1).values


def _shifted(t, shift):
    b, C = t.shape
    flat = torch.zeros(b * C + 4, device=DEV)
    d = flat[shift:shift + b * C].view(b, C)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 * shift and d.is_contiguous()
    return d


def _inputs(b, C, shift, mixed):
    g = torch.Generator().manual_seed(1000 * b + C)
    z = torch.randn(b, C, generator=g)
    z[0, 1] = z[0, 0]                                         # a tie: the lower index ranks first
    u = 3 * torch.randn(b, C, generator=g)
    u[0, C - 1] = u[0, 2] = u[0].max()                        # and a tied teacher maximum
    y = torch.randint(0, C, (b,), generator=g)
    yb = torch.randint(0, C, (b,), generator=g)
    lam = torch.cat([torch.tensor([1.0, 0.0, 0.5]), torch.rand(b, generator=g)])[:b].contiguous()
    yb[1] = y[1]
    yb[b - 1] = y[b - 1]
    if not mixed:
        yb = lam = None
    dev = lambda t: None if t is None else t.to(DEV)
    return z, u, y, yb, lam, _shifted(z, shift), _shifted(u, shift), dev(y), dev(yb), dev(lam)


def _state(alpha, tau):
    st = HF.kd_state(DEV)
    HF.kd_set(st, alpha, tau)
    return st


# ------------------------------------------------------------------------------------------ 1. the kernels against fp64
@pytest.mark.parametrize("mixed", [True, False], ids=["pairs", "labels"])
@pytest.mark.parametrize("b,C,shift", KERNEL_CASES)
def test_kd_kernels_against_fp64(b, C, shift, mixed):
    z, u, y, yb, lam, zd, ud, yd, ybd, lamd = _inputs(b, C, shift, mixed)
    g_dev = torch.tensor([G_UP], device=DEV)
    dom = y if lam is None else torch.where(lam >= 0.5, y, yb)
    rank_ref, pred_ref, tpred_ref = _stable_rank(z, dom), z.argmax(-1), _lowest_argmax(u)
    assert int(tpred_ref[0]) <= 2
    worst = {"loss": 0.0, "kd": 0.0, "dz": 0.0}
    for alpha, tau in HYPER:
        st = _state(alpha, tau)
        for offset in (0, 3):
            for n_rows in range(0, offset + b + 3):
                v = min(max(n_rows - offset, 0), b)
                word = torch.tensor([n_rows], device=DEV, dtype=torch.int32)
                out = tuple(torch.full_like(t, 77) for t in HF.kd_forward(zd, ud, yd, ybd, lamd, st, EPS, word, offset))
                (loss, row_loss, lse, rank, pred, correct, live, row_loss_b, rank_b, lse_s, lse_t, row_kd, t_pred, kd, agree,
                 t_correct) = HF.kd_forward(zd, ud, yd, ybd, lamd, st, EPS, word, offset, out=out)
                dz = HF.kd_backward(zd, ud, yd, ybd, lamd, st, lse, lse_s, lse_t, g_dev, EPS, word, offset,
                                    out=torch.full((b, C), 7.5, device=DEV))
                where = (alpha, tau, offset, n_rows)
                assert int(live) == v, where
                assert bool((dz[v:] == 0).all()), where                               # dead rows: exactly zero
                dead_from = 0 if not mixed else v                                     # without a mixer: never written
                for t in (row_loss, lse, rank, pred, lse_s, lse_t, row_kd, t_pred):   # and untouched in the forward
                    assert bool((t[v:] == 77).all()), where
                for t in (row_loss_b, rank_b):
                    assert bool((t[dead_from:] == 77).all()), where
                assert torch.equal(rank[:v].cpu().long(), rank_ref[:v]), where
                assert torch.equal(pred[:v].cpu().long(), pred_ref[:v]), where
                assert torch.equal(t_pred[:v].cpu().long(), tpred_ref[:v]), where
                assert correct.dtype == agree.dtype == t_correct.dtype == torch.int64
                assert int(correct) == int((rank_ref[:v] == 0).sum()), where
                assert int(agree) == int((pred_ref[:v] == tpred_ref[:v]).sum()), where
                assert int(t_correct) == int((tpred_ref[:v] == dom[:v]).sum()), where
                if v == 0:
                    assert float(loss) == 0.0 and float(kd) == 0.0 and not bool(dz.any()), where
                    continue
                ref = DH.kd_ref(z.double(), u, y, yb, lam, alpha, tau, v, n_rows)
                r32 = DH.kd_ref(z, u, y, yb, lam, alpha, tau, v, n_rows)
                e = {"loss": GM._rel(loss[0], ref[0]), "kd": GM._rel(kd[0], ref[1]), "dz": GM._entry(dz, ref[2])}
                e32 = {"loss": GM._rel(r32[0], ref[0]), "kd": GM._rel(r32[1], ref[1]), "dz": GM._entry(r32[2], ref[2])}
                for k in worst:
                    worst[k] = max(worst[k], e[k])
                    assert e[k] <= max(FLOOR, 4 * e32[k]), (k, where, e[k], e32[k])
                # the rows: lse_s / lse_t and the blend
                assert GM._rel(lse_s[:v], torch.logsumexp(z.double()[:v] / tau, -1)) <= FLOOR, where
                assert GM._rel(lse_t[:v], torch.logsumexp(u.double()[:v] / tau, -1)) <= FLOOR, where
                assert GM._rel(row_kd[:v], DH.kd_rows(z.double()[:v], u.double()[:v], tau)) <= max(
                    FLOOR, 4 * GM._rel(DH.kd_rows(z[:v], u[:v], tau), DH.kd_rows(z.double()[:v], u.double()[:v], tau))), where
                # a repeat is bit-equal
                again = HF.kd_forward(zd, ud, yd, ybd, lamd, st, EPS, word, offset)
                assert torch.equal(again[0], loss) and torch.equal(again[13], kd) and torch.equal(again[5], correct)
                assert torch.equal(again[14], agree) and torch.equal(again[15], t_correct)
                assert torch.equal(_bits(again[1][:v]), _bits(row_loss[:v])) and torch.equal(_bits(again[11][:v]), _bits(row_kd[:v]))
                assert torch.equal(_bits(HF.kd_backward(zd, ud, yd, ybd, lamd, st, again[2], again[9], again[10], g_dev, EPS, word,
                                                        offset)), _bits(dz)), where
    print(f"WORST_kd b={b} C={C} shift={shift} {'pairs' if mixed else 'labels'}: loss {worst['loss']:.2e}, "
          f"kd {worst['kd']:.2e}, dz {worst['dz']:.2e}")


# ------------------------------------------------------------------------------------------ 2. bit properties
@pytest.mark.parametrize("mixed", [True, False], ids=["pairs", "labels"])
@pytest.mark.parametrize("b,C,shift", KERNEL_CASES)
def test_alpha_zero_and_teacher_equal_student_bit_properties(b, C, shift, mixed):
    z, u, y, yb, lam, zd, ud, yd, ybd, lamd = _inputs(b, C, shift, mixed)
    g_dev = torch.tensor([G_UP], device=DEV)
    nan_teacher = _shifted(torch.full((b, C), math.nan), shift)
    same = _shifted(z, shift)                                 # the student's bits at another address
    assert torch.equal(_bits(same), _bits(zd)) and same.data_ptr() != zd.data_ptr()
    for offset, n_rows in ((0, b), (3, b + 1), (0, b + 4)):
        v = min(max(n_rows - offset, 0), b)
        word = torch.tensor([n_rows], device=DEV, dtype=torch.int32)
        # alpha == 0: the undistilled criterion's bits, and the teacher is not read
        st = _state(0.0, 4.0)
        if mixed:
            plain = HF.mbsce_forward(zd, yd, ybd, lamd, EPS, word, offset)
            dz_plain = HF.mbsce_backward(zd, yd, ybd, lamd, plain[2], g_dev, EPS, word, offset)
        else:
            plain = HF.bsce_forward(zd, yd, EPS, word, offset)
            dz_plain = HF.bsce_backward(zd, yd, plain[2], g_dev, EPS, word, offset)
        got = HF.kd_forward(zd, nan_teacher, yd, ybd, lamd, st, EPS, word, offset)
        dz = HF.kd_backward(zd, nan_teacher, yd, ybd, lamd, st, got[2], got[9], got[10], g_dev, EPS, word, offset)
        assert torch.equal(_bits(got[0]), _bits(plain[0])) and torch.equal(_bits(got[1][:v]), _bits(plain[1][:v]))
        assert torch.equal(_bits(got[2][:v]), _bits(plain[2][:v])) and torch.equal(got[3][:v], plain[3][:v])
        assert torch.equal(got[5], plain[5]) and torch.equal(_bits(dz), _bits(dz_plain))
        assert float(got[13]) == 0.0 and not bool(got[11][:v].any()) and int(got[14]) == 0 and int(got[15]) == 0
        assert math.isfinite(float(got[0])) and bool(torch.isfinite(dz).all())
        # with any other alpha that teacher makes the loss NaN, as the header says
        bad = HF.kd_forward(zd, nan_teacher, yd, ybd, lamd, _state(0.5, 4.0), EPS, word, offset)
        if v > 0:
            assert math.isnan(float(bad[0])) and math.isnan(float(bad[13])) and bool(torch.isnan(bad[11][:v]).all())
        else:
            assert float(bad[0]) == 0.0 and float(bad[13]) == 0.0                     # an empty slice reads no row at all
        # teacher == student, bit for bit: no divergence, exactly
        for alpha, tau in HYPER + [(0.5, 3.0)]:
            st = _state(alpha, tau)
            got = HF.kd_forward(zd, same, yd, ybd, lamd, st, EPS, word, offset)
            assert bool((got[11][:v] == 0).all()) and float(got[13]) == 0.0, (alpha, tau, got[11][:v])
            assert torch.equal(_bits(got[9][:v]), _bits(got[10][:v]))
            assert int(got[14]) == v                          # and every row agrees with itself
            if alpha == 1.0:                                  # nothing but the soft term: an exactly zero gradient
                dz = HF.kd_backward(zd, same, yd, ybd, lamd, st, got[2], got[9], got[10], g_dev, EPS, word, offset)
                assert not bool(dz.any())


# ------------------------------------------------------------------------------------------ 3. the whole step
B, FEED = 6, [6, 5, 6]                                        # a short batch of 5 in the middle
MIXED = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.8, cutmix_share=0.5, seed=5)


def _tiny(kind, dtype, seed, drop=True):
    """tests/test_gpu_graph_micro.py's tiny models, built from another seed"""
    if kind == "stgcn":
        cfg = dict(SH.CONFIGS["a"], B=B, T=8)
        torch.manual_seed(seed)
        m = hw.STGCNModel(*SH.model_args(cfg, 0.05 if drop else 0.0)).to(DEV).train()
        m.deterministic_train = True
        return m
    m = GM._build(dtype, kind, drop)                          # seeds torch with 11
    if seed != 11:
        torch.manual_seed(seed)
        ds = {"src_len": 16, "num_class": 7}
        hp = {"hgate": lambda: hw.HGATEParams(ds, 2, DEV), "wgate": lambda: hw.WGATEParams(ds, 2, DEV, num_kps=32),
              "hwgate": lambda: hw.HWGATEParams(ds, 2, DEV, num_kps=32)}[kind]()
        if not drop:
            hp.drop_rate = 0.0
        other = type(m)(*hp.get_model_params()).to(DEV)
        m.load_state_dict(other.state_dict())
    return m


def _batch(kind, student):
    if kind == "stgcn":
        return tuple(t.to(DEV) for t in SH.make_input(dict(SH.CONFIGS["a"], B=B, T=8)))
    return GM._batch(student, B)


def _run(kind, t_kind, dtype, graphed, feed, t_seed=23, mixer_kw=None, alpha=0.5, tau=4.0, after_capture=None, lr=5e-4,
         drop=True, distill=True, **step_kw):
    m = _tiny(kind, dtype, 11 if kind != "stgcn" else 21, drop)
    x, y = _batch(kind, m)
    o = optim.DeviceAdamW(list(m.parameters()), lr=lr)
    kw = dict(step_kw)
    d = teacher = None
    if distill:
        teacher = _tiny(t_kind, dtype, t_seed, drop)
        teacher._drop_calls = 5
        d = train.Distiller(teacher, alpha=alpha, temperature=tau)
        kw["distiller"] = d
    if mixer_kw is not None:
        kw["mixer"] = train.BatchMixer(**mixer_kw)
    torch.manual_seed(11)                                     # the dropout base seeds hash torch.initial_seed(): one for every run
    before = None if teacher is None else {k: v.clone() for k, v in teacher.state_dict().items()}
    if graphed:
        s = train.GraphedTrainStep(m, o, x, y, **kw)
    else:
        if kw.pop("ragged", False):
            kw["pad_to"] = B
        s = train.TrainStep(m, o, **kw)
    if after_capture is not None:
        after_capture(d)
    graph = s.graph if graphed else None
    x_before = x.clone()
    trace = []
    for n in feed:
        loss = s(x[:n], y[:n]).clone()
        rec = [loss, s.correct.clone()]
        if d is not None:
            rec += [s.kd.clone(), s.agree.clone(), s.teacher_correct.clone()]
        trace.append(rec)
    assert graph is (s.graph if graphed else None) and torch.equal(x, x_before)      # one capture; the caller's batch is its own
    if teacher is not None:                                   # the teacher is where it was
        after = teacher.state_dict()
        assert set(after) == set(before) and all(torch.equal(_raw(after[k]), _raw(before[k])) for k in before)
        assert not teacher.training and teacher._drop_calls == 5
        assert all(p.grad is None and not p.requires_grad for p in teacher.parameters())
    return dict(trace=trace, weights=[p.detach().clone() for p in m.parameters()], step=s, distiller=d, model=m, feed=feed)


def _raw(t):
    return t.view(torch.uint8) if t.is_floating_point() else t


def _same(a, b, upto=None):
    assert len(a["trace"]) == len(b["trace"])
    for k, (ra, rb) in enumerate(zip(a["trace"], b["trace"])):
        for i, (ta, tb) in enumerate(zip(ra[:upto], rb[:upto])):
            assert torch.equal(ta, tb), (k, ("loss", "correct", "kd", "agree", "teacher_correct")[i], ta, tb)
    assert len(a["weights"]) == len(b["weights"]) and all(torch.equal(p, q) for p, q in zip(a["weights"], b["weights"]))
    assert a["model"]._drop_calls == b["model"]._drop_calls


@pytest.mark.parametrize("kind,t_kind,dtype,mixer_kw,step_kw", [
    ("hwgate", "wgate", torch.float32, None, dict(micro_batch=4, ragged=True)),
    ("hwgate", "wgate", torch.bfloat16, None, dict(micro_batch=4, ragged=True)),
    ("hgate", "hgate", torch.float32, MIXED, dict(micro_batch=4, ragged=True)),
    ("hwgate", "wgate", torch.float32, None, dict()),
    ("stgcn", "stgcn", torch.float32, None, dict(micro_batch=4))],
    ids=["hwgate-fp32", "hwgate-bf16", "hgate-mixed", "hwgate-unsliced", "stgcn"])
def test_distilled_graph_equals_the_distilled_eager_step(kind, t_kind, dtype, mixer_kw, step_kw):
    feed = FEED if step_kw.get("ragged") else [B] * 3
    eager, graph = (_run(kind, t_kind, dtype, g, feed, mixer_kw=mixer_kw, **step_kw) for g in (False, True))
    s = graph["step"]
    assert type(s.criterion) is train.DistilledCrossEntropyLoss and s.criterion.distiller is graph["distiller"]
    assert (s.criterion.mixer is None) == (mixer_kw is None)
    _same(eager, graph)
    for n, (loss, correct, kd, agree, t_correct) in zip(feed, graph["trace"]):
        assert math.isfinite(float(loss)) and float(kd) > 0.0 and float(loss) > 0.0 and not kd.requires_grad
        assert 0 <= int(correct) <= n and 0 <= int(agree) <= n and 0 <= int(t_correct) <= n
        assert kd.dtype == torch.float32 and agree.dtype == t_correct.dtype == torch.int64
    assert graph["model"]._drop_calls == eager["model"]._drop_calls


# ------------------------------------------------------------------------------------------ 4. the composition by hand
def test_eager_distilled_step_is_the_composition_by_hand():
    """the distilled step in slices of 4 against one forward of the batch with the teacher's logits from a plain eval forward
    and the loss in torch ops, no dropout: the same sums in another order, so the bounds are those of
    tests/test_gpu_mix.py::test_eager_mixed_step_is_the_composition_by_hand"""
    alpha, tau = 0.6, 3.0
    m = _tiny("hwgate", torch.float32, 11, drop=False)
    x, y = GM._batch(m, B)
    teacher = _tiny("wgate", torch.float32, 23, drop=False)
    s = train.TrainStep(m, None, None, micro_batch=4, distiller=train.Distiller(teacher, alpha=alpha, temperature=tau))
    s(x, y)
    l0, g0 = float(s.loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m2 = _tiny("hwgate", torch.float32, 11, drop=False)
    with torch.no_grad():
        u = teacher(x).float()
    out = m2(x).float()
    rk = DH.kd_rows(out, u, tau)
    loss = ((1.0 - alpha) * GM._rows(out, y) + alpha * rk).mean()
    loss.backward()
    l1, g1 = float(loss.detach()), {k: p.grad.clone() for k, p in m2.named_parameters() if p.grad is not None}
    kd1 = float(rk.detach().mean())
    print(f"step {l0:.7f} by hand {l1:.7f}; kd {float(s.kd):.7f} by hand {kd1:.7f}")
    assert abs(l1 - l0) < 1e-4 and abs(float(s.kd) - kd1) < 1e-4 and kd1 > 1e-3
    assert int(s.correct) == int((out.argmax(-1) == y).sum()) and int(s.agree) == int((out.argmax(-1) == u.argmax(-1)).sum())
    assert int(s.teacher_correct) == int((u.argmax(-1) == y).sum())
    assert set(g0) == set(g1) and len(g0) > 10
    for k in g0:
        if k.endswith("attn.qkv.bias"):
            continue                                         # the key third has an exactly-zero true gradient: pure rounding noise
        assert rel_err(g1[k].cpu(), g0[k].cpu()) < 1e-4, (k, rel_err(g1[k].cpu(), g0[k].cpu()))


# ------------------------------------------------------------------------------------------ 5. hyper-parameters after capture
def test_alpha_zero_after_capture_leaves_the_plain_ragged_step():
    kw = dict(micro_batch=4, ragged=True)
    plain = _run("hwgate", None, torch.float32, True, FEED, distill=False, **kw)
    assert type(plain["step"].criterion) is train.BatchSlicedCrossEntropyLoss

    def off(d):
        d.alpha = 0.0

    zero = _run("hwgate", "wgate", torch.float32, True, FEED, after_capture=off, **kw)
    _same(plain, zero, upto=2)                                # loss, correct and every weight, bit for bit; no new capture
    assert all(float(rec[2]) == 0.0 for rec in zero["trace"])
    on = _run("hwgate", "wgate", torch.float32, True, FEED, **kw)
    assert not torch.equal(on["trace"][0][0], plain["trace"][0][0]) and float(on["trace"][0][2]) > 0.0


def test_a_new_temperature_reaches_the_next_replay():
    def cool(d):
        d.temperature = 1.0

    base = _run("hgate", "hgate", torch.float32, True, [B], **dict(micro_batch=4, ragged=True))
    cooled = _run("hgate", "hgate", torch.float32, True, [B], after_capture=cool, **dict(micro_batch=4, ragged=True))
    assert float(base["trace"][0][2]) > 0.0 and float(cooled["trace"][0][2]) > 0.0
    assert not torch.equal(base["trace"][0][2], cooled["trace"][0][2])
    assert torch.equal(base["trace"][0][1], cooled["trace"][0][1]) and torch.equal(base["trace"][0][3], cooled["trace"][0][3])
    # and it is the value an eager step with that temperature gives
    eager = _run("hgate", "hgate", torch.float32, False, [B], tau=1.0, **dict(micro_batch=4, ragged=True))
    _same(eager, cooled)


# ------------------------------------------------------------------------------------------ 6. bystanders
def test_student_counter_advances_as_without_a_distiller():
    kw = dict(micro_batch=4, ragged=True)
    plain = _run("hwgate", None, torch.float32, True, FEED, distill=False, **kw)
    kd = _run("hwgate", "wgate", torch.float32, True, FEED, **kw)      # _run checks the teacher and the caller's x
    assert plain["model"]._drop_calls == kd["model"]._drop_calls == GM.C0 + 2 * len(FEED)
    assert torch.equal(GM._probe(plain["model"]), GM._probe(kd["model"]))


def test_distiller_none_is_the_step_without_the_keyword():
    for kw in (dict(), dict(micro_batch=3, ragged=True)):
        base = GM._run("hwgate", torch.float32, "adamw", True, [8, 8, 8], **kw)
        none = GM._run("hwgate", torch.float32, "adamw", True, [8, 8, 8], distiller=None, **kw)
        GM._same(base, none)
        assert type(none["step"].criterion) is type(base["step"].criterion)
        assert none["step"].kd is None and none["step"].agree is None and none["step"].teacher_correct is None


def test_a_teacher_of_another_width_is_refused_at_the_first_forward():
    m = _tiny("hgate", torch.float32, 11)
    x, y = GM._batch(m, B)
    torch.manual_seed(2)
    hp = hw.HGATEParams({"src_len": 16, "num_class": 9}, 2, DEV)
    wide = hw.HGATEModel(*hp.get_model_params()).to(DEV)
    s = train.TrainStep(m, None, None, distiller=train.Distiller(wide))
    with pytest.raises(ValueError, match="same classes"):
        s(x, y)


# ------------------------------------------------------------------------------------------ 7. it teaches
def test_the_student_moves_towards_the_teacher():
    r = _run("hgate", "hgate", torch.float32, True, [B] * 40, alpha=1.0, tau=2.0, lr=1e-3, drop=False)
    kd = [float(rec[2]) for rec in r["trace"]]
    agree = [int(rec[3]) for rec in r["trace"]]
    print(f"kd first five {kd[:5]} last five {kd[-5:]}; agree {agree[0]} -> {agree[-1]}")
    assert all(math.isfinite(v) and v >= 0.0 for v in kd)
    assert sum(kd[-5:]) / 5 < sum(kd[:5]) / 5 and agree[-1] >= agree[0]
    assert all(torch.equal(rec[0], rec[2]) for rec in r["trace"])     # alpha = 1: the loss is the KD term


# ------------------------------------------------------------------------------------------ 8. the epoch loop
def test_epoch_loop_carries_alpha_and_temperature(tmp_path):
    cfg = SH.CONFIGS["a"]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(8, cfg["T"], cfg["V"], cfg["C"], generator=g).to(DEV)
    y = torch.randint(0, cfg["nclass"], (8,), generator=g).to(DEV)
    tr = [(x[:4], y[:4]), (x[4:], y[4:])]
    kw = dict(batch_size=4, example=(x[:4], y[:4]), num_classes=cfg["nclass"], save_interval=1)

    def build(seed):
        torch.manual_seed(seed)
        model = hw.STGCNModel(*SH.model_args(cfg, 0.0)).to(DEV)
        model.deterministic_train = True
        return model, optim.DeviceAdamW(list(model.parameters()), lr=1e-3)

    teacher, _ = build(9)
    model, opt = build(3)
    d = train.Distiller(teacher, alpha=0.7, temperature=3.0)
    first = train.EpochLoop(model, opt, None, distiller=d, out_prefix=str(tmp_path / "kd"), **kw)
    first.run(tr, tr, epochs=0)
    assert type(first.step.criterion) is train.DistilledCrossEntropyLoss and float(first.step.kd) > 0.0
    path = str(tmp_path / "kd_best_loss.pt")
    assert path in first.written
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert raw["extra"]["distiller"] == dict(alpha=0.7, temperature=3.0)
    assert not any(k.startswith("teacher") for k in raw["extra"])

    model, opt = build(4)
    d2 = train.Distiller(teacher)
    second = train.EpochLoop(model, opt, None, distiller=d2, **kw)
    assert second.resume(path) == 1 and (d2.alpha, d2.temperature) == (0.7, 3.0)
    second.train_epoch(tr[:1])
    assert float(second.step.kd) > 0.0

    model, opt = build(3)
    plain = train.EpochLoop(model, opt, None, out_prefix=str(tmp_path / "plain"), **kw)
    plain.run(tr, tr, epochs=0)
    raw = torch.load(str(tmp_path / "plain_best_loss.pt"), map_location="cpu", weights_only=True)
    assert "distiller" not in raw["extra"]
    third = train.EpochLoop(model, opt, None, distiller=train.Distiller(teacher, alpha=0.2), **kw)
    assert third.resume(str(tmp_path / "plain_best_loss.pt")) == 1 and third.distiller.alpha == 0.2
