"""CPU: the host side of knowledge distillation inside the train step (hwgat_kd_* of csrc/loss_eval.hip, train.Distiller /
train.DistilledCrossEntropyLoss) -- the entry points in the header, the binding and the library, their argument checks
before any HIP call, what Distiller, the two steps and the epoch loop refuse before they look at a device, and the torch
restatement of the criterion (tests/distill_helpers.py): its closed-form gradient is autograd's in fp64, and the soft part
of it vanishes where the teacher's logits are the student's."""
import ctypes
import importlib
import math
import re

import pytest
import torch

import distill_helpers as DH

hw = importlib.import_module("sl-hwgat_amd")
train = importlib.import_module("sl-hwgat_amd.train")
HF = hw.functional
KD_SYMBOLS = {"hwgat_kd_state_bytes", "hwgat_kd_set", "hwgat_kd_fwd", "hwgat_kd_bwd"}
EINVAL, ESHAPE = -1, -2


def _buf():
    """aligned host memory standing in for a device pointer: never dereferenced, every call below is refused first"""
    keep = (ctypes.c_double * 64)()
    return keep, ctypes.cast(keep, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ header, binding, library
def test_symbols_abi_and_constants_follow_the_header():
    assert KD_SYMBOLS <= set(hw._lib.declared_symbols())
    assert KD_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_kd_")}
    assert KD_SYMBOLS == {n for n in hw._lib.declared_symbols() if n.startswith("hwgat_kd_")}
    assert set(hw._lib.declared_symbols()) == set(hw._lib._SIGS)
    L = hw._lib.lib()
    for name in KD_SYMBOLS:
        assert getattr(L, name) is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007     # additions only
    assert L.hwgat_kd_state_bytes() == 8 == 4 * HF.KD_STATE_WORDS
    with open(hw._lib.HEADER) as fh:
        src = fh.read()
    for name, want in (("MIN", HF.KD_TAU_MIN), ("MAX", HF.KD_TAU_MAX)):
        assert float(re.search(r"#define\s+HWGAT_KD_TAU_" + name + r"\s+(\S+)", src).group(1)) == want, name
    assert (HF.KD_TAU_MIN, HF.KD_TAU_MAX) == (0.25, 32.0)


def test_entry_points_check_their_arguments_without_launching():
    L = hw._lib.lib()
    keep, buf = _buf()
    odd = ctypes.c_void_p(buf.value + 4)
    # (state, alpha, tau, stream)
    assert L.hwgat_kd_set(None, 0.5, 4.0, None) == EINVAL and L.hwgat_kd_set(odd, 0.5, 4.0, None) == EINVAL
    for alpha, tau in ((-0.01, 4.0), (1.01, 4.0), (math.nan, 4.0), (0.5, 0.24), (0.5, 32.5), (0.5, math.nan), (0.5, math.inf),
                       (0.5, 0.0), (0.5, -1.0), (math.inf, 1.0)):
        assert L.hwgat_kd_set(buf, alpha, tau, None) == ESHAPE, (alpha, tau)
    # (logits, teacher, target, target_b, lam, n_rows, offset, state, lse, row_loss, rank, pred, loss, correct, live,
    #  row_loss_b, rank_b, lse_s, lse_t, row_kd, t_pred, kd, agree, t_correct, B, C, eps, stream)
    good = [buf] * 6 + [0] + [buf] * 17 + [4, 7, 0.01, None]
    for i in [0, 1, 2, 5] + list(range(7, 24)):
        assert L.hwgat_kd_fwd(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i in (3, 4):                                          # exactly one of target_b / lam NULL
        assert L.hwgat_kd_fwd(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    assert L.hwgat_kd_fwd(*(good[:7] + [odd] + good[8:])) == EINVAL             # the state: 8-byte aligned
    for i, bad, rc in ((6, -1, EINVAL), (6, 1 << 31, EINVAL), (24, 0, ESHAPE), (24, 1 << 31, ESHAPE), (25, 0, ESHAPE),
                       (25, 65537, ESHAPE)):
        assert L.hwgat_kd_fwd(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    none = good[:3] + [None, None] + good[5:]                 # no mixer: both NULL, and then no row_loss_b / rank_b either
    none[15] = none[16] = None
    for i, bad, rc in ((0, None, EINVAL), (7, None, EINVAL), (6, -1, EINVAL), (24, 0, ESHAPE), (25, 65537, ESHAPE)):
        assert L.hwgat_kd_fwd(*(none[:i] + [bad] + none[i + 1:])) == rc, (i, bad)
    # (logits, teacher, target, target_b, lam, n_rows, offset, state, lse, lse_s, lse_t, g, dlogits, B, C, eps, stream)
    good = [buf] * 6 + [0] + [buf] * 6 + [4, 7, 0.01, None]
    for i in [0, 1, 2, 5] + list(range(7, 13)):
        assert L.hwgat_kd_bwd(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i in (3, 4):
        assert L.hwgat_kd_bwd(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    assert L.hwgat_kd_bwd(*(good[:7] + [odd] + good[8:])) == EINVAL
    for i, bad, rc in ((6, -1, EINVAL), (6, 1 << 31, EINVAL), (13, 0, ESHAPE), (14, 0, ESHAPE), (14, 65537, ESHAPE)):
        assert L.hwgat_kd_bwd(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    none = good[:3] + [None, None] + good[5:]
    for i, bad, rc in ((1, None, EINVAL), (12, None, EINVAL), (13, 0, ESHAPE)):
        assert L.hwgat_kd_bwd(*(none[:i] + [bad] + none[i + 1:])) == rc, (i, bad)
    del keep


# ------------------------------------------------------------------------------------------ what the classes refuse
def test_distiller_refuses_values_outside_its_ranges():
    teacher = torch.nn.Linear(4, 3)
    teacher.train()
    d = train.Distiller(teacher)
    assert (d.alpha, d.temperature) == (0.5, 4.0)
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    for kw in (dict(alpha=-0.1), dict(alpha=1.1), dict(alpha=math.nan), dict(alpha="0.5"), dict(alpha=True),
               dict(temperature=0.2), dict(temperature=33), dict(temperature=math.nan), dict(temperature=math.inf),
               dict(temperature="4"), dict(temperature=True), dict(temperature=0)):
        with pytest.raises(ValueError, match="Distiller"):
            train.Distiller(torch.nn.Linear(4, 3), **kw)
    with pytest.raises(ValueError, match="Distiller"):
        train.Distiller(object())
    train.Distiller(torch.nn.Linear(4, 3), alpha=0, temperature=0.25)
    train.Distiller(torch.nn.Linear(4, 3), alpha=1, temperature=32)
    for bad in (-0.1, 2.0, math.nan, "1", False):
        with pytest.raises(ValueError, match="alpha"):
            d.alpha = bad
    for bad in (0.1, 64, math.nan, None):
        with pytest.raises(ValueError, match="temperature"):
            d.temperature = bad
    assert (d.alpha, d.temperature) == (0.5, 4.0)
    d.alpha, d.temperature = 0.25, 2
    d.push_hyper()                                            # unbound: nothing to launch
    # a value that got past the properties is refused when it is about to be pushed, before any launch
    d._alpha = 2.0
    with pytest.raises(ValueError, match="alpha"):
        d.push_hyper()
    d._alpha, d._tau = 0.25, 100.0
    with pytest.raises(ValueError, match="temperature"):
        d.push_hyper()
    d._tau = 2
    sd = d.state_dict()
    assert sd == dict(alpha=0.25, temperature=2.0) and all(type(v) is float for v in sd.values())
    d2 = train.Distiller(torch.nn.Linear(4, 3))
    d2.load_state_dict(sd)
    assert d2.state_dict() == sd and (d2.alpha, d2.temperature) == (0.25, 2.0)
    for bad in (dict(sd, alpha=3.0), dict(sd, temperature=0.0)):
        with pytest.raises(ValueError, match="Distiller"):
            d2.load_state_dict(bad)
    assert d2.state_dict() == sd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.bind("cpu")
    teacher.train()
    with pytest.raises(RuntimeError, match="eval"):
        d.observe(torch.zeros(2, 4))
    teacher.eval()
    assert d.observe(torch.zeros(2, 4)).shape == (2, 3) and not d.logits.requires_grad


def test_steps_and_the_loop_refuse_before_touching_a_device():
    model, teacher = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)
    x, y = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64)
    loop_kw = dict(batch_size=2, example=(x, y), num_classes=3)
    for crit in (train.SmoothedCrossEntropyLoss(), train.FusedSmoothedCrossEntropyLoss(), train.BatchSlicedCrossEntropyLoss(),
                 train.MixedCrossEntropyLoss(), torch.nn.CrossEntropyLoss()):
        with pytest.raises(ValueError, match="teacher's logits beside its labels"):
            train.TrainStep(model, None, criterion=crit, distiller=train.Distiller(teacher))
        with pytest.raises(ValueError, match="teacher's logits beside its labels"):
            train.GraphedTrainStep(model, None, x, y, criterion=crit, distiller=train.Distiller(teacher))
    for make in (lambda **kw: train.TrainStep(model, None, **kw), lambda **kw: train.GraphedTrainStep(model, None, x, y, **kw),
                 lambda **kw: train.EpochLoop(model, None, None, **loop_kw, **kw)):
        with pytest.raises(ValueError, match="must be a train.Distiller"):
            make(distiller=object())
        with pytest.raises(ValueError, match="the teacher is the student"):
            make(distiller=train.Distiller(model))
        model.train().requires_grad_(True)                    # the refused Distiller froze it
    for make in (lambda **kw: train.TrainStep(model, None, **kw), lambda **kw: train.GraphedTrainStep(model, None, x, y, **kw)):
        with pytest.raises(NotImplementedError, match="reducer"):
            make(distiller=train.Distiller(teacher), reducer=object())
    d = train.Distiller(teacher)
    s = train.TrainStep(model, None, distiller=d)
    assert type(s.criterion) is train.DistilledCrossEntropyLoss and s.criterion.distiller is d and s.criterion.mixer is None
    assert isinstance(s.criterion, train.MixedCrossEntropyLoss)                  # what a mixer asks for
    with pytest.raises(ValueError, match="another Distiller"):
        train.TrainStep(model, None, criterion=s.criterion, distiller=train.Distiller(teacher))
    mixer = train.BatchMixer()
    s2 = train.TrainStep(model, None, distiller=train.Distiller(teacher), mixer=mixer)
    assert type(s2.criterion) is train.DistilledCrossEntropyLoss and s2.criterion.mixer is mixer
    with pytest.raises(RuntimeError, match="bind_distiller"):
        train.DistilledCrossEntropyLoss()(torch.zeros(2, 3), y)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loop = train.EpochLoop(model, opt, None, distiller=d, **loop_kw)
    assert loop.distiller is d and loop._extra()["distiller"] == dict(alpha=0.5, temperature=4.0)
    assert "distiller" not in train.EpochLoop(model, opt, None, **loop_kw)._extra()
    # without a distiller the criteria are what they were
    assert type(train.TrainStep(model, None).criterion) is train.SmoothedCrossEntropyLoss
    assert type(train.TrainStep(model, None, distiller=None).criterion) is train.SmoothedCrossEntropyLoss
    assert type(train.TrainStep(model, None, mixer=train.BatchMixer()).criterion) is train.MixedCrossEntropyLoss


# ------------------------------------------------------------------------------------------ the torch restatement
CASES = [(0.5, 0.25), (0.5, 1.0), (1.0, 4.0), (0.3, 32.0), (0.0, 2.0)]


@pytest.mark.parametrize("mixed", [False, True], ids=["labels", "pairs"])
@pytest.mark.parametrize("alpha,tau", CASES)
def test_helper_gradient_is_autograd_in_fp64(alpha, tau, mixed):
    g = torch.Generator().manual_seed(5)
    b, C = 5, 37
    z = torch.randn(b, C, generator=g, dtype=torch.float64)
    u = 3 * torch.randn(b, C, generator=g, dtype=torch.float64)
    u[1, 4] = -math.inf                                       # a column the teacher rules out: p = 0, no term
    y, yb = torch.randint(0, C, (b,), generator=g), torch.randint(0, C, (b,), generator=g)
    lam = torch.cat([torch.tensor([1.0, 0.0, 0.5]), torch.rand(b, generator=g)])[:b] if mixed else None
    yb = yb if mixed else None
    for v, n_rows in ((5, 5), (3, 3), (2, 7), (0, 4)):
        zz = z.clone().requires_grad_(True)
        loss, kd = DH.kd_loss(zz, u, y, yb, lam, alpha, tau, v, n_rows)
        (loss * DH.G_UP).backward()
        ref_loss, ref_kd, dz = DH.kd_ref(z, u, y, yb, lam, alpha, tau, v, n_rows)
        loss, kd = loss.detach(), kd.detach()
        assert float(ref_loss) == float(loss) and float(ref_kd) == float(kd) and math.isfinite(float(loss))
        assert float(kd) >= 0.0 and (v == 0) == (float(kd) == 0.0)
        assert bool((dz[v:] == 0).all()) and bool((zz.grad[v:] == 0).all())
        assert float((dz - zz.grad).abs().max()) <= 1e-13 * max(1.0, float(zz.grad.abs().max())), (v, n_rows)


def test_soft_gradient_vanishes_where_the_teacher_is_the_student():
    g = torch.Generator().manual_seed(6)
    z = torch.randn(4, 19, generator=g, dtype=torch.float64)
    y = torch.randint(0, 19, (4,), generator=g)
    for tau in (0.25, 1.0, 4.0, 32.0):
        soft = DH.kd_grad(z, z.clone(), y, None, None, 0.7, tau, 4, 4, soft_only=True)
        assert not bool(soft.any()), tau
        assert float(DH.kd_rows(z, z.clone(), tau).abs().max()) == 0.0
        other = DH.kd_grad(z, z + 0.1 * torch.randn(4, 19, generator=g, dtype=torch.float64), y, None, None, 0.7, tau, 4, 4,
                           soft_only=True)
        assert bool(other.any())
