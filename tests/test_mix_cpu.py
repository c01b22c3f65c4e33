"""CPU: the host side of Mixup / temporal CutMix inside the train step (csrc/mix.hip, hwgat_mbsce_* of csrc/loss_eval.hip,
train.BatchMixer / train.MixedCrossEntropyLoss) -- the entry points in the header, the binding and the library, their
argument checks before any HIP call, what BatchMixer and the two steps refuse before they look at a device, and the numpy
restatement of the draw (tests/mix_helpers.py): the seeds of the GPU tests trip none of its margin assertions, its Joehnk
sampler has Beta(alpha, alpha)'s moments, and its matching is a fixed-point-free involution of the live rows."""
import ctypes
import importlib
import math
import re

import numpy as np
import pytest
import torch

import mix_helpers as MH

hw = importlib.import_module("sl-hwgat_amd")
train = importlib.import_module("sl-hwgat_amd.train")
HF = hw.functional
MIX_SYMBOLS = {"hwgat_mix_state_bytes", "hwgat_mix_set", "hwgat_mix_draw", "hwgat_mix_apply"}
MBSCE_SYMBOLS = {"hwgat_mbsce_fwd", "hwgat_mbsce_bwd"}
EINVAL, ESHAPE = -1, -2


def _buf():
    """aligned host memory standing in for a device pointer: never dereferenced, every call below is refused first"""
    keep = (ctypes.c_double * 64)()
    return keep, ctypes.cast(keep, ctypes.c_void_p)


# ------------------------------------------------------------------------------------------ header, binding, library
def test_symbols_abi_and_constants_follow_the_header():
    assert MIX_SYMBOLS | MBSCE_SYMBOLS <= set(hw._lib.declared_symbols())
    assert MIX_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_mix_")}
    assert MBSCE_SYMBOLS == {n for n in hw._lib._SIGS if n.startswith("hwgat_mbsce_")}
    assert set(hw._lib.declared_symbols()) == set(hw._lib._SIGS)
    L = hw._lib.lib()
    for name in MIX_SYMBOLS | MBSCE_SYMBOLS:
        assert getattr(L, name) is not None
    assert hw._lib.header_abi_version() == 4007 and L.hwgat_abi_version() == 4007     # additions only
    assert L.hwgat_mix_state_bytes() == 40 == 8 * HF.MIX_STATE_WORDS
    with open(hw._lib.HEADER) as fh:
        src = fh.read()

    def define(name):
        return re.search(r"#define\s+HWGAT_MIX_" + name + r"\s+(\S+)", src).group(1)

    assert int(define("MAX_BATCH")) == HF.MIX_MAX_BATCH and float(define("ALPHA_MIN")) == HF.MIX_ALPHA_MIN == MH.ALPHA_MIN
    assert int(define("TAG")) == MH.MIX_TAG
    for name in ("APPLY", "MODE", "BETA", "START"):
        assert int(define("TAG_" + name), 16) == getattr(MH, "TAG_" + name), name
    for name, want in (("NONE", (HF.MIX_NONE, MH.NONE)), ("MIXUP", (HF.MIX_MIXUP, MH.MIXUP)),
                       ("CUTMIX", (HF.MIX_CUTMIX, MH.CUTMIX))):
        assert (int(define(name)),) * 2 == want, name


def test_entry_points_check_their_arguments_without_launching():
    L = hw._lib.lib()
    keep, buf = _buf()
    odd = ctypes.c_void_p(buf.value + 4)
    # (state, prob, cutmix_share, mixup_alpha, cutmix_alpha, set_counter, seed, step, stream)
    good = [buf, 1.0, 0.5, 0.4, 1.0, 1, 0, 0, None]
    assert L.hwgat_mix_set(*([None] + good[1:])) == EINVAL and L.hwgat_mix_set(*([odd] + good[1:])) == EINVAL
    for i, bad in ((1, -0.1), (1, 1.5), (1, math.nan), (2, -1e-9), (2, 2.0), (2, math.nan), (3, 0.049), (3, 1.01),
                   (3, math.nan), (4, 0.0), (4, 2.0), (4, math.inf)):
        assert L.hwgat_mix_set(*(good[:i] + [bad] + good[i + 1:])) == ESHAPE, (i, bad)
    # (state, y, n_rows, pairs, partner, lam, seg, mode, y_b, B, T, stream)
    good = [buf] * 9 + [8, 16, None]
    for i in (0, 1, 3, 4, 5, 6, 7, 8):                        # n_rows (2) may be NULL: all rows are live
        assert L.hwgat_mix_draw(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i in (0, 1, 8):                                       # 8-byte words
        assert L.hwgat_mix_draw(*(good[:i] + [odd] + good[i + 1:])) == EINVAL, i
    for i, bad, rc in ((9, 0, EINVAL), (9, -2, EINVAL), (9, 65537, ESHAPE), (10, 0, EINVAL), (10, (1 << 20) + 1, ESHAPE)):
        assert L.hwgat_mix_draw(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    # (x, pairs, lam, seg, mode, n_rows, B, T, R, stream)
    good = [buf] * 6 + [8, 16, 58, None]
    for i in range(5):
        assert L.hwgat_mix_apply(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    assert L.hwgat_mix_apply(*([ctypes.c_void_p(buf.value + 2)] + good[1:])) == EINVAL
    for i, bad, rc in ((6, 0, EINVAL), (6, 65537, ESHAPE), (7, 0, EINVAL), (7, (1 << 20) + 1, ESHAPE), (8, 0, EINVAL),
                       (8, 1 << 31, ESHAPE), (8, 1 << 27, ESHAPE)):            # T * R at or beyond 2^31
        assert L.hwgat_mix_apply(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    # (logits, target, target_b, lam, n_rows, offset, lse, row_loss, rank, pred, loss, correct, live, row_loss_b, rank_b, B, C,
    #  eps, stream)
    good = [buf] * 5 + [0] + [buf] * 9 + [4, 7, 0.01, None]
    for i in [0, 1, 2, 3, 4] + list(range(6, 15)):
        assert L.hwgat_mbsce_fwd(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i, bad, rc in ((5, -1, EINVAL), (5, 1 << 31, EINVAL), (15, 0, ESHAPE), (16, 0, ESHAPE), (16, 65537, ESHAPE)):
        assert L.hwgat_mbsce_fwd(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    # (logits, target, target_b, lam, n_rows, offset, lse, g, dlogits, B, C, eps, stream)
    good = [buf] * 5 + [0] + [buf] * 3 + [4, 7, 0.01, None]
    for i in [0, 1, 2, 3, 4, 6, 7, 8]:
        assert L.hwgat_mbsce_bwd(*(good[:i] + [None] + good[i + 1:])) == EINVAL, i
    for i, bad, rc in ((5, -1, EINVAL), (9, 0, ESHAPE), (10, 65537, ESHAPE)):
        assert L.hwgat_mbsce_bwd(*(good[:i] + [bad] + good[i + 1:])) == rc, (i, bad)
    del keep


# ------------------------------------------------------------------------------------------ what the classes refuse
def test_batch_mixer_refuses_values_outside_its_ranges():
    m = train.BatchMixer()
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob, m.cutmix_share, m.seed, m.step) == (0.4, 1.0, 1.0, 0.5, 0, 0)
    for kw in (dict(mixup_alpha=0.04), dict(mixup_alpha=1.5), dict(cutmix_alpha=0.0), dict(cutmix_alpha=2.0),
               dict(mixup_alpha=math.nan), dict(prob=-0.1), dict(prob=1.1), dict(prob=math.nan), dict(cutmix_share=-1),
               dict(cutmix_share=1.5), dict(prob="1"), dict(prob=True), dict(seed=-1), dict(seed=2 ** 32), dict(seed=1.5),
               dict(seed=True)):
        with pytest.raises(ValueError, match="BatchMixer"):
            train.BatchMixer(**kw)
    train.BatchMixer(mixup_alpha=0.05, cutmix_alpha=1, prob=0, cutmix_share=1, seed=2 ** 32 - 1)
    # a value that changed is refused when it is about to be pushed, before any launch
    m.prob = 2.0
    with pytest.raises(ValueError, match="prob"):
        m.push_hyper()
    m.prob = 0.25
    m.push_hyper()                                            # unbound: nothing to launch
    with pytest.raises(ValueError, match="step"):
        m.step = -1
    m.step = 7
    for bad in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            m.seed = bad
    m.seed = 3
    assert m.seed == 3 and m.step == 7
    m.seed = 0
    sd = m.state_dict()
    assert sd == dict(seed=0, step=7, prob=0.25, cutmix_share=0.5, mixup_alpha=0.4, cutmix_alpha=1.0)
    m2 = train.BatchMixer(seed=9)
    m2.load_state_dict(sd)
    assert m2.state_dict() == sd
    with pytest.raises(ValueError, match="alpha"):
        m2.load_state_dict(dict(sd, mixup_alpha=3.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.bind("cpu", 4, 16)
    with pytest.raises(RuntimeError, match="drawn nothing"):
        m.records()


def test_steps_refuse_a_foreign_criterion_with_a_mixer():
    model = torch.nn.Linear(4, 3)
    x, y = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64)
    for crit in (train.SmoothedCrossEntropyLoss(), train.FusedSmoothedCrossEntropyLoss(),
                 train.BatchSlicedCrossEntropyLoss(), torch.nn.CrossEntropyLoss()):
        with pytest.raises(ValueError, match="two targets and a weight"):
            train.TrainStep(model, None, criterion=crit, mixer=train.BatchMixer())
        with pytest.raises(ValueError, match="two targets and a weight"):
            train.GraphedTrainStep(model, None, x, y, criterion=crit, mixer=train.BatchMixer())
    with pytest.raises(ValueError, match="must be a train.BatchMixer"):
        train.TrainStep(model, None, mixer=object())
    mixer = train.BatchMixer()
    s = train.TrainStep(model, None, mixer=mixer)
    assert type(s.criterion) is train.MixedCrossEntropyLoss and s.criterion.mixer is mixer
    assert isinstance(s.criterion, train.BatchSlicedCrossEntropyLoss)            # what the padded steps ask for
    with pytest.raises(ValueError, match="another BatchMixer"):
        train.TrainStep(model, None, criterion=s.criterion, mixer=train.BatchMixer())
    with pytest.raises(RuntimeError, match="bind_mixer"):
        train.MixedCrossEntropyLoss()(torch.zeros(2, 3), y)
    # without a mixer the criteria are what they were
    assert type(train.TrainStep(model, None).criterion) is train.SmoothedCrossEntropyLoss
    assert type(train.TrainStep(model, None, pad_to=None, mixer=None).criterion) is train.SmoothedCrossEntropyLoss


# ------------------------------------------------------------------------------------------ the numpy restatement
def test_the_gpu_tests_draws_trip_no_margin():
    modes = set()
    for B, n in MH.DRAW_SHAPES:
        y = np.arange(B) % 7
        for k in range(MH.DRAW_STEPS):
            for prob in MH.DRAW_PROBS:
                for share in MH.DRAW_SHARES:
                    rec = MH.draw(MH.DRAW_SEED, MH.DRAW_STEP0 + k, y, n, MH.DRAW_T, prob, share, *MH.DRAW_ALPHAS)
                    modes |= set(rec["mode"].tolist())
                    if prob == 0.0:
                        assert not rec["mode"].any() and (rec["lam"] == 1).all()
                    if prob == 1.0 and n >= 2:
                        want = MH.CUTMIX if share == 1.0 else MH.MIXUP if share == 0.0 else None
                        mixed = rec["mode"][rec["partner"] != np.arange(B)]
                        assert len(mixed) == 2 * (n // 2) and (want is None or (mixed == want).all())
    assert modes == {MH.NONE, MH.MIXUP, MH.CUTMIX}


@pytest.mark.parametrize("alpha", [0.05, 0.4, 1.0])
def test_johnk_sampler_has_the_moments_of_beta(alpha):
    N = 4000
    k_step, _ = MH.step_keys(77, 3)
    draws = np.array([MH.johnk(MH.pair_key(k_step, p), alpha, check=False) for p in range(N)])
    v, tries = draws[:, 0], draws[:, 1]
    assert ((v > 0) & (v <= 1)).all() and tries.max() < MH.BETA_TRIES   # X > 0 always; X / (X + Y) may round to 1 at alpha 0.05
    # Beta(a, a): mean 1/2, variance 1 / (4 (2 a + 1)), excess kurtosis -6 / (2 a + 3)
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    mu4 = var * var * (3.0 - 6.0 / (2.0 * alpha + 3.0))
    se_mean, se_var = math.sqrt(var / N), math.sqrt((mu4 - var * var) / N)
    assert abs(v.mean() - 0.5) <= 5 * se_mean, (v.mean(), se_mean)
    assert abs(v.var() - var) <= 5 * se_var, (v.var(), var, se_var)
    # accepted with probability Gamma(a + 1)^2 / Gamma(2 a + 1) >= 1/2 per try
    accept = math.gamma(alpha + 1) ** 2 / math.gamma(2 * alpha + 1)
    se_tries = math.sqrt((1.0 - accept) / accept ** 2 / N)                            # a geometric law's
    assert accept >= 0.5 and abs(tries.mean() - 1.0 / accept) <= 5 * se_tries, (tries.mean(), accept)


def test_matching_is_a_fixed_point_free_involution_of_the_live_rows():
    seen = set()
    for B, n in MH.DRAW_SHAPES + [(9, 9), (33, 32), (1024, 1001)]:
        for step in range(4):
            rec = MH.draw(3, step, np.zeros(B, dtype=np.int64), n, 16, prob=1.0, cutmix_share=0.0)
            partner = rec["partner"]
            rows = np.arange(B)
            assert (partner[partner] == rows).all()                                  # an involution
            assert (partner[n:] == rows[n:]).all()                                   # the identity on the padding
            fixed = rows[:n][partner[:n] == rows[:n]]
            assert len(fixed) == n % 2                                               # one unpaired row iff n is odd
            assert ((partner[:n] >= 0) & (partner[:n] < max(n, 1))).all()
            pairs, single = MH.matching(3, step, n)
            assert sorted(pairs.reshape(-1).tolist() + ([] if single is None else [single])) == list(range(n))
            assert (rec["pairs"][n // 2:] == -1).all()
            if n % 2:
                assert fixed[0] == single
            if n == 7:
                seen.add(tuple(partner.tolist()))
    assert len(seen) > 1                                                             # another matching every step
