"""GPU: the fused smoothed cross-entropy (csrc/loss_eval.hip: hwgat_sce_fwd / hwgat_sce_bwd), the evaluation accumulator
(hwgat_eval_accumulate), train.FusedSmoothedCrossEntropyLoss in a train step and evaluate.Evaluator.

Values are held against the reference's formula (hwgat/losses/SmoothCrossEntropy.py), restated below and evaluated by
torch in fp64 on the same fp32 logits.  The bound follows tests/test_gpu_stgcn.py: max(FLOOR, 4 x refdev), refdev being the
deviation of the same formula run by torch in fp32 on the CPU from the fp64 result on that input (computed here, never
taken from the kernel).  Integers -- rank, arg-max, every counter of the accumulator -- are exact."""
import functools
import importlib

import pytest
import torch

import stgcn_helpers as SH

pytestmark = pytest.mark.gpu
hw = importlib.import_module("sl-hwgat_amd")
HF = hw.functional
train = importlib.import_module("sl-hwgat_amd.train")
evaluate = importlib.import_module("sl-hwgat_amd.evaluate")
DEV = torch.device("cuda:0")

FLOOR = 2e-5            # observed: row loss 1.8e-7, batch mean 1.1e-7, lse 1.5e-7; gradient entries 1.33e-5 at logit scale 80
                        # (the backward reuses the rounded lse: half an ulp of a number near 300; 2.8e-7 at scale 1);
                        # train-step gradients 3.6e-7 in norm, Evaluator losses 1.3e-7
LDS_ROW = 8192          # SCE_LDS_FLOATS of loss_eval.hip: longer rows are read twice instead of staged
SHAPES = [(1, 1), (1, 2), (3, 5),                 # degenerate rows
          (7, 63), (7, 64), (7, 65),              # one wave's width, one short, one over
          (5, 257),                               # one over a workgroup's width
          (4, 2002),                              # the headline class count, C % 4 != 0
          (2, 4099),                              # several passes per thread, odd
          (3, LDS_ROW), (3, LDS_ROW + 1),         # the longest staged row (16-byte loads) and the first that is not
          (2, LDS_ROW + 4), (3, 20000),           # not staged: 16-byte loads, and scalar
          (300, 10)]                              # many rows
G_UP = 0.37             # upstream gradient of the scalar loss


# ------------------------------------------------------------------------------------------ the reference's formula
def formula(z, y, eps, n=None):
    """(row losses, their mean over the first n rows, lse) of SmoothCrossEntropy.py in z's dtype"""
    lp = torch.log_softmax(z, dim=-1)
    nll = -lp.gather(-1, y.unsqueeze(1)).squeeze(1)
    rows = (1.0 - eps) * nll + eps * (-lp.mean(-1))
    return rows, rows[:n].mean(), torch.logsumexp(z, -1)


def formula_grad(z, y, eps, g, n=None):
    z = z.clone().requires_grad_(True)
    (formula(z, y, eps, n)[1] * g).backward()
    return z.grad


def rel(got, ref):
    """largest error relative to max(1, |ref|), entry by entry"""
    got, ref = got.detach().double().cpu(), ref.double()
    return float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())


def entry(got, ref):
    """largest entry-wise error relative to the largest reference entry"""
    got, ref = got.detach().double().cpu(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def case(B, C, scale, eps):
    """logits, targets, the fp64 reference and the fp32 CPU reference's own deviation from it -- built once per case"""
    g = torch.Generator().manual_seed(1000 * B + C)
    z = torch.randn(B, C, generator=g) * scale
    y = torch.randint(0, C, (B,), generator=g)
    rows, mean, lse = formula(z.double(), y, eps)
    dz = formula_grad(z.double(), y, eps, G_UP)
    rows32, mean32, lse32 = formula(z, y, eps)
    dev = {"rows": rel(rows32, rows), "mean": rel(mean32, mean), "lse": rel(lse32, lse)}
    if C > 1:
        dev["dz"] = entry(formula_grad(z, y, eps, G_UP), dz)
    return z, y, rows, mean, lse, dz, dev


def stable_rank(z, y):
    order = torch.argsort(z, dim=-1, descending=True, stable=True)
    return (order == y.unsqueeze(1)).nonzero()[:, 1].to(torch.int32)


def lowest_argmax(z):
    C = z.shape[1]
    top = z == z.max(-1, keepdim=True).values
    return torch.where(top, torch.arange(C).expand_as(z), C).min(-1).values.to(torch.int32)


def g_dev(v=G_UP):
    return torch.tensor([v], device=DEV, dtype=torch.float32)


# ------------------------------------------------------------------------------------------ kernels: values
@pytest.mark.parametrize("scale", [1.0, 80.0])
@pytest.mark.parametrize("eps", [0.0, 0.01, 0.3])
@pytest.mark.parametrize("B,C", SHAPES)
def test_values_against_fp64(B, C, eps, scale):
    z, y, rows, mean, lse, dz, dev = case(B, C, scale, eps)
    zd, yd = z.to(DEV), y.to(DEV)
    loss, row_loss, lse_k, rank, pred = HF.sce_forward(zd, yd, eps)
    dz_k = HF.sce_backward(zd, yd, lse_k, g_dev(), eps)
    err = {"rows": rel(row_loss, rows), "mean": rel(loss[0], mean), "lse": rel(lse_k, lse)}
    if C > 1:
        err["dz"] = entry(dz_k, dz)
    print(f"WORST_sce B={B} C={C} eps={eps} scale={scale}: " +
          ", ".join(f"{k} {v:.2e} (refdev {dev[k]:.2e})" for k, v in err.items()))
    for k, v in err.items():
        assert v <= max(FLOOR, 4 * dev[k]), (k, v, dev[k])
    if C == 1:
        # floor rule: with one class the gradient is analytically zero (the fp64 formula leaves 1e-17 of rounding), so
        # there is no largest reference entry to divide by.  The kernel's exp(z - lse) is exactly 1; what is left is the
        # fp32 rounding of 1 - (1 - eps) - eps: three roundings of numbers <= 1, at most 3 * 2^-25 < 2^-22, times g / B
        assert float(dz.abs().max()) < 1e-15 and float(dz_k.abs().max()) <= 2.0 ** -22 * G_UP / B
    # the integers on the same input
    assert torch.equal(rank.cpu(), stable_rank(z, y)) and torch.equal(pred.cpu(), lowest_argmax(z))
    assert rank.dtype == pred.dtype == torch.int32


def test_autograd_node_is_the_two_launchers():
    z, y, rows, mean, lse, dz, dev = case(4, 2002, 1.0, 0.01)
    zd = z.to(DEV).requires_grad_(True)
    loss, rank, pred = HF.smooth_ce(zd, y.to(DEV), 0.01)
    assert loss.dim() == 0 and not rank.requires_grad and not pred.requires_grad
    (loss * G_UP).backward()
    assert torch.equal(zd.grad, HF.sce_backward(zd.detach(), y.to(DEV), HF.sce_forward(zd.detach(), y.to(DEV), 0.01)[2],
                                                g_dev(), 0.01))
    assert entry(zd.grad, dz) <= max(FLOOR, 4 * dev["dz"])
    crit = train.FusedSmoothedCrossEntropyLoss()
    assert torch.equal(crit(zd.detach(), y.to(DEV)), loss.detach())
    assert int(crit.correct()) == int((lowest_argmax(z) == y).sum()) == int((crit.last_pred.cpu() == y).sum())


# ------------------------------------------------------------------------------------------ kernels: integers
def _tie_rows(C):
    """rows built to tie, with their targets"""
    g = torch.Generator().manual_seed(C)
    rows, tgt = [], []
    t = C // 2
    r = torch.randn(C, generator=g)
    r[t - 2] = r[t + 2] = r[t]                                  # tied with a lower and a higher index
    rows.append(r), tgt.append(t)
    r = torch.randn(C, generator=g)
    r[0] = r[C - 1] = r[t] = r.max() + 1.0                      # a three-way tie for the maximum, target in the middle
    rows.append(r), tgt.append(t)
    for t_all in (t, 0, C - 1):                                 # all logits equal: target in the middle, first, last
        rows.append(torch.full((C,), 0.25)), tgt.append(t_all)
    r = torch.randn(C, generator=g)
    rows.append(r), tgt.append(0)                               # target first / last on an ordinary row
    rows.append(r.clone()), tgt.append(C - 1)
    r = torch.full((C,), -float("inf"))                         # -inf everywhere but one: still a finite plain CE
    r[3] = 1.5
    rows.append(r), tgt.append(3)
    return torch.stack(rows), torch.tensor(tgt)


@pytest.mark.parametrize("C", [5, 64, 65, 257, 2002, LDS_ROW, LDS_ROW + 1, LDS_ROW + 4])
def test_rank_and_prediction_are_exact_with_ties(C):
    z, y = _tie_rows(C)
    g = torch.Generator().manual_seed(C + 1)
    zq = (torch.randn(6, C, generator=g) * 2).round() / 2        # half-integer logits: ties all over every row
    z, y = torch.cat([z, zq]), torch.cat([y, torch.randint(0, C, (6,), generator=g)])
    loss, row_loss, lse, rank, pred = HF.sce_forward(z.to(DEV), y.to(DEV), 0.0)
    want = stable_rank(z, y)
    assert torch.equal(rank.cpu(), want), (rank.cpu().tolist(), want.tolist())
    assert torch.equal(pred.cpu(), lowest_argmax(z))
    assert rank[1].item() == 1 and rank[2].item() == C // 2 and rank[3].item() == 0 and rank[4].item() == C - 1
    assert torch.equal((rank == 0).cpu(), pred.cpu() == y)      # rank 0 <=> the prediction is the target
    # eps = 0 is plain cross_entropy, -inf logits included
    assert rel(row_loss, torch.nn.functional.cross_entropy(z.double(), y, reduction="none")) <= FLOOR


# ------------------------------------------------------------------------------------------ kernels: n_valid, bad rows
def _acc_parts(acc, C, k_max, cap):
    h = acc.cpu()
    o = 5 + k_max + 1
    logs = h[o + C * C:].view(torch.int32)
    return {"n": int(h[0]), "batches": int(h[1]), "invalid": int(h[2]), "sums": h[3:5].view(torch.float64),
            "hist": h[5:o], "conf": h[o:o + C * C].view(C, C), "pred_log": logs[:cap], "target_log": logs[cap:2 * cap]}


def test_rows_beyond_n_valid_take_no_part():
    B, C, eps, k_max, cap = 6, 37, 0.01, 5, 8
    z, y, rows, _, _, _, dev = case(B, C, 1.0, eps)
    zd, yd = z.to(DEV), y.to(DEV)
    nv = torch.tensor([B - 2], device=DEV, dtype=torch.int32)
    out = (torch.full((1,), 7.5, device=DEV), torch.full((B,), 7.5, device=DEV), torch.full((B,), 7.5, device=DEV),
           torch.full((B,), -9, device=DEV, dtype=torch.int32), torch.full((B,), -9, device=DEV, dtype=torch.int32))
    loss, row_loss, lse, rank, pred = HF.sce_forward(zd, yd, eps, nv, out=out)
    assert rel(loss[0], rows[:B - 2].mean()) <= max(FLOOR, 4 * dev["mean"])
    assert rel(row_loss[:B - 2], rows[:B - 2]) <= max(FLOOR, 4 * dev["rows"])
    for t, s in ((row_loss, 7.5), (lse, 7.5), (rank, -9), (pred, -9)):
        assert (t[B - 2:] == s).all() and not (t[:B - 2] == s).any()
    dz = HF.sce_backward(zd, yd, lse, g_dev(), eps, nv, out=torch.full((B, C), 7.5, device=DEV))
    assert (dz[B - 2:] == 0).all()
    ref = formula_grad(z.double(), y, eps, G_UP, n=B - 2)
    assert entry(dz[:B - 2], ref[:B - 2]) <= max(FLOOR, 4 * entry(formula_grad(z, y, eps, G_UP, n=B - 2), ref))
    acc = torch.zeros(HF.eval_acc_words(C, k_max, cap), device=DEV, dtype=torch.int64)
    HF.eval_accumulate(acc, row_loss, rank, pred, yd, loss, nv, C, k_max, cap)
    a = _acc_parts(acc, C, k_max, cap)
    assert (a["n"], a["batches"], a["invalid"]) == (B - 2, 1, 0)
    assert int(a["hist"].sum()) == int(a["conf"].sum()) == B - 2
    assert a["pred_log"].tolist() == pred[:B - 2].tolist() + [0] * (cap - B + 2)
    assert a["target_log"].tolist() == y[:B - 2].tolist() + [0] * (cap - B + 2)
    assert float(a["sums"][1]) == float(loss[0]) and float(a["sums"][0]) == float(row_loss[:B - 2].double().sum())
    # n_valid = 0: an empty batch is no batch
    before = acc.clone()
    HF.eval_accumulate(acc, row_loss, rank, pred, yd, loss, torch.zeros(1, device=DEV, dtype=torch.int32), C, k_max, cap)
    assert torch.equal(acc, before)


def test_bad_labels_and_nan_rows_are_never_indexed():
    """valid launches on valid buffers: rows whose target is -1 or C, and a row with a NaN logit.  Everything the kernels
    write lies between guard margins that must come back untouched."""
    B, C, eps, k_max, cap, M = 5, 7, 0.01, 3, 4, 64
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, C, generator=g)
    y = torch.tensor([2, -1, 6, C, 0])
    zd, yd = z.to(DEV), y.to(DEV)
    loss, row_loss, lse, rank, pred = HF.sce_forward(zd, yd, eps)
    good = [0, 2, 4]
    rows = formula(z.double()[good], y[good], eps)[0]
    assert rel(row_loss[good], rows) <= FLOOR
    assert torch.isnan(row_loss[[1, 3]]).all() and torch.isnan(loss).all()
    assert rank[[1, 3]].tolist() == [C, C] and torch.equal(rank[good].cpu(), stable_rank(z[good], y[good]))
    assert torch.equal(pred.cpu(), lowest_argmax(z))
    # backward into a guarded buffer
    SENT = -12345.0
    buf = torch.full((M + B * C + M,), SENT, device=DEV)
    dz = HF.sce_backward(zd, yd, lse, g_dev(), eps, out=buf[M:M + B * C].view(B, C))
    assert (buf[:M] == SENT).all() and (buf[M + B * C:] == SENT).all()
    assert torch.isnan(dz[[1, 3]]).all() and torch.isfinite(dz[good]).all()
    # the accumulator between guards
    W = HF.eval_acc_words(C, k_max, cap)
    ISENT = -(1 << 40) - 77
    big = torch.full((M + W + M,), ISENT, device=DEV, dtype=torch.int64)
    acc = big[M:M + W]
    acc.zero_()
    for _ in range(2):                                          # the second call finds the log full after four rows
        HF.eval_accumulate(acc, row_loss, rank, pred, yd, loss, None, C, k_max, cap)
    assert (big[:M] == ISENT).all() and (big[M + W:] == ISENT).all()
    a = _acc_parts(acc, C, k_max, cap)
    assert (a["n"], a["batches"], a["invalid"]) == (2 * B, 2, 4)
    assert int(a["conf"].sum()) == int(a["hist"].sum()) == a["n"] - 4
    assert a["pred_log"].tolist() == pred[:cap].tolist() and a["target_log"].tolist() == [2, -1, 6, -1]
    for i in good:
        assert int(a["conf"][int(y[i]), int(pred[i])]) >= 2
    # a NaN logit: NaN loss, rank C, a prediction in range; the other rows are untouched by it
    zn = z.clone()
    zn[2, 4] = float("nan")
    y_ok = torch.tensor([2, 1, 6, 3, 0])
    loss, row_loss, lse, rank, pred = HF.sce_forward(zn.to(DEV), y_ok.to(DEV), eps)
    assert torch.isnan(row_loss[2]) and torch.isnan(lse[2]) and torch.isnan(loss).all() and rank[2].item() == C
    assert 0 <= pred[2].item() < C
    keep = [0, 1, 3, 4]
    assert rel(row_loss[keep], formula(z.double()[keep], y_ok[keep], eps)[0]) <= FLOOR
    assert torch.equal(rank[keep].cpu(), stable_rank(z[keep], y_ok[keep]))


# ------------------------------------------------------------------------------------------ kernels: determinism
@pytest.mark.parametrize("B,C", [(300, 10), (4, 2002), (3, LDS_ROW + 1)])
def test_every_kernel_is_bit_reproducible(B, C):
    z, y = case(B, C, 80.0, 0.01)[:2]
    zd, yd = z.to(DEV), y.to(DEV)
    runs = []
    for _ in range(2):
        out = HF.sce_forward(zd, yd, 0.01)
        dz = HF.sce_backward(zd, yd, out[2], g_dev(), 0.01)
        acc = torch.zeros(HF.eval_acc_words(C, 5, 16), device=DEV, dtype=torch.int64)
        for _ in range(3):
            HF.eval_accumulate(acc, out[1], out[3], out[4], yd, out[0], None, C, 5, 16)
        runs.append([t.clone() for t in out] + [dz, acc])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                # the double loss sums are compared as their int64 bits
    a = _acc_parts(runs[0][-1], C, 5, 16)
    assert a["n"] == 3 * B and a["batches"] == 3 and int(a["hist"].sum()) == 3 * B


# ------------------------------------------------------------------------------------------ kernels: the one row rule
def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _word(n):
    return torch.tensor([n], device=DEV, dtype=torch.int32)


# (b, C, floats the logits sit past a 16-byte boundary): the cases of tests/test_gpu_graph_micro.py
ROW_RULE_CASES = [(3, 7, 0), (4, 2003, 1), (5, 2002, 0), (3, 2004, 0), (3, 2004, 1)]


@pytest.mark.parametrize("b,C,shift", ROW_RULE_CASES)
def test_slice_at_offset_zero_is_the_batch_with_n_valid_bit_for_bit(b, C, shift):
    """A slice that starts at row 0 of a batch with n real rows has n live rows and divides by n: the same rows, the same
    sums in the same order and the same divisor as the whole batch with n_valid = n.  So loss, the live rows' outputs and
    the whole gradient (exact zeros in the dead rows) agree in every bit; only the empty case differs by rule (slice: 0,
    batch: NaN).  A slice at or beyond the batch's last real row is as empty as one of a batch without rows."""
    eps = 0.01
    g = torch.Generator().manual_seed(1000 * b + C)
    flat = torch.zeros(b * C + 4, device=DEV)
    zd = flat[shift:shift + b * C].view(b, C)
    zd.copy_(torch.randn(b, C, generator=g))
    assert zd.data_ptr() % 16 == 4 * shift and zd.is_contiguous()
    yd = torch.randint(0, C, (b,), generator=g).to(DEV)
    yd[0] = zd[0].argmax()                                   # one row that counts as correct
    up = g_dev()
    for n in range(1, b + 1):
        s_loss, s_rows, s_lse, s_rank, s_pred, correct, live = HF.bsce_forward(zd, yd, eps, _word(n), 0)
        b_loss, b_rows, b_lse, b_rank, b_pred = HF.sce_forward(zd, yd, eps, n_valid=_word(n))
        assert torch.equal(_bits(s_loss), _bits(b_loss)) and torch.isfinite(s_loss).all()
        for s, t in ((s_rows, b_rows), (s_lse, b_lse), (s_rank, b_rank), (s_pred, b_pred)):
            assert torch.equal(_bits(s[:n]), _bits(t[:n]))
        assert int(correct) == int((s_rank[:n] == 0).sum()) >= 1 and int(live) == n
        s_dz = HF.bsce_backward(zd, yd, s_lse, up, eps, _word(n), 0, out=torch.full((b, C), 7.5, device=DEV))
        b_dz = HF.sce_backward(zd, yd, b_lse, up, eps, _word(n), out=torch.full((b, C), 7.5, device=DEV))
        assert torch.equal(_bits(s_dz), _bits(b_dz))
        assert (_bits(s_dz[n:]) == 0).all() and (s_dz[:n] != 0).any(dim=1).all()
    # no live row.  The slice: +0.0 and zeros, from an empty batch and from an offset at or beyond the batch's last real row
    lse = HF.sce_forward(zd, yd, eps)[2]
    for n_rows, offset in ((0, 0), (2, 2), (2, 5)):
        out = HF.bsce_forward(zd, yd, eps, _word(n_rows), offset)
        assert int(_bits(out[0])) == 0 and int(out[5]) == 0 and int(out[6]) == 0
        dz = HF.bsce_backward(zd, yd, lse, up, eps, _word(n_rows), offset, out=torch.full((b, C), 7.5, device=DEV))
        assert (_bits(dz) == 0).all()
    # the batch: an empty mean is NaN; the gradient is zeros all the same
    assert torch.isnan(HF.sce_forward(zd, yd, eps, n_valid=_word(0))[0]).all()
    dz = HF.sce_backward(zd, yd, lse, up, eps, _word(0), out=torch.full((b, C), 7.5, device=DEV))
    assert (_bits(dz) == 0).all()


# ------------------------------------------------------------------------------------------ the criterion in a train step
def _hwgate(training=True):
    """the configuration of tests/test_gpu_graph.py"""
    torch.manual_seed(11)
    hp = hw.HWGATEParams({"src_len": 16, "num_class": 7}, 2, DEV, num_kps=32)
    model = hw.Model(*hp.get_model_params()).to(DEV)
    model.set_activation_dtype(torch.float32)
    model.deterministic_train = True                            # bit-reproducible gradients: runs differ by the criterion alone
    model.train(training)
    if training:
        model.threshold_override = [0.3, 0.1, 0.5, 0.2, 0.07, 0.4, 0.25, 0.6]
    model._drop_calls = 17
    return model


def _clips(model, B=8, nclass=7):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(B, model.temporal_dim, model.num_kps, model.kp_dim, device=DEV, generator=g)
    return x, torch.randint(0, nclass, (B,), device=DEV, generator=g)


class _OneUlpOff(torch.nn.Module):
    """the torch criterion on logits moved by one fp32 ulp each (up or down by position); gradients pass unchanged"""

    def __init__(self):
        super().__init__()
        self.inner = train.SmoothedCrossEntropyLoss()

    def forward(self, out, y):
        o = out.detach()
        i = torch.arange(o.numel(), device=o.device).view_as(o)
        moved = torch.nextafter(o, torch.where(i % 2 == 0, 1.0, -1.0).to(o.dtype) * float("inf"))
        return self.inner(out + (moved - o), y)


def _step(criterion, micro_batch):
    m = _hwgate()
    x, y = _clips(m)
    s = train.TrainStep(m, criterion=criterion, micro_batch=micro_batch)
    loss = s(x, y)
    return float(loss), int(s.correct), {n: p.grad.double().cpu() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("micro_batch", [None, 3])
def test_train_step_with_the_fused_criterion(micro_batch):
    """TrainStep with the fused criterion against the default one.  Each parameter gradient is compared in norm; its bound
    is max(FLOOR, 4 d), d being how far that gradient moves when the TORCH criterion is fed logits one fp32 ulp off --
    the backward's own sensitivity to a rounding-level change of dz, not anything the fused kernels produce.  With
    micro_batch = 3 the 8 clips go as 3 + 3 + 2 and the upstream gradient the backward reads on the device is 3/8, 3/8, 2/8."""
    loss_t, correct_t, grads_t = _step(None, micro_batch)
    loss_f, correct_f, grads_f = _step(train.FusedSmoothedCrossEntropyLoss(), micro_batch)
    _, _, grads_p = _step(_OneUlpOff(), micro_batch)
    assert abs(loss_f - loss_t) <= FLOOR * max(1.0, abs(loss_t)), (loss_f, loss_t)
    assert correct_f == correct_t
    assert set(grads_f) == set(grads_t) and len(grads_t) > 20
    worst = (0.0, 0.0, "")
    for n, gt in grads_t.items():
        norm = float(gt.norm())
        assert norm > 0, n
        d = float((grads_p[n] - gt).norm()) / norm
        e = float((grads_f[n] - gt).norm()) / norm
        worst = max(worst, (e, d, n))
        assert e <= max(FLOOR, 4 * d), (n, e, d)
    print(f"WORST_step micro_batch={micro_batch}: loss {abs(loss_f - loss_t):.2e}, gradient {worst[0]:.2e} "
          f"(one-ulp d {worst[1]:.2e}) at {worst[2]}")


def test_graphed_train_step_equals_eager_with_the_fused_criterion():
    """as test_graphed_train_step_equals_eager of test_gpu_stgcn.py: losses, correct-counts and weights bit for bit over
    4 steps under deterministic_train, across one scheduler step"""
    runs = []
    for graphed in (False, True):
        m = _hwgate()
        x, y = _clips(m)
        o = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
        sched = torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5)
        crit = train.FusedSmoothedCrossEntropyLoss()
        s = train.GraphedTrainStep(m, o, x, y, criterion=crit) if graphed else train.TrainStep(m, o, criterion=crit)
        losses, corrects = [], []
        for i in range(4):
            losses.append(s(x, y).clone())
            corrects.append(int(s.correct))
            if i == 1:
                sched.step()
        runs.append((losses, corrects, [p.detach().clone() for p in m.parameters()]))
    (le, ce, we), (lg, cg, wg) = runs
    assert all(torch.equal(a, b) for a, b in zip(le, lg)), ([float(v) for v in le], [float(v) for v in lg])
    assert ce == cg
    assert all(torch.equal(a, b) for a, b in zip(we, wg))


# ------------------------------------------------------------------------------------------ Evaluator
def _stgcn():
    cfg = SH.CONFIGS["a"]
    m = hw.STGCNModel(*SH.model_args(cfg, 0.0))
    m.load_state_dict(SH.fixture_weights(m.state_dict(), cfg), strict=False)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(21)
    x = torch.rand(11, cfg["T"], cfg["V"], cfg["C"], generator=g).to(DEV)
    return m, x, torch.randint(0, cfg["nclass"], (11,), generator=g).to(DEV), cfg["nclass"]


def _hwgate_eval():
    m = _hwgate(training=False)
    x, y = _clips(m, B=11)
    return m, x, y, 7


def _reference_loop(model, x, y, C, k_max, eps, sizes):
    """the reference's evaluate / predictions_plus_true / gen_cm_w on the model's eager logits, the criterion in fp64"""
    total, hits, preds, conf, rows_sum, i = 0.0, {k: [] for k in range(1, k_max + 1)}, [], torch.zeros(C, C, dtype=torch.int64), 0.0, 0
    with torch.no_grad():
        for n in sizes:
            out = model(x[i:i + n]).float().cpu()
            t = y[i:i + n].cpu()
            rows, mean, _ = formula(out.double(), t, eps)
            total += mean.item()
            rows_sum += rows.sum().item()
            order = torch.argsort(out, dim=-1, descending=True, stable=True)
            for k in hits:
                hits[k] += (order[:, 0:k] == t.unsqueeze(-1)).any(-1).float().tolist()
            p = lowest_argmax(out)
            preds += p.tolist()
            for tr, pr in zip(t.tolist(), p.tolist()):
                conf[tr, pr] += 1
            i += n
    return {"loss": total / len(sizes), "loss_per_sample": rows_sum / i, "acc": {k: sum(v) / len(v) for k, v in hits.items()},
            "confusion": conf, "predictions": preds, "targets": y.cpu().tolist()}


@pytest.mark.parametrize("kind", ["hwgate", "stgcn"])
def test_evaluator_against_the_reference_loop(kind, tmp_path):
    model, x, y, C = _hwgate_eval() if kind == "hwgate" else _stgcn()
    sizes, k_max, eps = (4, 4, 3), 5, 0.01
    ref = _reference_loop(model, x, y, C, k_max, eps, sizes)
    evs = {}
    for graph in (False, True):
        ev = evaluate.Evaluator(model, C, x[:4], k_max=k_max, smooth_factor=eps, graph=graph, log_capacity=16)
        assert ev.result()["n"] == 0                            # construction (warm-up, capture) left nothing behind
        i = 0
        for n in sizes:
            ev.update(x[i:i + n], y[i:i + n])
            i += n
        evs[graph] = ev
    assert torch.equal(evs[False]._acc, evs[True]._acc)         # eager and replayed: bit for bit, loss sums included
    for graph, ev in evs.items():
        r = ev.result()
        assert r["n"] == 11 and r["acc"] == ref["acc"], (r["acc"], ref["acc"])
        assert torch.equal(r["confusion"], ref["confusion"]) and r["confusion"].dtype == torch.int64
        assert ev.predictions() == ref["predictions"] and ev.targets() == ref["targets"]
        for k in ("loss", "loss_per_sample"):
            assert abs(r[k] - ref[k]) <= FLOOR * max(1.0, abs(ref[k])), (k, r[k], ref[k])
        print(f"WORST_eval {kind} graph={graph}: loss {abs(r['loss'] - ref['loss']):.2e}, per sample "
              f"{abs(r['loss_per_sample'] - ref['loss_per_sample']):.2e}")
    ev = evs[True]
    # the zero-padded last batch predicts what its three clips predict alone
    with torch.no_grad():
        alone = lowest_argmax(model(x[8:11]).float().cpu()).tolist()
    assert ev.predictions()[8:] == alone
    # the CSV is the module function on the same matrix
    names = [f"w{i}" for i in range(C)]
    ev.write_confusion_csv(tmp_path / "a.csv", names)
    evaluate.write_confusion_csv(tmp_path / "b.csv", names, ref["confusion"])
    assert (tmp_path / "a.csv").read_text() == (tmp_path / "b.csv").read_text()
    # reset, and a full batch after a short one
    ev.reset()
    z = ev.result()
    assert z["n"] == 0 and z["loss"] == 0.0 and int(z["confusion"].sum()) == 0 and not any(z["acc"].values())
    assert ev.predictions() == [] and int(ev._acc.abs().sum()) == 0
    ev.update(x[:4], y[:4])
    assert ev.result()["n"] == 4 and ev.predictions() == ref["predictions"][:4]
    # a log of 8 sees eleven clips: eight logged, eleven counted
    small = evaluate.Evaluator(model, C, x[:4], k_max=k_max, smooth_factor=eps, graph=False, log_capacity=8)
    i = 0
    for n in sizes:
        small.update(x[i:i + n], y[i:i + n])
        i += n
    assert small.result()["n"] == 11 and small.predictions() == ref["predictions"][:8] and small.targets() == ref["targets"][:8]
    assert torch.equal(small.result()["confusion"], ref["confusion"])
    # a label out of range is reported by result(), the only place that can without a sync per batch
    ev.reset()
    bad = y[:4].clone()
    bad[1], bad[3] = -1, C
    ev.update(x[:4], bad)
    with pytest.raises(ValueError, match="2 of 4 targets"):
        ev.result()
    # refusals: other shapes, CPU tensors, train mode, a reallocated parameter
    with pytest.raises(ValueError):
        ev.update(x[:5], y[:5])
    with pytest.raises(ValueError, match="GPU"):
        ev.update(x[:4].cpu(), y[:4])
    model.train()
    for e in (ev, small):
        with pytest.raises(RuntimeError, match=r"train\(\)"):
            e.update(x[:4], y[:4])
    model.eval()
    p = next(model.parameters())
    p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="capture again"):
        ev.update(x[:4], y[:4])
