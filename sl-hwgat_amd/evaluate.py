"""Evaluation loop without a host round trip per batch.

The reference's `evaluate` (hwgat/utils.py:118-142) reads `loss.item()` and `.cpu().tolist()` after every batch and sorts all
classes for its top-k; `predictions_plus_true` and `gen_cm_w` (utils.py:144-161, 324-350) walk the loader again for the
confusion list.  Here one forward per batch feeds two kernels (csrc/loss_eval.hip): the smoothed cross-entropy with the
target's rank and the arg-max, and an accumulator that keeps sample / batch counts, both loss sums, the rank histogram, the
confusion matrix and (optionally) the prediction log on the device.  `update` synchronises nothing; `result()` is the only
host read.

    evaluate = importlib.import_module("sl-hwgat_amd.evaluate")
    ev = evaluate.Evaluator(model, num_classes, example, k_max=5)
    ev.reset()
    for x, y in loader:
        ev.update(x.to(dev), y.to(dev))       # the last batch may have fewer rows than `example`
    r = ev.result()                           # loss, loss_per_sample, acc[k], n, confusion

With `graph=True` the eval forward and the two kernels are captured once (serve.GraphedEval with a tail) and replayed;
inputs, targets and the row count live in static device buffers.  A short batch is zero-padded and the row count is set
on the device, so it needs no second capture.  Padding is safe because in eval() every model of this package treats
clips independently: BatchNorm reads its running statistics and attention never crosses clips.

Summing the accumulators of several ranks is not implemented: it would be one integer / double all-reduce of the block
before `result()`, and nothing here can exercise it on one GPU.
"""
import csv

import numpy as np
import torch

from . import functional as HF
from . import serve


def write_confusion_csv(path, class_names, confusion):
    """the file gen_cm_w writes (utils.py:338-350): header word,total,predicted; per true class `Word-<name>`, the row
    total and the non-zero predicted classes as `word-<name>(<count>) ` in class order.  The reference counts in a float
    matrix, so totals and counts print as floats (3.0)."""
    cm = np.asarray(confusion)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or len(class_names) != cm.shape[0]:
        raise ValueError(f"need a square matrix and one name per class, got {cm.shape} and {len(class_names)} names")
    with open(path, "w") as fh:
        w = csv.writer(fh)
        w.writerow(["word", "total", "predicted"])
        for i, row in enumerate(cm):
            predicted = "".join(f"word-{class_names[j]}({float(c)}) " for j, c in enumerate(row) if c > 0)
            w.writerow([f"Word-{class_names[i]}", str(float(row.sum())), predicted])


class Evaluator:
    """`example` fixes the batch shape (its first dimension is the largest batch `update` takes).  `k_max`: top-k accuracies
    are kept for k = 1..k_max.  `log_capacity` > 0 keeps the first that many (prediction, target) pairs for
    `predictions()` / `targets()`; rows past it are still counted."""

    def __init__(self, model, num_classes, example, k_max=5, smooth_factor=0.01, graph=True, log_capacity=0):
        if not example.is_cuda:
            raise ValueError("the example input must live on the GPU")
        if k_max < 1 or log_capacity < 0:
            raise ValueError(f"k_max must be at least 1 and log_capacity non-negative, got {k_max} and {log_capacity}")
        self.num_classes, self.k_max, self.smooth_factor = int(num_classes), int(k_max), float(smooth_factor)
        self.log_capacity = int(log_capacity)
        dev, B = example.device, example.shape[0]
        self._acc = torch.zeros(HF.eval_acc_words(self.num_classes, self.k_max, self.log_capacity), device=dev,
                                dtype=torch.int64)
        self._y = torch.zeros(B, device=dev, dtype=torch.int64)
        self._n_valid = torch.full((1,), B, device=dev, dtype=torch.int32)
        self._rows = B                                        # what _n_valid holds, mirrored on the host
        self._runner = serve.GraphedEval(model, torch.zeros_like(example), tail=self._tail, graph=graph)
        self.reset()                                          # warm-up and capture ran the tail on the zero batch

    def _tail(self, logits):
        z = logits.float().contiguous()
        loss, row_loss, _, rank, pred = HF.sce_forward(z, self._y, self.smooth_factor, self._n_valid)
        HF.eval_accumulate(self._acc, row_loss, rank, pred, self._y, loss, self._n_valid, self.num_classes, self.k_max,
                           self.log_capacity)
        return loss, rank, pred

    def reset(self):
        self._acc.zero_()

    def update(self, x, y):
        """fold one batch in: x (n, ...) with 1 <= n <= the example's batch, y (n,) integer labels, both on the device"""
        sin = self._runner.static_in
        if not x.is_cuda or not y.is_cuda:
            raise ValueError("inputs and targets must live on the GPU")
        n = x.shape[0]
        if not 1 <= n <= sin.shape[0] or x.shape[1:] != sin.shape[1:] or x.dtype != sin.dtype or y.shape != (n,):
            raise ValueError(f"built for up to {sin.shape[0]} clips of {tuple(sin.shape[1:])} {sin.dtype}, got "
                             f"{tuple(x.shape)} {x.dtype} with targets {tuple(y.shape)}")
        self._runner.check()
        sin[:n].copy_(x, non_blocking=True)
        self._y[:n].copy_(y, non_blocking=True)
        if n != self._rows:
            sin[n:].zero_()                                   # rows a longer batch left behind
            self._y[n:].zero_()
            self._n_valid.fill_(n)
            self._rows = n
        self._runner._replay()

    def _host(self, lo, hi):
        """words [lo, hi) of the accumulator block on the host (synchronises)"""
        return self._acc[lo:hi].cpu().numpy()

    def result(self):
        """{"loss": sum of batch means / batches (utils.py:131,142), "loss_per_sample", "acc": {k: top-k accuracy per
        sample}, "n", "confusion": (C, C) int64 CPU tensor}; raises when a target was outside [0, num_classes)"""
        C, H = self.num_classes, HF.EVAL_ACC_HEADER_WORDS
        h = self._host(0, H + self.k_max + 1 + C * C)             # everything but the log
        n, n_batches, n_invalid = (int(v) for v in h[:3])
        if n_invalid > 0:
            raise ValueError(f"{n_invalid} of {n} targets were outside [0, {C}): they are in no statistic")
        sums = h[3:H].view(np.float64)
        hist = h[H:H + self.k_max + 1]
        conf = h[H + self.k_max + 1:].reshape(C, C)
        return {"loss": float(sums[1]) / max(n_batches, 1), "loss_per_sample": float(sums[0]) / max(n, 1),
                "acc": {k: int(hist[:k].sum()) / max(n, 1) for k in range(1, self.k_max + 1)}, "n": n,
                "confusion": torch.from_numpy(conf.copy())}

    def _log(self, which):
        if self.log_capacity == 0:
            raise ValueError("built with log_capacity=0: no predictions were logged")
        start = HF.EVAL_ACC_HEADER_WORDS + self.k_max + 1 + self.num_classes ** 2
        kept = min(int(self._host(0, 1)[0]), self.log_capacity)
        logs = self._host(start, start + self.log_capacity).view(np.int32)
        return logs[which * self.log_capacity:which * self.log_capacity + kept].tolist()

    def predictions(self):
        """the logged arg-max classes, in the order the clips came (what predictions_plus_true returns as y_pred)"""
        return self._log(0)

    def targets(self):
        return self._log(1)

    def write_confusion_csv(self, path, class_names):
        write_confusion_csv(path, class_names, self.result()["confusion"].numpy())
