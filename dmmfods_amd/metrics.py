"""Validation threshold sweep: every thresholded metric at every threshold from ONE more read of the logits
and targets that ``loss_metrics`` already reads.

``dmm_logit_hist`` (csrc/lhist.hip) bins every logit by the number of thresholds it reaches, split by ground truth, into int64
counts ``(B, NC, 2, K + 1)``.  For threshold ``k`` a prediction is positive when ``bin > k``, so tp / fp / fn / tn - and with them
IoU, precision, recall, F1, accuracy and average precision - are suffix sums of those integers (``curves_from_counts``).  Integer
counts are exact and bit-reproducible, and they add across batches (and across ranks: ``torch.distributed.all_reduce`` sums an int64
tensor exactly) without rounding; nothing waits for the host until the caller asks for numbers.

Thresholds are in LOGIT space, the reference's convention (``config.agent.iou_threshold`` cuts raw logits);
``probabilities=`` converts."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MAX_THRESHOLDS = _lib.HIST_MAX_THRESHOLDS


def logit_thresholds(probabilities):
    """p -> log(p / (1 - p)), formed in double and rounded once to fp32; every p must lie in (0, 1)."""
    out = []
    for p in probabilities:
        p = float(p)
        if not 0.0 < p < 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"probabilities must lie in (0, 1), got {p}")
        out.append(math.log(p / (1.0 - p)))
    return np.asarray(out, dtype=np.float64).astype(np.float32)


def _ratio(num, den):
    return num.double() / den.double()   # 0/0 = NaN, iou_from_counts' rule


def curves_from_counts(counts):
    """counts: int64 (..., NC, 2, K + 1), ``counts[..., g, j]`` = elements with ground truth g whose logit reaches exactly j thresholds.
    Returns a dict: the integer counts tp, fp, fn, tn (..., NC, K) and, in float64, iou, precision, recall, f1, accuracy (0/0 = NaN)
    and average_precision (..., NC).  Pure torch, on the device of `counts`."""
    if counts.dtype != torch.int64 or counts.dim() < 3 or counts.shape[-2] != 2 or counts.shape[-1] < 2:
        raise ValueError("counts must be an int64 tensor of shape (..., NC, 2, K + 1)")
    # suffix sums: above[.., j] = sum_{i >= j} counts[.., i]; threshold k takes j = k + 1
    above = counts.flip(-1).cumsum(-1).flip(-1)
    tp, fp = above[..., 1, 1:], above[..., 0, 1:]
    P, N = above[..., 1, :1], above[..., 0, :1]
    fn, tn = P - tp, N - fp
    precision, recall = _ratio(tp, tp + fp), _ratio(tp, tp + fn)
    # sum_k (recall[k] - recall[k + 1]) * precision[k] with recall[K] = 0; a NaN precision (nothing predicted) is taken as 0: its
    # recall step is 0 anyway.  Without positives every recall is NaN and so is the result.
    r_next = torch.cat([recall[..., 1:], torch.zeros_like(recall[..., :1])], dim=-1)
    ap = ((recall - r_next) * torch.nan_to_num(precision, nan=0.0)).sum(-1)
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn,
            "iou": _ratio(tp, tp + fp + fn), "precision": precision, "recall": recall, "f1": _ratio(2 * tp, 2 * tp + fp + fn),
            "accuracy": _ratio(tp + tn, P + N), "average_precision": ap}


class ThresholdSweep:
    """Accumulates the histograms of a validation pass.  Exactly one of `thresholds` (logit space) or `probabilities` is given;
    at most 255 values, strictly ascending as fp32 values."""

    def __init__(self, num_classes, thresholds=None, probabilities=None, gt_threshold=0.7):
        if (thresholds is None) == (probabilities is None):
            raise ValueError("give exactly one of thresholds (logit space) or probabilities")
        if int(num_classes) < 1:
            raise ValueError("num_classes must be >= 1")
        if thresholds is not None:
            thr = np.asarray([float(v) for v in thresholds], dtype=np.float64).astype(np.float32)
        else:
            thr = logit_thresholds(probabilities)
        if thr.ndim != 1 or not 1 <= thr.size <= MAX_THRESHOLDS:
            raise ValueError(f"between 1 and {MAX_THRESHOLDS} thresholds, got {thr.size}")
        if not np.isfinite(thr).all():
            raise ValueError("thresholds must be finite (no NaN, no infinity)")
        if not (np.diff(thr) > 0).all():
            raise ValueError("thresholds must be strictly ascending as fp32 values (sorted, no duplicates after rounding)")
        gt = float(gt_threshold)
        if math.isnan(gt):
            raise ValueError("gt_threshold is NaN")
        self.num_classes, self.gt_threshold = int(num_classes), gt
        self.thresholds = thr
        self._thr_c = (C.c_float * thr.size)(*thr.tolist())   # host memory: the values travel by value with every launch
        self.reset()

    @property
    def num_thresholds(self):
        return int(self.thresholds.size)

    def reset(self):
        self.counts = None        # int64 (NC, 2, K + 1): the dataset totals, made on the first batch's device
        self._batch_curves = []   # per batch: the reference-style IoU curve (NC, K), float32, on the device

    def update(self, logits, target):
        """One dmm_logit_hist launch on the current stream, no synchronisation.  Returns the batch's (B, NC, 2, K + 1) int64 counts."""
        if not (torch.is_tensor(logits) and torch.is_tensor(target)) or not logits.is_cuda or not target.is_cuda:
            raise RuntimeError("dmmfods_amd computes on the GPU only; move logits and target to 'cuda' (no CPU fallback)")
        if logits.dim() != 4 or logits.shape != target.shape or logits.shape[1] != self.num_classes:
            raise ValueError(f"logits and target must both be (B, {self.num_classes}, H, W), got {tuple(logits.shape)} and {tuple(target.shape)}")
        lg, t = logits.detach().contiguous().float(), target.detach().contiguous().float()
        B, NC, H, W = lg.shape
        K = self.num_thresholds
        batch = torch.empty((B, NC, 2, K + 1), dtype=torch.int64, device=lg.device)
        _lib.check(_lib.lib().dmm_logit_hist(lg.data_ptr(), t.data_ptr(), B, NC, H, W, C.addressof(self._thr_c), K, self.gt_threshold, 0,
                                             batch.data_ptr(), _lib.stream_ptr()))
        total = batch.sum(dim=0)
        self.counts = total if self.counts is None else self.counts + total
        self._batch_curves.append(self._reference_iou(batch))
        return batch

    @staticmethod
    def _reference_iou(batch):
        """The agent's per-batch IoU (Agent._batch_metrics: per-sample IoU in fp32, NaN-mean over the samples, all-NaN -> 0), the same
        operations in the same order, at every threshold: (NC, K)."""
        c = curves_from_counts(batch)
        iou = (c["tp"].double() / (c["tp"] + c["fp"] + c["fn"]).double()).float()
        nan = torch.isnan(iou)
        cnt = (~nan).sum(dim=0).clamp_min(1)
        iou_pc = torch.where(nan, torch.zeros_like(iou), iou).sum(dim=0) / cnt
        return torch.where((~nan).any(dim=0), iou_pc, torch.zeros_like(iou_pc))

    def compute(self):
        """curves_from_counts of the totals plus thresholds, iou_per_instance (the mean over the batches of the reference-style
        curve) and, per class, best_threshold / best_iou: the argmax of the dataset-level IoU, NaN as -inf, first index on ties.
        Everything stays on the device."""
        if self.counts is None:
            raise RuntimeError("compute() needs at least one update()")
        out = curves_from_counts(self.counts)
        dev = self.counts.device
        thr = torch.from_numpy(self.thresholds.copy()).to(dev)
        out["thresholds"] = thr
        # (a mean over the stacked rows: the operation the agent applies to its per-batch IoU rows, so that the two agree bit for bit)
        out["iou_per_instance"] = torch.stack(self._batch_curves).mean(0)
        iou = torch.nan_to_num(out["iou"], nan=-math.inf)
        best = iou.max(dim=-1, keepdim=True).values
        K = self.num_thresholds
        idx = torch.where(iou == best, torch.arange(K, device=dev).expand_as(iou), torch.full_like(iou, K, dtype=torch.int64)).min(dim=-1).values
        out["best_threshold"] = thr[idx]
        out["best_iou"] = out["iou"].gather(-1, idx.unsqueeze(-1)).squeeze(-1)
        return out
