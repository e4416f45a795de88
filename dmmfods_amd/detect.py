"""Heat maps to objects: connected components on the device, object-level precision / recall / AP on the host.

``dmm_heat_components`` (csrc/components.hip) thresholds a ``(B, NC, H, W)`` fp32 map - logits, or a target map the loader rendered -
labels the connected components of every plane and emits one 32-byte record per component: root, inclusive box, area, largest value
(``score``) and where it first occurs (``peak``).  Every output is an integer or a copied input value, so the result is exact and
bit-reproducible.  The ground truth of this project is boxes filled into maps, so the SAME call over the target recovers the
ground-truth objects; ``match_objects`` then pairs predictions with them and ``ObjectMetrics`` accumulates an epoch.

``DeviceObjectMetrics`` does the pairing on the device instead: ``dmm_match_objects`` (csrc/match.hip) restates
``match_plane`` and keeps the epoch's counts and ranked list in device memory; the host classes stay as they are and are its reference.

Nothing here synchronises except ``Detections.to_host()`` and ``DeviceObjectMetrics.state()`` / ``compute()``, once per epoch.
"""
import numpy as np
import torch

from . import _lib

RECORD_DTYPE = np.dtype([("root", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("area", "<i4"),
                         ("score", "<f4"), ("peak", "<i4")])


class PlaneObjects:
    """The objects of one (sample, class) plane on the host: boxes (n, 4) int32 as inclusive x0, y0, x1, y1; areas, peaks, roots (n,)
    int32; scores (n,) float32; ascending roots.  count is the plane's true number of components, overflow says that the device
    kept fewer (count > max_per_plane): min_area filters what was kept, it does not change count."""

    __slots__ = ("boxes", "areas", "scores", "peaks", "roots", "count", "overflow")

    def __init__(self, rec, count, overflow):
        self.boxes = np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], axis=1).astype(np.int32).reshape(-1, 4)
        self.areas, self.scores = rec["area"].copy(), rec["score"].copy()
        self.peaks, self.roots = rec["peak"].copy(), rec["root"].copy()
        self.count, self.overflow = int(count), bool(overflow)

    def __len__(self):
        return self.roots.shape[0]


class Detections:
    """Device results of one HeatMapDetector call: records (B, NC, max_per_plane, 8) int32 - column 6 holds the fp32 bits of the
    score, `scores` is the float view of that column - counts (B, NC) int32, labels (B, NC, H, W) int32 or None."""

    def __init__(self, records, counts, labels, min_area):
        self.records, self.counts, self.labels, self.min_area = records, counts, labels, min_area

    @property
    def scores(self):
        return self.records.view(torch.float32)[..., 6]

    def to_host(self):
        """The one synchronising call.  A list over samples of lists over classes of PlaneObjects."""
        rec = self.records.cpu().numpy()
        cnt = self.counts.cpu().numpy()
        B, NC, cap, _ = rec.shape
        rec = np.ascontiguousarray(rec).view(RECORD_DTYPE).reshape(B, NC, cap)
        out = []
        for b in range(B):
            row = []
            for n in range(NC):
                kept = min(int(cnt[b, n]), cap)
                r = rec[b, n, :kept]
                row.append(PlaneObjects(r[r["area"] >= self.min_area], cnt[b, n], cnt[b, n] > cap))
            out.append(row)
        return out


class HeatMapDetector:
    """threshold: the value a pixel has to reach (>=, fp32) - logit space for logits, map values for a target.  connectivity 4 or 8;
    max_per_plane: records kept per plane (the smallest roots), 1 .. 65536; min_area: Detections.to_host() drops smaller objects."""

    def __init__(self, threshold, connectivity=8, max_per_plane=1024, min_area=1):
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold is NaN")
        if connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8")
        if isinstance(max_per_plane, bool) or int(max_per_plane) != max_per_plane or not 1 <= max_per_plane <= _lib.CC_MAX_PER_PLANE:
            raise ValueError(f"max_per_plane must be an integer in [1, {_lib.CC_MAX_PER_PLANE}]")
        if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 1:
            raise ValueError("min_area must be an integer >= 1")
        self.threshold, self.connectivity = threshold, int(connectivity)
        self.max_per_plane, self.min_area = int(max_per_plane), int(min_area)
        self._workspace = {}   # (device, B, NC, H, W) -> uint8 tensor; a call's scratch, reused by the next call on the same stream

    def _workspace_for(self, device, shape):
        key = (device,) + tuple(shape)
        ws = self._workspace.get(key)
        if ws is None:
            nbytes = _lib.lib().dmm_heat_components_workspace(*shape, self.max_per_plane)
            if nbytes == 0:
                raise ValueError(f"dmm_heat_components refuses the shape {tuple(shape)}")
            ws = self._workspace[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def __call__(self, maps, return_labels=False):
        """Seven launches on the current stream, no synchronisation."""
        if not torch.is_tensor(maps) or not maps.is_cuda:
            raise RuntimeError("dmmfods_amd computes on the GPU only; move the maps to 'cuda' (no CPU fallback)")
        if maps.dim() != 4 or maps.dtype != torch.float32:
            raise ValueError(f"maps must be a (B, NC, H, W) float32 tensor, got {tuple(maps.shape)} {maps.dtype}")
        m = maps.detach().contiguous()
        B, NC, H, W = m.shape
        ws = self._workspace_for(m.device, (B, NC, H, W))
        records = torch.empty((B, NC, self.max_per_plane, 8), dtype=torch.int32, device=m.device)
        counts = torch.empty((B, NC), dtype=torch.int32, device=m.device)
        labels = torch.empty((B, NC, H, W), dtype=torch.int32, device=m.device) if return_labels else None
        _lib.check(_lib.lib().dmm_heat_components(m.data_ptr(), B, NC, H, W, self.threshold, self.connectivity, self.max_per_plane,
                                                  ws.data_ptr(), ws.numel(), labels.data_ptr() if return_labels else None,
                                                  records.data_ptr(), counts.data_ptr(), _lib.stream_ptr()))
        return Detections(records, counts, labels, self.min_area)


def box_iou(a, b):
    """IoU of inclusive pixel boxes (x0, y0, x1, y1), float64: a box covers (x1 - x0 + 1) * (y1 - y0 + 1) pixels."""
    iw = min(int(a[2]), int(b[2])) - max(int(a[0]), int(b[0])) + 1
    ih = min(int(a[3]), int(b[3])) - max(int(a[1]), int(b[1])) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = float(iw) * float(ih)
    area_a = float(int(a[2]) - int(a[0]) + 1) * float(int(a[3]) - int(a[1]) + 1)
    area_b = float(int(b[2]) - int(b[0]) + 1) * float(int(b[3]) - int(b[1]) + 1)
    return inter / (area_a + area_b - inter)


def match_plane(pred, gt, iou=0.5):
    """One (sample, class) plane.  Predictions in descending score, ties to the ascending root; each takes the still unmatched
    ground-truth box of highest IoU >= iou, ties to the ascending root.  Returns a bool array aligned with pred's order."""
    matched = np.zeros(len(pred), dtype=bool)
    order = sorted(range(len(pred)), key=lambda i: (-float(pred.scores[i]), int(pred.roots[i])))
    taken = np.zeros(len(gt), dtype=bool)
    for i in order:
        best, best_iou = -1, -1.0
        for j in range(len(gt)):   # ascending roots: a strict > keeps the first of equal IoUs
            if taken[j]:
                continue
            v = box_iou(pred.boxes[i], gt.boxes[j])
            if v >= iou and v > best_iou:
                best, best_iou = j, v
        if best >= 0:
            taken[best] = True
            matched[i] = True
    return matched


def match_objects(pred, gt, iou=0.5):
    """pred, gt: what Detections.to_host() returns (samples x classes of PlaneObjects).  Returns a dict: matched - per sample and class
    the flags of match_plane - and tp, fp, fn: int64 arrays per class, summed over the samples."""
    if len(pred) != len(gt) or any(len(p) != len(g) for p, g in zip(pred, gt)):
        raise ValueError("pred and gt must cover the same samples and classes")
    nc = len(pred[0]) if pred else 0
    tp, fp, fn = (np.zeros(nc, dtype=np.int64) for _ in range(3))
    flags = []
    for prow, grow in zip(pred, gt):
        frow = []
        for n, (p, g) in enumerate(zip(prow, grow)):
            m = match_plane(p, g, iou)
            frow.append(m)
            tp[n] += int(m.sum())
            fp[n] += int(len(p) - m.sum())
            fn[n] += int(len(g) - m.sum())
        flags.append(frow)
    return {"matched": flags, "tp": tp, "fp": fp, "fn": fn}


def _ratio(num, den):
    """num / den as float64 with 0 / 0 = NaN (iou_from_counts' rule)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0, np.nan, num / np.where(den == 0, 1.0, den))


def average_precision(scores, matched, num_gt):
    """All-point interpolated AP of one class.  The predictions are ranked by descending score (ties keep the order given, which
    ObjectMetrics makes the order of arrival); with tp_k the matched ones among the first k,
        precision_k = tp_k / k,  recall_k = tp_k / num_gt,  p*_k = max_{j >= k} precision_j,
        AP = sum_k (recall_k - recall_{k-1}) * p*_k,  recall_0 = 0,
    in float64.  NaN when num_gt == 0; 0.0 with ground truth and no prediction."""
    if num_gt == 0:
        return float("nan")
    scores, matched = np.asarray(scores, dtype=np.float32), np.asarray(matched, dtype=bool)
    if scores.size == 0:
        return 0.0
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    tp = np.cumsum(matched[order].astype(np.float64))
    k = np.arange(1, scores.size + 1, dtype=np.float64)
    precision, recall = tp / k, tp / float(num_gt)
    envelope = np.maximum.accumulate(precision[::-1])[::-1]
    return float(np.sum(np.diff(np.concatenate([[0.0], recall])) * envelope))


class ObjectMetrics:
    """Object-level metrics of a validation pass.  update() takes the Detections of the predictions and of the ground truth of one
    batch (device objects: it pulls them, ONE synchronisation per batch) or what their to_host() returned."""

    def __init__(self, num_classes, iou=0.5):
        iou = float(iou)
        if not 0.0 < iou <= 1.0:
            raise ValueError("iou must be in (0, 1]")
        self.num_classes, self.iou = int(num_classes), iou
        self.reset()

    def reset(self):
        nc = self.num_classes
        self.tp, self.fp, self.fn = (np.zeros(nc, dtype=np.int64) for _ in range(3))
        self.num_pred, self.num_gt = np.zeros(nc, dtype=np.int64), np.zeros(nc, dtype=np.int64)
        self.overflowed_planes = 0
        self._scores = [[] for _ in range(nc)]
        self._matched = [[] for _ in range(nc)]

    def update(self, pred, gt):
        pred = pred.to_host() if isinstance(pred, Detections) else pred
        gt = gt.to_host() if isinstance(gt, Detections) else gt
        if any(len(row) != self.num_classes for row in pred):
            raise ValueError(f"expected {self.num_classes} classes")
        m = match_objects(pred, gt, self.iou)
        self.tp += m["tp"]
        self.fp += m["fp"]
        self.fn += m["fn"]
        for prow, grow, frow in zip(pred, gt, m["matched"]):
            for n in range(self.num_classes):
                self.num_pred[n] += len(prow[n])
                self.num_gt[n] += len(grow[n])
                self.overflowed_planes += int(prow[n].overflow) + int(grow[n].overflow)
                self._scores[n].append(prow[n].scores)
                self._matched[n].append(frow[n])
        return m

    def compute(self):
        """precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn) per class, 0 / 0 = NaN; ap:
        average_precision over every prediction of the epoch, in order of arrival (batch, sample, root) among equal scores."""
        ap = np.empty(self.num_classes, dtype=np.float64)
        for n in range(self.num_classes):
            s = np.concatenate(self._scores[n]) if self._scores[n] else np.zeros(0, dtype=np.float32)
            f = np.concatenate(self._matched[n]) if self._matched[n] else np.zeros(0, dtype=bool)
            ap[n] = average_precision(s, f, int(self.num_gt[n]))
        return {"precision": _ratio(self.tp, self.tp + self.fp), "recall": _ratio(self.tp, self.tp + self.fn),
                "f1": _ratio(2 * self.tp, 2 * self.tp + self.fp + self.fn), "ap": ap,
                "tp": self.tp.copy(), "fp": self.fp.copy(), "fn": self.fn.copy(),
                "num_pred": self.num_pred.copy(), "num_gt": self.num_gt.copy(), "overflowed_planes": int(self.overflowed_planes)}


TOTALS_FIELDS = ("tp", "fp", "fn", "num_pred", "num_gt", "overflowed_planes", "cursor", "reserved")   # dmm_match_objects' totals row


class DeviceObjectMetrics:
    """ObjectMetrics with the matching on the device: update() is one dmm_match_objects call on the current stream - no
    synchronisation, no to_host() - which adds to an epoch state in device memory: totals (NC, 8) int64 and, per class, the (score
    bits, matched) entries of up to `capacity` predictions in order of arrival.  compute() performs the one synchronisation of the
    epoch and returns ObjectMetrics.compute()'s keys, bit-equal, plus dropped_predictions (NC, int64): the predictions of a class
    that arrived behind its capacity.  They are counted in tp / fp / fn / num_pred; only the AP, which needs every score, is NaN for
    that class."""

    def __init__(self, num_classes, iou=0.5, capacity=1 << 20):
        iou = float(iou)
        if not 0.0 < iou <= 1.0:
            raise ValueError("iou must be in (0, 1]")
        if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= capacity <= 2 ** 31 - 1:
            raise ValueError("capacity must be an integer in [1, 2^31 - 1]")
        self.num_classes, self.iou, self.capacity = int(num_classes), iou, int(capacity)
        self._totals = self._entries = None   # device state, allocated by the first update
        self._workspace = {}                  # (device, B, NC, cap_pred, cap_gt) -> uint8 tensor, as HeatMapDetector's

    def reset(self):
        """Zeroes the epoch state where there is one: a memset on the current stream, no synchronisation."""
        if self._totals is not None:
            self._totals.zero_()

    def _workspace_for(self, device, shape):
        key = (device,) + tuple(shape)
        ws = self._workspace.get(key)
        if ws is None:
            nbytes = _lib.lib().dmm_match_objects_workspace(*shape)
            if nbytes == 0:
                B, NC, cap_pred, cap_gt = shape
                if max(cap_pred, cap_gt) > _lib.MATCH_MAX_PER_PLANE:
                    raise ValueError(f"dmm_match_objects takes at most {_lib.MATCH_MAX_PER_PLANE} records a plane (DMM_MATCH_MAX_PER_PLANE), "
                                     f"got max_per_plane {max(cap_pred, cap_gt)}: lower the detector's max_per_plane or match on the host")
                raise ValueError(f"dmm_match_objects refuses the shape {tuple(shape)}")
            ws = self._workspace[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def update(self, pred, gt, return_matched=False):
        """pred, gt: the Detections of the predictions and of the ground truth of one batch.  Three launches, no synchronisation.
        return_matched: returns the (B, NC, max_per_plane) uint8 device tensor of dmm_match_objects' `matched`."""
        if not isinstance(pred, Detections) or not isinstance(gt, Detections):
            raise TypeError("DeviceObjectMetrics.update takes two Detections (device objects); host lists go to ObjectMetrics")
        pr, gr = pred.records, gt.records
        if pr.dim() != 4 or gr.dim() != 4 or pr.shape[:2] != gr.shape[:2] or pred.counts.shape != pr.shape[:2] or gt.counts.shape != gr.shape[:2]:
            raise ValueError("pred and gt must cover the same samples and classes")
        B, NC, cap_pred, _ = pr.shape
        cap_gt = gr.shape[2]
        if NC != self.num_classes:
            raise ValueError(f"expected {self.num_classes} classes")
        if pred.min_area != gt.min_area:
            raise ValueError(f"pred and gt must share min_area, got {pred.min_area} and {gt.min_area}")
        if not pr.is_cuda or gr.device != pr.device:
            raise RuntimeError("dmmfods_amd computes on the GPU only; the Detections must live on one 'cuda' device (no CPU fallback)")
        ws = self._workspace_for(pr.device, (B, NC, cap_pred, cap_gt))
        if self._totals is None or self._totals.device != pr.device:
            self._totals = torch.zeros((NC, 8), dtype=torch.int64, device=pr.device)
            self._entries = torch.empty((NC, self.capacity, 2), dtype=torch.int32, device=pr.device)
        pr, gr, pc, gc = pr.contiguous(), gr.contiguous(), pred.counts.contiguous(), gt.counts.contiguous()
        matched = torch.empty((B, NC, cap_pred), dtype=torch.uint8, device=pr.device) if return_matched else None
        _lib.check(_lib.lib().dmm_match_objects(pr.data_ptr(), pc.data_ptr(), cap_pred, gr.data_ptr(), gc.data_ptr(), cap_gt, B, NC,
                                                int(pred.min_area), self.iou, ws.data_ptr(), ws.numel(),
                                                matched.data_ptr() if return_matched else None, self._totals.data_ptr(),
                                                self._entries.data_ptr(), self.capacity, _lib.stream_ptr()))
        return matched

    def state(self):
        """The epoch state on the host (ONE synchronisation): a dict of numpy arrays - totals (NC, 8) int64 with the columns
        TOTALS_FIELDS, filled (NC,) int64 = min(cursor, capacity), entries (sum(filled), 2) int32: the filled (score bits, matched)
        rows class after class.  What a multi-rank caller gathers; merge_states() takes a list of them."""
        nc = self.num_classes
        if self._totals is None:
            return {"totals": np.zeros((nc, 8), dtype=np.int64), "filled": np.zeros(nc, dtype=np.int64), "entries": np.zeros((0, 2), dtype=np.int32)}
        totals = self._totals.cpu().numpy()
        filled = np.minimum(totals[:, 6], self.capacity).astype(np.int64)
        parts = [self._entries[n, :int(filled[n])] for n in range(nc)]
        entries = torch.cat(parts).cpu().numpy() if int(filled.sum()) else np.zeros((0, 2), dtype=np.int32)
        return {"totals": totals, "filled": filled, "entries": np.ascontiguousarray(entries, dtype=np.int32)}

    def compute(self):
        return merge_states([self.state()])


def merge_states(states):
    """states: a list of DeviceObjectMetrics.state() dicts (one, or one per rank).  Returns what compute() would have returned had the
    states' updates happened in list order on one device of unbounded capacity: totals added, entries concatenated class by class,
    then ObjectMetrics.compute()'s own arithmetic (_ratio, average_precision).  dropped_predictions adds up what each state dropped
    (cursor - filled); the AP of a class with a dropped prediction is NaN."""
    if not states:
        raise ValueError("merge_states needs at least one state")
    nc = states[0]["totals"].shape[0]
    totals = np.zeros((nc, 8), dtype=np.int64)
    scores, flags = [[] for _ in range(nc)], [[] for _ in range(nc)]
    dropped = np.zeros(nc, dtype=np.int64)
    for s in states:
        t, filled, e = np.asarray(s["totals"], dtype=np.int64), np.asarray(s["filled"], dtype=np.int64), np.asarray(s["entries"], dtype=np.int32)
        if t.shape != (nc, 8) or filled.shape != (nc,) or e.shape != (int(filled.sum()), 2):
            raise ValueError("merge_states: the states do not agree on the number of classes, or one is malformed")
        totals += t
        dropped += t[:, 6] - filled
        first = np.concatenate([[0], np.cumsum(filled)])
        for n in range(nc):
            part = e[first[n]:first[n + 1]]
            scores[n].append(np.ascontiguousarray(part[:, 0]).view(np.float32))
            flags[n].append(part[:, 1] != 0)
    tp, fp, fn, num_pred, num_gt = (totals[:, k].copy() for k in range(5))
    ap = np.empty(nc, dtype=np.float64)
    for n in range(nc):
        ap[n] = average_precision(np.concatenate(scores[n]), np.concatenate(flags[n]), int(num_gt[n])) if dropped[n] == 0 else float("nan")
    return {"precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn), "f1": _ratio(2 * tp, 2 * tp + fp + fn), "ap": ap,
            "tp": tp, "fp": fp, "fn": fn, "num_pred": num_pred, "num_gt": num_gt, "overflowed_planes": int(totals[:, 5].sum()),
            "dropped_predictions": dropped}
