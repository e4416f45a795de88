"""Synthetic record arrays for dmm_match_objects and the host reference that goes with them: the inputs of
tests/test_match_gpu.py, tests/test_match_cpu.py and tools/match_cost.py.  Records are made on the host in the layout
dmm_heat_components writes - (B, NC, cap, 8) int32 and (B, NC) counts - so that plane sizes do not depend on images; the reference is
the project's own host path: PlaneObjects built from the same arrays as Detections.to_host() builds them, then match_objects."""
import numpy as np

from dmmfods_amd.detect import RECORD_DTYPE, PlaneObjects, match_objects

FRAME = 512
SCORES = np.asarray([0.75, 0.5, 0.25, 0.0, -0.0, -0.5, -1.25], dtype=np.float32)   # few values: ties are frequent; both zeros; negatives
POISON = np.zeros(1, dtype=RECORD_DTYPE)
POISON["root"], POISON["x0"], POISON["y0"], POISON["x1"], POISON["y1"] = 0x7FFFFFFF, 0, 0, FRAME - 1, FRAME - 1
POISON["area"], POISON["peak"] = 0x7FFFFFFF, -1
POISON["score"] = np.asarray([0x7F800000], dtype=np.uint32).view(np.float32)   # +inf: it would be visited first


def records(boxes, scores=None, areas=None, roots=None):
    """A plane's records from inclusive boxes (x0, y0, x1, y1): ascending roots (0, 1, ... unless given), area 1000 unless given -
    NOT the box area, which the matcher has to take from the corners - and score 0.5 unless given."""
    n = len(boxes)
    r = np.zeros(n, dtype=RECORD_DTYPE)
    b = np.asarray(boxes, dtype=np.int32).reshape(n, 4)
    r["x0"], r["y0"], r["x1"], r["y1"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    r["root"] = np.arange(n) if roots is None else np.asarray(roots)
    r["area"] = 1000 if areas is None else np.asarray(areas)
    r["score"] = 0.5 if scores is None else np.asarray(scores, dtype=np.float32)
    r["peak"] = r["root"]
    assert n < 2 or (np.diff(r["root"]) > 0).all(), "records stand in ascending root order"
    return r


def jittered(P, G, seed, frame=FRAME):
    """P predictions and G ground-truth boxes on a jittered grid in a frame x frame square.  A tenth of the ground truth are one-pixel
    stripes nothing matches (false negatives); seven in ten predictions are a ground-truth box moved by up to a pixel, drawn WITH
    replacement (contests), the others lie anywhere (false positives); scores come from SCORES (ties); areas are 1 .. 100."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(max(P, G, 1))))
    cell = min(max(frame // side, 4), 64)

    def roots(n):
        return np.sort(rng.choice(frame * frame, size=n, replace=False)).astype(np.int32)

    cells = rng.permutation(side * side)[:G] if G <= side * side else rng.integers(0, side * side, G)
    gb = np.zeros((G, 4), dtype=np.int64)
    for j in range(G):
        cy, cx = divmod(int(cells[j]), side)
        w, h = int(rng.integers(cell // 2 + 1, cell + cell // 2 + 2)), int(rng.integers(cell // 2 + 1, cell + cell // 2 + 2))
        if j % 10 == 3:
            w, h = 3 * cell, 1
        x0 = min(max(cx * cell + int(rng.integers(-2, 3)), 0), frame - 2)
        y0 = min(max(cy * cell + int(rng.integers(-2, 3)), 0), frame - 2)
        gb[j] = (x0, y0, min(x0 + w - 1, frame - 1), min(y0 + h - 1, frame - 1))
    pb = np.zeros((P, 4), dtype=np.int64)
    plain = [j for j in range(G) if j % 10 != 3]   # (no prediction is derived from a stripe)
    for i in range(P):
        if plain and rng.random() < 0.7:
            x0, y0, x1, y1 = gb[plain[int(rng.integers(0, len(plain)))]]
            dx, dy = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
            x0, y0 = max(x0 + dx, 0), max(y0 + dy, 0)
            x1, y1 = max(min(x1 + dx + int(rng.integers(0, 2)), frame - 1), x0), max(min(y1 + dy + int(rng.integers(0, 2)), frame - 1), y0)
            pb[i] = (x0, y0, x1, y1)
        else:
            x0, y0 = int(rng.integers(0, frame - cell)), int(rng.integers(0, frame - cell))
            pb[i] = (x0, y0, x0 + int(rng.integers(1, cell)), y0 + int(rng.integers(1, cell)))
    pred = records(pb, scores=SCORES[rng.integers(0, len(SCORES), P)], areas=rng.integers(1, 101, P), roots=roots(P))
    gt = records(gb, areas=rng.integers(1, 101, G), roots=roots(G))
    return pred, gt


def pack(planes, B, NC, cap, counts=None):
    """planes: B * NC record arrays, plane (b, n) at b * NC + n.  Returns the (B, NC, cap, 8) int32 array - the first min(len, cap)
    records of every plane, POISON in every slot behind them - and the (B, NC) int32 counts: len(plane) unless `counts` says otherwise."""
    assert len(planes) == B * NC
    arr = np.repeat(POISON, B * NC * cap).reshape(B, NC, cap)
    cnt = np.zeros((B, NC), dtype=np.int32)
    for i, r in enumerate(planes):
        b, n = divmod(i, NC)
        k = min(len(r), cap)
        arr[b, n, :k] = r[:k]
        cnt[b, n] = len(r)
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.int32).reshape(B, NC)
    return np.ascontiguousarray(arr).view(np.int32).reshape(B, NC, cap, 8), cnt


def to_host(arr, cnt, min_area):
    """Detections.to_host() on host arrays: a list over samples of lists over classes of PlaneObjects."""
    B, NC, cap, _ = arr.shape
    rec = np.ascontiguousarray(arr).view(RECORD_DTYPE).reshape(B, NC, cap)
    out = []
    for b in range(B):
        row = []
        for n in range(NC):
            r = rec[b, n, :max(0, min(int(cnt[b, n]), cap))]
            row.append(PlaneObjects(r[r["area"] >= min_area], cnt[b, n], cnt[b, n] > cap))
        out.append(row)
    return out


def reference(pred_arr, pred_cnt, gt_arr, gt_cnt, min_area, iou):
    """What one dmm_match_objects call must produce, from match_objects: a dict with matched (B, NC, cap_pred) uint8 - the flags
    scattered to their slots -, tp / fp / fn / num_pred / num_gt / overflowed (NC,) int64 and entries: per class the (k, 2) int32
    rows (score bits, matched) in order of arrival (sample, then ascending root)."""
    B, NC, cap_pred, _ = pred_arr.shape
    hp, hg = to_host(pred_arr, pred_cnt, min_area), to_host(gt_arr, gt_cnt, min_area)
    m = match_objects(hp, hg, iou)
    matched = np.zeros((B, NC, cap_pred), dtype=np.uint8)
    rec = np.ascontiguousarray(pred_arr).view(RECORD_DTYPE).reshape(B, NC, cap_pred)
    num_pred, num_gt, over = (np.zeros(NC, dtype=np.int64) for _ in range(3))
    entries = [[] for _ in range(NC)]
    for b in range(B):
        for n in range(NC):
            kept = max(0, min(int(pred_cnt[b, n]), cap_pred))
            slots = np.nonzero(rec[b, n, :kept]["area"] >= min_area)[0]
            flags = m["matched"][b][n]
            assert len(slots) == len(flags)
            matched[b, n, slots] = flags
            num_pred[n] += len(hp[b][n])
            num_gt[n] += len(hg[b][n])
            over[n] += int(hp[b][n].overflow) + int(hg[b][n].overflow)
            entries[n].append(np.stack([hp[b][n].scores.view(np.int32), flags.astype(np.int32)], axis=1).reshape(-1, 2))
    return {"matched": matched, "tp": m["tp"], "fp": m["fp"], "fn": m["fn"], "num_pred": num_pred, "num_gt": num_gt, "overflowed": over,
            "entries": [np.concatenate(e).astype(np.int32) if e else np.zeros((0, 2), dtype=np.int32) for e in entries],
            "host": (hp, hg)}
