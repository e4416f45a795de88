"""dmm_match_objects and DeviceObjectMetrics on the GPU against the project's own host path: PlaneObjects built
from the same record arrays, then match_objects, ObjectMetrics and average_precision (tools/match_cases.py).  Integers are compared
exactly, fp64 results bit for bit (NaN equal to NaN), entries as int32 bits.

Every direct call is set up the same way (_call): the slots behind a plane's kept records hold a poison record - a huge area, a
frame-wide box, score bits 0x7f800000 -, `matched` sits between sentinel margins, totals and entries are pre-loaded with non-zero
values (the call ADDS to totals and writes entries from the pre-loaded cursor on, nothing else), entries has a guard band behind it,
and the inputs are compared with copies afterwards."""
import collections
import functools

import numpy as np
import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
from tools import components_patterns as P
from tools import match_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 64
ENTRY_FILL = 0x5A5A5A5A
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)


def _preload(NC):
    """Non-zero totals: every field of every class differs; cursor (column 6) is 3 + 2 n."""
    t = (np.arange(NC * 8, dtype=np.int64).reshape(NC, 8) + 1) * 1000003
    t[:, 6] = 3 + 2 * np.arange(NC)
    return t


def _call(pred, pc, gt, gc, min_area=1, iou=0.5, capacity=None, totals0=None, with_matched=True):
    """One dmm_match_objects call on host arrays.  Returns (matched (B, NC, cap_pred) uint8, totals delta (NC, 8) int64, entries: per
    class the rows the call wrote, (k, 2) int32) after checking everything that must not have changed."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    B, NC, cap_pred, _ = pred.shape
    cap_gt = gt.shape[2]
    totals0 = _preload(NC) if totals0 is None else totals0
    if capacity is None:
        capacity = int(totals0[:, 6].max()) + B * cap_pred + 5
    d_pred, d_pc, d_gt, d_gc = (torch.from_numpy(np.array(x)).to(DEV) for x in (pred, pc, gt, gc))   # (copies: the cached cases are read-only)
    nbytes = L.dmm_match_objects_workspace(B, NC, cap_pred, cap_gt)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=DEV)
    n_m = B * NC * cap_pred
    m_buf = torch.full((MARGIN + n_m + MARGIN,), 0xAB, dtype=torch.uint8, device=DEV)
    totals = torch.from_numpy(totals0.copy()).to(DEV)
    e_buf = torch.full((NC * capacity * 2 + MARGIN,), ENTRY_FILL, dtype=torch.int32, device=DEV)
    m_ptr = m_buf.data_ptr() + MARGIN if with_matched else None
    _lib.check(L.dmm_match_objects(d_pred.data_ptr(), d_pc.data_ptr(), cap_pred, d_gt.data_ptr(), d_gc.data_ptr(), cap_gt, B, NC, min_area, iou,
                                   ws.data_ptr(), nbytes, m_ptr, totals.data_ptr(), e_buf.data_ptr(), capacity, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for dev, host in ((d_pred, pred), (d_pc, pc), (d_gt, gt), (d_gc, gc)):
        assert np.array_equal(dev.cpu().numpy(), host), "an input was written"
    m = m_buf.cpu().numpy()
    assert (m[:MARGIN] == 0xAB).all() and (m[MARGIN + n_m:] == 0xAB).all(), "matched: a margin was written"
    if not with_matched:
        assert (m == 0xAB).all()
    e = e_buf.cpu().numpy()
    assert (e[NC * capacity * 2:] == ENTRY_FILL).all(), "entries: the guard band was written"
    e = e[:NC * capacity * 2].reshape(NC, capacity, 2)
    delta = totals.cpu().numpy() - totals0
    assert (delta[:, 7] == 0).all() and (delta[:, 6] == delta[:, 3]).all(), "reserved moved, or cursor and num_pred advanced differently"
    rows = []
    for n in range(NC):
        lo, hi = int(totals0[n, 6]), int(totals0[n, 6] + delta[n, 6])
        assert (e[n, :min(lo, capacity)] == ENTRY_FILL).all() and (e[n, min(hi, capacity):] == ENTRY_FILL).all(), "entries outside the call's range were written"
        rows.append(e[n, min(lo, capacity):min(hi, capacity)].copy())
    return m[MARGIN:MARGIN + n_m].reshape(B, NC, cap_pred), delta, rows


def _check(pred, pc, gt, gc, min_area=1, iou=0.5):
    """The call against the host reference; returns the reference."""
    want = M.reference(pred, pc, gt, gc, min_area, iou)
    matched, delta, rows = _call(pred, pc, gt, gc, min_area, iou)
    assert np.array_equal(matched, want["matched"]), np.argwhere(matched != want["matched"])[:10]
    for k, col in (("tp", 0), ("fp", 1), ("fn", 2), ("num_pred", 3), ("num_gt", 4), ("overflowed", 5)):
        assert np.array_equal(delta[:, col], want[k]), (k, delta[:, col], want[k])
    for n, (g, w) in enumerate(zip(rows, want["entries"])):
        assert g.shape == w.shape and np.array_equal(g, w), (n, g[:8], w[:8])
    return want


def _one_plane(pred, gt, cap_pred=None, cap_gt=None, **kw):
    pa, pc = M.pack([pred], 1, 1, cap_pred or max(len(pred), 1))
    ga, gc = M.pack([gt], 1, 1, cap_gt or max(len(gt), 1))
    return _check(pa, pc, ga, gc, **kw)


def _boxes(n, seed):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, 100, n), rng.integers(0, 100, n)
    return np.stack([x0, y0, x0 + rng.integers(0, 20, n), y0 + rng.integers(0, 20, n)], axis=1)


# ------------------------------------------------------------------------------------------------ 1. empty sides
@pytest.mark.parametrize("pg", [(0, 0), (0, 3), (3, 0)])
def test_empty_sides(pg):
    p, g = pg
    b = _boxes(3, 1)
    want = _one_plane(M.records(b[:p]), M.records(b[:g]), cap_pred=5, cap_gt=4)
    assert want["tp"][0] == 0 and want["fp"][0] == p and want["fn"][0] == g


def test_a_batch_without_any_record():
    pa, pc = M.pack([M.records([])] * 6, 2, 3, 7)
    ga, gc = M.pack([M.records([])] * 6, 2, 3, 9)
    want = _check(pa, pc, ga, gc)
    assert not want["matched"].any() and all(len(e) == 0 for e in want["entries"])


# ------------------------------------------------------------------------------------------------ 2. contests
def test_two_predictions_over_one_box():
    # both predictions are the first box; the loser's second best is 6 x 10 of 140 = 0.43 (a false positive) or 8 x 10 of 120 = 0.67
    for second, loser_matches in (((14, 10, 23, 19), False), ((12, 10, 21, 19), True)):
        gt = M.records([(10, 10, 19, 19), second])
        pred = M.records([(10, 10, 19, 19), (10, 10, 19, 19)], scores=[0.2, 0.9])   # the later root has the higher score: it wins
        want = _one_plane(pred, gt)
        assert want["matched"][0, 0].tolist() == [int(loser_matches), 1] and want["tp"][0] == 1 + loser_matches


def test_a_chain_of_five_where_each_choice_displaces_the_next():
    # ground truth g0 .. g3, 10 wide, every 4 pixels.  X is g0 itself; p_k sits one pixel right of g_k: 0.82 with g_k, 0.54 with g_k+1.
    # Visited X, p0, p1, p2, p3: X takes g0, so p0 falls back to g1, so p1 falls back to g2, so p2 to g3, and p3 finds g3 gone.
    gt = M.records([(4 * k, 0, 4 * k + 9, 9) for k in range(4)])
    boxes = [(4 * k + 1, 0, 4 * k + 10, 9) for k in (3, 2, 1, 0)] + [(0, 0, 9, 9)]     # slots: p3, p2, p1, p0, X - scores ascending
    want = _one_plane(M.records(boxes, scores=[0.1, 0.2, 0.3, 0.4, 0.5]), gt)
    assert want["matched"][0, 0].tolist() == [0, 1, 1, 1, 1]
    want = _one_plane(M.records(boxes, scores=[0.1, 0.2, 0.3, 0.4, 0.5]), gt, iou=0.6)   # no fall-back reaches 0.6: p0 fails, p1 .. p3 keep their own
    assert want["matched"][0, 0].tolist() == [1, 1, 1, 0, 1]


# ------------------------------------------------------------------------------------------------ 3. score ties
@pytest.mark.parametrize("scores", [[0.5, 0.5, 0.5], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [-3.0, -1.0, -2.0], [-1.0, 2.0, -0.0], [1e-40, -1e-40, 0.0]])
def test_score_ties_and_signs(scores):
    # three predictions over ONE box: only the first visited matches - the highest score, the lowest root among equals
    pred = M.records([(0, 0, 9, 9)] * 3, scores=scores, roots=[5, 17, 40])
    want = _one_plane(pred, M.records([(0, 0, 9, 9)]))
    s = np.asarray(scores, dtype=np.float32)
    assert want["matched"][0, 0].tolist() == [int(i == int(np.argmax(s))) for i in range(3)]   # (argmax: the first of equal maxima)


# ------------------------------------------------------------------------------------------------ 4. IoU ties and edges
def test_two_boxes_of_equal_iou_go_to_the_lower_root():
    # the first prediction overlaps both boxes by 8 x 10 of 120; the second IS the box of root 3 and overlaps the other by 0.43
    pred = M.records([(10, 0, 19, 9), (12, 0, 21, 9)], scores=[0.9, 0.1])
    for boxes in ([(12, 0, 21, 9), (8, 0, 17, 9)], [(8, 0, 17, 9), (12, 0, 21, 9)]):
        want = _one_plane(pred, M.records(boxes, roots=[3, 8]), iou=0.6)
        # the first takes root 3 either way; the second is left without its own box only where root 3 was that box
        assert want["matched"][0, 0].tolist() == [1, int(boxes[0] != (12, 0, 21, 9))]


def test_iou_on_the_threshold_and_around_it():
    # 2 of 4 pixels at 0.5; 3 of 10 at 0.3 (3.0 / 10.0 is the double the literal 0.3 is); 7 of 25 at 0.28, where the quotient reaches the
    # literal and the multiplied form 7 >= 0.28 * 25 = 7.000000000000001 does not; identical boxes at 1.0
    for pb, gb, iou, hit in (((0, 0, 1, 0), (1, 0, 3, 0), 0.5, False),               # 1 of 4
                             ((0, 0, 2, 0), (1, 0, 3, 0), 0.5, True),                # 2 of 4
                             ((0, 0, 5, 0), (3, 0, 9, 0), 0.3, True),                # 3 of 10
                             ((0, 0, 5, 0), (3, 0, 9, 0), float(np.nextafter(0.3, 1)), False),
                             ((0, 0, 15, 0), (9, 0, 24, 0), 0.28, True),             # 7 of 25
                             ((5, 5, 20, 30), (5, 5, 20, 30), 1.0, True),
                             ((5, 5, 20, 30), (5, 5, 20, 31), 1.0, False),
                             ((5, 5, 20, 30), (6, 5, 21, 30), 1.0, False),
                             ((0, 0, 9, 9), (10, 0, 19, 9), 1e-300, False),          # touching, iw == 0
                             ((0, 0, 9, 9), (0, 10, 9, 19), 1e-300, False),          # touching, ih == 0
                             ((0, 0, 9, 9), (9, 9, 500, 500), 1e-300, True)):        # one pixel in common
        assert 3.0 / 10.0 >= 0.3 and 7.0 / 25.0 >= 0.28 and not 7.0 >= 0.28 * 25.0
        want = _one_plane(M.records([pb]), M.records([gb]), iou=iou)
        assert bool(want["tp"][0]) is hit, (pb, gb, iou)


# ------------------------------------------------------------------------------------------------ 5. sizes across the wave and the workgroup
SIZES = [(63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (600, 600), (4096, 33), (33, 4096)]


@functools.lru_cache(maxsize=None)
def _jittered(P_, G_):
    pred, gt = M.jittered(P_, G_, seed=1000 + P_)
    pa, pc = M.pack([pred], 1, 1, P_)
    ga, gc = M.pack([gt], 1, 1, G_)
    for a in (pa, pc, ga, gc):
        a.setflags(write=False)
    return pa, pc, ga, gc


@pytest.mark.parametrize("pg", SIZES, ids=lambda pg: f"{pg[0]}x{pg[1]}")
def test_sizes_across_the_wave_and_the_workgroup(pg):
    want = _check(*_jittered(*pg))
    assert want["tp"][0] > 0 and want["fp"][0] > 0 and want["fn"][0] > 0, (want["tp"], want["fp"], want["fn"])


# ------------------------------------------------------------------------------------------------ 6. min_area
@pytest.mark.parametrize("min_area", [1, 2, 50])
def test_min_area_filters_both_sides(min_area):
    pred, gt = M.jittered(300, 280, seed=7)
    rng = np.random.default_rng(8)
    pred["area"] = np.where(np.arange(300) % 3 == 1, rng.integers(1, 3, 300), rng.integers(50, 400, 300))   # small ones interleaved by root
    gt["area"] = np.where(np.arange(280) % 4 == 2, rng.integers(1, 3, 280), rng.integers(49, 400, 280))
    pa, pc = M.pack([pred], 1, 1, 300)
    ga, gc = M.pack([gt], 1, 1, 280)
    want = _check(pa, pc, ga, gc, min_area=min_area)
    small = pred["area"] < min_area
    assert not want["matched"][0, 0][small].any() and want["num_pred"][0] == int((~small).sum()) == len(want["entries"][0])
    assert want["num_gt"][0] == int((gt["area"] >= min_area).sum()) and want["tp"][0] > 0
    if min_area > 1:
        assert small.any() and (gt["area"] < min_area).any()


# ------------------------------------------------------------------------------------------------ 7. overflow
@pytest.mark.parametrize("side", ["pred", "gt", "both"])
def test_overflow_keeps_cap_records_and_counts_the_plane(side):
    pred, gt = M.jittered(90, 80, seed=11)
    cap_p, cap_g = (40, 80) if side == "pred" else ((90, 33) if side == "gt" else (40, 33))
    planes_p, planes_g = [pred, pred[:20], pred[:cap_p]], [gt, gt[:cap_g], gt[:10]]       # (a count that equals the cap is no overflow)
    pa, pc = M.pack(planes_p, 3, 1, cap_p)
    ga, gc = M.pack(planes_g, 3, 1, cap_g)
    (gc if side == "gt" else pc)[0, 0] += 1000                                             # far more components than slots
    want = _check(pa, pc, ga, gc)
    assert want["overflowed"][0] == {"pred": 1, "gt": 1, "both": 2}[side] and want["tp"][0] > 0
    assert want["num_pred"][0] == min(90, cap_p) + 20 + cap_p and want["num_gt"][0] == min(80, cap_g) + min(80, cap_g) + 10


# ------------------------------------------------------------------------------------------------ 8. many planes
@pytest.mark.parametrize("shape", [(33, 3), (70, 5), (300, 1)])
def test_many_planes(shape):
    """(The implementation has no per-launch plane cap - a plane is a workgroup of a one-dimensional grid - so no case goes past one;
    (300, 1) takes the offsets step past one stride of its 256 lanes over the samples.)"""
    B, NC = shape
    rng = np.random.default_rng(B)
    planes_p, planes_g = [], []
    for i in range(B * NC):
        pred, gt = M.jittered(int(rng.integers(0, 10)), int(rng.integers(0, 10)), seed=2000 + i)
        planes_p.append(pred)
        planes_g.append(gt)
    pa, pc = M.pack(planes_p, B, NC, 9)
    ga, gc = M.pack(planes_g, B, NC, 12)
    want = _check(pa, pc, ga, gc)
    assert want["tp"].min() > 0 and want["fp"].min() > 0 and want["fn"].min() > 0


# ------------------------------------------------------------------------------------------------ 9. an epoch, 10. capacity (through Python)
def _detections(arr, cnt, min_area=1):
    from dmmfods_amd.detect import Detections
    return Detections(torch.from_numpy(np.ascontiguousarray(arr)).to(DEV), torch.from_numpy(cnt).to(DEV), None, min_area)


def _same(got, want, keys=None):
    for k in (keys or want):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype)
        if w.dtype.kind == "f":   # bit for bit, NaN equal to NaN
            g, w = np.atleast_1d(g), np.atleast_1d(w)
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(g)].view(np.int64), w[~np.isnan(w)].view(np.int64)), (k, g, w)
        else:
            assert np.array_equal(g, w), (k, g, w)


def _epoch_batches(sizes, NC, seed, cap=16):
    out = []
    for i, B in enumerate(sizes):
        pl = [M.jittered(int(np.random.default_rng(seed + 100 * i + j).integers(0, 14)), 8 + j % 5, seed=seed + 100 * i + j) for j in range(B * NC)]
        pl = [(p, g[:0]) if j % NC == 1 else ((p[:0], g) if j % NC == 2 else (p, g)) for j, (p, g) in enumerate(pl)]
        out.append(M.pack([p for p, _ in pl], B, NC, cap) + M.pack([g for _, g in pl], B, NC, cap))
    return out


def test_an_epoch_of_three_updates_and_reset():
    from dmmfods_amd.detect import DeviceObjectMetrics, ObjectMetrics
    NC = 4   # class 1 has no ground truth (AP NaN), class 2 no predictions (AP 0.0)
    batches = _epoch_batches((1, 3, 2), NC, seed=50)
    dom, om = DeviceObjectMetrics(NC, iou=0.4, capacity=500), ObjectMetrics(NC, iou=0.4)
    assert dom.compute()["tp"].tolist() == [0] * NC                      # before any update: zeros, as ObjectMetrics
    want_entries = [[] for _ in range(NC)]
    for pa, pc, ga, gc in batches:
        assert dom.update(_detections(pa, pc), _detections(ga, gc)) is None
        om.update(M.to_host(pa, pc, 1), M.to_host(ga, gc, 1))
        for n, e in enumerate(M.reference(pa, pc, ga, gc, 1, 0.4)["entries"]):
            want_entries[n].append(e)
    got, want = dom.compute(), om.compute()
    assert set(got) == set(want) | {"dropped_predictions"} and got["dropped_predictions"].tolist() == [0] * NC
    _same(got, want)
    assert isinstance(got["overflowed_planes"], int)
    assert np.isnan(got["ap"][1]) and got["ap"][2] == 0.0 and 0 < got["ap"][0] <= 1 and got["tp"][0] > 0 and got["fp"][0] > 0 and got["fn"][0] > 0
    st = dom.state()
    first = np.concatenate([[0], np.cumsum(st["filled"])])
    for n in range(NC):                                                   # arrival order: update, sample, ascending root
        assert np.array_equal(st["entries"][first[n]:first[n + 1]], np.concatenate(want_entries[n]))
    assert len(dom._workspace) == 3                                      # cached per shape
    dom.reset()
    fresh, om2 = DeviceObjectMetrics(NC, iou=0.4, capacity=500), ObjectMetrics(NC, iou=0.4)
    pa, pc, ga, gc = batches[1]
    dom.update(_detections(pa, pc), _detections(ga, gc))
    fresh.update(_detections(pa, pc), _detections(ga, gc))
    om2.update(M.to_host(pa, pc, 1), M.to_host(ga, gc, 1))
    _same(dom.compute(), fresh.compute())
    _same(dom.compute(), om2.compute())
    with pytest.raises(TypeError):
        dom.update(M.to_host(pa, pc, 1), M.to_host(ga, gc, 1))
    with pytest.raises(ValueError, match="min_area"):
        dom.update(_detections(pa, pc, 1), _detections(ga, gc, 2))
    with pytest.raises(ValueError, match="same samples"):
        dom.update(_detections(pa, pc), _detections(ga[:1], gc[:1]))
    with pytest.raises(ValueError, match="4096"):
        dom.update(_detections(np.zeros((1, NC, 4097, 8), dtype=np.int32), np.zeros((1, NC), dtype=np.int32)), _detections(ga[:1], gc[:1]))


def test_capacity_drops_entries_but_no_count():
    from dmmfods_amd.detect import DeviceObjectMetrics, ObjectMetrics, merge_states
    NC = 2
    pl = [M.jittered(P_, 6, seed=70 + i) for i, P_ in enumerate((7, 4, 9, 3, 9, 2))]      # class 0: 7 + 9 + 9 = 25 predictions, class 1: 9
    pa, pc = M.pack([p for p, _ in pl], 3, NC, 9)
    ga, gc = M.pack([g for _, g in pl], 3, NC, 6)
    want = M.reference(pa, pc, ga, gc, 1, 0.5)
    # directly: the first 10 of class 0 in arrival order, nothing behind them; class 1 whole
    matched, delta, rows = _call(pa, pc, ga, gc, capacity=10, totals0=np.zeros((NC, 8), dtype=np.int64))
    assert np.array_equal(matched, want["matched"]) and delta[:, 6].tolist() == [25, 9]
    assert np.array_equal(rows[0], want["entries"][0][:10]) and np.array_equal(rows[1], want["entries"][1])
    assert np.array_equal(delta[:, 0], want["tp"]) and np.array_equal(delta[:, 1], want["fp"]) and np.array_equal(delta[:, 2], want["fn"])
    # a cursor that starts behind the capacity writes nothing
    t0 = np.zeros((NC, 8), dtype=np.int64)
    t0[:, 6] = (12, 8)
    _, delta, rows = _call(pa, pc, ga, gc, capacity=10, totals0=t0)
    assert len(rows[0]) == 0 and np.array_equal(rows[1], want["entries"][1][:2]) and delta[:, 6].tolist() == [25, 9]
    # through Python
    dom, om = DeviceObjectMetrics(NC, capacity=10), ObjectMetrics(NC)
    dom.update(_detections(pa, pc), _detections(ga, gc))
    om.update(M.to_host(pa, pc, 1), M.to_host(ga, gc, 1))
    got, ref = dom.compute(), om.compute()
    assert got["dropped_predictions"].tolist() == [15, 0] and np.isnan(got["ap"][0]) and not np.isnan(ref["ap"][0])
    _same(got, ref, keys=[k for k in ref if k != "ap"])
    assert got["ap"][1] == ref["ap"][1]
    assert np.array_equal(dom.state()["entries"][:10], want["entries"][0][:10]) and dom.state()["filled"].tolist() == [10, 9]
    _same(merge_states([dom.state()]), got)


# ------------------------------------------------------------------------------------------------ 11. repeatability
def test_three_runs_are_bit_equal():
    runs = [_call(*_jittered(257, 255)) for _ in range(3)]
    for m, d, rows in runs[1:]:
        assert np.array_equal(m, runs[0][0]) and np.array_equal(d, runs[0][1]) and np.array_equal(rows[0], runs[0][2][0])
    m, d, rows = _call(*_jittered(257, 255), with_matched=False)          # a null `matched` changes nothing else
    assert np.array_equal(d, runs[0][1]) and np.array_equal(rows[0], runs[0][2][0])


# ------------------------------------------------------------------------------------------------ 12. end to end
def test_detector_to_device_metrics_end_to_end():
    from dmmfods_amd.detect import DeviceObjectMetrics, HeatMapDetector, ObjectMetrics, match_objects
    rng = np.random.default_rng(22)
    det_p, det_g = HeatMapDetector(0.0, max_per_plane=64), HeatMapDetector(0.7, max_per_plane=64)
    om, dom = ObjectMetrics(3, iou=0.5), DeviceObjectMetrics(3, iou=0.5, capacity=4096)
    for i, B in enumerate((1, 3, 2)):
        gt, _ = P.rectangles(48, 64, seed=30 + i, per_class=3)
        gt = np.concatenate([gt] + [P.rectangles(48, 64, seed=40 + 10 * i + k, per_class=3)[0] for k in range(1, B)])
        pred = np.roll(gt, 1, axis=3) * rng.uniform(1, 4, gt.shape).astype(np.float32) - np.float32(0.5)
        pred[:, :, :, :20] = -1.0
        pred[:, 2] = -1.0
        pred[:, 0, 2:4, 60:63] = 1.5
        dp, dg = det_p(torch.from_numpy(pred).to(DEV)), det_g(torch.from_numpy(gt).to(DEV))
        matched = dom.update(dp, dg, return_matched=True)
        assert matched.shape == (B, 3, 64) and matched.dtype == torch.uint8 and matched.is_cuda
        hp, hg = dp.to_host(), dg.to_host()
        om.update(hp, hg)
        flags = match_objects(hp, hg, 0.5)["matched"]
        want = np.zeros((B, 3, 64), dtype=np.uint8)
        for b in range(B):
            for n in range(3):
                want[b, n, :len(flags[b][n])] = flags[b][n]               # (min_area 1: every kept record takes part, slot = index)
        assert np.array_equal(matched.cpu().numpy(), want)
    got, want = dom.compute(), om.compute()
    _same(got, want)
    assert got["tp"].sum() > 0 and got["fp"].sum() > 0 and got["fn"].sum() > 0


# ------------------------------------------------------------------------------------------------ 13. the agent
class _Loader:
    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = batches, len(batches)


class _Watching:
    """Stands in front of the loaded library: counts the calls of dmm_match_objects, or refuses them."""

    def __init__(self, real, forbid=False):
        self._real, self.calls, self.forbid = real, collections.Counter(), forbid

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name != "dmm_match_objects":
            return f
        if self.forbid:
            raise AssertionError("dmm_match_objects was called without match = 'device'")

        def counted(*a):
            self.calls[name] += 1
            return f(*a)
        return counted


def _tiny_agent(tmp_path, monkeypatch, batches, objects):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from oracle import restatement as O
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    cfg.agent.max_epoch = 1
    cfg.optimizer.learning_rate, cfg.optimizer.weight_decay = 0.0, 0.0   # (the step moves nothing)
    if objects is not None:
        cfg.agent.object_metrics = objects

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    agent = mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=True, compute_dtype="fp32", data_loader=_Loader(batches))
    arch = O.Arch(**TINY, concat_before_block_num=3, stream_2_in_channels=3)
    agent.model.load_state_dict(O.make_state(arch, seed=99))
    return agent


def test_agent_matches_on_the_device_when_asked_and_only_then(tmp_path, monkeypatch):
    from oracle import restatement as O
    from dmmfods_amd import _lib, detect
    arch = O.Arch(**TINY, concat_before_block_num=3, stream_2_in_channels=3)
    batches = [O.make_inputs(arch, 2, 64, 96, seed=s) for s in range(2)]
    watch = _Watching(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", watch)
    spec = dict(threshold=0.0, iou=0.3, max_per_plane=64, min_area=2, connectivity=4)
    host = _tiny_agent(tmp_path / "h", monkeypatch, batches, dict(spec, match="host"))
    assert type(host.object_metrics) is detect.ObjectMetrics
    host.train()
    assert watch.calls["dmm_match_objects"] == 0
    want = host.val_history[-1]["objects"]
    host.model.close()

    def no_pull(self):
        raise AssertionError("Detections.to_host() ran with match = 'device'")
    with monkeypatch.context() as mp:
        mp.setattr(detect.Detections, "to_host", no_pull)
        dev = _tiny_agent(tmp_path / "d", mp, batches, dict(spec, match="device", capacity=1 << 12))
        assert type(dev.object_metrics) is detect.DeviceObjectMetrics and dev.object_metrics.capacity == 1 << 12
        dev.train()
        assert watch.calls["dmm_match_objects"] == len(batches) and len(dev.val_history) == 1
        got = dev.val_history[-1]["objects"]
        dev.model.close()
    assert set(got) == set(want) | {"dropped_predictions"}
    _same(got, want)
    assert int(got["num_pred"].sum()) > 0 and int(got["num_gt"].sum()) > 0
    assert torch.equal(dev.val_history[-1]["iou"], host.val_history[-1]["iou"]) and dev.best_val_iou == host.best_val_iou
    # without the key: the host objects, and the new entry point is never reached
    watch.forbid = True
    plain = _tiny_agent(tmp_path / "p", monkeypatch, batches, spec)
    assert type(plain.object_metrics) is detect.ObjectMetrics
    plain.train()
    _same(plain.val_history[-1]["objects"], want)
    assert set(plain.val_history[-1]["objects"]) == set(want) and torch.equal(plain.val_history[-1]["iou"], host.val_history[-1]["iou"])
    plain.model.close()
