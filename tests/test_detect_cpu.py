"""Heat maps to objects (dmm_heat_components, dmmfods_amd/detect.py, config.agent.object_metrics) as far as it goes without a GPU:
the entry points and every refusal before HIP is touched, the reference labeller (tools/components_ref.py, the oracle of the GPU
tests) against scipy on every pattern of the GPU list, the cap and peak rules against direct numpy statements, match_objects and
ObjectMetrics against a brute-force restatement, the agent's config field, and the sanitizer harness (DRIVE_COMPONENTS=1 drives the
entry point's argument checks, launch geometry and workspace carve-up under ASan + UBSan; without the switch a pinned enqueue trace
keeps its hash)."""
import hashlib
import itertools
import json
import os
import subprocess
import types

import numpy as np
import pytest

from tools import components_patterns as P
from tools import components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ C entry points
def test_symbols_are_declared_exported_and_bound(lib):
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "dmmfods_hip.h")).read()
    L = lib.lib()
    for sym in ("dmm_heat_components", "dmm_heat_components_workspace"):
        assert sym + "(" in header and sym in lib.EXPORTS and hasattr(L, sym), sym
    assert f"#define DMM_CC_TILE_H {lib.CC_TILE_H}" in header and f"#define DMM_CC_TILE_W {lib.CC_TILE_W}" in header
    assert f"#define DMM_CC_MAX_PER_PLANE {lib.CC_MAX_PER_PLANE}" in header and "typedef struct dmm_component" in header
    assert C.sizeof(lib.Component) == 32 == R.RECORD_DTYPE.itemsize
    assert [n for n, _ in lib.Component._fields_] == list(R.RECORD_DTYPE.names)
    for n, _ in lib.Component._fields_:
        assert getattr(lib.Component, n).offset == R.RECORD_DTYPE.fields[n][1], n


def test_workspace(lib):
    WS = lib.lib().dmm_heat_components_workspace
    seg = 4096   # CC_SEG: the label array, then one int per segment of a plane, each part rounded up to 16 bytes
    for (B, NC, H, W, cap) in ((1, 1, 1, 1, 1), (2, 3, 101, 67, 1024), (4, 3, 1280, 1920, 1024), (65535, 1, 3, 5, 65536), (1, 1, 46340, 46340, 7)):
        planes, plane = B * NC, H * W
        want = (planes * plane * 4 + 15) // 16 * 16 + (planes * ((plane + seg - 1) // seg) * 4 + 15) // 16 * 16
        assert WS(B, NC, H, W, cap) == want, (B, NC, H, W, cap)
    for bad in ((0, 3, 8, 8, 4), (2, 0, 8, 8, 4), (-1, 3, 8, 8, 4), (2, 3, 0, 8, 4), (2, 3, 8, -8, 4), (256, 256, 8, 8, 4), (65536, 1, 8, 8, 4),
                (1, 1, 65536, 32768, 4), (1, 1, 46341, 46341, 4), (1, 1, 8, 8, 0), (1, 1, 8, 8, -1), (1, 1, 8, 8, 65537)):
        assert WS(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    """Every refusal is made through addresses nothing dereferences: a call that got past the checks would fault here, where there is
    no device."""
    L = lib.lib()
    x, ws, lab, rec, cnt = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    need = L.dmm_heat_components_workspace(1, 1, 8, 8, 4)
    ok = dict(maps=x, B=1, NC=1, H=8, W=8, thr=0.5, conn=8, cap=4, ws=ws, wsb=need, labels=lab, records=rec, counts=cnt)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dmm_heat_components(a["maps"], a["B"], a["NC"], a["H"], a["W"], a["thr"], a["conn"], a["cap"], a["ws"], a["wsb"], a["labels"],
                                     a["records"], a["counts"], None)

    cases = [(dict(maps=None), b"null"), (dict(ws=None), b"null"), (dict(records=None), b"null"), (dict(counts=None), b"null"),
             (dict(maps=x + 2), b"4-byte aligned"), (dict(labels=lab + 1), b"4-byte aligned"), (dict(counts=cnt + 2), b"4-byte aligned"),
             (dict(records=rec + 4), b"records must be 8-byte aligned"), (dict(ws=ws + 8), b"workspace must be 16-byte aligned"),
             (dict(B=0), b">= 1"), (dict(NC=0), b">= 1"), (dict(H=0), b">= 1"), (dict(W=-3), b">= 1"),
             (dict(B=256, NC=256), b"B * NC must be <= 65535"), (dict(B=65536), b"B * NC must be <= 65535"),
             (dict(H=65536, W=32768), b"H * W must be < 2^31"), (dict(H=2 ** 31 - 1, W=2 ** 31 - 1), b"H * W must be < 2^31"),
             (dict(conn=0), b"connectivity must be 4 or 8"), (dict(conn=6), b"connectivity must be 4 or 8"), (dict(conn=-8), b"connectivity must be 4 or 8"),
             (dict(cap=0), b"max_per_plane must be in [1, 65536]"), (dict(cap=-1), b"max_per_plane must be in [1, 65536]"),
             (dict(cap=65537), b"max_per_plane must be in [1, 65536]"),
             (dict(thr=float("nan")), b"threshold is NaN"),
             (dict(wsb=need - 1), b"workspace_bytes"), (dict(wsb=0), b"workspace_bytes")]
    for kw, text in cases:
        rc = call(**kw)
        msg = L.dmm_last_error()
        assert rc == lib.ERR_INVALID and msg.startswith(b"dmm_heat_components: ") and text in msg, (kw, rc, msg)
    with pytest.raises(ValueError):
        lib.check(call(cap=0))


# ------------------------------------------------------------------------------------------------ the reference labeller
def _patterns(lib):
    return P.patterns(lib.CC_TILE_H, lib.CC_TILE_W)


def test_the_pattern_list_covers_what_the_gpu_tests_name(lib):
    names = {p["name"] for p in _patterns(lib)}
    assert {"spiral", "spiral_cut", "comb", "comb_upside_down", "corners", "staircase", "checkerboard", "all_foreground", "no_foreground",
            "one_pixel", "one_row", "one_column", "smaller_than_a_tile", "width_not_a_multiple_of_four", "width_a_multiple_of_four",
            "isolation", "values", "rectangles"} <= names
    assert {f"noise{p}_seed{s}" for p in (50, 60) for s in range(3)} <= names
    TH, TW = lib.CC_TILE_H, lib.CC_TILE_W
    shape = {p["name"]: p["maps"].shape for p in _patterns(lib)}
    assert shape["spiral"] == (1, 1, 3 * TH + 5, 2 * TW + 3) and shape["checkerboard"] == (1, 1, 2 * TH + 1, 2 * TW + 1)
    assert shape["noise60_seed0"] == (1, 1, 3 * TH + 1, 3 * TW + 2) and shape["isolation"][:2] == (2, 3)
    for p in _patterns(lib):
        if p["name"].startswith("noise"):
            with np.errstate(invalid="ignore"):
                frac = float((p["maps"] >= np.float32(p["threshold"])).mean())
            assert abs(frac - int(p["name"][5:7]) / 100) < 0.02, (p["name"], frac)


@pytest.mark.parametrize("conn", [8, 4])
def test_reference_labeller_against_scipy(lib, conn):
    """Up to relabelling on the labels (a bijection between the two label sets over the same foreground), then exactly on boxes and
    areas, on every pattern of the GPU list."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3)) if conn == 8 else ndimage.generate_binary_structure(2, 1)
    for p in _patterns(lib):
        maps = p["maps"]
        labels, records, counts = R.heat_components(maps, p["threshold"], conn, 4096)
        for b in range(maps.shape[0]):
            for n in range(maps.shape[1]):
                with np.errstate(invalid="ignore"):
                    fg = maps[b, n] >= np.float32(p["threshold"])
                theirs, k = ndimage.label(fg, structure=structure)
                ours = labels[b, n]
                what = (p["name"], conn, b, n)
                assert int(counts[b, n]) == k and np.array_equal(ours >= 0, fg), what
                pairs = np.unique(np.stack([ours[fg], theirs[fg]]), axis=1)
                assert pairs.shape[1] == k and np.unique(pairs[0]).size == k and np.unique(pairs[1]).size == k, what
                rec = records[b, n, :k]
                assert (np.diff(rec["root"]) > 0).all() and not records[b, n, k:].view(np.int32).any(), what
                W = maps.shape[3]
                for r in rec:   # the root is the component's first pixel in raster order, and scipy's box / area for that component
                    j = theirs[r["root"] // W, r["root"] % W]
                    ys, xs = np.nonzero(theirs == j)
                    assert r["root"] == (ys * W + xs).min(), what
                    sl = ndimage.find_objects(theirs)[j - 1]
                    assert (r["x0"], r["y0"], r["x1"], r["y1"]) == (sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1), what
                    assert r["area"] == ys.size, what
        k = p.get(f"count{conn}")
        if k is not None:
            assert int(counts[0, 0]) == k, (p["name"], conn)


def test_reference_cap_rule(lib):
    """More components than max_per_plane: counts is the true number, the kept records are the smallest roots in order - the first
    `cap` records of an uncapped run - and the rest is zero."""
    p = {q["name"]: q for q in _patterns(lib)}["checkerboard"]
    H, W = p["maps"].shape[2:]
    true = (H * W + 1) // 2
    _, full, cnt_full = R.heat_components(p["maps"], p["threshold"], 4, true)
    assert int(cnt_full[0, 0]) == true and full[0, 0]["root"].tolist() == list(range(0, H * W, 2))
    for cap in (1, 37, true - 1, true, true + 5):
        _, rec, cnt = R.heat_components(p["maps"], p["threshold"], 4, cap)
        kept = min(cap, true)
        assert int(cnt[0, 0]) == true
        assert np.array_equal(rec[0, 0, :kept], full[0, 0, :kept]) and not rec[0, 0, kept:].view(np.int32).any()


def test_reference_peak_and_score_rules():
    """score is the largest value with -0.0 below +0.0, peak the first pixel in raster order that holds exactly that value."""
    m = np.full((1, 1, 6, 9), -1.0, dtype=np.float32)
    m[0, 0, 1, 1:5] = (0.5, 3.0, 1.0, 3.0)
    m[0, 0, 2, 1:5] = (3.0, 0.0, 0.0, 0.0)
    m[0, 0, 4, 1:4] = (-0.0, 0.0, -0.0)
    m[0, 0, 4, 6:8] = (-0.0, -0.0)
    labels, rec, cnt = R.heat_components(m, 0.0, 8, 8)
    assert int(cnt[0, 0]) == 3
    a, b, c = rec[0, 0, :3]
    vals = m[0, 0].ravel()
    members = np.nonzero(labels[0, 0].ravel() == a["root"])[0]
    assert a["score"] == vals[members].max() == 3.0 and a["peak"] == members[vals[members] == 3.0][0] == 1 * 9 + 2 and a["area"] == 8
    assert b["score"] == 0.0 and not np.signbit(b["score"]) and b["peak"] == 4 * 9 + 2
    assert c["score"] == 0.0 and np.signbit(c["score"]) and c["peak"] == 4 * 9 + 6
    keys = R.ordered_bits(np.asarray([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], dtype=np.float32))
    assert (np.diff(keys.astype(np.int64)) > 0).all()


# ------------------------------------------------------------------------------------------------ matching and metrics
def _plane(boxes, scores=None, roots=None):
    from dmmfods_amd.detect import PlaneObjects
    n = len(boxes)
    rec = np.zeros(n, dtype=R.RECORD_DTYPE)
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        rec[i] = (roots[i] if roots else y0 * 1000 + x0, x0, y0, x1, y1, (x1 - x0 + 1) * (y1 - y0 + 1), scores[i] if scores else 1.0, y0 * 1000 + x0)
    order = np.argsort(rec["root"], kind="stable")
    return PlaneObjects(rec[order], n, False)


def _brute_iou(a, b):
    """Pixel sets of the two inclusive boxes."""
    pa = {(x, y) for x in range(a[0], a[2] + 1) for y in range(a[1], a[3] + 1)}
    pb = {(x, y) for x in range(b[0], b[2] + 1) for y in range(b[1], b[3] + 1)}
    return len(pa & pb) / len(pa | pb)


def _brute_match(pred, gt, iou):
    """The rule restated: predictions by (-score, root); each takes the free ground-truth box with the largest (IoU, -root) among
    those with IoU >= iou."""
    free = set(range(len(gt)))
    flags = [False] * len(pred)
    for i in sorted(range(len(pred)), key=lambda i: (-float(pred.scores[i]), int(pred.roots[i]))):
        cand = [(_brute_iou(pred.boxes[i], gt.boxes[j]), -int(gt.roots[j]), j) for j in free]
        cand = [c for c in cand if c[0] >= iou]
        if cand:
            free.discard(max(cand)[2])
            flags[i] = True
    return flags


def _brute_ap(scores, flags, num_gt):
    """Area under the precision envelope, by summing over recall steps."""
    if num_gt == 0:
        return float("nan")
    order = sorted(range(len(scores)), key=lambda i: -float(scores[i]))   # stable
    prec, rec, tp = [], [], 0
    for k, i in enumerate(order, 1):
        tp += bool(flags[i])
        prec.append(tp / k)
        rec.append(tp / num_gt)
    ap, last = 0.0, 0.0
    for k in range(len(order)):
        ap += (rec[k] - last) * max(prec[k:])
        last = rec[k]
    return ap


def test_box_iou_is_taken_on_inclusive_pixel_boxes():
    from dmmfods_amd.detect import box_iou
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = rng.integers(0, 12, 4)
        b = rng.integers(0, 12, 4)
        a = (min(a[0], a[2]), min(a[1], a[3]), max(a[0], a[2]), max(a[1], a[3]))
        b = (min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3]))
        assert box_iou(a, b) == _brute_iou(a, b), (a, b)
    assert box_iou((3, 3, 3, 3), (3, 3, 3, 3)) == 1.0 and box_iou((0, 0, 1, 1), (2, 0, 3, 1)) == 0.0


def test_match_objects_against_a_brute_force_restatement():
    from dmmfods_amd.detect import match_objects
    # class 0: two predictions on one ground-truth box - the better-scored one takes it, the second is a false positive; one miss
    gt0 = _plane([(0, 0, 9, 9), (40, 40, 49, 49)])
    pr0 = _plane([(0, 0, 9, 8), (0, 1, 9, 9)], scores=[0.6, 0.9])
    # class 1: no ground truth; class 2: no predictions
    gt1, pr1 = _plane([]), _plane([(5, 5, 8, 8)])
    gt2, pr2 = _plane([(1, 1, 4, 4)]), _plane([])
    # class 3: equal scores - the smaller root goes first and takes the box both overlap best; IoU exactly on the bound:
    # (0,0)-(9,9) against (0,0)-(9,4) is 50 / 100 = 0.5, which counts
    gt3 = _plane([(20, 20, 29, 29), (0, 0, 9, 9)])
    pr3 = _plane([(20, 20, 29, 28), (20, 21, 29, 29), (0, 0, 9, 4)], scores=[0.5, 0.5, 0.5])
    pred, gt = [[pr0, pr1, pr2, pr3]], [[gt0, gt1, gt2, gt3]]
    m = match_objects(pred, gt, iou=0.5)
    assert m["matched"][0][0].tolist() == [False, True]          # (sorted by root: the 0.6 box has root 0, the 0.9 box root 1000)
    assert m["matched"][0][1].tolist() == [False] and m["matched"][0][2].tolist() == []
    assert m["matched"][0][3].tolist() == [True, True, False]     # roots 0 (on the bound), 20020 (first of the equal pair), 21020
    assert m["tp"].tolist() == [1, 0, 0, 2] and m["fp"].tolist() == [1, 1, 0, 1] and m["fn"].tolist() == [1, 0, 1, 0]
    assert m["tp"].dtype == np.int64
    assert not match_objects(pred, gt, iou=0.5 + 1e-12)["matched"][0][3][0]      # just above the bound it no longer counts
    for p, g, f in zip(pred[0], gt[0], m["matched"][0]):
        assert f.tolist() == _brute_match(p, g, 0.5)
    # random planes
    rng = np.random.default_rng(8)

    def boxes(k):
        out = []
        for _ in range(k):
            x0, y0 = rng.integers(0, 30, 2)
            out.append((int(x0), int(y0), int(x0 + rng.integers(0, 12)), int(y0 + rng.integers(0, 12))))
        return out
    for trial in range(40):
        gb = boxes(int(rng.integers(0, 7)))
        g = _plane(gb, roots=list(range(len(gb))))
        pb = boxes(int(rng.integers(0, 9)))
        p = _plane(pb, scores=[float(rng.integers(0, 4)) / 4 for _ in pb], roots=list(range(len(pb))))
        for iou in (0.1, 0.5):
            got = match_objects([[p]], [[g]], iou)
            want = _brute_match(p, g, iou)
            assert got["matched"][0][0].tolist() == want, (trial, iou)
            assert (int(got["tp"][0]), int(got["fp"][0]), int(got["fn"][0])) == (sum(want), len(p) - sum(want), len(g) - sum(want))
    with pytest.raises(ValueError):
        match_objects([[p]], [[g, g]])


def test_object_metrics_against_a_brute_force_restatement():
    from dmmfods_amd.detect import ObjectMetrics, average_precision
    rng = np.random.default_rng(9)
    nc = 4
    om = ObjectMetrics(nc, iou=0.4)
    tp, fp, fn = [0] * nc, [0] * nc, [0] * nc
    scores, flags, ngt = [[] for _ in range(nc)], [[] for _ in range(nc)], [0] * nc
    for batch, B in enumerate((1, 3, 2)):
        pred, gt = [], []
        for b in range(B):
            prow, grow = [], []
            for n in range(nc):
                gb = [] if n == 1 else [(12 * i, 3 * i, 12 * i + 8, 3 * i + 6) for i in range(int(rng.integers(1, 4)))]
                pb = [] if n == 2 else [(x0 + int(rng.integers(-2, 3)), y0, x1, y1 + int(rng.integers(0, 3))) for (x0, y0, x1, y1) in gb] + [(50, 50, 53, 53)]
                pb = [(max(0, x0), y0, x1, y1) for (x0, y0, x1, y1) in pb]
                prow.append(_plane(pb, scores=[float(rng.integers(1, 4)) / 4 for _ in pb], roots=list(range(len(pb)))))
                grow.append(_plane(gb, roots=list(range(len(gb)))))
            pred.append(prow)
            gt.append(grow)
        om.update(pred, gt)
        for prow, grow in zip(pred, gt):
            for n in range(nc):
                f = _brute_match(prow[n], grow[n], 0.4)
                tp[n] += sum(f); fp[n] += len(f) - sum(f); fn[n] += len(grow[n]) - sum(f); ngt[n] += len(grow[n])
                scores[n] += prow[n].scores.tolist(); flags[n] += f
    got = om.compute()
    assert got["tp"].tolist() == tp and got["fp"].tolist() == fp and got["fn"].tolist() == fn
    assert got["num_gt"].tolist() == ngt and got["num_pred"].tolist() == [len(s) for s in scores] and got["overflowed_planes"] == 0
    for n in range(nc):
        for k, want in (("precision", (tp[n], tp[n] + fp[n])), ("recall", (tp[n], tp[n] + fn[n])), ("f1", (2 * tp[n], 2 * tp[n] + fp[n] + fn[n]))):
            if want[1] == 0:
                assert np.isnan(got[k][n]), (k, n)
            else:
                assert got[k][n] == want[0] / want[1], (k, n)
        want = _brute_ap(scores[n], flags[n], ngt[n])
        assert (np.isnan(want) and np.isnan(got["ap"][n])) or abs(got["ap"][n] - want) < 1e-12, (n, got["ap"][n], want)
    assert np.isnan(got["recall"][1]) and np.isnan(got["ap"][1]) and got["precision"][1] == 0.0      # no ground truth, only false positives
    assert np.isnan(got["precision"][2]) and got["recall"][2] == 0.0 and got["ap"][2] == 0.0          # no predictions
    assert 0 < got["ap"][0] <= 1
    assert average_precision([0.9, 0.8, 0.7], [True, False, True], 2) == 0.5 * 1.0 + 0.5 * (2 / 3)
    om.reset()
    assert om.compute()["tp"].tolist() == [0] * nc
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            ObjectMetrics(3, iou=bad)


def test_detector_validates_its_arguments(lib):
    import torch
    from dmmfods_amd.detect import HeatMapDetector
    d = HeatMapDetector(0.7)
    assert (d.threshold, d.connectivity, d.max_per_plane, d.min_area) == (0.7, 8, 1024, 1)
    for kw in (dict(threshold=float("nan")), dict(threshold=0.5, connectivity=6), dict(threshold=0.5, max_per_plane=0),
               dict(threshold=0.5, max_per_plane=65537), dict(threshold=0.5, max_per_plane=1.5), dict(threshold=0.5, max_per_plane=True),
               dict(threshold=0.5, min_area=0), dict(threshold=0.5, min_area=2.5)):
        with pytest.raises(ValueError):
            HeatMapDetector(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d(torch.zeros(1, 3, 8, 8))


# ------------------------------------------------------------------------------------------------ the agent's config field
def test_agent_reads_the_config_field_only_if_present(lib):
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    assert Agent._optional(cfg.agent, "object_metrics") is None
    me = types.SimpleNamespace(config=cfg)
    assert Agent._make_object_metrics(me, None) == (None, None)
    det, om = Agent._make_object_metrics(me, {})
    assert det.threshold == float(cfg.agent.iou_threshold) and (det.connectivity, det.max_per_plane, det.min_area) == (8, 1024, 1)
    assert om.iou == 0.5 and om.num_classes == cfg.model.num_classes
    det, om = Agent._make_object_metrics(me, dict(iou=0.3, connectivity=4, max_per_plane=16, min_area=5, threshold=-1.5))
    assert (det.threshold, det.connectivity, det.max_per_plane, det.min_area, om.iou) == (-1.5, 4, 16, 5, 0.3)
    for bad in (True, 5, [0.5], dict(iuo=0.5), dict(iou=0.0), dict(iou=2.0), dict(connectivity=6), dict(max_per_plane=0), dict(min_area=0),
                dict(threshold=float("nan")), dict(threshold="high")):
        with pytest.raises(ValueError, match="agent.object_metrics"):
            Agent._make_object_metrics(me, bad)


# ------------------------------------------------------------------------------------------------ the sanitizer harness
@pytest.fixture(scope="module")
def drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


def _run(drive, envx, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(envx, DRIVE_TRACE_ENQUEUE="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([drive] + args.split(), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DRIVE OK" in r.stdout, (envx, (r.stdout[-1000:] + r.stderr)[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_harness_drives_the_entry_point_and_leaves_the_pinned_trace_alone(drive, lib):
    """DRIVE_COMPONENTS=1: behind the plan's life the stand-alone driver calls dmm_heat_components on three shapes (a plane smaller than
    a tile, ragged in both directions, many planes; every operand an address only), with and without a labels array, and tries every
    refusal, under ASan + UBSan.  Without the switch the row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = [ln for ln in _run(drive, {}, args) if ln.startswith("T ")]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["(none) | " + args]
    out = _run(drive, {"DRIVE_COMPONENTS": "1"}, args)
    assert "COMPONENTS OK" in out and len([ln for ln in out if ln.startswith("COMPONENTS ") and ln.endswith(" ok")]) == 3, out[-12:]
    trace = [ln for ln in out if ln.startswith("T ")]
    assert trace[:len(base)] == base                               # the plan's schedule is untouched ...
    extra = trace[len(base):]                                      # ... and behind it: seven launches per call, nothing else
    assert all(ln.startswith("T launch") for ln in extra) and len(extra) == 3 * 2 * 7
    kernels = ["cc_local_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_scan_kernel", "cc_slots_kernel", "cc_stats_kernel", "cc_finish_kernel"]
    TH, TW, seg = lib.CC_TILE_H, lib.CC_TILE_W, 4096
    shapes = [(1, 1, 7, 9, 16), (2, 3, 3 * TH + 5, 2 * TW + 3, 1024), (64, 300, 40, 50, 300)]
    want = []
    for (B, NC, H, W, cap) in shapes:
        tiles, nseg = -(-H // TH) * -(-W // TW), -(-(H * W) // seg)
        want += [(k, g, B * NC) for k, g in zip(kernels, (tiles, tiles, nseg, 1, nseg, tiles, -(-cap // 256)))] * 2
    got = [(ln.split()[2], int(ln.split()[3]), int(ln.split()[4])) for ln in extra]
    assert all(w[0] in g[0] and w[1:] == g[1:] for w, g in zip(want, got)), list(itertools.islice(zip(want, got), 14))
