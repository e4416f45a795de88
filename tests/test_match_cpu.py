"""Object matching on the device (dmm_match_objects, DeviceObjectMetrics, config.agent.object_metrics.match) as
far as it goes without a GPU: the entry points and every refusal before HIP is touched, DeviceObjectMetrics' argument checks,
merge_states against ObjectMetrics fed the same planes in the same order, the generator of the GPU tests' inputs (its fixed seeds
must give true positives, false positives and false negatives at every size), the agent's config field, and the sanitizer harness
(DRIVE_MATCH=1 drives the entry point's argument checks, launch geometry and workspace carve-up under ASan + UBSan; without the
switch a pinned enqueue trace keeps its hash)."""
import hashlib
import json
import os
import subprocess
import types

import numpy as np
import pytest

from tools import match_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ C entry points
def test_symbols_are_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "dmmfods_hip.h")).read()
    L = lib.lib()
    for sym in ("dmm_match_objects", "dmm_match_objects_workspace"):
        assert sym + "(" in header and sym in lib.EXPORTS and hasattr(L, sym), sym
    assert f"#define DMM_MATCH_MAX_PER_PLANE {lib.MATCH_MAX_PER_PLANE}" in header and lib.MATCH_MAX_PER_PLANE == 4096
    assert lib.MATCH_MAX_PER_PLANE < lib.CC_MAX_PER_PLANE and 1024 <= lib.MATCH_MAX_PER_PLANE   # the detector's default is inside, its maximum is not


def test_workspace(lib):
    WS = lib.lib().dmm_match_objects_workspace
    for (B, NC, cp, cg) in ((1, 1, 1, 1), (4, 3, 1024, 1024), (2, 3, 4096, 7), (65535, 1, 8, 4096), (21845, 3, 1, 1)):
        planes = B * NC   # two int32 and one int64 per plane, each array rounded up to 16 bytes
        assert WS(B, NC, cp, cg) == 2 * ((planes * 4 + 15) // 16 * 16) + (planes * 8 + 15) // 16 * 16, (B, NC, cp, cg)
    for bad in ((0, 3, 8, 8), (2, 0, 8, 8), (-1, 3, 8, 8), (256, 256, 8, 8), (65536, 1, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, -1, 8),
                (1, 1, 4097, 8), (1, 1, 8, 4097), (1, 1, 65536, 65536)):
        assert WS(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    """Every refusal is made through addresses nothing dereferences: a call that got past the checks would fault here, where there is
    no device."""
    L = lib.lib()
    need = L.dmm_match_objects_workspace(2, 3, 8, 8)
    ok = dict(pred=0x10000, pc=0x20000, cp=8, gt=0x30000, gc=0x40000, cg=8, B=2, NC=3, min_area=1, iou=0.5, ws=0x50000, wsb=need,
              matched=0x60000, totals=0x70000, entries=0x80000, capacity=100)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dmm_match_objects(a["pred"], a["pc"], a["cp"], a["gt"], a["gc"], a["cg"], a["B"], a["NC"], a["min_area"], a["iou"], a["ws"], a["wsb"],
                                   a["matched"], a["totals"], a["entries"], a["capacity"], None)

    cases = [(dict(pred=None), b"null"), (dict(pc=None), b"null"), (dict(gt=None), b"null"), (dict(gc=None), b"null"), (dict(ws=None), b"null"),
             (dict(totals=None), b"null"), (dict(entries=None), b"null"),
             (dict(pred=0x10004), b"records must be 8-byte aligned"), (dict(gt=0x30004), b"records must be 8-byte aligned"),
             (dict(pc=0x20002), b"counts must be 4-byte aligned"), (dict(gc=0x40001), b"counts must be 4-byte aligned"),
             (dict(totals=0x70004), b"totals must be 8-byte aligned"), (dict(entries=0x80002), b"entries must be 4-byte aligned"),
             (dict(ws=0x50008), b"workspace must be 16-byte aligned"),
             (dict(B=0), b"B and NC must be >= 1"), (dict(NC=0), b"B and NC must be >= 1"), (dict(B=-2), b"B and NC must be >= 1"),
             (dict(B=256, NC=256), b"B * NC must be <= 65535"), (dict(B=65536, NC=1), b"B * NC must be <= 65535"),
             (dict(cp=0), b"must be in [1, 4096]"), (dict(cg=0), b"must be in [1, 4096]"), (dict(cp=-5), b"must be in [1, 4096]"),
             (dict(cp=4097), b"must be in [1, 4096]"), (dict(cg=4097), b"must be in [1, 4096]"),
             (dict(cp=65536, cg=65536), b"it does not take dmm_heat_components' maximum of 65536"),
             (dict(min_area=0), b"min_area must be >= 1"), (dict(min_area=-1), b"min_area must be >= 1"),
             (dict(iou=0.0), b"iou must be in (0, 1]"), (dict(iou=-0.5), b"iou must be in (0, 1]"), (dict(iou=1.5), b"iou must be in (0, 1]"),
             (dict(iou=float("nan")), b"iou must be in (0, 1]"), (dict(iou=float("inf")), b"iou must be in (0, 1]"),
             (dict(capacity=0), b"capacity must be in [1, 2^31 - 1]"), (dict(capacity=-1), b"capacity must be in [1, 2^31 - 1]"),
             (dict(capacity=2 ** 31), b"capacity must be in [1, 2^31 - 1]"),
             (dict(wsb=need - 1), b"workspace_bytes is below dmm_match_objects_workspace"), (dict(wsb=0), b"workspace_bytes is below")]
    for kw, msg in cases:
        assert call(**kw) == lib.ERR_INVALID, kw
        err = L.dmm_last_error()
        assert err.startswith(b"dmm_match_objects: ") and msg in err, (kw, err)
    # (a null `matched` and iou = 1.0 are fine, but those calls would launch: the GPU tests make them)


# ------------------------------------------------------------------------------------------------ Python
def test_device_object_metrics_validates_its_arguments(lib):
    from dmmfods_amd.detect import DeviceObjectMetrics, ObjectMetrics
    d = DeviceObjectMetrics(3)
    assert (d.num_classes, d.iou, d.capacity) == (3, 0.5, 1 << 20) and d.iou == ObjectMetrics(3).iou
    d = DeviceObjectMetrics(2, iou=1.0, capacity=1)
    assert (d.iou, d.capacity) == (1.0, 1)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="iou"):
            DeviceObjectMetrics(3, iou=bad)
    for bad in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="capacity"):
            DeviceObjectMetrics(3, capacity=bad)
    # nothing is allocated before the first update; compute() and reset() work on the empty state
    d = DeviceObjectMetrics(3)
    d.reset()
    got, want = d.compute(), ObjectMetrics(3).compute()
    assert set(got) == set(want) | {"dropped_predictions"}
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True) and np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, k
    planes = M.to_host(*M.pack([M.records([(0, 0, 3, 3)])] * 3, 1, 3, 2), 1)
    with pytest.raises(TypeError, match="Detections"):
        d.update(planes, planes)


def _state(batches, nc, min_area, iou, capacity):
    """The state a DeviceObjectMetrics of that capacity would hold behind these updates, made by hand from the host reference."""
    totals = np.zeros((nc, 8), dtype=np.int64)
    entries = [np.zeros((0, 2), dtype=np.int32) for _ in range(nc)]
    for pa, pc, ga, gc in batches:
        r = M.reference(pa, pc, ga, gc, min_area, iou)
        for col, k in enumerate(("tp", "fp", "fn", "num_pred", "num_gt", "overflowed")):
            totals[:, col] += r[k]
        totals[:, 6] += r["num_pred"]
        entries = [np.concatenate([e, x]) for e, x in zip(entries, r["entries"])]
    filled = np.minimum(totals[:, 6], capacity)
    return {"totals": totals, "filled": filled, "entries": np.concatenate([e[:k] for e, k in zip(entries, filled)]).astype(np.int32)}


def _batches(sizes, nc, seed):
    out = []
    for i, B in enumerate(sizes):
        pl = [M.jittered(3 + (7 * j + i) % 9, 8 + j % 5, seed=seed + 100 * i + j) for j in range(B * nc)]
        # class 1 never has ground truth (AP NaN), class 2 never a prediction (AP 0.0)
        pl = [(p, g[:0]) if j % nc == 1 else ((p[:0], g) if j % nc == 2 else (p, g)) for j, (p, g) in enumerate(pl)]
        out.append(M.pack([p for p, _ in pl], B, nc, 8) + M.pack([g for _, g in pl], B, nc, 16))   # (cap 8 < 11: some planes overflow)
    return out


def test_merge_states_agrees_with_object_metrics(lib):
    from dmmfods_amd.detect import ObjectMetrics, merge_states
    nc, iou = 4, 0.4
    a, b = _batches((1, 3), nc, seed=5), _batches((2,), nc, seed=900)
    om = ObjectMetrics(nc, iou=iou)
    for pa, pc, ga, gc in a + b:
        om.update(M.to_host(pa, pc, 2), M.to_host(ga, gc, 2))
    want = om.compute()
    got = merge_states([_state(a, nc, 2, iou, 1 << 20), _state(b, nc, 2, iou, 1 << 20)])      # two ranks, gathered in list order
    assert set(got) == set(want) | {"dropped_predictions"} and got["dropped_predictions"].tolist() == [0] * nc
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), (k, g, w)
        if w.dtype.kind == "f":
            assert np.array_equal(g[~np.isnan(g)].view(np.int64), w[~np.isnan(w)].view(np.int64)), k      # bit for bit
    assert isinstance(got["overflowed_planes"], int) and got["overflowed_planes"] > 0
    assert np.isnan(got["ap"][1]) and got["precision"][1] == 0.0 and got["ap"][2] == 0.0 and np.isnan(got["precision"][2])
    assert 0 < got["ap"][0] <= 1 and got["tp"][0] > 0 and got["fp"][0] > 0 and got["fn"][0] > 0
    one = merge_states([_state(a + b, nc, 2, iou, 1 << 20)])                                       # one rank that saw everything
    for k in got:
        assert np.array_equal(np.asarray(one[k]), np.asarray(got[k]), equal_nan=True), k
    # drops: the second state kept 5 entries a class; the counts stay, the AP of the classes that lost predictions is NaN
    small = _state(b, nc, 2, iou, 5)
    assert small["filled"].tolist() == [5, 5, 0, 5] and small["entries"].shape == (15, 2)
    cut = merge_states([_state(a, nc, 2, iou, 1 << 20), small])
    assert cut["dropped_predictions"].tolist() == (small["totals"][:, 6] - small["filled"]).tolist() and cut["dropped_predictions"][0] > 0
    assert np.isnan(cut["ap"][0]) and np.isnan(cut["ap"][3]) and cut["ap"][2] == 0.0
    for k in want:
        if k != "ap":
            assert np.array_equal(np.asarray(cut[k]), np.asarray(want[k]), equal_nan=True), k
    with pytest.raises(ValueError):
        merge_states([])
    with pytest.raises(ValueError, match="malformed"):
        merge_states([_state(a, nc, 2, iou, 100), _state(_batches((1,), 3, seed=1), 3, 2, iou, 100)])


def test_the_gpu_tests_inputs_show_something():
    """tests/test_match_gpu.py asserts per size that the host result has true positives, false positives and false negatives; the
    seeds are fixed, so it is checked here already."""
    for (P, G) in ((63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (600, 600), (4096, 33), (33, 4096)):
        pred, gt = M.jittered(P, G, seed=1000 + P)
        assert len(pred) == P and len(gt) == G and len(np.unique(pred["score"])) < 8
        if P + G > 600:
            pred, gt = pred[:300], gt[:300]       # (the whole planes are matched on the GPU box; here a corner of them is enough)
        r = M.reference(*M.pack([pred], 1, 1, len(pred)), *M.pack([gt], 1, 1, len(gt)), 1, 0.5)
        assert r["tp"][0] > 0 and r["fp"][0] > 0 and r["fn"][0] > 0, (P, G, r["tp"], r["fp"], r["fn"])
    arr, cnt = M.pack([M.records([(0, 0, 1, 1)])], 1, 1, 3)
    assert arr[0, 0, 1].tolist() == [0x7FFFFFFF, 0, 0, 511, 511, 0x7FFFFFFF, 0x7F800000, -1] and cnt.tolist() == [[1]]   # the poison


# ------------------------------------------------------------------------------------------------ the agent's config field
def test_agent_reads_the_match_field(lib):
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    from dmmfods_amd.detect import DeviceObjectMetrics, ObjectMetrics
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    me = types.SimpleNamespace(config=cfg)
    for spec in ({}, dict(match="host"), dict(iou=0.3, match="host")):
        det, om = Agent._make_object_metrics(me, spec)
        assert type(om) is ObjectMetrics and om.iou == spec.get("iou", 0.5) and det.max_per_plane == 1024
    det, om = Agent._make_object_metrics(me, dict(match="device"))
    assert type(om) is DeviceObjectMetrics and (om.iou, om.capacity, om.num_classes) == (0.5, 1 << 20, cfg.model.num_classes)
    det, om = Agent._make_object_metrics(me, dict(match="device", capacity=77, iou=0.3, min_area=5, max_per_plane=4096, threshold=-1.5))
    assert type(om) is DeviceObjectMetrics and (om.iou, om.capacity) == (0.3, 77) and (det.min_area, det.max_per_plane, det.threshold) == (5, 4096, -1.5)
    for bad in (dict(match="gpu"), dict(match=None), dict(match=True), dict(match="host", capacity=100), dict(capacity=100),
                dict(match="device", capacity=0), dict(match="device", capacity=2.5), dict(match="device", iou=0.0),
                dict(match="device", max_per_plane=4097), dict(match="device", max_per_plane=65536)):
        with pytest.raises(ValueError, match="agent.object_metrics"):
            Agent._make_object_metrics(me, bad)
    assert Agent._make_object_metrics(me, dict(max_per_plane=65536))[0].max_per_plane == 65536      # the host path keeps the detector's maximum


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
    """DRIVE_MATCH=1: behind the plan's life the stand-alone driver calls dmm_match_objects on three shapes (one plane, a small batch at
    the detector's default cap, B * NC at the entry point's limit; operands addresses only, the workspace real between guard bands),
    with and without `matched`, and tries every refusal, under ASan + UBSan.  Without the switch the row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = [ln for ln in _run(drive, {}, args) if ln.startswith("T ")]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["(none) | " + args]
    out = _run(drive, {"DRIVE_MATCH": "1"}, args)
    assert "MATCH OK" in out and len([ln for ln in out if ln.startswith("MATCH ") and ln.endswith(" ok")]) == 3, out[-12:]
    trace = [ln for ln in out if ln.startswith("T ")]
    assert trace[:len(base)] == base                               # the plan's schedule is untouched ...
    extra = trace[len(base):]                                      # ... and behind it: three launches per call, nothing else
    assert all(ln.startswith("T launch") for ln in extra) and len(extra) == 3 * 2 * 3
    kernels = ["match_count_kernel", "match_offsets_kernel", "match_plane_kernel"]
    want = []
    for (B, NC) in ((1, 1), (4, 3), (21845, 3)):
        want += [(k, g, 1) for k, g in zip(kernels, (B * NC, NC, B * NC))] * 2
    got = [(ln.split()[2], int(ln.split()[3]), int(ln.split()[4])) for ln in extra]
    assert all(w[0] in g[0] and w[1:] == g[1:] for w, g in zip(want, got)), list(zip(want, got))[:6]
