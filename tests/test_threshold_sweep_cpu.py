"""The validation threshold sweep (dmm_logit_hist, dmmfods_amd/metrics.py, config.agent.threshold_sweep) as far as it goes without a
GPU: every refusal of the entry point before it touches HIP, dmm_logit_hist_elems, curves_from_counts against a direct numpy
evaluation of the comparisons, ThresholdSweep's validation, the agent's config field, and the sanitizer harness (DRIVE_HIST=1 drives
the entry point's argument checks and launch geometry under ASan + UBSan; without the switch a pinned enqueue trace keeps its hash)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import types

import numpy as np
import pytest
import torch

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
    for sym in ("dmm_logit_hist", "dmm_logit_hist_elems"):
        assert sym + "(" in header and sym in lib.EXPORTS and hasattr(L, sym), sym
    assert "#define DMM_HIST_MAX_THRESHOLDS 255" in header and lib.HIST_MAX_THRESHOLDS == 255


def test_elems(lib):
    E = lib.lib().dmm_logit_hist_elems
    assert E(2, 3, 16) == 2 * 3 * 2 * 17 and E(1, 1, 1) == 4 and E(4, 3, 255) == 4 * 3 * 2 * 256
    assert E(65535, 1, 255) == 65535 * 2 * 256 and E(255, 257, 1) == 255 * 257 * 4
    for bad in ((0, 3, 4), (2, 0, 4), (-1, 3, 4), (256, 256, 4), (65536, 1, 4), (2, 3, 0), (2, 3, 256), (2, 3, -1)):
        assert E(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    """Every refusal is made through addresses nothing dereferences (only `thresholds` is host memory the checks read): a call that
    got past the checks would fault here, where there is no device."""
    L = lib.lib()
    x, t, c = 0x10000, 0x20000, 0x30000
    thr = (C.c_float * 4)(-1.0, 0.0, 0.5, 2.0)
    ok = dict(logits=x, target=t, B=1, NC=1, H=8, W=8, thr=thr, nthr=4, gt=0.7, acc=0, counts=c)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dmm_logit_hist(a["logits"], a["target"], a["B"], a["NC"], a["H"], a["W"], a["thr"], a["nthr"], a["gt"], a["acc"], a["counts"], None)

    nan, inf = float("nan"), float("inf")
    big = (C.c_float * 256)(*[float(i) for i in range(256)])
    cases = [(dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(thr=None), b"null"), (dict(counts=None), b"null"),
             (dict(logits=x + 2), b"4-byte aligned"), (dict(target=t + 1), b"4-byte aligned"), (dict(counts=c + 4), b"8-byte aligned"),
             (dict(B=0), b">= 1"), (dict(NC=0), b">= 1"), (dict(H=0), b">= 1"), (dict(W=-3), b">= 1"),
             (dict(B=256, NC=256), b"B * NC must be <= 65535"), (dict(B=65536), b"B * NC must be <= 65535"),
             (dict(H=65536, W=32768), b"H * W must be < 2^31"), (dict(H=2 ** 31 - 1, W=2 ** 31 - 1), b"H * W must be < 2^31"),
             (dict(nthr=0), b"nthr must be in [1, 255]"), (dict(nthr=-1), b"nthr must be in [1, 255]"), (dict(thr=big, nthr=256), b"nthr must be in [1, 255]"),
             (dict(thr=(C.c_float * 3)(0.0, nan, 2.0), nthr=3), b"thresholds[1] is NaN or infinite"),
             (dict(thr=(C.c_float * 3)(0.0, 1.0, inf), nthr=3), b"thresholds[2] is NaN or infinite"),
             (dict(thr=(C.c_float * 3)(-inf, 1.0, 2.0), nthr=3), b"thresholds[0] is NaN or infinite"),
             (dict(thr=(C.c_float * 3)(0.0, 1.0, 1.0), nthr=3), b"strictly ascending"),
             (dict(thr=(C.c_float * 3)(0.0, 1.0, 0.5), nthr=3), b"strictly ascending"),
             (dict(gt=nan), b"gt_threshold is NaN")]
    for kw, text in cases:
        rc = call(**kw)
        assert rc == lib.ERR_INVALID and L.dmm_last_error().startswith(b"dmm_logit_hist: ") and text in L.dmm_last_error(), (kw, rc, L.dmm_last_error())
    with pytest.raises(ValueError):
        lib.check(call(nthr=0))


# ------------------------------------------------------------------------------------------------ curves_from_counts
def _direct(x, t, thr, gt):
    """Every count straight from the comparisons, per class and threshold (numpy, float32 operands)."""
    nc = x.shape[0]
    out = {k: np.zeros((nc, len(thr)), dtype=np.int64) for k in ("tp", "fp", "fn", "tn")}
    g = t >= np.float32(gt)
    for k, th in enumerate(thr):
        p = x >= th
        out["tp"][:, k] = (p & g).reshape(nc, -1).sum(1)
        out["fp"][:, k] = (p & ~g).reshape(nc, -1).sum(1)
        out["fn"][:, k] = (~p & g).reshape(nc, -1).sum(1)
        out["tn"][:, k] = (~p & ~g).reshape(nc, -1).sum(1)
    return out


def _counts(x, t, thr, gt):
    bins = (x[..., None] >= thr).sum(-1)
    g = (t >= np.float32(gt)).astype(np.int64)
    nc, K = x.shape[0], len(thr)
    return np.stack([np.bincount((g[n] * (K + 1) + bins[n]).ravel(), minlength=2 * (K + 1)).reshape(2, K + 1) for n in range(nc)])


def test_curves_from_counts_against_direct_evaluation():
    from dmmfods_amd.metrics import curves_from_counts
    rng = np.random.default_rng(3)
    nc, H, W = 4, 24, 40
    x = rng.normal(0, 2, (nc, H, W)).astype(np.float32)
    t = rng.uniform(0, 1, (nc, H, W)).astype(np.float32)
    t[2] = 0.1                                        # a class with no positives
    t[3, :2] = 0.9
    x[3, :2] = -9.0                                   # ... and one whose positives are never predicted at the upper thresholds
    thr = np.asarray([-3.0, -1.0, 0.0, 0.25, 1.5, 40.0], dtype=np.float32)   # the last lies above every logit
    assert x.max() < thr[-1]
    x.ravel()[::17] = thr[2]                          # ties count as >=
    d = _direct(x, t, thr, 0.7)
    got = curves_from_counts(torch.from_numpy(_counts(x, t, thr, 0.7)))
    for k in ("tp", "fp", "fn", "tn"):
        assert got[k].dtype == torch.int64 and np.array_equal(got[k].numpy(), d[k]), k
    tp, fp, fn, tn = (d[k].astype(np.float64) for k in ("tp", "fp", "fn", "tn"))
    with np.errstate(invalid="ignore", divide="ignore"):
        want = {"iou": tp / (tp + fp + fn), "precision": tp / (tp + fp), "recall": tp / (tp + fn), "f1": 2 * tp / (2 * tp + fp + fn),
                "accuracy": (tp + tn) / (tp + tn + fp + fn)}
        rec_next = np.concatenate([want["recall"][:, 1:], np.zeros((nc, 1))], axis=1)
        want["average_precision"] = ((want["recall"] - rec_next) * np.nan_to_num(want["precision"], nan=0.0)).sum(1)
    for k, w in want.items():
        g = got[k].numpy()
        assert got[k].dtype == torch.float64 and g.shape == w.shape, k
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        assert np.allclose(g, w, rtol=0, atol=1e-15, equal_nan=True), (k, np.nanmax(np.abs(g - w)))
    # the class without positives: recall, IoU where nothing is predicted, and the average precision are 0/0
    assert np.isnan(want["recall"][2]).all() and np.isnan(float(got["average_precision"][2])) and np.isnan(float(got["iou"][2, -1]))
    # the threshold above every logit: nothing is predicted - precision 0/0, tp = fp = 0
    assert np.isnan(got["precision"][:, -1].numpy()).all() and int(got["tp"][:, -1].sum()) == 0 and int(got["fp"][:, -1].sum()) == 0
    assert 0 < float(got["average_precision"][0]) <= 1
    # leading dimensions pass through
    both = curves_from_counts(torch.from_numpy(np.stack([_counts(x, t, thr, 0.7)] * 2)))
    assert both["iou"].shape == (2, nc, len(thr)) and torch.equal(both["tp"][1], got["tp"])
    for bad in (torch.zeros(3, 2, 4), torch.zeros(3, 3, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), torch.zeros(3, 2, 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            curves_from_counts(bad)


# ------------------------------------------------------------------------------------------------ ThresholdSweep
def test_threshold_sweep_validates_its_arguments(lib):
    from dmmfods_amd.metrics import ThresholdSweep, logit_thresholds
    s = ThresholdSweep(3, thresholds=[-2, 0, 0.7, 3])
    assert s.thresholds.dtype == np.float32 and s.thresholds.tolist() == [-2.0, 0.0, float(np.float32(0.7)), 3.0] and s.num_thresholds == 4
    assert s.counts is None and s.gt_threshold == 0.7 and s.num_classes == 3
    p = ThresholdSweep(3, probabilities=[0.1, 0.5, 0.9], gt_threshold=0.5)
    want = np.asarray([np.log(0.1 / 0.9), 0.0, np.log(0.9 / (1 - 0.9))], dtype=np.float64).astype(np.float32)
    assert np.array_equal(p.thresholds, want) and np.array_equal(logit_thresholds([0.1, 0.5, 0.9]), want)
    assert ThresholdSweep(1, thresholds=np.linspace(-8, 8, 255)).num_thresholds == 255
    bad = [dict(), dict(thresholds=[0.0], probabilities=[0.5]), dict(thresholds=[]), dict(thresholds=[1.0, 0.0]), dict(thresholds=[0.0, 0.0]),
           dict(thresholds=[0.0, float("nan")]), dict(thresholds=[0.0, float("inf")]), dict(thresholds=np.linspace(-8, 8, 256)),
           dict(thresholds=[1.0, 1.0 + 1e-9]),                       # duplicates after rounding to fp32
           dict(probabilities=[0.9, 0.9 + 1e-10]),                   # distinct in double, one fp32 logit
           dict(probabilities=[0.0, 0.5]), dict(probabilities=[0.5, 1.0]), dict(probabilities=[-0.1]), dict(probabilities=[float("nan")]),
           dict(probabilities=[0.9, 0.1]), dict(probabilities=np.linspace(0.001, 0.999, 256)),
           dict(thresholds=[0.0], gt_threshold=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            ThresholdSweep(3, **kw)
    with pytest.raises(ValueError):
        ThresholdSweep(0, thresholds=[0.0])
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.update(x, x)
    with pytest.raises(RuntimeError):
        s.compute()


# ------------------------------------------------------------------------------------------------ the agent's config field
def test_agent_reads_the_config_field_only_if_present(lib):
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    assert Agent._optional(cfg.agent, "threshold_sweep") is None
    me = types.SimpleNamespace(config=cfg)
    assert Agent._make_sweep(me, None) == (None, None)
    op = np.float32(cfg.agent.iou_threshold)
    sweep, col = Agent._make_sweep(me, 19)
    want = np.union1d(np.log(np.arange(1, 20) / 20.0 / (1 - np.arange(1, 20) / 20.0)).astype(np.float32), [op])
    assert sweep.num_thresholds == 20 and sweep.thresholds[col] == op and np.array_equal(sweep.thresholds, want.astype(np.float32))
    assert sweep.gt_threshold == float(cfg.agent.iou_threshold) and sweep.num_classes == cfg.model.num_classes
    sweep, col = Agent._make_sweep(me, [-1.0, 0.0, 2.5])
    assert sweep.thresholds.tolist() == [-1.0, 0.0, float(op), 2.5] and col == 2
    sweep, col = Agent._make_sweep(me, [-1.0, float(op), 2.5])          # already a column: not twice
    assert sweep.num_thresholds == 3 and col == 1
    for bad in (0, -2, True, [], [1.0, 0.0], [float("nan")], 255):           # 255 + the operating point: one too many
        with pytest.raises(ValueError):
            Agent._make_sweep(me, bad)


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


def test_harness_drives_the_entry_point_and_leaves_the_pinned_trace_alone(drive):
    """DRIVE_HIST=1: behind the plan's life the stand-alone driver calls dmm_logit_hist on three shapes (operands that are addresses
    only, counts a heap block of exactly dmm_logit_hist_elems elements) in both accumulate modes and tries every refusal, under
    ASan + UBSan.  Without the switch the row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = [ln for ln in _run(drive, {}, args) if ln.startswith("T ")]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["(none) | " + args]
    out = _run(drive, {"DRIVE_HIST": "1"}, args)
    assert "HIST OK" in out and len([ln for ln in out if ln.startswith("HIST ") and ln.endswith(" ok")]) == 3, out[-12:]
    hist = [ln for ln in out if ln.startswith("T ")]
    assert hist[:len(base)] == base                                # the plan's schedule is untouched ...
    extra = hist[len(base):]                                       # ... and behind it: per shape memset + launch, then the launch alone
    assert not [ln for ln in extra if ln.startswith("T error")]   # (a refusal that is expected is checked by the driver itself)
    launches = [ln.split() for ln in extra if ln.startswith("T launch")]
    assert len(launches) == 6 and all("logit_hist_kernel" in ln[2] for ln in launches)
    # the grids: about 512 workgroups in all, never more than one four-pixel step per thread, gridDim.y = B * NC
    assert [tuple(map(int, ln[3:5])) for ln in launches] == [(6, 6), (6, 6), (2, 1), (2, 1), (42, 12), (42, 12)]
    memsets = [int(ln.split()[2]) for ln in extra if ln.startswith("T memset")]
    assert memsets == [2 * 3 * 2 * 17 * 8, 1 * 1 * 2 * 2 * 8, 4 * 3 * 2 * 256 * 8]
    assert [ln.split()[1] for ln in extra] == ["memset", "launch", "launch"] * 3
