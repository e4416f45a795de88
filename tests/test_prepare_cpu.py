"""Device-side batch preparation (dmm_prep_image / dmm_prep_lidar / dmm_prep_heat_maps, dmmfods_amd/prepare.py, config.loader.raw_frames)
as far as it goes without a GPU: the entry points and every refusal before HIP is touched, the numpy oracle of the GPU tests
(tools/prepare_ref.py) against direct statements of each rule - torch's pooling layers on the CPU, naive ordered loops, the pedestrian
pattern as five sequential slice assignments - the host-side collation, the agent's config field, and the sanitizer harness
(DRIVE_PREPARE=1 drives the three entry points' argument checks, launch counts and geometry and the workspace memset under ASan + UBSan;
without the switch a pinned enqueue trace keeps its hash)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from tools import prepare_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


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
    for sym in ("dmm_prep_image", "dmm_prep_lidar_workspace", "dmm_prep_lidar", "dmm_prep_heat_maps"):
        assert sym + "(" in header and sym in lib.EXPORTS and hasattr(L, sym), sym
    assert f"#define DMM_PREP_LAUNCH_BATCH {lib.PREP_LAUNCH_BATCH}" in header and "typedef struct dmm_prep_box" in header
    assert lib.PREP_LAUNCH_BATCH == 32 and lib.PREP_MAX_ITEMS == 2 ** 31 // 256
    assert C.sizeof(lib.PrepBox) == 20
    assert [(n, getattr(lib.PrepBox, n).offset) for n, _ in lib.PrepBox._fields_] == [("type", 0), ("x", 4), ("y", 8), ("width", 12), ("height", 16)]
    assert L.dmm_version() >= 102


def test_workspace(lib):
    WS = lib.lib().dmm_prep_lidar_workspace
    for (B, H, W) in ((1, 1, 1), (1, 3, 1), (2, 40, 30), (4, 1280, 1920), (65, 7, 9), (1, 46340, 46340)):
        assert WS(B, H, W) == (B * H * W * 4 + 15) // 16 * 16, (B, H, W)
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -8), (1, 65536, 32768), (1, 46341, 46341)):
        assert WS(*bad) == 0, bad


X, DST, PTS, BOXES, WSP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def _offsets(values):
    return (C.c_int32 * len(values))(*values)


def _refusals(lib, who, call, cases):
    L = lib.lib()
    for kw, msg in cases:
        assert call(**kw) == lib.ERR_INVALID, (who, kw)
        err = L.dmm_last_error()
        assert err.startswith(who) and msg in err, (kw, err)


def test_image_refuses_bad_arguments_before_any_hip_call(lib):
    """Every refusal is made through addresses nothing dereferences: a call that got past the checks would fault here, where there is
    no device."""
    L = lib.lib()
    ok = dict(src=X, ss=3600, dst=DST, ds=36, B=2, H=40, W=30, C=3, p=10)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dmm_prep_image(a["src"], a["ss"], a["dst"], a["ds"], a["B"], a["H"], a["W"], a["C"], a["p"], None)
    _refusals(lib, b"dmm_prep_image: ", call, [
        (dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(dst=DST + 2), b"dst must be 4-byte aligned"),
        (dict(B=0), b">= 1"), (dict(H=0), b">= 1"), (dict(W=-30), b">= 1"), (dict(p=0), b">= 1"), (dict(p=-10), b">= 1"),
        (dict(H=45), b"multiples of pool"), (dict(W=35), b"multiples of pool"),
        (dict(H=65536, W=32768, p=1, ss=2 ** 33, ds=2 ** 33), b"H * W must be < 2^31"),
        (dict(C=0), b"C must be in [1, 4]"), (dict(C=5, ss=6000, ds=60), b"C must be in [1, 4]"),
        (dict(ss=3599), b"src_batch_stride"), (dict(ss=0), b"src_batch_stride"), (dict(ds=35), b"dst_batch_stride"), (dict(ds=-36), b"dst_batch_stride")])


def test_lidar_refuses_bad_arguments_before_any_hip_call(lib):
    L = lib.lib()
    need = L.dmm_prep_lidar_workspace(2, 40, 30)
    ok = dict(pts=PTS, off=(0, 2, 5), dst=DST, ds=12, B=2, H=40, W=30, p=10, k=5, ws=WSP, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        off = None if a["off"] is None else _offsets(a["off"])
        return L.dmm_prep_lidar(a["pts"], off, a["dst"], a["ds"], a["B"], a["H"], a["W"], a["p"], a["k"], a["ws"], a["wsb"], None)
    _refusals(lib, b"dmm_prep_lidar: ", call, [
        (dict(pts=None), b"null points"), (dict(off=None), b"null"), (dict(dst=None), b"null"), (dict(ws=None), b"null"),
        (dict(pts=PTS + 2), b"4-byte aligned"), (dict(dst=DST + 1), b"4-byte aligned"), (dict(ws=WSP + 8), b"workspace must be 16-byte aligned"),
        (dict(B=0), b">= 1"), (dict(H=-40), b">= 1"), (dict(W=0), b">= 1"), (dict(p=0), b">= 1"),
        (dict(H=45), b"multiples of pool"), (dict(W=33), b"multiples of pool"),
        (dict(H=10, ds=3), b"H must be >= 2 * pool"), (dict(H=2, W=2, p=2, ds=1), b"H must be >= 2 * pool"),
        (dict(B=1, off=(0, 2), H=65536, W=32768, p=1, ds=2 ** 33), b"H * W must be < 2^31"),
        (dict(k=0), b"kernel_size"), (dict(k=4), b"kernel_size"), (dict(k=17), b"kernel_size"), (dict(k=-3), b"kernel_size"),
        (dict(ds=11), b"dst_batch_stride"),
        (dict(off=(1, 2, 5)), b"offsets[0] must be 0"), (dict(off=(0, 3, 2)), b"offsets must not decrease"),
        (dict(off=(0, -1, 2)), b"offsets must not decrease"), (dict(off=(0, 2, 2 ** 23 + 1)), b"2^31 / 256"),
        (dict(wsb=need - 1), b"workspace_bytes"), (dict(wsb=0), b"workspace_bytes")])


def test_heat_maps_refuses_bad_arguments_before_any_hip_call(lib):
    L = lib.lib()
    ok = dict(boxes=BOXES, off=(0, 2, 5), dst=DST, ds=36, B=2, H=40, W=30, p=10)

    def call(**kw):
        a = dict(ok, **kw)
        off = None if a["off"] is None else _offsets(a["off"])
        return L.dmm_prep_heat_maps(a["boxes"], off, a["dst"], a["ds"], a["B"], a["H"], a["W"], a["p"], None)
    _refusals(lib, b"dmm_prep_heat_maps: ", call, [
        (dict(boxes=None), b"null boxes"), (dict(off=None), b"null"), (dict(dst=None), b"null"),
        (dict(boxes=BOXES + 2), b"4-byte aligned"), (dict(dst=DST + 3), b"4-byte aligned"),
        (dict(B=-2), b">= 1"), (dict(H=0), b">= 1"), (dict(W=0), b">= 1"), (dict(p=0), b">= 1"),
        (dict(p=7), b"multiples of pool"), (dict(B=1, off=(0, 2), H=65536, W=32768, p=1, ds=2 ** 34), b"H * W must be < 2^31"),
        (dict(ds=35), b"dst_batch_stride"),
        (dict(off=(1, 2, 5)), b"offsets[0] must be 0"), (dict(off=(0, 3, 2)), b"offsets must not decrease"), (dict(off=(0, 2, 2 ** 23 + 1)), b"2^31 / 256")])


# ------------------------------------------------------------------------------------------------ the oracle against direct statements
@pytest.mark.parametrize("p", [1, 2, 3, 10])
def test_ref_image_is_torchs_average_pool(p):
    rng = np.random.default_rng(p)
    for C_ in (1, 3, 4):
        img = rng.integers(0, 256, (4 * p, 3 * p, C_), dtype=np.uint8)
        img[:p, :p] = 255
        img[p:2 * p, :p] = 0
        want = torch.nn.AvgPool2d(p, stride=p)(torch.from_numpy(img).permute(2, 0, 1).float()).numpy()
        got = R.image(img, p)
        assert got.dtype == F32 and got.shape == (C_, 4, 3) and np.array_equal(_bits(got), _bits(want)), (p, C_)
        if p == 1:
            assert np.array_equal(got, img.transpose(2, 0, 1).astype(F32))
    # the reciprocal form is another function: it differs somewhere for p = 3 and 10 (why the rule says division)
    if p in (3, 10):
        S = np.arange(0, 255 * p * p + 1, dtype=np.int64)
        assert np.any((S.astype(F32) / F32(p * p)) != (S.astype(F32) * (F32(1) / F32(p * p))))


def _naive_splat(points, H, W, k):
    """The rule, pixel by pixel and point by point in list order."""
    s = (k - 1) // 2
    plane = np.full((H, W), -1, dtype=F32)
    for x, y, d in np.asarray(points, dtype=F32).reshape(-1, 3):
        if not (np.isfinite([x, y, d]).all() and x >= 0 and y >= 0 and d >= 0):
            continue
        cx, cy = int(x), int(y)
        for row in range(cy - s, cy + s + 1):
            for col in range(cx - s, cx + s + 1):
                if 0 <= row < H - 1 and 0 <= col < W - 1:
                    plane[row, col] = d
    return plane


def _naive_code(plane):
    """The in-place masked assignments, one after the other, in fp32."""
    t = torch.from_numpy(np.array(plane, dtype=F32))
    t[t > 75.0] = 75.0
    t[t == -1.0] = 76.0
    near = t <= 25
    t[near] = t[near] * -6.2 + 255
    far = (t > 25) & (t <= 76.0)         # (on the updated plane: what the first assignment mapped lies in [100, 255], outside)
    t[far] = t[far] * -2 + 150
    return t


@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_ref_lidar_is_the_ordered_splat_the_code_and_torchs_max_pool(k):
    rng = np.random.default_rng(10 + k)
    H, W, p = 12, 10, 2
    pts = np.stack([rng.uniform(-2, W + 3, 60), rng.uniform(-2, H + 3, 60), rng.uniform(0, 90, 60)], axis=1).astype(F32)
    pts[5] = (W - 1, H - 1, 3)
    pts[6] = (W + 1, H + 1, 3)
    pts[7:13, 2] = (0, 25, np.nextafter(F32(25), F32(np.inf)), 75, 76.5, 24.999)
    pts[13] = (np.nan, 2, 2)
    pts[14] = (2, np.inf, 2)
    pts[15] = (2, 2, -1)
    pts[16] = (-0.0, -0.0, 4)
    plane = _naive_splat(pts, H, W, k)
    owner = R.lidar_owner(pts, H, W, k)
    assert np.array_equal(_bits(np.where(owner >= 0, pts[np.maximum(owner, 0), 2], F32(-1))), _bits(plane))
    assert np.all(plane[H - 1] == -1) and np.all(plane[:, W - 1] == -1)          # the last row and column are never written
    coded = _naive_code(plane)
    assert np.array_equal(_bits(R.lidar_code(plane)), _bits(coded.numpy()))
    pooled = torch.nn.MaxPool2d((2 * p, p), stride=(p, p))(coded[None])
    pooled = torch.nn.functional.pad(pooled[None], pad=(0, 0, 0, 1), mode="replicate")[0]
    pooled[pooled < 0] = 0
    got = R.lidar(pts, H, W, p, k)
    assert got.shape == (1, H // p, W // p) and np.array_equal(_bits(got), _bits(pooled.numpy()))
    full = coded.clone()
    full[full < 0] = 0
    assert np.array_equal(_bits(R.lidar(pts, H, W, 1, k)), _bits(full.numpy()[None]))
    assert np.array_equal(R.lidar(np.zeros((0, 3), F32), H, W, p, k), np.zeros((1, H // p, W // p), F32))


def test_ref_lidar_code_at_the_breakpoints():
    v = np.array([-1, 0, 25, np.nextafter(F32(25), F32(np.inf)), 75, 76.5, 1000], dtype=F32)
    got = R.lidar_code(v)
    assert got.tolist()[:3] == [-2.0, 255.0, 100.0] and got[4] == 0.0 and got[5] == 0.0 and got[6] == 0.0
    assert got[3] == F32(F32(v[3] * F32(-2)) + F32(150))          # (the far branch: -50.000004 + 150, which rounds to 100)
    # two roundings, not one: a fused multiply-add gives another float somewhere on [0, 25]
    e = np.linspace(0, 25, 100001).astype(F32)
    fused = (e.astype(np.float64) * np.float64(F32(-6.2)) + 255.0).astype(F32)
    assert np.any(fused != R.lidar_code(e))


def _five_assignments(height, width):
    """The pedestrian pattern as five sequential slice assignments on a box of ones."""
    box = np.ones((height, width), dtype=F32)
    hf, wf = height // 5, width // 4
    box[0:hf, :wf] = 0.3
    box[0:hf, wf * 3:] = 0.3
    box[hf * 3:, :wf] = 0.5
    box[hf * 3:, wf * 3:] = 0.5
    box[hf * 3:, wf:wf * 3] = 0.75
    return box


def test_ref_pedestrian_pattern_is_the_five_assignments_for_all_sizes():
    for h in range(1, 41):
        for w in range(1, 41):
            assert np.array_equal(_bits(R.box_pattern(2, h, w)), _bits(_five_assignments(h, w))), (h, w)
            assert np.all(R.box_pattern(1, h, w) == 1) and np.all(R.box_pattern(4, h, w) == 1)


def _naive_heat(boxes, H, W):
    """The rule, pixel by pixel: the last box of the class in list order that covers the pixel."""
    out = np.zeros((3, H, W), dtype=F32)
    for Y in range(H):
        for X in range(W):
            for t, x, y, w, h in boxes:
                if t in (1, 2, 4) and w > 0 and h > 0 and x <= X < x + w and y <= Y < y + h:
                    v = 1.0
                    if t == 2:
                        r, c, hf, wf = Y - y, X - x, h // 5, w // 4
                        side = c < wf or c >= 3 * wf
                        v = 0.3 if (r < hf and side) else ((0.5 if side else 0.75) if r >= 3 * hf else 1.0)
                    out[{1: 0, 2: 1, 4: 2}[t], Y, X] = v
    return out


def test_ref_heat_maps_are_the_ordered_overwrite_and_torchs_max_pool():
    rng = np.random.default_rng(3)
    H, W = 20, 24
    boxes = [[int(rng.choice([1, 2, 2, 3, 4])), int(rng.integers(-6, W)), int(rng.integers(-6, H)), int(rng.integers(-1, 14)), int(rng.integers(-1, 14))]
             for _ in range(40)]
    boxes += [[2, 3, 2, 12, 10], [2, 5, 4, 8, 10], [1, -3, -3, 2 ** 31 - 1, 5], [4, W, 0, 3, 3], [2, 0, H - 1, 4, 5]]
    full = R.heat_maps_full(boxes, H, W)
    assert np.array_equal(_bits(full), _bits(_naive_heat(boxes, H, W)))
    assert set(np.unique(full).tolist()) <= {0.0, float(F32(0.3)), 0.5, 0.75, 1.0}
    for p in (1, 2, 4):
        want = torch.nn.MaxPool2d(p, stride=p)(torch.from_numpy(full)).numpy()
        assert np.array_equal(_bits(R.heat_maps(boxes, H, W, p)), _bits(want)), p
    # inside the image the rule is the slice assignment of whole patterns
    inside = [[2, 1, 1, 9, 11], [1, 0, 0, 5, 5], [2, 4, 6, 7, 9], [4, 10, 10, 14, 10]]
    maps = np.zeros((3, H, W), dtype=F32)
    for t, x, y, w, h in inside:
        maps[{1: 0, 2: 1, 4: 2}[t], y:y + h, x:x + w] = _five_assignments(h, w) if t == 2 else 1.0
    assert np.array_equal(_bits(R.heat_maps_full(inside, H, W)), _bits(maps))
    assert not R.heat_maps([], H, W, 2).any()


# ------------------------------------------------------------------------------------------------ host side
def test_collate_raw_and_labels_to_boxes():
    from dmmfods_amd.prepare import BatchPrepare, RawBatch, collate_raw, labels_to_boxes
    labels = {"b": dict(type=2, x=5, y=6, width=7, height=8, id="x"), "a": dict(type=1, x=1.0, y=2, width=3, height=4), "c": dict(type=4, x=-1, y=0, width=2, height=2)}
    boxes = labels_to_boxes(labels)
    assert boxes.dtype == torch.int32 and boxes.tolist() == [[2, 5, 6, 7, 8], [1, 1, 2, 3, 4], [4, -1, 0, 2, 2]]     # dict order
    assert labels_to_boxes({}).shape == (0, 5) and labels_to_boxes({}).dtype == torch.int32
    rng = np.random.default_rng(0)
    frames = [dict(image=torch.from_numpy(rng.integers(0, 256, (8, 6, 3), dtype=np.uint8)), points=torch.rand(n, 3), boxes=boxes[:m])
              for n, m in ((4, 3), (0, 0), (2, 1))]
    raw = collate_raw(frames)
    assert isinstance(raw, RawBatch) and len(raw) == 3
    assert raw.image.dtype == torch.uint8 and raw.image.shape == (3, 8, 6, 3) and torch.equal(raw.image[2], frames[2]["image"])
    assert raw.point_offsets.dtype == torch.int32 and raw.point_offsets.tolist() == [0, 4, 4, 6] and raw.box_offsets.tolist() == [0, 3, 3, 4]
    assert raw.points.dtype == torch.float32 and raw.points.shape == (6, 3) and torch.equal(raw.points[4:], frames[2]["points"])
    assert raw.boxes.dtype == torch.int32 and raw.boxes.tolist() == boxes.tolist() + boxes[:1].tolist()
    none = collate_raw([dict(image=frames[0]["image"], points=np.zeros((0, 3), F32), boxes=np.zeros((0, 5), np.int32))])
    assert none.points.shape == (0, 3) and none.boxes.shape == (0, 5) and none.point_offsets.tolist() == [0, 0]
    with pytest.raises(ValueError):
        collate_raw([])
    with pytest.raises(ValueError):
        collate_raw([frames[0], dict(frames[1], image=torch.zeros(8, 7, 3, dtype=torch.uint8))])
    with pytest.raises(ValueError):
        collate_raw([dict(frames[0], image=torch.zeros(8, 6, 3))])
    bp = BatchPrepare()
    assert (bp.pool, bp.kernel_size) == (10, 5) and bp.output_size(1280, 1920) == (128, 192)
    for kw in (dict(pool=0), dict(pool=2.5), dict(pool=True), dict(kernel_size=4), dict(kernel_size=17), dict(kernel_size=-1), dict(kernel_size="5")):
        with pytest.raises(ValueError):
            BatchPrepare(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bp(raw, device="cpu")


def test_raw_frames_dataset_reads_one_dict_per_frame(tmp_path):
    from dmmfods_amd.datasets.RawFrames import RawFrames_Loader
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    rng = np.random.default_rng(1)
    for mode, n in (("train", 5), ("val", 2)):
        os.makedirs(tmp_path / mode)
        for i in range(n):
            torch.save({"image": torch.from_numpy(rng.integers(0, 256, (8, 6, 3), dtype=np.uint8)), "points": torch.full((i, 3), float(i)),
                        "boxes": torch.tensor([[1, i, 0, 2, 2]], dtype=torch.int32)}, str(tmp_path / mode / f"frame_{i:04d}.pt"))
    cfg = get_config(str(tmp_path))
    cfg.dir.data.root = str(tmp_path)
    cfg.loader.mode, cfg.loader.batch_size, cfg.loader.num_workers, cfg.loader.pin_memory, cfg.loader.drop_last = "train", 2, 0, False, False
    loader = RawFrames_Loader(cfg)
    assert (loader.train_iterations, loader.valid_iterations) == (3, 1)
    batches = list(loader.train_loader)
    assert [len(b) for b in batches] == [2, 2, 1] and batches[1].point_offsets.tolist() == [0, 2, 5] and batches[1].boxes[:, 1].tolist() == [2, 3]
    assert len(list(loader.valid_loader)) == 1


# ------------------------------------------------------------------------------------------------ the agent's config field
def test_agent_reads_the_config_field_only_if_present(lib):
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    assert Agent._optional(cfg.loader, "raw_frames") is None and Agent._make_prepare(None) is None
    bp = Agent._make_prepare({})
    assert (bp.pool, bp.kernel_size) == (10, 5)
    bp = Agent._make_prepare(dict(pool=2, kernel_size=7))
    assert (bp.pool, bp.kernel_size) == (2, 7)
    for bad in (True, 10, [10], dict(pol=10), dict(pool=0), dict(kernel_size=6), dict(pool="10")):
        with pytest.raises(ValueError, match="loader.raw_frames"):
            Agent._make_prepare(bad)


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


def test_harness_drives_the_entry_points_and_leaves_the_pinned_trace_alone(drive, lib):
    """DRIVE_PREPARE=1: behind the plan's life the stand-alone driver calls the three entry points on B = 1, 33 and 65 samples at pool 10
    and 1 (operands that are addresses only; the workspace real, with a guard band), and tries every refusal, under ASan + UBSan.  Without
    the switch the row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = [ln for ln in _run(drive, {}, args) if ln.startswith("T ")]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["(none) | " + args]
    out = _run(drive, {"DRIVE_PREPARE": "1"}, args)
    assert "PREPARE OK" in out and len([ln for ln in out if ln.startswith("PREPARE ") and ln.endswith(" ok")]) == 6, out[-12:]
    trace = [ln for ln in out if ln.startswith("T ")]
    assert trace[:len(base)] == base                               # the plan's schedule is untouched ...
    extra = trace[len(base):]                                      # ... and behind it, per (B, pool):
    H, W, K = 40, 30, 5
    want = []
    for B in (1, 33, 65):
        chunks = [min(32, B - b0) for b0 in range(0, B, 32)]
        points = [7 * (min(b0 + nb, 33) - min(b0, 33)) for b0, nb in zip(range(0, B, 32), chunks)]
        for p in (10, 1):
            plane = (H // p) * (W // p)
            gx = -(-plane // 256)
            want += [("launch", "prep_image_kernel", gx, 3)] * len(chunks)
            want.append(("memset", B * H * W * 4))
            for nb, n in zip(chunks, points):
                if n:
                    want.append(("launch", "prep_lidar_splat_kernel", -(-n * K * K // 256), 1))
                want.append(("launch", "prep_lidar_pool_kernel", gx, nb))
            want += [("launch", "prep_heat_kernel", -(-(H // p) // 16) * -(-(W // p) // 16), nb) for nb in chunks]
    assert len(extra) == len(want), (len(extra), len(want))
    for ln, w in zip(extra, want):
        f = ln.split()
        if w[0] == "memset":
            assert f[1] == "memset" and int(f[2]) == w[1], (ln, w)
        else:
            assert f[1] == "launch" and w[1] in f[2] and (int(f[3]), int(f[4])) == w[2:], (ln, w)
