"""Device-side batch preparation on the GPU: dmm_prep_image, dmm_prep_lidar and dmm_prep_heat_maps (csrc/prepare.hip) against the numpy
restatement of their rules (tools/prepare_ref.py, itself held against torch's pooling layers and naive loops in test_prepare_cpu.py),
and what stands on them (dmmfods_amd.prepare.BatchPrepare, the agent's config.loader.raw_frames).

Every comparison is BIT FOR BIT: each output is an integer sum under one division, a coded copy of an input under two stated roundings,
or one of four constants.  Throughout (the `_Rig` below): the three outputs are written into the channel slices of one (B, C + 4, Ho, Wo)
tensor that starts as a sentinel pattern with a margin on either side - so every element of a dst must be written, and nothing else may
be, neither the other slices nor the margins nor the guard bands around the LiDAR workspace; the inputs are compared with copies taken
before; every call is made three times and the three results must agree in every bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
from tools import prepare_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
SENT = 0x7fc0dead                                                           # a NaN no kernel here produces
MARGIN = 64                                                                 # elements (dst) / bytes (workspace) on either side


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


class _Rig:
    """One (B, nch, Ho, Wo) batch between two margins, all sentinel; `slice_ptr(c)` is the address of channel c of sample 0."""

    def __init__(self, B, nch, Ho, Wo):
        self.B, self.nch, self.plane, self.shape = B, nch, Ho * Wo, (B, nch, Ho, Wo)
        self.buf = torch.full((2 * MARGIN + B * nch * Ho * Wo,), SENT, dtype=torch.int32, device=DEV)

    @property
    def stride(self):
        return self.nch * self.plane

    def slice_ptr(self, c):
        return self.buf.data_ptr() + 4 * (MARGIN + c * self.plane)

    def result(self, c0, c1):
        """The bits of channels [c0, c1) after checking that everything else still holds the sentinel."""
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy().view(np.uint32)
        sent = np.uint32(SENT)
        assert np.all(host[:MARGIN] == sent) and np.all(host[-MARGIN:] == sent), "a margin of the batch was written"
        body = host[MARGIN:-MARGIN].reshape(self.shape)
        assert np.all(body[:, :c0] == sent) and np.all(body[:, c1:] == sent), "another slice of the batch was written"
        return body[:, c0:c1].copy()


def _thrice(make):
    """make() -> bits; three fresh runs, all equal."""
    a, b, c = make(), make(), make()
    assert np.array_equal(a, b) and np.array_equal(a, c), "two runs of one call differ"
    return a


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ image
def run_image(L, img, p, shift=0, pad=0):
    """img uint8 (B, H, W, C).  shift: the source starts that many bytes behind a 256-byte boundary; pad: extra bytes between samples."""
    B, H, W, Cc = img.shape
    Ho, Wo = H // p, W // p
    stride = H * W * Cc + pad
    host = np.full(B * stride, 0xEE, dtype=np.uint8)
    for b in range(B):
        host[b * stride:b * stride + H * W * Cc] = img[b].reshape(-1)
    raw = torch.zeros(shift + B * stride + 256, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 256 == 0
    raw[shift:shift + B * stride] = torch.from_numpy(host).to(DEV)
    before = raw.clone()

    def make():
        rig = _Rig(B, Cc + 4, Ho, Wo)
        L.check(L.lib().dmm_prep_image(raw.data_ptr() + shift, stride, rig.slice_ptr(0), rig.stride, B, H, W, Cc, p, L.stream_ptr()))
        return rig.result(0, Cc)
    got = _thrice(make)
    assert torch.equal(raw, before), "the source was written"
    want = np.stack([R.image(img[b], p) for b in range(B)])
    assert np.array_equal(got, _bits(want)), f"image {img.shape} pool {p}: {np.count_nonzero(got != _bits(want))} elements differ"


IMAGE_CASES = {
    "60x50x3_pool10": (2, 60, 50, 3, 10), "12x14_pool2": (1, 12, 14, 3, 2), "9x7_pool1": (2, 9, 7, 3, 1), "9x6_pool3": (2, 9, 6, 3, 3),
    "one_channel": (2, 12, 14, 1, 2), "four_channels": (2, 12, 14, 4, 2), "four_channels_pool1": (1, 9, 7, 4, 1),
    "two_workgroups": (1, 34, 18, 3, 1), "B33": (33, 6, 4, 3, 2),
}


@pytest.mark.parametrize("case", list(IMAGE_CASES))
def test_image(L, case):
    B, H, W, Cc, p = IMAGE_CASES[case]
    rng = np.random.default_rng(B * 10000 + H * 100 + W + Cc + p)
    run_image(L, rng.integers(0, 256, (B, H, W, Cc), dtype=np.uint8), p)


def test_image_9x7_at_pool_3_is_refused(L):
    """7 is no multiple of 3: the rule (H % p == 0 and W % p == 0) refuses the shape; 9 x 6 at pool 3 is in the list above."""
    src = torch.zeros(9 * 7 * 3, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(3 * 3 * 2, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="dmm_prep_image: H and W must be multiples of pool"):
        L.check(L.lib().dmm_prep_image(src.data_ptr(), 9 * 7 * 3, dst.data_ptr(), 18, 1, 9, 7, 3, 3, L.stream_ptr()))
    torch.cuda.synchronize()
    assert not dst.any()


def test_image_division_not_reciprocal(L):
    """Every block sum 0 .. 255 * p * p is reachable; a plane whose blocks run through many of them holds the sums at which a multiplication
    with the reciprocal rounds differently (p = 3 and p = 10: test_prepare_cpu.py shows such sums exist)."""
    for p in (3, 10):
        n = 255 * p * p + 1
        sums = np.arange(n)
        differ = sums[(sums.astype(F32) / F32(p * p)) != (sums.astype(F32) * (F32(1) / F32(p * p)))]
        assert len(differ) > 0
        pick = differ[:48]
        img = np.zeros((1, 6 * p, 8 * p, 1), dtype=np.uint8)
        for n_, s in enumerate(pick):
            blk = np.full(p * p, s // (p * p), dtype=np.int64)
            blk[:s % (p * p)] += 1
            i, j = divmod(n_, 8)
            img[0, i * p:(i + 1) * p, j * p:(j + 1) * p, 0] = blk.reshape(p, p)
        run_image(L, img, p)


def test_image_extremes_alignment_and_stride(L):
    run_image(L, np.full((2, 20, 30, 3), 255, dtype=np.uint8), 10)
    run_image(L, np.zeros((2, 20, 30, 3), dtype=np.uint8), 10)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (3, 12, 14, 3), dtype=np.uint8)
    run_image(L, img, 2, shift=15)                  # one byte in front of a 16-byte boundary
    run_image(L, img, 1, shift=1)
    run_image(L, img, 2, pad=37)                    # samples further apart than one image
    run_image(L, img, 2, shift=15, pad=5)


# ------------------------------------------------------------------------------------------------ LiDAR
def run_lidar(L, samples, H, W, p, k=5):
    """samples: one (n, 3) array of (x, y, d) per sample."""
    B = len(samples)
    Ho, Wo = H // p, W // p
    samples = [np.asarray(s, dtype=F32).reshape(-1, 3) for s in samples]
    off = _offsets(samples)
    pts = torch.from_numpy(np.concatenate(samples + [np.zeros((1, 3), F32)])).to(DEV)     # (one spare row: never a null pointer)
    before = pts.clone()
    need = L.lib().dmm_prep_lidar_workspace(B, H, W)
    assert need == (B * H * W * 4 + 15) // 16 * 16

    def make():
        rig = _Rig(B, 7, Ho, Wo)
        ws = torch.full((need + 2 * MARGIN,), 0xA5, dtype=torch.uint8, device=DEV)
        assert (ws.data_ptr() + MARGIN) % 16 == 0
        L.check(L.lib().dmm_prep_lidar(pts.data_ptr(), off.ctypes.data_as(C.POINTER(C.c_int32)), rig.slice_ptr(3), rig.stride, B, H, W, p, k,
                                       ws.data_ptr() + MARGIN, need, L.stream_ptr()))
        got = rig.result(3, 4)
        assert bool((ws[:MARGIN] == 0xA5).all()) and bool((ws[-MARGIN:] == 0xA5).all()), "a guard band of the workspace was written"
        return got
    got = _thrice(make)
    assert torch.equal(pts.view(torch.int32), before.view(torch.int32)), "the points were written"
    want = np.stack([R.lidar(s, H, W, p, k) for s in samples])
    assert np.array_equal(got, _bits(want)), f"lidar {H}x{W} pool {p} k {k}: {np.count_nonzero(got != _bits(want))} elements differ"
    return got.view(F32)


def _random_points(rng, n, H, W):
    return np.stack([rng.uniform(-1, W + 4, n), rng.uniform(-1, H + 4, n), rng.uniform(0, 90, n)], axis=1).astype(F32)


@pytest.mark.parametrize("shape", [(60, 50, 10), (40, 30, 10), (20, 30, 10), (8, 8, 2), (8, 8, 1)], ids=lambda s: "%dx%d_pool%d" % s)
@pytest.mark.parametrize("k", [1, 5, 7])
def test_lidar_random_points(L, shape, k):
    H, W, p = shape
    rng = np.random.default_rng(H * 1000 + W * 10 + k)
    run_lidar(L, [_random_points(rng, 50, H, W), _random_points(rng, 17, H, W)], H, W, p, k)


def test_lidar_last_writer_wins(L):
    """Two points on one pixel in both orders: the higher index gives the value, whatever the values are."""
    a = run_lidar(L, [[[3, 3, 10], [3, 3, 40]]], 8, 8, 1, 1)
    b = run_lidar(L, [[[3, 3, 40], [3, 3, 10]]], 8, 8, 1, 1)
    assert a[0, 0, 3, 3] == R.lidar_code(F32(40)) and b[0, 0, 3, 3] == R.lidar_code(F32(10)) and a[0, 0, 3, 3] != b[0, 0, 3, 3]
    run_lidar(L, [[[3.2, 3.9, 10], [4.5, 2.1, 40], [3, 3, 60]], [[3, 3, 60], [4.5, 2.1, 40], [3.2, 3.9, 10]]], 8, 8, 2, 5)


def test_lidar_edges_of_the_plane(L):
    """The last row and column are never written; a window may be empty; far points write nothing."""
    H, W = 8, 8
    for k in (1, 5):
        got = run_lidar(L, [[[W - 1, H - 1, 5]]], H, W, 1, k)
        assert np.all(got[0, 0, H - 1] == 0) and np.all(got[0, 0, :, W - 1] == 0)
        assert (got[0, 0, H - 2, W - 2] == R.lidar_code(F32(5))) == (k == 5) and np.count_nonzero(got) == (4 if k == 5 else 0)
        assert not run_lidar(L, [[[W + 1, H + 1, 5]]], H, W, 1, k).any()     # k = 5: rows [H - 1, H - 1), an empty window
    run_lidar(L, [[[W + 2, 3, 5], [3, H + 2, 5], [W + 7, H + 9, 5], [1e9, 3, 5], [3, 3e38, 5], [0, 0, 5]]], H, W, 2, 5)
    run_lidar(L, [[[W - 2, H - 2, 5], [W - 1.5, 0.5, 7], [0.5, H - 1.5, 9]]], H, W, 2, 3)
    run_lidar(L, [[[29, 19, 12], [0, 10, 3], [15, 9.99, 30]]], 20, 30, 10, 5)          # H == 2 * pool: both output rows are one window


def test_lidar_invalid_points_are_skipped(L):
    nan, inf = np.nan, np.inf
    bad = [[nan, 3, 5], [3, nan, 5], [3, 3, nan], [inf, 3, 5], [3, inf, 5], [3, 3, inf], [-inf, 3, 5], [-1, 3, 5], [3, -0.5, 5], [3, 3, -1], [3, 3, -1e-30]]
    got = run_lidar(L, [bad], 8, 8, 1, 5)
    assert not got.any()
    got = run_lidar(L, [[[4, 4, 50]] + bad], 8, 8, 1, 5)                      # none of them overwrites the valid point in front
    assert got[0, 0, 4, 4] == F32(50)
    got = run_lidar(L, [[[-0.0, -0.0, -0.0]]], 8, 8, 1, 1)                    # -0.0 >= 0: valid, d = -0.0 codes as 255
    assert got[0, 0, 0, 0] == F32(255) and np.count_nonzero(got) == 1


def test_lidar_code_breakpoints(L):
    up = np.nextafter(F32(25), F32(np.inf))
    ds = [0, 25, 75, 76.5, up, 24.999, 25.5, 74.99, 1e-3, 12.345, 1000]
    pts = [[2 * n % 14, 2 * (2 * n // 14), d] for n, d in enumerate(ds)]
    got = run_lidar(L, [pts], 8, 16, 1, 1)
    assert got[0, 0, 0, 0] == 255 and got[0, 0, 0, 2] == 100 and got[0, 0, 0, 4] == 0 and got[0, 0, 0, 6] == 0
    # values at which (e * -6.2f) + 255 in one rounding differs from two: the fused form must not appear
    e = np.linspace(0, 25, 20001).astype(F32)
    fused = (e.astype(np.float64) * np.float64(F32(-6.2)) + 255.0).astype(F32)
    pick = e[fused != R.lidar_code(e)][:60]
    assert len(pick) >= 10
    run_lidar(L, [[[n % 15, n // 15, d] for n, d in enumerate(pick)]], 8, 16, 1, 1)


def test_lidar_samples_and_chunks(L):
    rng = np.random.default_rng(77)
    assert not run_lidar(L, [np.zeros((0, 3), F32)], 8, 8, 2, 5).any()                       # a sample with no points: all zeros
    assert not run_lidar(L, [np.zeros((0, 3), F32)] * 2, 20, 30, 10, 5).any()
    got = run_lidar(L, [_random_points(rng, 9, 8, 8), np.zeros((0, 3), F32), _random_points(rng, 30, 8, 8)], 8, 8, 2, 5)
    assert not got[1].any() and got[0].any() and got[2].any()
    for B in (33, 65):                                                                        # two and three launch chunks
        run_lidar(L, [_random_points(rng, int(rng.integers(0, 12)) * (b != 40), 8, 12) for b in range(B)], 8, 12, 2, 3)
    run_lidar(L, [_random_points(rng, 5, 8, 12) if b < 3 else np.zeros((0, 3), F32) for b in range(65)], 8, 12, 2, 3)   # chunks without points


def test_lidar_padded_row_repeats_the_row_above(L):
    """The last output row is row Ho - 2's window again, not a window of its own: a point in rows [(Ho - 2) * p, (Ho - 1) * p) shows in
    it although a window that started at row (Ho - 1) * p would not hold it."""
    H, W, p = 40, 30, 10
    v = float(R.lidar_code(F32(20)))
    got = run_lidar(L, [[[5, 12, 20]]], H, W, p, 1)          # row 12: windows r = 0 (rows 0..19) and r = 1 (rows 10..29)
    assert got[0, 0, :, 0].tolist() == [v, v, 0.0, 0.0]
    got = run_lidar(L, [[[5, 25, 20]]], H, W, p, 1)          # row 25: r = 1 and r = 2 (rows 20..39); output row 3 repeats r = 2
    assert got[0, 0, :, 0].tolist() == [0.0, v, v, v]
    got = run_lidar(L, [[[5, 33, 20]]], H, W, p, 1)          # row 33: r = 2 only - and the padded row
    assert got[0, 0, :, 0].tolist() == [0.0, 0.0, v, v]


# ------------------------------------------------------------------------------------------------ heat maps
def run_heat(L, samples, H, W, p):
    """samples: one list of (type, x, y, width, height) per sample."""
    B = len(samples)
    Ho, Wo = H // p, W // p
    samples = [np.asarray(s, dtype=np.int64).reshape(-1, 5) for s in samples]
    off = _offsets(samples)
    host = np.concatenate(samples + [np.zeros((1, 5), np.int64)]).astype(np.int32)
    boxes = torch.from_numpy(host).to(DEV)
    before = boxes.clone()

    def make():
        rig = _Rig(B, 7, Ho, Wo)
        L.check(L.lib().dmm_prep_heat_maps(boxes.data_ptr(), off.ctypes.data_as(C.POINTER(C.c_int32)), rig.slice_ptr(4), rig.stride, B, H, W, p,
                                           L.stream_ptr()))
        return rig.result(4, 7)
    got = _thrice(make)
    assert torch.equal(boxes, before), "the boxes were written"
    want = np.stack([R.heat_maps(s, H, W, p) for s in samples])
    assert np.array_equal(got, _bits(want)), f"heat maps {H}x{W} pool {p}: {np.count_nonzero(got != _bits(want))} elements differ"
    return got.view(F32)


POOLS = [1, 2, 10]


@pytest.mark.parametrize("p", POOLS)
def test_heat_every_type_and_pedestrian_sizes(L, p):
    H, W = 40, 60
    got = run_heat(L, [[[1, 2, 3, 9, 7], [2, 20, 5, 12, 20], [4, 40, 10, 8, 8], [3, 0, 0, 30, 30], [0, 5, 5, 9, 9], [5, 5, 5, 9, 9], [-1, 5, 5, 9, 9]]], H, W, p)
    assert got[0, 0].any() and got[0, 1].any() and got[0, 2].any()
    for (h, w) in ((1, 1), (3, 4), (4, 3), (5, 4), (20, 12)):
        for (x, y) in ((0, 0), (7, 9), (W - w, H - h)):
            run_heat(L, [[[2, x, y, w, h]]], H, W, p)


@pytest.mark.parametrize("p", POOLS)
def test_heat_order_within_and_across_classes(L, p):
    H, W = 40, 60
    ped, veh = [2, 10, 5, 12, 20], [1, 8, 8, 20, 10]
    a = run_heat(L, [[ped, veh]], H, W, p)
    b = run_heat(L, [[veh, ped]], H, W, p)
    assert np.array_equal(a, b)                                     # classes do not touch each other
    # two pedestrian boxes, both orders: the later one's 0.3 corners and 0.5 / 0.75 feet overwrite the earlier one's 1
    first, second = [2, 10, 5, 12, 20], [2, 14, 9, 12, 20]
    a = run_heat(L, [[first, second]], H, W, p)
    b = run_heat(L, [[second, first]], H, W, p)
    assert not np.array_equal(a, b)
    if p == 1:
        assert a[0, 1, 9, 14] == F32(0.3) and b[0, 1, 9, 14] == F32(1)
    # a later box whose whole 0.3 corner covers a pooled block of an earlier 1 lowers the pooled value (pool 2: corner 4 x 3 of a 20 x 12 box)
    low = run_heat(L, [[[2, 0, 0, 40, 40], [2, 20, 20, 12, 20]]], H, W, p)
    if p == 2:
        assert low[0, 1, 10, 10] == F32(0.3)


@pytest.mark.parametrize("p", POOLS)
def test_heat_clipping_and_ignored_boxes(L, p):
    H, W = 40, 60
    over = [[2, -5, 10, 12, 20], [2, W - 6, 10, 12, 20], [2, 20, -7, 12, 20], [2, 20, H - 9, 12, 20], [1, -3, -3, 8, 8], [4, W - 2, H - 2, 9, 9],
            [2, -4, -6, W + 10, H + 13]]
    for bx in over:
        run_heat(L, [[bx]], H, W, p)
    run_heat(L, [over], H, W, p)
    outside = [[1, W, 0, 5, 5], [1, 0, H, 5, 5], [2, -12, 3, 12, 20], [4, 3, -20, 12, 20], [1, 2 ** 31 - 10, 3, 5, 5], [1, -2 ** 31, -2 ** 31, 5, 5]]
    assert not run_heat(L, [outside], H, W, p).any()
    none = [[1, 5, 5, 0, 9], [1, 5, 5, 9, 0], [2, 5, 5, -3, 9], [4, 5, 5, 9, -2 ** 31], [1, 5, 5, -1, -1]]
    assert not run_heat(L, [none], H, W, p).any()
    # x + width beyond int32: the bounds are formed in 64-bit
    got = run_heat(L, [[[1, 30, 10, 2 ** 31 - 1, 4], [2, 2 ** 31 - 5, 10, 2 ** 31 - 1, 2 ** 31 - 1], [4, 10, 2 ** 31 - 1, 5, 2 ** 31 - 1],
                        [2, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1], [2, -8, 20, 2 ** 31 - 1, 2 ** 31 - 1]]], H, W, p)
    assert got[0, 0].any() and got[0, 1].any() and not got[0, 2].any()


@pytest.mark.parametrize("p", POOLS)
def test_heat_more_boxes_than_one_chunk(L, p):
    """300 boxes in one sample (the workgroup culls 256 list entries at a time): the box that decides a pixel first, last and in
    the middle of the list; every box touches every tile's neighbourhood."""
    H, W = 40, 60
    rng = np.random.default_rng(31 + p)
    filler = [[int(rng.choice([1, 2, 4])), int(rng.integers(-5, W)), int(rng.integers(-5, H)), int(rng.integers(1, 25)), int(rng.integers(1, 25))] for _ in range(298)]
    big = [2, 0, 0, W, H]
    run_heat(L, [[big] + filler + [[1, 3, 3, 4, 4]]], H, W, p)        # deciding pedestrian box first: everything behind it overwrites
    got = run_heat(L, [filler + [[1, 3, 3, 4, 4], big]], H, W, p)     # ... and last: the plane is exactly its pattern
    assert np.array_equal(_bits(got[0, 1]), _bits(R.heat_maps([big], H, W, p)[1]))
    run_heat(L, [filler[:150] + [big] + filler[150:]], H, W, p)
    only_first = [[4, 1, 1, 6, 6]] + [[1, 0, 0, W, H]] * 299           # a class whose only box is entry 0 of a two-chunk list
    got = run_heat(L, [only_first], H, W, p)
    assert got[0, 2].any()
    run_heat(L, [filler * 3], H, W, p)                                 # 894 boxes: four chunks


def test_heat_samples_and_chunks(L):
    rng = np.random.default_rng(8)
    H, W = 20, 20

    def some(n):
        return [[int(rng.choice([1, 2, 4, 3])), int(rng.integers(-4, W)), int(rng.integers(-4, H)), int(rng.integers(0, 15)), int(rng.integers(0, 15))] for _ in range(n)]
    assert not run_heat(L, [[]], H, W, 2).any()
    got = run_heat(L, [some(6), [], some(9)], H, W, 2)
    assert not got[1].any()
    run_heat(L, [some(int(rng.integers(0, 7))) for _ in range(33)], H, W, 2)
    run_heat(L, [some(3) for _ in range(65)], H, W, 10)
    run_heat(L, [some(40)], 48, 80, 1)                                 # ragged tiles: 3 x 5 tiles of 16 x 16 output pixels
    run_heat(L, [some(40)], 34, 36, 2)                                 # 17 x 18 output pixels: four tiles, three of them ragged


# ------------------------------------------------------------------------------------------------ the reference's own size
def _frame(rng, H, W, npoints, nboxes):
    pts = np.stack([rng.uniform(0, W, npoints), rng.uniform(0, H, npoints), rng.uniform(0, 80, npoints)], axis=1).astype(F32)
    boxes = np.stack([rng.choice([1, 2, 4], nboxes), rng.integers(0, W - 200, nboxes), rng.integers(0, H - 200, nboxes), rng.integers(5, 200, nboxes),
                      rng.integers(5, 200, nboxes)], axis=1).astype(np.int32)
    return dict(image=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), points=pts, boxes=boxes)


def test_full_size_frame(L):
    H, W, p = 1280, 1920, 10
    f = _frame(np.random.default_rng(2024), H, W, 3000, 40)
    run_image(L, f["image"][None], p)
    run_lidar(L, [f["points"]], H, W, p, 5)
    run_heat(L, [f["boxes"]], H, W, p)


# ------------------------------------------------------------------------------------------------ BatchPrepare
def test_batch_prepare_on_a_raw_batch(L):
    from dmmfods_amd.prepare import BatchPrepare, collate_raw
    rng = np.random.default_rng(11)
    H, W = 60, 50
    frames = [_frame_small(rng, H, W, n, m) for n, m in ((40, 5), (0, 0), (25, 9))]
    raw = collate_raw(frames)
    for p, k in ((10, 5), (2, 7), (1, 1)):
        bp = BatchPrepare(pool=p, kernel_size=k)
        image, lidar, heat = bp(raw)
        assert image.shape == (3, 3, H // p, W // p) and lidar.shape == (3, 1, H // p, W // p) and heat.shape == (3, 3, H // p, W // p)
        assert image.data_ptr() + 4 * 3 * (H // p) * (W // p) == lidar.data_ptr() and image.stride(0) == 7 * (H // p) * (W // p)    # views of one batch
        want = R.batch(raw.image.numpy(), raw.points.numpy(), raw.point_offsets.numpy(), raw.boxes.numpy(), raw.box_offsets.numpy(), p, k)
        got = torch.cat([image, lidar, heat], dim=1).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (p, k)
        again = bp(raw)
        assert again[0].data_ptr() == image.data_ptr()                    # the output is cached per shape
        assert np.array_equal(_bits(torch.cat(again, dim=1).cpu().numpy()), _bits(want))
    pinned = collate_raw(frames, pin_memory=True)
    assert pinned.image.is_pinned() and pinned.points.is_pinned() and pinned.boxes.is_pinned()
    got = torch.cat(BatchPrepare(pool=10)(pinned), dim=1).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(R.batch(raw.image.numpy(), raw.points.numpy(), raw.point_offsets.numpy(), raw.boxes.numpy(),
                                                    raw.box_offsets.numpy(), 10, 5)))
    with pytest.raises(ValueError):
        BatchPrepare(pool=7)(raw)


def _frame_small(rng, H, W, npoints, nboxes):
    pts = np.stack([rng.uniform(-1, W + 2, npoints), rng.uniform(-1, H + 2, npoints), rng.uniform(0, 80, npoints)], axis=1).astype(F32)
    boxes = np.stack([rng.choice([1, 2, 4, 3], nboxes), rng.integers(-5, W, nboxes), rng.integers(-5, H, nboxes), rng.integers(0, 30, nboxes),
                      rng.integers(0, 30, nboxes)], axis=1).astype(np.int32).reshape(-1, 5)
    return dict(image=torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)), points=torch.from_numpy(pts), boxes=torch.from_numpy(boxes))


# ------------------------------------------------------------------------------------------------ the agent
class _Loader:
    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = batches[:1], 1


def _agent(tmp_path, monkeypatch, batches, raw_frames):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    if raw_frames is not None:
        cfg.loader.raw_frames = raw_frames

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        torch.manual_seed(1234)
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    agent = mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=True, compute_dtype="fp32", data_loader=_Loader(batches))
    agent.seen = {"forward": [], "loss_backward": [], "loss_metrics": []}
    model = agent.model
    fwd, lb, lm = model.forward, model.loss_backward, model.loss_metrics

    def forward(image, lidar):
        agent.seen["forward"].append((model.training, _bits(image.cpu().numpy()).copy(), _bits(lidar.cpu().numpy()).copy()))
        return fwd(image, lidar)

    def loss_backward(target):
        agent.seen["loss_backward"].append(_bits(target.cpu().numpy()).copy())
        return lb(target)

    def loss_metrics(logits, target):
        agent.seen["loss_metrics"].append(_bits(target.cpu().numpy()).copy())
        return lm(logits, target)
    model.forward, model.loss_backward, model.loss_metrics = forward, loss_backward, loss_metrics
    return agent


def test_agent_prepares_raw_frames_in_training_and_validation(L, tmp_path, monkeypatch):
    from dmmfods_amd.prepare import collate_raw
    rng = np.random.default_rng(21)
    H, W, p = 128, 192, 2
    raws = [collate_raw([_frame_small(rng, H, W, 300, 8) for _ in range(2)]) for _ in range(2)]
    wants = [R.batch(r.image.numpy(), r.points.numpy(), r.point_offsets.numpy(), r.boxes.numpy(), r.box_offsets.numpy(), p, 5) for r in raws]
    agent = _agent(tmp_path / "a", monkeypatch, raws, dict(pool=p))
    assert agent.prepare is not None and (agent.prepare.pool, agent.prepare.kernel_size) == (p, 5)
    agent.train_one_epoch()
    assert len(agent.seen["forward"]) == 2 and len(agent.seen["loss_backward"]) == 2
    for k in range(2):
        training, image, lidar = agent.seen["forward"][k]
        assert training and image.shape == (2, 3, H // p, W // p)
        assert np.array_equal(np.concatenate([image, lidar, agent.seen["loss_backward"][k]], axis=1), _bits(wants[k])), k
    with torch.no_grad():
        agent.validate()
    training, image, lidar = agent.seen["forward"][-1]
    assert not training and np.array_equal(np.concatenate([image, lidar, agent.seen["loss_metrics"][-1]], axis=1), _bits(wants[0]))
    agent.model.close()

    # the same frames prepared on the host and fed through the reference's loader path: without the field none of the new entry points
    # is called, and a fresh model of the same seed validates to the same numbers on the same bits
    def forbidden(*a, **k):
        raise AssertionError("a dmm_prep_* entry point was called without loader.raw_frames")
    for sym in ("dmm_prep_image", "dmm_prep_lidar", "dmm_prep_lidar_workspace", "dmm_prep_heat_maps"):
        monkeypatch.setattr(L.lib(), sym, forbidden, raising=True)
    tensors = [tuple(torch.from_numpy(w[:, a:b].copy()) for a, b in ((0, 3), (3, 4), (4, 7))) for w in wants]
    plain = _agent(tmp_path / "b", monkeypatch, tensors, None)
    assert plain.prepare is None
    with torch.no_grad():
        iou_plain = plain.validate()
    plain.train_one_epoch()
    training, image, lidar = plain.seen["forward"][-1]
    assert np.array_equal(np.concatenate([image, lidar, plain.seen["loss_backward"][-1]], axis=1), _bits(wants[1]))
    plain.save_checkpoint(is_best=True)
    ck = torch.load(os.path.join(plain.config.dir.current_run.checkpoints, plain.config.agent.best_checkpoint_name), map_location="cpu")
    assert set(ck) == {"epoch", "train_iteration", "val_iteration", "best_val_iou", "state_dict", "optimizer"}
    plain.model.close()
    monkeypatch.undo()
    fresh = _agent(tmp_path / "c", monkeypatch, raws, dict(pool=p))
    with torch.no_grad():
        iou_raw = fresh.validate()
    # (the per-class IoU, from which best_val_iou is formed, stands on integer counts; the loss is a float sum whose order is not fixed)
    assert iou_raw == iou_plain and sum(iou_raw) > 0
    fresh.model.close()
