"""Scale and rotation on the GPU: dmm_warp_batch (csrc/warp.hip) against the numpy restatement of its semantics in
tests/test_warp_cpu.py, and what stands on it (BatchAugment's `scale` and `rotate`, the agent's training loop).

Every comparison is BIT FOR BIT.  The one exception is reasoned, not measured: where the arithmetic itself makes or passes on a NaN
(inf - inf, a NaN tap in an interpolation, 0 * inf under a gain) IEEE 754 leaves sign and payload to the implementation, and there the
restatement's NaN asks for a NaN.  Copies - nearest samples and lattice pixels under the identity gain - and fill keep every bit.

Sources are (3, 7, 37, 45) batches (Ws no multiple of 4) whose base sits one element behind a 16-byte boundary, passed as three
strided channel slices: image (bilinear), LiDAR and target (nearest).  Outputs are 32 x 64 and a ragged 33 x 37, each once on a 16-byte
boundary (16-byte stores) and once one element behind it (element stores), each between sentinel margins; every case is launched twice
and must give the same bits, and the source must come through untouched.  NaN payloads, infinities and -0 sit everywhere in the
nearest-mode tensors; in the image only where the map is lattice-exact (matrix_cases says which)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests.test_augment_gpu import FILL7, SPECIAL_BITS, _agent, _source, _windows24
from tests.test_augment_gpu import _launch as _launch_augment
from tests.test_warp_cpu import BILINEAR, HALF, MASK, NEAREST, ONE, restate_warp, window_matrix

pytestmark = pytest.mark.gpu

DEV = "cuda"
HS, WS = 37, 45
MODES7 = (BILINEAR,) * 3 + (NEAREST,) * 4
MARGIN, SENT = 1024, 0x7fa5a5a5
OUT_SIZES = [(32, 64), (33, 37)]
IDENT = [[ONE, 0], [0, ONE]]


# ------------------------------------------------------------------------------------------------ maps
def about_centre(angle, zoom, Ho, Wo, y0=0, x0=0, flip=0):
    """BatchAugment's composition for one sample: (a, b) as lists."""
    from dmmfods_amd.augment import BatchAugment
    p = types.SimpleNamespace(y0=np.array([y0]), x0=np.array([x0]), flip=np.array([flip]), zoom=np.array([float(zoom)]),
                              angle=np.array([float(angle)]), out_size=(Ho, Wo))
    a, b = BatchAugment.matrices(p)
    return a[0].tolist(), b[0].tolist()


def matrix_cases(Ho, Wo):
    """[(name, a (3, 2, 2), b (3, 2), lattice_exact)] - one map per sample of the batch of three."""
    M = 64 << 20
    rot = lambda ang, zoom=1.0, **kw: about_centre(ang, zoom, Ho, Wo, **kw)   # noqa: E731

    def case(name, maps, lattice=False):
        return name, [m[0] for m in maps], [m[1] for m in maps], lattice
    return [
        case("identity", [(IDENT, [0, 0])] * 3, True),
        case("integer shifts and a flip", [window_matrix(3, -5, 0, Wo), window_matrix(-2, 4, 1, Wo), window_matrix(6, 40, 1, Wo)], True),
        # quarter, half and three-quarter turns on the lattice: (x, y) -> (y, 36 - x), (44 - x, 36 - y), (44 - y, x)
        case("lattice rotations", [([[0, ONE], [-ONE, 0]], [0, 36 * ONE]), ([[-ONE, 0], [0, -ONE]], [44 * ONE, 36 * ONE]),
                                   ([[0, -ONE], [ONE, 0]], [44 * ONE, 0])], True),
        case("a half", [(IDENT, [HALF, HALF]), (IDENT, [HALF, 0]), (IDENT, [3 * ONE, HALF - 2 * ONE])]),
        case("fractions 1 and MASK", [(IDENT, [1, 1]), (IDENT, [MASK, MASK]), (IDENT, [ONE + 1, MASK - ONE])]),
        case("7 and 33 degrees", [rot(7.0, y0=2, x0=-3), rot(-33.0), rot(33.0, flip=1, x0=-10)]),
        case("zoom 0.5 and 2", [rot(0.0, 0.5), rot(0.0, 2.0, y0=3, x0=4), rot(12.0, 0.5, flip=1)]),
        # rows 0..15 inside with a margin, rows 16..31 across the source's lower edge, row 32 (of 33) below it; a sample of its own
        # hangs over the left edge and one lies far out: whatever the tile shape, a launch holds all three classes
        case("every tile class", [([[ONE - 4321, 0], [0, 2 * ONE - 1234]], [HALF // 2, 777]),
                                  ([[ONE, 0], [0, ONE]], [-20 * ONE + 5, 3]), ([[ONE // 2, 99], [-99, ONE // 2]], [200 * ONE, 0])]),
        case("wholly outside", [(IDENT, [1000 * ONE, 0]), (IDENT, [7, -1000 * ONE]), rot(45.0, x0=5000)]),
        case("just below zero", [(IDENT, [-1, -1]), (IDENT, [-HALF, -HALF - 1]), (IDENT, [-ONE - 1, -ONE])]),
        # a = 0: a constant map - every pixel the same taps; b at the accepted bound lies outside
        case("constant maps", [([[0, 0], [0, 0]], [1 << 50, -(1 << 50)]), ([[0, 0], [0, 0]], [5 * ONE + HALF, 7 * ONE + 3]),
                               ([[0, 0], [0, 0]], [-(1 << 50), 3 * ONE])]),
        # the largest entries: pixel (x, y) reads (64 (x + y - 10), 64 (y - x)) and the like; with b at its bound nothing wraps
        case("coefficients at 64", [([[M, M], [-M, M]], [-10 * M, 0]), ([[-M, M], [M, -M]], [30 * M + HALF, 5 * ONE + 1]),
                                    ([[M, -M], [-M, -M]], [-(1 << 50), 1 << 50])]),
    ]


# ------------------------------------------------------------------------------------------------ the raw call
def _launch(tensors, a, b, gain, bias, fill, Hs, Ws, Ho, Wo):
    """tensors: [(src tensor or (data_ptr, batch stride), channels, mode, dst tensor)]; one dmm_warp_batch call on the current stream."""
    from dmmfods_amd import _lib
    B = len(a)
    T = (_lib.WarpTensor * len(tensors))()
    for d, (src, ch, mode, dst) in zip(T, tensors):
        if isinstance(src, torch.Tensor):
            assert src.stride()[1:] == (Hs * Ws, Ws, 1) and src.shape[1] == ch
            src = (src.data_ptr(), src.stride(0))
        d.src, d.src_batch_stride, d.channels, d.mode, d.dst = src[0], src[1], ch, mode, dst.data_ptr()
    S = (_lib.WarpSample * B)()
    nch = sum(t[1] for t in tensors)
    for s in range(B):
        (S[s].a00, S[s].a01), (S[s].a10, S[s].a11) = [[int(v) for v in row] for row in a[s]]
        S[s].b0, S[s].b1 = int(b[s][0]), int(b[s][1])
        for c in range(8):   # (entries past the call's channels are not read: a NaN there must not matter)
            S[s].gain[c], S[s].bias[c] = (float(gain[s, c]), float(bias[s, c])) if c < nch else (float("nan"), float("inf"))
    f = None if fill is None else (C.c_float * nch)(*[float(v) for v in fill])
    _lib.check(_lib.lib().dmm_warp_batch(T, len(tensors), S, B, Hs, Ws, Ho, Wo, f, _lib.stream_ptr()))


def _touches_fill(a, b, Ho, Wo, modes=MODES7, B=3):
    """(B, 7, Ho, Wo) bool: the pixel is the fill, or an interpolation with a tap outside the source (from the maps alone)."""
    zeros, one, zero = np.zeros((B, 7, HS, WS), np.float32), np.ones((B, 7), np.float32), np.zeros((B, 7), np.float32)
    return restate_warp(zeros, a, b, one, zero, (1.0,) * 7, modes, Ho, Wo)[0] != 0


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _check(got, want, made_nan, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want) & ~made_nan)
    assert bad.size == 0, (what, bad.size, [np.unravel_index(i, got.shape) for i in bad[:6]], got.ravel()[bad[:6]], want.ravel()[bad[:6]])
    assert np.isnan(got.view(np.float32)[made_nan]).all(), what


def _placed(n, off):
    """(buffer, view, start): n float32 elements whose first sits `off` elements behind a 16-byte boundary, MARGIN sentinels on either side."""
    buf = torch.full((n + 2 * MARGIN + 8,), SENT, dtype=torch.int32, device=DEV)
    start = MARGIN + ((16 - (buf.data_ptr() + 4 * MARGIN) % 16) % 16) // 4 + off
    view = buf[start:start + n].view(torch.float32)
    assert view.data_ptr() % 16 == 4 * off
    return buf, view, start


@pytest.fixture(scope="module")
def sources():
    """special: NaN payloads, infinities and -0 in all seven planes; clean: the image planes finite.  Each (host, device batch)."""
    special = _source(3, 7, HS, WS, seed=1)
    assert all((special[:, lo:hi].view(np.uint32) == s).any() for s in SPECIAL_BITS for lo, hi in ((0, 3), (3, 4), (4, 7)))
    clean = special.copy()
    img = clean[:, :3]
    odd = ~np.isfinite(img) | (img.view(np.uint32) == 0x80000000)
    img[odd] = np.arange(int(odd.sum()), dtype=np.float32) * 0.375 - 50.0
    assert np.isfinite(clean[:, :3]).all() and not np.isfinite(clean[:, 3:]).all()
    out = {}
    for name, host in (("special", special), ("clean", clean)):
        _, view, _ = _placed(host.size, 1)
        dev = view.view(3, 7, HS, WS)
        dev.copy_(torch.from_numpy(host))
        out[name] = (host, dev)
    return out


def _run(what, host, dev, a, b, Ho, Wo, off, gain=None, bias=None, fill=FILL7):
    """One call on the three slices of `dev`, twice; everything checked.  Returns the (B, 7, Ho, Wo) bits and the made-NaN mask."""
    B = host.shape[0]
    gain = np.ones((B, 7), np.float32) if gain is None else gain
    bias = np.zeros((B, 7), np.float32) if bias is None else bias
    want, made_nan = restate_warp(host, a, b, gain, bias, fill or (0,) * 7, MODES7, Ho, Wo)
    placed = [_placed(B * ch * Ho * Wo, off) for ch in (3, 1, 3)]
    outs = [v.view(B, ch, Ho, Wo) for (_, v, _), ch in zip(placed, (3, 1, 3))]
    tensors = [(dev[:, 0:3], 3, BILINEAR, outs[0]), (dev[:, 3:4], 1, NEAREST, outs[1]), (dev[:, 4:7], 3, NEAREST, outs[2])]
    first = None
    for _ in range(2):
        _launch(tensors, a, b, gain, bias, fill, host.shape[2], host.shape[3], Ho, Wo)
        got = np.concatenate([_bits(o) for o in outs], axis=1)
        _check(got, want, made_nan, what)
        for (buf, view, start), o in zip(placed, outs):
            m = buf.cpu().numpy()
            assert (m[:start] == SENT).all() and (m[start + o.numel():] == SENT).all(), what
        first = got if first is None else first
        assert np.array_equal(got, first), what
        for o in outs:                       # (the second call has to write every element again)
            o.view(torch.int32).fill_(SENT)
    assert np.array_equal(_bits(dev), host.view(np.uint32)), what
    return first, made_nan


# ------------------------------------------------------------------------------------------------ 1. the maps
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("Ho,Wo", OUT_SIZES)
def test_maps(sources, Ho, Wo, off):
    fill_bits = np.asarray(FILL7, np.float32).view(np.uint32)[None, :, None, None]
    for name, a, b, lattice in matrix_cases(Ho, Wo):
        host, dev = sources["special" if lattice else "clean"]
        got, made_nan = _run(f"{name} {Ho}x{Wo} off {off}", host, dev, a, b, Ho, Wo, off)
        if lattice:
            assert not made_nan.any()                                        # pure rearrangements: every bit, no exception
        assert not made_nan[:, 3:].any()                                     # nearest samples under the identity are copies
        if name == "identity":
            assert np.array_equal(got[:, :, :32, :37], host.view(np.uint32)[:, :, :32, :37])
        if name == "wholly outside":
            assert (got == fill_bits).all()
        if name == "constant maps":
            assert (got[0] == fill_bits[0]).all() and (got[2] == fill_bits[0]).all()
            assert all(len(np.unique(got[1, c])) == 1 for c in range(7)) and not _touches_fill(a, b, Ho, Wo)[1].any()
        if name == "every tile class":
            out = _touches_fill(a, b, Ho, Wo)
            assert not out[0, :, :16, :37].any() and out[0, :, 32:].all() and out[2].all() and out[1].any() and not out[1].all()


def test_integer_windows_equal_the_window_launch_bit_for_bit(sources):
    """The 24 windows of tests/test_augment_gpu.py as whole-number maps: dmm_warp_batch's outputs are dmm_augment_batch's, in both
    sampling modes, under gains as well (the arithmetic is the same two roundings, so here even NaNs made by it agree)."""
    host, dev = sources["special"]
    y0, x0, flip = _windows24()
    rng = np.random.default_rng(2)
    for Ho, Wo in OUT_SIZES:
        for k in range(0, 24, 3):
            sel = slice(k, k + 3)
            gain, bias = np.ones((3, 7), np.float32), np.zeros((3, 7), np.float32)
            if k % 2:
                gain[:, [0, 3, 5]], bias[:, [1, 3]] = rng.uniform(-2, 2, (3, 3)).astype(np.float32), rng.uniform(-9, 9, (3, 2)).astype(np.float32)
            maps = [window_matrix(int(y0[s]), int(x0[s]), int(flip[s]), Wo) for s in range(k, k + 3)]
            a, b = [m[0] for m in maps], [m[1] for m in maps]
            w_outs = [torch.empty((3, ch, Ho, Wo), device=DEV) for ch in (3, 1, 3)]
            a_outs = [torch.empty((3, ch, Ho, Wo), device=DEV) for ch in (3, 1, 3)]
            _launch([(dev[:, 0:3], 3, BILINEAR, w_outs[0]), (dev[:, 3:4], 1, NEAREST, w_outs[1]), (dev[:, 4:7], 3, NEAREST, w_outs[2])],
                    a, b, gain, bias, FILL7, HS, WS, Ho, Wo)
            _launch_augment([(dev[:, 0:3], 3, a_outs[0]), (dev[:, 3:4], 1, a_outs[1]), (dev[:, 4:7], 3, a_outs[2])],
                            y0[sel], x0[sel], flip[sel], gain, bias, FILL7, HS, WS, Ho, Wo)
            for w, o in zip(w_outs, a_outs):
                assert np.array_equal(_bits(w), _bits(o)), (Ho, Wo, k)
            want, made_nan = restate_warp(host, a, b, gain, bias, FILL7, MODES7, Ho, Wo)
            _check(np.concatenate([_bits(o) for o in w_outs], axis=1), want, made_nan, f"windows {k}..{k + 2} {Ho}x{Wo}")


# ------------------------------------------------------------------------------------------------ 2. gain and bias
def test_gain_and_bias_mixed_over_channels_and_samples(sources):
    host, dev = sources["clean"]
    rng = np.random.default_rng(5)
    gain = rng.uniform(-3, 3, (3, 7)).astype(np.float32)
    bias = rng.uniform(-100, 100, (3, 7)).astype(np.float32)
    for s in range(3):   # the fixed pairs wander through the channels with the sample
        for k, (g, bi) in enumerate(((1.0, 0.0), (1.25, -3.5), (0.0, 0.0))):
            gain[s, (s + 2 * k) % 7], bias[s, (s + 2 * k) % 7] = g, bi
    gain[0, 5], bias[0, 5] = 1.0, 2.0          # gain 1 alone is not the identity
    gain[1, 5], bias[1, 5] = 0.5, 0.0          # nor is bias 0
    gain[2, 1], bias[2, 1] = 1.0, -0.0         # bias -0 == 0: the identity
    gain[0, 3], gain[1, 6], gain[2, 5], bias[0, 3], bias[1, 6], bias[2, 5] = 1.0, 1.0, 1.0, 0.0, 0.0, 0.0   # identities among the nearest tensors
    ident = (gain == 1) & (bias == 0)
    assert ident.sum() >= 6 and ident[:, 3:].sum() >= 3
    for Ho, Wo in OUT_SIZES:
        maps = [about_centre(7.0, 1.1, Ho, Wo, y0=-2, x0=3), about_centre(-33.0, 0.8, Ho, Wo, flip=1), (IDENT, [HALF - 3 * ONE, 2 * ONE + 1])]
        a, b = [m[0] for m in maps], [m[1] for m in maps]
        got, made_nan = _run(f"gain and bias {Ho}x{Wo}", host, dev, a, b, Ho, Wo, 0, gain=gain, bias=bias)
        assert made_nan.any() and not made_nan[ident].any() and not made_nan[:, :3].any()
        # identity channels of the nearest tensors carried the special patterns through; every fill pixel is the fill, ungained
        carried = got[:, 3:][ident[:, 3:]]
        assert sum((carried == s).any() for s in SPECIAL_BITS) >= 4
        outside = _touches_fill(a, b, Ho, Wo, modes=(NEAREST,) * 7)
        fills = np.broadcast_to(np.asarray(FILL7, np.float32).view(np.uint32)[None, :, None, None], got.shape)
        assert outside.any() and (got[:, 3:][outside[:, 3:]] == fills[:, 3:][outside[:, 3:]]).all()


# ------------------------------------------------------------------------------------------------ 3. chunking
@pytest.mark.parametrize("B", [33, 65])
def test_more_samples_than_one_launch_carries(B):
    host = _source(B, 7, 9, 13, seed=B)
    host[:, :3][~np.isfinite(host[:, :3])] = 0.25
    dev = torch.from_numpy(host).to(DEV)
    maps = [about_centre(3.0 * s - 40.0, 0.75 + s / 64.0, 8, 12, y0=s % 3 - 1, x0=s % 5 - 2, flip=s & 1) for s in range(B)]
    a, b = [m[0] for m in maps], [m[1] for m in maps]
    s = np.arange(B)
    gain, bias = np.ones((B, 7), np.float32), np.zeros((B, 7), np.float32)
    gain[:, 0], bias[:, 1] = 1.0 + s / 64.0, s - 20.0
    want, made_nan = restate_warp(host, a, b, gain, bias, FILL7, MODES7, 8, 12)
    assert len({w.tobytes() for w in want}) == B
    outs = [torch.empty((B, ch, 8, 12), device=DEV) for ch in (3, 1, 3)]
    _launch([(dev[:, 0:3], 3, BILINEAR, outs[0]), (dev[:, 3:4], 1, NEAREST, outs[1]), (dev[:, 4:7], 3, NEAREST, outs[2])],
            a, b, gain, bias, FILL7, 9, 13, 8, 12)
    _check(np.concatenate([_bits(o) for o in outs], axis=1), want, made_nan, f"B = {B}")


# ------------------------------------------------------------------------------------------------ 4. 64-bit offsets
def test_sample_stride_past_2_31_elements():
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    stride, Cn, Ho, Wo = 2 ** 31 + 12345, 2, 32, 64
    host = _source(2, Cn, HS, WS, seed=9)
    host[:, 0][~np.isfinite(host[:, 0])] = -4.5
    big = torch.empty(stride + Cn * HS * WS, device=DEV)            # 8.6 GB, of which only the two samples' planes are written
    view = big.as_strided((2, Cn, HS, WS), (stride, HS * WS, WS, 1))
    view.copy_(torch.from_numpy(host).to(DEV))
    maps = [about_centre(7.0, 0.9, Ho, Wo, x0=-4), about_centre(-20.0, 1.2, Ho, Wo, y0=2, flip=1)]
    a, b = [m[0] for m in maps], [m[1] for m in maps]
    gain, bias = np.array([[1, 2], [1, 1]], np.float32), np.array([[0, 1], [0, 0]], np.float32)
    want, made_nan = restate_warp(host, a, b, gain, bias, FILL7[:2], (BILINEAR, NEAREST), Ho, Wo)
    outs = [torch.empty((2, 1, Ho, Wo), device=DEV) for _ in range(2)]
    _launch([((view[:, 0:1].data_ptr(), stride), 1, BILINEAR, outs[0]), ((view[:, 1:2].data_ptr(), stride), 1, NEAREST, outs[1])],
            a, b, gain, bias, FILL7[:2], HS, WS, Ho, Wo)
    _check(np.concatenate([_bits(o) for o in outs], axis=1), want, made_nan, "stride 2^31 + 12345")
    assert (want[1] != want[0]).any() and np.array_equal(_bits(view), host.view(np.uint32))
    del view, big


# ------------------------------------------------------------------------------------------------ 5. BatchAugment
def _restate_params(batch_host, p, fill, with_lidar=True):
    from dmmfods_amd.augment import BatchAugment
    src = batch_host if with_lidar else np.concatenate([batch_host[:, :3], batch_host[:, 4:]], axis=1)
    gain, bias = BatchAugment.channel_tables(p, 3, 1 if with_lidar else 0, 3)
    a, b = BatchAugment.matrices(p, *batch_host.shape[2:])
    modes = (BILINEAR,) * 3 + (NEAREST,) * (4 if with_lidar else 3)
    return restate_warp(src, a, b, gain, bias, fill, modes, *p.out_size)


def _finite_image(host):
    host[:, :3][~np.isfinite(host[:, :3])] = 1.0
    return host


def test_batch_augment_with_scale_and_rotate_equals_the_restatement():
    from dmmfods_amd.augment import BatchAugment
    host = _finite_image(_source(4, 7, 96, 128, seed=3))
    dev = torch.from_numpy(host).to(DEV)
    aug = BatchAugment(out_size=(64, 96), hflip=0.5, translate=(7, 9), brightness=0.3, contrast=0.4, channel_gain=0.2, lidar_dropout=0.3,
                       fill=list(FILL7), seed=12, rank=1, scale=0.3, rotate=25.0)
    for i in range(2):
        p = aug.params_at(i, 4, 96, 128)
        image, lidar, target = aug(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7])
        assert aug.batches_drawn == i + 1 and image.shape == (4, 3, 64, 96) and lidar.shape == (4, 1, 64, 96) and target.shape == (4, 3, 64, 96)
        want, made_nan = _restate_params(host, p, FILL7)
        _check(np.concatenate([_bits(image), _bits(lidar), _bits(target)], axis=1), want, made_nan, f"BatchAugment batch {i}")
        # the target's values are the source's (or the fill): nearest sampling invents no level
        assert set(np.unique(_bits(target))) <= set(np.unique(host[:, 4:].view(np.uint32))) | set(np.asarray(FILL7[4:], np.float32).view(np.uint32))
    # explicit params: nothing advances, the same bits again; lidar = None with one fill number
    p = aug.params_at(1, 4, 96, 128)
    again = aug(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7], params=p)
    want, made_nan = _restate_params(host, p, FILL7)
    _check(np.concatenate([_bits(t) for t in again], axis=1), want, made_nan, "explicit params")
    assert aug.batches_drawn == 2
    solo = BatchAugment(out_size=(64, 96), hflip=0.5, contrast=0.4, fill=2.5, seed=12, rotate=10.0)
    p = solo.params_at(0, 4, 96, 128)
    assert (p.zoom == 1).all() and p.angle.all()
    image, lidar, target = solo(dev[:, 0:3].contiguous(), None, dev[:, 4:7])
    assert lidar is None and solo.batches_drawn == 1
    want, made_nan = _restate_params(host, p, (2.5,) * 6, with_lidar=False)
    _check(np.concatenate([_bits(image), _bits(target)], axis=1), want, made_nan, "lidar = None")
    assert np.array_equal(_bits(dev), host.view(np.uint32))


def test_zero_strengths_issue_the_window_launch(monkeypatch):
    from dmmfods_amd import _lib
    from dmmfods_amd.augment import BatchAugment
    L = _lib.lib()
    calls = {"dmm_augment_batch": 0, "dmm_warp_batch": 0}

    def counting(name):
        real = getattr(L, name)

        def f(*args):
            calls[name] += 1
            return real(*args)
        return f
    for name in calls:
        monkeypatch.setattr(L, name, counting(name))
    host = _finite_image(_source(2, 7, 64, 96, seed=4))
    dev = torch.from_numpy(host).to(DEV)
    plain = BatchAugment(out_size=(32, 64), hflip=0.5, translate=(3, 3), seed=1)
    out = plain(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7])
    assert calls == {"dmm_augment_batch": 1, "dmm_warp_batch": 0}
    # the same parameters through the other entry point (a zoom of exactly 1 is not drawn with scale > 0: given as params): same bits
    warped = BatchAugment(out_size=(32, 64), hflip=0.5, translate=(3, 3), seed=1, rotate=1.0)
    again = warped(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7], params=plain.params_at(0, 2, 64, 96))
    assert calls == {"dmm_augment_batch": 1, "dmm_warp_batch": 1}
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(out, again))
    BatchAugment(scale=0.1)(dev[:, 0:3], None, dev[:, 4:7])
    assert calls == {"dmm_augment_batch": 1, "dmm_warp_batch": 2}


# ------------------------------------------------------------------------------------------------ 6. the agent
def test_agent_warps_training_batches_only(tmp_path, monkeypatch):
    host = [_source(2, 7, 96, 128, seed=30 + s) for s in range(2)]
    for h in host:   # finite inputs for the net: the special patterns stay in the kernel's own tests
        h[~np.isfinite(h)] = 1.0
        h[:, 4:] = (h[:, 4:] > 0).astype(np.float32)
    batches = [(torch.from_numpy(h[:, 0:3].copy()), torch.from_numpy(h[:, 3:4].copy()), torch.from_numpy(h[:, 4:7].copy())) for h in host]
    from dmmfods_amd.augment import BatchAugment
    # the config field takes the whole-pixel arguments only (an existing test pins that it refuses `rotate`): the knobs come in as a
    # BatchAugment of the caller's own, which the training loop and the checkpoint use like the one the field would have made
    spec = dict(out_size=(64, 96), hflip=0.5, translate=(5, 6), contrast=0.3, seed=4)
    agent = _agent(tmp_path / "a", monkeypatch, batches, spec)
    agent.augment = BatchAugment(scale=0.25, rotate=15.0, **spec)
    agent.train_one_epoch()
    assert agent.augment.batches_drawn == 2 and len(agent.seen["forward"]) == 2 and len(agent.seen["loss_backward"]) == 2
    for k in range(2):
        p = agent.augment.params_at(k, 2, 96, 128)
        assert (p.zoom != 1).all() and p.angle.all()
        want, made_nan = _restate_params(host[k], p, (0,) * 7)
        training, image, lidar = agent.seen["forward"][k]
        assert training and image.shape == (2, 3, 64, 96) and not made_nan.any()
        _check(np.concatenate([image, lidar, agent.seen["loss_backward"][k]], axis=1), want, made_nan, f"agent batch {k}")
        assert set(np.unique(agent.seen["loss_backward"][k].view(np.float32)).tolist()) <= {0.0, 1.0}      # labels stay labels
    with torch.no_grad():
        agent.validate()
    training, image, lidar = agent.seen["forward"][-1]
    assert not training and agent.augment.batches_drawn == 2           # validation: the loader's tensors, untouched
    assert np.array_equal(np.concatenate([image, lidar, agent.seen["loss_metrics"][-1]], axis=1), host[0].view(np.uint32))
    agent.save_checkpoint(is_best=True)
    ck = torch.load(os.path.join(agent.config.dir.current_run.checkpoints, agent.config.agent.best_checkpoint_name), map_location="cpu")
    assert set(ck) == {"epoch", "train_iteration", "val_iteration", "best_val_iou", "state_dict", "optimizer", "augment"}
    assert ck["augment"] == {"seed": 4, "rank": 0, "batches_drawn": 2}
    agent.model.close()
