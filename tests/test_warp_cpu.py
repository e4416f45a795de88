"""Scale and rotation on the device (dmm_warp_batch, csrc/warp.hip; BatchAugment's `scale` and `rotate`) as far as it goes without a
GPU: the symbol, the struct layouts against a compiled C probe, every refusal of the entry point before it touches HIP, BatchAugment's
two new knobs - with the parameters of existing configurations pinned to what the commit before the knobs drew - the numpy
restatement of the semantics (which tests/test_warp_gpu.py imports) on hand-computed cases, and the sanitizer harness
(DRIVE_WARP=1: one valid call of 33 samples - two launches - and every refusal, stand-alone under ASan + UBSan).

THE RESTATEMENT.  F = 20, ONE = 1 << F, HALF = ONE / 2, MASK = ONE - 1.  For sample b, channel c, output pixel (x, y), in integers:
    SX = a00 x + a01 y + b0        SY = a10 x + a11 y + b1
  nearest:   (sx, sy) = ((SX + HALF) >> F, (SY + HALF) >> F) (floors).  Inside the source: v = src[sy][sx], out = v where gain == 1 and
             bias == 0, else fl(fl(gain * v) + bias).  Outside: fill[c].
  bilinear:  (x0, y0) = (SX >> F, SY >> F), (fx, fy) = (SX & MASK, SY & MASK), wx = fl(fx) * 2^-F, wy likewise (exact).  A tap outside the
             source has the value fill[c].  fx == fy == 0: tap 00 alone, as nearest at (x0, y0).  No tap inside: fill[c].  Otherwise
             top = fl(v00 + fl(wx * fl(v01 - v00))), bot = fl(v10 + fl(wx * fl(v11 - v10))), v = fl(top + fl(wy * fl(bot - top))), then the
             gain / bias rule on v."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 20
ONE = 1 << F
HALF, MASK = ONE >> 1, ONE - 1
NEAREST, BILINEAR = 0, 1


# ------------------------------------------------------------------------------------------------ the restatement
def _gain_rule(v, g, bi):
    """v float32 array -> (uint32 bits, mask of NaNs the arithmetic made or passed on)."""
    if g == 1 and bi == 0:
        return v.view(np.uint32), np.zeros(v.shape, dtype=bool)
    with np.errstate(all="ignore"):
        w = (g * v).astype(np.float32) + bi
    assert w.dtype == np.float32
    return w.view(np.uint32), np.isnan(w)


def restate_warp(src, a, b, gain, bias, fill, modes, Ho, Wo):
    """src (B, C, Hs, Ws) float32; a (B, 2, 2) and b (B, 2) integers in Q20; gain, bias (B, C); fill, modes (C,).  Returns the uint32 bits
    of the (B, C, Ho, Wo) output and the mask of elements whose value is a NaN that the ARITHMETIC made or passed on (an interpolation,
    or a gain other than the identity): there IEEE 754 leaves sign and payload to the implementation, and only "is a NaN" is asked."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    B, Cn, Hs, Ws = src.shape
    out = np.empty((B, Cn, Ho, Wo), dtype=np.uint32)
    made_nan = np.zeros((B, Cn, Ho, Wo), dtype=bool)
    fill = np.asarray(fill, dtype=np.float32)
    fill_bits = fill.view(np.uint32)
    ys, xs = np.arange(Ho, dtype=np.int64)[:, None], np.arange(Wo, dtype=np.int64)[None, :]
    scale = np.float32(2.0 ** -F)

    def tap(plane, tx, ty, fillv):
        inside = (tx >= 0) & (tx < Ws) & (ty >= 0) & (ty < Hs)
        return np.where(inside, plane[np.clip(ty, 0, Hs - 1), np.clip(tx, 0, Ws - 1)], fillv).astype(np.float32), inside

    for s in range(B):
        (a00, a01), (a10, a11) = [[int(v) for v in row] for row in np.asarray(a[s]).tolist()]
        b0, b1 = int(b[s][0]), int(b[s][1])
        assert max(abs(a00), abs(a01), abs(a10), abs(a11)) <= 64 << F and max(abs(b0), abs(b1)) <= 1 << 50   # (so int64 is exact)
        SX, SY = a00 * xs + a01 * ys + b0, a10 * xs + a11 * ys + b1
        for c in range(Cn):
            g, bi = np.float32(gain[s, c]), np.float32(bias[s, c])
            if modes[c] == NEAREST:
                v, inside = tap(src[s, c], (SX + HALF) >> F, (SY + HALF) >> F, fill[c])
                val, nan = _gain_rule(v, g, bi)
                out[s, c], made_nan[s, c] = np.where(inside, val, fill_bits[c]), inside & nan
                continue
            x0, y0, fx, fy = SX >> F, SY >> F, SX & MASK, SY & MASK
            wx, wy = fx.astype(np.float32) * scale, fy.astype(np.float32) * scale
            assert np.array_equal(wx.astype(np.float64) * ONE, fx) and np.array_equal(wy.astype(np.float64) * ONE, fy)   # exact
            (v00, i00), (v01, i01) = tap(src[s, c], x0, y0, fill[c]), tap(src[s, c], x0 + 1, y0, fill[c])
            (v10, i10), (v11, i11) = tap(src[s, c], x0, y0 + 1, fill[c]), tap(src[s, c], x0 + 1, y0 + 1, fill[c])
            with np.errstate(all="ignore"):
                top = v00 + (wx * (v01 - v00)).astype(np.float32)
                bot = v10 + (wx * (v11 - v10)).astype(np.float32)
                v = top + (wy * (bot - top)).astype(np.float32)
            assert v.dtype == top.dtype == np.float32
            on_lattice = (fx == 0) & (fy == 0)
            copied, nan_c = _gain_rule(v00, g, bi)
            mixed, nan_m = _gain_rule(v, g, bi)
            any_in = i00 | i01 | i10 | i11
            out[s, c] = np.where(on_lattice, np.where(i00, copied, fill_bits[c]), np.where(any_in, mixed, fill_bits[c]))
            made_nan[s, c] = np.where(on_lattice, i00 & nan_c, any_in & (nan_m | np.isnan(v)))
    return out, made_nan


def window_matrix(y0, x0, flip, Wo):
    """The whole-number map of dmm_augment_batch's window (y0, x0, flip): (a (2, 2), b (2,)) in Q20."""
    return ([[-ONE if flip else ONE, 0], [0, ONE]], [(x0 + Wo - 1 if flip else x0) * ONE, y0 * ONE])


def _bits(vals):
    return np.asarray(vals, dtype=np.float32).view(np.uint32)


def test_restatement_half_pixel_shift_averages_neighbours():
    src = np.array([[1, 2, 4], [8, 16, 32], [64, 128, 256]], dtype=np.float32)[None, None]
    one, zero = np.ones((1, 1), np.float32), np.zeros((1, 1), np.float32)
    out, nan = restate_warp(src, [[[ONE, 0], [0, ONE]]], [[HALF, 0]], one, zero, [-7.0], [BILINEAR], 3, 3)
    # (x + 1/2, y): the mean of horizontal neighbours; the last column's right tap is the fill, -7
    assert not nan.any() and np.array_equal(out[0, 0], _bits([[1.5, 3, -1.5], [12, 24, 12.5], [96, 192, 124.5]]))
    out, _ = restate_warp(src, [[[ONE, 0], [0, ONE]]], [[HALF, HALF]], one, zero, [0.0], [BILINEAR], 2, 2)
    assert np.array_equal(out[0, 0], _bits([[6.75, 13.5], [54, 108]]))                     # the mean of four
    out, _ = restate_warp(src, [[[ONE, 0], [0, ONE]]], [[ONE // 4, 0]], one * 2, one, [0.0], [BILINEAR], 1, 2)
    assert np.array_equal(out[0, 0], _bits([[2 * 1.25 + 1, 2 * 2.5 + 1]]))                 # weights 3/4, 1/4; then gain 2, bias 1
    # nearest at the same half: a half rounds up, to the right-hand neighbour; past the edge the fill
    out, _ = restate_warp(src, [[[ONE, 0], [0, ONE]]], [[HALF, 0]], one, zero, [-7.0], [NEAREST], 3, 3)
    assert np.array_equal(out[0, 0], _bits([[2, 4, -7], [16, 32, -7], [128, 256, -7]]))
    out, _ = restate_warp(src, [[[ONE, 0], [0, ONE]]], [[HALF - 1, 0]], one, zero, [-7.0], [NEAREST], 3, 3)
    assert np.array_equal(out[0, 0], src[0, 0].view(np.uint32))                            # one unit below the half: stays


def test_restatement_lattice_rotation_copies_bits():
    src = np.arange(9, dtype=np.float32).reshape(1, 1, 3, 3)
    src.view(np.uint32)[0, 0, 0, 1], src.view(np.uint32)[0, 0, 1, 1], src.view(np.uint32)[0, 0, 2, 0] = 0x7fc12345, 0x80000000, 0xff800000
    one, zero = np.ones((1, 2), np.float32), np.zeros((1, 2), np.float32)
    two = np.concatenate([src, src], axis=1)
    # a quarter turn: (x, y) -> (y, 2 - x), i.e. out[y][x] = src[2 - x][y]; both modes, bit for bit (a NaN payload, -0, -inf included)
    out, nan = restate_warp(two, [[[0, ONE], [-ONE, 0]]], [[0, 2 * ONE]], one, zero, [5.0, 5.0], [NEAREST, BILINEAR], 3, 3)
    want = np.array([[src.view(np.uint32)[0, 0, 2 - x, y] for x in range(3)] for y in range(3)])
    assert not nan.any() and np.array_equal(out[0, 0], want) and np.array_equal(out[0, 1], want)
    assert np.array_equal(want, np.rot90(src[0, 0].view(np.uint32), -1))
    # a half turn
    out, nan = restate_warp(two, [[[-ONE, 0], [0, -ONE]]], [[2 * ONE, 2 * ONE]], one, zero, [5.0, 5.0], [NEAREST, BILINEAR], 3, 3)
    assert not nan.any() and np.array_equal(out[0, 0], src[0, 0, ::-1, ::-1].view(np.uint32)) and np.array_equal(out[0, 1], out[0, 0])
    # the window map: a mirrored window one column to the left, its overhang the fill
    a, b = window_matrix(0, -1, 1, 3)
    out, _ = restate_warp(two, [a], [b], one, zero, [5.0, 6.0], [NEAREST, BILINEAR], 3, 3)
    assert np.array_equal(out[0, 0, :, :2], src[0, 0, :, 1::-1].view(np.uint32)) and (out[0, 0, :, 2] == _bits(5.0)).all()
    assert np.array_equal(out[0, 1, :, :2], out[0, 0, :, :2]) and (out[0, 1, :, 2] == _bits(6.0)).all()


def test_restatement_negative_coordinates_floor():
    src = np.array([[1, 2, 4], [8, 16, 32], [64, 128, 256]], dtype=np.float32)[None, None]
    one, zero = np.ones((1, 1), np.float32), np.zeros((1, 1), np.float32)
    ident = [[[ONE, 0], [0, ONE]]]
    # SX = -1 (one unit below zero): x0 = -1, not 0; fx = MASK.  v = fill + (MASK / ONE) * (src - fill), nearly the source
    out, nan = restate_warp(src, ident, [[-1, 0]], one, zero, [0.0], [BILINEAR], 1, 1)
    w = np.float32(MASK) * np.float32(2.0 ** -F)
    assert not nan.any() and out[0, 0, 0, 0] == _bits(np.float32(w * np.float32(1.0))) and w < 1
    # a truncating shift would have read tap (0, 0) with weight ~1 on tap (1, 0): 2, not 1
    out, _ = restate_warp(src, ident, [[-HALF, 0]], one, zero, [3.0], [BILINEAR], 1, 2)
    assert np.array_equal(out[0, 0], _bits([[2.0, 1.5]]))                                   # (3 + 1) / 2, (1 + 2) / 2
    # nearest: -HALF rounds up to 0, one unit less to -1 (outside)
    out, _ = restate_warp(src, ident, [[-HALF, -HALF]], one, zero, [3.0], [NEAREST], 1, 1)
    assert out[0, 0, 0, 0] == _bits(1.0)
    out, _ = restate_warp(src, ident, [[-HALF - 1, 0]], one, zero, [3.0], [NEAREST], 1, 1)
    assert out[0, 0, 0, 0] == _bits(3.0)
    # all four taps outside: the fill, untouched by the gain; one tap inside: interpolated and gained
    out, _ = restate_warp(src, ident, [[-ONE - 1, HALF]], one * 2, zero, [3.0], [BILINEAR], 1, 1)
    assert out[0, 0, 0, 0] == _bits(3.0)
    out, _ = restate_warp(src, ident, [[-ONE, HALF]], one * 2, zero, [3.0], [BILINEAR], 1, 1)
    assert out[0, 0, 0, 0] == _bits(2 * (3 + 0.5 * (3 - 3)))                                # x0 = -1, fx = 0: taps (-1, 0), (-1, 1), both fill
    out, _ = restate_warp(src, ident, [[-HALF, HALF]], one * 2, zero, [3.0], [BILINEAR], 1, 1)
    assert out[0, 0, 0, 0] == _bits(2 * ((3 + 1) / 2 + 0.5 * ((3 + 8) / 2 - (3 + 1) / 2)))


# ------------------------------------------------------------------------------------------------ C entry point
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "dmmfods_hip.h")).read()
    assert "dmm_warp_batch(" in header and "dmm_warp_batch" in lib.EXPORTS and hasattr(lib.lib(), "dmm_warp_batch")
    for name, val in (("DMM_WARP_NEAREST", lib.WARP_NEAREST), ("DMM_WARP_BILINEAR", lib.WARP_BILINEAR), ("DMM_WARP_FRAC_BITS", lib.WARP_FRAC_BITS),
                      ("DMM_WARP_LAUNCH_BATCH", lib.WARP_LAUNCH_BATCH)):
        assert any(ln.split()[:3] == ["#define", name, str(val)] for ln in header.splitlines()), name
    assert (lib.WARP_NEAREST, lib.WARP_BILINEAR, lib.WARP_FRAC_BITS, lib.WARP_LAUNCH_BATCH) == (NEAREST, BILINEAR, F, 32)
    assert (lib.WARP_MAX_A, lib.WARP_MAX_B) == (64 << F, 1 << 50)
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T dmm_warp_batch\n" in nm


def test_struct_layouts_match_the_header(lib, tmp_path):
    fields_t = ("src", "dst", "src_batch_stride", "channels", "mode", "reserved")
    fields_s = ("a00", "a01", "a10", "a11", "b0", "b1", "gain", "bias")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmfods_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(dmm_warp_tensor));\n'
                   + "".join(f'  printf(" %zu", offsetof(dmm_warp_tensor, {f}));\n' for f in fields_t)
                   + '  printf(" %zu", sizeof(dmm_warp_sample));\n'
                   + "".join(f'  printf(" %zu", offsetof(dmm_warp_sample, {f}));\n' for f in fields_s)
                   + '  printf(" %d %lld %lld\\n", DMM_WARP_LAUNCH_BATCH, (long long)DMM_WARP_MAX_A, (long long)DMM_WARP_MAX_B);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = next(c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if subprocess.run(["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T, S = lib.WarpTensor, lib.WarpSample
    mine = [C.sizeof(T)] + [getattr(T, f).offset for f in fields_t] + [C.sizeof(S)] + [getattr(S, f).offset for f in fields_s]
    assert got[:-3] == mine == [40, 0, 8, 16, 24, 28, 32, 96, 0, 4, 8, 12, 16, 24, 32, 64]
    assert got[-3:] == [lib.WARP_LAUNCH_BATCH, lib.WARP_MAX_A, lib.WARP_MAX_B]
    # the launch batch is the largest power of two whose records fit the 4 KB argument block beside the 344 bytes of everything else
    assert 344 + 32 * C.sizeof(S) <= 4096 < 344 + 64 * C.sizeof(S)


def _call(lib, B=3, Hs=16, Ws=24, Ho=16, Wo=24, ntensors=2, fill=(0.5,) * 8, tweak_tensor=None, tweak_sample=None, null_tensors=False,
          null_samples=False):
    """A call on addresses nothing dereferences (only the structures and `fill` are host memory the checks read)."""
    src, dst = 0x10000000, 0x20000000
    T = (lib.WarpTensor * 4)()
    for t in range(4):   # 2 channels each, slices of one (B, 8, Hs, Ws) batch
        T[t].src, T[t].dst, T[t].src_batch_stride, T[t].channels = src + t * 2 * Hs * Ws * 4, dst + t * B * 2 * Ho * Wo * 4, 8 * Hs * Ws, 2
        T[t].mode = t & 1
    S = (lib.WarpSample * max(B, 1))()
    for b in range(max(B, 1)):
        S[b].a00, S[b].a01, S[b].a10, S[b].a11, S[b].b0, S[b].b1 = ONE + b, -b, b, ONE - b, (b - 1) * ONE + 5, (1 - b) * ONE
        for c in range(8):
            S[b].gain[c], S[b].bias[c] = 1.0 + c, float(-c)
    if tweak_tensor:
        tweak_tensor(T)
    if tweak_sample:
        tweak_sample(S)
    f = None if fill is None else (C.c_float * 8)(*fill)
    return lib.lib().dmm_warp_batch(None if null_tensors else T, ntensors, None if null_samples else S, B, Hs, Ws, Ho, Wo, f, None)


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    """Every refusal the header lists, on a machine without a device: a call that got past the checks would reach the runtime."""
    nan, inf = float("nan"), float("inf")

    def tt(t, **kw):
        def f(T):
            for k, v in kw.items():
                if k == "reserved":
                    T[t].reserved[v[0]] = v[1]
                else:
                    setattr(T[t], k, v)
        return dict(tweak_tensor=f)

    def ss(b, c=None, **kw):
        def f(S):
            for k, v in kw.items():
                if c is None:
                    setattr(S[b], k, v)
                else:
                    getattr(S[b], k)[c] = v
        return dict(tweak_sample=f)

    plane = 16 * 24
    amax, bmax = 64 << F, 1 << 50
    cases = [
        (dict(null_tensors=True), b"null"), (dict(null_samples=True), b"null"),
        (tt(1, src=None), b"null src or dst"), (tt(0, dst=None), b"null src or dst"),
        (dict(ntensors=0), b"ntensors"), (dict(ntensors=5), b"ntensors"), (dict(ntensors=-1), b"ntensors"),
        (tt(1, channels=0), b"channels must be >= 1"), (tt(0, channels=-2), b"channels must be >= 1"),
        (dict(ntensors=4, **tt(3, channels=3)), b"sum to at most 8"), (tt(0, channels=9), b"sum to at most 8"),
        (dict(B=0), b">= 1"), (dict(Hs=0), b">= 1"), (dict(Ws=-3), b">= 1"), (dict(Ho=0), b">= 1"), (dict(Wo=0), b">= 1"),
        (dict(B=1, Hs=65536, Ws=32768), b"Hs * Ws"), (dict(B=1, Ho=32768, Wo=65536), b"Ho * Wo"),
        (tt(0, src_batch_stride=2 * plane - 1), b"src_batch_stride"), (tt(1, src_batch_stride=0), b"src_batch_stride"),
        (tt(1, src=0x10000000 + 2), b"4-byte aligned"), (tt(0, dst=0x20000000 + 1), b"4-byte aligned"),
        (tt(1, reserved=(0, 1)), b"reserved"), (tt(0, reserved=(1, -1)), b"reserved"),
        (tt(0, mode=2), b"mode"), (tt(1, mode=-1), b"mode"),
        (ss(1, a00=amax + 1), b"64 << 20"), (ss(2, a01=-amax - 1), b"64 << 20"), (ss(0, a10=amax + 1), b"64 << 20"), (ss(1, a11=-2 ** 31), b"64 << 20"),
        (ss(0, b0=bmax + 1), b"2^50"), (ss(2, b0=-bmax - 1), b"2^50"), (ss(1, b1=bmax + 1), b"2^50"), (ss(0, b1=-2 ** 63), b"2^50"),
        (ss(0, 0, gain=nan), b"NaN or infinite"), (ss(2, 3, gain=inf), b"NaN or infinite"), (ss(1, 1, bias=nan), b"NaN or infinite"),
        (ss(2, 2, bias=-inf), b"NaN or infinite"),
        (dict(fill=(0, 0, nan, 0, 0, 0, 0, 0)), b"fill"), (dict(fill=(inf, 0, 0, 0, 0, 0, 0, 0)), b"fill"),
        (tt(0, dst=0x10000000), b"overlaps src"),                                            # in place
        (tt(1, dst=0x10000000 + (2 * 8 * plane + 4 * plane) * 4 - 4), b"overlaps src"),      # the last element of tensor 1's span
        (tt(0, dst=0x10000000 - 3 * 2 * plane * 4 + 4), b"overlaps src"),                    # dst's last element on src's first
        (tt(1, dst=0x20000000 + 3 * 2 * plane * 4 - 4), b"overlaps dst"),                    # dst 1 begins on dst 0's last element
    ]
    L = lib.lib()
    for kw, needle in cases:
        rc = _call(lib, **kw)
        msg = L.dmm_last_error()
        assert rc == lib.ERR_INVALID and needle in msg and msg.startswith(b"dmm_warp_batch: "), (kw.keys(), needle, rc, msg)


# ------------------------------------------------------------------------------------------------ BatchAugment
ID8 = [1065353216] * 8      # 1.0f, eight times
# params_at of existing configurations as the commit BEFORE `scale` and `rotate` drew them: ((constructor arguments), (i, B, Hs, Ws),
# the values; image_gain and image_bias as the bits of their float32)
RECORDED = [
    ({}, (0, 2, 48, 80),
     {'y0': [0, 0], 'x0': [0, 0], 'flip': [0, 0], 'image_gain': [ID8, ID8], 'image_bias': [0, 0], 'drop_lidar': [False, False],
      'drop_image': [False, False], 'out_size': (48, 80)}),
    ({'out_size': (64, 96), 'hflip': 0.5, 'translate': (5, 9), 'brightness': 0.2, 'contrast': 0.3, 'channel_gain': 0.1, 'lidar_dropout': 0.3,
      'image_dropout': 0.3, 'seed': 7, 'rank': 1}, (3, 2, 96, 128),
     {'y0': [33, 6], 'x0': [31, 39], 'flip': [1, 1],
      'image_gain': [[1064124937, 1062508758, 1063248540, 1062996875, 1062554879, 1062860293, 1063724324, 1063639680],
                     [1062062556, 1062377611, 1061312008, 1060877291, 1063222246, 1061154922, 1062788404, 1060907996]],
      'image_bias': [3185939546, 3189173165], 'drop_lidar': [True, False], 'drop_image': [False, False], 'out_size': (64, 96)}),
    ({'out_size': (32, 64), 'hflip': 1.0, 'translate': (0, 4), 'seed': 18446744073709551615}, (0, 2, 37, 70),
     {'y0': [5, 2], 'x0': [4, 4], 'flip': [1, 1], 'image_gain': [ID8, ID8], 'image_bias': [0, 0], 'drop_lidar': [False, False],
      'drop_image': [False, False], 'out_size': (32, 64)}),
    ({'hflip': 0.25, 'translate': 3, 'brightness': 8.0, 'seed': 11, 'rank': 4}, (9, 2, 48, 80),
     {'y0': [-3, 0], 'x0': [-3, -1], 'flip': [0, 0], 'image_gain': [ID8, ID8], 'image_bias': [3232142547, 3226704226],
      'drop_lidar': [False, False], 'drop_image': [False, False], 'out_size': (48, 80)}),
    ({'out_size': (128, 160), 'contrast': 0.5, 'lidar_dropout': 1.0}, (1099511627776, 2, 96, 128),
     {'y0': [0, 0], 'x0': [0, 0], 'flip': [0, 0], 'image_gain': [[1068189964] * 8, [1059096482] * 8], 'image_bias': [0, 0],
      'drop_lidar': [True, True], 'drop_image': [False, False], 'out_size': (128, 160)}),
    ({'out_size': 64, 'channel_gain': 0.9, 'image_dropout': 0.5, 'seed': 5}, (1, 2, 64, 64),
     {'y0': [0, 0], 'x0': [0, 0], 'flip': [0, 0],
      'image_gain': [[1054999958, 1057353629, 1065588166, 1039037658, 1066434800, 1058611116, 1070911909, 1070404483],
                     [1058971067, 1062198746, 1065494310, 1047120547, 1041923443, 1053373442, 1054407957, 1065645181]],
      'image_bias': [0, 0], 'drop_lidar': [False, False], 'drop_image': [True, False], 'out_size': (64, 64)}),
]


def _record(p):
    return dict(y0=p.y0.tolist(), x0=p.x0.tolist(), flip=p.flip.tolist(), image_gain=p.image_gain.view(np.uint32).tolist(),
                image_bias=p.image_bias.view(np.uint32).tolist(), drop_lidar=p.drop_lidar.tolist(), drop_image=p.drop_image.tolist(),
                out_size=tuple(p.out_size))


def test_existing_configurations_draw_what_they_drew_before(lib):
    from dmmfods_amd.augment import BatchAugment
    for kw, args, want in RECORDED:
        p = BatchAugment(**kw).params_at(*args)
        assert _record(p) == want, kw
        assert p.zoom.tolist() == [1.0, 1.0] and p.angle.tolist() == [0.0, 0.0] and p.zoom.dtype == p.angle.dtype == np.float64
        # the new knobs take draws of their own, behind the others: turning them moves nothing else
        q = BatchAugment(scale=0.3, rotate=20.0, **kw).params_at(*args)
        assert _record(q) == want and not np.array_equal(q.zoom, p.zoom) and not np.array_equal(q.angle, p.angle)


def test_constructor_validates_scale_and_rotate(lib):
    from dmmfods_amd.augment import BatchAugment
    a = BatchAugment(scale=0.25, rotate=15)
    assert (a.scale, a.rotate) == (0.25, 15.0) and (BatchAugment().scale, BatchAugment().rotate) == (0.0, 0.0)
    BatchAugment(scale=63 / 64, rotate=180)
    for kw in (dict(scale=-0.1), dict(scale=1.0), dict(scale=0.99), dict(scale=float("nan")), dict(rotate=-1), dict(rotate=180.5),
               dict(rotate=float("nan")), dict(rotate=float("inf"))):
        with pytest.raises(ValueError):
            BatchAugment(**kw)
    with pytest.raises((TypeError, ValueError)):
        BatchAugment(rotate="a lot")


def test_matrices_at_zero_strengths_are_the_windows(lib):
    from dmmfods_amd.augment import BatchAugment
    aug = BatchAugment(out_size=(32, 64), hflip=0.5, translate=(5, 9), seed=3)
    p = aug.params_at(2, 64, 37, 70)
    a, b = BatchAugment.matrices(p, 37, 70)
    assert a.dtype == np.int32 and a.shape == (64, 2, 2) and b.dtype == np.int64 and b.shape == (64, 2) and set(p.flip.tolist()) == {0, 1}
    for s in range(64):
        wa, wb = window_matrix(int(p.y0[s]), int(p.x0[s]), int(p.flip[s]), 64)
        assert a[s].tolist() == wa and b[s].tolist() == wb, s
    # an even and an odd output size alike (the centre (Wo - 1) / 2 is a half or whole): nothing is left of it
    p = BatchAugment(out_size=(33, 37), hflip=1.0).params_at(0, 3, 40, 40)
    a, b = BatchAugment.matrices(p)
    assert all(a[s].tolist() == window_matrix(int(p.y0[s]), int(p.x0[s]), 1, 37)[0] and b[s].tolist() == window_matrix(int(p.y0[s]), int(p.x0[s]), 1, 37)[1]
               for s in range(3))


def test_matrices_follow_the_documented_composition(lib):
    from dmmfods_amd.augment import BatchAugment
    aug = BatchAugment(out_size=(32, 64), hflip=0.5, translate=(2, 3), scale=0.4, rotate=30.0, seed=9)
    p = aug.params_at(0, 32, 48, 80)
    assert p.zoom.min() >= 0.6 and p.zoom.max() <= 1.4 and np.abs(p.angle).max() <= 30.0 and len(set(p.zoom.tolist())) == 32 == len(set(p.angle.tolist()))
    big = aug.params_at(1, 4096, 48, 80)
    assert 0.6 <= big.zoom.min() < 0.61 and 1.39 < big.zoom.max() <= 1.4 and -30 <= big.angle.min() < -29.9 and 29.9 < big.angle.max() <= 30
    a, b = BatchAugment.matrices(p, 48, 80)
    Ho, Wo = 32, 64
    for s in range(32):
        t, z = np.deg2rad(p.angle[s]), p.zoom[s]
        for x, y in ((0, 0), (63, 0), (0, 31), (20, 11)):
            u, v = x - (Wo - 1) / 2, y - (Ho - 1) / 2
            xw = (np.cos(t) * u - np.sin(t) * v) / z + (Wo - 1) / 2
            yw = (np.sin(t) * u + np.cos(t) * v) / z + (Ho - 1) / 2
            sx, sy = p.x0[s] + (Wo - 1 - xw if p.flip[s] else xw), p.y0[s] + yw
            got = (a[s].astype(np.float64) @ np.array([x, y]) + b[s]) / ONE
            # six coefficients rounded to 2^-21 each, multiplied by at most 63 and 31
            assert abs(got[0] - sx) <= (63 + 31 + 1) * 2.0 ** -21 + 1e-9 and abs(got[1] - sy) <= (63 + 31 + 1) * 2.0 ** -21 + 1e-9
    # the centre of the window is the fixed point of zoom and rotation
    p1 = BatchAugment(out_size=(33, 65), scale=0.4, rotate=30.0, seed=9).params_at(0, 8, 33, 65)
    a, b = BatchAugment.matrices(p1)
    centre = (a.astype(np.float64) @ np.array([32.0, 16.0]) + b) / ONE
    assert np.abs(centre - np.array([32.0, 16.0])).max() <= 49 * 2.0 ** -21


def test_new_draws_are_pure_and_independent_between_batches(lib):
    from dmmfods_amd.augment import BatchAugment
    kw = dict(out_size=(64, 96), hflip=0.5, scale=0.2, rotate=10.0, seed=7, rank=1)
    a, b = BatchAugment(**kw), BatchAugment(**kw)
    p = a.params_at(3, 16, 96, 128)
    b.params_at(0, 16, 96, 128), b.params_at(9, 4, 96, 128)
    q = b.params_at(3, 16, 96, 128)
    assert np.array_equal(p.zoom, q.zoom) and np.array_equal(p.angle, q.angle) and a.batches_drawn == b.batches_drawn == 0
    n = a.params_at(4, 16, 96, 128)
    assert not set(p.zoom.tolist()) & set(n.zoom.tolist()) and not set(p.angle.tolist()) & set(n.angle.tolist())
    other = BatchAugment(**dict(kw, rank=2)).params_at(3, 16, 96, 128)
    assert not set(p.zoom.tolist()) & set(other.zoom.tolist())
    # zoom does not depend on rotate's strength nor the other way round
    z = BatchAugment(**dict(kw, rotate=0.0)).params_at(3, 16, 96, 128)
    r = BatchAugment(**dict(kw, scale=0.0)).params_at(3, 16, 96, 128)
    assert np.array_equal(z.zoom, p.zoom) and not z.angle.any() and np.array_equal(r.angle, p.angle) and (r.zoom == 1).all()


def test_state_dict_round_trip_keeps_its_keys(lib):
    from dmmfods_amd.augment import BatchAugment
    kw = dict(scale=0.2, rotate=10.0, hflip=0.5)
    a = BatchAugment(seed=5, rank=2, **kw)
    a.batches_drawn = 17
    st = a.state_dict()
    assert st == {"seed": 5, "rank": 2, "batches_drawn": 17}
    b = BatchAugment(**kw)
    b.load_state_dict(json.loads(json.dumps(st)))
    p, q = b.params_at(b.batches_drawn, 8, 32, 32), a.params_at(17, 8, 32, 32)
    assert b.state_dict() == st and np.array_equal(p.zoom, q.zoom) and np.array_equal(p.angle, q.angle)
    assert np.array_equal(BatchAugment.matrices(p)[0], BatchAugment.matrices(q)[0])


def test_agent_config_field_keeps_refusing_scale_and_rotate(lib):
    """config.loader.augment takes what it took (tests/test_augment_cpu.py pins that `rotate` there is a TypeError); the knobs reach
    the agent as a BatchAugment of the caller's own in `agent.augment` (tests/test_warp_gpu.py)."""
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    for spec in ({"rotate": 10}, {"scale": 0.2}, {"out_size": (64, 96), "scale": 0.2, "rotate": 10.0, "seed": 9}):
        with pytest.raises(TypeError, match="scale|rotate"):
            Agent._make_augment(spec)
    aug = Agent._make_augment({"out_size": (64, 96), "seed": 9})
    assert (aug.scale, aug.rotate) == (0.0, 0.0)


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
    """DRIVE_WARP=1: behind the plan's life the stand-alone driver makes one valid call with 33 samples (operands that are addresses
    only) - exactly two launches of one workgroup per 64 x 16 tile and channel - and tries every refusal, under ASan + UBSan.  Without
    the switch the row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = [ln for ln in _run(drive, {}, args) if ln.startswith("T ")]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["(none) | " + args]
    out = _run(drive, {"DRIVE_WARP": "1"}, args)
    assert "WARP OK" in out and "WARP 33 samples: 2 launches, grid 2 x 7 ok" in out, out[-12:]
    trace = [ln for ln in out if ln.startswith("T ")]
    assert trace[:len(base)] == base                                # the plan's schedule is untouched ...
    extra = trace[len(base):]                                       # ... and behind it: the two launches, nothing else
    assert len(extra) == 2 and all(ln.startswith("T launch") and "warp_kernel" in ln for ln in extra), extra
    assert [tuple(map(int, ln.split()[3:5])) for ln in extra] == [(2, 7), (2, 7)]
