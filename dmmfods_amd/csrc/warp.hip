// On-device affine warp: scale and rotation of every plane of a batch - a fixed-point affine map per sample, each tensor
// sampled nearest or bilinear, with dmm_augment_batch's per-channel gain, bias and fill - in one memory-bound launch.  The semantics
// are stated in include/dmmfods_hip.h (dmm_warp_batch); F = DMM_WARP_FRAC_BITS.  For sample b, output pixel (x, y), in int64:
//   SX = a00 * x + a01 * y + b0;   SY = a10 * x + a11 * y + b1
//   nearest:   (sx, sy) = ((SX + HALF) >> F, (SY + HALF) >> F); inside: the source's bits, then the gain / bias rule; outside: fill
//   bilinear:  taps (SX >> F, SY >> F) + {0, 1}^2, weights the low F bits; fx == fy == 0: tap 00 alone, as nearest; no tap inside: fill;
//              else top = v00 + wx * (v01 - v00), bot = v10 + wx * (v11 - v10), v = top + wy * (bot - top), then the gain / bias rule
// Grid: x = output TILES of a plane (TW x TH pixels, row-major), y = global channel, z = sample within the launch.  The sample's six
// coefficients, the channel's gain, bias, fill and mode, the tile's origin and class and every base pointer are uniform over a
// workgroup and live in scalar registers.  A lane owns one QUAD, four consecutive output pixels of one row: SX and SY are formed once
// per lane and advance along the quad by a00 / a10; the quad is stored as 16 bytes where its address is aligned, else by elements.
// The tile is two-dimensional so that under a rotation its source footprint stays a compact patch whose lines the taps of
// neighbouring lanes share; the shape is chosen by measurement (tools/warp_cost.py, profiles/r17/warp_cost.txt).
//
// TILE CLASSES.  A tile covers the pixels [X0, X1] x [Y0, Y1] (clipped to the output).  SX is affine in (x, y), so over that rectangle
// it takes its least and its greatest value at corners: with dx = a00 * (X1 - X0) and dy = a01 * (Y1 - Y0),
//   lo = SX(X0, Y0) + min(dx, 0) + min(dy, 0)  <=  SX(x, y)  <=  SX(X0, Y0) + max(dx, 0) + max(dy, 0) = hi      for every pixel of the tile
// and both bounds are attained.  t -> (t + r) >> F is monotone, so every pixel's integer coordinate lies in [(lo + r) >> F, (hi + r) >> F]
// (r = HALF for nearest, 0 for bilinear's x0; bilinear's second tap adds 1 to both ends).  Hence
//   INSIDE:   0 <= least coordinate and greatest coordinate (+ 1 for bilinear) <= Ws - 1, likewise in y: every tap of every pixel is
//             inside the source - no test per tap;
//   OUTSIDE:  in x or in y the whole interval (with bilinear's + 1) misses [0, Ws - 1]: every pixel has that coordinate of all its taps
//             outside, so every pixel is fill - nothing is loaded;
//   otherwise the GUARDED path, which tests every tap and is right for any tile.
// Both claims are implications from interval bounds that hold for every pixel, so a tile is never classed INSIDE or OUTSIDE wrongly;
// a tile that could have been either and was not only runs the guarded path.  No LDS, no scratch, no atomics: every output element is
// written exactly once by exactly one lane.
#include "common.h"
#include "pointwise.h"

namespace dmm {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int F = DMM_WARP_FRAC_BITS;
constexpr long long ONE = 1ll << F, HALF = ONE >> 1, MASK = ONE - 1;

// (gain * v) + bias: two fp32 roundings, contraction off as in augment.hip, so that no fma is formed
__device__ __forceinline__ unsigned warp_gain(unsigned bits, bool ident, float gain, float bias) {
#pragma clang fp contract(off)
  if (ident) return bits;
  const float p = gain * __uint_as_float(bits);
  return __float_as_uint(p + bias);
}

// the three interpolation steps, each product and each sum rounded on its own
__device__ __forceinline__ float warp_lerp2(float v00, float v01, float v10, float v11, float wx, float wy) {
#pragma clang fp contract(off)
  const float dt = v01 - v00, pt = wx * dt, top = v00 + pt;
  const float db = v11 - v10, pb = wx * db, bot = v10 + pb;
  const float dv = bot - top, pv = wy * dv;
  return top + pv;
}

enum { TILE_OUTSIDE = 0, TILE_INSIDE = 1, TILE_GUARDED = 2 };

// LXB: log2 of the quads in a tile row; the tile is (4 << LXB) x (256 >> LXB) pixels
template <int LXB, bool NT>
__global__ __launch_bounds__(256) void warp_kernel(WarpArgs a) {
  constexpr int TW = 4 << LXB, TH = 256 >> LXB;
  const int c = blockIdx.y;
  const unsigned tiles_x = ((unsigned)a.Wo + TW - 1) / TW;
  const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int X0 = (int)tx * TW, Y0 = (int)ty * TH;                    // < Wo, < Ho
  const int X1 = X0 + min(TW, a.Wo - X0) - 1, Y1 = Y0 + min(TH, a.Ho - Y0) - 1;
  const int Hs = a.Hs, Ws = a.Ws;
  const long long a00 = a.s[blockIdx.z].a00, a01 = a.s[blockIdx.z].a01, a10 = a.s[blockIdx.z].a10, a11 = a.s[blockIdx.z].a11;
  const long long b0 = a.s[blockIdx.z].b0, b1 = a.s[blockIdx.z].b1;
  const float gain = a.s[blockIdx.z].gain[c], bias = a.s[blockIdx.z].bias[c];
  const bool ident = gain == 1.f && bias == 0.f;
  const float fillf = a.fill[c];
  const unsigned fill = __float_as_uint(fillf);
  // a map whose coefficients are all whole: fx == fy == 0 at every pixel, bilinear is tap 00 alone - the nearest rule, where HALF is
  // floored away again
  const bool lattice = ((a00 | a01 | a10 | a11 | b0 | b1) & MASK) == 0;
  const bool nearest = a.mode[c] == DMM_WARP_NEAREST || lattice;
  const size_t b = (size_t)(a.b0 + (int)blockIdx.z);
  const float* P = a.ch[c].src + b * (size_t)a.ch[c].src_stride;     // the sample's source plane

  // the tile's class (see the head of the file); all uniform
  const long long rnd = nearest ? HALF : 0, second = nearest ? 0 : 1;
  const long long cx = a00 * X0 + a01 * Y0 + b0 + rnd, cy = a10 * X0 + a11 * Y0 + b1 + rnd;
  const long long dxx = a00 * (X1 - X0), dxy = a01 * (Y1 - Y0), dyx = a10 * (X1 - X0), dyy = a11 * (Y1 - Y0);
  const long long xlo = (cx + min(dxx, 0ll) + min(dxy, 0ll)) >> F, xhi = ((cx + max(dxx, 0ll) + max(dxy, 0ll)) >> F) + second;
  const long long ylo = (cy + min(dyx, 0ll) + min(dyy, 0ll)) >> F, yhi = ((cy + max(dyx, 0ll) + max(dyy, 0ll)) >> F) + second;
  int cls = TILE_GUARDED;
  if (xhi < 0 || xlo >= Ws || yhi < 0 || ylo >= Hs) cls = TILE_OUTSIDE;
  else if (xlo >= 0 && xhi < Ws && ylo >= 0 && yhi < Hs) cls = TILE_INSIDE;

  const int lx = threadIdx.x & ((1 << LXB) - 1), ly = threadIdx.x >> LXB;
  const int x = X0 + lx * 4, y = Y0 + ly;
  if (x > X1 || y > Y1) return;
  const int n = min(4, a.Wo - x);
  float* D = a.ch[c].dst + b * (size_t)a.ch[c].dst_stride + ((size_t)y * (size_t)a.Wo + (size_t)x);
  unsigned r[4] = {fill, fill, fill, fill};

  if (cls != TILE_OUTSIDE) {
    long long SX = cx + a00 * (lx * 4) + a01 * ly, SY = cy + a10 * (lx * 4) + a11 * ly;   // (rnd is in cx, cy)
    const bool in_all = cls == TILE_INSIDE;
    if (nearest) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long sx = SX >> F, sy = SY >> F;
        if (j < n && (in_all || (sx >= 0 && sx < Ws && sy >= 0 && sy < Hs)))
          r[j] = warp_gain(__float_as_uint(P[sy * Ws + sx]), ident, gain, bias);
        SX += a00; SY += a10;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long x0 = SX >> F, y0 = SY >> F;
        const int fx = (int)(SX & MASK), fy = (int)(SY & MASK);
        const bool ix0 = in_all || (x0 >= 0 && x0 < Ws), ix1 = in_all || (x0 >= -1 && x0 < Ws - 1);
        const bool iy0 = in_all || (y0 >= 0 && y0 < Hs), iy1 = in_all || (y0 >= -1 && y0 < Hs - 1);
        if (j < n) {
          // tap 00, the others at + 1, + Ws, + Ws + 1 (formed unsigned: far outside it may wrap, and is then not used)
          const long long e = (long long)((unsigned long long)y0 * (unsigned long long)Ws + (unsigned long long)x0);
          if ((fx | fy) == 0) {
            if (ix0 && iy0) r[j] = warp_gain(__float_as_uint(P[e]), ident, gain, bias);
          } else if ((ix0 || ix1) && (iy0 || iy1)) {
            const float v00 = ix0 && iy0 ? P[e] : fillf, v01 = ix1 && iy0 ? P[e + 1] : fillf;
            const float v10 = ix0 && iy1 ? P[e + Ws] : fillf, v11 = ix1 && iy1 ? P[e + Ws + 1] : fillf;
            const float v = warp_lerp2(v00, v01, v10, v11, (float)fx * 0x1p-20f, (float)fy * 0x1p-20f);
            r[j] = warp_gain(__float_as_uint(v), ident, gain, bias);
          }
        }
        SX += a00; SY += a10;
      }
    }
  }
  if (n == 4 && ((uintptr_t)D & 15) == 0) {
    const u32x4 v = {r[0], r[1], r[2], r[3]};
    if (NT) __builtin_nontemporal_store(v, (u32x4*)D);
    else *(u32x4*)D = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) ((unsigned*)D)[j] = r[j];
  }
}
static_assert(F == 20, "the weight's scale 0x1p-20f is 2^-F");

// What ships: quads per tile row, log2 (3 = 32 x 32 pixels, 4 = 64 x 16, 5 = 128 x 8, 6 = 256 x 4), and the store kind.  Both by
// measurement at C2's shapes, profiles/r17/warp_cost.txt.
constexpr int WARP_LXB = 4;
constexpr bool WARP_NT = true;

// (a lab build, -DDMM_LAB=1, holds every shape and both store kinds and reads the choice from the environment at EVERY launch, so
// that tools/warp_cost.py can let them take turns inside one process; the library proper holds the one kernel that ships)
inline int warp_lxb() {
  const int v = lab_int("DMM_WARP_LXB", WARP_LXB);
  return v >= 3 && v <= 6 ? v : WARP_LXB;
}

}  // namespace

unsigned warp_grid_x(int Ho, int Wo) {
  const int lxb = warp_lxb(), TW = 4 << lxb, TH = 256 >> lxb;
  return (unsigned)((((size_t)Wo + TW - 1) / TW) * (((size_t)Ho + TH - 1) / TH));
}

hipError_t launch_warp(const WarpArgs& a, int nchannels, int nsamples, hipStream_t st) {
  const dim3 grid(warp_grid_x(a.Ho, a.Wo), nchannels, nsamples);
#if DMM_LAB
  const int lxb = warp_lxb();
  if (lab_int("DMM_WARP_NT", WARP_NT)) {
    if (lxb == 3) hipLaunchKernelGGL((warp_kernel<3, true>), grid, dim3(256), 0, st, a);
    else if (lxb == 4) hipLaunchKernelGGL((warp_kernel<4, true>), grid, dim3(256), 0, st, a);
    else if (lxb == 5) hipLaunchKernelGGL((warp_kernel<5, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((warp_kernel<6, true>), grid, dim3(256), 0, st, a);
  } else {
    if (lxb == 3) hipLaunchKernelGGL((warp_kernel<3, false>), grid, dim3(256), 0, st, a);
    else if (lxb == 4) hipLaunchKernelGGL((warp_kernel<4, false>), grid, dim3(256), 0, st, a);
    else if (lxb == 5) hipLaunchKernelGGL((warp_kernel<5, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((warp_kernel<6, false>), grid, dim3(256), 0, st, a);
  }
#else
  hipLaunchKernelGGL((warp_kernel<WARP_LXB, WARP_NT>), grid, dim3(256), 0, st, a);
#endif
  return hipGetLastError();
}

}  // namespace dmm
