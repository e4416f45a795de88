// Forward of the parity-phase convolutions with many input channels - the decoder's ConvTranspose2d 3x3 stride 2 (reference
// M:155-160), run as four output-parity phases of 1, 2, 2 and 4 taps over the input grid - on an LDS halo tile.  gfx950, 16-bit
// storage types.
//
//   out[S p + parity][n] = sum over taps t, channels c of  A[p + t][c] * W_t[c][n],     A = relu(bn(x))
// The generic implicit-GEMM kernel (igemm.hip) gathers, bounds-tests and normalises A once per tap AND per 128-column output
// tile: 9/4 x 4 = up to 36 times per element for the first stage (1024 -> 512 channels), and does so inside every K stage.
// Here a workgroup owns an 8 x 16 pixel tile x 128 output channels and walks the input channels in groups of 128:
//   * per group the 9 x 17 pixel halo of A is loaded once (16-byte slots, branch-free, the next group's loads in flight behind the
//     current group's MFMAs), normalised once per element and written to an LDS image (pixel pitch 272 bytes: the 16 lanes of a
//     ds_read_b128 group hit 16 different slots); a tap is an address offset of the A fragment;
//   * the packed weights of a stage (2 chunks x 128 columns) go through a double-buffered LDS image (registers -> ds_write, XOR
//     swizzle as in igemm.hip), prefetched one stage ahead;
//   * one barrier per stage of 16 MFMAs per wave and nothing but fragment reads and MFMAs between barriers;
//   * epilogue as in conv3.hip: values staged as T, BatchNorm sums straight from the accumulator layout, parity-strided store.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.h"
#include "dispatch.h"
#include "gather.h"
#include "isa.h"

namespace dmm {

constexpr int CP_TH = 8, CP_TW = 16, CP_HH = 9, CP_HW = 17;
constexpr int CP_CA = 128;                      // input channels per group
constexpr int CP_BN = 128;                      // output channels per workgroup
constexpr int CP_PP = CP_CA * 2 + 16;           // pixel pitch of the halo image
constexpr int CP_RP = (CP_HW * CP_PP + 255) / 256 * 256;
constexpr int CP_X_BYTES = CP_HH * CP_RP;       // 43 KB
constexpr int CP_B_STAGE = 2 * CP_BN * 64;      // 16 KB: two 64-byte chunks of K for 128 columns
constexpr int CP_MAIN = CP_X_BYTES + 2 * CP_B_STAGE;
constexpr int CP_CPITCH = CP_BN + 8;            // staging pitch (elements of T)
constexpr int CP_EXTRA = BM * 4;                 // rowpix (the epilogue's column partials / fp64 sums overlay the dead operand images)
constexpr int CP_LDS = CP_MAIN + CP_EXTRA;
static_assert(BM * (CP_BN + 4) * 4 + 4 * 2 * CP_BN * 4 <= CP_MAIN, "fp32 staging + partials fit the operand images");
constexpr int CP_PART = BM * (CP_BN + 4) * 4;   // offset of the partials inside the dead images (behind the largest staging form)
static_assert(2 * CP_LDS <= 160 * 1024, "two workgroups per CU");

struct CvpArgs {
  ConvArgs c;
  int tiles_y, tiles_x, ntn;  // pixel tiles, 128-column tiles
  int dymin, dxmin;           // origin of the tap box
  // multi-phase launches (ConvArgs::nphase = 4): workgroups per phase, per XCD and phase (rounded up), the phases longest first, the
  // origin of each phase's tap box
  int per, per8;
  signed char order[4], ph_dymin[4], ph_dxmin[4];
};
// What distinguishes the phases of a multi-phase launch (the single-phase launch: the fields of ConvArgs / CvpArgs themselves).
struct CvpPhase { const void* wpack; const short* taps; int py, px, dymin, dxmin; };

template <typename T, int NTAP>
__device__ __forceinline__ void cvp_body(const CvpArgs& g, const int lbid, const CvpPhase P) {
  static_assert(sizeof(T) == 2, "16-bit storage");
  typedef typename TT<T>::vec V;
  constexpr int SLOT = 8, BN = CP_BN, NT = BN / 32;
  constexpr int NX = (CP_HH * CP_HW * (CP_CA / SLOT) + NTHREADS - 1) / NTHREADS;  // 10 halo slots per thread
  constexpr int NST = NTAP * 2;                                                   // stages per channel group
  const ConvArgs& a = g.c;
  const Seg& sx = a.seg[0];

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Xs = smem;
  unsigned char* Bs = smem + CP_X_BYTES;
  int* rowpix = (int*)(smem + CP_MAIN);
  float* wpart = (float*)(smem + CP_PART);  // [wave][2][BN]; only touched after the K loop

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ntile = lbid % g.ntn;
  int tile = lbid / g.ntn;
  const int tx_i = tile % g.tiles_x; tile /= g.tiles_x;
  const int ty_i = tile % g.tiles_y;
  const int b = tile / g.tiles_y;
  const int y0 = ty_i * CP_TH, x0 = tx_i * CP_TW, n0 = ntile * BN;

  if (tid < BM) {
    const int y = y0 + (tid >> 4), x = x0 + (tid & 15);
    rowpix[tid] = (y < a.Ho && x < a.Wo) ? (b * a.Hout + y * a.ostride + P.py) * a.Wout + x * a.ostride + P.px : -1;
  }

  // ---- the halo slots of this thread: fixed pixel positions, channel column cx of the current group ----
  const int cx = tid & 15, px0 = tid >> 4;
  int xlds[NX];
  size_t xpix[NX];
  unsigned xin = 0, okx = 0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const int hp = px0 + 16 * i;
    const int hy = hp / CP_HW, hx = hp - hy * CP_HW;
    const int y = y0 + P.dymin + hy, x = x0 + P.dxmin + hx;
    if (hp < CP_HH * CP_HW) {
      xin |= 1u << i;
      if ((unsigned)y < (unsigned)sx.Hs && (unsigned)x < (unsigned)sx.Ws) okx |= 1u << i;
    }
    xlds[i] = hy * CP_RP + hx * CP_PP + cx * 16;
    xpix[i] = ((size_t)(b * sx.Hs + min(max(y, 0), sx.Hs - 1)) * sx.Ws + min(max(x, 0), sx.Ws - 1)) * sx.ld + cx * SLOT;
  }
  const T* xsrc = (const T*)sx.src;
  V rx[NX];
  auto issue_halo = [&](int grp) {  // branch-free: clamped addresses, zeroed at the write if outside the picture
#pragma unroll
    for (int i = 0; i < NX; ++i) rx[i] = *(const V*)(xsrc + xpix[i] + grp * CP_CA);
  };
  auto store_halo = [&](int grp) {
    SlotK<SLOT> kx;
    kx.k0 = load_fv<SLOT>(sx.scale + grp * CP_CA + cx * SLOT); kx.k1 = load_fv<SLOT>(sx.shift + grp * CP_CA + cx * SLOT); kx.k2 = 0.f; kx.k3 = 0.f;
    V z;
#pragma unroll
    for (int e = 0; e < SLOT; ++e) z[e] = (T)0;
#pragma unroll
    for (int i = 0; i < NX; ++i)
      if ((xin >> i) & 1) *(V*)(Xs + xlds[i]) = ((okx >> i) & 1) ? bn_relu_slot(rx[i], kx) : z;
  };

  // ---- weights: a stage = chunks (c0, c0 + 1) x 128 columns = 2 x 8 KB contiguous; thread -> pieces tid, tid + 256 of each ----
  const T* wp = (const T*)P.wpack;
  const int cpt = sx.Cpad / 32;  // chunks per tap
  // two register sets, filled two stages ahead: a stage's MFMAs are shorter than an L2 round trip.  Every load is issued
  // unconditionally (past the end: a valid chunk again) so that the compiler's counted waits leave the other set in flight.
  struct BRegs { V v[2][2]; };
  BRegs rb0, rb1;
  int blds[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int piece = tid + NTHREADS * j, row = piece >> 2, slot = piece & 3;
    blds[j] = row * 64 + ((slot ^ ((row >> 2) & 3)) << 4);
  }
  const int ngrp = sx.C / CP_CA;
  auto issue_b = [&](BRegs& R, int grp, int st) {  // stage st of group grp; st may run past the group (the next group's stages)
    int gq = grp + (st >= NST ? 1 : 0);
    const int sq = st >= NST ? st - NST : st;
    gq = min(gq, ngrp - 1);
    const int c0 = (sq >> 1) * cpt + gq * 4 + 2 * (sq & 1);
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {
      const T* src = wp + ((size_t)(c0 + uu) * a.Npad + n0) * 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) R.v[uu][j] = *(const V*)(src + (size_t)(tid + NTHREADS * j) * SLOT);
    }
  };
  auto store_b = [&](const BRegs& R, int buf) {
    unsigned char* B = Bs + buf * CP_B_STAGE;
#pragma unroll
    for (int uu = 0; uu < 2; ++uu)
#pragma unroll
      for (int j = 0; j < 2; ++j) *(V*)(B + uu * (BN * 64) + blds[j]) = R.v[uu][j];
  };

  // ---- fragments: wave w owns tile rows 2w, 2w + 1 (32 pixels) x 128 columns ----
  int aoff[NTAP];
#pragma unroll
  for (int t = 0; t < NTAP; ++t) {
    const int tw = P.taps[t];
    const int dy = (int)(signed char)(tw & 0xff) - P.dymin, dx = (int)(signed char)((tw >> 8) & 0xff) - P.dxmin;
    aoff[t] = (2 * wave + (r >> 4) + dy) * CP_RP + ((r & 15) + dx) * CP_PP + h * 16;
  }
  const int bsw = (r >> 2) & 3;

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  issue_halo(0);
  issue_b(rb0, 0, 0);
  issue_b(rb1, 0, 1);
  for (int grp = 0; grp < ngrp; ++grp) {
    store_halo(grp);  // (the barrier that ended the previous group made the image free)
    issue_halo(min(grp + 1, ngrp - 1));
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      BRegs& R = (st & 1) ? rb1 : rb0;  // NST is even: stage parity = register set = LDS buffer, across groups as well
      store_b(R, st & 1);
      __syncthreads();  // this stage's weights (and, in the first stage of a group, the halo image) are complete
      issue_b(R, grp, st + 2);
      const unsigned char* B = Bs + (st & 1) * CP_B_STAGE;
      const unsigned char* A = Xs + aoff[st >> 1] + (st & 1) * 128;
#pragma unroll
      for (int uu = 0; uu < 2; ++uu)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const V av = *(const V*)(A + uu * 64 + s * 32);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const V bv = *(const V*)(B + (uu * BN + 32 * t + r) * 64 + (((2 * s + h) ^ bsw) << 4));
            acc[t] = mma16(av, bv, acc[t]);
          }
        }
    }
    __syncthreads();  // every wave is done with the halo image of this group
  }

  // ---- epilogue (conv3.hip): stage as T, column sums of the stored values straight from the accumulator layout ----
  T* Cs = (T*)smem;
  float ps1[NT], ps2[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    ps1[t] = 0.f; ps2[t] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
      const T v = from_f32<T>(acc[t][i]);
      Cs[row * CP_CPITCH + 32 * t + r] = v;
      if (rowpix[row] >= 0) { const float f = to_f32(v); ps1[t] += f; ps2[t] = fmaf(f, f, ps2[t]); }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    wpart[(wave * 2 + h) * BN + 32 * t + r] = fold_swap32(ps1[t], ps2[t]);  // lane half 0: the sum, half 1: the sum of squares
  }
  __syncthreads();
  constexpr int NCV = BN / SLOT, RPP = NTHREADS / NCV, NIT = BM / RPP;
  const int cv = tid % NCV, rr = tid / NCV;
  const int n = n0 + cv * SLOT;
  T* out = (T*)a.out;
  if (n < a.N) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int row = rr + RPP * i;
      const int pix = rowpix[row];
      if (pix >= 0) *(V*)(out + (size_t)pix * a.ldo + n) = *(const V*)(Cs + row * CP_CPITCH + cv * SLOT);
    }
  }
  if (a.stat_sum == nullptr) return;
  if (tid < 2 * BN) {
    const int col = tid % BN, which = tid / BN;
    if (n0 + col < a.N) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < 4; ++w) s += (double)wpart[(w * 2 + which) * BN + col];
      const size_t rep = (size_t)(blockIdx.x & (STAT_REPS - 1)) * a.stat_stride;
      atomic_add_f64((which ? a.stat_sq : a.stat_sum) + rep + n0 + col, s);
    }
  }
}

template <typename T, int NTAP>
__global__ __launch_bounds__(NTHREADS, 2) void cvp_kernel(const CvpArgs g) {
  const CvpPhase P = {g.c.wpack, g.c.seg[0].taps, g.c.py, g.c.px, g.dymin, g.dxmin};
  cvp_body<T, NTAP>(g, xcd_remap(blockIdx.x, gridDim.x), P);
}

// All parity phases of a ConvTranspose in one launch.  Workgroup b runs on XCD b % 8 and is the (b / 8)-th the XCD is handed: the
// phases are dealt in the order g.order (most taps first), per8 workgroups per XCD and phase, and inside a phase an XCD owns a
// contiguous range of the tile order (as xcd_remap gives a single-phase launch).
template <typename T>
__global__ __launch_bounds__(NTHREADS, 2) void cvp_multi_kernel(const CvpArgs g) {
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int slot = q / g.per8, j = q - slot * g.per8;
  const int lbid = xcd * g.per8 + j;
  if (lbid >= g.per) return;   // (workgroup-uniform: the rounding of per8)
  const int ph = g.order[slot];
  const CvpPhase P = {g.c.ph_wpack[ph], g.c.ph_taps0[ph], g.c.ph_py[ph], g.c.ph_px[ph], g.ph_dymin[ph], g.ph_dxmin[ph]};
  const int nt = g.c.ph_ntaps[ph];
  if (nt == 4) cvp_body<T, 4>(g, lbid, P);
  else if (nt == 2) cvp_body<T, 2>(g, lbid, P);
  else cvp_body<T, 1>(g, lbid, P);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Data gradient of the ConvTranspose stages: d a[p][c] = sum over the 9 taps (dy, dx) of dY[2 p + (dy, dx)][n] * W_t[n][c], fused
// with the BN+ReLU backward of the input's norm (EPI_BNBWD of igemm.hip).  The stride-2 gather splits by the PARITY of the
// gathered position into four sub-grids of dY, on each of which the taps form a box of 1, 2, 2 or 4 (exactly the forward
// phases, mirrored): the kernel above with the halo addressed at stride 2, the four classes accumulated into one tile.
struct CvdArgs {
  ConvArgs c;
  int tiles_y, tiles_x, ntn;
  int tapidx[16];  // the launch's taps ordered by class (even, even), (even, odd), (odd, even), (odd, odd)
};

// CA = channels of dY per group (128, or 64 for the head); UP2 = the 16 merged taps (-1..2)^2 of the 3x3 convolution over a
// nearest-x2 upsampled map (reference M:126-127; four taps in every class) instead of the ConvTranspose's nine.
template <typename T, int CA, bool UP2>
__global__ __launch_bounds__(NTHREADS, 2) void cvd_kernel(const CvdArgs g) {
  static_assert(sizeof(T) == 2 && (CA == 64 || CA == 128), "16-bit storage, 64 or 128 channels per group");
  typedef typename TT<T>::vec V;
  constexpr int SLOT = 8, BN = CP_BN, NT = BN / 32;
  constexpr int CSL = CA / SLOT;                       // slot columns of a halo pixel
  constexpr int PSTEP = NTHREADS / CSL;                // halo pixels between a thread's slots
  constexpr int NX = (CP_HH * CP_HW + PSTEP - 1) / PSTEP;
  constexpr int PP = CA * 2 + 16;                      // pixel pitch (an odd number of 16-byte slots)
  constexpr int RP = (CP_HW * PP + 255) / 256 * 256;
  constexpr int HALVES = CA / 64;                      // stages (2 chunks) per tap and group
  static_assert(CP_HH * RP <= CP_X_BYTES, "halo image fits");
  const ConvArgs& a = g.c;
  const Seg& sy = a.seg[0];  // dY (materialised gradient), 9 taps at stride 2

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Xs = smem;
  unsigned char* Bs = smem + CP_X_BYTES;
  int* rowpix = (int*)(smem + CP_MAIN);
  double* red = (double*)(smem + CP_PART);  // [2][BN] fp64; zeroed after the K loop

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int ntile = lbid % g.ntn;
  int tile = lbid / g.ntn;
  const int tx_i = tile % g.tiles_x; tile /= g.tiles_x;
  const int ty_i = tile % g.tiles_y;
  const int b = tile / g.tiles_y;
  const int y0 = ty_i * CP_TH, x0 = tx_i * CP_TW, n0 = ntile * BN;

  if (tid < BM) {
    const int y = y0 + (tid >> 4), x = x0 + (tid & 15);
    rowpix[tid] = (y < a.Ho && x < a.Wo) ? (b * a.Hout + y) * a.Wout + x : -1;
  }
  const int cx = tid % CSL, px0 = tid / CSL;
  int xlds[NX];
  unsigned xin = 0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const int hp = px0 + PSTEP * i;
    const int hy = hp / CP_HW, hx = hp - hy * CP_HW;
    if (hp < CP_HH * CP_HW) xin |= 1u << i;
    xlds[i] = hy * RP + hx * PP + cx * 16;
  }
  const T* ysrc = (const T*)sy.src + cx * SLOT;
  V rx[NX];
  unsigned okx = 0;
  // class (pa, pb): sub-grid pixel (y', x') = dY[2 y' + pa, 2 x' + pb]; its halo starts at (y0 - pa, x0 - pb)
  auto issue_halo = [&](int pa, int pb, int grp, unsigned& ok) {
    ok = 0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int hp = px0 + PSTEP * i;
      const int hy = hp / CP_HW, hx = hp - hy * CP_HW;
      const int y = 2 * (y0 - pa + hy) + pa, x = 2 * (x0 - pb + hx) + pb;
      if (hp < CP_HH * CP_HW && (unsigned)y < (unsigned)sy.Hs && (unsigned)x < (unsigned)sy.Ws) ok |= 1u << i;
      const size_t pix = (size_t)(b * sy.Hs + min(max(y, 0), sy.Hs - 1)) * sy.Ws + min(max(x, 0), sy.Ws - 1);
      rx[i] = *(const V*)(ysrc + pix * sy.ld + grp * CA);
    }
  };
  auto store_halo = [&](unsigned ok) {
    V z;
#pragma unroll
    for (int e = 0; e < SLOT; ++e) z[e] = (T)0;
#pragma unroll
    for (int i = 0; i < NX; ++i)
      if ((xin >> i) & 1) *(V*)(Xs + xlds[i]) = ((ok >> i) & 1) ? rx[i] : z;
  };

  const T* wp = (const T*)a.wpack;
  const int cpt = sy.Cpad / 32;
  V rb[2][2];
  int blds[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int piece = tid + NTHREADS * j, row = piece >> 2, slot = piece & 3;
    blds[j] = row * 64 + ((slot ^ ((row >> 2) & 3)) << 4);
  }
  auto issue_b = [&](int tap, int grp, int half) {
    const int c0 = tap * cpt + grp * (CA / 32) + 2 * half;
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {
      const T* src = wp + ((size_t)(c0 + uu) * a.Npad + n0) * 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) rb[uu][j] = *(const V*)(src + (size_t)(tid + NTHREADS * j) * SLOT);
    }
  };
  auto store_b = [&](int buf) {
    unsigned char* B = Bs + buf * CP_B_STAGE;
#pragma unroll
    for (int uu = 0; uu < 2; ++uu)
#pragma unroll
      for (int j = 0; j < 2; ++j) *(V*)(B + uu * (BN * 64) + blds[j]) = rb[uu][j];
  };

  const int abase = (2 * wave + (r >> 4)) * RP + (r & 15) * PP + h * 16;
  const int bsw = (r >> 2) & 3;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  constexpr int NCV = BN / SLOT, RPP = NTHREADS / NCV, NIT = BM / RPP;
  const int cv = tid % NCV, rr = tid / NCV;
  const int n = n0 + cv * SLOT;
  const bool colvalid = n < a.N;

  const int ngrp = sy.C / CA;
  // flat walk: class -> channel group -> tap of the class -> half (2 chunks).  Stage s of the walk uses B buffer s & 1.
  int buf = 0;
  int first_tap = 0;
  unsigned ok_cur = 0;
  issue_halo(0, 0, 0, ok_cur);
  issue_b(g.tapidx[0], 0, 0);
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int pa = cls >> 1, pb = cls & 1;
    const int ntap = UP2 ? 4 : (pa + 1) * (pb + 1);
    for (int grp = 0; grp < ngrp; ++grp) {
      store_halo(ok_cur);
      // the next halo: next group of this class, or group 0 of the next class
      const bool last_grp = grp + 1 == ngrp;
      if (!(last_grp && cls == 3)) {
        const int ncls = last_grp ? cls + 1 : cls;
        issue_halo(ncls >> 1, ncls & 1, last_grp ? 0 : grp + 1, ok_cur);
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        if (tt < ntap) {
          const int tap = g.tapidx[first_tap + tt];
          const int tw = sy.taps[tap];
          const int dy = (int)(signed char)(tw & 0xff), dx = (int)(signed char)((tw >> 8) & 0xff);
          // halo position of the tap inside the class: row offset (dy - pa) / 2 + pa = (dy + pa) / 2, likewise the column
          const int aoff = abase + ((dy + pa) >> 1) * RP + ((dx + pb) >> 1) * PP;
#pragma unroll
          for (int half = 0; half < HALVES; ++half) {
            store_b(buf);
            __syncthreads();
            // next stage's weights
            if (half + 1 < HALVES) issue_b(tap, grp, half + 1);
            else if (tt + 1 < ntap) issue_b(g.tapidx[first_tap + tt + 1], grp, 0);
            else if (!last_grp) issue_b(g.tapidx[first_tap], grp + 1, 0);
            else if (cls < 3) issue_b(g.tapidx[first_tap + ntap], 0, 0);
            const unsigned char* B = Bs + buf * CP_B_STAGE;
            const unsigned char* A = Xs + aoff + half * 128;
#pragma unroll
            for (int uu = 0; uu < 2; ++uu)
#pragma unroll
              for (int s = 0; s < 2; ++s) {
                const V av = *(const V*)(A + uu * 64 + s * 32);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                  const V bv = *(const V*)(B + (uu * BN + 32 * t + r) * 64 + (((2 * s + h) ^ bsw) << 4));
                  acc[t] = mma16(av, bv, acc[t]);
                }
              }
            buf ^= 1;
          }
        }
      }
      __syncthreads();  // every wave is done with this halo image
    }
    first_tap += ntap;
  }

  // ---- epilogue: fused BN+ReLU backward (see igemm.hip / conv3.hip) ----
  V xpre[NIT], gpre[NIT];
  int ppre[NIT];
  {
    const T* bx = (const T*)a.bx;
    const T* gold = (const T*)a.out;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int pix = rowpix[rr + RPP * i];
      ppre[i] = colvalid ? pix : -1;
#pragma unroll
      for (int e = 0; e < SLOT; ++e) { xpre[i][e] = (T)0; gpre[i][e] = (T)0; }
      if (ppre[i] >= 0) {
        xpre[i] = *(const V*)(bx + (size_t)pix * a.ldbx + n);
        if (a.accumulate) gpre[i] = *(const V*)(gold + (size_t)pix * a.ldo + n);
      }
    }
  }
  if (tid < 2 * BN) red[tid] = 0.0;  // (the K loop ended with a barrier: the images are dead)
  float* Cs = (float*)smem;  // fp32 staging (as igemm.hip): the ReLU mask and the reductions see the unrounded gradient
  constexpr int FPITCH = BN + 4;
  static_assert(BM * FPITCH * 4 <= CP_MAIN, "fp32 staging fits the operand images");
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
      Cs[row * FPITCH + 32 * t + r] = acc[t][i];
    }
  __syncthreads();
  float s1[SLOT], s2[SLOT];
#pragma unroll
  for (int i = 0; i < SLOT; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  T* gout = (T*)a.out;
  float sc[SLOT], sh[SLOT], mu[SLOT], is[SLOT];
  if (colvalid) {
    load_f32s<SLOT>(a.bscale + n, sc); load_f32s<SLOT>(a.bshift + n, sh);
    load_f32s<SLOT>(a.bmean + n, mu); load_f32s<SLOT>(a.binvstd + n, is);
  }
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    if (ppre[i] < 0) continue;
    const int row = rr + RPP * i;
    float av[SLOT], xf[SLOT], gf[SLOT];
#pragma unroll
    for (int e = 0; e < SLOT; e += 4) {
      const f32x4 t4 = *(const f32x4*)(Cs + row * FPITCH + cv * SLOT + e);
      av[e] = t4[0]; av[e + 1] = t4[1]; av[e + 2] = t4[2]; av[e + 3] = t4[3];
    }
    vec_to_f32<T>(xpre[i], xf);
    vec_to_f32<T>(gpre[i], gf);  // zeros unless accumulating
#pragma unroll
    for (int e = 0; e < SLOT; ++e) {
      const float dz = (fmaf(xf[e], sc[e], sh[e]) > 0.f) ? av[e] : 0.f;
      s1[e] += dz;
      s2[e] = fmaf(dz, (xf[e] - mu[e]) * is[e], s2[e]);
      gf[e] += sc[e] * dz;
    }
    *(V*)(gout + (size_t)ppre[i] * a.ldo + n) = f32_to_vec<T>(gf);
  }
  fold_to_lds<NCV, SLOT, BN>(s1, s2, red, cv, colvalid, lane);
  __syncthreads();
  if (tid < BN && n0 + tid < a.N) {
    const size_t rep = (size_t)(blockIdx.x & (STAT_REPS - 1)) * a.stat_stride;
    atomic_add_f64(a.red1 + rep + n0 + tid, red[fold_slot<NCV, SLOT>(0, tid)]);
    atomic_add_f64(a.red2 + rep + n0 + tid, red[fold_slot<NCV, SLOT>(1, tid)]);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// cvd_kernel<T, 64, true> - the head's stride-2 data gradient (the 3x3 convolution over the nearest-x2 upsampled decoder output,
// reference M:120, M:126-127; 16 merged taps over the 64-channel full-resolution gradient) - at THREE workgroups per CU (round 5).
// Measured: the stretches of a one-tile workgroup add up (halo wait, 16 weight stages with a barrier each, fp32 staging, the
// epilogue's dependent loads) and neither the weight stream nor the bytes bound it (a tile twice as wide under one weight walk took
// twice as long, ablations.txt); what hides such stretches is another resident workgroup - a third one was worth 20-25 % on both
// factor forms of wg5.hip.  cvd_kernel holds two: 76.5 KB of LDS (a halo image sized for 128-channel groups, fp32 staging of the whole
// 128 x 128 tile) and 202 registers (the epilogue's x / old-gradient rows prefetched under the staging).  Here:
//   * the halo image of the 64-channel gradient is 153 pixels x 128 bytes WITHOUT the padding slot: slot s of halo pixel p sits at
//     p * 128 + ((s ^ ((p >> 1) & 7)) << 4) - the 16 pixels of a fragment read (consecutive p) hit 16 different 16-byte slots of the
//     256-byte bank period: the two parities of p take the halves, (p >> 1) & 7 permutes the slots inside a half -, 19.1 KB;
//   * the fp32 staging runs in two column halves of 64 (34.8 KB over the dead images) with the epilogue of a half behind each;
//   * the weights stream through a RING of four 8 KB chunk slots (the 32 KB of the former two stage buffers) filled by LDS-DMA
//     (isa.h lds_dma16; the XOR swizzle of the B image on the per-lane SOURCE address) three chunks ahead of their use, across tap,
//     group and class boundaries: the walk is one flat sequence of chunks, a cursor names the source of the next one.  One raw
//     barrier per chunk behind a COUNTED wait (vm_lds_barrier_n): the chunk about to be multiplied has landed, the two behind it
//     and the next halo stay in flight; the refill of the slot just released is issued right behind the barrier (every fragment
//     read of it has returned: lgkmcnt(0) in the same asm statement, conv3.hip's rule).  Formerly a stage's weights went through 16
//     registers one stage ahead and every stage barrier was __syncthreads() - vmcnt(0): each stage began with a memory latency, and
//     the next halo was drained at the first stage barrier behind its issue.  The halo loads are still plain loads that hipcc counts:
//     its wait for them at the top of a group (vmcnt(0) as far as it knows) also retires the ring's two or three requests in flight -
//     once per group, not per stage; exact there would be gload16 loads with DMM_VM_WAIT(4) (isa.h) - not built;
//   * the 16 registers the ring frees hold the epilogue's x rows of the first column half, requested behind the LAST refill of the
//     walk - three chunks of MFMAs in front of the staging - and counted by the walk's last three barriers; the second half's x flies
//     under the first half's arithmetic; the old gradient of a half (a.accumulate) is requested in front of that half's staging (under
//     the walk with x it spilled: 36 bytes of scratch in the ConvTranspose form).
// Round 10, alone at 4 x 1280 x 1920 / the stages of C2 b4 (us, parent -> ring): head 1009 -> 905, TC_1 212 -> 208, TC_2 190 -> 186,
// TC_3 213 -> 202; three slots of a 16 KB stage at two workgroups per CU instead: 993 / 243 / 201 / 216 (profiles/r10/ablations.txt).
// 52.9 KB of LDS; 168 (head) / 166 (ConvTranspose form) registers, no AGPRs, no scratch: three workgroups per CU.  Same K order and
// epilogue arithmetic per output element as
// cvd_kernel: gradients bit-equal, the BatchNorm sums equal up to the grouping of their fp32 partials (rows per thread: 4 instead of 8).
#ifndef CVD3_DBG
#define CVD3_DBG 0  // timing experiments only (tools/build_variant.sh ... -DCVD3_DBG=n; the shipped library carries no switch): 1 every
#endif              // chunk multiplies the first chunk's weights, no weight request after the prologue's; 2 no halo after the first; 4 no epilogue
constexpr int C3D_NHP = CP_HH * CP_HW;                       // 153 halo pixels
constexpr int C3D_X_BYTES = C3D_NHP * 128;                   // 19 584
constexpr int C3D_CHUNK = CP_BN * 64;                        // 8 KB: 32 values of K for 128 columns
constexpr int C3D_STEP = 1;                                  // chunks per barrier
constexpr int C3D_RING = 4;                                  // ring slots (of one chunk)
constexpr int C3D_AHEAD = C3D_RING / C3D_STEP - 1;           // a step's weights are requested this many steps ahead
constexpr int C3D_PW = C3D_CHUNK / 1024 / (NTHREADS / 64);   // LDS-DMA requests per wave and chunk: 2
constexpr int C3D_WCUR = (C3D_AHEAD - 1) * C3D_STEP * C3D_PW;  // requests that stay in flight across a step barrier: 4
constexpr int C3D_MAIN = C3D_X_BYTES + C3D_RING * C3D_CHUNK; // 52 352
constexpr int C3D_LDS = C3D_MAIN + BM * 4;                   // + rowpix
constexpr int C3D_FP = 64 + 4;                               // staging pitch (floats) of a column half
constexpr int C3D_RED = BM * C3D_FP * 4;                     // offset of the fp64 sums inside the dead images
static_assert(C3D_RED + 2 * 128 * 8 <= C3D_MAIN, "staging of a column half + the fp64 sums fit the operand images");
static_assert(3 * C3D_LDS <= 160 * 1024, "three workgroups per CU");
static_assert(C3D_RING * C3D_CHUNK == 2 * CP_B_STAGE && C3D_RING % C3D_STEP == 0 && C3D_AHEAD >= 2, "ring geometry");

// vm_lds_barrier<n> (isa.h) for an n that is a constant only after unrolling
__device__ __forceinline__ void vm_lds_barrier_n(int n) {
  switch (n) {
    case 0: vm_lds_barrier<0>(); break;
    case 2: vm_lds_barrier<2>(); break;
    case 4: vm_lds_barrier<4>(); break;
    case 6: vm_lds_barrier<6>(); break;
    case 8: vm_lds_barrier<8>(); break;
    case 10: vm_lds_barrier<10>(); break;
    case 12: vm_lds_barrier<12>(); break;
    default: vm_lds_barrier<0>(); break;
  }
}

// UP2: the head's 16 merged taps (four per class) over ONE 64-channel group; !UP2: a ConvTranspose stage's nine taps (1, 2, 2, 4 per class)
// over C / 64 channel groups (cvd_kernel<T, 128, false> walks them in groups of 128: 256 registers, 76.5 KB)
template <typename T, bool UP2>
__global__ __launch_bounds__(NTHREADS, 3) void cvd3_kernel(const CvdArgs g) {
  static_assert(sizeof(T) == 2, "16-bit storage");
  typedef typename TT<T>::vec V;
  constexpr int SLOT = 8, BN = CP_BN, NT = BN / 32;
  constexpr int CSL = 8, PSTEP = NTHREADS / CSL;           // 8 slot columns of a halo pixel, 32 halo pixels between a thread's slots
  constexpr int NX = (C3D_NHP + PSTEP - 1) / PSTEP;        // 5
  const ConvArgs& a = g.c;
  const Seg& sy = a.seg[0];  // dY (materialised gradient), taps at stride 2

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Xs = smem;
  unsigned char* Bs = smem + C3D_X_BYTES;
  int* rowpix = (int*)(smem + C3D_MAIN);
  double* red = (double*)(smem + C3D_RED);  // [2 halves][16 values][8 slot columns] fp64; zeroed after the K loop

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int ntile = lbid % g.ntn;
  int tile = lbid / g.ntn;
  const int tx_i = tile % g.tiles_x; tile /= g.tiles_x;
  const int ty_i = tile % g.tiles_y;
  const int b = tile / g.tiles_y;
  const int y0 = ty_i * CP_TH, x0 = tx_i * CP_TW, n0 = ntile * BN;

  if (tid < BM) {
    const int y = y0 + (tid >> 4), x = x0 + (tid & 15);
    rowpix[tid] = (y < a.Ho && x < a.Wo) ? (b * a.Hout + y) * a.Wout + x : -1;
  }
  const int cx = tid % CSL, px0 = tid / CSL;
  const T* ysrc = (const T*)sy.src + cx * SLOT;
  V rx[NX];
  // class (pa, pb): sub-grid pixel (y', x') = dY[2 y' + pa, 2 x' + pb]; its halo starts at (y0 - pa, x0 - pb)
  auto issue_halo = [&](int pa, int pb, int grp, unsigned& ok) {
    ok = 0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int hp = px0 + PSTEP * i;
      const int hy = hp / CP_HW, hx = hp - hy * CP_HW;
      const int y = 2 * (y0 - pa + hy) + pa, x = 2 * (x0 - pb + hx) + pb;
      if (hp < C3D_NHP && (unsigned)y < (unsigned)sy.Hs && (unsigned)x < (unsigned)sy.Ws) ok |= 1u << i;
      const size_t pix = (size_t)(b * sy.Hs + min(max(y, 0), sy.Hs - 1)) * sy.Ws + min(max(x, 0), sy.Ws - 1);
      rx[i] = *(const V*)(ysrc + pix * sy.ld + grp * 64);
    }
  };
  auto store_halo = [&](unsigned ok) {
    V z;
#pragma unroll
    for (int e = 0; e < SLOT; ++e) z[e] = (T)0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int hp = px0 + PSTEP * i;
      if (hp < C3D_NHP) *(V*)(Xs + hp * 128 + ((cx ^ ((hp >> 1) & 7)) << 4)) = ((ok >> i) & 1) ? rx[i] : z;
    }
  };

  const T* wp = (const T*)a.wpack;
  const int cpt = sy.Cpad / 32;
  const int ngrp = UP2 ? 1 : sy.C / 64;   // (the head: one group, known to the compiler - the walk is then straight-line code)
  // ---- weights: a chunk = 128 columns x 64 bytes = 8 x 1 KB LDS-DMA pieces of 16 columns, wave w issues pieces 2 w and 2 w + 1.  Lane l
  // of a piece writes the 16 bytes at l * 16: column l >> 2, slot l & 3 of the image, which holds slot (l & 3) ^ ((column >> 2) & 3) of
  // the source (the swizzle the fragment reads undo).  The cursor (q_*) walks class -> group -> tap -> chunk, one chunk per request.
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const unsigned wdst0 = __builtin_amdgcn_readfirstlane(lds0 + C3D_X_BYTES + wave * (C3D_PW * 1024));
  const T* wsrc = wp + (size_t)n0 * 32 + (wave * (C3D_PW * 16) + (lane >> 2)) * 32 + (((lane & 3) ^ ((lane >> 4) & 3)) << 3);
  const size_t wchunk = (size_t)a.Npad * 32;   // elements from a chunk to the next
  int q_cls = 0, q_grp = 0, q_tt = 0, q_uu = 0, q_first = 0, q_slot = 0;
  int q_c0 = g.tapidx[0] * cpt;   // first chunk of the cursor's tap (read when the cursor enters the tap: a step before it is used)
  auto issue_w = [&]() {   // the next chunk of the walk -> the next slot of the ring; nothing behind the last chunk
    if (q_cls < 4) {
      const T* s = wsrc + (size_t)(q_c0 + q_grp * 2 + q_uu) * wchunk;
      const unsigned dst = wdst0 + q_slot * C3D_CHUNK;
#pragma unroll
      for (int q = 0; q < C3D_PW; ++q) lds_dma16(s + q * (16 * 32), dst + q * 1024);
      q_slot = q_slot + 1 == C3D_RING ? 0 : q_slot + 1;
      if (++q_uu == 2) {
        q_uu = 0;
        const int nt = UP2 ? 4 : ((q_cls >> 1) + 1) * ((q_cls & 1) + 1);
        if (++q_tt == nt) {
          q_tt = 0;
          if (++q_grp == ngrp) { q_grp = 0; ++q_cls; q_first += nt; }
        }
        if (q_cls < 4) q_c0 = g.tapidx[q_first + q_tt] * cpt;
      }
    }
  };

  const int hpl = (2 * wave + (r >> 4)) * CP_HW + (r & 15);   // this lane's halo pixel of tap (0, 0)
  const int bsw = (r >> 2) & 3;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // ---- the epilogue's operands: x and, when accumulating, the old gradient of this thread's 4 rows of a column half.  Every load is
  // issued by every lane (a row or column outside the picture reads row 0 / column n0 and is not used): the number of requests
  // behind the walk's last refill is then the same in every wave, and the walk's last barriers count them (below).
  constexpr int NCV = 64 / SLOT, RPP = NTHREADS / NCV, NIT = BM / RPP;   // 8 slot columns x 32 row phases, 4 rows per thread
  const int cv = tid % NCV, rr = tid / NCV;
  const T* bx = (const T*)a.bx;
  T* gout = (T*)a.out;
  const bool accum = a.accumulate != 0;
  V xpre[2][NIT], gpre[2][NIT];
  auto issue_x = [&](int ch) {
    const int n = n0 + 64 * ch + cv * SLOT;
    const int nn = n < a.N ? n : n0;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      xpre[ch][i] = *(const V*)(bx + (size_t)max(rowpix[rr + RPP * i], 0) * a.ldbx + nn);
    }
  };
  auto issue_g = [&](int ch) {
    const int n = n0 + 64 * ch + cv * SLOT;
    const int nn = n < a.N ? n : n0;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
#pragma unroll
      for (int e = 0; e < SLOT; ++e) gpre[ch][i][e] = (T)0;
      if (accum) gpre[ch][i] = *(const V*)(gout + (size_t)max(rowpix[rr + RPP * i], 0) * a.ldo + nn);
    }
  };

  // flat walk: class -> channel group of 64 -> tap of the class -> chunk.  Chunk c of the walk sits in ring slot c % C3D_RING; a step
  // (C3D_STEP chunks) is: the counted barrier, the refill C3D_AHEAD steps ahead into the slots the barrier released, the MFMAs.
  // The taps' halo offsets, class by class, in scalar registers before the walk: a 16-bit load is a vector-memory request, and the
  // wait for one inside the walk drains the ring.  Tap k of class (pa, pb): row offset (dy + pa) / 2, likewise the column.
  constexpr int NTAPS = UP2 ? 16 : 9;
  int toff[NTAPS];
#pragma unroll
  for (int k = 0; k < NTAPS; ++k) {
    const int kc = UP2 ? k >> 2 : (k < 1 ? 0 : k < 3 ? 1 : k < 5 ? 2 : 3);
    const int tw = sy.taps[g.tapidx[k]];
    const int dy = (int)(signed char)(tw & 0xff), dx = (int)(signed char)((tw >> 8) & 0xff);
    toff[k] = __builtin_amdgcn_readfirstlane(((dy + (kc >> 1)) >> 1) * CP_HW + ((dx + (kc & 1)) >> 1));
  }
  int c_slot = 0;
  int first_tap = 0;
  unsigned ok_cur = 0;
  issue_halo(0, 0, 0, ok_cur);
#pragma unroll
  for (int i = 0; i < C3D_AHEAD * C3D_STEP; ++i) issue_w();
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int pa = cls >> 1, pb = cls & 1;
    const int ntap = UP2 ? 4 : (pa + 1) * (pb + 1);
    for (int grp = 0; grp < ngrp; ++grp) {
      const bool last_grp = grp + 1 == ngrp;
      const bool final = cls == 3 && last_grp;   // the last group of the walk: the ring runs empty, the epilogue's operands are requested
      if (!(CVD3_DBG & 2) || (cls == 0 && grp == 0)) store_halo(ok_cur);
      // the next halo - next group of this class, or group 0 of the next class - flies under this group's steps
      if (!final && !(CVD3_DBG & 2)) {
        const int ncls = last_grp ? cls + 1 : cls;
        issue_halo(ncls >> 1, ncls & 1, last_grp ? 0 : grp + 1, ok_cur);
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        if (tt < ntap) {
          const int hpt = hpl + toff[first_tap + tt];
          const unsigned char* A = Xs + hpt * 128;
          const int asw = (hpt >> 1) & 7;
#pragma unroll
          for (int uu = 0; uu < 2; ++uu) {
            if (uu % C3D_STEP == 0) {
              // Steps of this group behind this one.  In flight across the barrier: the requests of the min(rem, AHEAD - 1) steps
              // behind this one - the cursor stops at the end of the walk, so the final group's last steps have fewer - and, behind
              // the last refill (rem < AHEAD of the final group), the epilogue's 4 or 8.  Requests the compiler counts itself (the
              // halo) are younger than a step's weights only by being issued later: they can make this wait stricter, never laxer.
              const int rem = (2 * ntap - 1 - (2 * tt + uu)) / C3D_STEP;
              if (CVD3_DBG & 1) vm_lds_barrier<0>();
              else if (final && rem < C3D_AHEAD) {
                const int nw = (rem < C3D_AHEAD - 1 ? rem : C3D_AHEAD - 1) * C3D_STEP * C3D_PW;
                vm_lds_barrier_n(nw + NIT);
              } else vm_lds_barrier<C3D_WCUR>();
              if (!(CVD3_DBG & 1)) {
#pragma unroll
                for (int i = 0; i < C3D_STEP; ++i) issue_w();
              }
              if (final && rem == C3D_AHEAD) issue_x(0);   // behind the walk's last refill
            }
            const unsigned char* B = Bs + ((CVD3_DBG & 1) ? uu % C3D_STEP : c_slot) * C3D_CHUNK;
            c_slot = c_slot + 1 == C3D_RING ? 0 : c_slot + 1;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const V av = *(const V*)(A + (((uu * 4 + s * 2 + h) ^ asw) << 4));
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                const V bv = *(const V*)(B + (32 * t + r) * 64 + (((2 * s + h) ^ bsw) << 4));
                acc[t] = mma16(av, bv, acc[t]);
              }
            }
          }
        }
      }
      lds_barrier();  // every wave is done with this halo image (and, behind the final group, with the ring: its last barrier waited for every request)
    }
    first_tap += ntap;
  }

  // ---- epilogue in two column halves: fused BN+ReLU backward (see cvd_kernel / igemm.hip) ----
  if ((CVD3_DBG & 4) && acc[0][0] + acc[1][1] + acc[2][2] + acc[3][3] != 123.f) return;
  issue_g(0);                         // the old gradient of the first half flies under the staging
  if (tid < 2 * 128) red[tid] = 0.0;  // (the K loop ended with a barrier: the images are dead)
  float* Cs = (float*)smem;  // fp32 staging: the ReLU mask and the reductions see the unrounded gradient
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    if (ch) lds_barrier();  // the first half's staging has been read
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
        Cs[row * C3D_FP + 32 * tt + r] = acc[2 * ch + tt][i];
      }
    lds_barrier();
    if (ch == 0) issue_x(1);   // the second half's x flies under the first half's arithmetic
    const int n = n0 + 64 * ch + cv * SLOT;
    const bool colvalid = n < a.N;
    float s1[SLOT], s2[SLOT], sc[SLOT], sh[SLOT], mu[SLOT], is[SLOT];
#pragma unroll
    for (int e = 0; e < SLOT; ++e) { s1[e] = 0.f; s2[e] = 0.f; sc[e] = 0.f; sh[e] = 0.f; mu[e] = 0.f; is[e] = 0.f; }
    if (colvalid) {
      load_f32s<SLOT>(a.bscale + n, sc); load_f32s<SLOT>(a.bshift + n, sh);
      load_f32s<SLOT>(a.bmean + n, mu); load_f32s<SLOT>(a.binvstd + n, is);
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int row = rr + RPP * i;
      const int pix = colvalid ? rowpix[row] : -1;
      if (pix < 0) continue;
      const V xv = xpre[ch][i], gv = gpre[ch][i];
      float av[SLOT], xf[SLOT], gf[SLOT];
#pragma unroll
      for (int e = 0; e < SLOT; e += 4) {
        const f32x4 t4 = *(const f32x4*)(Cs + row * C3D_FP + cv * SLOT + e);
        av[e] = t4[0]; av[e + 1] = t4[1]; av[e + 2] = t4[2]; av[e + 3] = t4[3];
      }
      vec_to_f32<T>(xv, xf);
      vec_to_f32<T>(gv, gf);  // zeros unless accumulating
#pragma unroll
      for (int e = 0; e < SLOT; ++e) {
        const float dz = (fmaf(xf[e], sc[e], sh[e]) > 0.f) ? av[e] : 0.f;
        s1[e] += dz;
        s2[e] = fmaf(dz, (xf[e] - mu[e]) * is[e], s2[e]);
        gf[e] += sc[e] * dz;
      }
      *(V*)(gout + (size_t)pix * a.ldo + n) = f32_to_vec<T>(gf);
    }
    if (ch == 0) issue_g(1);     // (its registers are the first half's: the old gradient of the second half flies under the staging)
    fold_to_lds<NCV, SLOT, 64>(s1, s2, red + ch * 128, cv, colvalid, lane);
  }
  lds_barrier();
  if (tid < BN && n0 + tid < a.N) {
    const size_t rep = (size_t)(blockIdx.x & (STAT_REPS - 1)) * a.stat_stride;
    const double* rh = red + (tid >> 6) * 128;
    atomic_add_f64(a.red1 + rep + n0 + tid, rh[fold_slot<NCV, SLOT>(0, tid & 63)]);
    atomic_add_f64(a.red2 + rep + n0 + tid, rh[fold_slot<NCV, SLOT>(1, tid & 63)]);
  }
}

// the wave-specialised form of the forward (cvw.hip, round 5): noted as IMPL_CVW beside IMPL_CVP when it runs
bool cvw_resolve(const ConvArgs& a, int dtype, const int* ph_dymin, const int* ph_dxmin, Resolved& r);
hipError_t cvw_launch(const Resolved& r, hipStream_t st);
static const bool g_cvw = !lab_flag("DMM_NO_CVW");
constexpr int CVP_FORM_CVD = -1;   // Resolved::form of the data gradient (0: this file's forward kernels, IMPL_CVW: cvw.hip's)

static bool cvp_tap_box(const short* taps, int ntaps, int& dymin, int& dxmin) {
  int dymax = -128, dxmax = -128;
  dymin = 127; dxmin = 127;
  for (int t = 0; t < ntaps; ++t) {
    const int dy = (int)(signed char)(taps[t] & 0xff), dx = (int)(signed char)((taps[t] >> 8) & 0xff);
    dymin = dy < dymin ? dy : dymin; dymax = dy > dymax ? dy : dymax; dxmin = dx < dxmin ? dx : dxmin; dxmax = dx > dxmax ? dx : dxmax;
  }
  return dymax - dymin <= 1 && dxmax - dxmin <= 1;
}

static bool cvd_resolve(const ConvArgs& a, int dtype, Resolved& r);
template <typename G> static void cvp_tiles(const ConvArgs& a, G& g) {   // the launch and its pixel / column tiles (CvpArgs, CvdArgs)
  g.c = a;
  g.tiles_y = (a.Ho + CP_TH - 1) / CP_TH;
  g.tiles_x = (a.Wo + CP_TW - 1) / CP_TW;
  g.ntn = a.Npad / CP_BN;
}

// Takes a forward launch (EPI_STORE) with one plain segment of a multiple of 128 BN+ReLU-normalised input channels whose 1, 2 or
// 4 taps lie in a 2x2 box, a multiple of 128 padded output columns, 16-bit storage - in cvw.hip's form where that accepts the launch,
// else in this file's - and the stride-2 data gradients (EPI_BNBWD: cvd_resolve).  Refused otherwise.
bool cvp_resolve(const ConvArgs& a, int dtype, int epi, Resolved& r) {
  if (dtype == DT_F32) return false;
  if (epi == EPI_BNBWD) return cvd_resolve(a, dtype, r);
  if (epi != EPI_STORE || a.nseg != 1 || a.pool2) return false;
  const Seg& x = a.seg[0];
  if (x.mode != G_PLAIN || x.istride != 1 || x.Hs != a.Ho || x.Ws != a.Wo || x.scale == nullptr || x.C % CP_CA || x.Cpad != x.C)
    return false;
  const bool f16t = dtype == DT_F16;
  if (a.nphase != 0) {   // the parity phases of a ConvTranspose in one launch
    if (a.nphase != 4 || a.ostride != 2 || a.Npad % CP_BN || a.out == nullptr) return false;
    int nt[4], dy4[4], dx4[4];
    for (int ph = 0; ph < 4; ++ph) {
      nt[ph] = a.ph_ntaps[ph];
      if ((nt[ph] != 1 && nt[ph] != 2 && nt[ph] != 4) || a.ph_wpack[ph] == nullptr || !cvp_tap_box(a.ph_taps0[ph], nt[ph], dy4[ph], dx4[ph]) ||
          a.ph_py[ph] < 0 || a.ph_py[ph] > 1 || a.ph_px[ph] < 0 || a.ph_px[ph] > 1)
        return false;
    }
    if (g_cvw && cvw_resolve(a, dtype, dy4, dx4, r)) { r.form = IMPL_CVW; return true; }
    LdsLaunch<CvpArgs>& l = r.put<LdsLaunch<CvpArgs>>();
    CvpArgs& g = l.g;
    for (int ph = 0; ph < 4; ++ph) { g.ph_dymin[ph] = (signed char)dy4[ph]; g.ph_dxmin[ph] = (signed char)dx4[ph]; }
    cvp_tiles(a, g);
    g.dymin = g.dxmin = 0;
    g.per = a.B * g.tiles_y * g.tiles_x * g.ntn;
    g.per8 = (g.per + 7) / 8;
    int idx[4] = {0, 1, 2, 3};
    std::stable_sort(idx, idx + 4, [&](int p, int q) { return nt[p] > nt[q]; });   // most taps first
    for (int k = 0; k < 4; ++k) g.order[k] = (signed char)idx[k];
    l.nwg = 8 * g.per8 * 4;
    l.nthreads = NTHREADS;
    l.attr_bytes = l.lds = CP_LDS;
    l.run = f16t ? launch_lds<cvp_multi_kernel<f16>, CvpArgs> : launch_lds<cvp_multi_kernel<bf16>, CvpArgs>;
    return true;
  }
  if (x.ntaps != 1 && x.ntaps != 2 && x.ntaps != 4) return false;
  if (x.ntaps == 1 && a.ostride == 1) return false;  // plain 1x1 convolutions stay with igemm's lean path
  if (a.Npad % CP_BN || a.out == nullptr) return false;
  int dymin, dxmin;
  if (!cvp_tap_box(x.taps, x.ntaps, dymin, dxmin)) return false;
  if (g_cvw && a.ostride == 2) {
    const int dy4[4] = {dymin, 0, 0, 0}, dx4[4] = {dxmin, 0, 0, 0};
    if (cvw_resolve(a, dtype, dy4, dx4, r)) { r.form = IMPL_CVW; return true; }
  }
  LdsLaunch<CvpArgs>& l = r.put<LdsLaunch<CvpArgs>>();
  CvpArgs& g = l.g;
  cvp_tiles(a, g);
  g.dymin = dymin; g.dxmin = dxmin;
  l.nwg = a.B * g.tiles_y * g.tiles_x * g.ntn;
  l.nthreads = NTHREADS;
  l.attr_bytes = l.lds = CP_LDS;
  if (f16t) {
    if (x.ntaps == 4) l.run = launch_lds<cvp_kernel<f16, 4>, CvpArgs>;
    else if (x.ntaps == 2) l.run = launch_lds<cvp_kernel<f16, 2>, CvpArgs>;
    else l.run = launch_lds<cvp_kernel<f16, 1>, CvpArgs>;
  } else {
    if (x.ntaps == 4) l.run = launch_lds<cvp_kernel<bf16, 4>, CvpArgs>;
    else if (x.ntaps == 2) l.run = launch_lds<cvp_kernel<bf16, 2>, CvpArgs>;
    else l.run = launch_lds<cvp_kernel<bf16, 1>, CvpArgs>;
  }
  return true;
}

// Stride-2 data gradients with the fused BN+ReLU backward (EPI_BNBWD): one plain segment (the materialised output gradient), the
// gradient stored (not only reduced), a multiple of 128 output columns, and either the ConvTranspose's nine taps (-1..1)^2 over
// a multiple of 128 channels or the upsampled 3x3's sixteen merged taps (-1..2)^2 over 64 channels.
static bool cvd_resolve(const ConvArgs& a, int dtype, Resolved& r) {
  const Seg& y = a.seg[0];
  if (a.nseg != 1 || a.pool2 || y.mode != G_PLAIN || y.istride != 2 || y.scale != nullptr || y.q != nullptr) return false;
  const bool up2 = y.ntaps == 16;
  if (!up2 && y.ntaps != 9) return false;
  if (y.Hs != 2 * a.Ho || y.Ws != 2 * a.Wo || y.Cpad != y.C || (up2 ? y.C != 64 : y.C % CP_CA != 0)) return false;
  if (a.Npad % CP_BN || a.out == nullptr || a.bx == nullptr || a.ostride != 1 || a.Hout != a.Ho || a.Wout != a.Wo) return false;
  LdsLaunch<CvdArgs>& l = r.put<LdsLaunch<CvdArgs>>();
  CvdArgs& g = l.g;
  int cnt[4] = {0, 0, 0, 0};
  const int base9[4] = {0, 1, 3, 5}, base16[4] = {0, 4, 8, 12};
  for (int t = 0; t < y.ntaps; ++t) {
    const int dy = (int)(signed char)(y.taps[t] & 0xff), dx = (int)(signed char)((y.taps[t] >> 8) & 0xff);
    if (dy < -1 || dx < -1 || dy > (up2 ? 2 : 1) || dx > (up2 ? 2 : 1)) return false;
    const int cls = (dy & 1) * 2 + (dx & 1);
    const int cap = up2 ? 4 : (cls == 0 ? 1 : (cls == 3 ? 4 : 2));
    if (cnt[cls] >= cap) return false;
    g.tapidx[(up2 ? base16 : base9)[cls] + cnt[cls]++] = t;
  }
  cvp_tiles(a, g);
  l.nwg = a.B * g.tiles_y * g.tiles_x * g.ntn;
  l.nthreads = NTHREADS;
  static const bool three = !lab_flag("DMM_NO_CVD3");
  static const bool three_ct = !lab_flag("DMM_NO_CVD3_CT");
  const bool f16t = dtype == DT_F16;
  l.attr_bytes = l.lds = CP_LDS;
  if (up2 && three) { l.attr_bytes = l.lds = C3D_LDS; l.run = f16t ? launch_lds<cvd3_kernel<f16, true>, CvdArgs> : launch_lds<cvd3_kernel<bf16, true>, CvdArgs>; }
  else if (!up2 && three && three_ct) { l.attr_bytes = l.lds = C3D_LDS; l.run = f16t ? launch_lds<cvd3_kernel<f16, false>, CvdArgs> : launch_lds<cvd3_kernel<bf16, false>, CvdArgs>; }
  else if (up2) l.run = f16t ? launch_lds<cvd_kernel<f16, 64, true>, CvdArgs> : launch_lds<cvd_kernel<bf16, 64, true>, CvdArgs>;
  else l.run = f16t ? launch_lds<cvd_kernel<f16, 128, false>, CvdArgs> : launch_lds<cvd_kernel<bf16, 128, false>, CvdArgs>;
  r.form = CVP_FORM_CVD;
  return true;
}

hipError_t cvp_launch(const Resolved& r, hipStream_t st) {
  if (r.form == IMPL_CVW) {
    note_impl(IMPL_CVW);   // (beside IMPL_CVP, which the dispatcher notes: the family is cvp, this says which form ran)
    return cvw_launch(r, st);
  }
  return r.form == CVP_FORM_CVD ? r.get<LdsLaunch<CvdArgs>>().go(st) : r.get<LdsLaunch<CvpArgs>>().go(st);
}

}  // namespace dmm
