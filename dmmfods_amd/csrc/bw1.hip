// Backward of the dense layers' 1x1 bottleneck convolution (torchvision _DenseLayer.conv1: C_in -> 128 channels behind norm1 + ReLU;
// reference call sites M:85-92, M:169-176) - data gradient AND weight gradient in one pass.  gfx950, 16-bit storage types.
//
//   G   = g + q + r*y            the bottleneck's effective gradient (128 channels), read ONCE
//   dX  = G W                    data gradient, fused with norm1's backward:  dz = dX * [bn1(x) > 0],  g_x (+)= s*dz,  sum dz, sum dz*xhat
//   dW  = G^T relu(bn1(x))       weight gradient, accumulated in registers over the workgroup's rows
// The two generic kernels (igemm.hip EPI_BNBWD on the main stream, wgrad.hip on the side stream) each read G, y and x: three
// tensors of the layer twice, 37 % of the pair's HBM traffic on a pair that is HBM-bound (43 flop per byte).  Here a persistent
// workgroup owns a 128-channel slice of C_in and a range of 64-pixel row tiles; per tile x and G go to LDS once (prologues once per
// element), the data-gradient GEMM reads G rows and the resident weight slice, the weight-gradient GEMM reads both images with
// the transposing read ds_read_b64_tr_b16 (contraction over pixels, as wgrad.hip), the fp32 tile is staged over the dead images and
// finished in the slot layout the loads came in - the raw x of the ReLU mask is still in the loading thread's registers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "dispatch.h"
#include "gather.h"
#include "isa.h"
#include "pointwise.h"

namespace dmm {

#ifndef B1_DBG
#define B1_DBG 0  // timing experiments only (tools/build_variant.sh ... -DB1_DBG=n): 1 no weight-gradient atomics, 2 no weight-gradient
                  // GEMM, 4 no data-gradient GEMM, 8 no epilogue (staging, norm1 backward, store), 16 every load hits row 0,
                  // 32 the old gradient is not read (as if not accumulating), 64 the gradient is not stored
#endif
// Tried on the tile loop and measured as no gain (profiles/r03/ablations.txt, profiles/r04/ablations.txt): the next tile's loads
// requested behind the GEMMs and the old gradient, with raw LDS-only barriers from there to the end of the tile; non-temporal hints on
// the x / old-gradient loads and on the gradient store.
constexpr int B1_TM = 64;                       // pixels per tile
constexpr int B1_NB = 128;                      // bottleneck channels (K of the data gradient, N of the weight gradient)
constexpr int B1_CT = 128;                      // input channels per workgroup
constexpr int B1_IMG = B1_TM * 256;             // 16 KB: 64 rows x 256 bytes, slots permuted per row (b1_swz)
constexpr int B1_W = 4 * B1_CT * 64;            // 32 KB: the weight slice [chunk][c][32 n], igemm's B image
constexpr int B1_STAGE = B1_TM * B1_CT * 4;     // fp32 tile over the two operand images
static_assert(B1_STAGE == 2 * B1_IMG, "staging aliases the operand images exactly");
constexpr int B1_LDS = 2 * B1_IMG + B1_W + 2 * B1_CT * 8 + 6 * B1_CT * 4;  // + fp64 reduction scratch + per-channel constants

// Physical 16-byte slot of (row, slot) in a 256-byte image row.  The images are read two ways: 16 rows x one slot (ds_read_b128
// fragments of the data-gradient GEMM) and 4 consecutive rows x 32 contiguous bytes (ds_read_b64_tr_b16 of the weight-gradient
// GEMM).  The 64-byte granule is XOR-ed with (row & 3), the slot inside it with (row >> 2) & 3: 16 rows hit 16 different slots, 4
// consecutive rows 4 different granules, and a 32-byte span stays inside its granule.  Rows 16 apart share the permutation.
__device__ __forceinline__ int b1_swz(int row, int slot) { return ((((slot >> 2) ^ (row & 3)) << 2) | ((slot & 3) ^ ((row >> 2) & 3))); }

// PQ = prologue of G: 0 none (materialised gradient), 2 effective gradient.  ACC = the gradient of x is accumulated (an earlier
// consumer of the block buffer has already written it).
template <typename T, int PQ, bool ACC_, bool PART>
__global__ __launch_bounds__(NTHREADS, 2) void bw1_kernel(const Bw1Args g) {
  constexpr bool ACC = ACC_ && !(B1_DBG & 32);
  constexpr bool UNC = std::is_same<T, f16>::value;  // the second per-channel sum is taken uncentred and centred once per workgroup (f16 epilogue)
  static_assert(sizeof(T) == 2, "16-bit storage");
  typedef typename TT<T>::vec V;
  constexpr int SLOT = 8;
  constexpr int NL = B1_TM * 16 / NTHREADS;  // 4 slots per thread and operand
  const ConvArgs& a = g.c;
  const Seg& sg = a.seg[0];  // G: the bottleneck gradient (+ y, q, r)

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Ai = smem;                 // relu(bn(x)) [64 px][128 c]
  unsigned char* Gi = smem + B1_IMG;        // G [64 px][128 n]
  unsigned char* Wi = smem + 2 * B1_IMG;    // weight slice
  double* red = (double*)(smem + 2 * B1_IMG + B1_W);
  float* kc = (float*)(smem + 2 * B1_IMG + B1_W + 2 * B1_CT * 8);  // [scale | shift | mean | invstd | q | r] x 128

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  // Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each with its own L2.  The nct workgroups that walk the same rows
  // (one per 128-channel slice) all read the same G and y tiles: they get consecutive slots of ONE XCD, so the tiles come from HBM once.
  // (Launches with few row ranges keep the plain order: rounding them up to groups of 8 costs more than the re-reads.)
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int ct = g.xcd_group ? q % g.nct : (int)(blockIdx.x % g.nct);
  const int split = g.xcd_group ? (q / g.nct) * 8 + xcd : (int)(blockIdx.x / g.nct);
  const int c0 = ct * B1_CT;
  const int t_beg = split * g.tiles_per_wg, t_end = min(g.ntiles, t_beg + g.tiles_per_wg);
  if (t_beg >= t_end) return;

  // ---- this thread's slots: column cs (8 channels), rows p0 + 16 i of the tile; the same mapping loads and finishes a tile ----
  const int cs = tid & 15, p0 = tid >> 4;
  const int cx = c0 + cs * SLOT;          // input channel of the x / gradient slot
  const bool cvalid = cx < a.N;
  // the per-channel constants - norm1's scale / shift / mean / invstd of this channel slice, q / r of G - live in LDS and are read
  // where a tile needs them: held in registers across the MFMA phases they spill the accumulators
  if (tid < B1_CT) {
    const int c = c0 + tid;
    const bool v = c < a.N;
    kc[tid] = v ? a.bscale[c] : 0.f; kc[B1_CT + tid] = v ? a.bshift[c] : 0.f;
    kc[2 * B1_CT + tid] = v ? a.bmean[c] : 0.f; kc[3 * B1_CT + tid] = v ? a.binvstd[c] : 0.f;
    kc[4 * B1_CT + tid] = PQ == 2 ? sg.q[tid] : 0.f; kc[5 * B1_CT + tid] = PQ == 2 ? sg.r[tid] : 0.f;
  }
  // uniform base pointers (scalar registers) + 32-bit per-lane byte offsets: four 64-bit per-lane pointers were the registers that
  // spilled the <effective gradient, accumulate> variant (the launcher checks that every operand spans < 4 GiB)
  const unsigned char* xbase = (const unsigned char*)a.bx;
  const unsigned char* gbase = (const unsigned char*)sg.src;
  const unsigned char* ybase = (const unsigned char*)sg.src2;
  unsigned char* obase = (unsigned char*)a.out;
  const unsigned xcol = (unsigned)(cvalid ? cx : 0) * 2u, gcol = (unsigned)(cs * SLOT) * 2u;
  const unsigned xpitch = (unsigned)a.ldbx * 2u, gpitch = (unsigned)sg.ld * 2u, ypitch = (unsigned)sg.ld2 * 2u, opitch = (unsigned)a.ldo * 2u;
  // (p0 + 16 i keeps p & 15, hence the row's slot permutation: the four LDS addresses of a thread are base + 4096 i)
  const int lds0 = p0 * 256 + (b1_swz(p0, cs) << 4);

  // ---- the weight slice, once: chunks of 32 bottleneck channels x 128 input channels (igemm's B image, XOR swizzle) ----
  {
    const T* wp = (const T*)a.wpack;
#pragma unroll
    for (int j = 0; j < B1_W / 16 / NTHREADS; ++j) {
      const int piece = tid + NTHREADS * j;           // 16-byte piece of the slice: (chunk, row c, slot)
      const int chunk = piece >> 9, rowc = (piece >> 2) & 127, slot = piece & 3;
      const int c = c0 + rowc;
      V v;
#pragma unroll
      for (int e = 0; e < SLOT; ++e) v[e] = (T)0;
      if (c < a.Npad) v = *(const V*)(wp + ((size_t)chunk * a.Npad + c) * 32 + slot * SLOT);
      *(V*)(Wi + chunk * (B1_CT * 64) + rowc * 64 + ((slot ^ ((rowc >> 2) & 3)) << 4)) = v;
    }
  }
  if (tid < 2 * B1_CT) red[tid] = 0.0;
  __syncthreads();  // constants readable by the first tile's prologues

  V rx[NL], rg[NL], ry[PQ == 2 ? NL : 1];
  unsigned okp = 0;  // row validity of the slots in flight
  auto issue = [&](int tile) {
    okp = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {  // branch-free: clamped rows, dropped at the write
      const int m = tile * B1_TM + p0 + 16 * i;
      if (m < a.M) okp |= 1u << i;
      const unsigned mm = (B1_DBG & 16) ? 0u : (unsigned)min(m, a.M - 1);
      rx[i] = *(const V*)(xbase + (size_t)(mm * xpitch + xcol));
      rg[i] = *(const V*)(gbase + (size_t)(mm * gpitch + gcol));
      if constexpr (PQ == 2) ry[i] = *(const V*)(ybase + (size_t)(mm * ypitch + gcol));
    }
  };

  // ---- fragments ----
  // data gradient: wave w -> pixel rows 32 (w & 1) .., input channels 64 (w >> 1) ..  (2 tiles of 32 columns)
  const int dpx = 32 * (wave & 1) + r;
  const int dgoff = dpx * 256;            // + (b1_swz(dpx, slot) << 4) per k-step
  const int dcb = 64 * (wave >> 1);       // first column of this wave's half
  const int bsw = (r >> 2) & 3;
  // weight gradient: wave w -> input channels 32 w .. (rows of dP chunk c0 / 32 + w), all 128 bottleneck channels (4 tiles)
  const int tg = lane >> 4, ti = lane & 15, tq = ti >> 2, tp = ti & 3;
  const int arow = 8 * (tg >> 1) + tq;    // pixel row of the first transposing read; the second is 4 rows further
  auto tr_off = [&](int px, int colbyte) { return px * 256 + ((b1_swz(px, colbyte >> 4) << 4) | (colbyte & 15)); };
  // a k-step further down the tile is 16 rows = 4096 bytes further: the slot permutation of the row does not change
  const int acolb = (32 * wave + 16 * (tg & 1) + 4 * tp) * 2;
  // the fragment's second half sits 4 rows further: (row & 3) is unchanged and (row >> 2) & 3 goes from even to odd, i.e. the slot's
  // low bit flips: offset2 = (offset1 ^ 16) + 4 * 256 (two instructions at the use instead of five more live registers)
  const int aoff1 = tr_off(arow, acolb);
  int goff1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) goff1[j] = tr_off(arow, (32 * j + 16 * (tg & 1) + 4 * tp) * 2);
  auto second = [](int off) { return (off ^ 16) + 4 * 256; };

  f32x16 accw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) accw[j][i] = 0.f;

  issue(t_beg);
  for (int tile = t_beg; tile < t_end; ++tile) {
    // ---- operands to LDS (prologues once per element); raw x and the old gradient stay in registers for the epilogue ----
    // FULL: all 64 rows of the tile exist (every tile but possibly the launch's last) - the row-validity selects in front of the LDS
    // writes and the per-row branches of the epilogue are compiled out (a sixth of the loop's vector instructions, and the kernel is
    // bound by them: 32 MFMA = 1024 cycles against ~500 VALU = 2000 cycles per wave and tile).  Only these two stretches exist twice;
    // the GEMMs between them are shared, so the accumulators' live ranges are those of a single path.
    V xraw[NL], gold[ACC ? NL : 1];
    const bool full = (tile + 1) * B1_TM <= a.M;   // (workgroup-uniform)
    const unsigned okt = okp;
    auto stage = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
      V z;
#pragma unroll
      for (int e = 0; e < SLOT; ++e) z[e] = (T)0;
      {  // x first, then G: the two sets of per-channel constants are never live together
        SlotK<SLOT> kx;
        kx.k0 = load_fv<SLOT>(kc + cs * SLOT); kx.k1 = load_fv<SLOT>(kc + B1_CT + cs * SLOT); kx.k2 = 0.f; kx.k3 = 0.f;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          xraw[i] = rx[i];
          const bool v = FULL || ((okt >> i) & 1) != 0;
          // (channels past C_in: their scale / shift constants are zeros, relu(0 x + 0) = 0 needs no select)
          const V av_ = bn_relu_slot(rx[i], kx);
          *(V*)(Ai + lds0 + 4096 * i) = v ? av_ : z;
        }
      }
      {
        SlotK<SLOT> kg;
        kg.k0 = 0.f; kg.k1 = 0.f; kg.k2 = 0.f; kg.k3 = 0.f;
        if (PQ == 2) { kg.k0 = load_fv<SLOT>(kc + 4 * B1_CT + cs * SLOT); kg.k1 = load_fv<SLOT>(kc + 5 * B1_CT + cs * SLOT); }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          const bool v = FULL || ((okt >> i) & 1) != 0;
          V gv = rg[i];
          if constexpr (PQ == 2) gv = eff_grad_slot(rg[i], ry[i], kg);
          *(V*)(Gi + lds0 + 4096 * i) = v ? gv : z;
        }
      }
    };
    if (UNC && full) stage(std::true_type()); else stage(std::false_type());   // (bf16: the second copy spills its generic epilogue)
    __syncthreads();  // images (and, the first time, the weight slice) complete
    if (tile + 1 < t_end) issue(tile + 1);

    // ---- data gradient: dX[64 px][128 c] = G W ----
    f32x16 accd[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) accd[t][i] = 0.f;
    if (!(B1_DBG & 4))
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int slot = ch * 4 + 2 * s + h;
        const V av = *(const V*)(Gi + dgoff + (b1_swz(dpx, slot) << 4));
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const V bv = *(const V*)(Wi + ch * (B1_CT * 64) + (dcb + 32 * t + r) * 64 + (((2 * s + h) ^ bsw) << 4));
          accd[t] = mma16(av, bv, accd[t]);
        }
      }
    // ---- weight gradient: dP[c][n] += sum over the tile's pixels G[p][n] a[p][c] ----
    if (!(B1_DBG & 2))
#pragma unroll
    for (int ms = 0; ms < B1_TM / 16; ++ms) {
      const V af = frag16<T>(lds_tr16(Ai + aoff1 + ms * 4096), lds_tr16(Ai + second(aoff1) + ms * 4096));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const V gf = frag16<T>(lds_tr16(Gi + goff1[j] + ms * 4096), lds_tr16(Gi + second(goff1[j]) + ms * 4096));
        accw[j] = mma16(gf, af, accw[j]);  // rows: bottleneck channel n, columns: input channel c
      }
    }
    if constexpr (ACC) {  // the old gradient of this tile: requested behind the MFMAs (16 registers that would otherwise live across both
                          // GEMMs), needed two barriers and the staging later; the CU's other workgroup covers what is left of the latency
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const unsigned mm = (unsigned)min(tile * B1_TM + p0 + 16 * i, a.M - 1);
        gold[i] = *(const V*)(obase + (size_t)(mm * opitch + xcol));
      }
    }
    __syncthreads();  // all waves done with the images: stage the data-gradient tile over them
    if (B1_DBG & 8) {  // keep the data-gradient GEMM alive
      float sa = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) sa += accd[t][i];
      if (sa == 1.2345e33f) obase[0] = 1;
    } else {
    float* Cs = (float*)smem;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = 32 * (wave & 1) + (i & 3) + 8 * (i >> 2) + 4 * h;
        // (row bit 2 = the lane half h: rows of the upper half go to the OTHER 32 banks - columns ^ 32 - instead of on top of the lower
        // half's; the readers apply the same XOR, which keeps their 16-byte groups intact)
        Cs[row * B1_CT + ((dcb + 32 * t + r) ^ (h << 5))] = accd[t][i];
      }
    __syncthreads();
    // ---- norm1 backward in the slot layout of the loads ----
    float s1[SLOT], s2[SLOT];
#pragma unroll
    for (int e = 0; e < SLOT; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    auto finish = [&](auto full_tag) {
      constexpr bool FULL = decltype(full_tag)::value;
      float sc[SLOT], sh[SLOT], mu[UNC ? 1 : SLOT], is[UNC ? 1 : SLOT];
      load_f32s<SLOT>(kc + cs * SLOT, sc); load_f32s<SLOT>(kc + B1_CT + cs * SLOT, sh);
      if constexpr (!UNC) { load_f32s<SLOT>(kc + 2 * B1_CT + cs * SLOT, mu); load_f32s<SLOT>(kc + 3 * B1_CT + cs * SLOT, is); }
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        if (!FULL && !((okt >> i) & 1)) continue;
        const int p = p0 + 16 * i;
        float av[SLOT];
#pragma unroll
        for (int e = 0; e < SLOT; e += 4) {
          const f32x4 t4 = *(const f32x4*)(Cs + p * B1_CT + ((cs * SLOT + e) ^ (((p >> 2) & 1) << 5)));
          av[e] = t4[0]; av[e + 1] = t4[1]; av[e + 2] = t4[2]; av[e + 3] = t4[3];
        }
        const unsigned m = (unsigned)(tile * B1_TM + p);
        if constexpr (UNC) {  // f16: mixed-precision instructions on the packed halves, uncentred second sum (gather.h bnbwd_slot)
          const V ov = bnbwd_slot<ACC>(av, xraw[i], gold[ACC ? i : 0], sc, sh, s1, s2);
          if (!(B1_DBG & 64) || av[0] == 1.2345e33f) *(V*)(obase + (size_t)(m * opitch + xcol)) = ov;
        } else {
          float xf[SLOT], gf[SLOT];
          vec_to_f32<T>(xraw[i], xf);
          if constexpr (ACC) vec_to_f32<T>(gold[i], gf);
#pragma unroll
          for (int e = 0; e < SLOT; ++e) {
            const float dz = (fmaf(xf[e], sc[e], sh[e]) > 0.f) ? av[e] : 0.f;
            s1[e] += dz;
            s2[e] = fmaf(dz, (xf[e] - mu[e]) * is[e], s2[e]);
            gf[e] = (ACC ? gf[e] : 0.f) + sc[e] * dz;
          }
          if (!(B1_DBG & 64) || gf[0] == 1.2345e33f) *(V*)(obase + (size_t)(m * opitch + xcol)) = f32_to_vec<T>(gf);
        }
      }
    };
    if (cvalid) { if (UNC && full) finish(std::true_type()); else finish(std::false_type()); }
    // per-tile partials cover 4 rows per thread: fold the 4 lanes of a wave that share the slot column (lane swaps: every lane ends
    // up with 4 of the 16 finished wave totals), then fp64 in LDS - 4 LDS atomics per lane instead of 16 on a quarter of the lanes
    fold_to_lds<16, SLOT, B1_CT>(s1, s2, red, cs, cvalid, lane);
    }  // (epilogue)
    __syncthreads();  // staging read: the next tile's images may be written
  }

  // ---- results of the walk: per-channel sums (one fp64 atomic per channel and workgroup), the weight-gradient slice ----
  if (tid < B1_CT && c0 + tid < a.N) {
    const size_t rep = (size_t)(blockIdx.x & (STAT_REPS - 1)) * a.stat_stride;
    const double S1 = red[fold_slot<16, SLOT>(0, tid)];
    double S2 = red[fold_slot<16, SLOT>(1, tid)];
    if constexpr (UNC) S2 = (S2 - (double)kc[2 * B1_CT + tid] * S1) * (double)kc[3 * B1_CT + tid];  // sum dz x -> sum dz xhat
    atomic_add_f64(a.red1 + rep + c0 + tid, S1);
    atomic_add_f64(a.red2 + rep + c0 + tid, S2);
  }
  const int c = c0 + 32 * wave + r;
  if constexpr (PART) {  // this workgroup's slot, in the layout of the dpack slice (whole slot: the reduction reads all of it)
    float* slot = g.part + ((size_t)split * g.nct + ct) * B1_SLOT_FLOATS + (size_t)wave * (B1_NB * 32);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int n = 32 * j + (i & 3) + 8 * (i >> 2) + 4 * h;
        slot[n * 32 + r] = accw[j][i];
      }
  } else if (!(B1_DBG & 1) && c < g.wC) {
    const size_t chunk = (size_t)(c0 / 32 + wave);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int n = 32 * j + (i & 3) + 8 * (i >> 2) + 4 * h;
        atomic_add_f32(g.dpack + (chunk * g.dNpad + n) * 32 + r, accw[j][i]);
      }
  }
  if (B1_DBG & 1) {  // keep the weight-gradient GEMM alive
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 16; ++i) s += accw[j][i];
    if (s == 1.2345e33f) g.dpack[0] = s;
  }
}

template <typename T, int PQ, bool ACC, bool PART>
static hipError_t launch_bw1_t(const Bw1Args& g, int nwg, hipStream_t st) {
  return launch_lds<bw1_kernel<T, PQ, ACC, PART>>(B1_LDS, nwg, NTHREADS, B1_LDS, st, g);
}

// Do these two launches - the weight gradient `w` (normal form) and the data gradient `d` (EPI_BNBWD) of one convolution - form
// the pair this kernel fuses?  1x1, unit stride, 128 output channels, the same x / norm and the same gradient operand on both - and
// the family not switched off (deny: 1 << family, dispatch.h).
bool bw1_eligible(const WgradArgs& w, const ConvArgs& d, int dtype, unsigned deny) {
  if (((deny >> IMPL_BW1) & 1u) || dtype == DT_F32 || w.nseg != 1 || d.nseg != 1 || d.pool2) return false;
  const Seg& wx = w.seg[0];   // x with norm1's scale / shift
  const Seg& wg = w.dy;       // G
  const Seg& dg = d.seg[0];   // G again
  if (wx.mode != G_PLAIN || wx.istride != 1 || wx.ntaps != 1 || wx.taps[0] != 0 || wx.scale == nullptr || wx.C % 32) return false;
  if (wg.mode != G_PLAIN || wg.istride != 1 || wg.ntaps != 1 || wg.taps[0] != 0 || wg.scale != nullptr || wg.C != B1_NB) return false;
  if (dg.mode != G_PLAIN || dg.istride != 1 || dg.ntaps != 1 || dg.taps[0] != 0 || dg.scale != nullptr || dg.C != B1_NB || dg.Cpad != B1_NB) return false;
  if (dg.src != wg.src || dg.ld != wg.ld || dg.q != wg.q || dg.src2 != wg.src2) return false;
  if (w.N != B1_NB || w.Npad != B1_NB || w.M != d.M || d.N != wx.C || d.Npad % 32) return false;
  if (d.bx != wx.src || d.ldbx != wx.ld || d.bscale != wx.scale || d.bshift != wx.shift) return false;
  if (d.out == nullptr || d.ostride != 1 || d.Hout != d.Ho || d.Wout != d.Wo || wx.Hs != d.Ho || wx.Ws != d.Wo) return false;
  const double span = 2.0 * (double)d.M;  // 32-bit byte offsets inside every operand
  if (span * d.ldbx >= 4294967296.0 || span * d.ldo >= 4294967296.0 || span * dg.ld >= 4294967296.0 || span * dg.ld2 >= 4294967296.0) return false;
  return true;
}

Bw1Geom bw1_geometry(const ConvArgs& a) {
  Bw1Geom q;
  q.nct = (a.N + B1_CT - 1) / B1_CT;
  q.ntiles = (a.M + B1_TM - 1) / B1_TM;
  // A pure function of the shape: the plan's sizing pass reserves the slots from it WITHOUT a GPU (dmm_plan_create /
  // dmm_plan_workspace_bytes never touch the HIP runtime), and a launch must split exactly as the plan reserved.  The split is laid
  // out for the 256 compute units of the MI355X this library is written for.
  constexpr int cus = DESIGN_CUS;
  static const int per_cu = lab_int("DMM_BW1_PER_CU", 2);
  // every workgroup ends with 64 KB of weight gradient to hand over and a tile is ~2 us of work: at least 4 tiles per workgroup
  int nsplit = std::max(1, (per_cu * cus + q.nct - 1) / q.nct);
  nsplit = std::min(nsplit, std::max(1, q.ntiles / 4));
  q.tiles_per_wg = (q.ntiles + nsplit - 1) / nsplit;
  q.nsplit = (q.ntiles + q.tiles_per_wg - 1) / q.tiles_per_wg;   // every row range has at least one tile
  q.xcd_group = (q.nct > 1 && q.nsplit >= 32 && q.tiles_per_wg >= 8) ? 1 : 0;  // (measured: block 1-2 gain, block 3 loses)
  // whole groups of 8 row ranges (one per XCD); surplus workgroups return at once
  q.nwg = q.xcd_group ? ((q.nsplit + 7) / 8) * 8 * q.nct : q.nsplit * q.nct;
  return q;
}

static bool g_bw1_part = !lab_flag("DMM_NO_BW1_PART");

static bool bw1_uses_part(const Bw1Args& g, const Bw1Geom& q) {
  return g_bw1_part && g.part != nullptr && q.nsplit * q.nct <= g.part_slots && q.nsplit > 1;
}

hipError_t launch_bw1(const Bw1Args& g0, int dtype, hipStream_t st) {
  Bw1Args g = g0;
  const ConvArgs& a = g.c;
  if (a.M <= 0) return hipSuccess;
  const Bw1Geom q = bw1_geometry(a);
  note_impl(IMPL_BW1);
  g.nct = q.nct; g.ntiles = q.ntiles; g.tiles_per_wg = q.tiles_per_wg; g.xcd_group = q.xcd_group; g.nsplit = q.nsplit;
  const int nwg = q.nwg;
  const int pq = a.seg[0].q ? 2 : 0;
  const bool acc = a.accumulate != 0;
  const bool part = bw1_uses_part(g, q);
#define B1_GO(T) \
  (part ? (pq ? (acc ? launch_bw1_t<T, 2, true, true>(g, nwg, st) : launch_bw1_t<T, 2, false, true>(g, nwg, st))     \
              : (acc ? launch_bw1_t<T, 0, true, true>(g, nwg, st) : launch_bw1_t<T, 0, false, true>(g, nwg, st)))    \
        : (pq ? (acc ? launch_bw1_t<T, 2, true, false>(g, nwg, st) : launch_bw1_t<T, 2, false, false>(g, nwg, st))   \
              : (acc ? launch_bw1_t<T, 0, true, false>(g, nwg, st) : launch_bw1_t<T, 0, false, false>(g, nwg, st))))
  if (dtype == DT_F16) return B1_GO(f16);
  return B1_GO(bf16);
#undef B1_GO
}

// dpack slice = sum over the row ranges of the slots; the slots hold zeros for padding channels, which dpack has rows for as well
// (chunks of 32 channels) up to ceil(wC / 32) chunks: a thread owns 4 consecutive floats of a slice.
__device__ __forceinline__ void bw1_reduce_slots(const float* __restrict__ part, float* __restrict__ dpack, int nct, int nsplit, int nfloats) {
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;  // float index into the packed gradient (all slices)
  if (e >= nct * B1_SLOT_FLOATS) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  const float* p = part + e;  // slot (0, ct) starts at ct * B1_SLOT_FLOATS: the slices of one row range are contiguous
  const size_t pitch = (size_t)nct * B1_SLOT_FLOATS;
  int k = 0;
  for (; k + 16 <= nsplit; k += 16) {  // sixteen independent 16-byte loads in flight per thread: the launch has few workgroups
    f32x4 v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = __builtin_nontemporal_load((const f32x4*)(p + (size_t)(k + u) * pitch));
#pragma unroll
    for (int u = 0; u < 16; u += 4) s += (v[u] + v[u + 1]) + (v[u + 2] + v[u + 3]);
  }
  for (; k + 4 <= nsplit; k += 4) {
    const f32x4 v0 = *(const f32x4*)(p + (size_t)k * pitch), v1 = *(const f32x4*)(p + (size_t)(k + 1) * pitch);
    const f32x4 v2 = *(const f32x4*)(p + (size_t)(k + 2) * pitch), v3 = *(const f32x4*)(p + (size_t)(k + 3) * pitch);
    s += (v0 + v1) + (v2 + v3);
  }
  for (; k < nsplit; ++k) s += *(const f32x4*)(p + (size_t)k * pitch);
  if (e < nfloats) *(f32x4*)(dpack + e) = s;
}
__global__ __launch_bounds__(256) void bw1_reduce_kernel(const float* __restrict__ part, float* __restrict__ dpack, int nct, int nsplit, int nfloats) {
  bw1_reduce_slots(part, dpack, nct, nsplit, nfloats);
}
// The grouped form: blockIdx.y = member, each with its own slots, split and packed gradient; gridDim.x covers the largest member and
// the surplus workgroups of a smaller one return at once.  The table travels in the kernel argument.
struct Bw1RedGroupArgs { Bw1RedMember m[B1_RED_GROUP_MAX]; };
static_assert(sizeof(Bw1RedMember) % 8 == 0, "members are read with aligned scalar loads");
__global__ __launch_bounds__(256) void bw1_reduce_group_kernel(const Bw1RedGroupArgs g) {
  const Bw1RedMember& m = g.m[blockIdx.y];
  bw1_reduce_slots(m.part, m.dpack, m.nct, m.nsplit, m.nfloats);
}

// What the reduction of `g` adds up (false: nothing - the fused launch added into dpack itself)
static bool bw1_reduce_member(const Bw1Args& g, Bw1RedMember& m) {
  const ConvArgs& a = g.c;
  if (a.M <= 0) return false;
  const Bw1Geom q = bw1_geometry(a);
  if (!bw1_uses_part(g, q)) return false;
  m.part = g.part; m.dpack = g.dpack; m.nct = q.nct; m.nsplit = q.nsplit;
  m.nfloats = ((g.wC + 31) / 32) * g.dNpad * 32;  // size of dpack
  return true;
}

hipError_t launch_bw1_reduce_member(const Bw1RedMember& m, hipStream_t st) {
  const int nthreads = m.nct * B1_SLOT_FLOATS / 4;
  hipLaunchKernelGGL(bw1_reduce_kernel, dim3((nthreads + 255) / 256), dim3(256), 0, st, m.part, m.dpack, m.nct, m.nsplit, m.nfloats);
  return hipGetLastError();
}

hipError_t launch_bw1_reduce(const Bw1Args& g, hipStream_t st) {
  Bw1RedMember m;
  if (!bw1_reduce_member(g, m)) return hipSuccess;
  return launch_bw1_reduce_member(m, st);
}

bool bw1_reduce_group_add(Bw1RedGroup& G, const Bw1Args& g) {
  Bw1RedMember m;
  if (!bw1_reduce_member(g, m)) return true;  // nothing to add up
  if (G.n >= B1_RED_GROUP_MAX) return false;
  G.m[G.n++] = m;
  return true;
}

hipError_t bw1_reduce_group_launch(Bw1RedGroup& G, hipStream_t st) {
  if (G.n <= 0) return hipSuccess;
  Bw1RedGroupArgs a;
  memset(&a, 0, sizeof(a));
  int nct = 0;
  for (int i = 0; i < G.n; ++i) { a.m[i] = G.m[i]; nct = std::max(nct, G.m[i].nct); }
  const int n = G.n;
  G.n = 0;
  hipLaunchKernelGGL(bw1_reduce_group_kernel, dim3((nct * (B1_SLOT_FLOATS / 4) + 255) / 256, n), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmm
