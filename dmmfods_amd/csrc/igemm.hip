// Implicit-GEMM convolution for gfx950: out[m][n] = sum_k A[m][k] * W[n][k]
//   m = output pixel (NHWC rows), k = (tap, input channel), n = output channel.
// One kernel serves forward convolutions (1x1, 3x3, 5x5, 7x7 s2, transposed 3x3 s2 as 4 gather phases,
// 2x2-avg-pool-then-1x1 transitions, nearest-upsampled sources) and data gradients (the same gather applied
// to the output gradient with re-packed weights), selected by the tap table / gather mode in ConvArgs and by
// the epilogue:
//   EPI_STORE  : write the tile (T) and accumulate per-channel sum / sum-of-squares (BatchNorm batch stats)
//   EPI_BNBWD  : acc is d(relu(bn(x))): apply the ReLU mask, reduce sum(dz), sum(dz*x) per channel and
//                scatter s*dz into the gradient buffer of x (assign or accumulate)
//   EPI_LOGITS : write fp32 NCHW logits
// Tile: 128 rows x BN columns per 256-thread workgroup; each wave owns 32 rows x BN columns as BN/32
// v_mfma_f32_32x32x16_f16 (or 32x32x2_f32) accumulators.  K advances in 64-byte chunks, register-staged
// through a double-buffered LDS image with 80-byte rows (conflict-free ds_read_b128).
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "dispatch.h"
#include "gather.h"
#include "isa.h"

namespace dmm {

template <typename T> struct Mma;
template <> struct Mma<f16> {
  static __device__ __forceinline__ void run(f32x16& acc, const f16x8& a, const f16x8& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  }
};
template <> struct Mma<bf16> {
  static __device__ __forceinline__ void run(f32x16& acc, const bf16x8& a, const bf16x8& b) { acc = mma16(a, b, acc); }
};
template <> struct Mma<float> {
  // lane (r, h) holds k = 8s + 4h + i of row r: the i-th 32x32x2 MFMA pairs k(h=0,i) with k(h=1,i)
  static __device__ __forceinline__ void run(f32x16& acc, const f32x4& a, const f32x4& b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
  }
};

#ifndef IGEMM_DBG
#define IGEMM_DBG 0  // timing experiments only: 1 no A loads, 2 no prologue math, 4 no epilogue, 8 no weight DMA, 16 no MFMA
#endif

template <typename T, int BN>
struct IgemmSmem {
  static constexpr int SLOT = TT<T>::SLOT;
  static constexpr int KS = 2;  // K chunks per pipeline stage (1 and 4 were measured: see the note at launch_bn)
  static constexpr int A_BYTES = KS * BM * ROWB;
  static constexpr int B_BYTES = KS * BN * ROWB;
  static constexpr int STAGE_PITCH_T = BN + SLOT;  // elements of T
  static constexpr int STAGE_PITCH_F = BN + 4;     // floats
  static constexpr int MAIN = 2 * (A_BYTES + B_BYTES);
  static constexpr int STAGE_T = BM * STAGE_PITCH_T * (int)sizeof(T);
  static constexpr int STAGE_F = BM * STAGE_PITCH_F * 4;
  static constexpr int EXTRA = BM * 4 + 2 * BN * 8 + BM * 16;  // rowpix + fp64 reduction scratch + row coordinates
  static constexpr int bytes(int epi) {  // without the per-launch prologue-constant image
    int st = (epi == EPI_STORE) ? STAGE_T : STAGE_F;
    int m = MAIN > st ? MAIN : st;
    return m + EXTRA;
  }
};

// LIN = lean path for plain 1x1 convolutions (one segment, one tap, unit stride, same grid): the source pixel of a row
// is the row itself, so the K loop needs no tap walker, coordinates or bounds tests.
// PRO = prologue of every segment, fixed at compile time for the MFMA variants (-1: look at the segment at run time).
//
// Operand staging per pipeline stage (KS = 2 chunks of 64 bytes of K):
//   A (gathered activations): waves 0-1 stage chunk 0, waves 2-3 chunk 1.  A thread owns ONE slot column j and FOUR rows
//     (rg + 32 i), so the chunk-level work (K-table entry, prologue constants) is shared by four slots.  The loads are
//     issued right after the barrier and consumed (prologue + ds_write) one iteration later, behind the MFMAs.
//   B (packed weights): never touches registers - an LDS-DMA load writes the tile image directly; the XOR
//     swizzle of the image is applied on the per-lane SOURCE address (the LDS side of an LDS-DMA is lane-linear).
//   K walk: a table in LDS, built once per workgroup, maps (chunk, j) -> segment, tap offset and channel, so the loop
//     has no divisions, tap-table loads or walker state.
struct SegU {  // the wave-uniform part of a Seg that the K loop needs (lives in SGPRs)
  const void* src;
  const void* src2;
  int ld, ld2, Hs, Ws, istride, mode, C, narr;
};
__device__ __forceinline__ SegU seg_uniform(const Seg& sg) {
  SegU r;
  r.src = sg.src; r.src2 = sg.src2; r.ld = sg.ld; r.ld2 = sg.ld2; r.Hs = sg.Hs; r.Ws = sg.Ws;
  r.istride = sg.istride; r.mode = sg.mode; r.C = sg.C; r.narr = sg.scale ? 2 : (sg.q ? 4 : 0);
  return r;
}

// KSV (chunks per stage) and NW (waves per workgroup) are fixed: they stay template parameters only because the kernels' mangled
// names are pinned (tests/golden/enqueue_trace_sha256.json, the recorded profiles).
template <typename T, int BN, int EPI, bool MFMA, bool LIN, int PRO, int KSV, int NW>
__global__ __launch_bounds__(NTHREADS) void igemm_kernel(const ConvArgs a) {
  static_assert(KSV == 2 && NW == 4, "two chunks per stage, four waves");
  constexpr int SLOT = TT<T>::SLOT;
  constexpr int BK = 4 * SLOT;
  typedef typename TT<T>::vec V;
  typedef IgemmSmem<T, BN> SM;
  constexpr int NT = BN / 32;
  constexpr int KS = SM::KS;
  constexpr bool ACCSTAT = MFMA && sizeof(T) == 2;  // EPI_STORE statistics from the accumulator layout (fp32 storage keeps the row-wise form: its parity tests pin it)
  constexpr int NB = KS * BN / (16 * NW);  // 1-KiB LDS-DMA pieces of the B image per wave per stage
  constexpr int RST = NTHREADS / KS / 4;   // row groups; a thread owns rows rg + RST i
  constexpr int NR = BM / RST;             // rows per thread

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int MAINB = (SM::MAIN > (EPI == EPI_STORE ? SM::STAGE_T : SM::STAGE_F)) ? SM::MAIN
                        : (EPI == EPI_STORE ? SM::STAGE_T : SM::STAGE_F);
  int* rowpix = (int*)(smem + MAINB);
  // Per-channel reductions are carried in fp64 from the first add: BatchNorm backward subtracts per-channel means of
  // the gradient, and an error of 1e-7*sum|dz| in that mean is a coherent offset that the next weight-gradient GEMM
  // amplifies over all pixels (torch's CPU BatchNorm accumulates in double for the same reason).
  double* red = (double*)(smem + MAINB + BM * 4);
  int4* rowinfo = (int4*)(smem + MAINB + BM * 4 + 2 * BN * 8);  // (b, y, x, valid) of every tile row
  // prologue constants (scale/shift or q/r/q_lo/r_lo) of every segment, staged once: the gather then issues ONE vector
  // memory instruction per slot instead of five (the L1-hit constant loads were saturating the texture-address path)
  float* lk0 = (float*)(smem + MAINB + SM::EXTRA);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ntiles = a.Npad / BN;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int mtile = lbid / ntiles, ntile = lbid - mtile * ntiles;
  const int m0 = mtile * BM, n0 = ntile * BN;

  const int u = tid / (NTHREADS / KS);  // chunk of the stage this thread gathers (wave-uniform: 256/KS threads per chunk)
  const int j = tid & 3;           // slot column
  const int rg = (tid >> 2) & (RST - 1);  // rows rg + RST i

  if (tid < BM) {
    const int m = m0 + tid;
    int pb, py_, px_;
    row_to_byx(m < a.M ? m : 0, a.Ho, a.Wo, pb, py_, px_);
    rowpix[tid] = m < a.M ? (pb * a.Hout + py_ * a.ostride + a.py) * a.Wout + px_ * a.ostride + a.px : -1;
    rowinfo[tid] = make_int4(pb, py_, px_, m < a.M ? 1 : 0);
  }
  if (tid < 2 * BN) red[tid] = 0.0;
  const int nk0 = stage_consts(a.seg[0], lk0, tid, NTHREADS);
  float* lk1 = lk0 + nk0;
  int nk1 = 0;
  if (a.nseg > 1) nk1 = stage_consts(a.seg[1], lk1, tid, NTHREADS);

  const int nch0 = a.seg[0].nchunks;
  const int total = nch0 + (a.nseg > 1 ? a.seg[1].nchunks : 0);

  // K table: bit 0 segment, bit 1 slot is inside the enumeration, bits 2-9 dy, 10-17 dx (signed), 18.. channel
  int* ktab = (int*)(lk1 + nk1);
  if constexpr (!LIN) {
    for (int e = tid; e < total * 4; e += NTHREADS) {
      const int g = e >> 2, jj = e & 3;
      const int s = g >= nch0 ? 1 : 0;
      const Seg& sg = a.seg[s];
      const int k = (g - (s ? nch0 : 0)) * BK + jj * SLOT;
      const int tap = k / sg.Cpad, c = k - tap * sg.Cpad;
      int ent = s;
      if (tap < sg.ntaps && c < sg.C) {
        const int t = sg.taps[tap];
        ent |= 2 | ((t & 0xff) << 2) | (((t >> 8) & 0xff) << 10) | (c << 18);
      }
      ktab[e] = ent;
    }
  }
  __syncthreads();

  const SegU su0 = seg_uniform(a.seg[0]);
  const SegU su1 = seg_uniform(a.seg[a.nseg > 1 ? 1 : 0]);

  int rb[NR], ry[NR], rx[NR];
  bool rv[NR];
  size_t roff[NR], roff2[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    if constexpr (LIN) {
      const int m = m0 + rg + RST * i;
      rv[i] = m < a.M;
      roff[i] = (size_t)(rv[i] ? m : 0) * su0.ld;
      roff2[i] = (size_t)(rv[i] ? m : 0) * su0.ld2;
    } else {
      const int4 ri = rowinfo[rg + RST * i];
      rb[i] = ri.x; ry[i] = ri.y; rx[i] = ri.z; rv[i] = ri.w != 0;
    }
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // B: per-lane source offsets of this wave's LDS-DMA pieces (fixed over K); piece p covers 16 weight rows of chunk ub
  const T* wp = (const T*)a.wpack;
  constexpr int PPC = BN / 16;  // pieces per chunk
  const int ub = (wave * NB) / PPC;
  int boff[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) {
    const int nn = ((wave * NB + q) % PPC) * 16 + (lane >> 2);
    const int sl = (lane & 3) ^ ((nn >> 2) & 3);
    boff[q] = (n0 + nn) * BK + sl * SLOT;
  }

  // issue-early / write-late: issue_a only issues the global loads of a later K-step; the prologue (BN+ReLU or the
  // deferred-gradient correction) runs in store_a one iteration later, behind the MFMAs of the step in between.
  struct {
    RawSlot<T> raw[NR];
    int s, c, narr;
  } R;
  auto issue_b = [&](int buf, int stage) {  // weights: LDS-DMA (a dead chunk re-reads chunk 0: its A slots are zero)
    const int g = stage * KS + ub;
    const T* bsrc = wp + (size_t)(g < total ? g : 0) * a.Npad * BK;
    unsigned char* Bs = smem + buf * (SM::A_BYTES + SM::B_BYTES) + SM::A_BYTES + wave * NB * 1024;
#pragma unroll
    for (int q = 0; q < NB; ++q)
      if (!(IGEMM_DBG & 8)) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc + boff[q]),
                                       (__attribute__((address_space(3))) void*)(Bs + q * 1024), 16, 0, 0);
  };
  auto issue_a = [&](int stage) {
    RawSlot<T>(&araw)[NR] = R.raw;
    const int g = stage * KS + u;
    const bool live = g < total;
    if constexpr (!LIN) {
#pragma unroll
      for (int i = 0; i < NR; ++i) {
#pragma unroll
        for (int e = 0; e < SLOT; ++e) { araw[i].v[e] = (T)0; araw[i].v2[e] = (T)0; }
        araw[i].state = 0;
      }
    }
    if constexpr (LIN) {
      // branch-free: every thread issues every load of every stage (addresses clamped to a valid slot, the result dropped by
      // `state`), so that the number of loads in flight behind a given one is a compile-time constant and the compiler's
      // counted s_waitcnt in store_a leaves the next stage's loads in flight
      const int c = g * BK + j * SLOT;
      const bool cv = live && c < su0.C;
      const int cc = cv ? c : 0;
      R.s = 0; R.c = cc; R.narr = cv ? su0.narr : 0;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        if (!(IGEMM_DBG & 1)) araw[i].v = *(const V*)((const T*)su0.src + roff[i] + cc);
        if (!(IGEMM_DBG & 1) && (PRO == 2 || (PRO < 0 && su0.narr == 4))) araw[i].v2 = *(const V*)((const T*)su0.src2 + roff2[i] + cc);
        araw[i].state = (cv && rv[i]) ? 1 : 3;
      }
      return;
    }
    const int ent = live ? ktab[g * 4 + j] : 0;
    const bool s1 = (__builtin_amdgcn_readfirstlane(ent) & 1) != 0;  // the segment is chunk- (hence wave-) uniform
    const SegU& su = s1 ? su1 : su0;
    const bool inside = (ent & 2) != 0;
    const int dy = (ent << 22) >> 24, dx = (ent << 14) >> 24, c = (int)((unsigned)ent >> 18);
    R.s = s1 ? 1 : 0; R.c = c; R.narr = inside ? su.narr : 0;
    if (PRO < 0 && su.mode == G_POOL2) {  // four loads + averaging: rare (transitions, always the run-time variant), synchronous
      const Seg& sg = a.seg[R.s];
      const SlotK<SLOT> kpool = lds_slot_consts<SLOT>(s1 ? lk1 : lk0, su.C, R.narr, c);
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        if (inside && rv[i]) {
          araw[i].v = gather_slot<T, true>(sg, rb[i], ry[i], rx[i], true, 0, c, kpool);
          araw[i].state = 2;
        }
      }
      return;
    }
    const int up = su.mode == G_UP2 ? 1 : 0;
    const unsigned hl = (unsigned)su.Hs << up, wl = (unsigned)su.Ws << up;
    const bool two = PRO == 2 || (PRO < 0 && su.narr == 4);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int sy = ry[i] * su.istride + dy, sx = rx[i] * su.istride + dx;
      const bool ok = inside && rv[i] && (unsigned)sy < hl && (unsigned)sx < wl;
      const size_t pix = ok ? (size_t)((rb[i] * su.Hs + (sy >> up)) * su.Ws + (sx >> up)) : 0;  // branch-free, as above
      if (!(IGEMM_DBG & 1)) araw[i].v = *(const V*)((const T*)su.src + pix * su.ld + c);
      if (!(IGEMM_DBG & 1) && two) araw[i].v2 = *(const V*)((const T*)su.src2 + pix * su.ld2 + c);
      araw[i].state = ok ? 1 : 3;
    }
  };
  auto store_a = [&](int buf) {
    unsigned char* As = smem + buf * (SM::A_BYTES + SM::B_BYTES);
    const float* lk = R.s ? lk1 : lk0;
    const int cst = R.s ? su1.C : su0.C;
    SlotK<SLOT> kk;
    if constexpr (PRO >= 0) kk = lds_slot_consts_n<SLOT, PRO == 1 ? 2 : (PRO == 2 ? (sizeof(T) == 2 ? 2 : 4) : 0)>(lk, cst, R.c);
    else kk = lds_slot_consts<SLOT>(lk, cst, R.narr, R.c);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int row = u * BM + rg + RST * i;
      *(V*)(As + row * ROWB + ((j ^ ((rg >> 2) & 3)) << 4)) = (IGEMM_DBG & 2) ? R.raw[i].v : finish_slot<T, PRO>(R.narr, R.raw[i], kk);
    }
  };

  const int r = lane & 31, h = lane >> 5;
  const int nstages = ((total + 2 * KS - 1) / (2 * KS)) * 2;  // even: the loop body holds two stages (a dead stage has zero A)
  auto mma = [&](int buf) {
    const unsigned char* As = smem + buf * (SM::A_BYTES + SM::B_BYTES);
    const unsigned char* Bs = As + SM::A_BYTES;
    if (MFMA) {
#pragma unroll
      for (int uq = 0; uq < KS; ++uq)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          // (wave >> 2 is 0 and wave & 3 is wave, as wave < 4 below is true: left from the retired 8-wave variants.  hipcc learns
          // the range of `wave` only after its optimiser has run, so dropping them is not a no-op: registers and schedule change)
          const int uu = (wave >> 2) * KS + uq;
          const int sw = ((2 * s + h) ^ ((r >> 2) & 3)) << 4;  // BM, BN and 32 are multiples of 16: swizzle depends on r only
          const V av = *(const V*)(As + (uu * BM + 32 * (wave & 3) + r) * ROWB + sw);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const V bv = *(const V*)(Bs + (uu * BN + 32 * t + r) * ROWB + sw);
            if (!(IGEMM_DBG & 16)) Mma<T>::run(acc[t], av, bv); else acc[t][0] += (float)av[0] * (float)bv[0];
          }
        }
    } else {
      // scalar check path with the same accumulator layout as the MFMA (debug / bring-up)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
          float s = 0.f;
          for (int uu = 0; uu < KS; ++uu) {
            const T* ap = (const T*)(As + (uu * BM + row) * ROWB);
            const T* bp = (const T*)(Bs + (uu * BN + 32 * t + r) * ROWB);
            for (int k = 0; k < BK; ++k) {
              const int ka = (((k / SLOT) ^ ((row >> 2) & 3)) * SLOT) + k % SLOT;
              const int kb = (((k / SLOT) ^ ((r >> 2) & 3)) * SLOT) + k % SLOT;
              s = fmaf(to_f32(ap[ka]), to_f32(bp[kb]), s);
            }
          }
          acc[t][i] += s;
        }
    }
  };

  // ---- epilogue geometry: thread = (slot column cv, row phase rr), rows rr + RPP i ----
  constexpr int NCV = BN / SLOT;       // slot columns in the tile
  constexpr int RPP = NTHREADS / NCV;  // rows per pass
  constexpr int NIT = BM / RPP;        // rows per thread
  const int cv = tid % NCV, rr = tid / NCV;
  const int n = n0 + cv * SLOT;
  const bool colvalid = n < a.N;
  // EPI_BNBWD reads x (and, when accumulating, the gradient) at every output position: issue those loads now, so that
  // they fly while the accumulators are staged through LDS instead of serialising eight memory latencies per thread
  V xpre[NIT], gpre[NIT];
  int ppre[NIT];
  const bool prefetched = EPI == EPI_BNBWD && !a.pool2;
  auto prefetch_epi = [&]() {
    if (!(EPI == EPI_BNBWD && prefetched)) return;
    const T* bx = (const T*)a.bx;
    const T* g = (const T*)a.out;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int pix = rowpix[rr + RPP * i];
      ppre[i] = colvalid ? pix : -1;
#pragma unroll
      for (int e = 0; e < SLOT; ++e) { xpre[i][e] = (T)0; gpre[i][e] = (T)0; }
      if (ppre[i] >= 0) {
        xpre[i] = *(const V*)(bx + (size_t)pix * a.ldbx + n);
        if (a.accumulate && g != nullptr) gpre[i] = *(const V*)(g + (size_t)pix * a.ldo + n);
      }
    }
  };
  issue_b(0, 0);
  issue_a(0);
  for (int it = 0; it < nstages; it += 2) {  // (each __syncthreads() also retires its stage's weight LDS-DMA: vmcnt(0))
    store_a(0);
    __syncthreads();
    issue_b(1, it + 1);
    issue_a(it + 1);  // past the end: dead stage (clamped loads, dropped)
    mma(0);
    store_a(1);
    __syncthreads();
    if (it + 2 < nstages) issue_b(0, it + 2);  // (the staging below reuses the image: no DMA may be left in flight)
    issue_a(it + 2);
    mma(1);
  }
  prefetch_epi();
  __syncthreads();  // all waves done with the operand image; reuse it for epilogue staging
  if ((IGEMM_DBG & 4) && acc[0][0] != 123.f) return;

  // ---- stage the accumulators through LDS: Cs[row][col] ----
  if (wave < 4) {  // (always: see mma)
    if (EPI == EPI_STORE) {
      T* Cs = (T*)smem;
      // BatchNorm statistics straight from the accumulator layout (as conv3.hip / cvp.hip): lane (r, h) holds column 32 t + r of 16
      // rows; column sums of the values AS STORED (rounded to T), the two lane halves folded, one LDS word per column and wave
      float* wpart = (float*)red;  // [wave][2][BN] floats over the fp64 scratch + row table (both dead here)
      bool rok[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) rok[i] = rowpix[32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h] >= 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        float ps1 = 0.f, ps2 = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
          const T v = from_f32<T>(acc[t][i]);
          Cs[row * SM::STAGE_PITCH_T + 32 * t + r] = v;
          if (ACCSTAT && rok[i]) { const float f = to_f32(v); ps1 += f; ps2 = fmaf(f, f, ps2); }
        }
        if (ACCSTAT) {
          wpart[(wave * 2 + h) * BN + 32 * t + r] = fold_swap32(ps1, ps2);  // lane half 0: the sum, half 1: the sum of squares
        }
      }
    } else {
      float* Cs = (float*)smem;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
          Cs[row * SM::STAGE_PITCH_F + 32 * t + r] = acc[t][i];
        }
    }
  }
  __syncthreads();

  if (EPI == EPI_LOGITS) {
    const float* Cs = (const float*)smem;
    const size_t plane = (size_t)a.Hout * a.Wout;
    for (int idx = tid; idx < BM * a.N; idx += NTHREADS) {
      const int n = idx / BM, row = idx - n * BM;
      const int pix = rowpix[row];
      if (pix < 0 || n0 + n >= a.N) continue;
      const int bimg = pix / (int)plane;
      const int rem = pix - bimg * (int)plane;
      a.logits[((size_t)bimg * a.N + n0 + n) * plane + rem] = Cs[row * SM::STAGE_PITCH_F + n];
    }
    return;
  }

  // per-thread partials cover <= 128/RPP rows: float is exact enough here; everything above this level is fp64
  float s1[SLOT], s2[SLOT];
#pragma unroll
  for (int i = 0; i < SLOT; ++i) { s1[i] = 0.f; s2[i] = 0.f; }

  if (EPI == EPI_STORE) {
    const T* Cs = (const T*)smem;
    T* out = (T*)a.out;
    for (int row = rr; row < BM; row += RPP) {
      const int pix = rowpix[row];
      if (pix < 0 || !colvalid) continue;
      const V v = *(const V*)(Cs + row * SM::STAGE_PITCH_T + cv * SLOT);
      *(V*)(out + (size_t)pix * a.ldo + n) = v;
      if (!ACCSTAT) {
        float f[SLOT];
        vec_to_f32<T>(v, f);
#pragma unroll
        for (int i = 0; i < SLOT; ++i) { s1[i] += f[i]; s2[i] = fmaf(f[i], f[i], s2[i]); }
      }
    }
    if (a.stat_sum == nullptr) return;
    if (ACCSTAT) {  // four wave partials per column -> fp64 -> one atomic per column and workgroup (per-XCD replica)
      const float* wpart = (const float*)red;
      if (!(IGEMM_DBG & 32) && tid < 2 * BN) {
        const int col = tid % BN, which = tid / BN;
        if (n0 + col < a.N) {
          double s = 0.0;
#pragma unroll
          for (int w = 0; w < 4; ++w) s += (double)wpart[(w * 2 + which) * BN + col];
          const size_t rep = (size_t)(blockIdx.x & (STAT_REPS - 1)) * a.stat_stride;
          atomic_add_f64((which ? a.stat_sq : a.stat_sum) + rep + n0 + col, s);
        }
      }
      return;
    }
  } else {  // EPI_BNBWD
    const float* Cs = (const float*)smem;
    const T* bx = (const T*)a.bx;
    T* g = (T*)a.out;
    float sc[SLOT], sh[SLOT], mu[SLOT], is[SLOT];
    if (colvalid) {
      load_f32s<SLOT>(a.bscale + n, sc); load_f32s<SLOT>(a.bshift + n, sh);
      load_f32s<SLOT>(a.bmean + n, mu); load_f32s<SLOT>(a.binvstd + n, is);
    }
    if (prefetched) {
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        if (ppre[i] < 0) continue;
        const int row = rr + RPP * i;
        float av[SLOT], xf[SLOT], gf[SLOT];
#pragma unroll
        for (int e = 0; e < SLOT; e += 4) {
          const f32x4 t4 = *(const f32x4*)(Cs + row * SM::STAGE_PITCH_F + cv * SLOT + e);
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
        if (g != nullptr) *(V*)(g + (size_t)ppre[i] * a.ldo + n) = f32_to_vec<T>(gf);  // null: only the reductions are wanted
      }
    }
    const int nsub = a.pool2 ? 4 : 1;
    const float wgt = a.pool2 ? 0.25f : 1.f;
    for (int row = rr; row < BM && !prefetched; row += RPP) {
      const int pix = rowpix[row];
      if (pix < 0 || !colvalid) continue;
      float av[SLOT];
#pragma unroll
      for (int i = 0; i < SLOT; i += 4) {
        const f32x4 t4 = *(const f32x4*)(Cs + row * SM::STAGE_PITCH_F + cv * SLOT + i);
        av[i] = t4[0]; av[i + 1] = t4[1]; av[i + 2] = t4[2]; av[i + 3] = t4[3];
      }
      for (int sub = 0; sub < nsub; ++sub) {
        const size_t p = (size_t)pix + (sub >> 1) * a.Wout + (sub & 1);
        float xf[SLOT], gf[SLOT];
        vec_to_f32<T>(*(const V*)(bx + p * a.ldbx + n), xf);
        if (a.accumulate && g != nullptr) vec_to_f32<T>(*(const V*)(g + p * a.ldo + n), gf);
#pragma unroll
        for (int i = 0; i < SLOT; ++i) {
          const float dz = (fmaf(xf[i], sc[i], sh[i]) > 0.f) ? av[i] * wgt : 0.f;
          s1[i] += dz;
          s2[i] = fmaf(dz, (xf[i] - mu[i]) * is[i], s2[i]);  // sum dz * xhat: centred, so nothing cancels later
          gf[i] = (a.accumulate ? gf[i] : 0.f) + sc[i] * dz;
        }
        if (g != nullptr) *(V*)(g + p * a.ldo + n) = f32_to_vec<T>(gf);
      }
    }
  }

  // ---- per-channel reductions: threads -> LDS -> one fp64 atomic per channel per workgroup ----
  // lanes l, l + NCV, l + 2 NCV, ... of a wave hold the same slot column: fold them with cross-lane adds first, so that one
  // lane per column and wave touches LDS (4-way instead of 16..64-way contention on every fp64 LDS atomic)
  if constexpr (sizeof(T) == 4 || !MFMA) {  // (the scalar bring-up kernels of f16 spill as heavily as fp32's)
    // fp32 storage (the parity configuration) keeps the round-2 butterfly.  What round 3 saw with fold_to_lds here - and shelved as "not
    // understood" - was run down in round 4 with experiment builds that used the fold in the fp32 instantiations too, all of them or one
    // epilogue / column tile at a time (the switches are retired; results in profiles/r04/ablations.txt and DESIGN 2):
    //  * it was NOT the gfx950 lane swaps, the DPP rotations, hipcc's spilling or its pairing of fp32 operations: the same fold written
    //    with ds_bpermute shuffles only failed the same test with the same numbers, -mllvm -amdgpu-spill-vgpr-to-agpr=0 and
    //    -fno-slp-vectorize changed nothing, the machine verifier was clean, and the lane algebra is
    //    emulated exactly on the CPU (tests/test_host_cpu.py::test_fold_lane_algebra);
    //  * the scalar bring-up kernels' symptom (rows 25 / 29 of every 32) did not reproduce in any variant;
    //  * every per-kernel sum of every fp32 instantiation was right to 1e-8 of the tensor with the fold (forward statistics and both
    //    data-gradient reductions, with and without the deferred correction, accumulate on and off);
    //  * the one failing test (tiny no-fusion model, fp32) narrowed to the FORWARD statistics of the 32-column tiles
    //    (every data-gradient fold alone was clean): the fold adds a column's eight lane partials
    //    in a different order, the batch mean / variance of ONE channel (decoder stage 4, input channel 4) move by 1.4e-7 / 6.6e-8
    //    relative, one element of that channel sits within that distance of its ReLU threshold, its mask flips in backward, and
    //    that channel's bias gradient moves by exactly one element's gradient (10.746 -> 11.947 of 768 summands); everything
    //    upstream follows by 1-6 %.  Both results are correct fp32 evaluations of the same network - the fp64 oracle happens to sit
    //    on the butterfly's side of that threshold for the fixture's seed.  The parity fixtures therefore pin the butterfly's order
    //    for fp32; the 16-bit kernels, whose parity bounds are norm-wise, use the fold.
#pragma unroll
    for (int i = 0; i < SLOT; ++i) {
#pragma unroll
      for (int d = NCV; d < 64; d <<= 1) {
        s1[i] += __shfl_xor(s1[i], d, 64);
        s2[i] += __shfl_xor(s2[i], d, 64);
      }
    }
    if (colvalid && lane < NCV) {
#pragma unroll
      for (int i = 0; i < SLOT; ++i) {
        atomicAdd(&red[fold_slot<NCV, SLOT>(0, cv * SLOT + i)], (double)s1[i]);
        atomicAdd(&red[fold_slot<NCV, SLOT>(1, cv * SLOT + i)], (double)s2[i]);
      }
    }
  } else {
    fold_to_lds<NCV, SLOT, BN>(s1, s2, red, cv, colvalid, lane);
  }
  __syncthreads();
  if (!(IGEMM_DBG & 32) && tid < BN && n0 + tid < a.N) {
    double* d1 = (EPI == EPI_STORE) ? a.stat_sum : a.red1;
    double* d2 = (EPI == EPI_STORE) ? a.stat_sq : a.red2;
    const size_t rep = (size_t)(blockIdx.x & (STAT_REPS - 1)) * a.stat_stride;
    atomic_add_f64(d1 + rep + n0 + tid, red[fold_slot<NCV, SLOT>(0, tid)]);
    atomic_add_f64(d2 + rep + n0 + tid, red[fold_slot<NCV, SLOT>(1, tid)]);
  }
}

// ------------------------------------------------------------------------------------------------
// What was tried on this kernel and did not pay (MI355X, C2 b4; rounds 2-3), each a compile-time switch up to the commit that
// retired them: 4 K chunks per stage for launches of <= 512 workgroups (step +1.2 ms) and 1 for the 128-column tiles (a third
// workgroup per CU: +-1 %) instead of 2; two stages of the gathered operand in flight (a second register set, an inline-assembly
// weight DMA: store class -4 %, bnbwd class +3 % at 264 VGPRs, step +-0; with raw counted barriers in the K loop: bnbwd 0.96 ->
// 0.93 ms, step +-0); the epilogue operands of 1x1 data gradients requested before the K loop (+-0); 8-wave workgroups that split
// K for small grids (block-3 1x1: 25 -> 38 us; for fp32 the split changes the summation order the parity tests pin).  Records:
// DESIGN.md 7 ("where the time went", round 2) and profiles/r03/ablations.txt.  Ablation builds
// (tools/conv_time.py with IGEMM_DBG) say why: with every load, the prologue math and the MFMAs removed a 1x1 launch still takes
// 70-90 % of its time - the cost is the skeleton (LDS writes, barrier, fragment reads, staging, the per-channel reductions and
// the stores of the epilogue), not latency that more bytes or waves in flight could hide.
template <typename T, int BN, int EPI>
static hipError_t launch_bn(const ConvArgs& a, bool mfma, hipStream_t st) {
  constexpr int KSV = 2, NW = 4;  // (igemm_kernel)
  const int mtiles = (a.M + BM - 1) / BM;
  const int ntiles = a.Npad / BN;
  int kfl = 0;
  for (int s = 0; s < a.nseg; ++s) kfl += seg_const_floats(a.seg[s]);
  int nchunks = 0;
  for (int s = 0; s < a.nseg; ++s) nchunks += a.seg[s].nchunks;
  const int smem = IgemmSmem<T, BN>::bytes(EPI) + kfl * 4 + nchunks * 16 + 16;
  const Seg& s0 = a.seg[0];
  const bool lin = mfma && a.nseg == 1 && s0.ntaps == 1 && s0.taps[0] == 0 && s0.mode == G_PLAIN && s0.istride == 1 &&
                   s0.Hs == a.Ho && s0.Ws == a.Wo;
  // prologue kind, identical for all segments of a launch: 0 none, 1 BN+ReLU, 2 effective gradient; pooled sources and
  // mixed segments take the run-time variant
  int pro = s0.scale ? 1 : (s0.q ? 2 : 0);
  for (int s = 0; s < a.nseg; ++s) {
    const Seg& sg = a.seg[s];
    if (sg.mode == G_POOL2 || (sg.scale ? 1 : (sg.q ? 2 : 0)) != pro) pro = -1;
  }
  constexpr int P1 = EPI == EPI_BNBWD ? 2 : 1;  // the prologue this epilogue normally sees
  LdsLauncher<ConvArgs> run;
  if (!mfma) {
    // the scalar check kernels exist for fp32 / f16 (bring-up); bf16 arrived with the MFMA kernels already proven
    if constexpr (std::is_same<T, bf16>::value) return hipErrorNotSupported;
    else run = launch_lds<igemm_kernel<T, BN, EPI, false, false, -1, KSV, NW>, ConvArgs>;
  }
  else if (pro == P1) run = lin ? launch_lds<igemm_kernel<T, BN, EPI, true, true, P1, KSV, NW>, ConvArgs> : launch_lds<igemm_kernel<T, BN, EPI, true, false, P1, KSV, NW>, ConvArgs>;
  else if (pro == 0) run = lin ? launch_lds<igemm_kernel<T, BN, EPI, true, true, 0, KSV, NW>, ConvArgs> : launch_lds<igemm_kernel<T, BN, EPI, true, false, 0, KSV, NW>, ConvArgs>;
  else run = launch_lds<igemm_kernel<T, BN, EPI, true, false, -1, KSV, NW>, ConvArgs>;
  if (smem > 160 * 1024) return hipErrorInvalidValue;
  return run(smem > 48 * 1024 ? 160 * 1024 : 0, mtiles * ntiles, NTHREADS, smem, st, a);
}

template <typename T, int EPI>
static hipError_t launch_epi(const ConvArgs& a, bool mfma, hipStream_t st) {
  if (EPI == EPI_LOGITS) return launch_bn<T, 32, EPI>(a, mfma, st);
  // Column tile: as wide as the padded output allows (128-column tiles re-gather the A operand half as often as 64-column
  // ones).  Narrower tiles for launches with few workgroups (DMM_MIN_WGS = n: halve the tile until the launch has n workgroups)
  // were measured on C2 b4 and do NOT help the small maps of blocks 3-4 / decoder stages 1-2 (33.57 ms/step at 0, 33.45 at 300,
  // 33.71 at 400, 34.13 at 1000): their cost is the length of each workgroup's chain of dependent stages, not idle CUs.
  // fp32 storage is the opposite case (round 3, C1 = 1x256x384): a 48-workgroup launch with K = 1024 is 2048 v_mfma_f32_32x32x2_f32 of 64
  // cycles per wave - bound by the fp32 matrix rate of a fifth of the chip.  Narrower tiles spread the same MFMAs over more CUs:
  // 16.7 -> 11.9 ms/step at 128 workgroups or more.  Default: 256 for fp32, 0 for the 16-bit types.
  static const int min_wgs = lab_int("DMM_MIN_WGS", sizeof(T) == 4 ? 256 : 0);
  const int mtiles = (a.M + BM - 1) / BM;
  int bn = a.Npad % 128 == 0 ? 128 : (a.Npad % 64 == 0 ? 64 : 32);
  while (bn > 32 && mtiles * (a.Npad / bn) < min_wgs) bn >>= 1;
  if (bn == 128) return launch_bn<T, 128, EPI>(a, mfma, st);
  if (bn == 64) return launch_bn<T, 64, EPI>(a, mfma, st);
  return launch_bn<T, 32, EPI>(a, mfma, st);
}

// One translation unit per storage type (IGEMM_PART = 0 fp32, 1 f16, 2 bf16; see the Makefile): the ~50 kernel instantiations
// of a type compile in parallel with the other types'.
template <typename T>
hipError_t launch_igemm_type(const ConvArgs& a, int epi, bool mfma, hipStream_t st) {
  if (epi == EPI_STORE) return launch_epi<T, EPI_STORE>(a, mfma, st);
  if (epi == EPI_BNBWD) return launch_epi<T, EPI_BNBWD>(a, mfma, st);
  return launch_epi<T, EPI_LOGITS>(a, mfma, st);
}
#if !defined(IGEMM_PART) || IGEMM_PART == 0
template hipError_t launch_igemm_type<float>(const ConvArgs&, int, bool, hipStream_t);
#endif
#if !defined(IGEMM_PART) || IGEMM_PART == 1
template hipError_t launch_igemm_type<f16>(const ConvArgs&, int, bool, hipStream_t);
#endif
#if !defined(IGEMM_PART) || IGEMM_PART == 2
template hipError_t launch_igemm_type<bf16>(const ConvArgs&, int, bool, hipStream_t);
#endif

#if !defined(IGEMM_PART) || IGEMM_PART == 1
extern template hipError_t launch_igemm_type<float>(const ConvArgs&, int, bool, hipStream_t);
extern template hipError_t launch_igemm_type<bf16>(const ConvArgs&, int, bool, hipStream_t);

// The special-case families in dispatch order.
static const ConvFamily kConvFamilies[] = {
    {IMPL_THIN, thin_resolve, thin_launch},     // few output channels x many taps: gather once, reduce the taps in LDS
    {IMPL_HF, hf_resolve, hf_launch},           // the head's first convolution, four parity phases in one launch: wave-specialised, phase weights resident in LDS
    {IMPL_CF, cf_resolve, cf_launch},           // the dense 3x3 forward on the large maps: wave-specialised, weights resident in LDS
    {IMPL_CONV3, conv3_resolve, conv3_launch},  // 3x3 convolutions of the dense layers (16-bit storage): LDS halo tile, prologue once per element
    {IMPL_CVP, cvp_resolve, cvp_launch},        // forward of the ConvTranspose parity phases: halo tile per 128-channel group, a tap is a fragment address
    {IMPL_PIG, pig_resolve, pig_launch},        // plain 1x1 convolutions, forward: persistent workgroups (next tile's loads under this tile's epilogue)
    {IMPL_HALO, halo_resolve, halo_launch},     // multi-tap layers whose weights fit in LDS may take the halo-tile kernel
};

// The first family that may take the launch (family_allowed) and resolves it; nullptr: none does - the launch is the generic kernel's.
static const ConvFamily* conv_family(const ConvArgs& a, int dtype, int epi, int impl, unsigned deny, Resolved& r) {
  // second pass of a two-pass BatchNorm backward: ONE kernel variant stores s*dz + q + r*x (conv3.hip's thin-only data gradient);
  // every other family would silently store s*dz
  const bool conv3_only = a.eq != nullptr || a.er != nullptr;
  for (const ConvFamily& f : kConvFamilies)
    if ((!conv3_only || f.family == IMPL_CONV3) && family_allowed(f, impl, deny) && f.resolve(a, dtype, epi, r)) return &f;
  return nullptr;
}

// impl = IMPL_AUTO: every family `deny` does not name may take the launch (the single-kernel test entry points, which pass the
// process-wide switches); otherwise the family a plan recorded for this launch when it was built (igemm_pick), whatever the option
// switches say now.
hipError_t launch_igemm(const ConvArgs& a, int dtype, int epi, bool mfma, hipStream_t st, int impl, unsigned deny) {
  if (a.M <= 0) return hipSuccess;
  if (mfma && impl != IMPL_GENERIC) {
    Resolved r;
    if (const ConvFamily* f = conv_family(a, dtype, epi, impl, deny, r)) {
      const hipError_t e = f->launch(r, st);
      note_impl(f->family);
      return e;
    }
  }
  note_impl(IMPL_GENERIC);
  // what the generic kernels do not implement must fail here, not compute something else
  if (a.eq != nullptr || a.er != nullptr) return hipErrorNotSupported;                      // the second pass of a two-pass BatchNorm backward
  if (epi == EPI_BNBWD && a.out == nullptr && (a.pool2 || a.accumulate)) return hipErrorNotSupported;  // reductions-only: the plain prefetched path
  if (a.nphase != 0) return hipErrorNotSupported;                                           // merged parity phases belong to conv3 / hf / cvp
  if (dtype == DT_F16) return launch_igemm_type<f16>(a, epi, mfma, st);
  if (dtype == DT_BF16) return launch_igemm_type<bf16>(a, epi, mfma, st);
  return launch_igemm_type<float>(a, epi, mfma, st);
}

// Which family launch_igemm(..., IMPL_AUTO, deny) would run for this launch (nothing is launched, the runtime is not asked anything).
int igemm_pick(const ConvArgs& a, int dtype, int epi, bool mfma, unsigned deny) {
  if (!mfma) return IMPL_GENERIC;
  Resolved r;
  const ConvFamily* f = conv_family(a, dtype, epi, IMPL_AUTO, deny, r);
  return f ? f->family : IMPL_GENERIC;
}
#endif

}  // namespace dmm
