// Weight gradient of the dense layers' 3x3 growth convolution (torchvision _DenseLayer.conv2, 128 -> 32 channels; reference call
// sites M:85-92, M:169-176) on LDS tiles, gfx950, 16-bit storage types.
//
//   dW[n][c][tap] = sum over pixels p of  A[p][c] * dYeff[p + t_tap][n]        (transposed form of wgrad.hip: taps on the dY side)
//     A     = relu(bn2(y1))           128 channels, normalised ONCE per pixel
//     dYeff = g + q + r*x             32 channels of the block's gradient buffer with the deferred BatchNorm-backward correction
// A PERSISTENT workgroup keeps the WHOLE 9 x 32 x 128 result in accumulators and walks 8 x 16 pixel tiles; per tile the A tile
// (128 px x 128 ch) and the 10 x 18 pixel dYeff halo (32 ch) go to LDS once, a tap is an address offset into the halo image, both
// MFMA operands are read with the transposing read ds_read_b64_tr_b16 (the contraction index is the pixel).
//
// Round 4: WAVE-SPECIALISED.  Rounds 2-3 ran this as four waves that each loaded, normalised, wrote LDS, multiplied - one phase
// after the other, one wave per SIMD (328 registers), so the phases added up: 6.3 us per tile against 1.1 us of fragment reads and
// MFMAs (the same on every block: 121 us on block 1's 18.75 tiles per workgroup, 58 us on block 2's 9.2, profiles/r03).  Now a
// workgroup is EIGHT waves, two per SIMD:
//   * waves 0-3 (matrix waves) own the accumulators (wave w: channels 32w .. 32w+31 of A, nine 32x32 tiles = 144 registers) and do
//     nothing but fragment reads and MFMAs on the image set of the current tile;
//   * waves 4-7 (loader waves) own the global loads - TWO register sets, i.e. the loads of tiles t+1 and t+2 are in flight while tile
//     t is multiplied -, the prologues (BN+ReLU on A, effective gradient on dY) and the LDS writes of the NEXT tile's image set;
//   * two image sets in LDS and ONE raw barrier per tile (isa.h lds_barrier: the loaders' prefetch stays in flight across it): the
//     loaders write set (t+1)&1 while the matrix waves read set t&1; barrier t+1 tells the matrix waves that image t+1 is complete
//     and the loaders that image t is free again.
// The partial result of a workgroup (147 KB) is either added to the packed gradient with fp32 atomics or - `part` - STORED to the
// workgroup's slot and added up in fixed order by wg3_reduce_kernel (the recipe of bw1.hip): no float atomics, and the number of
// workgroups no longer has to balance tiles per workgroup against 147 KB of atomics each.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "dispatch.h"
#include "gather.h"
#include "isa.h"
#include "pointwise.h"

#ifndef WG3_DBG
#define WG3_DBG 0  // timing experiments only (tools/build_variant.sh): 1 no output at the end of the walk, 2 no MFMA phase, 4 no loads
#endif
namespace dmm {

constexpr int W3_TH = 8, W3_TW = 16, W3_HH = 10, W3_HW = 18;
constexpr int W3_CA = 128, W3_CY = 32;                 // channels of A and of dY
constexpr int W3_A_BYTES = BM * W3_CA * 2;             // 32 KB, 256-byte rows, 64-byte granule XOR-ed with (row & 3)
constexpr int W3_Y_BYTES = W3_HH * W3_HW * W3_CY * 2;  // 11.25 KB, 64-byte rows
constexpr int W3_IMG = W3_A_BYTES + W3_Y_BYTES;        // one image set
constexpr int W3_LDS = 2 * W3_IMG;                     // 86.5 KB: one workgroup (8 waves) per CU
constexpr int W3_NT = 512;                             // threads: 4 matrix waves + 4 loader waves

struct Wg3Args {
  WgradArgs w;
  int tiles_y, tiles_x, ntiles, tiles_per_wg;
  float* part;  // per-workgroup slots of W3_SLOT_FLOATS (nullable: fp32 atomics into w.dpack)
};

// What the walk over the tiles reads of a launch: the operands of ONE weight gradient.  wg3_kernel fills it from its WgradArgs, the
// grouped kernel (wg3_group_kernel) from the member of its table the workgroup belongs to.
struct W3View {
  const void *asrc, *ysrc, *ysrc2;         // A = y1; dY (the compact copy or the block's gradient buffer) and its second operand
  const float *ascale, *ashift, *yq, *yr;  // norm2's constants; the effective gradient's
  float* dpack;
  int ald, yld, yld2, Ho, Wo, tiles_y, tiles_x;
};
struct W3Taps { short t[12]; };  // the nine taps of dY: (dy & 0xff) | ((dx & 0xff) << 8)

// The loaders' global loads and their waits are inline assembly: isa.h explains why.  The sets of this kernel: NA slots of A, NY of dY
// and, with the effective gradient (PQ == 2), NY of its second operand - one set is NLD = NA + NY or NA + 2 NY requests.
// MODE 0: wait until this set has landed (the other set's NLD requests stay in flight); 1: wait for everything; 2: keep alive only
template <typename T, int NA, int NY, int PQ, int MODE>
__device__ __forceinline__ void w3_sync(typename TT<T>::vec (&ra)[NA], typename TT<T>::vec (&ry)[NY], typename TT<T>::vec (&ry2)[PQ == 2 ? NY : 1]) {
  static_assert(NA == 8 && NY == 3, "DMM_V8 / DMM_V3 below");
  if constexpr (PQ == 2) {
    if constexpr (MODE == 2) DMM_VM_HOLD(DMM_V8(ra), DMM_V3(ry), DMM_V3(ry2));
    else DMM_VM_WAIT(MODE == 0 ? NA + 2 * NY : 0, DMM_V8(ra), DMM_V3(ry), DMM_V3(ry2));
  } else {
    if constexpr (MODE == 2) DMM_VM_HOLD(DMM_V8(ra), DMM_V3(ry));
    else DMM_VM_WAIT(MODE == 0 ? NA + NY : 0, DMM_V8(ra), DMM_V3(ry));
  }
}

// PQ = prologue of dY: 0 none (materialised gradient), 2 effective gradient (q, r of the 16-bit form)
// The walk of one workgroup over the tiles [t_beg, t_end) of `a`; the partial result goes to `slot` (null: fp32 atomics into a.dpack).
template <typename T, int PQ>
__device__ __forceinline__ void wg3_walk(const W3View& a, const W3Taps& taps, const int t_beg, const int t_end, float* slot) {
  static_assert(sizeof(T) == 2, "16-bit storage");
  typedef typename TT<T>::vec V;
  constexpr int SLOT = 8;
  constexpr int NL = 256;                                                   // loader threads
  constexpr int NA = BM * (W3_CA / SLOT) / NL;                              // 8 A slots per loader thread
  constexpr int NY = (W3_HH * W3_HW * (W3_CY / SLOT) + NL - 1) / NL;        // 3 dY slots per loader thread

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (t_beg >= t_end) return;  // (workgroup-uniform)
  const int nt = t_end - t_beg;

  if (wave >= 4) {
    // ================================ loader waves ================================
    const int lt = tid - NL;
    const int ca = lt & 15, pa0 = lt >> 4;  // A: slot column, pixel column pa0 of tile rows i = 0..7
    const int cy = lt & 3, hy0 = lt >> 2;   // dY: slot column, halo pixels hy0 + 64 i
    SlotK<SLOT> ka, ky;
    ka.k0 = load_fv<SLOT>(a.ascale + ca * SLOT); ka.k1 = load_fv<SLOT>(a.ashift + ca * SLOT); ka.k2 = 0.f; ka.k3 = 0.f;
    ky.k0 = 0.f; ky.k1 = 0.f; ky.k2 = 0.f; ky.k3 = 0.f;
    if (PQ == 2) { ky.k0 = load_fv<SLOT>(a.yq + cy * SLOT); ky.k1 = load_fv<SLOT>(a.yr + cy * SLOT); }
    const T* asrc = (const T*)a.asrc + ca * SLOT;
    const T* ysrc = (const T*)a.ysrc + cy * SLOT;
    const T* ysrc2 = (const T*)a.ysrc2 + cy * SLOT;
    int hyy[NY], hxx[NY];  // this thread's halo positions (fixed over the walk)
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const int hp = min(hy0 + 64 * i, W3_HH * W3_HW - 1);
      hyy[i] = hp / W3_HW - 1; hxx[i] = hp % W3_HW - 1;
    }
    struct LSet {
      V ra[NA], ry[NY], ry2[PQ == 2 ? NY : 1];
      unsigned oka, oky;  // validity bits of the slots
    };
    // the issue cursor walks the tiles of this workgroup in order, two tiles ahead of the image being written
    const int tiles_img = a.tiles_y * a.tiles_x;
    int cb = t_beg / tiles_img, cty, ctx, cleft = nt;
    { const int tr = t_beg - cb * tiles_img; cty = tr / a.tiles_x; ctx = tr - cty * a.tiles_x; }
    auto issue = [&](LSet& R) {  // branch-free: clamped addresses, zeroed at the write if outside; past the end: the last tile again
      const int y0 = cty * W3_TH, x0 = ctx * W3_TW;
      R.oka = 0; R.oky = 0;
      const int xa = x0 + pa0;
      const size_t arow = (size_t)cb * a.Ho;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int y = y0 + i;
        if (y < a.Ho && xa < a.Wo) R.oka |= 1u << i;
        const size_t pix = (arow + min(y, a.Ho - 1)) * a.Wo + min(xa, a.Wo - 1);
        if (!(WG3_DBG & 4)) gload16(R.ra[i], asrc + pix * a.ald);
      }
      const size_t yrow = (size_t)cb * a.Ho;
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        const int y = y0 + hyy[i], x = x0 + hxx[i];
        if (hy0 + 64 * i < W3_HH * W3_HW && (unsigned)y < (unsigned)a.Ho && (unsigned)x < (unsigned)a.Wo) R.oky |= 1u << i;
        const size_t pix = (yrow + min(max(y, 0), a.Ho - 1)) * a.Wo + min(max(x, 0), a.Wo - 1);
        if (!(WG3_DBG & 4)) gload16(R.ry[i], ysrc + pix * a.yld);
        if constexpr (PQ == 2) { if (!(WG3_DBG & 4)) gload16(R.ry2[i], ysrc2 + pix * a.yld2); }
      }
      if (--cleft > 0) {  // (uniform) advance; the cursor parks on the last tile
        if (++ctx == a.tiles_x) { ctx = 0; if (++cty == a.tiles_y) { cty = 0; ++cb; } }
      }
    };
    auto store = [&](LSet& R, int set, bool wait = true) {
      if (wait && !(WG3_DBG & 4)) w3_sync<T, NA, NY, PQ, 0>(R.ra, R.ry, R.ry2);  // this set has landed; the other set's NLD requests stay in flight
      unsigned char* As = smem + set * W3_IMG;
      unsigned char* Ys = As + W3_A_BYTES;
      V z;
#pragma unroll
      for (int e = 0; e < SLOT; ++e) z[e] = (T)0;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int p = pa0 + 16 * i;
        const V v = bn_relu_slot(R.ra[i], ka);
        *(V*)(As + p * 256 + ((ca * 16) ^ ((p & 3) << 6))) = ((R.oka >> i) & 1) ? v : z;
      }
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        const int hp = hy0 + 64 * i;
        if (hp < W3_HH * W3_HW) {
          V v = R.ry[i];
          if constexpr (PQ == 2) v = eff_grad_slot(R.ry[i], R.ry2[i], ky);
          *(V*)(Ys + hp * 64 + cy * 16) = ((R.oky >> i) & 1) ? v : z;
        }
      }
    };
    // The prologue constants must have ARRIVED before the ring starts: loaded in front of it and first used inside the loop they stay
    // "pending" in hipcc's wait-count model on the loop's entry path, the merged state at the loop header then waits for them in EVERY
    // iteration - with the ring's loads issued behind them that wait was vmcnt(13) ... vmcnt(0): it drained the second register set
    // (seen in the ISA of the first version of this kernel: no gain over the four-wave kernel until this was fixed).
#pragma unroll
    for (int e = 0; e < SLOT; ++e) {
      asm volatile("" : "+v"(ka.k0[e]), "+v"(ka.k1[e]));
      if constexpr (PQ == 2) asm volatile("" : "+v"(ky.k0[e]), "+v"(ky.k1[e]));
    }
    LSet R0, R1;
    issue(R0);
    issue(R1);
    // (both halves unconditional in the loop, the odd last tile behind it: with a break in the middle the compiled loop has a path
    // from the first half straight to the latch, which tools/check_asm_loads.py - it cannot know that path always leaves - must flag)
    for (int k = 0; k + 1 < nt; k += 2) {
      store(R0, 0);    // waits for R0's loads only: R1's stay in flight
      lds_barrier();   // barrier k: image 0 complete / the matrix waves have left image 1
      issue(R0);       // tile k + 2
      store(R1, 1);
      lds_barrier();   // barrier k + 1
      issue(R1);       // tile k + 3
    }
    // Behind the loop BOTH sets may still have requests in flight (the cursor's surplus requests for tiles past the end), and the
    // compiler - which does not know that - considers a set's registers free from its last use on: it reused R1's registers as
    // temporaries of the odd tile's prologue below while R1's loads were still landing in them (found by tools/check_asm_loads.py
    // before the first run).  So: everything lands HERE, and both sets are operands of the statements, i.e. alive until then.
    if (!(WG3_DBG & 4)) {
      w3_sync<T, NA, NY, PQ, 1>(R0.ra, R0.ry, R0.ry2);
      w3_sync<T, NA, NY, PQ, 2>(R1.ra, R1.ry, R1.ry2);
    }
    if (nt & 1) {
      store(R0, 0, false);
      lds_barrier();
    }
    return;
  }

  // ================================ matrix waves ================================
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  // transposed-read lane geometry (see wgrad.hip): group tg = lane >> 4 covers columns 16 (tg & 1) .., rows 8 (tg >> 1) + tq (+4)
  const int tg = lane >> 4, ti = lane & 15, tq = ti >> 2, tp = ti & 3;
  const int acol = ((32 * wave + 16 * (tg & 1) + 4 * tp) * 2) ^ (tq << 6);  // row & 3 == tq for every row this lane reads
  const int arow = 8 * (tg >> 1) + tq;
  const int ycol = (16 * (tg & 1) + 4 * tp) * 2;
  int yoff[9];  // halo offset of (pixel x = arow of the k-step's tile row, tap)
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int tw = taps.t[t];
    const int dy = (int)(signed char)(tw & 0xff), dx = (int)(signed char)((tw >> 8) & 0xff);
    yoff[t] = ((1 + dy) * W3_HW + (arow + 1 + dx)) * 64 + ycol;
  }
  for (int k = 0; k < nt; ++k) {
    lds_barrier();  // barrier k: image k & 1 is complete
    const unsigned char* As = smem + (k & 1) * W3_IMG;
    const unsigned char* Ys = As + W3_A_BYTES;
    if (!(WG3_DBG & 2)) {
#pragma unroll 2
      for (int ms = 0; ms < W3_TH; ++ms) {  // one tile row = 16 pixels of the contraction per step
        const unsigned char* ap = As + (16 * ms + arow) * 256 + acol;
        const V af = frag16<T>(lds_tr16(ap), lds_tr16(ap + 4 * 256));
        const unsigned char* yp = Ys + ms * (W3_HW * 64);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const V bf = frag16<T>(lds_tr16(yp + yoff[t]), lds_tr16(yp + yoff[t] + 4 * 64));
          acc[t] = mma16(af, bf, acc[t]);
        }
      }
    }
  }

  // ---- the partial result: to this workgroup's slot (plain 16-byte stores) or added to the packed gradient dP[tap][c][n] ----
  // Slot layout = the accumulator layout: float4 j of tap t of wave w of lane l at (((t * 4 + w) * 4 + j) * 64 + l) * 4, i.e. every
  // store instruction writes 1 KB contiguous (36 per lane instead of 144 scalar ones); wg3_reduce_kernel knows the permutation.
  const int r = lane & 31, h = lane >> 5;
  if (slot != nullptr) {
    f32x4* s4 = (f32x4*)slot;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = {acc[t][4 * j], acc[t][4 * j + 1], acc[t][4 * j + 2], acc[t][4 * j + 3]};
        if (!(WG3_DBG & 1) || v[0] == 1.2345e33f) s4[((t * 4 + wave) * 4 + j) * 64 + lane] = v;
      }
  } else {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (!(WG3_DBG & 1) || acc[t][i] == 1.2345e33f) atomic_add_f32(a.dpack + ((size_t)t * W3_CA + c) * 32 + r, acc[t][i]);
      }
  }
}

template <typename T, int PQ>
__global__ __launch_bounds__(W3_NT, 1) void wg3_kernel(const Wg3Args g) {
  const Seg& sy_ = g.w.seg[0];  // dY, nine taps
  const Seg& sa = g.w.dy;       // A, pixel aligned
  // (wg3_resolve: both operands have the launch's map size, Npad = 128)
  const W3View a = {sa.src, sy_.src, sy_.src2, sa.scale, sa.shift, sy_.q, sy_.r, g.w.dpack, sa.ld, sy_.ld, sy_.ld2, g.w.Ho, g.w.Wo, g.tiles_y, g.tiles_x};
  W3Taps taps;
#pragma unroll
  for (int t = 0; t < 9; ++t) taps.t[t] = sy_.taps[t];
  const int t_beg = blockIdx.x * g.tiles_per_wg;
  wg3_walk<T, PQ>(a, taps, t_beg, min(g.ntiles, t_beg + g.tiles_per_wg), g.part ? g.part + (size_t)blockIdx.x * W3_SLOT_FLOATS : nullptr);
}

// The GROUPED launch: the weight gradients of up to W3_GROUP_MAX layers in one grid.  Late in the network a layer has one or two tiles
// per workgroup, and the launch, the prologue and the 147 KB hand-over are paid for those; the layers of a dense block are independent
// (each reads its own compact gradient and y1 and writes its own packed gradient), so the executor (capi.cpp run_ops) hands consecutive
// ones over together.  The table travels in the kernel argument (no upload).  Workgroups [wg0[i], wg0[i + 1]) belong to member i and
// walk its tiles exactly as wg3_kernel does; slot index = workgroup index, and wg3_group_reduce_kernel adds each member's slot range.
struct Wg3Member {
  W3View v;
  int ntiles, tiles_per_wg;
};
struct Wg3GroupArgs {
  float* part;
  int n;
  int wg0[W3_GROUP_MAX + 1];  // first workgroup of each member; [n] = the grid
  W3Taps taps;                // (the same for every member: wg3_group_fits)
  Wg3Member m[W3_GROUP_MAX];
};
static_assert(sizeof(Wg3GroupArgs) <= 3840, "the table is a kernel argument: 4 KB with the hidden arguments");
static_assert(sizeof(Wg3Member) % 8 == 0 && offsetof(Wg3GroupArgs, m) % 8 == 0, "members are read with aligned scalar loads");

template <typename T, int PQ>
__global__ __launch_bounds__(W3_NT, 1) void wg3_group_kernel(const Wg3GroupArgs g) {
  const int bid = blockIdx.x;
  int mi = 0;  // (uniform scan; wg0 is ascending)
#pragma unroll
  for (int i = 1; i < W3_GROUP_MAX; ++i)
    if (i < g.n && bid >= g.wg0[i]) mi = i;
  const Wg3Member& M = g.m[mi];
  const int t_beg = (bid - g.wg0[mi]) * M.tiles_per_wg;
  wg3_walk<T, PQ>(M.v, g.taps, t_beg, min(M.ntiles, t_beg + M.tiles_per_wg), g.part + (size_t)bid * W3_SLOT_FLOATS);
}

// dpack += sum of the slots, in a fixed order (no float atomics).  288 workgroups: thread (o, sg) adds the slots sg, sg + 8, ... of one
// float4 of the slot layout - all its loads are independent and in flight together - and the eight partial sums are added through
// LDS in the order sg = 0..7.  (First version: one thread per output walking ALL slots, 36 workgroups: 19 dependent rounds of
// loads, ~35 us per launch - more than the weight-gradient kernel itself on blocks 3-4.)
// float4 f of a slot = (tap t, wave w, quad j, lane l): accumulator elements 4j .. 4j+3 = channels 32 w + 8 j + 4 (l >> 5) + 0..3 of
// column n = l & 31 (the 32x32 MFMA result layout), i.e. four dP rows 128 bytes apart.
constexpr int W3_RG = 8;  // slot groups
__device__ __forceinline__ void wg3_reduce_slots(const float* __restrict__ part, float* __restrict__ dpack, int nslots) {
  __shared__ f32x4 red[W3_RG][32];
  const int o = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int f = blockIdx.x * 32 + o;
  const float* p = part + (size_t)f * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int k = sg;
  for (; k + 3 * W3_RG < nslots; k += 4 * W3_RG) {
    const f32x4 v0 = __builtin_nontemporal_load((const f32x4*)(p + (size_t)k * W3_SLOT_FLOATS));
    const f32x4 v1 = __builtin_nontemporal_load((const f32x4*)(p + (size_t)(k + W3_RG) * W3_SLOT_FLOATS));
    const f32x4 v2 = __builtin_nontemporal_load((const f32x4*)(p + (size_t)(k + 2 * W3_RG) * W3_SLOT_FLOATS));
    const f32x4 v3 = __builtin_nontemporal_load((const f32x4*)(p + (size_t)(k + 3 * W3_RG) * W3_SLOT_FLOATS));
    s += (v0 + v1) + (v2 + v3);
  }
  for (; k < nslots; k += W3_RG) s += __builtin_nontemporal_load((const f32x4*)(p + (size_t)k * W3_SLOT_FLOATS));
  red[sg][o] = s;
  __syncthreads();
  if (sg == 0) {
    f32x4 t4 = red[0][o];
#pragma unroll
    for (int g2 = 1; g2 < W3_RG; ++g2) t4 += red[g2][o];
    const int l = f & 63, j = (f >> 6) & 3, w = (f >> 8) & 3, t = f >> 10;
    float* d = dpack + ((size_t)t * W3_CA + 32 * w + 8 * j + 4 * (l >> 5)) * 32 + (l & 31);
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q * 32] += t4[q];
  }
}
__global__ __launch_bounds__(256) void wg3_reduce_kernel(const float* __restrict__ part, float* __restrict__ dpack, int nslots) {
  wg3_reduce_slots(part, dpack, nslots);
}
// The grouped form: blockIdx.y = member; the member's slot range in the same fixed order into the member's packed gradient.
struct Wg3ReduceGroupArgs {
  const float* part;
  int wg0[W3_GROUP_MAX + 1];
  float* dpack[W3_GROUP_MAX];
};
__global__ __launch_bounds__(256) void wg3_group_reduce_kernel(const Wg3ReduceGroupArgs g) {
  const int mi = blockIdx.y;
  const int s0 = g.wg0[mi];
  wg3_reduce_slots(g.part + (size_t)s0 * W3_SLOT_FLOATS, g.dpack[mi], g.wg0[mi + 1] - s0);
}

// What wg3_resolve hands to wg3_launch: the kernel's arguments but for the split over workgroups, and the instantiation that runs.
struct Wg3Launch {
  Wg3Args g;
  LdsLauncher<Wg3Args> run;
};

// Refused unless this is the transposed-form weight gradient of a 128 -> 32 channel 3x3 convolution in a 16-bit storage type.
bool wg3_resolve(const WgradArgs& a, int dtype, Resolved& r) {
  if (dtype == DT_F32 || a.nseg != 1) return false;
  const Seg& q = a.seg[0];
  const Seg& p = a.dy;
  if (q.mode != G_PLAIN || q.istride != 1 || q.ntaps != 9 || q.C != W3_CY || q.Cpad != W3_CY || q.Hs != a.Ho || q.Ws != a.Wo || q.scale != nullptr)
    return false;
  if (p.mode != G_PLAIN || p.istride != 1 || p.ntaps != 1 || p.taps[0] != 0 || p.C != W3_CA || p.Hs != a.Ho || p.Ws != a.Wo || p.scale == nullptr)
    return false;
  if (a.N != W3_CA || a.Npad != W3_CA) return false;
  bool seen[9] = {false, false, false, false, false, false, false, false, false};
  for (int t = 0; t < 9; ++t) {
    const int dy = (int)(signed char)(q.taps[t] & 0xff), dx = (int)(signed char)((q.taps[t] >> 8) & 0xff);
    if (dy < -1 || dy > 1 || dx < -1 || dx > 1 || seen[(dy + 1) * 3 + dx + 1]) return false;
    seen[(dy + 1) * 3 + dx + 1] = true;
  }
  Wg3Launch& l = r.put<Wg3Launch>();
  Wg3Args& g = l.g;
  g.w = a;
  g.tiles_y = (a.Ho + W3_TH - 1) / W3_TH;
  g.tiles_x = (a.Wo + W3_TW - 1) / W3_TW;
  g.ntiles = a.B * g.tiles_y * g.tiles_x;
  if (dtype == DT_F16) l.run = q.q ? launch_lds<wg3_kernel<f16, 2>, Wg3Args> : launch_lds<wg3_kernel<f16, 0>, Wg3Args>;
  else l.run = q.q ? launch_lds<wg3_kernel<bf16, 2>, Wg3Args> : launch_lds<wg3_kernel<bf16, 0>, Wg3Args>;
  return true;
}

// The workgroups of a launch with slots: one per compute unit (W3_MAX_SLOTS and the slots of the buffer cap it).
static int wg3_slot_wgs(int part_slots) {
  static const int cus = device_cus();
  static const int wgs_cap = lab_int("DMM_WG3_WGS", 0);
  int nwg = std::min(std::min(cus, W3_MAX_SLOTS), part_slots);
  if (wgs_cap > 0) nwg = std::min(nwg, wgs_cap);
  return std::max(1, nwg);
}
static bool wg3_use_slots() {
  static const bool use_slots = lab_int("DMM_WG3_SLOTS", 1) != 0;
  return use_slots;
}

hipError_t wg3_launch(const Resolved& r, hipStream_t st) {
  const Wg3Launch& l = r.get<Wg3Launch>();
  Wg3Args g = l.g;
  const WgradArgs& a = g.w;
  // Workgroups.  With slots: one per compute unit (8 waves each; W3_MAX_SLOTS caps it), every workgroup stores its 147 KB partial
  // and the reduction reads them once.  With atomics (no slots, DMM_WG3_SLOTS=0): time ~ tiles/nwg * t_tile + nwg * (147 KB of
  // fp32 atomics at the chip-wide atomic rate of 1.3 TB/s = 0.11 us): minimum at nwg ~ sqrt(t_tile / 0.11 us * tiles), t_tile ~ 1.3 us.
  static const int cus = device_cus();
  static const int wgs_cap = lab_int("DMM_WG3_WGS", 0);
  g.part = (wg3_use_slots() && a.part != nullptr) ? a.part : nullptr;
  int nwg = g.part ? std::min(cus, a.part_slots) : (int)std::lround(std::sqrt(12.0 * g.ntiles));
  if (wgs_cap > 0) nwg = std::min(nwg, wgs_cap);
  nwg = std::max(1, std::min(std::min(nwg, cus), g.ntiles));
  g.tiles_per_wg = (g.ntiles + nwg - 1) / nwg;
  nwg = (g.ntiles + g.tiles_per_wg - 1) / g.tiles_per_wg;
  hipError_t e = l.run(W3_LDS, nwg, W3_NT, W3_LDS, st, g);
  if (e == hipSuccess && g.part != nullptr) {  // same stream: the slots are reused by the next launch of the family
    hipLaunchKernelGGL(wg3_reduce_kernel, dim3(W3_SLOT_FLOATS / 4 / 32), dim3(256), 0, st, g.part, g.w.dpack, nwg);
    e = hipGetLastError();
  }
  return e;
}

// ---- the grouped launch (pointwise.h: Wg3Group) ----
struct Wg3GroupLaunch {
  Wg3GroupArgs g;
  LdsLauncher<Wg3GroupArgs> run;
};
static_assert(sizeof(Wg3GroupLaunch) <= sizeof(Wg3Group::block) && alignof(Wg3GroupLaunch) <= 16, "Wg3Group::block is too small");

template <typename T> static LdsLauncher<Wg3GroupArgs> wg3_group_runner(bool pq) {
  return pq ? launch_lds<wg3_group_kernel<T, 2>, Wg3GroupArgs> : launch_lds<wg3_group_kernel<T, 0>, Wg3GroupArgs>;
}

bool wg3_group_add(Wg3Group& G, const WgradArgs& a, int dtype) {
  if (!wg3_use_slots() || a.part == nullptr || a.part_slots < 1 || a.M <= 0) return false;
  Resolved r;
  if (!wg3_resolve(a, dtype, r)) return false;
  const Wg3Launch& l = r.get<Wg3Launch>();
  const Seg& sy_ = a.seg[0];
  const Seg& sa = a.dy;
  Wg3GroupLaunch& L = *reinterpret_cast<Wg3GroupLaunch*>(G.block);
  const int pq = sy_.q ? 2 : 0;
  W3Taps taps;
  memset(&taps, 0, sizeof(taps));
  for (int t = 0; t < 9; ++t) taps.t[t] = sy_.taps[t];
  if (G.n == 0) {
    memset(&L, 0, sizeof(L));
    L.g.part = a.part;
    L.g.taps = taps;
    L.run = dtype == DT_F16 ? wg3_group_runner<f16>(pq != 0) : wg3_group_runner<bf16>(pq != 0);
    G.dtype = dtype; G.pq = pq; G.part_slots = a.part_slots; G.tiles = 0;
  } else {
    // a member that does not fit: another kernel instantiation, other slots or taps, the member cap, or no workgroup left for it
    if (G.dtype != dtype || G.pq != pq || L.g.part != a.part || G.part_slots != a.part_slots || memcmp(&L.g.taps, &taps, sizeof(taps)) != 0) return false;
    if (G.n >= W3_GROUP_MAX || G.n >= wg3_slot_wgs(G.part_slots)) return false;
  }
  Wg3Member& m = L.g.m[G.n++];
  m.v = {sa.src, sy_.src, sy_.src2, sa.scale, sa.shift, sy_.q, sy_.r, a.dpack, sa.ld, sy_.ld, sy_.ld2, a.Ho, a.Wo, l.g.tiles_y, l.g.tiles_x};
  m.ntiles = l.g.ntiles;
  m.tiles_per_wg = 0;
  G.tiles += l.g.ntiles;
  return true;
}

// Workgroups are dealt in proportion to tiles: at least 1 per member, at most the member's tiles, at most wg3_slot_wgs in all (the
// members number at most that: wg3_group_add).  A pure function of the members and the device's compute units.
hipError_t wg3_group_launch(Wg3Group& G, hipStream_t st) {
  if (G.n <= 0) return hipSuccess;
  Wg3GroupLaunch& L = *reinterpret_cast<Wg3GroupLaunch*>(G.block);
  Wg3GroupArgs& g = L.g;
  const int n = G.n, W = wg3_slot_wgs(G.part_slots);
  int w[W3_GROUP_MAX], sum = 0;
  for (int i = 0; i < n; ++i) {
    w[i] = (int)std::max<long long>(1, std::min<long long>(g.m[i].ntiles, (long long)W * g.m[i].ntiles / G.tiles));
    sum += w[i];
  }
  while (sum > W) {  // (the rounding up to 1 of small members: taken from the member with the fewest tiles per workgroup)
    int k = -1;
    for (int i = 0; i < n; ++i)
      if (w[i] > 1 && (k < 0 || (long long)g.m[i].ntiles * w[k] < (long long)g.m[k].ntiles * w[i])) k = i;
    --w[k]; --sum;
  }
  for (int i = 0; i < n && sum < W; ++i)  // what the rounding down left over: one more each, in order
    if (w[i] < g.m[i].ntiles) { ++w[i]; ++sum; }
  int wg = 0;
  Wg3ReduceGroupArgs rg;
  memset(&rg, 0, sizeof(rg));
  rg.part = g.part;
  for (int i = 0; i < n; ++i) {
    Wg3Member& m = g.m[i];
    m.tiles_per_wg = (m.ntiles + w[i] - 1) / w[i];
    g.wg0[i] = wg; rg.wg0[i] = wg;
    rg.dpack[i] = m.v.dpack;
    wg += (m.ntiles + m.tiles_per_wg - 1) / m.tiles_per_wg;
  }
  for (int i = n; i <= W3_GROUP_MAX; ++i) { g.wg0[i] = wg; rg.wg0[i] = wg; }
  g.n = n;
  G.n = 0; G.tiles = 0;  // (handed over, whatever the runtime says)
  if (wg > G.part_slots) return hipErrorInvalidValue;  // (cannot happen: sum <= W <= part_slots)
  hipError_t e = L.run(W3_LDS, wg, W3_NT, W3_LDS, st, g);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wg3_group_reduce_kernel, dim3(W3_SLOT_FLOATS / 4 / 32, n), dim3(256), 0, st, rg);
  return hipGetLastError();
}

}  // namespace dmm
