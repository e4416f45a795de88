// The guarded optimiser step (gfx950): dynamic loss scale, skipped step on overflow, clipping by global norm - all decided on the
// device, nothing in the step synchronises with the host.  (torch.amp.GradScaler's rule + torch.nn.utils.clip_grad_norm_'s formula;
// the reference trains in fp32 and has neither: agents/Dense_U_Net_lidar_Agent.py:263-265.)
//   grad_sumsq     : one streaming pass over (a range of) the gradient arena -> one fp64 partial sum of squares per workgroup
//   guard_finalize : partials (fixed order) -> apply / skip, clip coefficient, Adam bias corrections of the APPLIED step, next scale
//   adam_segmented : THE Adam kernel (torch.optim.Adam semantics, amsgrad off; AdamW's decay per class).  It walks the arena under a
//                    segment table - parameter groups and frozen gaps in one launch - or, without a table, one whole range; plain path
//                    (scalars from the host) and guarded path (scalars from the state block; writes nothing on a skipped step)
//                    and, asked to (AdamSegArgs::ema), keeps an exponential moving average of the parameters it writes
//   guard_init     : fills a state block (start of training, checkpoint load)
// No floating-point atomics anywhere: a workgroup owns its partial, the finalize kernel adds the partials in a fixed tree, so the
// norm, the decision and the step are bit-reproducible from run to run (and equal on every rank of a data-parallel job, which reads
// the same all-reduced arena).
#include "common.h"
#include "pointwise.h"

namespace dmm {

namespace {
// !isfinite without relying on what compiler flags leave of x != x: all exponent bits set
__device__ __forceinline__ bool nonfinite_f64(double x) {
  return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}
__device__ __forceinline__ double sq_acc(double acc, float x) {
  const double d = (double)x;  // a square of an fp32 value is exact in fp64; the fma rounds once
  return fma(d, d, acc);
}
__device__ __forceinline__ double sq_acc4(double acc, const f32x4& v) {
  return sq_acc(sq_acc(sq_acc(sq_acc(acc, v[0]), v[1]), v[2]), v[3]);
}
}  // namespace

// Grid: exactly GUARD_PARTIALS workgroups of 256 threads, whatever n is (two per compute unit; a grid-stride loop walks the range),
// so that every partial is written by every launch.  A range need not start on a 16-byte boundary (a gradient bucket starts at a
// tensor): up to three leading and three trailing elements are read one by one, everything between with 16-byte loads, four of them
// (64 bytes per thread, 16 KB per workgroup) in flight per step.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradSumsqArgs a) {
  __shared__ double red[4];
  const size_t T = (size_t)gridDim.x * blockDim.x, gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t head = (size_t)(((16u - (unsigned)((uintptr_t)a.g & 15u)) & 15u) >> 2);
  if (head > a.n) head = a.n;
  const size_t nv = (a.n - head) >> 2, tail0 = head + (nv << 2);
  const f32x4* gv = (const f32x4*)(a.g + head);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  size_t i = gid;
  for (; i + 3 * T < nv; i += 4 * T) {
    const f32x4 v0 = gv[i], v1 = gv[i + T], v2 = gv[i + 2 * T], v3 = gv[i + 3 * T];
    s0 = sq_acc4(s0, v0); s1 = sq_acc4(s1, v1); s2 = sq_acc4(s2, v2); s3 = sq_acc4(s3, v3);
  }
  for (; i < nv; i += T) s0 = sq_acc4(s0, gv[i]);
  if (gid < head) s1 = sq_acc(s1, a.g[gid]);
  if (tail0 + gid < a.n) s2 = sq_acc(s2, a.g[tail0 + gid]);
  double s = (s0 + s1) + (s2 + s3);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double w = (red[0] + red[1]) + (red[2] + red[3]);
    a.partials[blockIdx.x] = a.accumulate ? a.partials[blockIdx.x] + w : w;
  }
}

hipError_t launch_grad_sumsq(const GradSumsqArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GUARD_PARTIALS), dim3(256), 0, st, a);
  return hipGetLastError();
}

// One wave.  Lane l adds partials l, l + 64, ... in that order, then the 64 lane sums go down a fixed shuffle tree.
__global__ __launch_bounds__(64) void guard_finalize_kernel(GuardFinalizeArgs a) {
  double s = 0.0;
  for (int k = threadIdx.x; k < GUARD_PARTIALS; k += 64) s += a.partials[k];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if (threadIdx.x != 0) return;
  dmm_guard_state& g = *a.state;
  const float S = g.scale;
  g.sumsq = s;
  if (nonfinite_f64(s)) {
    // skipped: parameters, both moments and the applied-step count stay; step_size / bc2_sqrt are left as the last applied step's
    g.found_inf = 1;
    g.grad_norm = (float)s;   // inf or NaN: says which
    g.clip_coef = 0.f;
    g.grad_scale = 0.f;       // (the Adam kernel does not read it on a skipped step)
    g.skipped_steps += 1;
    g.growth_tracker = 0;
    const float ns = S * a.backoff_factor;
    if (ns > 0.f) g.scale = ns;   // never down to 0: 1 / scale must stay finite
    return;
  }
  const double norm = sqrt(s) / (double)S;
  double coef = 1.0;
  if (a.max_norm > 0.f) { coef = (double)a.max_norm / (norm + 1e-6); if (coef > 1.0) coef = 1.0; }
  const int64_t t = g.applied_steps + 1;
  const double bc1 = 1.0 - pow((double)a.beta1, (double)t), bc2 = 1.0 - pow((double)a.beta2, (double)t);
  g.found_inf = 0;
  g.grad_norm = (float)norm;
  g.clip_coef = (float)coef;
  g.grad_scale = (float)(coef / (double)S);
  g.step_size = (float)((double)a.lr / bc1);
  g.bc2_sqrt = (float)sqrt(bc2);
  g.applied_steps = t;
  int tr = g.growth_tracker;
  if (tr < 0x7fffffff) ++tr;
  if (a.growth_interval > 0 && tr >= a.growth_interval) {
    const float ns = S * a.growth_factor;
    if (ns < __builtin_huge_valf()) g.scale = ns;   // never up to inf
    tr = 0;
  }
  g.growth_tracker = tr;
}

hipError_t launch_guard_finalize(const GuardFinalizeArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ Adam
// The project's Adam arithmetic for one element, with the scalars of the element's class.  This function IS its definition, rounding
// points included (fp32 throughout, contraction off, so nothing is fused that is not written as an fma):
//   g  = g * grad_scale                                  one rounding
//   p  = p * decay                                       decoupled classes only (AdamW), one rounding; they have weight_decay == 0 here
//   g  = fma(weight_decay, p, g)                         L2 classes with weight_decay != 0 only, one rounding
//   m  = beta1 * m + (1 - beta1) * g                     four roundings: 1 - beta1, each product, the sum
//   v  = beta2 * v + ((1 - beta2) * g) * g               five roundings: 1 - beta2, each of the three products, the sum
//   d  = sqrt(v) / bc2_sqrt + eps                        three roundings: root, quotient, sum
//   p  = fma(-step_size, m / d, p)                       two roundings: the quotient, then the ONE fused multiply-add
// (step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) are formed in double and rounded to fp32 once, on the host or, guarded,
// in the kernel.)  Checkpoints and the recorded bits of tests/golden/adam_bits_sha256.json depend on every line: left to the compiler's
// contraction, the four-element form below would fuse the moment lines (packed fma) and change last bits.
__device__ __forceinline__ void adam_seg_elem(float& p, float g, float& m_, float& v_, const AdamSegClass& c, float grad_scale) {
#pragma clang fp contract(off)
  g = g * grad_scale;
  if (c.decoupled) p = p * c.decay;
  if (c.weight_decay != 0.f) g = fmaf(c.weight_decay, p, g);
  const float m = c.beta1 * m_ + (1.f - c.beta1) * g;
  const float v = c.beta2 * v_ + (1.f - c.beta2) * g * g;
  m_ = m;
  v_ = v;
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = fmaf(-c.step_size, m / denom, p);
}

// The parameter average (AdamSegArgs::ema), for one element, contraction off as above.  p is the parameter this launch has just computed,
// e the stored average, omd = (float)(1 - d_k) with the decay d_k of this update formed in double and rounded once:
//   d  = p - e                                           one rounding
//   e  = fma(omd, d, e)                                  one rounding (the ONE fused multiply-add)
// It comes after p is final and reads nothing Adam writes later, so p, m and v have the bits of a launch without an average.
__device__ __forceinline__ void ema_elem(float& e, float p, float omd) {
#pragma clang fp contract(off)
  const float d = p - e;
  e = fmaf(omd, d, e);
}

// ema: the average's arena, or nullptr (uniform over the launch: off, or this update's k is below 1)
__device__ __forceinline__ void adam_seg_vec(const AdamSegArgs& a, size_t i, const AdamSegClass& c, float grad_scale, float* ema, float omd) {
  f32x4 p = *(const f32x4*)(a.p + i), m = *(const f32x4*)(a.m + i), v = *(const f32x4*)(a.v + i);
  const f32x4 g = *(const f32x4*)(a.g + i);
  // The average is fetched with the other four: behind the stores below the compiler may not move the load up (the arenas could alias
  // for all it knows), and that second round trip to memory per chunk cost 16 us on C2's arena.  It is read and written once per
  // step and by nothing else in between, hence the non-temporal hint on both accesses: measured, 165 -> 151 us on one chip against
  // 118 us without an average - the 8 B/element at the rate of the other 28 (profiles/r11/ema_cost.txt).
  f32x4 e = {0.f, 0.f, 0.f, 0.f};
  if (ema != nullptr) e = __builtin_nontemporal_load((const f32x4*)(ema + i));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pk = p[k], mk = m[k], vk = v[k];
    adam_seg_elem(pk, g[k], mk, vk, c, grad_scale);
    p[k] = pk; m[k] = mk; v[k] = vk;
  }
  *(f32x4*)(a.m + i) = m;
  *(f32x4*)(a.v + i) = v;
  *(f32x4*)(a.p + i) = p;
  if (ema != nullptr) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float ek = e[k];
      ema_elem(ek, p[k], omd);
      e[k] = ek;
    }
    __builtin_nontemporal_store(e, (f32x4*)(ema + i));
  }
}

// One launch for every parameter group.  Grid: min(chunks, ADAM_SEG_MAX_GRID) workgroups of 256 threads; a workgroup takes chunks
// blockIdx.x, + gridDim.x, ... of ADAM_SEG_CHUNK elements, a thread the 4 elements at chunk + 4 * threadIdx.x.  first[chunk] names the
// first segment that can touch the chunk, so nothing is searched from the table's start:
//   * no segment reaches into the chunk (a frozen range): the workgroup moves on without touching the arenas;
//   * one segment covers the whole chunk (nearly every chunk of a real table): every thread takes the 16-byte path with that
//     segment's class - the branch is uniform and no thread reads the table again;
//   * otherwise a thread walks on from first[chunk] to its own elements: a vector that lies inside one segment still moves as 16 bytes,
//     a vector across an edge, in a gap or past n goes element by element, each element under the class of its own segment.
// Whole-range form (a.segs == nullptr; dmm_adam_step, dmm_adam_step_guarded): the table is one implicit segment [0, n) of class 0 and
// neither segs nor first is read - every chunk but the last is the covered case, the ragged tail and arenas that are not 16-byte aligned
// (a caller's offset pointers) the element case.
// The classes sit in LDS (a thread's class index is not uniform at an edge).  Guarded path (a.state): a skipped step returns before
// the first store - no NaN reaches p, m or v through a product with zero; torch counts steps per parameter, so a class that became
// trainable at applied step t0 is at step t = applied_steps - t0 (guard_finalize has already advanced applied_steps for this step), and
// thread c forms class c's step_size = (float)(lr / (1 - beta1^t)) and bc2_sqrt = (float)sqrt(1 - beta2^t) in double - guard_finalize's
// expressions - once per workgroup; a class with t < 1 (a state block set back behind t0) writes nothing.
// The parameter average (a.ema, else nullptr: no instruction below touches it): the average is written exactly where p is, by the
// thread that holds the new p in registers - nowhere on a skipped step, in a gap, past n or for an inactive class.  Plain path: omd comes
// with the launch.  Guarded path: update k = applied_steps - a.ema_t0; thread ADAM_MAX_CLASSES forms omd = (float)(1 - d_k) in double,
// once per workgroup, next to the classes' scalars; k < 1 writes no average.
// Every element is owned by one thread of one workgroup: no atomics, and the result does not depend on the grid.
__device__ __forceinline__ AdamSegDev adam_seg_at(const AdamSegArgs& a, int s, long long n) {
  return a.segs != nullptr ? a.segs[s] : AdamSegDev{0, n, 0, 0};
}

__global__ __launch_bounds__(256) void adam_segmented_kernel(AdamSegArgs a) {
  __shared__ AdamSegClass cls[ADAM_MAX_CLASSES];
  __shared__ float ema_omd_lds;
  __shared__ int ema_on_lds;
  if (a.state != nullptr && a.state->found_inf) return;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < ADAM_MAX_CLASSES; ++c)
      if (c < a.nclasses) cls[c] = a.cls[c];
  }
  __syncthreads();
  float grad_scale = a.grad_scale;
  if (a.state != nullptr) {
    grad_scale = a.state->grad_scale;
    if ((int)threadIdx.x < a.nclasses) {
      AdamSegClass& c = cls[threadIdx.x];
      const long long t = (long long)a.state->applied_steps - c.t0;
      if (t < 1) {
        c.active = 0;
      } else {
        const double bc1 = 1.0 - pow((double)c.beta1, (double)t), bc2 = 1.0 - pow((double)c.beta2, (double)t);
        c.step_size = (float)((double)c.lr / bc1);
        c.bc2_sqrt = (float)sqrt(bc2);
        c.active = 1;
      }
    }
    if (a.ema != nullptr && threadIdx.x == ADAM_MAX_CLASSES) {
      const long long k = (long long)a.state->applied_steps - a.ema_t0;
      double d = (double)a.ema_decay;
      if (a.ema_warmup) {
        const double w = (1.0 + (double)k) / (10.0 + (double)k);
        if (w < d) d = w;
      }
      ema_omd_lds = (float)(1.0 - d);
      ema_on_lds = k >= 1 ? 1 : 0;
    }
    __syncthreads();
  }
  float* ema = a.ema;
  float omd = a.ema_omd;
  if (a.ema != nullptr && a.state != nullptr) {   // (uniform)
    omd = ema_omd_lds;
    if (!ema_on_lds) ema = nullptr;
  }
  const long long n = (long long)a.n;
  // (a 32-bit chunk counter keeps the loop's test on the scalar unit: nchunks < 2^31 and the grid is at most ADAM_SEG_MAX_GRID)
  for (unsigned ch = blockIdx.x; ch < (unsigned)a.nchunks; ch += gridDim.x) {
    const long long c0 = (long long)ch * ADAM_SEG_CHUNK, c1 = c0 + ADAM_SEG_CHUNK;
    int s = 0, sc = 0;
    long long sb = 0, se = n;                                 // the implicit segment of the whole-range form
    if (a.segs != nullptr) {                                  // (uniform: the three fields are fetched together, one step behind first[ch])
      s = a.first[ch];
      if (s < 0 || s >= a.nsegs) continue;
      sb = a.segs[s].begin; se = a.segs[s].end; sc = a.segs[s].cls;
    }
    if (sb >= c1) continue;                                   // nothing trainable in this chunk
    const long long base = c0 + 4 * (long long)threadIdx.x;
    if (a.vec_ok && sb <= c0 && c1 <= se && se <= n) {        // one segment covers the chunk
      const AdamSegClass& c = cls[sc & (ADAM_MAX_CLASSES - 1)];
      if (c.active) adam_seg_vec(a, (size_t)base, c, grad_scale, ema, omd);
      continue;
    }
    while (s < a.nsegs && adam_seg_at(a, s, n).end <= base) ++s;
    if (s >= a.nsegs) continue;
    {
      const AdamSegDev t = adam_seg_at(a, s, n);
      if (a.vec_ok && t.begin <= base && base + 4 <= t.end && t.end <= n) {
        const AdamSegClass& c = cls[t.cls & (ADAM_MAX_CLASSES - 1)];
        if (c.active) adam_seg_vec(a, (size_t)base, c, grad_scale, ema, omd);
        continue;
      }
    }
    for (int k = 0; k < 4; ++k) {
      const long long i = base + k;
      if (i >= n) break;
      while (s < a.nsegs && adam_seg_at(a, s, n).end <= i) ++s;
      if (s >= a.nsegs) break;
      const AdamSegDev t = adam_seg_at(a, s, n);
      if (t.begin > i) continue;                              // a gap
      const AdamSegClass& c = cls[t.cls & (ADAM_MAX_CLASSES - 1)];
      if (!c.active) continue;
      float p = a.p[i], m = a.m[i], v = a.v[i];
      adam_seg_elem(p, a.g[i], m, v, c, grad_scale);
      a.m[i] = m;
      a.v[i] = v;
      a.p[i] = p;
      if (ema != nullptr) {
        float e = ema[i];
        ema_elem(e, p, omd);
        ema[i] = e;
      }
    }
  }
}

hipError_t launch_adam_segmented(const AdamSegArgs& a, hipStream_t st) {
  int grid = a.nchunks < ADAM_SEG_MAX_GRID ? a.nchunks : ADAM_SEG_MAX_GRID;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adam_segmented_kernel, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

__global__ void guard_init_kernel(dmm_guard_state* g, float scale, long long applied, int tracker) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  g->scale = scale;
  g->grad_scale = 0.f;
  g->sumsq = 0.0;
  g->grad_norm = 0.f;
  g->found_inf = 0;
  g->applied_steps = applied;
  g->skipped_steps = 0;
  g->growth_tracker = tracker;
  g->step_size = 0.f;
  g->bc2_sqrt = 1.f;
  g->clip_coef = 1.f;
  g->reserved[0] = g->reserved[1] = 0;
}

hipError_t launch_guard_init(dmm_guard_state* dev, float scale, int64_t applied, int32_t tracker, hipStream_t st) {
  hipLaunchKernelGGL(guard_init_kernel, dim3(1), dim3(64), 0, st, dev, scale, (long long)applied, (int)tracker);
  return hipGetLastError();
}

}  // namespace dmm
