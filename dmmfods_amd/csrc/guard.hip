// The guarded optimiser step (gfx950): dynamic loss scale, skipped step on overflow, clipping by global norm - all decided on the
// device, nothing in the step synchronises with the host.  (torch.amp.GradScaler's rule + torch.nn.utils.clip_grad_norm_'s formula;
// the reference trains in fp32 and has neither: agents/Dense_U_Net_lidar_Agent.py:263-265.)
//   grad_sumsq     : one streaming pass over (a range of) the gradient arena -> one fp64 partial sum of squares per workgroup
//   guard_finalize : partials (fixed order) -> apply / skip, clip coefficient, Adam bias corrections of the APPLIED step, next scale
//   adam_guarded   : adam_kernel's arithmetic with its scalars read from the state block; writes nothing on a skipped step
//   adam_guarded_from : the same for a range whose own step count started late (dmm_adam_step_guarded_ranges, t0 > 0)
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
    g.grad_scale = 0.f;       // (adam_guarded_kernel does not read it on a skipped step)
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

// adam_kernel (pointwise.hip) with grad_scale, step_size and bc2_sqrt from the state block: same expressions, same order, same launch
// geometry.  A skipped step returns before the first store - no NaN reaches p, m or v through a product with zero.
__global__ __launch_bounds__(256) void adam_guarded_kernel(AdamArgs a, const dmm_guard_state* state) {
  if (state->found_inf) return;
  a.grad_scale = state->grad_scale;
  a.step_size = state->step_size;
  a.bc2_sqrt = state->bc2_sqrt;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (size_t)gridDim.x * blockDim.x) {
    float g = a.g[i] * a.grad_scale;
    float p = a.p[i];
    if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, p, g);
    const float m = a.beta1 * a.m[i] + (1.f - a.beta1) * g;
    const float v = a.beta2 * a.v[i] + (1.f - a.beta2) * g * g;
    a.m[i] = m;
    a.v[i] = v;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    a.p[i] = p - a.step_size * (m / denom);
  }
}

hipError_t launch_adam_guarded(const AdamArgs& a, const dmm_guard_state* state, hipStream_t st) {
  int grid = (int)((a.n + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(grid), dim3(256), 0, st, a, state);
  return hipGetLastError();
}

// adam_guarded_kernel for a range of the arena that became trainable at applied step t0 > 0 (an encoder released after the decoder
// has trained): torch counts steps per parameter, so the range is at step t - t0 with t = applied_steps, which guard_finalize has
// already advanced for this step.  step_size and bc2_sqrt are formed here, in double, by guard_finalize's expressions (every thread
// computes the same two numbers: a few hundred cycles against a streaming pass); grad_scale is the step's own, and the element
// arithmetic is adam_guarded_kernel's.  A skipped step, or a count that is not positive (a state block set back behind t0), writes nothing.
__global__ __launch_bounds__(256) void adam_guarded_from_kernel(AdamArgs a, const dmm_guard_state* state, float lr, long long t0) {
  if (state->found_inf) return;
  const long long t = (long long)state->applied_steps - t0;
  if (t < 1) return;
  const double bc1 = 1.0 - pow((double)a.beta1, (double)t), bc2 = 1.0 - pow((double)a.beta2, (double)t);
  a.grad_scale = state->grad_scale;
  a.step_size = (float)((double)lr / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (size_t)gridDim.x * blockDim.x) {
    float g = a.g[i] * a.grad_scale;
    float p = a.p[i];
    if (a.weight_decay != 0.f) g = fmaf(a.weight_decay, p, g);
    const float m = a.beta1 * a.m[i] + (1.f - a.beta1) * g;
    const float v = a.beta2 * a.v[i] + (1.f - a.beta2) * g * g;
    a.m[i] = m;
    a.v[i] = v;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    a.p[i] = p - a.step_size * (m / denom);
  }
}

hipError_t launch_adam_guarded_from(const AdamArgs& a, const dmm_guard_state* state, float lr, int64_t t0, hipStream_t st) {
  int grid = (int)((a.n + 255) / 256);
  if (grid > 4096) grid = 4096;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(adam_guarded_from_kernel, dim3(grid), dim3(256), 0, st, a, state, lr, (long long)t0);
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
