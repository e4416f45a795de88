// Validation threshold sweep: per-class histograms of the logits, split by ground truth, in one pass.
//   bin = #{k : x >= thr[k]}  (0..K, fp32 comparison: a NaN logit fails every one and lands in bin 0)
//   g   = t >= gt ? 1 : 0     (a NaN target: 0)
//   counts[b][n][g][bin] += 1        int64 [B][NC][2][K + 1]
// Every thresholded count (tp, fp, fn, tn at every threshold) is a suffix sum of those integers (dmmfods_amd/metrics.py).
//
// A workgroup belongs to ONE (b, n) plane (gridDim.y = B * NC) and keeps one uint32 hist[2][256] in LDS; H * W < 2^31 (the entry
// point refuses more) so no bin of it can overflow.  Thresholds sit in LDS padded to 256 with NaN: the predicate x >= thr[i] is true
// then false along the padded array (NaN pads are false), so eight branch-free halving steps count the true ones.
// Most pixels of a real heat map hold the same (g, bin) - a far-negative logit, no object - so most of a wave instruction's sixty-four
// LDS atomics meet on one address and serialise.  A wave therefore aggregates first: the pair of its first lane is broadcast, the
// lanes that hold the same pair are balloted, ONE lane adds their number; the lanes left over add 1 each.  ONE such round, not
// more: measured at C2's validation shape (profiles/r12/threshold_sweep_cost.txt), with 95 % of the logits in one bin one round takes
// 130 us where plain per-lane adds take 163 and four rounds 215; with the logits uniform over the bins - where a round serves a lane
// or two - it takes 127 us against 100 and 223.  Each round is a scalar chain (find lane, read lane, compare, ballot, count) that
// costs a wave more than the few serialised adds it saves once the majority bin is gone.  ROUNDS is a template parameter so that a
// lab build can measure the other two forms.
// The flush is 64-bit INTEGER atomic adds to `counts`: they commute exactly, so the result depends neither on the grid nor on the
// order of arrival.  No floating-point atomics anywhere.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "pointwise.h"

namespace dmm {

namespace {

template <int ROUNDS>
__device__ __forceinline__ void hist_add(unsigned* hist, int key, bool active) {
  // (called by whole waves only: every loop around it has a wave-uniform trip count)
  unsigned long long todo = __ballot(active);
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int r = 0; r < ROUNDS && todo != 0; ++r) {
    const int lead = __ffsll((long long)todo) - 1;
    const int k = __builtin_amdgcn_readlane(key, lead);
    const unsigned long long same = __ballot(active && key == k);
    if (lane == lead) atomicAdd(&hist[k], (unsigned)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&hist[key], 1u);
}

// the number of leading thresholds that x reaches: eight halving steps over the NaN-padded array of 256 (thr[255] is always a pad)
__device__ __forceinline__ int hist_bin(const float* thr, float x) {
  int pos = 0;
#pragma unroll
  for (int step = 128; step > 0; step >>= 1) pos += (x >= thr[pos + step - 1]) ? step : 0;
  return pos;
}

template <int ROUNDS>
__global__ __launch_bounds__(256) void logit_hist_kernel(LogitHistArgs a) {
  __shared__ float thr[256];
  __shared__ unsigned hist[2 * 256];
  const int tid = threadIdx.x;
  thr[tid] = tid < a.K ? a.thr[tid] : __builtin_nanf("");
  hist[tid] = 0u;
  hist[256 + tid] = 0u;
  __syncthreads();
  const size_t plane = (size_t)a.H * a.W;
  const size_t pl = blockIdx.y;   // b * NC + n
  const float* xs = a.logits + pl * plane;
  const float* ts = a.target + pl * plane;
  // 16-byte loads of four consecutive pixels; the next step's pair of loads is issued before this step's pixels are binned
  const bool vec4 = (plane & 3) == 0 && ((((uintptr_t)xs) | ((uintptr_t)ts)) & 15) == 0;
  if (vec4) {
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    size_t base = (size_t)blockIdx.x * 256 * 4;   // workgroup-uniform, as is the trip count
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, tv = xv;
    if (base + (size_t)tid * 4 < plane) { xv = *(const f32x4*)(xs + base + (size_t)tid * 4); tv = *(const f32x4*)(ts + base + (size_t)tid * 4); }
    for (; base < plane; base += stride) {
      const bool active = base + (size_t)tid * 4 < plane;
      const size_t nxt = base + stride + (size_t)tid * 4;
      f32x4 xn = {0.f, 0.f, 0.f, 0.f}, tn = xn;
      if (nxt < plane) { xn = *(const f32x4*)(xs + nxt); tn = *(const f32x4*)(ts + nxt); }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = (tv[j] >= a.gt ? 256 : 0) + hist_bin(thr, xv[j]);
        hist_add<ROUNDS>(hist, key, active);
      }
      xv = xn; tv = tn;
    }
  } else {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < plane; base += stride) {
      const size_t p = base + tid;
      const bool active = p < plane;
      const float x = active ? xs[p] : 0.f, t = active ? ts[p] : 0.f;
      const int key = (t >= a.gt ? 256 : 0) + hist_bin(thr, x);
      hist_add<ROUNDS>(hist, key, active);
    }
  }
  __syncthreads();
  if (tid <= a.K) {
    unsigned long long* out = a.counts + pl * 2 * (size_t)(a.K + 1);
    const unsigned c0 = hist[tid], c1 = hist[256 + tid];
    if (c0) atomicAdd(out + tid, (unsigned long long)c0);
    if (c1) atomicAdd(out + (a.K + 1) + tid, (unsigned long long)c1);
  }
}

}  // namespace

int logit_hist_grid_x(int planes, size_t plane) {
  // About two workgroups per compute unit in all (launch_bce_metrics' reasoning: enough loads in flight, few flushes), and on small
  // planes no more than one step of four pixels per thread.
  static const int wgs = lab_int("DMM_HIST_WGS", 512);
  int gx = std::max(1, wgs / std::max(1, planes));
  return std::min(gx, (int)((plane + 256 * 4 - 1) / (256 * 4)));
}

hipError_t launch_logit_hist(const LogitHistArgs& a, int accumulate, hipStream_t st) {
  const size_t plane = (size_t)a.H * a.W;
  const int planes = a.B * a.NC;
  if (!accumulate) {
    const hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)planes * 2 * (a.K + 1) * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
  }
  dim3 grid(logit_hist_grid_x(planes, plane), planes);
  // (a lab build: DMM_HIST_ROUNDS=0 is the kernel with plain per-lane adds, 4 the one with four rounds of aggregation in front of them -
  // what tools/threshold_sweep_cost.py compares against)
  static const int rounds = lab_int("DMM_HIST_ROUNDS", 1);
  if (rounds == 0) hipLaunchKernelGGL(logit_hist_kernel<0>, grid, dim3(256), 0, st, a);
  else if (rounds == 1) hipLaunchKernelGGL(logit_hist_kernel<1>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(logit_hist_kernel<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmm
