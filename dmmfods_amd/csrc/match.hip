// Object matching on the device: detect.match_plane restated.  The records dmm_heat_components wrote for the predictions
// and for the ground truth of one batch are paired per (sample, class) plane, greedily: predictions in descending score (a float
// compare; ties to the ascending root), each taking the still untaken ground-truth record of highest IoU >= iou (ties to the lower root).
//   takes part   a record in a slot below min(count, cap) with area >= min_area, predictions and ground truth alike
//   IoU          box_iou term for term in fp64: double(iw) * double(ih) over area_a + area_b - inter, the areas from the corners;
//                every operand is an exact integer, the one rounding is the division (IEEE, no fast-math, contraction off)
//   order        a plane's records stand in ascending root order (dmm_heat_components' contract), so "the lower root" is the lower slot
// Three launches on one stream; the launch boundaries are the only ordering between them:
//   (a) match_count    one workgroup per plane: the participating predictions and ground-truth records of the plane
//   (b) match_offsets  one workgroup per class: the exclusive sum over the samples of (a)'s prediction counts, from totals' cursor on,
//                      is where each plane's entries start; ONE thread then adds the class sums to num_pred, num_gt, overflowed_planes
//                      and cursor
//   (c) match_plane    one workgroup per plane: compacts the participating predictions in LDS, ranks them by counting the keys in
//                      front of each ((-score, slot) is unique), walks them in that order - the 256 lanes stride over the ground
//                      truth, lane t owning the records t, t + 256, ... and their `taken` bits in a register; a wave reduction by
//                      shuffles and one LDS exchange across the four waves pick the winner - and writes matched, the entries and,
//                      with three 64-bit integer atomic adds, tp / fp / fn
// Every output is an integer or a copied input value and every global reduction is an integer add: the result depends neither on
// the grid nor on the order of arrival.  No floating-point atomics.  Slots behind min(count, cap) are never read.
#include <climits>

#include "common.h"
#include "pointwise.h"

namespace dmm {

namespace {

constexpr int MAXP = DMM_MATCH_MAX_PER_PLANE;
constexpr int LDS_GT = 1024;   // ground-truth boxes staged in LDS; the ones behind are read from global memory on every visit
static_assert(MAXP == 16 * 256, "a lane owns at most 16 ground-truth records: their `taken` bits are one 16-bit mask");
static_assert(LDS_GT % 256 == 0 && LDS_GT <= MAXP, "whole strides of the workgroup");
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int kept_of(int count, int cap) { return max(0, min(count, cap)); }
// (records are 8-byte aligned: the box is x0 at byte 4 .. y1 at byte 16)
__device__ __forceinline__ i32x4 box_of(const dmm_component* r) { return i32x4{r->x0, r->y0, r->x1, r->y1}; }

// box_iou (detect.py), fp64.  0.0 where the boxes do not overlap: that is below every admissible iou, the caller skips it.
#pragma clang fp contract(off)
__device__ __forceinline__ double box_iou(const i32x4 a, const i32x4 b) {
  const long long iw = (long long)min(a[2], b[2]) - max(a[0], b[0]) + 1;
  const long long ih = (long long)min(a[3], b[3]) - max(a[1], b[1]) + 1;
  if (iw <= 0 || ih <= 0) return 0.0;
  const double inter = (double)iw * (double)ih;
  const double area_a = (double)((long long)a[2] - a[0] + 1) * (double)((long long)a[3] - a[1] + 1);
  const double area_b = (double)((long long)b[2] - b[0] + 1) * (double)((long long)b[3] - b[1] + 1);
  return inter / (area_a + area_b - inter);
}

// the sum of v over the workgroup's 256 lanes, in every lane (wtot: four ints of LDS; a barrier stands in front of its reuse)
__device__ __forceinline__ int block_sum(int v, int* wtot) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = v;
  __syncthreads();
  return wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// (a) one workgroup per plane
__global__ __launch_bounds__(256) void match_count_kernel(MatchArgs a) {
  __shared__ int wtot[4];
  const int plane = blockIdx.x, tid = threadIdx.x;
  const int kp = kept_of(a.pred_counts[plane], a.cap_pred), kg = kept_of(a.gt_counts[plane], a.cap_gt);
  const dmm_component* P = a.pred + (size_t)plane * a.cap_pred;
  const dmm_component* G = a.gt + (size_t)plane * a.cap_gt;
  int np = 0, ng = 0;
  for (int i = tid; i < kp; i += 256) np += P[i].area >= a.min_area;
  for (int i = tid; i < kg; i += 256) ng += G[i].area >= a.min_area;
  np = block_sum(np, wtot);
  ng = block_sum(ng, wtot);
  if (tid == 0) { a.np[plane] = np; a.ng[plane] = ng; }
}

// (b) one workgroup per class: plane (b, n) is b * NC + n
__global__ __launch_bounds__(256) void match_offsets_kernel(MatchArgs a) {
  __shared__ long long wtot[2][4];
  __shared__ int rtot[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long* tot = a.totals + (size_t)n * 8;
  long long carry = tot[6];
  int ng = 0, over = 0;
  for (int base = 0, it = 0; base < a.B; base += 256, ++it) {   // workgroup-uniform trip count
    const int b = base + tid;
    const int plane = b * a.NC + n;
    long long v = 0;
    if (b < a.B) {
      v = a.np[plane];
      ng += a.ng[plane];
      over += (a.pred_counts[plane] > a.cap_pred) + (a.gt_counts[plane] > a.cap_gt);
    }
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wtot[it & 1][wave] = inc;
    __syncthreads();   // (two buffers, as in cc_scan_kernel)
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const long long t = wtot[it & 1][w]; total += t; if (w < wave) before += t; }
    if (b < a.B) a.base[plane] = carry + before + inc - v;
    carry += total;
  }
  ng = block_sum(ng, rtot);      // (at most 65535 planes of 4096 records: int32 holds the sums)
  over = block_sum(over, rtot);
  if (tid == 0) {
    tot[3] += carry - tot[6];   // num_pred
    tot[4] += ng;               // num_gt
    tot[5] += over;             // overflowed_planes
    tot[6] = carry;             // cursor: advances by the full number, whatever the capacity
  }
}

// (c) one workgroup per plane
__global__ __launch_bounds__(256) void match_plane_kernel(MatchArgs a) {
  __shared__ int s_bits[MAXP];              // by compact index: the score bits of the participating predictions, ascending slots
  __shared__ unsigned short s_slot[MAXP];   // by compact index: the slot
  __shared__ unsigned short s_order[MAXP];  // by rank: the compact index
  __shared__ unsigned char s_flag[MAXP];    // by slot: matched
  __shared__ i32x4 s_gt[LDS_GT];
  __shared__ double s_wv[2][4];
  __shared__ int s_wj[2][4];
  __shared__ int wtot[2][4];
  const int plane = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kp = kept_of(a.pred_counts[plane], a.cap_pred), kg = kept_of(a.gt_counts[plane], a.cap_gt);
  const dmm_component* P = a.pred + (size_t)plane * a.cap_pred;
  const dmm_component* G = a.gt + (size_t)plane * a.cap_gt;

  // the participating predictions, compacted in slot order
  int np = 0;
  for (int base = 0, it = 0; base < a.cap_pred; base += 256, ++it) {   // workgroup-uniform trip count
    const int i = base + tid;
    int bits = 0;
    bool part = false;
    if (i < kp) {
      part = P[i].area >= a.min_area;
      bits = __float_as_int(P[i].score);
    }
    if (i < a.cap_pred) s_flag[i] = 0;
    const unsigned long long m = __ballot(part);
    if (lane == 0) wtot[it & 1][wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int t = wtot[it & 1][w]; total += t; if (w < wave) before += t; }
    if (part) {
      const int c = np + before + __popcll(m & ((1ull << lane) - 1ull));
      s_bits[c] = bits;
      s_slot[c] = (unsigned short)i;
    }
    np += total;
  }
  // the ground truth: lane t owns the records t, t + 256, ...; bit k of `taken` is record t + 256 k.  A record that does not take
  // part is taken from the start.
  unsigned taken = 0;
  int ng = 0;
  const int gsteps = (kg + 255) >> 8;
  for (int k = 0; k < gsteps; ++k) {
    const int j = tid + (k << 8);
    bool part = false;
    if (j < kg) {
      part = G[j].area >= a.min_area;
      if (part && j < LDS_GT) s_gt[j] = box_of(G + j);
    }
    if (!part) taken |= 1u << k;
    ng += part;
  }
  __syncthreads();
  // rank: the keys in front of (-score, slot); compact indices ascend with the slots
  for (int c = tid; c < np; c += 256) {
    const float s = __int_as_float(s_bits[c]);
    int r = 0;
    for (int d = 0; d < np; ++d) {
      const float t = __int_as_float(s_bits[d]);
      r += (t > s) || (t == s && d < c);
    }
    s_order[r] = (unsigned short)c;
  }
  __syncthreads();
  // the walk
  int tp = 0;
  i32x4 next = i32x4{0, 0, 0, 0};
  // (min: the ranks are a permutation because scores are never NaN - NaN is not foreground; if one were, a rank would stay unwritten)
  auto slot_at = [&](int k) { return (int)s_slot[min((int)s_order[k], np - 1)]; };
  if (np > 0) next = box_of(P + slot_at(0));
  for (int k = 0; k < np; ++k) {
    const i32x4 pb = next;
    const int slot = slot_at(k);
    if (k + 1 < np) next = box_of(P + slot_at(k + 1));   // (in flight during this step's reduction)
    double best = -1.0;
    int bj = INT_MAX;
    for (int t = 0; t < gsteps; ++t) {
      if ((taken >> t) & 1u) continue;
      const int j = tid + (t << 8);
      const i32x4 gb = j < LDS_GT ? s_gt[j] : box_of(G + j);
      const double v = box_iou(pb, gb);
      if (v >= a.iou && v > best) { best = v; bj = j; }   // (j ascends: a strict > keeps the first of equal IoUs)
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const double ov = __shfl_xor(best, d, 64);
      const int oj = __shfl_xor(bj, d, 64);
      if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
    }
    if (lane == 0) { s_wv[k & 1][wave] = best; s_wj[k & 1][wave] = bj; }
    __syncthreads();   // (two buffers: the next step writes the other one, and the one after comes behind the next step's barrier)
    best = s_wv[k & 1][0]; bj = s_wj[k & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double ov = s_wv[k & 1][w];
      const int oj = s_wj[k & 1][w];
      if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
    }
    if (bj != INT_MAX) {           // workgroup-uniform
      ++tp;
      if ((bj & 255) == tid) taken |= 1u << (bj >> 8);   // its owner is the only lane that ever looks at it
      if (tid == 0) s_flag[slot] = 1;
    }
  }
  __syncthreads();
  // outputs: every slot of matched once; an entry per participating prediction, at its deterministic position
  if (a.matched) {
    unsigned char* M = a.matched + (size_t)plane * a.cap_pred;
    for (int i = tid; i < a.cap_pred; i += 256) M[i] = s_flag[i];
  }
  const long long first = a.base[plane];
  int* E = a.entries + (size_t)(plane % a.NC) * (size_t)a.capacity * 2;
  for (int c = tid; c < np; c += 256) {
    const long long pos = first + c;
    if (pos < a.capacity) { E[pos * 2] = s_bits[c]; E[pos * 2 + 1] = (int)s_flag[s_slot[c]]; }   // (entries are 4-byte aligned only)
  }
  ng = block_sum(ng, wtot[0]);
  if (tid == 0) {
    unsigned long long* tot = (unsigned long long*)(a.totals + (size_t)(plane % a.NC) * 8);
    if (tp) atomicAdd(tot + 0, (unsigned long long)tp);
    if (np - tp) atomicAdd(tot + 1, (unsigned long long)(np - tp));
    if (ng - tp) atomicAdd(tot + 2, (unsigned long long)(ng - tp));
  }
}

}  // namespace

MatchLayout match_layout(int planes) {
  MatchLayout l;
  l.np = 0;
  l.ng = ((size_t)planes * 4 + 15) / 16 * 16;
  l.base = l.ng + ((size_t)planes * 4 + 15) / 16 * 16;
  l.total = l.base + ((size_t)planes * 8 + 15) / 16 * 16;
  return l;
}

void match_grids(const MatchArgs& a, unsigned gx[MATCH_LAUNCHES]) {
  gx[0] = (unsigned)(a.B * a.NC); gx[1] = (unsigned)a.NC; gx[2] = (unsigned)(a.B * a.NC);
}

hipError_t launch_match(const MatchArgs& a, hipStream_t st) {
  unsigned gx[MATCH_LAUNCHES];
  match_grids(a, gx);
  // (a lab build, DMM_LAB=1: DMM_MATCH_LAUNCHES=k stops behind the first k launches - tools/match_cost.py times the prefixes and
  // reports each launch as a difference; the outputs of a cut call are not meaningful)
  const int n = lab_int("DMM_MATCH_LAUNCHES", MATCH_LAUNCHES);
  if (n > 0) hipLaunchKernelGGL(match_count_kernel, dim3(gx[0]), dim3(256), 0, st, a);
  if (n > 1) hipLaunchKernelGGL(match_offsets_kernel, dim3(gx[1]), dim3(256), 0, st, a);
  if (n > 2) hipLaunchKernelGGL(match_plane_kernel, dim3(gx[2]), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmm
