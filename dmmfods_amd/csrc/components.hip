// Heat maps to objects: threshold a (B, NC, H, W) fp32 map, label the connected components of every (b, n) plane and
// emit one record per component (box, area, largest value, where it first occurs).
//   foreground   x >= thr in fp32: a value on the threshold is in, NaN is out, -0.0 >= 0.0 holds
//   label        the component's ROOT, the smallest y * W + x among its pixels (plane-relative int32); background -1
//   records      per plane in ascending root order, the first `cap` of them; counts[plane] is the true number
// Seven launches on one stream; the launch boundaries are the only ordering between them (no spin-wait, no grid barrier):
//   (a) cc_local    one workgroup per 32 x 32 tile: union-find in LDS, labels written as plane-relative indices of the tile's roots
//   (b) cc_merge    the border pixels of every tile join their neighbours in other tiles: global union-find, atomicMin on the larger root
//   (c) cc_flatten  label[p] = find(p); roots (label[p] == p) are counted per segment of CC_SEG pixels, consecutive in raster order
//   (d) cc_scan     per plane, the exclusive scan of the segment counts; its total is counts[plane]
//   (e) cc_slots    every root's slot = its segment's offset + its rank in the segment: ascending root order, whatever arrives first;
//                   the slots below `cap` get a record with the root and the identities of the reductions of (f)
//   (f) cc_stats    every foreground pixel adds into its root's record: integer min / max / add, and ONE 64-bit integer atomicMax on
//                   (ordered value bits << 32) | ~index, which yields the largest value AND the first pixel that holds it
//                   (folded by root per thread, then per tile in an LDS table: one update per root and tile reaches the record)
//   (g) cc_finish   unpacks that 64-bit word into score and peak; zero-fills the slots behind min(count, cap)
// Every global reduction is an integer atomic: they commute exactly, so labels, records and counts depend neither on the grid nor on
// the order of arrival.  No floating-point atomics anywhere.
//
// Coherence (MI355X: eight XCDs, each with an L2 of its own; a plain load may be served from a line that does not hold another
// XCD's atomic of the same launch).  In (b) and (c) EVERY access to the label array is a relaxed agent-scope atomic (load, min or
// store), so each value read is one that some access stored.  That is all union-find needs: label[x] only ever decreases and only
// ever holds a member of x's own component, so any value read - the newest or an older one - is a valid step towards the root, and
// a link is made only where atomicMin RETURNS the root it was aimed at (old == a: a was still a root when it was linked).  When it
// returns something else the work goes on from the returned value.  Between launches the stream orders everything: (a) has written
// every label before (b) reads one, (b)'s links are complete before (c) follows them, and (d) to (g) read what earlier launches wrote.
//
// DMM_CC_MUTATE (a lab build, never the library's): seven value-only mutations that the tests must catch, profiles/r15/components_parity.txt.
#include <algorithm>
#include <climits>

#include "common.h"
#include "pointwise.h"

#ifndef DMM_CC_MUTATE
#define DMM_CC_MUTATE 0
#endif

namespace dmm {

namespace {

constexpr int TH = CC_TILE_H, TW = CC_TILE_W;
static_assert(TW == 32 && TH * TW == 4 * 256, "a tile is 256 threads x four pixels of a row, eight threads per row");
static_assert(CC_SEG % 256 == 0, "a segment is a whole number of workgroup steps");
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool is_fg(float x, float thr) {
#if DMM_CC_MUTATE == 4
  return x > thr;
#else
  return x >= thr;
#endif
}

// ---- union-find in LDS (one tile) ----
__device__ __forceinline__ int lds_find(int* lab, int x) {
  int p;
  while ((p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
  return x;
}
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  a = lds_find(lab, a);
  b = lds_find(lab, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lab[a], b);
    if (old == a) break;        // a was a root and now hangs below b
    a = lds_find(lab, old);     // a had a parent: that parent's set and b's still have to meet
    b = lds_find(lab, b);
  }
}

// ---- union-find in global memory (one plane); see Coherence above ----
__device__ __forceinline__ int ld_label(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* L, int x) {
  int p;
  while ((p = ld_label(L + x)) != x) x = p;
  return x;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
  a = g_find(L, a);
  b = g_find(L, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) break;
    a = g_find(L, old);
    b = g_find(L, b);
  }
}

// the four pixels (gy, gx0 .. gx0 + 3) of this thread: 16-byte load where every row of the plane starts on a 16-byte boundary
__device__ __forceinline__ void load_quad(const float* xs, int H, int W, int gy, int gx0, float v[4], bool in[4]) {
  const bool vec = (W & 3) == 0 && (((uintptr_t)xs) & 15) == 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { in[j] = gy < H && gx0 + j < W; v[j] = 0.f; }
  if (gy >= H || gx0 >= W) return;
  const float* row = xs + (size_t)gy * W + gx0;
  if (vec) {
    const f32x4 q = *(const f32x4*)row;   // (W % 4 == 0 and gx0 % 4 == 0: the quad is inside the row)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (in[j]) v[j] = row[j];
  }
}

// (a) one workgroup per tile
__global__ __launch_bounds__(256) void cc_local_kernel(ComponentsArgs a) {
  __shared__ int lab[TH * TW];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const size_t plane = (size_t)a.H * a.W;
  const float* xs = a.maps + (size_t)blockIdx.y * plane;
  int* L = a.labels + (size_t)blockIdx.y * plane;
  const int ly = tid >> 3, lx0 = (tid & 7) * 4;
  const int gy = ty * TH + ly, gx0 = tx * TW + lx0;
  float v[4];
  bool fg[4];
  load_quad(xs, a.H, a.W, gy, gx0, v, fg);
#if DMM_CC_MUTATE == 3
  if (gx0 >= (a.W / TW) * TW) { fg[0] = fg[1] = fg[2] = fg[3] = false; }
#endif
  const int li = ly * TW + lx0;
  // a pixel starts below the first pixel of its run inside the quad: parent < child, as everywhere
  int start = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fg[j] = fg[j] && is_fg(v[j], a.thr);
    if (!fg[j]) start = -1;
    else if (start < 0) start = li + j;
    lab[li + j] = fg[j] ? start : -1;
  }
  __syncthreads();
  // u[k + 1]: is the pixel above column lx0 + k foreground (k = -1 .. 4)
  bool u[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int x = lx0 + k - 1;
    u[k] = ly > 0 && x >= 0 && x < TW && lab[li - TW - lx0 + x] >= 0;
  }
  const bool left = lx0 > 0 && lab[li - 1] >= 0;
  // Only the unions that the others do not imply: a pixel behind a foreground pixel of its quad shares that pixel's links (the row
  // above is joined along itself), and where the pixel straight above is foreground the diagonal ones hang on it.
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!fg[j]) continue;
    const int i = li + j;
    const bool prev = j > 0 && fg[j - 1];
    if (j == 0 && left) lds_union(lab, i, i - 1);
    if (u[j + 1]) {
      if (!(prev && u[j])) lds_union(lab, i, i - TW);
    } else if (a.conn8) {
#if DMM_CC_MUTATE != 1
      if (u[j] && !prev) lds_union(lab, i, i - TW - 1);
      if (u[j + 2] && !(j < 3 && fg[j + 1])) lds_union(lab, i, i - TW + 1);
#endif
    }
  }
  __syncthreads();
  int out[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[j] = -1;
    if (fg[j]) {
      const int r = lds_find(lab, li + j);   // raster order inside the tile is raster order in the plane: the smallest local index
      out[j] = (ty * TH + (r >> 5)) * a.W + tx * TW + (r & 31);   // is the smallest plane index ((r >> 5, r & 31): TW == 32)
    }
  }
  if (gy >= a.H || gx0 >= a.W) return;
  int* row = L + (size_t)gy * a.W + gx0;
  if ((a.W & 3) == 0 && (((uintptr_t)L) & 15) == 0) {
    const i32x4 q = {out[0], out[1], out[2], out[3]};
    *(i32x4*)row = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (gx0 + j < a.W) row[j] = out[j];
  }
}

// (b) one workgroup per tile, one thread per pixel of its top row, left column and right column.  A pair of neighbours in different
// tiles is joined by the one of them that comes later in raster order: through its left, upper-left, upper or upper-right neighbour.
__global__ __launch_bounds__(128) void cc_merge_kernel(ComponentsArgs a) {
  const int tid = threadIdx.x;
  if (tid >= 96) return;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  int ly, lx;
  if (tid < 32) { ly = 0; lx = tid; }
  else if (tid < 64) { ly = tid - 32; lx = 0; if (ly == 0) return; }        // (the corners of the top row are served there)
  else { ly = tid - 64; lx = TW - 1; if (ly == 0) return; }
  const int gy = ty * TH + ly, gx = tx * TW + lx;
  if (gy >= a.H || gx >= a.W) return;
  int* L = a.labels + (size_t)blockIdx.y * ((size_t)a.H * a.W);
  const int p = gy * a.W + gx;
  const int lp = ld_label(L + p);
  if (lp < 0) return;
  const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, 0, -1, 1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= 2 && !a.conn8) break;
    const int qy = gy + dy[k], qx = gx + dx[k];
    if (qy < 0 || qx < 0 || qx >= a.W) continue;
    if (qy / TH == ty && qx / TW == tx) continue;   // inside this tile: (a) has joined them
#if DMM_CC_MUTATE == 2
    if (dy[k] != 0) continue;
#elif DMM_CC_MUTATE == 7
    if (qy / TH != ty && qx / TW != tx) continue;   // the neighbour across a tile CORNER
#endif
    const int lq = ld_label(L + (qy * a.W + qx));
    if (lq >= 0) g_union(L, lp, lq);
  }
}

// (c) one workgroup per segment: label[p] = find(p), and the number of roots in the segment
__global__ __launch_bounds__(256) void cc_flatten_kernel(ComponentsArgs a) {
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const size_t plane = (size_t)a.H * a.W;
  int* L = a.labels + (size_t)blockIdx.y * plane;
  const size_t base = (size_t)blockIdx.x * CC_SEG;
  int cnt = 0;
  for (int k = 0; k < CC_SEG / 256; ++k) {
    const size_t p = base + (size_t)k * 256 + tid;
    if (p >= plane) break;
    const int l = ld_label(L + p);
    if (l < 0) continue;
    const int r = g_find(L, l);   // (no link changes in this launch: another thread's store below only shortens a path to the same root)
    if (r != l) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    cnt += r == (int)p;
  }
  if (cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (tid == 0) a.seg[(size_t)blockIdx.y * a.nseg + blockIdx.x] = s_cnt;
}

// (d) one workgroup per plane: seg[] becomes its exclusive scan, counts[plane] the total
__global__ __launch_bounds__(256) void cc_scan_kernel(ComponentsArgs a) {
  __shared__ int wtot[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* seg = a.seg + (size_t)blockIdx.y * a.nseg;
  int carry = 0;
  for (int base = 0, it = 0; base < a.nseg; base += 256, ++it) {   // workgroup-uniform trip count
    const int i = base + tid;
    const int v = i < a.nseg ? seg[i] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) wtot[it & 1][wave] = inc;
    __syncthreads();   // (two buffers: the next step writes the other one, and the one after comes behind the next step's barrier)
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int t = wtot[it & 1][w]; total += t; if (w < wave) before += t; }
    if (i < a.nseg) seg[i] = carry + before + inc - v;
    carry += total;
  }
  if (tid == 0) a.counts[blockIdx.y] = carry;
}

// (e) one workgroup per segment: the roots of the segment, in raster order, take the slots from the segment's offset on
__global__ __launch_bounds__(256) void cc_slots_kernel(ComponentsArgs a) {
  __shared__ int wtot[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t plane = (size_t)a.H * a.W;
  const int* L = a.labels + (size_t)blockIdx.y * plane;
  dmm_component* rec = a.records + (size_t)blockIdx.y * a.cap;
  int running = a.seg[(size_t)blockIdx.y * a.nseg + blockIdx.x];
  const size_t base = (size_t)blockIdx.x * CC_SEG;
  for (int k = 0; k < CC_SEG / 256; ++k) {   // workgroup-uniform exits only
    if (running >= a.cap || base + (size_t)k * 256 >= plane) return;
    const size_t p = base + (size_t)k * 256 + tid;
    const bool root = p < plane && L[p] == (int)p;
    const unsigned long long m = __ballot(root);
    if (lane == 0) wtot[k & 1][wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int t = wtot[k & 1][w]; total += t; if (w < wave) before += t; }
#if DMM_CC_MUTATE == 6
    const int slot = root ? atomicAdd(&a.seg[(size_t)blockIdx.y * a.nseg], 1) : 0;   // (the first segment's offset is 0)
#else
    const int slot = running + before + __popcll(m & ((1ull << lane) - 1ull));
#endif
    if (root && slot < a.cap) {
      i32x2* r = (i32x2*)(rec + slot);   // (records are 8-byte aligned)
      const i32x2 w0 = {(int)p, INT_MAX}, w1 = {INT_MAX, -1}, w2 = {-1, 0}, w3 = {0, 0};
      r[0] = w0; r[1] = w1; r[2] = w2; r[3] = w3;
    }
    running += total;
  }
}

// the slot of `root` among the `kept` records of its plane (ascending roots), -1 where the cap has cut it off
__device__ __forceinline__ int find_slot(const dmm_component* rec, int kept, int root) {
  int lo = 0, hi = kept;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rec[mid].root < root) lo = mid + 1; else hi = mid;
  }
  return lo < kept && rec[lo].root == root ? lo : -1;
}

struct Stat { int root, x0, x1, y0, y1, area; unsigned long long key; };

__device__ __forceinline__ void stat_to_global(dmm_component* rec, int kept, const Stat& s) {
  const int slot = find_slot(rec, kept, s.root);
  if (slot < 0) return;
  dmm_component* r = rec + slot;
  atomicMin(&r->x0, s.x0);
  atomicMin(&r->y0, s.y0);
  atomicMax(&r->x1, s.x1);
  atomicMax(&r->y1, s.y1);
  atomicAdd(&r->area, s.area);
  atomicMax((unsigned long long*)&r->score, s.key);   // (offset 24 of a 32-byte record that is 8-byte aligned)
}

// value bits in an order that integers share: negative values reversed below the positive ones (-0.0 below +0.0; no NaN gets here)
__device__ __forceinline__ unsigned ordered_bits(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (f) one workgroup per tile, the pixels on the threads as in (a).  A thread first folds its own four pixels by root; the workgroup
// then folds by root in a small LDS table (open addressing, the key claimed with atomicCAS) and sends ONE update per root and tile to
// the record.  Without the table every thread of a large component meets on the same six global addresses: measured at C2's shape
// with i.i.d. noise (one component of a million pixels per plane) this launch alone took 100 ms.  A root that finds the table full
// goes to the record directly.  A tile without foreground leaves before it reads the map.
constexpr int CC_TABLE = 128;
__global__ __launch_bounds__(256) void cc_stats_kernel(ComponentsArgs a) {
  __shared__ int t_root[CC_TABLE], t_x0[CC_TABLE], t_y0[CC_TABLE], t_x1[CC_TABLE], t_y1[CC_TABLE], t_area[CC_TABLE];
  __shared__ unsigned long long t_key[CC_TABLE];
  const int tid = threadIdx.x;
  const int kept = min(a.counts[blockIdx.y], a.cap);
  if (kept == 0) return;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const size_t plane = (size_t)a.H * a.W;
  const float* xs = a.maps + (size_t)blockIdx.y * plane;
  const int* L = a.labels + (size_t)blockIdx.y * plane;
  dmm_component* rec = a.records + (size_t)blockIdx.y * a.cap;
  const int ly = tid >> 3, lx0 = (tid & 7) * 4;
  const int gy = ty * TH + ly, gx0 = tx * TW + lx0;
  int l[4] = {-1, -1, -1, -1};
  if (gy < a.H && gx0 < a.W) {
    const int* row = L + (size_t)gy * a.W + gx0;
    if ((a.W & 3) == 0 && (((uintptr_t)L) & 15) == 0) {
      const i32x4 q = *(const i32x4*)row;
#pragma unroll
      for (int j = 0; j < 4; ++j) l[j] = q[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (gx0 + j < a.W) l[j] = row[j];
    }
  }
  const bool any = (l[0] & l[1] & l[2] & l[3]) >= 0;   // (a label is -1 or >= 0: the sign bit survives the AND only if all four are -1)
  if (tid < CC_TABLE) { t_root[tid] = -1; t_x0[tid] = INT_MAX; t_y0[tid] = INT_MAX; t_x1[tid] = -1; t_y1[tid] = -1; t_area[tid] = 0; t_key[tid] = 0ull; }
  if (!__syncthreads_or(any)) return;   // no foreground in this tile (and the barrier behind the table's initialisation)
  if (any) {
    float v[4];
    bool in[4];
    load_quad(xs, a.H, a.W, gy, gx0, v, in);
    Stat s;
    s.root = -1;
    auto flush = [&]() {
      if (s.root < 0) return;
      unsigned h = ((unsigned)s.root * 2654435761u) >> 25;   // 7 bits: CC_TABLE == 128
      for (int probe = 0; probe < CC_TABLE; ++probe, h = (h + 1) & (CC_TABLE - 1)) {
        const int cur = atomicCAS(&t_root[h], -1, s.root);
        if (cur != -1 && cur != s.root) continue;
        atomicMin(&t_x0[h], s.x0); atomicMax(&t_x1[h], s.x1); atomicMin(&t_y0[h], s.y0); atomicMax(&t_y1[h], s.y1);
        atomicAdd(&t_area[h], s.area); atomicMax(&t_key[h], s.key);
        return;
      }
      stat_to_global(rec, kept, s);   // the table is full
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (l[j] < 0) continue;
      const int p = gy * a.W + gx0 + j;
#if DMM_CC_MUTATE == 5
      const unsigned long long key = ((unsigned long long)ordered_bits(v[j]) << 32) | (unsigned)p;
#else
      const unsigned long long key = ((unsigned long long)ordered_bits(v[j]) << 32) | (unsigned)~p;
#endif
      if (l[j] != s.root) {
        flush();
        s.root = l[j]; s.x0 = gx0 + j; s.y0 = s.y1 = gy; s.area = 0; s.key = 0ull;
      }
      s.x1 = gx0 + j;
      s.area += 1;
      s.key = key > s.key ? key : s.key;
    }
    flush();
  }
  __syncthreads();
  if (tid < CC_TABLE && t_root[tid] >= 0) {
    Stat t;
    t.root = t_root[tid]; t.x0 = t_x0[tid]; t.x1 = t_x1[tid]; t.y0 = t_y0[tid]; t.y1 = t_y1[tid]; t.area = t_area[tid]; t.key = t_key[tid];
    stat_to_global(rec, kept, t);
  }
}

// (g) one thread per slot: a kept record's 64-bit word becomes score and peak, every other slot becomes zero
__global__ __launch_bounds__(256) void cc_finish_kernel(ComponentsArgs a) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= a.cap) return;
  const int kept = min(a.counts[blockIdx.y], a.cap);
  i32x2* r = (i32x2*)(a.records + (size_t)blockIdx.y * a.cap + slot);
  if (slot < kept) {
    const i32x2 w = r[3];   // little-endian: w[0] = ~index (or, mutated, index), w[1] = ordered value bits
    const unsigned o = (unsigned)w[1];
    const unsigned bits = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
#if DMM_CC_MUTATE == 5
    const i32x2 out = {(int)bits, w[0]};
#else
    const i32x2 out = {(int)bits, ~w[0]};
#endif
    r[3] = out;
  } else {
    const i32x2 z = {0, 0};
    r[0] = z; r[1] = z; r[2] = z; r[3] = z;
  }
}

}  // namespace

ComponentsLayout components_layout(int planes, size_t plane) {
  const size_t nseg = (plane + CC_SEG - 1) / CC_SEG;
  ComponentsLayout l;
  l.labels = 0;
  l.seg = ((size_t)planes * plane * 4 + 15) / 16 * 16;
  l.total = l.seg + ((size_t)planes * nseg * 4 + 15) / 16 * 16;
  return l;
}

void components_grids(const ComponentsArgs& a, unsigned gx[CC_LAUNCHES]) {
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
  gx[0] = tiles; gx[1] = tiles; gx[2] = (unsigned)a.nseg; gx[3] = 1u; gx[4] = (unsigned)a.nseg; gx[5] = tiles;
  gx[6] = (unsigned)((a.cap + 255) / 256);
}

hipError_t launch_components(const ComponentsArgs& a, hipStream_t st) {
  unsigned gx[CC_LAUNCHES];
  components_grids(a, gx);
  const unsigned planes = (unsigned)(a.B * a.NC);
  // (a lab build, DMM_LAB=1: DMM_CC_LAUNCHES=k stops behind the first k launches - tools/components_cost.py times the prefixes and
  // reports each launch as a difference; the outputs of a cut call are not meaningful)
  const int n = lab_int("DMM_CC_LAUNCHES", CC_LAUNCHES);
  if (n > 0) hipLaunchKernelGGL(cc_local_kernel, dim3(gx[0], planes), dim3(256), 0, st, a);
  if (n > 1) hipLaunchKernelGGL(cc_merge_kernel, dim3(gx[1], planes), dim3(128), 0, st, a);
  if (n > 2) hipLaunchKernelGGL(cc_flatten_kernel, dim3(gx[2], planes), dim3(256), 0, st, a);
  if (n > 3) hipLaunchKernelGGL(cc_scan_kernel, dim3(gx[3], planes), dim3(256), 0, st, a);
  if (n > 4) hipLaunchKernelGGL(cc_slots_kernel, dim3(gx[4], planes), dim3(256), 0, st, a);
  if (n > 5) hipLaunchKernelGGL(cc_stats_kernel, dim3(gx[5], planes), dim3(256), 0, st, a);
  if (n > 6) hipLaunchKernelGGL(cc_finish_kernel, dim3(gx[6], planes), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmm
