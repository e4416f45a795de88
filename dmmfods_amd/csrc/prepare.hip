// Raw frames to training tensors on the device: the uint8 camera image, the projected LiDAR points and the labelled boxes of
// a batch become the fp32 planes the model and the loss read.  Three independent entry points (capi.cpp), plain launches on the
// caller's stream.  Each dst is (B, channels, Ho, Wo) with samples `dst_stride` elements apart; p = pool, Ho = H / p, Wo = W / p.
//   image      out = fdiv_rn(float(S), float(p * p)),  S the exact integer sum of the p x p block of one channel.
//   LiDAR      owner[b][y][x] = the highest point index whose k x k window (the last row and column of the plane are never written)
//              covers the pixel: an integer atomicMax, which commutes exactly; then each output pixel gathers d through its owners,
//              codes it (two fp32 roundings, never fused) and takes the maximum of a 2p x p window, clamped at 0.
//   heat maps  a workgroup owns a 16 x 16 tile of output pixels; it culls its sample's boxes against the tile into LDS in list order,
//              256 list entries at a time, and every lane scans the culled list from the back: the last box of a class that covers a
//              full-resolution pixel gives its value; the output is the maximum over the p x p block.
// Every output element is written exactly once by exactly one lane; no floating-point atomics; all address arithmetic is 64-bit.
#include "common.h"
#include "pointwise.h"

namespace dmm {

namespace {

// ------------------------------------------------------------------------------------------------ image
// grid: x = 256 output pixels of a plane, y = channel, z = sample of the launch
__global__ __launch_bounds__(256) void prep_image_kernel(PrepImageArgs a) {
  const unsigned o = blockIdx.x * 256u + threadIdx.x;          // < Ho * Wo + 256 <= 2^31 + 255
  if (o >= (unsigned)a.Ho * (unsigned)a.Wo) return;
  const int i = (int)(o / (unsigned)a.Wo), j = (int)(o - (unsigned)i * (unsigned)a.Wo);
  const int c = blockIdx.y;
  const size_t b = (size_t)(a.b0 + (int)blockIdx.z);
  const unsigned char* S = a.src + b * (size_t)a.src_stride;
  const size_t row = (size_t)a.W * (size_t)a.C;
  unsigned long long sum = 0;
  for (int dy = 0; dy < a.p; ++dy) {
    const unsigned char* q = S + (size_t)(i * (long long)a.p + dy) * row + (size_t)((long long)j * a.p) * (size_t)a.C + (size_t)c;
    for (int dx = 0; dx < a.p; ++dx) sum += q[(size_t)dx * (size_t)a.C];
  }
  const float den = (float)((long long)a.p * (long long)a.p);
  a.dst[b * (size_t)a.dst_stride + (size_t)c * ((size_t)a.Ho * (size_t)a.Wo) + o] = __fdiv_rn((float)sum, den);
}

// ------------------------------------------------------------------------------------------------ LiDAR
// the sample (within the launch) of global point index g: off[s] <= g < off[s + 1]
__device__ __forceinline__ int prep_sample_of(const int* off, int n, int g) {
  int lo = 0, hi = n;                     // invariant: off[lo] <= g < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// grid: x = 256 (point, window pixel) pairs of the launch's points
__global__ __launch_bounds__(256) void prep_lidar_splat_kernel(PrepLidarArgs a) {
  const int kk = a.k * a.k;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;          // < points * 225 + 256 < 2^31
  const unsigned npts = (unsigned)(a.off[a.nb] - a.off[0]);
  const unsigned pt = t / (unsigned)kk;
  if (pt >= npts) return;
  const int w = (int)(t - pt * (unsigned)kk);
  const int g = a.off[0] + (int)pt;
  const float x = a.points[(size_t)g * 3], y = a.points[(size_t)g * 3 + 1], d = a.points[(size_t)g * 3 + 2];
  // valid: finite and >= 0 (-0.0 is); a NaN fails the comparison
  if (!(x >= 0.f && y >= 0.f && d >= 0.f) || isinf(x) || isinf(y) || isinf(d)) return;
  const float big = 1073741824.f;         // 2^30: behind every plane, and the conversion stays defined
  const int cx = (int)fminf(x, big), cy = (int)fminf(y, big);
  const int s = (a.k - 1) >> 1;
  const long long row = (long long)cy - s + w / a.k, col = (long long)cx - s + w % a.k;
  if (row < 0 || col < 0 || row >= a.H - 1 || col >= a.W - 1) return;
  const size_t b = (size_t)(a.b0 + prep_sample_of(a.off, a.nb, g));
  atomicMax(a.owner + b * ((size_t)a.H * (size_t)a.W) + (size_t)row * (size_t)a.W + (size_t)col, g);
}

// (e * m) + c in two fp32 roundings: contraction off, as in augment.hip, so that no fma is formed
__device__ __forceinline__ float prep_lidar_code(const float* points, int owner) {
#pragma clang fp contract(off)
  float e = 76.f;
  if (owner >= 0) e = fminf(points[(size_t)owner * 3 + 2], 75.f);
  const float near = e * -6.2f, far = e * -2.f;
  return e <= 25.f ? near + 255.f : far + 150.f;
}

// grid: x = 256 output pixels of a plane, y = sample of the launch
__global__ __launch_bounds__(256) void prep_lidar_pool_kernel(PrepLidarArgs a) {
  const unsigned o = blockIdx.x * 256u + threadIdx.x;
  if (o >= (unsigned)a.Ho * (unsigned)a.Wo) return;
  const int i = (int)(o / (unsigned)a.Wo), j = (int)(o - (unsigned)i * (unsigned)a.Wo);
  const size_t b = (size_t)(a.b0 + (int)blockIdx.y);
  const int* own = a.owner + b * ((size_t)a.H * (size_t)a.W);
  float m = 0.f;                          // (the clamp of negatives)
  if (a.p == 1) {
    m = fmaxf(m, prep_lidar_code(a.points, own[o]));
  } else {
    const int r = min(i, a.Ho - 2);       // the last output row repeats the one above it
    const size_t y0 = (size_t)r * (size_t)a.p, x0 = (size_t)j * (size_t)a.p;
    for (int dy = 0; dy < 2 * a.p; ++dy)
      for (int dx = 0; dx < a.p; ++dx) m = fmaxf(m, prep_lidar_code(a.points, own[(y0 + dy) * (size_t)a.W + x0 + dx]));
  }
  a.dst[b * (size_t)a.dst_stride + o] = m;
}

// ------------------------------------------------------------------------------------------------ heat maps
struct CulledBox { int cls, x, y, w, h; };

// the value box q gives the full-resolution pixel (Y, X) it covers
__device__ __forceinline__ float prep_box_value(const CulledBox& q, long long Y, long long X) {
  if (q.cls != 1) return 1.f;
  const int r = (int)(Y - q.y), c = (int)(X - q.x);
  const int hf = q.h / 5, wf = q.w / 4;
  const bool side = c < wf || c >= 3 * wf;
  if (r < hf && side) return 0.3f;
  if (r >= 3 * hf) return side ? 0.5f : 0.75f;
  return 1.f;
}

// grid: x = tiles of PREP_TILE x PREP_TILE output pixels of a sample, y = sample of the launch
__global__ __launch_bounds__(256) void prep_heat_kernel(PrepHeatArgs a) {
  __shared__ CulledBox list[PREP_BOX_CHUNK];
  __shared__ int wave_count[4];
  const int tiles_x = (a.Wo + PREP_TILE - 1) / PREP_TILE;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int i = ty * PREP_TILE + (int)threadIdx.x / PREP_TILE, j = tx * PREP_TILE + (int)threadIdx.x % PREP_TILE;
  const bool live = i < a.Ho && j < a.Wo;
  const int first = a.off[blockIdx.y], count = a.off[blockIdx.y + 1] - first;
  const int nchunk = (count + PREP_BOX_CHUNK - 1) / PREP_BOX_CHUNK;
  // the tile's full-resolution pixels, inside the image
  const long long TY0 = (long long)ty * PREP_TILE * a.p, TX0 = (long long)tx * PREP_TILE * a.p;
  const long long TY1 = min(TY0 + (long long)PREP_TILE * a.p, (long long)a.H), TX1 = min(TX0 + (long long)PREP_TILE * a.p, (long long)a.W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int culled = 0;

  // boxes [first + ch * CHUNK, ...) that touch the tile, into `list` in list order; returns how many
  auto cull = [&](int ch) {
    const int n = min(PREP_BOX_CHUNK, count - ch * PREP_BOX_CHUNK);
    CulledBox q = {-1, 0, 0, 0, 0};
    bool keep = false;
    if ((int)threadIdx.x < n) {
      const dmm_prep_box bx = a.boxes[(size_t)first + (size_t)ch * PREP_BOX_CHUNK + threadIdx.x];
      q.cls = bx.type == 1 ? 0 : (bx.type == 2 ? 1 : (bx.type == 4 ? 2 : -1));
      q.x = bx.x; q.y = bx.y; q.w = bx.width; q.h = bx.height;
      keep = q.cls >= 0 && q.w > 0 && q.h > 0 && (long long)q.x < TX1 && (long long)q.x + q.w > TX0 && (long long)q.y < TY1 &&
             (long long)q.y + q.h > TY0;
    }
    const unsigned long long mask = __ballot(keep);
    __syncthreads();                      // every lane is done with the list of the chunk before
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 4; ++w) { if (w < wave) base += wave_count[w]; total += wave_count[w]; }
    if (keep) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = q;
    __syncthreads();
    return total;
  };

  if (nchunk == 1) culled = cull(0);
  float best[3] = {0.f, 0.f, 0.f};
  // every lane of the workgroup walks the same (dy, dx) of its own block at the same time, so a list of more than one chunk can be
  // culled again per pixel and scanned from its last chunk to its first
  for (int dy = 0; dy < a.p && nchunk > 0; ++dy)
    for (int dx = 0; dx < a.p; ++dx) {
      const long long Y = (long long)i * a.p + dy, X = (long long)j * a.p + dx;
      unsigned found = live ? 0u : 7u;
      for (int ch = nchunk - 1; ch >= 0; --ch) {
        if (nchunk > 1) {
          if (__syncthreads_count(found != 7u) == 0) break;
          culled = cull(ch);
        }
        for (int n = culled - 1; n >= 0 && found != 7u; --n) {
          const CulledBox q = list[n];
          if ((found >> q.cls) & 1u) continue;
          if (X < q.x || X >= (long long)q.x + q.w || Y < q.y || Y >= (long long)q.y + q.h) continue;
          found |= 1u << q.cls;
          best[q.cls] = fmaxf(best[q.cls], prep_box_value(q, Y, X));
        }
      }
    }
  if (!live) return;
  const size_t plane = (size_t)a.Ho * (size_t)a.Wo;
  float* D = a.dst + (size_t)(a.b0 + (int)blockIdx.y) * (size_t)a.dst_stride + (size_t)i * (size_t)a.Wo + (size_t)j;
  D[0] = best[0]; D[plane] = best[1]; D[2 * plane] = best[2];
}

unsigned ceil256(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

unsigned prep_plane_grid_x(int Ho, int Wo) { return ceil256((size_t)Ho * (size_t)Wo); }
unsigned prep_splat_grid_x(int npoints, int k) { return ceil256((size_t)npoints * (size_t)(k * k)); }
unsigned prep_heat_grid_x(int Ho, int Wo) { return (unsigned)((Ho + PREP_TILE - 1) / PREP_TILE) * (unsigned)((Wo + PREP_TILE - 1) / PREP_TILE); }

hipError_t launch_prep_image(const PrepImageArgs& a, int nsamples, hipStream_t st) {
  hipLaunchKernelGGL(prep_image_kernel, dim3(prep_plane_grid_x(a.Ho, a.Wo), a.C, nsamples), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_prep_lidar(const PrepLidarArgs& a, hipStream_t st) {
  const int npoints = a.off[a.nb] - a.off[0];
  if (npoints > 0) {
    hipLaunchKernelGGL(prep_lidar_splat_kernel, dim3(prep_splat_grid_x(npoints, a.k)), dim3(256), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(prep_lidar_pool_kernel, dim3(prep_plane_grid_x(a.Ho, a.Wo), a.nb), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_prep_heat(const PrepHeatArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(prep_heat_kernel, dim3(prep_heat_grid_x(a.Ho, a.Wo), a.nb), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmm
