// On-device batch augmentation: a per-sample window of every plane of a batch - cropped or shifted, optionally mirrored
// left-right, with a per-channel gain and bias - in one memory-bound launch.  For sample b, global channel c, output pixel (y, x):
//   sy = y0 + y;   sx = x0 + (flip ? Wo - 1 - x : x)
//   inside the source:   v = src[b][c][sy][sx];   out = v, bit for bit, where gain == 1 and bias == 0, else (gain * v) + bias
//   outside:             out = fill[c]
// Grid: x = 256-lane groups of a plane's quads, y = global channel, z = sample within the launch, so the sample's window, the
// channel's gain / bias (and with them the identity test) and every pointer are uniform over a workgroup and live in scalar registers.
// A lane owns one QUAD: four consecutive output pixels of one row (the last quad of a row is short when Wo is no multiple of 4).
//   * Quad wholly inside the source: its four source pixels are consecutive in memory, but start wherever x0, the row pitch and the
//     tensor's base put them.  They are read with NATURALLY ALIGNED 16-byte loads - the one that holds them, or the two that cover
//     them, four of whose eight words are picked by the misalignment; a mirrored window is the same span reversed in registers.
//     Both loads stay inside the sample's plane: the quad whose covering span would leave it takes the element path.
//   * Everything else (a row outside, a quad that touches the source's edge, a short quad): element by element, with the fill.
//   * The quad is stored as 16 bytes where its address is 16-byte aligned, else element by element.
// Every output element is written exactly once by exactly one lane; nothing is accumulated, no atomics.
#include "common.h"
#include "pointwise.h"

namespace dmm {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// (gain * v) + bias on the bits of v: two fp32 roundings, contraction off as in guard.hip, so that no fma is formed
__device__ __forceinline__ unsigned aug_affine(unsigned bits, float gain, float bias) {
#pragma clang fp contract(off)
  const float p = gain * __uint_as_float(bits);
  return __float_as_uint(p + bias);
}

template <bool NT>
__global__ __launch_bounds__(256) void augment_kernel(AugArgs a) {
  const int c = blockIdx.y;
  const unsigned qw = ((unsigned)a.Wo + 3u) >> 2;            // quads per output row
  const unsigned q = blockIdx.x * 256u + threadIdx.x;        // < Ho * qw + 256 <= 2^31 + 255
  const unsigned y = q / qw;
  if (y >= (unsigned)a.Ho) return;
  const int x = (int)(q - y * qw) * 4;
  const int n = min(4, a.Wo - x);
  const size_t b = (size_t)(a.b0 + (int)blockIdx.z);
  const float* P = a.ch[c].src + b * (size_t)a.ch[c].src_stride;   // the sample's source plane
  float* D = a.ch[c].dst + b * (size_t)a.ch[c].dst_stride + ((size_t)y * (size_t)a.Wo + (size_t)x);
  const int y0 = a.s[blockIdx.z].y0, x0 = a.s[blockIdx.z].x0;
  const bool flip = a.s[blockIdx.z].flip != 0;
  const float gain = a.s[blockIdx.z].gain[c], bias = a.s[blockIdx.z].bias[c];
  const bool ident = gain == 1.f && bias == 0.f;
  const unsigned fill = __float_as_uint(a.fill[c]);
  const long long sy = (long long)y0 + (long long)y;
  const bool row_in = sy >= 0 && sy < a.Hs;
  // the source column of the quad's lowest address: its first pixel, or mirrored its last
  const long long sl = (long long)x0 + (flip ? a.Wo - 4 - x : x);
  unsigned r[4] = {fill, fill, fill, fill};
  bool fast = row_in && n == 4 && sl >= 0 && sl + 4 <= a.Ws;
  if (fast) {
    const long long e = sy * a.Ws + sl;                      // plane-relative index of that pixel
    const int m = (int)((((uintptr_t)P >> 2) + (unsigned long long)e) & 3ull);   // words behind a 16-byte boundary
    const long long e0 = e - m;
    if (m == 0) {
      const u32x4 w = *(const u32x4*)(P + e0);
      r[0] = w[0]; r[1] = w[1]; r[2] = w[2]; r[3] = w[3];
    } else if (e0 >= 0 && e0 + 8 <= (long long)a.Hs * a.Ws) {
      const u32x4 w0 = *(const u32x4*)(P + e0), w1 = *(const u32x4*)(P + e0 + 4);
      const unsigned w[7] = {w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = m == 1 ? w[j] : (m == 2 ? w[j + 1] : w[j + 2]);
    } else {
      fast = false;
    }
  }
  if (fast) {
    if (flip) {
      const unsigned t0 = r[0], t1 = r[1];
      r[0] = r[3]; r[1] = r[2]; r[2] = t1; r[3] = t0;
    }
    if (!ident) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = aug_affine(r[j], gain, bias);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long sx = (long long)x0 + (flip ? a.Wo - 1 - (x + j) : x + j);
      if (j < n && row_in && sx >= 0 && sx < a.Ws) {
        const unsigned v = __float_as_uint(P[sy * a.Ws + sx]);
        r[j] = ident ? v : aug_affine(v, gain, bias);
      }
    }
  }
  if (n == 4 && ((uintptr_t)D & 15) == 0) {
    const u32x4 v = {r[0], r[1], r[2], r[3]};
    if (NT) __builtin_nontemporal_store(v, (u32x4*)D);
    else *(u32x4*)D = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) ((unsigned*)D)[j] = r[j];
  }
}

}  // namespace

unsigned augment_grid_x(int Ho, int Wo) {
  const size_t quads = (size_t)Ho * (size_t)((Wo + 3) / 4);
  return (unsigned)((quads + 255) / 256);
}

hipError_t launch_augment(const AugArgs& a, int nchannels, int nsamples, hipStream_t st) {
  const dim3 grid(augment_grid_x(a.Ho, a.Wo), nchannels, nsamples);
  // The outputs are read back only by the model's pack kernels, one launch later and from every XCD: the 16-byte stores carry the
  // non-temporal hint the EMA arena's stores carry (guard.hip).  Measured at C2's shapes (profiles/r14/augment_cost.txt): 96.7 us
  // against 99.1 with plain stores for the identity window, 98.9 against 104.8 for a shifted one - and 104.2 for torch's copy of
  // the same bytes.  (a lab build: DMM_AUG_NT=0 is the kernel with plain stores - what tools/augment_cost.py compares against)
  static const int nt = lab_int("DMM_AUG_NT", 1);
  if (nt) hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmm
