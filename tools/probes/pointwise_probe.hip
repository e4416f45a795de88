// Per-kernel parity of the helper kernels in dmmfods_amd/csrc/pointwise.hip, through the launchers of the BUILT libdmmfods_hip.so
// (no device code of its own: the binary that ships is the binary under test; pointwise.h keeps the argument blocks in step).
//   pointwise_probe <group>      group = convert | bn | pool | poolbwd | corr | loss
// prints one "name: ok" / "name: FAIL ..." line per case (first differing index, both values) and exits non-zero on any FAIL.
// A HIP error ends the program at once (exit code 3): nothing further is launched.
// build: hipcc -O2 -std=c++17 --offload-arch=gfx950 -I dmmfods_amd/csrc tools/probes/pointwise_probe.hip -o build_var/pointwise_probe
//        -L dmmfods_amd -ldmmfods_hip -Wl,-rpath,$PWD/dmmfods_amd -pthread
//
// The references are plain loops in double over (b, y, x, c), window by window.  Wherever the operation allows it the inputs come from
// small dyadic grids, so that every fp32 intermediate of a kernel is exactly representable: stored outputs must then equal the
// round-to-nearest-even conversion of the exact value bit for bit (zeros of either sign are the same value), argmax bytes must be equal
// and fp64 sums must be exactly equal (sums of bounded dyadics do not depend on the order).  Each such case also computes its
// intermediates in float and asserts they agree with double: a case that fails THAT is a bug of the probe, not a tolerance to widen.
// Every output buffer sits between two 256-byte canary regions; strided destinations also keep their foreign channels.
#include <hip/hip_runtime.h>
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "pointwise.h"
using namespace dmm;

// ---------------------------------------------------------------------------------------------------- plumbing
static int g_failed = 0;
static const char* DTN[3] = {"f32", "f16", "bf16"};

#define HIPOK(e)                                                                                  \
  do {                                                                                            \
    hipError_t rc_ = (e);                                                                         \
    if (rc_ != hipSuccess) {                                                                      \
      printf("%s: FAIL HIP error %s (line %d)\n", #e, hipGetErrorString(rc_), __LINE__);         \
      fflush(stdout);                                                                             \
      _exit(3);                                                                                   \
    }                                                                                             \
  } while (0)

// after every launch: the launcher's result, the last error and the synchronise result; any error ends the program
static void ran(hipError_t rc, const char* what) {
  const hipError_t e1 = hipGetLastError(), e2 = hipDeviceSynchronize();
  if (rc != hipSuccess || e1 != hipSuccess || e2 != hipSuccess) {
    printf("%s: FAIL HIP error (launch %s, last %s, sync %s)\n", what, hipGetErrorString(rc), hipGetErrorString(e1), hipGetErrorString(e2));
    fflush(stdout);
    _exit(3);
  }
}

struct Case {
  std::string name;
  bool bad = false;
  char msg[400];
  Case(const char* fmt, ...) {
    char b[200];
    va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof(b), fmt, ap); va_end(ap);
    name = b; msg[0] = 0;
  }
  void fail(const char* fmt, ...) {   // keeps the first failure
    if (bad) return;
    bad = true;
    va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof(msg), fmt, ap); va_end(ap);
  }
  void done() {
    if (bad) { printf("%s: FAIL %s\n", name.c_str(), msg); ++g_failed; }
    else printf("%s: ok\n", name.c_str());
    fflush(stdout);
  }
};

static int n_threads() { return (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }
// f(lo, hi, thread) over [0, n) in contiguous chunks on up to 16 host threads
static void par_for(size_t n, const std::function<void(size_t, size_t, int)>& f, size_t min_chunk = 1 << 16) {
  int nt = (int)std::min<size_t>(n_threads(), std::max<size_t>(1, n / min_chunk));
  if (nt <= 1) { f(0, n, 0); return; }
  std::vector<std::thread> th;
  const size_t per = (n + nt - 1) / nt;
  for (int t = 0; t < nt; ++t) th.emplace_back([=, &f] { const size_t lo = t * per, hi = std::min(n, lo + per); if (lo < hi) f(lo, hi, t); });
  for (auto& t : th) t.join();
}

static inline uint64_t mix(uint64_t seed, uint64_t i) {   // splitmix64 of (seed, i)
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + i * 0xD1B54A32D192ED03ull + 0x632BE59BD9B4E019ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline double unif(uint64_t seed, uint64_t i) { return (double)(mix(seed, i) >> 11) * (1.0 / 9007199254740992.0); }
// k * step with k uniform in [-kmax, kmax]
static inline float dyad(uint64_t seed, uint64_t i, int kmax, float step) { return (float)((int)(mix(seed, i) % (uint64_t)(2 * kmax + 1)) - kmax) * step; }
template <class T, size_t N> static inline T pick(uint64_t seed, uint64_t i, const T (&tab)[N]) { return tab[mix(seed, i) % N]; }

// ---- storage types: round-to-nearest-even conversions written out on the bits
static uint16_t f2h(float f) {
  uint32_t x; memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000);
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return sign | 0x7e00;
  if (x >= 0x477ff000u) return sign | 0x7c00;   // >= 65520 rounds to infinity
  if (x < 0x38800000u) {                        // below 2^-14: a multiple of 2^-24
    float a; memcpy(&a, &x, 4);
    return sign | (uint16_t)std::nearbyint((double)a * 16777216.0);
  }
  uint32_t h = (((x >> 23) - 112) << 10) | ((x & 0x7fffffu) >> 13);
  const uint32_t rem = x & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) ++h;
  return sign | (uint16_t)h;
}
static float h2f(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 0x3ff;
  float r = e == 0 ? std::ldexp((float)m, -24) : e == 31 ? (m ? NAN : INFINITY) : std::ldexp((float)(m | 0x400), e - 25);
  return (h & 0x8000) ? -r : r;
}
static uint16_t f2b(float f) {
  uint32_t x; memcpy(&x, &f, 4);
  if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40);
  x += 0x7fffu + ((x >> 16) & 1);
  return (uint16_t)(x >> 16);
}
static float b2f(uint16_t b) { uint32_t x = (uint32_t)b << 16; float f; memcpy(&f, &x, 4); return f; }

static inline size_t esz(int dt) { return dt == DT_F32 ? 4 : 2; }
static inline int slot_of(int dt) { return dt == DT_F32 ? 4 : 8; }
static inline uint32_t enc(int dt, float v) {
  if (dt == DT_F32) { uint32_t x; memcpy(&x, &v, 4); return x; }
  return dt == DT_F16 ? f2h(v) : f2b(v);
}
static inline float dec(int dt, uint32_t b) {
  if (dt == DT_F32) { float f; memcpy(&f, &b, 4); return f; }
  return dt == DT_F16 ? h2f((uint16_t)b) : b2f((uint16_t)b);
}
static inline float rnd_to(int dt, float v) { return dec(dt, enc(dt, v)); }
static inline uint32_t get_bits(int dt, const void* buf, size_t i) { return dt == DT_F32 ? ((const uint32_t*)buf)[i] : ((const uint16_t*)buf)[i]; }
static inline void put_bits(int dt, void* buf, size_t i, uint32_t b) { if (dt == DT_F32) ((uint32_t*)buf)[i] = b; else ((uint16_t*)buf)[i] = (uint16_t)b; }
static inline bool same_value(int dt, uint32_t a, uint32_t b) {
  if (a == b) return true;
  const uint32_t m = dt == DT_F32 ? 0x7fffffffu : 0x7fffu;
  return (a & m) == 0 && (b & m) == 0;
}
// half an ulp of the storage type at |v| (normal range)
static inline double half_ulp(int dt, double v) {
  const int mant = dt == DT_F32 ? 24 : dt == DT_F16 ? 11 : 8;
  int e; std::frexp(std::fabs(v), &e);
  if (dt == DT_F16 && e < -13) e = -13;
  return std::ldexp(1.0, e - mant - 1);
}
static std::vector<uint8_t> pack(int dt, const std::vector<float>& v) {
  std::vector<uint8_t> o(v.size() * esz(dt));
  par_for(v.size(), [&](size_t lo, size_t hi, int) { for (size_t i = lo; i < hi; ++i) put_bits(dt, o.data(), i, enc(dt, v[i])); });
  return o;
}

// ---- device buffers
struct Dev {   // an input
  void* p = nullptr;
  Dev() {}
  Dev(const void* src, size_t bytes) { set(src, bytes); }
  void set(const void* src, size_t bytes) { HIPOK(hipMalloc(&p, std::max<size_t>(bytes, 16))); if (bytes) HIPOK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice)); }
  template <class T> Dev(const std::vector<T>& v) { set(v.data(), v.size() * sizeof(T)); }
  ~Dev() { if (p) (void)hipFree(p); }
  Dev(const Dev&) = delete;
  template <class T> T* as() const { return (T*)p; }
};
constexpr size_t CANARY = 256;
struct Out {   // an output between two canary regions
  uint8_t* raw = nullptr;
  size_t n = 0;
  Out(const void* init, size_t bytes) : n(bytes) {   // init == nullptr: the body starts as canary bytes too
    HIPOK(hipMalloc((void**)&raw, n + 2 * CANARY));
    HIPOK(hipMemset(raw, 0xC9, n + 2 * CANARY));
    if (init && n) HIPOK(hipMemcpy(raw + CANARY, init, n, hipMemcpyHostToDevice));
  }
  ~Out() { if (raw) (void)hipFree(raw); }
  Out(const Out&) = delete;
  template <class T> T* as() const { return (T*)(raw + CANARY); }
  // the body into dst; false (and a note on the case) when a canary byte changed
  bool fetch(void* dst, Case& c, const char* what) {
    uint8_t g[2 * CANARY];
    HIPOK(hipMemcpy(g, raw, CANARY, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(g + CANARY, raw + CANARY + n, CANARY, hipMemcpyDeviceToHost));
    if (n) HIPOK(hipMemcpy(dst, raw + CANARY, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < 2 * CANARY; ++i)
      if (g[i] != 0xC9) { c.fail("%s: canary byte %s%zu overwritten (0x%02x)", what, i < CANARY ? "-" : "+", i < CANARY ? CANARY - i : i - CANARY, g[i]); return false; }
    return true;
  }
};

// first index whose stored bits differ in VALUE from want(i); SIZE_MAX when none
static size_t first_diff(int dt, const void* got, size_t n, const std::function<uint32_t(size_t)>& want) {
  std::vector<size_t> bad(n_threads(), SIZE_MAX);
  par_for(n, [&](size_t lo, size_t hi, int t) {
    for (size_t i = lo; i < hi; ++i)
      if (!same_value(dt, get_bits(dt, got, i), want(i))) { bad[t] = i; return; }
  });
  return *std::min_element(bad.begin(), bad.end());
}
static void check_tensor(Case& c, const char* what, int dt, const void* got, size_t n, const std::function<uint32_t(size_t)>& want) {
  const size_t i = first_diff(dt, got, n, want);
  if (i != SIZE_MAX) c.fail("%s[%zu] got %.9g (0x%x) want %.9g (0x%x)", what, i, dec(dt, get_bits(dt, got, i)), get_bits(dt, got, i), dec(dt, want(i)), want(i));
}

// Replicated fp64 accumulators: `stride` doubles between the STAT_REPS replicas (0: one copy of C).  The slots start at zero, the gaps
// between replicas hold a sentinel that must survive; a consumer reads sum_k acc[c + k * stride].
constexpr double SENTINEL = 12345.0;
static std::vector<double> stat_init(int C, int stride) {
  if (!stride) return std::vector<double>(C, 0.0);
  std::vector<double> v((size_t)STAT_REPS * stride, SENTINEL);
  for (int k = 0; k < STAT_REPS; ++k) for (int c = 0; c < C; ++c) v[(size_t)k * stride + c] = 0.0;
  return v;
}
static void check_stats(Case& c, const char* what, const std::vector<double>& got, int C, int stride, const std::vector<double>& want) {
  for (int ch = 0; ch < C; ++ch) {
    double s = got[ch];
    if (stride) for (int k = 1; k < STAT_REPS; ++k) s += got[(size_t)k * stride + ch];
    if (s != want[ch]) { c.fail("%s[%d] got %.17g want %.17g", what, ch, s, want[ch]); return; }
  }
  if (stride)
    for (int k = 0; k < STAT_REPS; ++k) for (int g = C; g < stride; ++g)
      if (got[(size_t)k * stride + g] != SENTINEL) { c.fail("%s: gap double %d of replica %d overwritten (%.17g)", what, g, k, got[(size_t)k * stride + g]); return; }
}

// ---------------------------------------------------------------------------------------------------- convert
// kmax: the dyadic grid is k / 4, |k| <= kmax.  1024: 11 significant bits, representable in f16.  8191 (the rounding cases): 13
// significant bits - the store to f16 / bf16 is ONE round-to-nearest-even of an exactly known number, ties included; the reference is
// the fp64 product followed by the conversion written out above (f2h / f2b), and the case fails if the grid does not need it.
static void convert_case(int dt, const char* nm, int B, int H, int W, int C1, int C2, float scale, bool dyn, bool stats, bool dyadic, int kmax = 1024) {
  Case cs("convert %s %s B%d H%d W%d C1=%d C2=%d", DTN[dt], nm, B, H, W, C1, C2);
  const size_t plane = (size_t)H * W, npix = (size_t)B * plane;
  const float dynv = 8.f;   // a power of two: x * (scale * dyn) and (x * scale) * dyn are the same fp32 number
  std::vector<float> s1(npix * C1), s2(npix * C2);
  auto fill = [&](std::vector<float>& s, uint64_t seed) {
    par_for(s.size(), [&](size_t lo, size_t hi, int) {
      for (size_t i = lo; i < hi; ++i) s[i] = dyadic ? dyad(seed, i, kmax, 0.25f) : (float)(unif(seed, i) * 6.0 - 3.0);
    });
  };
  fill(s1, 11 + dt); fill(s2, 23 + dt);
  const float sc = dyn ? scale * dynv : scale;
  // reference: value of channel c of pixel p, in fp32 (one product) and - for the dyadic cases - in double as well
  bool exact = true;
  auto val = [&](size_t p, int c) -> float {
    const size_t b = p / plane, rem = p % plane;
    float x = 0.f;
    if (c < C1) x = s1[(b * C1 + c) * plane + rem];
    else if (c < C1 + C2) x = s2[(b * C2 + (c - C1)) * plane + rem];
    return x * sc;
  };
  std::vector<uint8_t> want(npix * 8 * esz(dt));
  const int nt = n_threads();
  std::vector<double> ps(nt * 8, 0.0), pq(nt * 8, 0.0), pa(nt * 8, 0.0), pb(nt * 8, 0.0);
  std::vector<int> inexact(nt, 0);
  std::vector<size_t> nround(nt, 0), ntie(nt, 0);
  par_for(npix, [&](size_t lo, size_t hi, int t) {
    for (size_t p = lo; p < hi; ++p)
      for (int c = 0; c < 8; ++c) {
        const float v = val(p, c);
        if (rnd_to(dt, v) != v) { ++nround[t]; if (std::fabs((double)rnd_to(dt, v) - (double)v) == half_ulp(dt, v)) ++ntie[t]; }
        if (dyadic) {
          const size_t b = p / plane, rem = p % plane;
          const double x = c < C1 ? s1[(b * C1 + c) * plane + rem] : c < C1 + C2 ? s2[(b * C2 + (c - C1)) * plane + rem] : 0.0;
          if (x * (double)scale * (dyn ? (double)dynv : 1.0) != (double)v) inexact[t] = 1;
        }
        const uint32_t bits = enc(dt, v);
        put_bits(dt, want.data(), p * 8 + c, bits);
        const double f = dec(dt, bits);
        ps[t * 8 + c] += f; pq[t * 8 + c] += f * f; pa[t * 8 + c] += std::fabs(f); pb[t * 8 + c] += f * f;
      }
  }, 1 << 14);
  for (int t = 0; t < nt; ++t) exact = exact && !inexact[t];
  if (!exact) cs.fail("probe bug: the fp32 product is not exact on this grid");
  if (kmax > 1024) {   // a rounding case: at least a quarter of the stores round, one in fifty is an exact tie
    size_t nr = 0, nti = 0;
    for (int t = 0; t < nt; ++t) { nr += nround[t]; nti += ntie[t]; }
    if (4 * nr < npix * (size_t)(C1 + C2) || 50 * nti < npix * (size_t)(C1 + C2)) cs.fail("probe bug: only %zu of %zu values round (%zu ties)", nr, npix * (C1 + C2), nti);
  }
  std::vector<double> rs(8, 0.0), rq(8, 0.0), ra(8, 0.0);
  for (int t = 0; t < nt; ++t) for (int c = 0; c < 8; ++c) { rs[c] += ps[t * 8 + c]; rq[c] += pq[t * 8 + c]; ra[c] += pa[t * 8 + c]; }

  Dev d1(s1), d2(s2), ddyn(&dynv, 4);
  Out dst(nullptr, want.size());
  std::vector<double> zero8(8, 0.0);
  Out ssum(zero8.data(), 64), ssq(zero8.data(), 64);
  ConvertArgs a;
  memset(&a, 0, sizeof(a));
  a.src1 = d1.as<float>(); a.src2 = C2 ? d2.as<float>() : nullptr; a.C1 = C1; a.C2 = C2;
  a.dst = dst.as<void>(); a.B = B; a.H = H; a.W = W;
  a.stat_sum = stats ? ssum.as<double>() : nullptr; a.stat_sq = stats ? ssq.as<double>() : nullptr;
  a.scale = scale; a.dyn_scale = dyn ? ddyn.as<float>() : nullptr;
  ran(launch_convert_input(a, dt, nullptr), cs.name.c_str());

  std::vector<uint8_t> got(want.size());
  if (dst.fetch(got.data(), cs, "dst")) check_tensor(cs, "dst", dt, got.data(), npix * 8, [&](size_t i) { return get_bits(dt, want.data(), i); });
  std::vector<double> gs(8), gq(8);
  const bool ok1 = ssum.fetch(gs.data(), cs, "stat_sum"), ok2 = ssq.fetch(gq.data(), cs, "stat_sq");
  if (ok1 && ok2) {
    for (int c = 0; c < 8; ++c) {
      const double ws = stats ? rs[c] : 0.0, wq = stats ? rq[c] : 0.0;   // null stats: the buffers beside must stay zero
      // dyadic: exact.  Otherwise two fp64 summation orders of the same n numbers: n * 2^-53 * sum |v|
      const double ts = dyadic || !stats ? 0.0 : (double)npix * std::ldexp(1.0, -53) * ra[c], tq = dyadic || !stats ? 0.0 : (double)npix * std::ldexp(1.0, -53) * rq[c];
      if (std::fabs(gs[c] - ws) > ts) cs.fail("stat_sum[%d] got %.17g want %.17g (tol %.3g)", c, gs[c], ws, ts);
      if (std::fabs(gq[c] - wq) > tq) cs.fail("stat_sq[%d] got %.17g want %.17g (tol %.3g)", c, gq[c], wq, tq);
    }
  }
  cs.done();
}

static void group_convert() {
  for (int dt = 0; dt < 3; ++dt) {
    convert_case(dt, "plain", 2, 3, 5, 3, 3, 1.f, false, true, true);
    convert_case(dt, "src2-null dyn", 2, 3, 5, 8, 0, 0.25f, true, true, true);
    convert_case(dt, "no-stats", 2, 3, 5, 1, 0, 1.f, false, false, true);
    convert_case(dt, "no-stats dyn", 2, 3, 5, 4, 4, 0.25f, true, false, true);
    convert_case(dt, "grid-stride", 3, 419, 835, 3, 3, 0.25f, true, true, true);   // 1 049 595 pixels > 4096 x 256 threads
    convert_case(dt, "non-dyadic", 2, 3, 5, 3, 2, 0.37f, true, true, false);
    if (dt != DT_F32) {   // 13 significant bits into 11 / 8
      convert_case(dt, "rounding", 2, 13, 17, 3, 3, 1.f, false, true, true, 8191);
      convert_case(dt, "rounding dyn", 2, 13, 17, 5, 3, 0.25f, true, true, true, 8191);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- bn finalize
static bool close_rel(double got, double want, double mag, double rel) { return std::fabs(got - want) <= rel * mag; }

static void bn_fwd_case(int C, int training, bool reps, int cu_mode) {
  Case cs("bn fwd C%d %s%s cu=%s", C, training ? "train" : "eval", reps ? " replicas" : "", cu_mode == 0 ? "count" : cu_mode == 1 ? "4count" : "1");
  const double count = 1000.0, cu = cu_mode == 0 ? count : cu_mode == 1 ? 4 * count : 1.0;
  const float momentum = 0.1f, eps = 1e-5f;
  const int stride = reps ? C + 5 : 0;
  std::vector<double> sum(stride ? (size_t)STAT_REPS * stride : C, 0.0), sq(sum.size(), 0.0), tsum(C), tsq(C);
  std::vector<float> gamma(C), beta(C), rm(C), rv(C);
  for (int c = 0; c < C; ++c) {
    double m = unif(1, c) * 4 - 2, v = 0.01 + unif(2, c) * 3.99;
    tsum[c] = count * m; tsq[c] = count * (v + m * m);
    if (c == 0) {   // a constant channel: sq / count - m^2 comes out slightly negative and is clamped
      m = 0.1; tsum[c] = count * m; tsq[c] = count * m * m * (1.0 - 4e-16);
    }
    gamma[c] = (float)(unif(3, c) * 3 - 1.5); beta[c] = (float)(unif(4, c) * 2 - 1);
    rm[c] = (float)(unif(5, c) * 2 - 1); rv[c] = (float)(0.05 + unif(6, c) * 2);
    if (!stride) { sum[c] = tsum[c]; sq[c] = tsq[c]; }
    else {   // eight shares of sixteenths
      static const int w[8] = {1, 3, 2, 4, 1, 2, 1, 2};
      for (int k = 0; k < STAT_REPS; ++k) { sum[(size_t)k * stride + c] = tsum[c] * w[k % 8] / 16.0 * (8.0 / STAT_REPS); sq[(size_t)k * stride + c] = tsq[c] * w[k % 8] / 16.0 * (8.0 / STAT_REPS); }
    }
  }
  if (training) {
    const double m0 = tsum[0] / count;
    if (!(tsq[0] / count - m0 * m0 < 0)) cs.fail("probe bug: the constant channel's raw variance is not negative");
  }
  Dev dsum(sum), dsq(sq), dg(gamma), db(beta);
  Out orm(rm.data(), C * 4), orv(rv.data(), C * 4), osc(nullptr, C * 4), osh(nullptr, C * 4), omean(nullptr, C * 4), oistd(nullptr, C * 4);
  BnFinalizeArgs a;
  memset(&a, 0, sizeof(a));
  a.sum = dsum.as<double>(); a.sq = dsq.as<double>(); a.stat_stride = stride; a.count = count; a.count_unbiased = cu;
  a.gamma = dg.as<float>(); a.beta = db.as<float>(); a.running_mean = orm.as<float>(); a.running_var = orv.as<float>();
  a.scale = osc.as<float>(); a.shift = osh.as<float>(); a.mean = omean.as<float>(); a.invstd = oistd.as<float>();
  a.C = C; a.training = training; a.momentum = momentum; a.eps = eps;
  ran(launch_bn_finalize(a, nullptr), cs.name.c_str());
  std::vector<float> grm(C), grv(C), gsc(C), gsh(C), gmean(C), gistd(C);
  bool ok = orm.fetch(grm.data(), cs, "running_mean");
  ok = orv.fetch(grv.data(), cs, "running_var") && ok;
  ok = osc.fetch(gsc.data(), cs, "scale") && ok;
  ok = osh.fetch(gsh.data(), cs, "shift") && ok;
  ok = omean.fetch(gmean.data(), cs, "mean") && ok;
  ok = oistd.fetch(gistd.data(), cs, "invstd") && ok;
  // BatchNorm2d in fp64.  Every output is at most three correctly rounded fp32 operations away from its fp64 inputs: 2^-21 relative
  // (the operation count with a 2x margin); sums of two terms relative to the terms' magnitudes (shift: |beta| + |mean * scale|)
  const double R = std::ldexp(1.0, -21);
  for (int c = 0; ok && c < C; ++c) {
    double mean, var, wrm = rm[c], wrv = rv[c], mrm = std::fabs(wrm), mrv = std::fabs(wrv);
    if (training) {
      long double su = 0, s2 = 0;
      if (!stride) { su = sum[c]; s2 = sq[c]; }
      else for (int k = 0; k < STAT_REPS; ++k) { su += sum[(size_t)k * stride + c]; s2 += sq[(size_t)k * stride + c]; }
      mean = (double)(su / count);
      var = (double)(s2 / count) - mean * mean;
      if (c == 0 || var < 0) var = 0;   // channel 0 is constant: its true variance is 0
      const double unb = cu > 1 ? var * cu / (cu - 1) : var, mo = momentum;
      wrm = (1 - mo) * rm[c] + mo * mean; mrm = std::fabs((1 - mo) * rm[c]) + std::fabs(mo * mean);
      wrv = (1 - mo) * rv[c] + mo * unb; mrv = std::fabs(wrv);
    } else { mean = rm[c]; var = rv[c]; }
    const double istd = 1.0 / std::sqrt(var + (double)eps), s = gamma[c] * istd, sh = beta[c] - mean * s;
    if (!close_rel(gmean[c], mean, std::fabs(mean), R)) cs.fail("mean[%d] got %.9g want %.17g", c, gmean[c], mean);
    if (!close_rel(gistd[c], istd, istd, R)) cs.fail("invstd[%d] got %.9g want %.17g", c, gistd[c], istd);
    if (!close_rel(gsc[c], s, std::fabs(s), R)) cs.fail("scale[%d] got %.9g want %.17g", c, gsc[c], s);
    if (!close_rel(gsh[c], sh, std::fabs((double)beta[c]) + std::fabs(mean * s), R)) cs.fail("shift[%d] got %.9g want %.17g", c, gsh[c], sh);
    if (training) {
      if (!close_rel(grm[c], wrm, mrm, R)) cs.fail("running_mean[%d] got %.9g want %.17g", c, grm[c], wrm);
      if (!close_rel(grv[c], wrv, mrv, R)) cs.fail("running_var[%d] got %.9g want %.17g", c, grv[c], wrv);
    } else if (grm[c] != rm[c] || grv[c] != rv[c]) cs.fail("eval changed the running statistics of channel %d", c);
  }
  cs.done();
}

static void bn_bwd_case(int C, bool reps, bool with_q) {
  Case cs("bn bwd C%d%s %s", C, reps ? " replicas" : "", with_q ? "q/r x3" : "qd-null");
  const double count = 4096.0;
  const float gs = 1.f / 128.f;
  const int stride = reps ? C + 3 : 0, ncall = with_q ? 3 : 1;
  std::vector<float> mean(C), istd(C), scale(C);
  for (int c = 0; c < C; ++c) { mean[c] = (float)(unif(31, c) * 2 - 1); istd[c] = (float)(0.3 + unif(32, c) * 3); scale[c] = (float)(unif(33, c) * 3 - 1.5); }
  // S1, S2 of the three calls: multiples of 2^-10 up to 100, and a third call that cancels the first two down to 2^-30 (about 1e-9) of
  // their size - 48 significant bits at most, so that the sixteenth shares of a replicated layout and their fp64 sums are exact
  std::vector<std::vector<double>> S1(3, std::vector<double>(C)), S2(3, std::vector<double>(C));
  auto grid = [](uint64_t seed, int c) { return std::floor((unif(seed, c) * 200 - 100) * 1024.0) / 1024.0 + 1.0 / 1024; };
  for (int c = 0; c < C; ++c) {
    S1[0][c] = grid(41, c); S2[0][c] = grid(42, c);
    S1[1][c] = grid(43, c) + 3.0; S2[1][c] = grid(44, c) - 3.0;
    S1[2][c] = -(S1[0][c] + S1[1][c]) * (1.0 - std::ldexp(1.0, -30)); S2[2][c] = -(S2[0][c] + S2[1][c]) * (1.0 - std::ldexp(1.0, -30));
  }
  Dev dmean(mean), distd(istd), dscale(scale);
  std::vector<double> zc(C, 0.0);
  std::vector<float> fill(C, -77.f);
  Out odg(nullptr, C * 4), odb(nullptr, C * 4), oqd(zc.data(), C * 8), ord_(zc.data(), C * 8);
  Out oq(fill.data(), C * 4), orr(fill.data(), C * 4), oql(fill.data(), C * 4), orl(fill.data(), C * 4);
  std::vector<long double> qref(C, 0), rref(C, 0);
  std::vector<double> qbig(C, 0), rbig(C, 0);
  for (int call = 0; call < ncall; ++call) {
    std::vector<double> r1(stride ? (size_t)STAT_REPS * stride : C, 0.0), r2(r1.size(), 0.0);
    static const int w[8] = {2, 1, 4, 1, 3, 2, 1, 2};
    for (int c = 0; c < C; ++c) {
      if (!stride) { r1[c] = S1[call][c]; r2[c] = S2[call][c]; }
      else for (int k = 0; k < STAT_REPS; ++k) { r1[(size_t)k * stride + c] = S1[call][c] * w[k % 8] / 16.0 * (8.0 / STAT_REPS); r2[(size_t)k * stride + c] = S2[call][c] * w[k % 8] / 16.0 * (8.0 / STAT_REPS); }
    }
    Dev d1(r1), d2(r2);
    BnBwdFinalizeArgs a;
    memset(&a, 0, sizeof(a));
    a.red1 = d1.as<double>(); a.red2 = d2.as<double>(); a.stat_stride = stride;
    a.mean = dmean.as<float>(); a.invstd = distd.as<float>(); a.scale = dscale.as<float>();
    a.dgamma = odg.as<float>(); a.dbeta = odb.as<float>();
    a.qd = with_q ? oqd.as<double>() : nullptr; a.rd = with_q ? ord_.as<double>() : nullptr;
    a.q = oq.as<float>(); a.r = orr.as<float>(); a.ql = oql.as<float>(); a.rl = orl.as<float>();
    a.count = count; a.grad_scale = gs; a.C = C;
    ran(launch_bn_bwd_finalize(a, nullptr), cs.name.c_str());
    std::vector<float> gdg(C), gdb(C), gq(C), gr(C), gql(C), grl(C);
    std::vector<double> gqd(C), grd(C);
    bool ok = odg.fetch(gdg.data(), cs, "dgamma");
    ok = odb.fetch(gdb.data(), cs, "dbeta") && ok;
    ok = oqd.fetch(gqd.data(), cs, "qd") && ok;
    ok = ord_.fetch(grd.data(), cs, "rd") && ok;
    ok = oq.fetch(gq.data(), cs, "q") && ok;
    ok = orr.fetch(gr.data(), cs, "r") && ok;
    ok = oql.fetch(gql.data(), cs, "ql") && ok;
    ok = orl.fetch(grl.data(), cs, "rl") && ok;
    for (int c = 0; ok && c < C; ++c) {
      // dgamma / dbeta: one fp32 rounding of an fp64 product (half an ulp, 2^-24) with a 2x margin
      const double wdg = S2[call][c] * (double)gs, wdb = S1[call][c] * (double)gs, R1 = std::ldexp(1.0, -23);
      if (!close_rel(gdg[c], wdg, std::fabs(wdg), R1)) cs.fail("call %d dgamma[%d] got %.9g want %.17g", call, c, gdg[c], wdg);
      if (!close_rel(gdb[c], wdb, std::fabs(wdb), R1)) cs.fail("call %d dbeta[%d] got %.9g want %.17g", call, c, gdb[c], wdb);
      if (!with_q) {
        if (gq[c] != -77.f || gr[c] != -77.f || gql[c] != -77.f || grl[c] != -77.f || gqd[c] != 0 || grd[c] != 0) cs.fail("qd null, yet q / r of channel %d were written", c);
        continue;
      }
      const long double s = scale[c], mu = mean[c], is = istd[c], c1 = (long double)S1[call][c] / count, c2 = (long double)S2[call][c] / count;
      const long double t1 = -s * c1, t2 = s * c2 * mu * is, t3 = -s * c2 * is;
      qref[c] += t1 + t2; rref[c] += t3;
      qbig[c] = std::max(qbig[c], (double)std::max(fabsl(t1), fabsl(t2))); rbig[c] = std::max(rbig[c], (double)fabsl(t3));
      // accumulators: within 2^-50 of the largest term of the reference
      if (std::fabs((double)((long double)gqd[c] - qref[c])) > std::ldexp(qbig[c], -50)) cs.fail("call %d qd[%d] got %.17g want %.17Lg (largest term %.3g)", call, c, gqd[c], qref[c], qbig[c]);
      if (std::fabs((double)((long double)grd[c] - rref[c])) > std::ldexp(rbig[c], -50)) cs.fail("call %d rd[%d] got %.17g want %.17Lg (largest term %.3g)", call, c, grd[c], rref[c], rbig[c]);
      // the hi / lo split loses at most half an ulp of the lo part: 2^-48 of the accumulator, 2^-47 with the 2x margin - against the
      // accumulator the kernel holds after every call, and against the reference before any cancellation (first call)
      if (std::fabs(gqd[c] - ((double)gq[c] + (double)gql[c])) > std::ldexp(std::fabs(gqd[c]), -47)) cs.fail("call %d q+ql[%d] = %.17g, accumulator %.17g", call, c, (double)gq[c] + gql[c], gqd[c]);
      if (std::fabs(grd[c] - ((double)gr[c] + (double)grl[c])) > std::ldexp(std::fabs(grd[c]), -47)) cs.fail("call %d r+rl[%d] = %.17g, accumulator %.17g", call, c, (double)gr[c] + grl[c], grd[c]);
      if (call == 0) {
        if (std::fabs((double)(qref[c] - ((long double)gq[c] + gql[c]))) > std::ldexp((double)fabsl(qref[c]), -47) + std::ldexp(qbig[c], -50)) cs.fail("q+ql[%d] = %.17g want %.17Lg", c, (double)gq[c] + gql[c], qref[c]);
        if (std::fabs((double)(rref[c] - ((long double)gr[c] + grl[c]))) > std::ldexp((double)fabsl(rref[c]), -47)) cs.fail("r+rl[%d] = %.17g want %.17Lg", c, (double)gr[c] + grl[c], rref[c]);
      }
    }
  }
  cs.done();
}

static void group_bn() {
  for (int C : {1, 8, 129, 200}) {
    bn_fwd_case(C, 1, false, 0);
    bn_fwd_case(C, 1, true, 1);
    bn_fwd_case(C, 1, false, 2);
    bn_fwd_case(C, 0, false, 0);
  }
  for (int C : {1, 129})
    for (int reps = 0; reps < 2; ++reps) { bn_bwd_case(C, reps, false); bn_bwd_case(C, reps, true); }
}

// ---------------------------------------------------------------------------------------------------- max pooling
// BN + ReLU + 3x3 stride-2 pad-1 max pooling.  Grids: y0 in halves up to +-2, scale in {+-0.5, +-1, 2}, shift in halves up to +-1: the
// activation is a multiple of 1/4 up to 5 - exact in every storage type, with many ties (ReLU zeros above all).
struct Pool {
  int B, H0, W0, C, ld0, Hp, Wp;
  std::vector<float> y0;          // (B, H0, W0, ld0); padding channels hold 99
  std::vector<float> sc, sh;      // C
  std::vector<float> out;         // (B, Hp, Wp, C) reference
  std::vector<uint8_t> am;        // (B, Hp, Wp, C) reference: first maximum in row-major order among the in-image taps, counted 0..8
  bool exact = true;
  size_t npix0() const { return (size_t)B * H0 * W0; }
  size_t npixp() const { return (size_t)B * Hp * Wp; }
};
static void pool_make(Pool& P, int B, int H0, int W0, int C, int ld0, int mode, uint64_t seed) {
  P.B = B; P.H0 = H0; P.W0 = W0; P.C = C; P.ld0 = ld0; P.Hp = (H0 - 1) / 2 + 1; P.Wp = (W0 - 1) / 2 + 1;
  static const float SC[5] = {0.5f, -0.5f, 1.f, -1.f, 2.f};
  P.sc.resize(C); P.sh.resize(C);
  for (int c = 0; c < C; ++c) { P.sc[c] = pick(seed + 1, c, SC); P.sh[c] = dyad(seed + 2, c, 2, 0.5f); }
  if (C > 1) P.sc[1] = -1.f;   // at least one negative scale
  if (mode == 1) for (int c = 0; c < C; c += 2) { P.sc[c] = 1.f; P.sh[c] = -2.5f; }   // even channels: every window negative before the ReLU
  P.y0.assign(P.npix0() * ld0, 99.f);
  par_for(P.npix0(), [&](size_t lo, size_t hi, int) {
    for (size_t p = lo; p < hi; ++p)
      for (int c = 0; c < C; ++c) {
        const uint64_t i = p * C + c;
        P.y0[p * ld0 + c] = mode == 1 && (c & 1) ? (float)(mix(seed, i) & 1) : dyad(seed, i, 4, 0.5f);   // mode 1, odd channels: ties of {0, 1}
      }
  }, 1 << 12);
  P.out.resize(P.npixp() * C); P.am.resize(P.npixp() * C);
  std::vector<int> inexact(n_threads(), 0);
  par_for(P.npixp(), [&](size_t lo, size_t hi, int t) {
    for (size_t p = lo; p < hi; ++p) {
      const int ox = (int)(p % P.Wp), oy = (int)((p / P.Wp) % P.Hp), b = (int)(p / ((size_t)P.Wp * P.Hp));
      for (int c = 0; c < C; ++c) {
        double best = 0; int arg = -1;
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
            if (iy < 0 || ix < 0 || iy >= H0 || ix >= W0) continue;
            const float y = P.y0[((size_t)(b * H0 + iy) * W0 + ix) * ld0 + c];
            double v = (double)y * P.sc[c] + P.sh[c];
            if (v < 0) v = 0;
            float vf = y * P.sc[c]; vf += P.sh[c]; if (vf < 0) vf = 0;
            if ((double)vf != v) inexact[t] = 1;
            if (arg < 0 || v > best) { best = v; arg = ky * 3 + kx; }
          }
        P.out[p * C + c] = (float)best; P.am[p * C + c] = (uint8_t)arg;
      }
    }
  }, 1 << 10);
  for (int v : inexact) if (v) P.exact = false;
}

static void pool_case(int dt, const char* nm, int B, int H0, int W0, int C, int ld0, int ldo, int off, int stride, int mode) {
  Case cs("pool %s %s B%d H%d W%d C%d ld0=%d ldo=%d+%d stride=%d", DTN[dt], nm, B, H0, W0, C, ld0, ldo, off, stride);
  Pool P;
  pool_make(P, B, H0, W0, C, ld0, mode, 100 + dt);
  if (!P.exact) cs.fail("probe bug: the activation is not exact in fp32 on this grid");
  for (float v : P.out) if (rnd_to(dt, v) != v) { cs.fail("probe bug: pooled value %g is not representable in %s", v, DTN[dt]); break; }
  const size_t np = P.npixp();
  const float FILL = -7.5f;
  std::vector<float> out0(np * ldo, FILL);
  std::vector<uint8_t> y0b = pack(dt, P.y0), out0b = pack(dt, out0);
  Dev dy0(y0b), dsc(P.sc), dsh(P.sh);
  Out oout(out0b.data(), out0b.size()), oam(nullptr, np * C);
  std::vector<double> st0 = stat_init(C, stride);
  Out osum(st0.data(), st0.size() * 8), osq(st0.data(), st0.size() * 8);
  MaxpoolArgs a;
  memset(&a, 0, sizeof(a));
  a.y0 = dy0.p; a.ld0 = ld0; a.H0 = H0; a.W0 = W0; a.B = B; a.C = C; a.scale = dsc.as<float>(); a.shift = dsh.as<float>();
  a.out = oout.as<uint8_t>() + (size_t)off * esz(dt); a.ldo = ldo; a.Hp = P.Hp; a.Wp = P.Wp; a.argmax = oam.as<unsigned char>();
  a.stat_sum = osum.as<double>(); a.stat_sq = osq.as<double>(); a.stat_stride = stride;
  ran(launch_maxpool_fwd(a, dt, nullptr), cs.name.c_str());
  std::vector<uint8_t> gout(out0b.size()), gam(np * C);
  if (oout.fetch(gout.data(), cs, "out"))
    check_tensor(cs, "out", dt, gout.data(), np * ldo, [&](size_t i) {
      const size_t p = i / ldo; const int ch = (int)(i % ldo) - off;
      return enc(dt, ch >= 0 && ch < C ? P.out[p * C + ch] : FILL);   // channels beside the destination range stay as they were
    });
  if (oam.fetch(gam.data(), cs, "argmax"))
    for (size_t i = 0; i < gam.size(); ++i)
      if (gam[i] != P.am[i]) { cs.fail("argmax[%zu] (pixel %zu channel %zu) got %d want %d", i, i / C, i % C, gam[i], P.am[i]); break; }
  std::vector<double> ws(C, 0.0), wq(C, 0.0), gs(st0.size()), gq(st0.size());
  for (size_t p = 0; p < np; ++p) for (int c = 0; c < C; ++c) { const double v = P.out[p * C + c]; ws[c] += v; wq[c] += v * v; }
  if (osum.fetch(gs.data(), cs, "stat_sum")) check_stats(cs, "stat_sum", gs, C, stride, ws);
  if (osq.fetch(gq.data(), cs, "stat_sq")) check_stats(cs, "stat_sq", gq, C, stride, wq);
  cs.done();
}

static void group_pool() {
  for (int dt = 0; dt < 3; ++dt) {
    pool_case(dt, "offset", 2, 6, 10, 64, 64, 96, 32, 0, 0);
    pool_case(dt, "idle-lanes", 2, 5, 7, 96, 104, 104, 8, 0, 0);
    pool_case(dt, "replicas", 2, 22, 27, 64, 64, 64, 0, 72, 0);          // 308 pooled pixels: 10 (16-bit) / 20 (fp32) workgroups
    pool_case(dt, "one-pixel", 1, 2, 2, 64, 64, 64, 0, 0, 0);            // five of the nine taps lie outside the image
    pool_case(dt, "neg+ties", 2, 6, 10, 64, 64, 64, 0, 0, 1);
    pool_case(dt, "cap", 1, 516, 510, 64, 64, 64, 0, 64, 0);             // 65 790 pooled pixels > 2048 workgroups x 32 (16) rows
  }
}

// Backward: gy0 = scale * dz, dz = relu'(.) * sum over the windows whose saved argmax is this pixel of the effective gradient
// g + (q + ql) + (r + rl) * x; red1 = sum dz, red2 = sum dz * (y0 - mean) * invstd.  Grids: g, q in halves, r in {+-0.5, +-1}, ql in 2^-8,
// rl in 2^-6 (zero for f16, whose kernel drops them by design), mean in halves, invstd in {0.5, 1, 2}: the effective gradient is a multiple
// of 2^-8 below 8.2, dz of 2^-8 below 33, dz * xhat of 2^-10 below 200 - eight of them summed stay within 21 bits.
static void poolbwd_case(int dt, const char* nm, int B, int H0, int W0, int C, int ld0, int ldg, int goff, int stride) {
  Case cs("poolbwd %s %s B%d H%d W%d C%d ld0=%d ldg=%d+%d stride=%d", DTN[dt], nm, B, H0, W0, C, ld0, ldg, goff, stride);
  Pool P;
  pool_make(P, B, H0, W0, C, ld0, 0, 200 + dt);
  const size_t np = P.npixp(), n0 = P.npix0();
  static const float RR[4] = {0.5f, -0.5f, 1.f, -1.f}, IS[3] = {0.5f, 1.f, 2.f};
  static const float QL[6] = {-3.f / 256, -2.f / 256, -1.f / 256, 1.f / 256, 2.f / 256, 3.f / 256}, RL[4] = {-2.f / 64, -1.f / 64, 1.f / 64, 2.f / 64};
  std::vector<float> q(C), r(C), ql(C), rl(C), mu(C), is(C);
  for (int c = 0; c < C; ++c) {
    q[c] = dyad(301, c, 2, 0.5f); r[c] = pick(302, c, RR); mu[c] = dyad(303, c, 2, 0.5f); is[c] = pick(304, c, IS);
    ql[c] = dt == DT_F16 ? 0.f : pick(305, c, QL); rl[c] = dt == DT_F16 ? 0.f : pick(306, c, RL);
  }
  std::vector<float> gp(np * ldg, 99.f), xp(np * ldg, 99.f);   // both pre-offset by goff channels inside pixel stride ldg
  par_for(np, [&](size_t lo, size_t hi, int) {
    for (size_t p = lo; p < hi; ++p)
      for (int c = 0; c < C; ++c) { gp[p * ldg + goff + c] = dyad(310 + dt, p * C + c, 4, 0.5f); xp[p * ldg + goff + c] = P.out[p * C + c]; }
  }, 1 << 12);
  // reference, window by window: each window hands its effective gradient to the pixel its argmax names
  std::vector<double> G(n0 * C, 0.0);
  std::vector<float> Gf(n0 * C, 0.f);
  const int nt = n_threads();
  std::vector<int> inexact(nt, 0);
  std::vector<double> big(nt, 0.0);
  const int cper = (C + nt - 1) / nt;
  {
    std::vector<std::thread> th;   // a thread owns a range of channels: no two threads add into the same element
    for (int t = 0; t < nt; ++t)
      th.emplace_back([&, t] {
        const int c0 = t * cper, c1 = std::min(C, c0 + cper);
        for (int b = 0; b < B; ++b) for (int oy = 0; oy < P.Hp; ++oy) for (int ox = 0; ox < P.Wp; ++ox) {
          const size_t p = ((size_t)b * P.Hp + oy) * P.Wp + ox;
          for (int c = c0; c < c1; ++c) {
            const int k = P.am[p * C + c], iy = 2 * oy - 1 + k / 3, ix = 2 * ox - 1 + k % 3;
            const double g = gp[p * ldg + goff + c], x = xp[p * ldg + goff + c];
            const double e = g + ((double)q[c] + ql[c]) + ((double)r[c] + rl[c]) * x;
            float ef = r[c] * (float)x; ef += q[c]; ef += (float)g; float lo = rl[c] * (float)x; lo += ql[c]; ef += lo;
            const size_t at = ((size_t)(b * H0 + iy) * W0 + ix) * C + c;
            G[at] += e; Gf[at] += ef;
          }
        }
      });
    for (auto& t : th) t.join();
  }
  std::vector<uint8_t> want(n0 * ld0 * esz(dt));
  const float FILL = -7.5f;
  std::vector<double> p1((size_t)nt * C, 0.0), p2((size_t)nt * C, 0.0);
  par_for(n0, [&](size_t lo, size_t hi, int t) {
    for (size_t p = lo; p < hi; ++p)
      for (int ch = 0; ch < ld0; ++ch) {
        if (ch >= C) { put_bits(dt, want.data(), p * ld0 + ch, enc(dt, FILL)); continue; }
        const double y = P.y0[p * ld0 + ch];
        const bool on = y * P.sc[ch] + P.sh[ch] > 0;
        const double dz = on ? G[p * C + ch] : 0.0, xh = (y - mu[ch]) * is[ch], o = P.sc[ch] * dz, dx = dz * xh;
        const float dzf = on ? Gf[p * C + ch] : 0.f, xhf = ((float)y - mu[ch]) * is[ch], of = P.sc[ch] * dzf, dxf = dzf * xhf;
        if ((double)dzf != dz || (double)xhf != xh || (double)of != o || (double)dxf != dx) inexact[t] = 1;
        big[t] = std::max(big[t], std::fabs(dx));
        if (std::fmod(dx, std::ldexp(1.0, -10)) != 0.0) inexact[t] = 1;
        put_bits(dt, want.data(), p * ld0 + ch, enc(dt, of));
        p1[(size_t)t * C + ch] += dz; p2[(size_t)t * C + ch] += dx;
      }
  }, 1 << 10);
  std::vector<double> w1(C, 0.0), w2(C, 0.0);
  double bigall = 0;
  for (int t = 0; t < nt; ++t) { for (int c = 0; c < C; ++c) { w1[c] += p1[(size_t)t * C + c]; w2[c] += p2[(size_t)t * C + c]; } bigall = std::max(bigall, big[t]); if (inexact[t]) P.exact = false; }
  if (!P.exact) cs.fail("probe bug: an intermediate is not exact in fp32 on this grid");
  if (8 * bigall >= std::ldexp(1.0, 14)) cs.fail("probe bug: eight dz * xhat (multiples of 2^-10 up to %g) do not fit 24 bits", bigall);

  std::vector<float> gy0init(n0 * ld0, FILL);
  std::vector<uint8_t> y0b = pack(dt, P.y0), gpb = pack(dt, gp), xpb = pack(dt, xp), gyb = pack(dt, gy0init);
  Dev dy0(y0b), dsc(P.sc), dsh(P.sh), dgp(gpb), dxp(xpb), dq(q), dr(r), dql(ql), drl(rl), dmu(mu), dis(is), dam(P.am);
  Out ogy(gyb.data(), gyb.size());
  std::vector<double> st0 = stat_init(C, stride);
  Out o1(st0.data(), st0.size() * 8), o2(st0.data(), st0.size() * 8);
  MaxpoolBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.y0 = dy0.p; a.ld0 = ld0; a.H0 = H0; a.W0 = W0; a.B = B; a.C = C; a.scale = dsc.as<float>(); a.shift = dsh.as<float>();
  a.gpool = dgp.as<uint8_t>() + (size_t)goff * esz(dt); a.xpool = dxp.as<uint8_t>() + (size_t)goff * esz(dt);
  a.q = dq.as<float>(); a.r = dr.as<float>(); a.ql = dql.as<float>(); a.rl = drl.as<float>(); a.mean = dmu.as<float>(); a.invstd = dis.as<float>();
  a.ldg = ldg; a.Hp = P.Hp; a.Wp = P.Wp; a.argmax = dam.as<unsigned char>(); a.gy0 = ogy.as<void>();
  a.red1 = o1.as<double>(); a.red2 = o2.as<double>(); a.stat_stride = stride;
  ran(launch_maxpool_bwd(a, dt, nullptr), cs.name.c_str());
  std::vector<uint8_t> got(want.size());
  if (ogy.fetch(got.data(), cs, "gy0")) {
    const size_t i = first_diff(dt, got.data(), n0 * ld0, [&](size_t j) { return get_bits(dt, want.data(), j); });
    if (i != SIZE_MAX) {
      const size_t p = i / ld0;
      cs.fail("gy0[%zu] (b %zu y %zu x %zu c %zu) got %.9g want %.9g", i, p / ((size_t)H0 * W0), (p / W0) % H0, p % W0, i % ld0, dec(dt, get_bits(dt, got.data(), i)),
              dec(dt, get_bits(dt, want.data(), i)));
    }
  }
  std::vector<double> g1(st0.size()), g2(st0.size());
  if (o1.fetch(g1.data(), cs, "red1")) check_stats(cs, "red1", g1, C, stride, w1);
  if (o2.fetch(g2.data(), cs, "red2")) check_stats(cs, "red2", g2, C, stride, w2);
  cs.done();
}

static void group_poolbwd() {
  for (int dt = 0; dt < 3; ++dt) {
    poolbwd_case(dt, "offset", 2, 6, 10, 64, 64, 96, 32, 0);
    poolbwd_case(dt, "idle-lanes", 2, 5, 7, 96, 104, 128, 16, 0);
    poolbwd_case(dt, "replicas", 2, 22, 27, 64, 64, 72, 8, 72);
    poolbwd_case(dt, "one-pixel", 1, 2, 2, 64, 64, 80, 8, 0);
    // 69 540 pixels > 2048 x 32: the walk's stride 65 536 = (2, 100, 176) carries in x and in y (fp32: 32 768 = (1, 50, 88), two steps)
    poolbwd_case(dt, "walk", 3, 122, 190, 64, 64, 72, 8, 64);
    poolbwd_case(dt, "walk-2-steps", 5, 122, 190, 64, 64, 72, 8, 64);
  }
}

// ---------------------------------------------------------------------------------------------------- apply_corr
// g += (q + ql) + (r + rl) * y.  Grids: g, y in quarters up to +-4, r in {+-0.5, +-1, 2}, q in quarters, rl in 2^-8, ql in 2^-10: every
// value is a multiple of 2^-10 below 32 (15 bits); the store rounds it to the storage type.
// wide (the rounding cases, 16-bit types): the stored gradient is s * dz + q + r * x as the backward forms it - g = s * dz with s in
// {0.75, 1.5} and dz integers below 2^(sig - 3) (g itself representable), x integers below 2^sig, r in {+-0.75, +-1.5}, q in
// halves, ql = rl = 0: the result steps in quarters up to 2^(sig + 1), up to four bits more than the type holds, and the store is ONE
// round-to-nearest-even of it (reference: the fp64 sum and the conversion written out above; the case fails if too few values round).
static void corr_case(int dt, const char* nm, size_t npix, int C, int ldg, int ldy, bool wide = false) {
  Case cs("corr %s %s npix=%zu C%d ldg=%d ldy=%d", DTN[dt], nm, npix, C, ldg, ldy);
  static const float RR[5] = {0.5f, -0.5f, 1.f, -1.f, 2.f};
  static const float RW[4] = {0.75f, -0.75f, 1.5f, -1.5f};
  std::vector<float> q(C), r(C), ql(C), rl(C);
  for (int c = 0; c < C; ++c) { q[c] = dyad(401, c, 8, 0.25f); r[c] = pick(402, c, RR); ql[c] = dyad(403, c, 3, 1.f / 1024); rl[c] = dyad(404, c, 2, 1.f / 256); }
  if (wide) for (int c = 0; c < C; ++c) { q[c] = dyad(401, c, 3, 0.5f); r[c] = pick(402, c, RW); ql[c] = 0.f; rl[c] = 0.f; }
  const int sig = dt == DT_F16 ? 11 : 8;
  float tab[33]; uint32_t tabb[33];
  for (int k = 0; k < 33; ++k) { tab[k] = (k - 16) * 0.25f; tabb[k] = enc(dt, tab[k]); }
  // the wide grids, from the element's index
  auto gwide = [&](size_t i) { return ((mix(700 + dt, i) & 1) ? 0.75f : 1.5f) * dyad(701 + dt, i, (1 << (sig - 3)) - 1, 1.f); };
  auto ywide = [&](size_t i) { return dyad(702 + dt, i, (1 << sig) - 1, 1.f); };
  const uint32_t FILLB = enc(dt, -7.5f);
  const size_t ng = npix * ldg, ny = npix * ldy;
  std::vector<uint8_t> gb(ng * esz(dt)), yb(ny * esz(dt));
  auto gidx = [&](size_t i) { return (int)(mix(500 + dt, i) % 33); };
  auto yidx = [&](size_t i) { return (int)(mix(600 + dt, i) % 33); };
  par_for(ng, [&](size_t lo, size_t hi, int) { for (size_t i = lo; i < hi; ++i) put_bits(dt, gb.data(), i, (int)(i % ldg) < C ? (wide ? enc(dt, gwide(i)) : tabb[gidx(i)]) : FILLB); });
  par_for(ny, [&](size_t lo, size_t hi, int) { for (size_t i = lo; i < hi; ++i) put_bits(dt, yb.data(), i, wide ? enc(dt, ywide(i)) : tabb[yidx(i)]); });
  Dev dy(yb), dq(q), dr(r), dql(ql), drl(rl);
  Out og(gb.data(), gb.size());
  ApplyCorrArgs a;
  memset(&a, 0, sizeof(a));
  a.g = og.as<void>(); a.y = dy.p; a.q = dq.as<float>(); a.r = dr.as<float>(); a.ql = dql.as<float>(); a.rl = drl.as<float>();
  a.npix = npix; a.C = C; a.ldg = ldg; a.ldy = ldy;
  ran(launch_apply_corr(a, dt, nullptr), cs.name.c_str());
  std::vector<int> inexact(n_threads(), 0);
  std::vector<size_t> nround(n_threads(), 0), ntie(n_threads(), 0);
  const bool ok = og.fetch(gb.data(), cs, "g");   // (the inputs are regenerated from their index)
  if (ok) {
    std::vector<size_t> bad(n_threads(), SIZE_MAX);
    std::vector<uint32_t> badw(n_threads(), 0);
    par_for(ng, [&](size_t lo, size_t hi, int t) {
      for (size_t i = lo; i < hi; ++i) {
        const int c = (int)(i % ldg);
        uint32_t w = FILLB;
        if (c < C) {
          const double g = wide ? gwide(i) : tab[gidx(i)], y = wide ? ywide((i / ldg) * ldy + c) : tab[yidx((i / ldg) * ldy + c)];
          if (wide && ((double)rnd_to(dt, (float)g) != g || (double)rnd_to(dt, (float)y) != y)) inexact[t] = 1;   // (the inputs are stored exactly)
          const double e = g + ((double)q[c] + ql[c]) + ((double)r[c] + rl[c]) * y;
          float ef = r[c] * (float)y; ef += q[c]; ef += (float)g; float lo2 = rl[c] * (float)y; lo2 += ql[c]; ef += lo2;
          if ((double)ef != e) inexact[t] = 1;
          w = enc(dt, ef);
          if (dec(dt, w) != ef) { ++nround[t]; if (std::fabs((double)dec(dt, w) - e) == half_ulp(dt, e)) ++ntie[t]; }
        }
        if (!same_value(dt, get_bits(dt, gb.data(), i), w)) { bad[t] = i; badw[t] = w; return; }
      }
    });
    for (int t = 0; t < n_threads(); ++t)
      if (bad[t] != SIZE_MAX) { cs.fail("g[%zu] (pixel %zu channel %zu) got %.9g want %.9g", bad[t], bad[t] / ldg, bad[t] % ldg, dec(dt, get_bits(dt, gb.data(), bad[t])), dec(dt, badw[t])); break; }
    for (int v : inexact) if (v) cs.fail("probe bug: the corrected gradient is not exact in fp32 on this grid");
    if (wide) {   // at least a quarter of the stores round, one in fifty is an exact tie
      size_t nr = 0, nti = 0;
      for (int t = 0; t < n_threads(); ++t) { nr += nround[t]; nti += ntie[t]; }
      if (4 * nr < npix * (size_t)C || 50 * nti < npix * (size_t)C) cs.fail("probe bug: only %zu of %zu values round (%zu ties)", nr, npix * (size_t)C, nti);
    }
  }
  cs.done();
}

static void group_corr(bool big_only, bool small_only) {
  for (int dt = 0; dt < 3; ++dt) {
    if (!big_only) {
      corr_case(dt, "one-slot", 7, slot_of(dt), 16, 24);
      corr_case(dt, "tail-loop", 1000, 64, 96, 64);
      if (dt != DT_F32) corr_case(dt, "rounding", 1000, 64, 96, 64, true);
    }
    // 128 channel slots: rows = 4 Mi / 128 = 32 768, the 4-way unrolled loop runs once and the tail loop once or twice behind it.
    // (bf16 runs the f16 instance's template with another conversion, which the small cases cover.)
    if (!small_only && dt != DT_BF16) corr_case(dt, "unrolled", (size_t)5 * 32768 + 3, 128 * slot_of(dt), 128 * slot_of(dt), 128 * slot_of(dt));
  }
}

// ---------------------------------------------------------------------------------------------------- loss / metrics
static void loss_ref(int kind, double al, double ga, double x, double t, double& l, double& d) {
  const double bce = std::max(x, 0.0) - x * t + std::log1p(std::exp(-std::fabs(x))), db = 1.0 / (1.0 + std::exp(-x)) - t;
  if (kind == 0) { l = bce; d = db; return; }
  const double omp = -std::expm1(-bce), pt = 1.0 - omp;
  if (!(omp > 0)) { l = 0; d = 0; return; }
  l = al * std::pow(omp, ga) * bce;
  d = al * db * (ga * std::pow(omp, ga - 1.0) * pt * bce + std::pow(omp, ga));
}

// way 0: plane a multiple of 4, aligned (the 16-byte branch); 1: H=3 W=5; 2: logits 4 bytes past a 16-byte boundary (both scalar)
static void loss_case(int dt, int NC, int B, int H, int W, int way, int kind) {
  static const char* WAY[3] = {"vec4", "odd-plane", "misaligned"};
  Case cs("loss %s %s NC%d B%d H%d W%d %s", DTN[dt], WAY[way], NC, B, H, W, kind ? "focal" : "bce");
  const size_t plane = (size_t)H * W, n = (size_t)B * NC * plane;
  const float thr = 0.7f, loss_scale = 128.f, dynv = 0.5f;
  const float AL[8] = {1.f, 0.25f, 2.f, 0.5f, 1.f, 0.75f, 1.5f, 1.f}, GA[8] = {2.f, 1.f, 0.5f, 1.5f, 3.f, 2.f, 1.f, 2.5f};
  std::vector<float> x(n + 1), t(n);
  par_for(n, [&](size_t lo, size_t hi, int) {
    for (size_t i = lo; i < hi; ++i) {
      const uint64_t h = mix(700 + NC * 8 + B, i);
      x[i + 1] = (h & 7) == 0 ? thr : (float)(unif(701 + NC, i) * 12 - 6);
      const int m = (int)((h >> 3) & 7);
      t[i] = m == 0 ? thr : m < 3 ? 0.f : m < 5 ? 1.f : (float)unif(702 + B, i);
    }
  });
  const float* xs = x.data() + 1;
  const int nout = 2 * NC + B * 2 * NC;
  std::vector<double> want(nout, 0.0), zero(nout, 0.0);
  std::vector<double> dref(n);
  for (size_t i = 0; i < n; ++i) {
    const int c = (int)((i / plane) % NC), b = (int)(i / (plane * NC));
    double l, d;
    loss_ref(kind, AL[c], GA[c], xs[i], t[i], l, d);
    dref[i] = d;
    const bool pp = xs[i] >= thr, gg = t[i] >= thr;
    want[c] += l; want[NC + c] += pp == gg; want[2 * NC + b * 2 * NC + c] += pp && gg; want[2 * NC + b * 2 * NC + NC + c] += pp || gg;
  }
  // way 2 hands the kernel a pointer 4 bytes past the (256-byte aligned) allocation; the others skip the leading float
  Dev dx;
  if (way == 2) dx.set(x.data(), (n + 1) * 4);
  else dx.set(xs, n * 4);
  Dev dtg(t), ddyn(&dynv, 4);
  Out odl(nullptr, (size_t)B * plane * 8 * esz(dt)), oout(zero.data(), nout * 8);
  BceArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = dx.as<float>() + (way == 2 ? 1 : 0); a.target = dtg.as<float>(); a.dlogits = odl.as<void>(); a.out = oout.as<double>();
  a.B = B; a.NC = NC; a.H = H; a.W = W; a.thr = thr; a.loss_scale = loss_scale; a.kind = kind; a.from_prob = 0;
  for (int i = 0; i < 8; ++i) { a.alpha[i] = AL[i]; a.gamma[i] = GA[i]; }
  a.metrics = 1; a.dyn_scale = ddyn.as<float>();
  ran(launch_bce_metrics(a, dt, nullptr), cs.name.c_str());
  std::vector<double> got(nout);
  if (oout.fetch(got.data(), cs, "out"))
    for (int i = 0; i < nout; ++i) {
      if (i < NC) { if (std::fabs(got[i] - want[i]) > 1e-6 * std::fabs(want[i])) cs.fail("loss sum[%d] got %.12g want %.12g", i, got[i], want[i]); }
      else if (got[i] != want[i]) cs.fail("count out[%d] got %.17g want %.17g", i, got[i], want[i]);   // counts are exact
    }
  std::vector<uint8_t> gd(odl.n);
  if (odl.fetch(gd.data(), cs, "dlogits")) {
    const double gscale = (double)loss_scale * dynv;
    for (size_t p = 0; p < (size_t)B * plane && !cs.bad; ++p)
      for (int c = 0; c < 8; ++c) {
        const uint32_t bits = get_bits(dt, gd.data(), p * 8 + c);
        const double g = dec(dt, bits);
        if (c >= NC) { if (!same_value(dt, bits, 0)) cs.fail("dlogits pixel %zu slot %d (>= NC) holds %.9g (0x%x), not zero", p, c, g, bits); continue; }
        const double d = dref[((p / plane) * NC + c) * plane + p % plane], w = d * gscale;
        // the project's dx bound (rtol 2e-4, atol 2e-6) on the unscaled derivative plus half an ulp of the storage type
        const double tol = gscale * (2e-4 * std::fabs(d) + 2e-6) + half_ulp(dt, w);
        if (!(std::fabs(g - w) <= tol)) cs.fail("dlogits pixel %zu class %d got %.9g want %.9g (tol %.3g)", p, c, g, w, tol);
      }
  }
  cs.done();
}

static void group_loss() {
  for (int dt = 0; dt < 3; ++dt) {
    for (int NC : {1, 3, 4, 8})
      for (int B : {1, 3}) {
        const int kind = NC == 3 || NC == 8;
        loss_case(dt, NC, B, 4, 6, 0, kind);
        loss_case(dt, NC, B, 3, 5, 1, kind);
        loss_case(dt, NC, B, 4, 6, 2, kind);
      }
    loss_case(dt, 3, 8, 260, 256, 0, 0);   // 66 560 pixels per image > 64 workgroups x 256 threads x 4: the 16-byte branch loops
  }
}

int main(int argc, char** argv) {
  const std::string g = argc > 1 ? argv[1] : "";
  if (g == "convert") group_convert();
  else if (g == "bn") group_bn();
  else if (g == "pool") group_pool();
  else if (g == "poolbwd") group_poolbwd();
  else if (g == "corr") group_corr(false, false);
  else if (g == "corr-small") group_corr(false, true);   // the two halves of `corr`, for timing the 335 MB cases on their own
  else if (g == "corr-big") group_corr(true, false);
  else if (g == "loss") group_loss();
  else { fprintf(stderr, "usage: pointwise_probe convert|bn|pool|poolbwd|corr|loss\n"); return 2; }
  return g_failed ? 1 : 0;
}
