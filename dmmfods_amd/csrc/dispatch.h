// How a convolution / weight-gradient launch finds its kernel family, and the two host helpers every launcher shares.
//
// A family is one row of a table (igemm.hip: kConvFamilies, wgrad.hip: kWgradFamilies; the order of a table is the dispatch order):
//   resolve()  host-only and pure: refuses the launch (false) or fills `Resolved` with everything the launch needs that does not depend
//              on the device - the family's argument block AND the kernel instantiation that will run (a function pointer out of the
//              family's one ladder of instantiations: "is there an instantiation?" and "which one?" are the same question).  It does not
//              call the HIP runtime, read global state or print;
//   launch()   takes what resolve filled, adds the device-dependent part (workgroup counts from the compute-unit count) and launches.
//              It cannot refuse a shape: what it returns is the runtime's error.
// igemm_pick / wgrad_pick (plan.cpp, while a plan is built) and launch_igemm / launch_wgrad (at run time) walk the SAME table with the
// SAME resolve, so a refusal the plan cannot see does not exist.
// A family is switched off by ONE word, the deny mask (1 << family), handed down as an argument: a plan carries the mask it was built
// under (dmm_plan::deny = DMM_NO_HF + the process-wide switches of dmm_set_option, capi.cpp), a single-kernel entry point passes the
// process-wide switches of the moment.  No kernel file keeps a switch of its own.
#pragma once
#include <new>

#include "common.h"

namespace dmm {

// What a family's resolve hands to its launch: a block of the family's own type (CfLaunch, WgpLaunch, ...: plain data).
struct Resolved {
  int form = 0;  // the form of the family that runs, where a family has several (cvp: IMPL_CVW, wgp: IMPL_WGPW; 0: the family's own)
  alignas(16) unsigned char block[1536];
  template <typename L> L& put() {
    static_assert(sizeof(L) <= sizeof(block) && alignof(L) <= 16, "Resolved::block is too small for this family");
    return *new (block) L;
  }
  template <typename L> const L& get() const { return *reinterpret_cast<const L*>(block); }
};
struct ConvFamily {
  int family;  // enum Impl
  bool (*resolve)(const ConvArgs& a, int dtype, int epi, Resolved& r);
  hipError_t (*launch)(const Resolved& r, hipStream_t st);
};
struct WgradFamily {
  int family;
  bool (*resolve)(const WgradArgs& a, int dtype, Resolved& r);
  hipError_t (*launch)(const Resolved& r, hipStream_t st);
};
// May `f` take a launch?  impl = IMPL_AUTO: every family that `deny` (1 << family) does not name; otherwise only the family a plan
// recorded, whatever the switches say now.
template <typename F> inline bool family_allowed(const F& f, int impl, unsigned deny) {
  return impl == IMPL_AUTO ? !((deny >> f.family) & 1u) : impl == f.family;
}
// The families a lab build (common.h: lab_flag) switches off from the environment: the initial value of the process-wide mask.
// Constant 0 in the shipped library.
inline unsigned lab_family_off() {
  return (lab_flag("DMM_NO_CONV3") ? 1u << IMPL_CONV3 : 0) | (lab_flag("DMM_NO_WG3") ? 1u << IMPL_WG3 : 0) |
         (lab_flag("DMM_NO_WG5") ? 1u << IMPL_WG5 : 0) | (lab_flag("DMM_NO_WGP") ? 1u << IMPL_WGP : 0) |
         (lab_flag("DMM_NO_CVP") ? 1u << IMPL_CVP : 0) | (lab_flag("DMM_NO_PIG") ? 1u << IMPL_PIG : 0) |
         (lab_flag("DMM_NO_BW1") ? 1u << IMPL_BW1 : 0) | (lab_flag("DMM_NO_CF") ? 1u << IMPL_CF : 0) |
         (lab_flag("DMM_NO_HALO") ? 1u << IMPL_HALO : 0);
}

#define DMM_CONV_FAMILY(name)                                              \
  bool name##_resolve(const ConvArgs& a, int dtype, int epi, Resolved& r); \
  hipError_t name##_launch(const Resolved& r, hipStream_t st);
DMM_CONV_FAMILY(thin)   // thin.hip
DMM_CONV_FAMILY(hf)     // hf.hip
DMM_CONV_FAMILY(cf)     // cf.hip
DMM_CONV_FAMILY(conv3)  // conv3.hip
DMM_CONV_FAMILY(cvp)    // cvp.hip (forward, in its own form or cvw.hip's; data gradient: cvd)
DMM_CONV_FAMILY(pig)    // pig.hip
DMM_CONV_FAMILY(halo)   // halo.hip
#undef DMM_CONV_FAMILY
#define DMM_WGRAD_FAMILY(name)                                     \
  bool name##_resolve(const WgradArgs& a, int dtype, Resolved& r); \
  hipError_t name##_launch(const Resolved& r, hipStream_t st);
DMM_WGRAD_FAMILY(wg3)  // wg3.hip
DMM_WGRAD_FAMILY(wg5)  // wg5.hip
DMM_WGRAD_FAMILY(wgp)  // wgp.hip (in its own form or wgpw.hip's)
#undef DMM_WGRAD_FAMILY
// wgp.hip / wgpw.hip: how wgp_resolve cut a launch up, for either form's argument struct (the split of the tiles over workgroups is
// the launch's: wgp_split)
struct WgpGeom { int tiles_y, tiles_x, ntiles, nct, ncot, dymin, dxmin, ph_dymin[4], ph_dxmin[4]; };

// Compute units of the current device (256 where the runtime cannot say).  Not cached here: a launcher keeps the value in a static.
inline int device_cus() {
  hipDeviceProp_t pr;
  int dev = 0;
  hipGetDevice(&dev);
  return (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
}

#if defined(__HIPCC__)
// Raises KERN's limit of dynamic LDS to `bytes` - once per kernel instantiation (the flag is this instantiation's); bytes = 0: the
// default limit is enough, no attribute call.
template <auto KERN> inline hipError_t lds_limit(int bytes) {
  static bool done = false;
  if (bytes <= 0 || done) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  done = e == hipSuccess;
  return e;
}
// Launches KERN with `lds` bytes of dynamic LDS, its limit raised to `attr_bytes` first (lds_limit).
template <auto KERN, typename A>
inline hipError_t launch_lds(int attr_bytes, int nwg, int nthreads, int lds, hipStream_t st, const A& args) {
  const hipError_t e = lds_limit<KERN>(attr_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(KERN, dim3(nwg), dim3(nthreads), lds, st, args);
  return hipGetLastError();
}
#endif
// launch_lds of one instantiation of a family's kernel: what a ladder of instantiations returns (nullptr: there is none)
template <typename A> using LdsLauncher = hipError_t (*)(int attr_bytes, int nwg, int nthreads, int lds, hipStream_t st, const A& args);
// ... with its arguments: the block of a family whose launch geometry does not depend on the device
template <typename A> struct LdsLaunch {
  A g;
  int attr_bytes, nwg, nthreads, lds;
  LdsLauncher<A> run;
  hipError_t go(hipStream_t st) const { return run(attr_bytes, nwg, nthreads, lds, st, g); }
};

}  // namespace dmm
