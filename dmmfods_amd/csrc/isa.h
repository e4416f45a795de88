// The hand-written gfx950 instructions of the kernel files, once each: the transposing LDS read, raw barriers behind counted waits,
// global loads and LDS-DMA requests the compiler does not count, and the counted waits over a register set.  Device-only.
#pragma once
#include "common.h"

namespace dmm {

// ---- transposing LDS read -------------------------------------------------------------------------------------------------------
// ds_read_b64_tr_b16 moves 16-bit elements whatever they encode: the result is handed back as two dwords; two reads (rows r and
// r + 4 of the lane's group) make one MFMA fragment of eight elements.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x2 lds_tr16(const unsigned char* p) {
  typedef __fp16 h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
  h4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)(p));
  return __builtin_bit_cast(u32x2, r);
}
template <typename T>
__device__ __forceinline__ typename TT<T>::vec frag16(const u32x2& lo, const u32x2& hi) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(typename TT<T>::vec, v);
}

// ---- raw barriers ---------------------------------------------------------------------------------------------------------------
// __syncthreads() is a workgroup-scope FENCE - on gfx9 an s_waitcnt vmcnt(0) in front of the s_barrier - and drains every
// vector-memory request the wave has in flight: a prefetch, a second register set, an LDS-DMA.  Where requests must stay in flight
// across a barrier the kernels use a raw s_barrier behind a wait that names what has to be complete:
//   lds_barrier()         this wave's LDS traffic has returned; vector-memory requests stay in flight
//   vm_lds_barrier<N>()   ... and all but the wave's N youngest vector-memory requests have completed (N = 0: everything)
// Wait and barrier are ONE asm statement with a "memory" clobber, so that nothing is scheduled between them: hipcc otherwise sinks
// the last LDS reads in front of a barrier - and the wait for them - below it, where a refill of the slot they read can overtake
// them (conv3.hip's K loop, round 3: 0.1 % wrong outputs of the stem convolution at production size, never at parity-test sizes).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int N>
__device__ __forceinline__ void vm_lds_barrier() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory"); }

// ---- global loads and counted waits from inline assembly -------------------------------------------------------------------------
// The loader waves of the wave-specialised kernels keep TWO (or more) register sets of global loads in flight and wait for the OLDER
// one.  Written as plain C++ loads hipcc counted them itself and, at the header of the two-set loop, waited vmcnt(13) ... vmcnt(0) for
// the older set (27 ... 14 would do): its merged wait-count state dropped the newer set, every other tile drained the whole ring, and
// the kernel ran no faster than the four-wave one (ISA of wg3.hip's first version, round 4).  From assembly the compiler counts
// nothing: a loader wave's only vector-memory operations are these loads, issued set by set in program order, and loads return in
// order, so "all but the newest N have returned" - s_waitcnt vmcnt(N), N = the requests issued BEHIND the set - is exactly "the older
// set has landed".  Data flow is explicit - the load defines the register, the wait takes every register of the set as a read-write
// operand, the prologue reads the wait's outputs - so nothing can be scheduled across; tools/check_asm_loads.py checks in the
// disassembly that no instruction reads a loaded register between its load and its wait.
// Two rules for the code around them (both found by that checker): a set is an operand of a wait or a hold at the LAST point where
// its loads may still be landing - the compiler considers its registers free from their last use on -, and no load sits in an arm of
// a branch (the set would become a phi of two registers: a copy of data that has not landed).
//
//   gload16(dst, ptr)         16 bytes from a 64-bit per-lane address
//   gload16(dst, base, off)   ... from a uniform base (a scalar register pair) + a 32-bit per-lane byte offset: one register and
//                             32-bit arithmetic per load; the launchers refuse tensors of 4 GiB or more
template <typename V>
__device__ __forceinline__ void gload16(V& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p));
}
template <typename V>
__device__ __forceinline__ void gload16(V& dst, const void* base, unsigned off) {
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(off), "s"(base));
}

// Operand lists: every register of an array of that extent, read-write.  (A parameter pack cannot be expanded inside an operand
// list, and one statement per register is a different kernel: the wait is ONE statement over the whole set.)  The wrapper that uses
// one asserts the extent of the array it hands over right beside it.
#define DMM_V3(r) "+v"(r[0]), "+v"(r[1]), "+v"(r[2])
#define DMM_V4(r) DMM_V3(r), "+v"(r[3])
#define DMM_V6(r) DMM_V4(r), "+v"(r[4]), "+v"(r[5])
#define DMM_V8(r) DMM_V6(r), "+v"(r[6]), "+v"(r[7])
#define DMM_V10(r) DMM_V8(r), "+v"(r[8]), "+v"(r[9])
// DMM_VM_WAIT(keep, sets...): the sets have landed once all but the wave's `keep` youngest requests have returned (keep = 0: everything
// lands).  DMM_VM_HOLD(sets...): no instruction - the sets stay alive (their registers untouched) up to this point.
#define DMM_VM_WAIT(keep, ...) asm volatile("s_waitcnt vmcnt(%[k])" : __VA_ARGS__ : [k] "n"(keep))
#define DMM_VM_HOLD(...) asm volatile("; hold" : __VA_ARGS__)

// ---- LDS-DMA --------------------------------------------------------------------------------------------------------------------
// 16 bytes per lane from global memory straight into LDS at the wave-uniform address `lds_dst` (+ 16 x lane), m0 saved and restored.
// From assembly hipcc does not count the request, so it does not drain it (vmcnt(0)) in front of the next ds_read as it does for
// the builtin (it cannot prove that the LDS ranges differ); the callers' counted barriers retire it.
__device__ __forceinline__ void lds_dma16(const void* src, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}

}  // namespace dmm
