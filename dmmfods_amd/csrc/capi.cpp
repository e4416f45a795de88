// extern "C" surface of libdmmfods_hip.so (see include/dmmfods_hip.h) and the launch-list executor.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include <unistd.h>

#include "dispatch.h"
#include "plan.h"

using namespace dmm;

void plan_build_tables(dmm_plan* p);
void plan_bind(dmm_plan* p, void* ws);
void plan_size(dmm_plan* p);

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e__ = (expr);                                                                           \
    if (e__ != hipSuccess) return fail(DMM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

static bool g_overlap_wgrad = getenv("DMM_NO_OVERLAP") == nullptr;
static int g_graph = getenv("DMM_GRAPH") ? std::max(1, atoi(getenv("DMM_GRAPH"))) : 0;  // off by default: see launch_list (1: both lists, 2: the forward list only)
static unsigned long long g_option_epoch = 1;  // bumped by every dmm_set_option: captured graphs have the options of their time baked in
// Launch coalescing (WgradBatches): the dense 3x3 weight gradients (wg3) and the bw1 reductions of consecutive layers go out as grouped
// launches.  dmm_set_option("batch_wgrad"): 0 every record is its own launch, as before the option existed; 1 (default) grouped, on
// the CALLER's stream; 2 grouped, on the weight-gradient stream where the single launches run
static int g_batch_wgrad = 1;
static int g_bucket_mb = getenv("DMM_GRAD_BUCKET_MB") ? atoi(getenv("DMM_GRAD_BUCKET_MB")) : 25;
// The kernel families switched off for the process, 1 << family (dmm_set_option; a lab build starts from its DMM_NO_* flags).  The one
// switch there is: a plan copies it into dmm_plan::deny in front of each builder pass, a single-kernel entry point passes it at every call.
static std::atomic<unsigned> g_family_off{lab_family_off()};
// the deny mask a plan is built under: its own switch + the process-wide ones of this moment
static unsigned plan_deny(const dmm_plan* p) { return (p->sw.no_hf ? 1u << IMPL_HF : 0u) | g_family_off; }

// ------------------------------------------------------------------------------------------------ streams and events of the process
// One pool per device, created on first use and NEVER torn down: the three helper streams (side: weight gradients, backward leaves,
// the second encoder; pack: the late layers' weight pack; capture: hipGraph capture) live as long as the process, events go back
// to free lists when a plan is destroyed.  Round 4's teardown destroyed two low-priority streams and ~200 events per plan, ~350 plans
// per test process, without synchronising anything - and the driver's GPU suite died of a segmentation fault raised on a runtime
// thread (no Python thread state: faulthandler marked no thread "Current") while the main thread was inside dmm_plan_destroy.  The
// last user of a priority level's hardware queue going away is a queue destruction inside the runtime; a plan has no business causing
// one.  Nothing here is destroyed at exit either (no static destructor may touch a runtime that is unloading): the pointers leak by design.
namespace {
struct DevicePool {
  std::mutex mu;
  hipStream_t side = nullptr, pack = nullptr, capture = nullptr;
  std::vector<hipEvent_t> free_plain, free_timing;   // hipEventDisableTiming / timing events handed back by destroyed plans
  long events_made = 0;
};
constexpr int MAX_DEVICES = 64;
DevicePool* g_pools[MAX_DEVICES] = {};
std::mutex g_pools_mu;

DevicePool* pool_of(int device) {
  if (device < 0 || device >= MAX_DEVICES) return nullptr;
  std::lock_guard<std::mutex> l(g_pools_mu);
  if (g_pools[device] == nullptr) g_pools[device] = new DevicePool();
  return g_pools[device];
}
// the helper streams of the CURRENT device's pool (created on first use)
hipError_t pool_streams(DevicePool* dp, bool want_capture) {
  std::lock_guard<std::mutex> l(dp->mu);
  if (dp->side == nullptr) {
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (e != hipSuccess) return e;
    // lowest priority: the data-gradient chain on the caller's stream is the longer dependency chain (mid / high measured in round 2:
    // 33.6 / 33.8 / 33.9 ms; confining the stream to a CU mask in round 4: 41-57 ms instead of 28)
    hipStream_t s = nullptr, k = nullptr;
    if ((e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, lo)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithPriority(&k, hipStreamNonBlocking, lo)) != hipSuccess) return e;   // (s leaks: the process is in trouble anyway)
    dp->side = s; dp->pack = k;
  }
  if (want_capture && dp->capture == nullptr) {
    hipStream_t c = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&c, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    dp->capture = c;
  }
  return hipSuccess;
}
hipEvent_t pool_event(DevicePool* dp, bool timing) {
  std::lock_guard<std::mutex> l(dp->mu);
  auto& fl = timing ? dp->free_timing : dp->free_plain;
  if (!fl.empty()) { hipEvent_t e = fl.back(); fl.pop_back(); return e; }
  hipEvent_t e = nullptr;
  const hipError_t rc = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
  if (rc != hipSuccess) return nullptr;
  ++dp->events_made;
  return e;
}
void pool_return(DevicePool* dp, std::vector<void*>& evs, bool timing) {
  std::lock_guard<std::mutex> l(dp->mu);
  auto& fl = timing ? dp->free_timing : dp->free_plain;
  for (void* e : evs) if (e) fl.push_back((hipEvent_t)e);
  evs.clear();
}
// DMM_TRACE_DESTROY=1: one line per teardown step, written straight to fd 2 (no buffering: the line in front of a fault survives it)
void trace_destroy(const char* what) {
  static const bool on = getenv("DMM_TRACE_DESTROY") != nullptr;
  if (!on) return;
  char buf[160];
  const int n = snprintf(buf, sizeof(buf), "[dmm] destroy: %s\n", what);
  if (n > 0) { ssize_t w = write(2, buf, (size_t)std::min<int>(n, (int)sizeof(buf) - 1)); (void)w; }
}
}  // namespace

// ------------------------------------------------------------------------------------------------ the launch-list executor
// run_ops walks a range of launch records; each concern has one owner: the predicates (which lane, which batch - from the record alone),
// Lanes (streams, fork and join events), ProfilePass (event pairs), WgradBatches (the two pending grouped launches), launch_record.
// Overlap: a weight gradient only needs what the ops before it produced, and nothing but the final unpack reads it, so
// it goes to a low-priority side stream (fork event before, one join before unpack).  Late layers launch a few hundred
// workgroups of a few microseconds; two independent chains fill the CUs that one chain leaves idle.  The records that may run
// beside the data-gradient chain: weight gradients and the leaves of the backward graph (stem, raw-input branches) - unless the
// chain waits for them (Op::chain).
static bool beside_chain(const Op& o) { return !o.chain && (o.kind == OP_WGRAD || o.leaf); }
// the two kinds of record that have a grouped launch (batched or launched alone, they share the family's slot buffer)
static bool grouped_family(const Op& o) { return (o.kind == OP_WGRAD && o.impl == IMPL_WG3) || o.kind == OP_BW1RED; }
bool dmm::side_forks(const Op& o) { return beside_chain(o) && o.leaf != 2 && o.leaf != 3; }
// A record that carries a bucket signal is never batched (the bucket is final behind ITS launch).
BatchKind dmm::batch_kind(const Op& o, bool mfma) {
  if (!side_forks(o) || o.signal >= 0) return BATCH_NONE;
  if (o.kind == OP_WGRAD && o.impl == IMPL_WG3 && mfma) return BATCH_W3;
  return o.kind == OP_BW1RED ? BATCH_RD : BATCH_NONE;
}
// A batch is flushed before any other record of the weight-gradient side, before a join with that side and before a record that
// carries a bucket signal.  "Weight-gradient side" is decided from the record alone, not from the streams of this call: the batches -
// and the bits - are the same with overlap_wgrad on or off, under capture and in a profile pass.
bool dmm::flushes_batches(const Op& o) { return side_forks(o) || o.leaf == 3 || o.signal >= 0 || (o.kind == OP_JOIN && o.epi != 1); }
Lane dmm::route(const Op& o, bool overlap, bool forked, bool batch_main) {
  // A launch that continues a chain on the side stream (the second stream's encoder): everything it reads was produced by the
  // launch in front of it on that stream, or before the chain's first launch (which forked from the main stream).  Only while
  // the side stream is forked in THIS call: a range that starts mid-chain, or a join inside the chain, makes the next launch
  // of the chain fork again like any leaf.
  if (overlap && o.leaf == 3 && forked) return LANE_SIDE_CONTINUE;
  // batch_wgrad 1: on the caller's stream, behind its producer - no fork; also the ones launched alone (see WgradBatches::st)
  if (batch_main && side_forks(o) && grouped_family(o)) return LANE_MAIN;
  if (overlap && beside_chain(o)) return o.leaf == 2 ? LANE_PACK_FORK : LANE_SIDE_FORK;
  return LANE_MAIN;
}

// The invariant behind Op::impl: the family a plan recorded for a convolution launch (and shaped its launch list around: merged
// phases, finish launches, compact gradients) is the family that took it.  `ran` = the families the launch noted.  Returns the
// complaint, or an empty string.  The generic family beside another one is a launch that fell through; the ONE launch where that is
// the design is wgp's two-segment form, whose 8-channel raw-input remainder stays with the generic kernel (launch_wgrad reports that
// launch as wgp alone today; should the remainder ever be noted as well, the launch stays allowed - by this clause, not by silence).
static std::string family_check(const Op& o, unsigned ran) {
  if ((o.kind == OP_IGEMM ? o.c.M : o.w.M) <= 0) return std::string();   // an empty launch notes nothing
  const bool recorded_ran = (ran >> o.impl) & 1u, generic_ran = (ran >> IMPL_GENERIC) & 1u;
  const bool wgp_remainder = o.kind == OP_WGRAD && o.impl == IMPL_WGP && o.w.nseg == 2 && o.w.nphase == 0;
  if (recorded_ran && (o.impl == IMPL_GENERIC || !generic_ran || wgp_remainder)) return std::string();
  std::string names;
  for (int f = 1; f < IMPL_COUNT; ++f)
    if ((ran >> f) & 1u) names += (names.empty() ? "" : "+") + std::string(dmm_impl_name(f));
  return std::string("launch '") + o.label + "': the plan recorded family " + dmm_impl_name(o.impl) + ", " + (names.empty() ? "none" : names) + " ran";
}

namespace {
// evs[i] of a plan's event vector, which grows from the device pool up to index i on first use (null: the runtime gave none)
hipEvent_t plan_event(const dmm_plan* p, std::vector<void*>& evs, size_t i, bool timing = false) {
  DevicePool* dp = i < evs.size() ? nullptr : pool_of(p->device);
  while (evs.size() <= i) {
    hipEvent_t e = dp ? pool_event(dp, timing) : nullptr;
    if (e == nullptr) return nullptr;
    evs.push_back((void*)e);
  }
  return (hipEvent_t)evs[i];
}

// The streams of one run_ops call and what is outstanding on them.  ONE side stream: 2 and 3 side streams measured 0.3 / 0.6 ms
// slower, and the leaf chains need one FIFO.  The pack stream: the launch that packs the weights of the LATE layers (leaf == 2) runs
// there beside the first layers of the forward pass; OP_JOIN with epi == 1 in front of the first late layer makes the main stream
// wait for it.  Without overlap side and pack stay null and nothing is ever forked.
struct Lanes {
  dmm_plan* p;
  hipStream_t main, side = nullptr, pack = nullptr;
  bool forked = false, pack_pending = false;   // the side / pack stream has work the main stream has not waited for
  size_t nfork = 0;                            // fork events of the plan used by this call
  hipEvent_t side_join() const { return (hipEvent_t)p->join_events[0]; }   // (dmm_plan::join_events: [0] side stream, [1] pack stream)
  hipEvent_t pack_join() const { return (hipEvent_t)p->join_events[1]; }
  const char* open_helpers() {   // with overlap: the pool's helper streams and the plan's two join events (returns what could not be had, or null)
    DevicePool* dp = pool_of(p->device);
    if (dp == nullptr || pool_streams(dp, false) != hipSuccess) return "side stream";
    side = dp->side; pack = dp->pack;
    if (plan_event(p, p->join_events, 1) == nullptr) return "hipEventCreate failed";
    p->used_side = true;
    return nullptr;
  }
  // `st` = the stream of `lane`, forked from the main stream where the lane says so (false: no fork event to be had)
  bool enter(Lane lane, hipStream_t& st) {
    st = lane == LANE_MAIN ? main : (lane == LANE_PACK_FORK ? pack : side);
    if (lane == LANE_MAIN || lane == LANE_SIDE_CONTINUE) return true;
    hipEvent_t fe = plan_event(p, p->fork_events, nfork);
    if (fe == nullptr) return false;
    ++nfork;
    hipEventRecord(fe, main);
    hipStreamWaitEvent(st, fe, 0);
    (lane == LANE_PACK_FORK ? pack_pending : forked) = true;
    return true;
  }
  // the main stream waits for what the side (pack) stream has been given so far; the pack stream's event is recorded behind its launch
  void join_side() { if (forked) { hipEventRecord(side_join(), side); hipStreamWaitEvent(main, side_join(), 0); forked = false; } }
  void record_pack_join(hipStream_t behind) { hipEventRecord(pack_join(), behind); }
  void join_pack() { if (pack_pending) { hipStreamWaitEvent(main, pack_join(), 0); pack_pending = false; } }
  void join_all() { join_side(); join_pack(); }
};

// Per-record event pairs of one recorded pass (dmm_plan_profile_begin): events [2i], [2i + 1] bracket record i on the stream it runs on.
struct ProfilePass {
  std::vector<void*>* evs = nullptr;     // null: this call records nothing
  const std::string* filter = nullptr;   // only records whose label starts with it are bracketed (empty: all)
  // takes the next pass of list `which` if the plan has one left; false: no events to be had
  bool open(dmm_plan* p, int which, size_t nops) {
    filter = &p->prof_filter;
    if (which < 0 || p->prof_max_passes <= 0 || p->prof_pass[which] >= p->prof_max_passes) return true;
    auto& sets = p->prof_events[which];
    const int pass = p->prof_pass[which]++;
    if ((int)sets.size() <= pass) sets.resize(pass + 1);
    evs = &sets[pass];
    return nops == 0 || plan_event(p, *evs, 2 * nops - 1, true) != nullptr;
  }
  // Per-op profiling keeps everything on one stream so that the event pairs bracket each kernel alone; a FILTERED profile (one
  // kernel class) runs as in production.
  bool production_schedule() const { return evs == nullptr || !filter->empty(); }
  bool selected(const Op& o) const { return evs != nullptr && (filter->empty() || strncmp(o.label, filter->c_str(), filter->size()) == 0); }
  void begin(size_t i, hipStream_t st) const { hipEventRecord((hipEvent_t)(*evs)[2 * i], st); }
  void end(size_t i, hipStream_t st) const { hipEventRecord((hipEvent_t)(*evs)[2 * i + 1], st); }
  void empty_pair(size_t i, hipStream_t st) const { begin(i, st); end(i, st); }
};

// Launch coalescing.  Within a dense block every dense 3x3 weight gradient reads only its own compact gradient, y1 and
// norm2 constants and writes its own packed gradient, and every bw1 reduction its own slots: consecutive ones are handed to ONE
// grouped launch (wg3.hip wg3_group_kernel, bw1.hip bw1_reduce_group_kernel).  A record that joins a batch is ordered behind its
// producer as before (fork event, stream wait) and notes its family; the launch goes out at the flush.  A batch is flushed
//   * where flushes_batches says so, and at the end of the range;
//   * when a member does not fit (kernel instantiation, member cap, no workgroup left);
//   * wg3, lab builds only: as soon as the pending tiles reach DMM_WG3_BATCH_TILES.  Measured on the caller's stream (C2, profiles/r06/
//     ablations.txt): 2048 / 4096 / 8192 / 16384 tiles / no threshold = 25.00 / 24.88 / 24.78 / 24.78 / 24.71 ms per step against
//     25.13 ungrouped - a dense block's layers go out together whatever their map size, hence no threshold (0).
// In a profile pass the flushing member's event pair brackets the grouped launch, the other members record an empty pair.
struct WgradBatches {
  dmm_plan* p;
  const std::vector<Op>& ops;
  const ProfilePass& prof;
  // The stream of the grouped launches.  They fill the chip on their own (a workgroup per compute unit, 8 waves and 86 KB of LDS
  // each), so beside the data-gradient chain they do not fill its gaps, they hold its launches up: measured at C2 (profiles/r06),
  // grouped on the weight-gradient stream the step is 0.1-0.2 ms SLOWER than the ungrouped launches there, on the caller's
  // stream 0.2 ms faster.  Hence the caller's stream (batch_wgrad 1): the records of the two kinds then need no fork event either -
  // also the ones that are launched alone (a bucket signal), which share the family's slot buffer with the batches.
  hipStream_t st;
  Wg3Group w3g;
  Bw1RedGroup rdg;
  std::vector<size_t> w3_members, rd_members;
  enum Offer { ALONE, MEMBER, EMPTY };   // launched on its own; in a batch (launch and event pair at the flush); a bw1.reduce record without slots: nothing to add up
  // Record i, of batch kind k, is offered to its batch; one that does not fit sends the batch off first and is offered again.
  hipError_t offer(size_t i, const Op& o, BatchKind k, Offer& took) {
    const int dt = p->desc.dtype;
    hipError_t e = hipSuccess;
    bool in = k == BATCH_W3 ? wg3_group_add(w3g, o.w, dt) : bw1_reduce_group_add(rdg, o.b1);
    if (!in && k == BATCH_W3 && w3g.n > 0 && (e = flush_w3()) == hipSuccess) in = wg3_group_add(w3g, o.w, dt);
    if (!in && k == BATCH_RD && (e = flush_rd()) == hipSuccess) in = bw1_reduce_group_add(rdg, o.b1);
    took = !in ? ALONE : (k == BATCH_W3 || rdg.n > (int)rd_members.size()) ? MEMBER : EMPTY;
    if (took == MEMBER && k == BATCH_W3) { note_impl(IMPL_WG3); w3_members.push_back(i); ++p->batch_counts[1]; }
    if (took == MEMBER && k == BATCH_RD) { rd_members.push_back(i); ++p->batch_counts[3]; }
    return e;
  }
  template <typename Launch> hipError_t flush(std::vector<size_t>& members, Launch&& launch) {
    if (members.empty()) return hipSuccess;
    for (size_t k = 0; k + 1 < members.size(); ++k)
      if (prof.selected(ops[members[k]])) prof.empty_pair(members[k], st);
    const size_t last = members.back();
    const bool sel_last = prof.selected(ops[last]);
    members.clear();
    if (sel_last) prof.begin(last, st);
    const hipError_t e = launch();
    if (sel_last) prof.end(last, st);
    return e;
  }
  hipError_t flush_w3() { return flush(w3_members, [&] { ++p->batch_counts[0]; return wg3_group_launch(w3g, st); }); }
  hipError_t flush_rd() { return flush(rd_members, [&] { ++p->batch_counts[2]; return bw1_reduce_group_launch(rdg, st); }); }
  hipError_t flush_all() { const hipError_t e1 = flush_w3(), e2 = flush_rd(); return e1 != hipSuccess ? e1 : e2; }
  hipError_t flush_w3_if_full() { static const long long tiles = lab_int("DMM_WG3_BATCH_TILES", 0); return (tiles > 0 && w3g.tiles >= tiles) ? flush_w3() : hipSuccess; }
};

// The launch of one record on `st`.  Gradient accumulation: the list is the one of the plain mode; the arena's memset is passed over
// (its record, label and profiling slot stay) and the two kinds of launch that write the arena take their accumulate form.  known = false: no such kind.
hipError_t launch_record(dmm_plan* p, const Op& o, hipStream_t st, Lanes& lanes, bool& known) {
  const int dt = p->desc.dtype, mfma = p->desc.use_mfma != 0, accumulate = p->grad_accumulate;
  switch (o.kind) {
    case OP_MEMSET: return (accumulate && o.ms.p == (void*)p->grads) ? hipSuccess : hipMemsetAsync(o.ms.p, 0, o.ms.bytes, st);
    case OP_COPY: return hipMemcpyAsync(o.cp.dst, o.cp.src, o.cp.bytes, hipMemcpyDeviceToDevice, st);
    case OP_CONVERT: return launch_convert_input(o.cv, dt, st);
    case OP_IGEMM: return launch_igemm(o.c, dt, o.epi, mfma, st, o.impl);
    case OP_WGRAD:   // (not batched: counted as a launch of one)
      if (o.impl == IMPL_WG3 && o.w.M > 0) { ++p->batch_counts[0]; ++p->batch_counts[1]; }
      return launch_wgrad(o.w, dt, mfma, st, o.impl);
    case OP_BW1: return launch_bw1(o.b1, dt, st);
    case OP_BW1RED:
      { Bw1RedGroup one; if (bw1_reduce_group_add(one, o.b1) && one.n > 0) { ++p->batch_counts[2]; ++p->batch_counts[3]; } }
      return launch_bw1_reduce(o.b1, st);
    case OP_RAWFIN: return launch_wg5_rawfin(o.rf, st);
    case OP_FIN64: return launch_wg5_fin64(o.f64, st);
    case OP_JOIN: if (o.epi == 1) lanes.join_pack(); else lanes.join_side(); return hipSuccess;
    case OP_BNFIN: return launch_bn_finalize(o.bf, st);
    case OP_BNBWD:
      if (accumulate) { BnBwdFinalizeArgs bb = o.bb; bb.accumulate = 1; return launch_bn_bwd_finalize(bb, st); }
      return launch_bn_bwd_finalize(o.bb, st);
    case OP_POOL: return o.epi == POOL_AVG2 ? launch_avgpool2_fwd(o.ap, dt, st) : launch_maxpool_fwd(o.mp, dt, st);
    case OP_POOLBWD: return launch_maxpool_bwd(o.mpb, dt, st);
    case OP_BCE: return launch_bce_metrics(o.bce, dt, st);
    case OP_PACK: return launch_pack(o.pk.descs, o.pk.prefix, o.pk.ndesc, o.pk.total_rows, dt, st, o.pk.tdescs, o.pk.tiles, o.pk.nt1, o.pk.nt9);
    case OP_APPLYCORR: return launch_apply_corr(o.ac, dt, st);
    case OP_UNPACK: return launch_unpack(o.pk.descs, o.pk.prefix, o.pk.ndesc, o.pk.total_rows, dt, o.pk.grad_scale, st, o.pk.tdescs, o.pk.tiles, o.pk.nt1, o.pk.nt9, accumulate);
    default: known = false; return hipSuccess;
  }
}

// launch_record with the family check around it.  The families noted by THIS launch: the thread's mask is set aside, read behind the launch and
// merged back (it keeps what earlier launches noted, also when the launch fails).  Returns DMM_OK, or the error code with its message in `why`.
int launch_checked(dmm_plan* p, const Op& o, size_t i, hipStream_t st, Lanes& lanes, std::string& why) {
  const bool fam_check = (o.kind == OP_IGEMM || o.kind == OP_WGRAD) && o.impl != IMPL_AUTO;
  const unsigned mask_before = g_impl_mask;
  if (fam_check) g_impl_mask = 0;
  bool known = true;
  const hipError_t e = launch_record(p, o, st, lanes, known);
  const unsigned ran = g_impl_mask;
  if (fam_check) g_impl_mask = mask_before | ran;
  if (!known) { why = "unknown op"; return DMM_ERR_STATE; }
  if (e != hipSuccess) { why = "op " + std::to_string(i) + " kind " + std::to_string(o.kind) + ": " + hipGetErrorString(e); return DMM_ERR_HIP; }
  if (fam_check && !(why = family_check(o, ran)).empty()) return DMM_ERR_STATE;
  return DMM_OK;
}
}  // namespace

// Launches ops[begin, end) in order (end = 0: to the end of the list).
// capturing: the calls are being recorded into a hipGraph (no profiling, no bucket events: launch_list records those behind the graph).
// Per record: offer it to a batch; send the batches off if it must not overtake them; route it to its lane; bracket, launch and check it; signal
// its bucket.  ONE exit: whatever went wrong, the main stream is left ordered after whatever the side streams already got, then the error is reported.
static int run_ops(dmm_plan* p, std::vector<Op>& ops, hipStream_t st, int prof_which = -1, size_t begin = 0, size_t end = 0, bool capturing = false) {
  if (end == 0 || end > ops.size()) end = ops.size();
  ProfilePass prof;
  if (!prof.open(p, prof_which, ops.size())) return fail(DMM_ERR_HIP, "hipEventCreate failed");
  const bool overlap = g_overlap_wgrad && !capturing && prof.production_schedule();
  Lanes lanes{p, st};
  if (const char* missing = overlap ? lanes.open_helpers() : nullptr) return fail(DMM_ERR_HIP, missing);
  const bool mfma = p->desc.use_mfma != 0, batching = g_batch_wgrad != 0, batch_main = g_batch_wgrad == 1;
  WgradBatches batches{p, ops, prof, (overlap && !batch_main) ? lanes.side : st};
  int rc = DMM_OK; std::string why;   // the one error of the call and its message
  auto failed = [&](int code, std::string msg) { rc = code; why = std::move(msg); };
  auto flush_failed = [&](hipError_t e) { failed(DMM_ERR_HIP, std::string("grouped weight-gradient launch: ") + hipGetErrorString(e)); };
  for (size_t i = begin; i < end; ++i) {
    const Op& o = ops[i];
    hipError_t e = hipSuccess;
    const BatchKind bk = batching ? batch_kind(o, mfma) : BATCH_NONE;
    WgradBatches::Offer took = WgradBatches::ALONE;
    if (bk != BATCH_NONE) e = batches.offer(i, o, bk, took);
    if (e == hipSuccess && took == WgradBatches::ALONE && flushes_batches(o)) e = batches.flush_all();
    if (e != hipSuccess) { flush_failed(e); break; }
    hipStream_t lst = st;
    if (!lanes.enter(route(o, overlap, lanes.forked, batch_main), lst)) { failed(DMM_ERR_HIP, "hipEventCreate failed"); break; }
    if (took == WgradBatches::MEMBER) {   // (its launch and its event pair come with the flush)
      if (bk == BATCH_W3 && (e = batches.flush_w3_if_full()) != hipSuccess) { flush_failed(e); break; }
      continue;
    }
    const bool sel = prof.selected(o);
    if (sel) prof.begin(i, lst);
    if (took == WgradBatches::ALONE && (rc = launch_checked(p, o, i, lst, lanes, why)) != DMM_OK) break;
    if (sel) prof.end(i, lst);
    if (lanes.pack_pending && o.leaf == 2) lanes.record_pack_join(lst);
    if (o.signal >= 0 && !capturing) {  // a gradient bucket is final on this stream from here on
      hipEvent_t be = plan_event(p, p->bucket_events, (size_t)o.signal);
      if (be == nullptr) { failed(DMM_ERR_HIP, "hipEventCreate failed"); break; }
      hipEventRecord(be, lst);
    }
  }
  const hipError_t at_end = rc == DMM_OK ? batches.flush_all() : hipSuccess;
  if (at_end != hipSuccess) flush_failed(at_end);
  lanes.join_all();
  return rc == DMM_OK ? DMM_OK : fail(rc, why);
}

// Every bucket event of the list, recorded on `st`: behind a graph replay all buckets are final at once.
static int record_bucket_events(dmm_plan* p, const std::vector<Op>& ops, hipStream_t st) {
  for (const Op& o : ops) {
    if (o.signal < 0) continue;
    hipEvent_t be = plan_event(p, p->bucket_events, (size_t)o.signal);
    if (be == nullptr) return fail(DMM_ERR_HIP, "hipEventCreate failed");
    HIPCHK(hipEventRecord(be, st));
  }
  return DMM_OK;
}

// Runs a whole launch list.  The launches [seg_begin, seg_end) - everything that does not touch a caller pointer - are captured ONCE
// into a hipGraph the second time the list runs (on a plan-owned stream: the caller's may be the legacy default stream, which cannot
// be captured) as ONE chain - the weight gradients are not sent to the side stream - and replayed by one call from then on; the few
// launches in front of and behind the segment (input conversion, the stem convolution up to the join with the weight-packing stream,
// the logits kernel; the loss kernel) take the caller's pointers and stay eager, so the graph never has to be patched or captured
// again.  `which`: 0 training forward, 1 loss + backward.
// Measured on MI355X / ROCm 7.2 (round 3, tools/host_bound.py): a replay enqueues a step in 0.5 ms of host time instead of 14 ms (C1) /
// 25 ms (C2), but the GPU time of a step does not change (C1 18.6 ms, C2 31.7 ms replayed = the same launches eager on one stream):
// the small configurations are bound by the latency of ~700 dependent tiny-grid kernels, not by the host, and the eager
// two-stream schedule is faster than either (C1 16.5 ms, C2 29.5 ms).  A capture of the two-stream schedule (fork / join events
// between the streams) replayed at 37 ms (C1) / 41 ms (C2) and returned different weight gradients than the eager launches, so the
// capture is single-stream.  Hence OFF by default (dmm_set_option("graph", 1) / DMM_GRAPH=1): it frees the host, it does not buy time.
static int launch_list(dmm_plan* p, int which, std::vector<Op>& ops, size_t seg_begin, size_t seg_end, hipStream_t st) {
  dmm_plan::GraphCache& gc = p->graphs[which];
  const bool profiling = p->prof_max_passes > 0 && p->prof_pass[which] < p->prof_max_passes;
  if (gc.epoch != g_option_epoch) {  // an option changed (or the plan was re-bound) since the graph was captured
    if (gc.exec) hipGraphExecDestroy((hipGraphExec_t)gc.exec);
    gc = dmm_plan::GraphCache{nullptr, 0, g_option_epoch};
  }
  const bool want = g_graph && !(g_graph == 2 && which == 1) && !p->graph_failed && !profiling && !(which == 1 && p->dp_used) && seg_end > seg_begin + 8;
  if (!want) return run_ops(p, ops, st, which);
  if (gc.exec == nullptr && gc.nseen > 0) {  // the second run of the list: capture the segment
    DevicePool* dp = pool_of(p->device);
    if (dp == nullptr || pool_streams(dp, true) != hipSuccess) return fail(DMM_ERR_HIP, "capture stream");
    hipStream_t cs = dp->capture;
    p->used_capture = true;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    bool ok = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
      const int rc = run_ops(p, ops, cs, -1, seg_begin, seg_end, true);
      const bool ended = hipStreamEndCapture(cs, &graph) == hipSuccess && graph != nullptr;
      ok = rc == DMM_OK && ended;
      if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
      if (graph) hipGraphDestroy(graph);
    }
    static const bool gtrace = lab_flag("DMM_GRAPH_TRACE");
    if (gtrace) fprintf(stderr, "[dmm] graph capture of list %d, launches [%zu, %zu): %s\n", which, seg_begin, seg_end, ok ? "ok" : "FAILED");
    if (ok) gc.exec = (void*)exec;
    else { (void)hipGetLastError(); p->graph_failed = true; }  // stay eager on this plan
  }
  gc.nseen = 1;
  if (gc.exec == nullptr) return run_ops(p, ops, st, which);
  int rc = seg_begin > 0 ? run_ops(p, ops, st, -1, 0, seg_begin) : DMM_OK;
  if (rc) return rc;
  HIPCHK(hipGraphLaunch((hipGraphExec_t)gc.exec, st));
  p->graph_replays[which]++;
  if (seg_end < ops.size()) { rc = run_ops(p, ops, st, -1, seg_end, ops.size()); if (rc) return rc; }
  return which == 1 ? record_bucket_events(p, ops, st) : DMM_OK;
}

extern "C" {

const char* dmm_last_error(void) { return g_err.c_str(); }
int dmm_version(void) { return 102; }

// The names of enum Impl (dmm_impl_name), and the families dmm_set_option switches with the option name of each (hf, cf and halo
// are not settable).
static const char* const kImplNames[IMPL_COUNT] = {"auto", "generic", "thin", "conv3", "cvp", "halo", "wg3", "wg5", "wgp", "pig", "bw1", "hf", "cf", "wgpw", "cvw"};
static const struct { const char* option; int family; } kFamilyOptions[] = {
    {"thin_logits", IMPL_THIN}, {"conv3", IMPL_CONV3}, {"wg3", IMPL_WG3}, {"wgp", IMPL_WGP},
    {"wg5", IMPL_WG5},          {"cvp", IMPL_CVP},     {"bw1", IMPL_BW1}, {"pig", IMPL_PIG},
};

int dmm_set_option(const char* name, int value) {
  if (!name) return fail(DMM_ERR_INVALID, "null argument");
  ++g_option_epoch;
  if (std::string(name) == "overlap_wgrad") { g_overlap_wgrad = value != 0; return DMM_OK; }
  if (std::string(name) == "graph") { g_graph = value; return DMM_OK; }
  if (std::string(name) == "batch_wgrad") {
    if (value < 0 || value > 2) return fail(DMM_ERR_INVALID, "batch_wgrad must be 0, 1 or 2");
    g_batch_wgrad = value;
    return DMM_OK;
  }
  for (const auto& o : kFamilyOptions)
    if (std::string(name) == o.option) {
      if (value != 0) g_family_off &= ~(1u << o.family);
      else g_family_off |= 1u << o.family;
      return DMM_OK;
    }
  if (std::string(name) == "grad_bucket_mb") {  // applies to plans created afterwards; 0 = one bucket
    if (value < 0) return fail(DMM_ERR_INVALID, "grad_bucket_mb must be >= 0");
    g_bucket_mb = value;
    return DMM_OK;
  }
  return fail(DMM_ERR_INVALID, std::string("unknown option ") + name);
}

int dmm_plan_create(const dmm_model_desc* desc, dmm_plan** out) {
  if (!desc || !out) return fail(DMM_ERR_INVALID, "null argument");
  if (desc->num_blocks < 2 || desc->num_blocks > 8) return fail(DMM_ERR_INVALID, "num_blocks must be in [2, 8]");
  if (desc->dtype != DMM_F32 && desc->dtype != DMM_F16 && desc->dtype != DMM_BF16)
    return fail(DMM_ERR_INVALID, "dtype must be DMM_F32, DMM_F16 or DMM_BF16");
  if (desc->dtype == DMM_BF16 && !desc->use_mfma) return fail(DMM_ERR_INVALID, "DMM_BF16 has no scalar check kernels: use_mfma must be 1");
  if (desc->batch < 1) return fail(DMM_ERR_INVALID, "batch must be >= 1");
  if (!(desc->loss_scale > 0)) return fail(DMM_ERR_INVALID, "loss_scale must be > 0");
  dmm_plan* p = new dmm_plan();
  p->desc = *desc;
  p->sw = PlanSwitches::from_environment();   // the only place a plan's switches are read
  p->bucket_bytes = (size_t)g_bucket_mb << 20;
  p->deny = plan_deny(p);
  try {
    plan_build_tables(p);
  } catch (const std::domain_error& e) {
    delete p;
    return fail(DMM_ERR_SHAPE, e.what());
  } catch (const std::exception& e) {
    delete p;
    return fail(DMM_ERR_INVALID, e.what());
  }
  *out = p;
  return DMM_OK;
}

// Teardown contract (tests/test_host_cpu.py drives it under AddressSanitizer against a fake runtime that counts violations):
//   * every helper stream this plan has launched on is synchronised first - when the call returns nothing the library enqueued
//     outside the caller's own stream still reads the workspace or the arenas, so the caller may free them (what it enqueued on
//     the stream it passed in is the caller's to order, as with any stream-ordered allocator);
//   * no stream is destroyed (they belong to the process pool), events go back to the pool, a graph is destroyed behind its stream's
//     synchronisation; every HIP return code is looked at, the first failure is reported (DMM_ERR_HIP) and the teardown still completes;
//   * destroying NULL is DMM_OK; a handle must not be used after the call, whatever it returned.
int dmm_plan_destroy(dmm_plan* plan) {
  if (!plan) return DMM_OK;
  trace_destroy("begin");
  std::string first_err;
  auto note = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && first_err.empty()) first_err = std::string(what) + ": " + hipGetErrorString(e);
  };
  DevicePool* dp = plan->device >= 0 ? pool_of(plan->device) : nullptr;
  if (dp != nullptr) {
    int cur = -1;
    const bool switched = hipGetDevice(&cur) == hipSuccess && cur != plan->device && hipSetDevice(plan->device) == hipSuccess;
    if (plan->used_side) {
      trace_destroy("synchronise the side stream");
      note(hipStreamSynchronize(dp->side), "hipStreamSynchronize(side stream)");
      trace_destroy("synchronise the pack stream");
      note(hipStreamSynchronize(dp->pack), "hipStreamSynchronize(pack stream)");
    }
    if (plan->used_capture && dp->capture) {
      trace_destroy("synchronise the capture stream");
      note(hipStreamSynchronize(dp->capture), "hipStreamSynchronize(capture stream)");
    }
    trace_destroy("graphs");
    for (auto& gc : plan->graphs)
      if (gc.exec) { note(hipGraphExecDestroy((hipGraphExec_t)gc.exec), "hipGraphExecDestroy"); gc.exec = nullptr; }
    trace_destroy("events back to the pool");
    pool_return(dp, plan->fork_events, false);
    pool_return(dp, plan->join_events, false);
    pool_return(dp, plan->bucket_events, false);
    for (auto& which : plan->prof_events)
      for (auto& pass : which) pool_return(dp, pass, true);
    if (switched) (void)hipSetDevice(cur);
  }
  trace_destroy("delete");
  delete plan;
  trace_destroy("done");
  return first_err.empty() ? DMM_OK : fail(DMM_ERR_HIP, "dmm_plan_destroy: " + first_err);
}

int dmm_plan_num_tensors(const dmm_plan* plan) { return plan ? (int)plan->tensors.size() : 0; }

int dmm_plan_tensor_info(const dmm_plan* plan, int index, const char** name, int32_t* kind, int32_t* ndim, int64_t shape[4],
                         int64_t* arena_offset) {
  if (!plan || index < 0 || index >= (int)plan->tensors.size()) return fail(DMM_ERR_INVALID, "tensor index out of range");
  const TensorInfo& t = plan->tensors[index];
  if (name) *name = t.name.c_str();
  if (kind) *kind = t.kind;
  if (ndim) *ndim = t.ndim;
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
  if (arena_offset) *arena_offset = t.off;
  return DMM_OK;
}

int64_t dmm_plan_num_params(const dmm_plan* plan) { return plan ? plan->nparams : 0; }
int64_t dmm_plan_num_buffer_elems(const dmm_plan* plan) { return plan ? plan->nbuf : 0; }
size_t dmm_plan_workspace_bytes(const dmm_plan* plan) { return plan ? plan->zero_bytes + plan->zero_bwd_bytes + plan->main_bytes : 0; }
double dmm_plan_forward_flops(const dmm_plan* plan) { return plan ? plan->fwd_flops : 0; }

int dmm_plan_bind(dmm_plan* plan, void* workspace, size_t workspace_bytes, float* params, float* grads, float* buffers) {
  if (!plan || !workspace || !params || !grads || !buffers) return fail(DMM_ERR_INVALID, "null argument");
  if (workspace_bytes < dmm_plan_workspace_bytes(plan)) return fail(DMM_ERR_INVALID, "workspace too small");
  if ((uintptr_t)workspace % 256) return fail(DMM_ERR_INVALID, "workspace must be 256-byte aligned");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DMM_ERR_NO_DEVICE, "no HIP device");
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  if (plan->device >= 0 && plan->device != dev) return fail(DMM_ERR_STATE, "the plan is bound to another device");
  if (dev >= MAX_DEVICES) return fail(DMM_ERR_INVALID, "device index out of range");
  plan->device = dev;
  plan->params = params;
  plan->grads = grads;
  plan->buffers = buffers;
  plan->graphs[0].epoch = plan->graphs[1].epoch = 0;  // captured graphs hold the old pointers
  plan->bound = false;
  plan->deny = plan_deny(plan);   // the switches of the moment of bind decide the launches (buffers are reserved by shape alone)
  try {
    plan_bind(plan, workspace);
  } catch (const dmm::plan_sizing_error& e) {
    return fail(DMM_ERR_STATE, e.what());
  } catch (const std::exception& e) {
    return fail(DMM_ERR_INVALID, e.what());
  }
  HIPCHK(hipDeviceSynchronize());
  plan->bound = true;
  return DMM_OK;
}

int dmm_plan_forward(dmm_plan* plan, const float* stream_1, const float* stream_2, float* logits_out, int training, void* stream) {
  if (!plan || !plan->bound) return fail(DMM_ERR_STATE, "plan not bound");
  if (!stream_1 || !logits_out) return fail(DMM_ERR_INVALID, "null argument");
  if (plan->desc.stream_2_in_channels > 0 && !stream_2) return fail(DMM_ERR_INVALID, "stream_2 required");
  std::vector<Op>& ops = training ? plan->fwd_train : plan->fwd_eval;
  for (int idx : (training ? plan->convert_ops_train : plan->convert_ops_eval)) {
    Op& o = ops[idx];
    if (o.epi == 0) { o.cv.src1 = stream_1; o.cv.src2 = nullptr; }
    else if (o.epi == 1) { o.cv.src1 = stream_1; o.cv.src2 = stream_2; }
    else { o.cv.src1 = stream_2; o.cv.src2 = nullptr; }
  }
  ops[training ? plan->logits_op_train : plan->logits_op_eval].c.logits = logits_out;
  if (!training) return run_ops(plan, ops, (hipStream_t)stream, -1);
  // the replayed segment: behind the join with the weight-packing stream (the launches in front of it read the caller's inputs),
  // in front of the logits kernel (which writes the caller's tensor)
  size_t seg_begin = 0;
  for (size_t i = 0; i < ops.size(); ++i) if (ops[i].kind == OP_JOIN) seg_begin = i + 1;
  if (seg_begin == 0) for (int idx : plan->convert_ops_train) seg_begin = std::max(seg_begin, (size_t)idx + 1);
  return launch_list(plan, 0, ops, seg_begin, (size_t)plan->logits_op_train, (hipStream_t)stream);
}

static void set_loss_fields(const dmm_plan* plan, BceArgs& a) {
  a.kind = plan->loss_kind;
  for (int i = 0; i < 8; ++i) { a.alpha[i] = plan->loss_alpha[i]; a.gamma[i] = plan->loss_gamma[i]; }
}

int dmm_plan_set_loss(dmm_plan* plan, int kind, const float* alpha, const float* gamma, int nclass) {
  if (!plan) return fail(DMM_ERR_INVALID, "null plan");
  if (kind != DMM_LOSS_BCE && kind != DMM_LOSS_FOCAL) return fail(DMM_ERR_INVALID, "loss kind must be DMM_LOSS_BCE or DMM_LOSS_FOCAL");
  if (kind == DMM_LOSS_FOCAL) {
    if (!alpha || !gamma || nclass != plan->desc.num_classes) return fail(DMM_ERR_INVALID, "focal loss needs num_classes alpha / gamma values");
    for (int i = 0; i < nclass; ++i) { plan->loss_alpha[i] = alpha[i]; plan->loss_gamma[i] = gamma[i]; }
  }
  plan->loss_kind = kind;
  return DMM_OK;
}

int dmm_loss_forward(int kind, int from_prob, const float* alpha, const float* gamma, const float* input, const float* target,
                     float* loss_out, float* dinput_out, int batch, int nclass, int height, int width, void* stream) {
  if (!input || !target || (!loss_out && !dinput_out)) return fail(DMM_ERR_INVALID, "null argument");
  if (kind != DMM_LOSS_BCE && kind != DMM_LOSS_FOCAL) return fail(DMM_ERR_INVALID, "loss kind must be DMM_LOSS_BCE or DMM_LOSS_FOCAL");
  if (nclass < 1 || nclass > 8 || batch < 1 || height < 1 || width < 1) return fail(DMM_ERR_INVALID, "1..8 classes (dim 1) supported");
  if (kind == DMM_LOSS_FOCAL && (!alpha || !gamma)) return fail(DMM_ERR_INVALID, "focal loss needs alpha / gamma");
  BceArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = input; a.target = target; a.loss_out = loss_out; a.dx_out = dinput_out;
  a.B = batch; a.NC = nclass; a.H = height; a.W = width;
  a.thr = 0.f; a.loss_scale = 1.f; a.kind = kind; a.from_prob = from_prob ? 1 : 0;
  for (int i = 0; i < nclass; ++i) { a.alpha[i] = alpha ? alpha[i] : 1.f; a.gamma[i] = gamma ? gamma[i] : 2.f; }
  HIPCHK(launch_bce_metrics(a, DT_F32, (hipStream_t)stream));
  return DMM_OK;
}

size_t dmm_logit_hist_elems(int B, int NC, int nthr) {
  if (B < 1 || NC < 1 || (long long)B * NC > 65535 || nthr < 1 || nthr > DMM_HIST_MAX_THRESHOLDS) return 0;
  return (size_t)B * NC * 2 * (size_t)(nthr + 1);
}

int dmm_logit_hist(const float* logits, const float* target, int B, int NC, int H, int W, const float* thresholds, int nthr,
                   float gt_threshold, int accumulate, int64_t* counts, void* stream) {
  const std::string who = "dmm_logit_hist: ";
  if (!logits || !target || !thresholds || !counts) return fail(DMM_ERR_INVALID, who + "null argument");
  if ((uintptr_t)logits % 4 || (uintptr_t)target % 4) return fail(DMM_ERR_INVALID, who + "logits / target must be 4-byte aligned");
  if ((uintptr_t)counts % 8) return fail(DMM_ERR_INVALID, who + "counts must be 8-byte aligned");
  if (B < 1 || NC < 1 || H < 1 || W < 1) return fail(DMM_ERR_INVALID, who + "B, NC, H and W must be >= 1");
  if ((long long)B * NC > 65535) return fail(DMM_ERR_INVALID, who + "B * NC must be <= 65535");
  if ((long long)H * W >= (1ll << 31)) return fail(DMM_ERR_INVALID, who + "H * W must be < 2^31");
  if (nthr < 1 || nthr > DMM_HIST_MAX_THRESHOLDS) return fail(DMM_ERR_INVALID, who + "nthr must be in [1, " + std::to_string(DMM_HIST_MAX_THRESHOLDS) + "]");
  for (int k = 0; k < nthr; ++k)
    if (!std::isfinite(thresholds[k])) return fail(DMM_ERR_INVALID, who + "thresholds[" + std::to_string(k) + "] is NaN or infinite");
  for (int k = 1; k < nthr; ++k)
    if (!(thresholds[k] > thresholds[k - 1])) return fail(DMM_ERR_INVALID, who + "thresholds must be strictly ascending (at index " + std::to_string(k) + ")");
  if (std::isnan(gt_threshold)) return fail(DMM_ERR_INVALID, who + "gt_threshold is NaN");
  LogitHistArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.target = target; a.counts = (unsigned long long*)counts;
  a.B = B; a.NC = NC; a.H = H; a.W = W; a.K = nthr; a.gt = gt_threshold;
  for (int k = 0; k < nthr; ++k) a.thr[k] = thresholds[k];
  HIPCHK(launch_logit_hist(a, accumulate, (hipStream_t)stream));
  return DMM_OK;
}

// ---- batch augmentation (augment.hip) and affine warp (warp.hip): two entry points with one set of conventions ----
extern "C++" {   // (templates, inside the file's extern "C" block)
static bool aug_reserved_set(const dmm_aug_tensor& T) { return T.reserved != 0; }
static bool aug_reserved_set(const dmm_warp_tensor& T) { return T.reserved[0] != 0 || T.reserved[1] != 0; }

// What both refuse about sizes and tensors; *nch: the call's channels.  "" = nothing to refuse.
template <class Tensor>
static std::string aug_refuse_tensors(const Tensor* tensors, int ntensors, int B, int Hs, int Ws, int Ho, int Wo, int* nch_out) {
  if (ntensors < 1 || ntensors > DMM_AUG_MAX_TENSORS) return "ntensors must be in [1, " + std::to_string(DMM_AUG_MAX_TENSORS) + "]";
  if (B < 1 || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1) return "B, Hs, Ws, Ho and Wo must be >= 1";
  const long long splane = (long long)Hs * Ws, dplane = (long long)Ho * Wo;
  if (splane >= (1ll << 31)) return "Hs * Ws must be < 2^31";
  if (dplane >= (1ll << 31)) return "Ho * Wo must be < 2^31";
  int nch = 0;
  for (int t = 0; t < ntensors; ++t) {
    const Tensor& T = tensors[t];
    const std::string which = "tensor " + std::to_string(t) + ": ";
    if (!T.src || !T.dst) return which + "null src or dst";
    if ((uintptr_t)T.src % 4 || (uintptr_t)T.dst % 4) return which + "src / dst must be 4-byte aligned";
    if (aug_reserved_set(T)) return which + "reserved must be 0";
    if (T.channels < 1) return which + "channels must be >= 1";
    nch += T.channels;
    if (nch > DMM_AUG_MAX_CHANNELS) return "channels must sum to at most " + std::to_string(DMM_AUG_MAX_CHANNELS);
    if (T.src_batch_stride < T.channels * splane) return which + "src_batch_stride must be >= channels * Hs * Ws";
    // (the byte ranges of the checks below are formed in uintptr_t: a stride that would wrap them is refused here)
    if (T.src_batch_stride > (1ll << 60) / B) return which + "src_batch_stride * B is out of range";
  }
  // dst [dst, dst + B * channels * Ho * Wo) against every src span [src, src + (B - 1) * stride + channels * Hs * Ws) and every other dst
  auto overlaps = [](uintptr_t a, uintptr_t an, uintptr_t b, uintptr_t bn) { return a < b + bn && b < a + an; };
  auto dst_bytes = [&](int t) { return (uintptr_t)B * tensors[t].channels * dplane * 4; };
  for (int t = 0; t < ntensors; ++t)
    for (int u = 0; u < ntensors; ++u) {
      const uintptr_t sn = ((uintptr_t)(B - 1) * tensors[u].src_batch_stride + (uintptr_t)tensors[u].channels * splane) * 4;
      if (overlaps((uintptr_t)tensors[t].dst, dst_bytes(t), (uintptr_t)tensors[u].src, sn))
        return "dst of tensor " + std::to_string(t) + " overlaps src of tensor " + std::to_string(u) + " (in place is not supported)";
    }
  for (int t = 0; t < ntensors; ++t)
    for (int u = t + 1; u < ntensors; ++u)
      if (overlaps((uintptr_t)tensors[t].dst, dst_bytes(t), (uintptr_t)tensors[u].dst, dst_bytes(u)))
        return "dst of tensor " + std::to_string(t) + " overlaps dst of tensor " + std::to_string(u);
  *nch_out = nch;
  return "";
}

// the call's channels and fill into the launch arguments (AugArgs / WarpArgs); "" or what to refuse about fill
template <class Args, class Tensor>
static std::string aug_fill_args(Args& a, const Tensor* tensors, int ntensors, int nch, int Hs, int Ws, int Ho, int Wo, const float* fill) {
  const long long splane = (long long)Hs * Ws, dplane = (long long)Ho * Wo;
  for (int c = 0; c < nch; ++c) {
    a.fill[c] = fill ? fill[c] : 0.f;
    if (!std::isfinite(a.fill[c])) return "fill[" + std::to_string(c) + "] is NaN or infinite";
  }
  for (int t = 0, c = 0; t < ntensors; ++t)
    for (int k = 0; k < tensors[t].channels; ++k, ++c) {
      a.ch[c].src = tensors[t].src + (size_t)k * splane;
      a.ch[c].dst = tensors[t].dst + (size_t)k * dplane;
      a.ch[c].src_stride = tensors[t].src_batch_stride;
      a.ch[c].dst_stride = tensors[t].channels * dplane;
    }
  a.Hs = Hs; a.Ws = Ws; a.Ho = Ho; a.Wo = Wo;
  return "";
}

}  // extern "C++"

int dmm_augment_batch(const dmm_aug_tensor* tensors, int ntensors, const dmm_aug_sample* samples, int B, int Hs, int Ws, int Ho, int Wo,
                      const float* fill, void* stream) {
  const std::string who = "dmm_augment_batch: ";
  if (!tensors || !samples) return fail(DMM_ERR_INVALID, who + "null argument");
  int nch = 0;
  std::string why = aug_refuse_tensors(tensors, ntensors, B, Hs, Ws, Ho, Wo, &nch);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  for (int b = 0; b < B; ++b) {
    const dmm_aug_sample& s = samples[b];
    const std::string which = who + "sample " + std::to_string(b) + ": ";
    if (s.flip != 0 && s.flip != 1) return fail(DMM_ERR_INVALID, which + "flip must be 0 or 1");
    if (s.reserved != 0) return fail(DMM_ERR_INVALID, which + "reserved must be 0");
    if (s.y0 > (1 << 30) || s.y0 < -(1 << 30) || s.x0 > (1 << 30) || s.x0 < -(1 << 30)) return fail(DMM_ERR_INVALID, which + "|y0| and |x0| must be <= 2^30");
    for (int c = 0; c < nch; ++c)
      if (!std::isfinite(s.gain[c]) || !std::isfinite(s.bias[c])) return fail(DMM_ERR_INVALID, which + "gain / bias of channel " + std::to_string(c) + " is NaN or infinite");
  }
  AugArgs a;
  memset(&a, 0, sizeof(a));
  why = aug_fill_args(a, tensors, ntensors, nch, Hs, Ws, Ho, Wo, fill);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  for (int b0 = 0; b0 < B; b0 += DMM_AUG_LAUNCH_BATCH) {
    const int nb = std::min(DMM_AUG_LAUNCH_BATCH, B - b0);
    a.b0 = b0;
    memcpy(a.s, samples + b0, (size_t)nb * sizeof(dmm_aug_sample));
    HIPCHK(launch_augment(a, nch, nb, (hipStream_t)stream));
  }
  return DMM_OK;
}

int dmm_warp_batch(const dmm_warp_tensor* tensors, int ntensors, const dmm_warp_sample* samples, int B, int Hs, int Ws, int Ho, int Wo,
                   const float* fill, void* stream) {
  const std::string who = "dmm_warp_batch: ";
  if (!tensors || !samples) return fail(DMM_ERR_INVALID, who + "null argument");
  int nch = 0;
  std::string why = aug_refuse_tensors(tensors, ntensors, B, Hs, Ws, Ho, Wo, &nch);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  for (int t = 0; t < ntensors; ++t)
    if (tensors[t].mode != DMM_WARP_NEAREST && tensors[t].mode != DMM_WARP_BILINEAR)
      return fail(DMM_ERR_INVALID, who + "tensor " + std::to_string(t) + ": mode must be 0 (nearest) or 1 (bilinear)");
  for (int b = 0; b < B; ++b) {
    const dmm_warp_sample& s = samples[b];
    const std::string which = who + "sample " + std::to_string(b) + ": ";
    // with these bounds SX and SY stay below 2^59 for x, y < 2^31 (derived at the entry point's declaration): nothing wraps
    for (const int32_t v : {s.a00, s.a01, s.a10, s.a11})
      if (v > DMM_WARP_MAX_A || v < -DMM_WARP_MAX_A) return fail(DMM_ERR_INVALID, which + "|a00|, |a01|, |a10| and |a11| must be <= 64 << 20");
    if (s.b0 > DMM_WARP_MAX_B || s.b0 < -DMM_WARP_MAX_B || s.b1 > DMM_WARP_MAX_B || s.b1 < -DMM_WARP_MAX_B)
      return fail(DMM_ERR_INVALID, which + "|b0| and |b1| must be <= 2^50");
    for (int c = 0; c < nch; ++c)
      if (!std::isfinite(s.gain[c]) || !std::isfinite(s.bias[c])) return fail(DMM_ERR_INVALID, which + "gain / bias of channel " + std::to_string(c) + " is NaN or infinite");
  }
  WarpArgs a;
  memset(&a, 0, sizeof(a));
  why = aug_fill_args(a, tensors, ntensors, nch, Hs, Ws, Ho, Wo, fill);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  for (int t = 0, c = 0; t < ntensors; ++t)
    for (int k = 0; k < tensors[t].channels; ++k, ++c) a.mode[c] = tensors[t].mode;
  for (int b0 = 0; b0 < B; b0 += DMM_WARP_LAUNCH_BATCH) {
    const int nb = std::min(DMM_WARP_LAUNCH_BATCH, B - b0);
    a.b0 = b0;
    memcpy(a.s, samples + b0, (size_t)nb * sizeof(dmm_warp_sample));
    HIPCHK(launch_warp(a, nch, nb, (hipStream_t)stream));
  }
  return DMM_OK;
}

// ---- raw frames to training tensors (prepare.hip) ----
// why the three entry points would refuse these sizes ("" = they would not)
static std::string prep_sizes_refusal(int B, int H, int W, int pool) {
  if (B < 1 || H < 1 || W < 1 || pool < 1) return "B, H, W and pool must be >= 1";
  if (H % pool || W % pool) return "H and W must be multiples of pool";
  if ((long long)H * W >= (1ll << 31)) return "H * W must be < 2^31";
  return "";
}

static std::string prep_offsets_refusal(const int32_t* offsets, int B) {
  if (offsets[0] != 0) return "offsets[0] must be 0";
  for (int b = 0; b < B; ++b)
    if (offsets[b + 1] < offsets[b]) return "offsets must not decrease (at index " + std::to_string(b + 1) + ")";
  if (offsets[B] > DMM_PREP_MAX_ITEMS) return "offsets[B] must be <= 2^31 / 256";
  return "";
}

int dmm_prep_image(const uint8_t* src, int64_t src_batch_stride, float* dst, int64_t dst_batch_stride, int B, int H, int W, int C, int pool,
                   void* stream) {
  const std::string who = "dmm_prep_image: ";
  if (!src || !dst) return fail(DMM_ERR_INVALID, who + "null argument");
  if ((uintptr_t)dst % 4) return fail(DMM_ERR_INVALID, who + "dst must be 4-byte aligned");
  const std::string why = prep_sizes_refusal(B, H, W, pool);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  if (C < 1 || C > 4) return fail(DMM_ERR_INVALID, who + "C must be in [1, 4]");
  const int Ho = H / pool, Wo = W / pool;
  if (src_batch_stride < (long long)H * W * C) return fail(DMM_ERR_INVALID, who + "src_batch_stride must be >= H * W * C");
  if (dst_batch_stride < (long long)C * Ho * Wo) return fail(DMM_ERR_INVALID, who + "dst_batch_stride must be >= C * Ho * Wo");
  PrepImageArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src; a.dst = dst; a.src_stride = src_batch_stride; a.dst_stride = dst_batch_stride;
  a.H = H; a.W = W; a.C = C; a.Ho = Ho; a.Wo = Wo; a.p = pool;
  for (int b0 = 0; b0 < B; b0 += DMM_PREP_LAUNCH_BATCH) {
    a.b0 = b0;
    HIPCHK(launch_prep_image(a, std::min(DMM_PREP_LAUNCH_BATCH, B - b0), (hipStream_t)stream));
  }
  return DMM_OK;
}

size_t dmm_prep_lidar_workspace(int B, int H, int W) {
  if (!prep_sizes_refusal(B, H, W, 1).empty()) return 0;
  return ((size_t)B * (size_t)H * (size_t)W * 4 + 15) / 16 * 16;
}

int dmm_prep_lidar(const float* points, const int32_t* offsets, float* dst, int64_t dst_batch_stride, int B, int H, int W, int pool,
                   int kernel_size, void* workspace, size_t workspace_bytes, void* stream) {
  const std::string who = "dmm_prep_lidar: ";
  if (!offsets || !dst || !workspace) return fail(DMM_ERR_INVALID, who + "null argument");
  if ((uintptr_t)points % 4 || (uintptr_t)dst % 4) return fail(DMM_ERR_INVALID, who + "points / dst must be 4-byte aligned");
  if ((uintptr_t)workspace % 16) return fail(DMM_ERR_INVALID, who + "workspace must be 16-byte aligned");
  const std::string why = prep_sizes_refusal(B, H, W, pool);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  if (pool >= 2 && H < 2 * pool) return fail(DMM_ERR_INVALID, who + "H must be >= 2 * pool");
  if (kernel_size < 1 || kernel_size > 15 || kernel_size % 2 == 0) return fail(DMM_ERR_INVALID, who + "kernel_size must be odd and in [1, 15]");
  const int Ho = H / pool, Wo = W / pool;
  if (dst_batch_stride < (long long)Ho * Wo) return fail(DMM_ERR_INVALID, who + "dst_batch_stride must be >= Ho * Wo");
  const std::string bad = prep_offsets_refusal(offsets, B);
  if (!bad.empty()) return fail(DMM_ERR_INVALID, who + bad);
  if (offsets[B] > 0 && !points) return fail(DMM_ERR_INVALID, who + "null points");
  const size_t need = dmm_prep_lidar_workspace(B, H, W);
  if (workspace_bytes < need) return fail(DMM_ERR_INVALID, who + "workspace_bytes is below dmm_prep_lidar_workspace (" + std::to_string(need) + ")");
  PrepLidarArgs a;
  memset(&a, 0, sizeof(a));
  a.points = points; a.owner = (int*)workspace; a.dst = dst; a.dst_stride = dst_batch_stride;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.p = pool; a.k = kernel_size;
  HIPCHK(hipMemsetAsync(workspace, 0xFF, (size_t)B * (size_t)H * (size_t)W * 4, (hipStream_t)stream));   // every owner: -1
  for (int b0 = 0; b0 < B; b0 += DMM_PREP_LAUNCH_BATCH) {
    a.b0 = b0; a.nb = std::min(DMM_PREP_LAUNCH_BATCH, B - b0);
    memcpy(a.off, offsets + b0, (size_t)(a.nb + 1) * sizeof(int32_t));
    HIPCHK(launch_prep_lidar(a, (hipStream_t)stream));
  }
  return DMM_OK;
}

int dmm_prep_heat_maps(const dmm_prep_box* boxes, const int32_t* offsets, float* dst, int64_t dst_batch_stride, int B, int H, int W, int pool,
                       void* stream) {
  const std::string who = "dmm_prep_heat_maps: ";
  if (!offsets || !dst) return fail(DMM_ERR_INVALID, who + "null argument");
  if ((uintptr_t)boxes % 4 || (uintptr_t)dst % 4) return fail(DMM_ERR_INVALID, who + "boxes / dst must be 4-byte aligned");
  const std::string why = prep_sizes_refusal(B, H, W, pool);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  const int Ho = H / pool, Wo = W / pool;
  if (dst_batch_stride < 3ll * Ho * Wo) return fail(DMM_ERR_INVALID, who + "dst_batch_stride must be >= 3 * Ho * Wo");
  const std::string bad = prep_offsets_refusal(offsets, B);
  if (!bad.empty()) return fail(DMM_ERR_INVALID, who + bad);
  if (offsets[B] > 0 && !boxes) return fail(DMM_ERR_INVALID, who + "null boxes");
  PrepHeatArgs a;
  memset(&a, 0, sizeof(a));
  a.boxes = boxes; a.dst = dst; a.dst_stride = dst_batch_stride;
  a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.p = pool;
  for (int b0 = 0; b0 < B; b0 += DMM_PREP_LAUNCH_BATCH) {
    a.b0 = b0; a.nb = std::min(DMM_PREP_LAUNCH_BATCH, B - b0);
    memcpy(a.off, offsets + b0, (size_t)(a.nb + 1) * sizeof(int32_t));
    HIPCHK(launch_prep_heat(a, (hipStream_t)stream));
  }
  return DMM_OK;
}

// why dmm_heat_components would refuse these sizes ("" = it would not); shared with the workspace query
static std::string components_refusal(int B, int NC, int H, int W, int max_per_plane) {
  if (B < 1 || NC < 1 || H < 1 || W < 1) return "B, NC, H and W must be >= 1";
  if ((long long)B * NC > 65535) return "B * NC must be <= 65535";
  if ((long long)H * W >= (1ll << 31)) return "H * W must be < 2^31";
  if (max_per_plane < 1 || max_per_plane > DMM_CC_MAX_PER_PLANE) return "max_per_plane must be in [1, " + std::to_string(DMM_CC_MAX_PER_PLANE) + "]";
  return "";
}

size_t dmm_heat_components_workspace(int B, int NC, int H, int W, int max_per_plane) {
  if (!components_refusal(B, NC, H, W, max_per_plane).empty()) return 0;
  return components_layout(B * NC, (size_t)H * W).total;
}

int dmm_heat_components(const float* maps, int B, int NC, int H, int W, float threshold, int connectivity, int max_per_plane,
                        void* workspace, size_t workspace_bytes, int32_t* labels, dmm_component* records, int32_t* counts, void* stream) {
  const std::string who = "dmm_heat_components: ";
  if (!maps || !workspace || !records || !counts) return fail(DMM_ERR_INVALID, who + "null argument");
  if ((uintptr_t)maps % 4 || (uintptr_t)labels % 4 || (uintptr_t)counts % 4) return fail(DMM_ERR_INVALID, who + "maps / labels / counts must be 4-byte aligned");
  if ((uintptr_t)records % 8) return fail(DMM_ERR_INVALID, who + "records must be 8-byte aligned");
  if ((uintptr_t)workspace % 16) return fail(DMM_ERR_INVALID, who + "workspace must be 16-byte aligned");
  const std::string why = components_refusal(B, NC, H, W, max_per_plane);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  if (connectivity != 4 && connectivity != 8) return fail(DMM_ERR_INVALID, who + "connectivity must be 4 or 8");
  if (std::isnan(threshold)) return fail(DMM_ERR_INVALID, who + "threshold is NaN");
  const ComponentsLayout lay = components_layout(B * NC, (size_t)H * W);
  if (workspace_bytes < lay.total) return fail(DMM_ERR_INVALID, who + "workspace_bytes is below dmm_heat_components_workspace (" + std::to_string(lay.total) + ")");
  ComponentsArgs a;
  memset(&a, 0, sizeof(a));
  a.maps = maps;
  a.labels = labels ? labels : (int*)((char*)workspace + lay.labels);
  a.seg = (int*)((char*)workspace + lay.seg);
  a.records = records; a.counts = counts;
  a.B = B; a.NC = NC; a.H = H; a.W = W;
  a.tiles_x = (W + CC_TILE_W - 1) / CC_TILE_W; a.tiles_y = (H + CC_TILE_H - 1) / CC_TILE_H;
  a.nseg = (int)(((size_t)H * W + CC_SEG - 1) / CC_SEG);
  a.cap = max_per_plane; a.conn8 = connectivity == 8 ? 1 : 0; a.thr = threshold;
  HIPCHK(launch_components(a, (hipStream_t)stream));
  return DMM_OK;
}

// why dmm_match_objects would refuse these sizes ("" = it would not); shared with the workspace query
static std::string match_refusal(int B, int NC, int cap_pred, int cap_gt) {
  if (B < 1 || NC < 1) return "B and NC must be >= 1";
  if ((long long)B * NC > 65535) return "B * NC must be <= 65535";
  if (cap_pred < 1 || cap_pred > DMM_MATCH_MAX_PER_PLANE || cap_gt < 1 || cap_gt > DMM_MATCH_MAX_PER_PLANE)
    return "cap_pred and cap_gt must be in [1, " + std::to_string(DMM_MATCH_MAX_PER_PLANE) + "] (DMM_MATCH_MAX_PER_PLANE: the matcher walks a plane's "
           "predictions serially, it does not take dmm_heat_components' maximum of " + std::to_string(DMM_CC_MAX_PER_PLANE) + ")";
  return "";
}

size_t dmm_match_objects_workspace(int B, int NC, int cap_pred, int cap_gt) {
  if (!match_refusal(B, NC, cap_pred, cap_gt).empty()) return 0;
  return match_layout(B * NC).total;
}

int dmm_match_objects(const dmm_component* pred, const int32_t* pred_counts, int cap_pred, const dmm_component* gt, const int32_t* gt_counts,
                      int cap_gt, int B, int NC, int min_area, double iou, void* workspace, size_t workspace_bytes, uint8_t* matched,
                      int64_t* totals, int32_t* entries, int64_t capacity, void* stream) {
  const std::string who = "dmm_match_objects: ";
  if (!pred || !pred_counts || !gt || !gt_counts || !workspace || !totals || !entries) return fail(DMM_ERR_INVALID, who + "null argument");
  if ((uintptr_t)pred % 8 || (uintptr_t)gt % 8) return fail(DMM_ERR_INVALID, who + "pred / gt records must be 8-byte aligned");
  if ((uintptr_t)pred_counts % 4 || (uintptr_t)gt_counts % 4) return fail(DMM_ERR_INVALID, who + "pred_counts / gt_counts must be 4-byte aligned");
  if ((uintptr_t)totals % 8) return fail(DMM_ERR_INVALID, who + "totals must be 8-byte aligned");
  if ((uintptr_t)entries % 4) return fail(DMM_ERR_INVALID, who + "entries must be 4-byte aligned");
  if ((uintptr_t)workspace % 16) return fail(DMM_ERR_INVALID, who + "workspace must be 16-byte aligned");
  const std::string why = match_refusal(B, NC, cap_pred, cap_gt);
  if (!why.empty()) return fail(DMM_ERR_INVALID, who + why);
  if (min_area < 1) return fail(DMM_ERR_INVALID, who + "min_area must be >= 1");
  if (!(iou > 0.0 && iou <= 1.0)) return fail(DMM_ERR_INVALID, who + "iou must be in (0, 1]");   // (NaN fails both compares)
  if (capacity < 1 || capacity > 2147483647ll) return fail(DMM_ERR_INVALID, who + "capacity must be in [1, 2^31 - 1]");
  const MatchLayout lay = match_layout(B * NC);
  if (workspace_bytes < lay.total) return fail(DMM_ERR_INVALID, who + "workspace_bytes is below dmm_match_objects_workspace (" + std::to_string(lay.total) + ")");
  MatchArgs a;
  memset(&a, 0, sizeof(a));
  a.pred = pred; a.gt = gt; a.pred_counts = pred_counts; a.gt_counts = gt_counts;
  a.np = (int*)((char*)workspace + lay.np); a.ng = (int*)((char*)workspace + lay.ng); a.base = (long long*)((char*)workspace + lay.base);
  a.matched = matched; a.totals = (long long*)totals; a.entries = entries; a.capacity = capacity; a.iou = iou;
  a.B = B; a.NC = NC; a.cap_pred = cap_pred; a.cap_gt = cap_gt; a.min_area = min_area;
  HIPCHK(launch_match(a, (hipStream_t)stream));
  return DMM_OK;
}

int dmm_plan_loss_backward(dmm_plan* plan, const float* logits, const float* target, double* metrics_out, void* stream) {
  if (!plan || !plan->bound) return fail(DMM_ERR_STATE, "plan not bound");
  if (!logits || !target) return fail(DMM_ERR_INVALID, "null argument");
  Op& b = plan->bwd[plan->bce_op];
  b.bce.logits = logits;
  b.bce.target = target;
  set_loss_fields(plan, b.bce);
  b.bce.dyn_scale = plan->dyn_scale;
  // the loss kernel (caller pointers, loss parameters) stays eager; everything behind it is the replayed segment
  int rc = launch_list(plan, 1, plan->bwd, (size_t)plan->bce_op + 1, plan->bwd.size(), (hipStream_t)stream);
  if (rc) return rc;
  if (metrics_out) HIPCHK(hipMemcpyAsync(metrics_out, plan->metrics, plan->metrics_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DMM_OK;
}

int dmm_plan_backward(dmm_plan* plan, const float* dlogits, void* stream) {
  if (!plan || !plan->bound) return fail(DMM_ERR_STATE, "plan not bound");
  if (!dlogits) return fail(DMM_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const BceArgs& b = plan->bwd[plan->bce_op].bce;
  ConvertArgs cv;
  memset(&cv, 0, sizeof(cv));
  cv.src1 = dlogits; cv.C1 = b.NC; cv.dst = b.dlogits; cv.B = b.B; cv.H = b.H; cv.W = b.W;
  cv.scale = plan->desc.loss_scale;
  cv.dyn_scale = plan->dyn_scale;
  // everything the fused path runs in front of the loss kernel (backward accumulators AND, unless gradients accumulate, the
  // gradient arena: unpack adds into it for merged-tap / shared-master weights), then the external d(loss)/d(logit) instead of
  // the loss kernel
  int rc = run_ops(plan, plan->bwd, st, -1, 0, (size_t)plan->bce_op);
  if (rc) return rc;
  HIPCHK(launch_convert_input(cv, plan->desc.dtype, st));
  return run_ops(plan, plan->bwd, st, -1, (size_t)plan->bce_op + 1, 0);
}

int dmm_plan_wgrad_batch_counts(const dmm_plan* plan, long long counts[4]) {
  if (!plan || !counts) return fail(DMM_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; ++i) counts[i] = plan->batch_counts[i];
  return DMM_OK;
}

long long dmm_plan_num_graph_replays(const dmm_plan* plan, int which) {
  return (plan && which >= 0 && which <= 1) ? plan->graph_replays[which] : 0;
}

int dmm_plan_num_grad_buckets(const dmm_plan* plan) { return plan ? (int)plan->buckets.size() : 0; }

int dmm_plan_grad_bucket(const dmm_plan* plan, int index, int64_t* offset, int64_t* count) {
  if (!plan || index < 0 || index >= (int)plan->buckets.size()) return fail(DMM_ERR_INVALID, "bucket index out of range");
  if (offset) *offset = plan->buckets[index].off;
  if (count) *count = plan->buckets[index].n;
  return DMM_OK;
}

int dmm_plan_grad_bucket_wait(dmm_plan* plan, int index, void* stream) {
  if (!plan || index < 0 || index >= (int)plan->buckets.size()) return fail(DMM_ERR_INVALID, "bucket index out of range");
  const GradBucket& b = plan->buckets[index];
  plan->dp_used = true;  // from now on the backward runs eagerly: its bucket events must be recorded where the buckets become final
  for (int ev : {b.ev_main, b.ev_side}) {
    if (ev < 0) continue;
    if (ev >= (int)plan->bucket_events.size()) return fail(DMM_ERR_STATE, "no backward pass has been enqueued on this plan yet");
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)plan->bucket_events[ev], 0));
  }
  return DMM_OK;
}

int dmm_plan_profile_begin(dmm_plan* plan, int max_passes) {
  if (!plan) return fail(DMM_ERR_INVALID, "null plan");
  plan->prof_max_passes = max_passes;
  plan->prof_pass[0] = plan->prof_pass[1] = 0;
  return DMM_OK;
}

int dmm_plan_profile_filter(dmm_plan* plan, const char* label_prefix) {
  if (!plan) return fail(DMM_ERR_INVALID, "null plan");
  plan->prof_filter = label_prefix ? label_prefix : "";
  return DMM_OK;
}

int dmm_plan_profile_num_ops(const dmm_plan* plan, int which) {
  if (!plan || which < 0 || which > 1) return 0;
  return (int)(which == 0 ? plan->fwd_train.size() : plan->bwd.size());
}

int dmm_plan_profile_op(const dmm_plan* plan, int which, int index, const char** label, double* flops, double* bytes) {
  if (!plan || which < 0 || which > 1) return fail(DMM_ERR_INVALID, "bad argument");
  const std::vector<Op>& ops = which == 0 ? plan->fwd_train : plan->bwd;
  if (index < 0 || index >= (int)ops.size()) return fail(DMM_ERR_INVALID, "op index out of range");
  if (label) *label = ops[index].label;
  if (flops) *flops = ops[index].flops;
  if (bytes) *bytes = ops[index].bytes;
  return DMM_OK;
}

// Unit-test entry point (the header's last section): where a storing convolution record of the training forward list leaves its result -
// tests/test_transition_pool_gpu.py compares a layer's output between two plans of one network.
int dmm_plan_record_output(const dmm_plan* plan, int index, int64_t* ws_offset, int32_t* dims /* B, H, W, N, pixel pitch */) {
  if (!plan || !plan->bound || !ws_offset || !dims) return fail(DMM_ERR_INVALID, "bad argument");
  const std::vector<Op>& ops = plan->fwd_train;
  if (index < 0 || index >= (int)ops.size()) return fail(DMM_ERR_INVALID, "op index out of range");
  const Op& o = ops[index];
  if (o.kind != OP_IGEMM || o.epi != EPI_STORE || o.c.out == nullptr) return fail(DMM_ERR_INVALID, "not a storing convolution record");
  *ws_offset = (int64_t)((const uint8_t*)o.c.out - (const uint8_t*)plan->ws);
  dims[0] = o.c.B; dims[1] = o.c.Hout; dims[2] = o.c.Wout; dims[3] = o.c.N; dims[4] = o.c.ldo;
  return DMM_OK;
}

/* Sum of per-op durations (ms) over the recorded passes; the caller must have synchronised the stream. */
int dmm_plan_profile_collect(dmm_plan* plan, int which, double* ms_sum, int n, int* passes) {
  if (!plan || which < 0 || which > 1 || !ms_sum) return fail(DMM_ERR_INVALID, "bad argument");
  const int nops = dmm_plan_profile_num_ops(plan, which);
  if (n < nops) return fail(DMM_ERR_INVALID, "buffer too small");
  for (int i = 0; i < nops; ++i) ms_sum[i] = 0;
  int np = 0;
  for (auto& evs : plan->prof_events[which]) {
    if ((int)evs.size() < 2 * nops || np >= plan->prof_pass[which]) continue;
    const std::vector<Op>& ops = which == 0 ? plan->fwd_train : plan->bwd;
    const std::string& filt = plan->prof_filter;
    for (int i = 0; i < nops; ++i) {
      if (!filt.empty() && strncmp(ops[i].label, filt.c_str(), filt.size()) != 0) continue;
      float ms = 0;
      if (hipEventElapsedTime(&ms, (hipEvent_t)evs[2 * i], (hipEvent_t)evs[2 * i + 1]) != hipSuccess) return fail(DMM_ERR_HIP, "hipEventElapsedTime failed");
      ms_sum[i] += ms;
    }
    ++np;
  }
  if (passes) *passes = np;
  return DMM_OK;
}

int dmm_plan_loss_metrics(dmm_plan* plan, const float* logits, const float* target, double* metrics_out, void* stream) {
  if (!plan || !plan->bound) return fail(DMM_ERR_STATE, "plan not bound");
  if (!logits || !target || !metrics_out) return fail(DMM_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(plan->metrics, 0, plan->metrics_bytes, st));
  Op o = plan->bce_only;
  o.bce.logits = logits;
  o.bce.target = target;
  set_loss_fields(plan, o.bce);
  HIPCHK(launch_bce_metrics(o.bce, plan->desc.dtype, st));
  HIPCHK(hipMemcpyAsync(metrics_out, plan->metrics, plan->metrics_bytes, hipMemcpyDeviceToDevice, st));
  return DMM_OK;
}

int dmm_plan_set_dynamic_loss_scale(dmm_plan* plan, const float* scale_dev) {
  if (!plan) return fail(DMM_ERR_INVALID, "null plan");
  if (((uintptr_t)scale_dev & 3) != 0) return fail(DMM_ERR_INVALID, "dynamic loss scale pointer must be 4-byte aligned");
  plan->dyn_scale = scale_dev;
  // the loss record of a bound plan shows it at once (dmm_plan_loss_backward sets it again at every call: bind rebuilds the list).
  // bce_only (validation: no gradient) never takes it.
  if (plan->bound && plan->bce_op >= 0) plan->bwd[plan->bce_op].bce.dyn_scale = scale_dev;
  return DMM_OK;
}

int dmm_plan_set_grad_accumulate(dmm_plan* plan, int accumulate) {
  if (!plan) return fail(DMM_ERR_INVALID, "null plan");
  const bool on = accumulate != 0;
  if (on == plan->grad_accumulate) return DMM_OK;
  plan->grad_accumulate = on;
  // The arena's memset runs eagerly in front of the loss kernel, but the unpack and BatchNorm-finalize launches sit in the replayed
  // segment with their form baked in: drop the captured backward graph (launch_list destroys the entries of another epoch, as it
  // does behind dmm_set_option and dmm_plan_bind, and captures again when the list has run eagerly once more).  The forward
  // graph writes no gradient and stays.
  plan->graphs[1].epoch = 0;
  return DMM_OK;
}

int dmm_plan_set_encoder_frozen(dmm_plan* plan, int frozen) {
  if (!plan) return fail(DMM_ERR_INVALID, "null plan");
  if (plan->bound) return fail(DMM_ERR_STATE, "dmm_plan_set_encoder_frozen: the plan is bound (set the mode between dmm_plan_create and dmm_plan_bind)");
  const bool on = frozen != 0;
  if (on == plan->encoder_frozen) return DMM_OK;
  // the sizes, buckets and tables must be those of the mode: dmm_plan_bind compares the bytes of its pass with the sized ones exactly
  plan->encoder_frozen = on;
  plan->deny = plan_deny(plan);
  try {
    plan_size(plan);
  } catch (const std::exception& e) {
    plan->encoder_frozen = !on;
    try { plan_size(plan); } catch (...) {}
    return fail(DMM_ERR_INVALID, e.what());
  }
  return DMM_OK;
}

size_t dmm_grad_guard_scratch_bytes(int64_t n) {
  (void)n;  // one partial per workgroup of a fixed grid, whatever the arena's size
  return (size_t)GUARD_PARTIALS * sizeof(double);
}

int dmm_guard_state_init(dmm_guard_state* dev, float init_scale, int64_t applied_steps, int32_t growth_tracker, void* stream) {
  if (!dev) return fail(DMM_ERR_INVALID, "null guard state");
  if (((uintptr_t)dev & 7) != 0) return fail(DMM_ERR_INVALID, "guard state must be 8-byte aligned");
  if (!(init_scale > 0.f) || !std::isfinite(init_scale)) return fail(DMM_ERR_INVALID, "init_scale must be a finite number > 0");
  if (applied_steps < 0 || growth_tracker < 0) return fail(DMM_ERR_INVALID, "applied_steps and growth_tracker must be >= 0");
  HIPCHK(launch_guard_init(dev, init_scale, applied_steps, growth_tracker, (hipStream_t)stream));
  return DMM_OK;
}

int dmm_grad_sumsq(const float* grads, int64_t offset, int64_t count, int accumulate, void* scratch, void* stream) {
  if (!grads || !scratch) return fail(DMM_ERR_INVALID, "null argument");
  if (offset < 0 || count < 0) return fail(DMM_ERR_INVALID, "offset and count must be >= 0");
  if ((((uintptr_t)grads) & 3) != 0 || (((uintptr_t)scratch) & 7) != 0) return fail(DMM_ERR_INVALID, "misaligned gradient or scratch pointer");
  GradSumsqArgs r;
  r.g = grads + offset; r.n = (size_t)count; r.partials = (double*)scratch; r.accumulate = accumulate ? 1 : 0;
  HIPCHK(launch_grad_sumsq(r, (hipStream_t)stream));
  return DMM_OK;
}

// ------------------------------------------------------------------------------------------------ the Adam step: one kernel, four entry points (+ two that keep a parameter average)
namespace {
hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t st);   // (below: complete when it returns)
// What dmm_adam_table_init uploaded to each table_dev: the step calls take a device pointer and cannot read the table back without
// waiting for the device, but the guarded one needs the maximal contiguous runs (one reduction each), and both need to know that
// what they are about to walk was validated.  Entries are replaced by the next init of the same address and never removed (a few
// dozen bytes per table ever made).
struct AdamTableHost {
  int nsegs = 0, nclasses = 0;
  int64_t n = 0;
  std::vector<std::pair<int64_t, int64_t>> runs;   // (begin, count)
};
std::mutex g_adam_tables_mu;
std::vector<std::pair<const void*, AdamTableHost>> g_adam_tables;

size_t adam_table_chunks(int64_t n) { return (size_t)((n + ADAM_SEG_CHUNK - 1) / ADAM_SEG_CHUNK); }

bool bad_scalar(float x) { return std::isnan(x) || x < 0.f; }

// the refusals the two step calls share; on success *host is the record of the table
int adam_seg_check(const char* who, const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq, int64_t n,
                   const void* table_dev, int nsegs, const dmm_adam_class* classes, int nclasses, AdamTableHost* host) {
  const std::string w(who);
  if (!params || !grads || !exp_avg || !exp_avg_sq || !table_dev || !classes) return fail(DMM_ERR_INVALID, w + ": null argument");
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3) != 0 || ((uintptr_t)table_dev & 7) != 0)
    return fail(DMM_ERR_INVALID, w + ": misaligned arena (4 bytes) or table (8 bytes) pointer");
  if (n < 1) return fail(DMM_ERR_INVALID, w + ": n must be >= 1");
  if (nsegs < 1) return fail(DMM_ERR_INVALID, w + ": nsegs must be >= 1");
  if (nclasses < 1 || nclasses > ADAM_MAX_CLASSES)
    return fail(DMM_ERR_INVALID, w + ": nclasses must lie in [1, " + std::to_string(ADAM_MAX_CLASSES) + "]");
  for (int c = 0; c < nclasses; ++c) {
    const dmm_adam_class& k = classes[c];
    const std::string cw = w + ": class " + std::to_string(c) + ": ";
    if (!(k.beta1 >= 0.f && k.beta1 < 1.f) || !(k.beta2 >= 0.f && k.beta2 < 1.f)) return fail(DMM_ERR_INVALID, cw + "betas must lie in [0, 1)");
    if (bad_scalar(k.lr)) return fail(DMM_ERR_INVALID, cw + "lr must be >= 0 and not NaN");
    if (bad_scalar(k.eps)) return fail(DMM_ERR_INVALID, cw + "eps must be >= 0 and not NaN");
    if (bad_scalar(k.weight_decay)) return fail(DMM_ERR_INVALID, cw + "weight_decay must be >= 0 and not NaN");
    if (k.t0 < 0) return fail(DMM_ERR_INVALID, cw + "t0 must be >= 0");
  }
  std::lock_guard<std::mutex> l(g_adam_tables_mu);
  for (const auto& e : g_adam_tables)
    if (e.first == table_dev) {
      if (e.second.nsegs != nsegs || e.second.n != n)
        return fail(DMM_ERR_INVALID, w + ": table_dev was initialised for nsegs = " + std::to_string(e.second.nsegs) + ", n = " + std::to_string(e.second.n));
      if (e.second.nclasses != nclasses)
        return fail(DMM_ERR_INVALID, w + ": table_dev was initialised for nclasses = " + std::to_string(e.second.nclasses));
      *host = e.second;
      return DMM_OK;
    }
  return fail(DMM_ERR_INVALID, w + ": table_dev was not initialised by dmm_adam_table_init");
}

// table_dev == nullptr: the whole-range form, one implicit segment [0, n) of class 0
void adam_seg_args(AdamSegArgs& a, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const void* table_dev,
                   int nsegs, const dmm_adam_class* classes, int nclasses) {
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = (size_t)n;
  a.segs = (const AdamSegDev*)table_dev;
  a.first = table_dev ? (const int*)((const uint8_t*)table_dev + (size_t)nsegs * sizeof(AdamSegDev)) : nullptr;
  a.nsegs = table_dev ? nsegs : 1; a.nchunks = (int)adam_table_chunks(n); a.nclasses = nclasses;
  a.vec_ok = (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 ? 1 : 0;
  a.grad_scale = 0.f; a.state = nullptr;
  a.ema = nullptr; a.ema_omd = 0.f; a.ema_decay = 0.f; a.ema_warmup = 0; a.ema_t0 = 0;
  for (int c = 0; c < ADAM_MAX_CLASSES; ++c) {
    AdamSegClass& k = a.cls[c];
    k = AdamSegClass{};
    k.bc2_sqrt = 1.f;
    if (c >= nclasses) continue;
    const dmm_adam_class& s = classes[c];
    k.lr = s.lr; k.beta1 = s.beta1; k.beta2 = s.beta2; k.eps = s.eps; k.t0 = s.t0;
    k.decoupled = s.decoupled != 0 ? 1 : 0;
    k.weight_decay = k.decoupled ? 0.f : s.weight_decay;
    k.decay = k.decoupled ? (float)(1.0 - (double)s.lr * (double)s.weight_decay) : 1.f;
  }
}

// The refusals of the parameter average, in front of those of the step itself (none needs the table).
int adam_ema_check(const char* who, const dmm_adam_ema* ema, const float* params, const float* grads, const float* exp_avg,
                   const float* exp_avg_sq, int64_t n, bool plain) {
  const std::string w = std::string(who) + ": ";
  if (!ema) return fail(DMM_ERR_INVALID, w + "ema is null");
  if (!ema->ema) return fail(DMM_ERR_INVALID, w + "ema->ema is null");
  if (((uintptr_t)ema->ema & 3) != 0) return fail(DMM_ERR_INVALID, w + "ema->ema is misaligned (4 bytes)");
  const uintptr_t lo = (uintptr_t)ema->ema, bytes = n > 0 ? (uintptr_t)n * sizeof(float) : sizeof(float);
  const std::pair<const char*, const float*> others[4] = {{"params", params}, {"grads", grads}, {"exp_avg", exp_avg}, {"exp_avg_sq", exp_avg_sq}};
  for (const auto& o : others) {
    const uintptr_t b = (uintptr_t)o.second;
    if (o.second && lo < b + bytes && b < lo + bytes) return fail(DMM_ERR_INVALID, w + "ema->ema aliases " + o.first);
  }
  if (!(ema->decay >= 0.f && ema->decay < 1.f)) return fail(DMM_ERR_INVALID, w + "ema->decay must lie in [0, 1)");
  if (plain && ema->k_or_t0 < 1) return fail(DMM_ERR_INVALID, w + "ema->k_or_t0 (the k of this update) must be >= 1");
  return DMM_OK;
}

// d_k of averaging update k >= 1, in double (the guarded kernel's expression)
double adam_ema_decay_at(const dmm_adam_ema& e, int64_t k) {
  double d = (double)e.decay;
  if (e.warmup) {
    const double w = (1.0 + (double)k) / (10.0 + (double)k);
    if (w < d) d = w;
  }
  return d;
}

void adam_ema_args(AdamSegArgs& a, const dmm_adam_ema& e, bool plain) {
  a.ema = e.ema;
  if (((uintptr_t)e.ema & 15) != 0) a.vec_ok = 0;
  a.ema_decay = e.decay; a.ema_warmup = e.warmup != 0 ? 1 : 0;
  if (plain) a.ema_omd = (float)(1.0 - adam_ema_decay_at(e, e.k_or_t0));
  else a.ema_t0 = (long long)e.k_or_t0;
}

// Plain path: every class's step_size and bc2_sqrt at its own step count, step - t0, in double on the host.
hipError_t adam_launch_plain(AdamSegArgs& a, int64_t step, float grad_scale, hipStream_t st) {
  a.grad_scale = grad_scale;
  for (int c = 0; c < a.nclasses; ++c) {
    AdamSegClass& k = a.cls[c];
    const int64_t t = step - k.t0;
    k.active = t >= 1 ? 1 : 0;
    if (!k.active) continue;
    const double bc1 = 1.0 - std::pow((double)k.beta1, (double)t), bc2 = 1.0 - std::pow((double)k.beta2, (double)t);
    k.step_size = (float)(k.lr / bc1);
    k.bc2_sqrt = (float)std::sqrt(bc2);
  }
  return launch_adam_segmented(a, st);
}

// The refusals of the guard's own parameters, shared by the guarded entry points (who: "" or "<entry point>: ").
int guard_check(const std::string& who, const float* grads, const dmm_guard_state* state, const void* scratch, float max_norm,
                float growth_factor, float backoff_factor, int32_t growth_interval) {
  if (!state || !scratch) return fail(DMM_ERR_INVALID, who + "null state or scratch");
  if ((((uintptr_t)grads) & 3) != 0 || (((uintptr_t)state) & 7) != 0 || (((uintptr_t)scratch) & 7) != 0)
    return fail(DMM_ERR_INVALID, who + "misaligned gradient, state or scratch pointer");
  if (!(growth_factor >= 1.f) || !std::isfinite(growth_factor)) return fail(DMM_ERR_INVALID, "growth_factor must be a finite number >= 1");
  if (!(backoff_factor > 0.f) || !(backoff_factor <= 1.f)) return fail(DMM_ERR_INVALID, "backoff_factor must lie in (0, 1]");
  if (growth_interval < 0) return fail(DMM_ERR_INVALID, "growth_interval must be >= 0");
  if (std::isnan(max_norm)) return fail(DMM_ERR_INVALID, "max_norm is NaN");
  return DMM_OK;
}

// Guarded path: the norm over `runs` of the gradient arena (the first run assigns the partials, the rest add), the decision - one for all
// classes; the step_size / bc2_sqrt it leaves in the block are class 0's at t0 = 0 - and the Adam launch, which reads grad_scale, the
// step count and the skip from *state.
hipError_t adam_launch_guarded(AdamSegArgs& a, const std::vector<std::pair<int64_t, int64_t>>& runs, float max_norm, float growth_factor,
                               float backoff_factor, int32_t growth_interval, dmm_guard_state* state, void* scratch, hipStream_t st) {
  for (size_t i = 0; i < runs.size(); ++i) {
    GradSumsqArgs r;
    r.g = a.g + runs[i].first; r.n = (size_t)runs[i].second; r.partials = (double*)scratch; r.accumulate = i > 0 ? 1 : 0;
    if (hipError_t e = launch_grad_sumsq(r, st)) return e;
  }
  GuardFinalizeArgs f;
  f.partials = (const double*)scratch; f.state = state; f.lr = a.cls[0].lr; f.beta1 = a.cls[0].beta1; f.beta2 = a.cls[0].beta2;
  f.max_norm = max_norm; f.growth_factor = growth_factor; f.backoff_factor = backoff_factor; f.growth_interval = growth_interval;
  if (hipError_t e = launch_guard_finalize(f, st)) return e;
  a.state = state;
  return launch_adam_segmented(a, st);
}
}  // namespace

// The two whole-range entry points: one class filled from the scalars, no table.
int dmm_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, float grad_scale, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return fail(DMM_ERR_INVALID, "bad Adam argument");
  const dmm_adam_class one = {lr, beta1, beta2, eps, weight_decay, 0, 0};
  AdamSegArgs a;
  adam_seg_args(a, params, grads, exp_avg, exp_avg_sq, n, nullptr, 1, &one, 1);
  HIPCHK(adam_launch_plain(a, step, grad_scale, (hipStream_t)stream));
  return DMM_OK;
}

int dmm_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                          float beta2, float eps, float weight_decay, float max_norm, float growth_factor, float backoff_factor,
                          int32_t growth_interval, dmm_guard_state* state, void* scratch, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !scratch) return fail(DMM_ERR_INVALID, "null argument of the guarded Adam step");
  if (n < 0) return fail(DMM_ERR_INVALID, "n must be >= 0");
  if (int rc = guard_check("", grads, state, scratch, max_norm, growth_factor, backoff_factor, growth_interval)) return rc;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(DMM_ERR_INVALID, "betas must lie in [0, 1)");
  const dmm_adam_class one = {lr, beta1, beta2, eps, weight_decay, 0, 0};
  AdamSegArgs a;
  adam_seg_args(a, params, grads, exp_avg, exp_avg_sq, n, nullptr, 1, &one, 1);
  HIPCHK(adam_launch_guarded(a, {{0, n}}, max_norm, growth_factor, backoff_factor, growth_interval, state, scratch, (hipStream_t)stream));
  return DMM_OK;
}

size_t dmm_adam_table_bytes(int nsegs, int64_t n) {
  if (nsegs < 1 || n < 1 || n > (int64_t)INT32_MAX * ADAM_SEG_CHUNK) return 0;
  return (size_t)nsegs * sizeof(AdamSegDev) + adam_table_chunks(n) * sizeof(int);
}

int dmm_adam_table_init(void* table_dev, const dmm_adam_segment* segs, int nsegs, int64_t n, int nclasses, void* stream) {
  // every refusal comes before the first HIP call
  if (!table_dev || !segs) return fail(DMM_ERR_INVALID, "dmm_adam_table_init: null argument");
  if (((uintptr_t)table_dev & 7) != 0) return fail(DMM_ERR_INVALID, "dmm_adam_table_init: misaligned table pointer (8 bytes)");
  if (nsegs < 1) return fail(DMM_ERR_INVALID, "dmm_adam_table_init: nsegs must be >= 1");
  if (n < 1 || n > (int64_t)INT32_MAX * ADAM_SEG_CHUNK) return fail(DMM_ERR_INVALID, "dmm_adam_table_init: n must be >= 1 (and below 2^41)");
  if (nclasses < 1 || nclasses > ADAM_MAX_CLASSES)
    return fail(DMM_ERR_INVALID, "dmm_adam_table_init: nclasses must lie in [1, " + std::to_string(ADAM_MAX_CLASSES) + "]");
  for (int i = 0; i < nsegs; ++i) {
    const dmm_adam_segment& s = segs[i];
    const std::string w = "dmm_adam_table_init: segment " + std::to_string(i);
    if (s.count < 1) return fail(DMM_ERR_INVALID, w + ": count must be >= 1");
    if (s.begin < 0 || s.begin >= n || s.count > n - s.begin) return fail(DMM_ERR_INVALID, w + " lies outside [0, n)");
    if (s.cls < 0 || s.cls >= nclasses) return fail(DMM_ERR_INVALID, w + ": cls outside [0, nclasses)");
    if (i > 0 && s.begin < segs[i - 1].begin + segs[i - 1].count)
      return fail(DMM_ERR_INVALID, w + " is unsorted or overlaps segment " + std::to_string(i - 1));
  }
  const size_t nchunks = adam_table_chunks(n), bytes = dmm_adam_table_bytes(nsegs, n);
  std::vector<uint8_t> buf(bytes);
  AdamSegDev* sd = (AdamSegDev*)buf.data();
  int* first = (int*)(buf.data() + (size_t)nsegs * sizeof(AdamSegDev));
  AdamTableHost host;
  host.nsegs = nsegs; host.nclasses = nclasses; host.n = n;
  for (int i = 0; i < nsegs; ++i) {
    sd[i].begin = segs[i].begin; sd[i].end = segs[i].begin + segs[i].count; sd[i].cls = segs[i].cls; sd[i].pad = 0;
    if (!host.runs.empty() && host.runs.back().first + host.runs.back().second == segs[i].begin) host.runs.back().second += segs[i].count;
    else host.runs.emplace_back(segs[i].begin, segs[i].count);
  }
  int s = 0;
  for (size_t ch = 0; ch < nchunks; ++ch) {
    while (s < nsegs && sd[s].end <= (long long)(ch * ADAM_SEG_CHUNK)) ++s;
    first[ch] = s;
  }
  HIPCHK(upload(table_dev, buf.data(), bytes, (hipStream_t)stream));
  std::lock_guard<std::mutex> l(g_adam_tables_mu);
  for (auto& e : g_adam_tables)
    if (e.first == table_dev) { e.second = std::move(host); return DMM_OK; }
  g_adam_tables.emplace_back(table_dev, std::move(host));
  return DMM_OK;
}

int dmm_adam_step_segmented(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const void* table_dev,
                            int nsegs, const dmm_adam_class* classes, int nclasses, int64_t step, float grad_scale, void* stream) {
  if (step < 1) return fail(DMM_ERR_INVALID, "dmm_adam_step_segmented: step must be >= 1");
  AdamTableHost host;
  if (int rc = adam_seg_check("dmm_adam_step_segmented", params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses, &host)) return rc;
  AdamSegArgs a;
  adam_seg_args(a, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses);
  HIPCHK(adam_launch_plain(a, step, grad_scale, (hipStream_t)stream));
  return DMM_OK;
}

int dmm_adam_step_guarded_segmented(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    const void* table_dev, int nsegs, const dmm_adam_class* classes, int nclasses, float max_norm,
                                    float growth_factor, float backoff_factor, int32_t growth_interval, dmm_guard_state* state,
                                    void* scratch, void* stream) {
  const char* who = "dmm_adam_step_guarded_segmented";
  if (int rc = guard_check(std::string(who) + ": ", grads, state, scratch, max_norm, growth_factor, backoff_factor, growth_interval)) return rc;
  AdamTableHost host;
  if (int rc = adam_seg_check(who, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses, &host)) return rc;
  AdamSegArgs a;
  adam_seg_args(a, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses);
  HIPCHK(adam_launch_guarded(a, host.runs, max_norm, growth_factor, backoff_factor, growth_interval, state, scratch, (hipStream_t)stream));   // the norm over the segments only
  return DMM_OK;
}

int dmm_adam_step_segmented_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const void* table_dev,
                                int nsegs, const dmm_adam_class* classes, int nclasses, int64_t step, float grad_scale, void* stream,
                                const dmm_adam_ema* ema) {
  const char* who = "dmm_adam_step_segmented_ema";
  if (int rc = adam_ema_check(who, ema, params, grads, exp_avg, exp_avg_sq, n, true)) return rc;
  if (step < 1) return fail(DMM_ERR_INVALID, std::string(who) + ": step must be >= 1");
  AdamTableHost host;
  if (int rc = adam_seg_check(who, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses, &host)) return rc;
  AdamSegArgs a;
  adam_seg_args(a, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses);
  adam_ema_args(a, *ema, true);
  HIPCHK(adam_launch_plain(a, step, grad_scale, (hipStream_t)stream));
  return DMM_OK;
}

int dmm_adam_step_guarded_segmented_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                        const void* table_dev, int nsegs, const dmm_adam_class* classes, int nclasses, float max_norm,
                                        float growth_factor, float backoff_factor, int32_t growth_interval, dmm_guard_state* state,
                                        void* scratch, void* stream, const dmm_adam_ema* ema) {
  const char* who = "dmm_adam_step_guarded_segmented_ema";
  if (int rc = adam_ema_check(who, ema, params, grads, exp_avg, exp_avg_sq, n, false)) return rc;
  if (int rc = guard_check(std::string(who) + ": ", grads, state, scratch, max_norm, growth_factor, backoff_factor, growth_interval)) return rc;
  AdamTableHost host;
  if (int rc = adam_seg_check(who, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses, &host)) return rc;
  AdamSegArgs a;
  adam_seg_args(a, params, grads, exp_avg, exp_avg_sq, n, table_dev, nsegs, classes, nclasses);
  adam_ema_args(a, *ema, false);
  HIPCHK(adam_launch_guarded(a, host.runs, max_norm, growth_factor, backoff_factor, growth_interval, state, scratch, (hipStream_t)stream));
  return DMM_OK;
}

// ------------------------------------------------------------------------------------------------ single-kernel entry points
namespace {
// Descriptor upload of the single-kernel entry points.  The source is stack / local-vector memory of the call, so the copy must be
// COMPLETE when this returns (an asynchronous copy from pageable memory only happens to be staged at once by the runtime), and what
// the stream still runs may be reading the descriptors the scratch held before.
hipError_t upload(void* dst, const void* src, size_t bytes, hipStream_t st) {
  const hipError_t e = hipStreamSynchronize(st);
  return e != hipSuccess ? e : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}
struct OneConv {
  int esz, SLOT, BK;
  int Ho, Wo, Hout, Wout, ostride, istride;
  std::vector<std::vector<Tap>> phase_taps;
  std::vector<std::pair<int, int>> phase_xy;
  int Cst;  // storage channels of the input
};
int rup(int v, int m) { return (v + m - 1) / m * m; }

bool geometry(const dmm_conv_desc* d, OneConv& g) {
  g.esz = (int)dtype_size(d->dtype);
  g.SLOT = 16 / g.esz;
  g.BK = 4 * g.SLOT;
  g.Cst = d->Cin;
  g.ostride = 1;
  g.istride = 1;
  if (d->Cin % 8 || d->Cout % 8 == 7) return false;
  if (d->transposed) {
    g.Ho = d->H; g.Wo = d->W; g.Hout = 2 * d->H; g.Wout = 2 * d->W; g.ostride = 2;
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) { g.phase_taps.push_back(taps_convT_phase(py, px)); g.phase_xy.push_back({py, px}); }
    return true;
  }
  if (d->mode == 2) { g.Ho = d->H / 2; g.Wo = d->W / 2; g.phase_taps.push_back(taps_conv(1, 1, 0)); }
  else if (d->mode == 1) { g.Ho = 2 * d->H; g.Wo = 2 * d->W; g.phase_taps.push_back(taps_conv(d->R, d->S, d->pad)); }
  else {
    g.Ho = (d->H + 2 * d->pad - d->R) / d->stride + 1;
    g.Wo = (d->W + 2 * d->pad - d->S) / d->stride + 1;
    g.istride = d->stride;
    g.phase_taps.push_back(taps_conv(d->R, d->S, d->pad));
  }
  g.Hout = g.Ho; g.Wout = g.Wo;
  g.phase_xy.push_back({0, 0});
  return true;
}

struct Scratch {
  uint8_t* base;
  size_t off = 0;
  void* take(size_t bytes) {
    off = (off + 255) / 256 * 256;
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};

// builds forward pack descriptors (one per phase); returns bytes used
size_t layout_fwd(const dmm_conv_desc* d, const OneConv& g, uint8_t* scratch, const float* w, float* dw, std::vector<PackDesc>& packs,
                  PackDesc** dev_descs, int** dev_prefix, std::vector<int>& prefix, int& total_rows) {
  Scratch S{scratch};
  *dev_descs = (PackDesc*)S.take(8 * sizeof(PackDesc));
  *dev_prefix = (int*)S.take(8 * sizeof(int));
  total_rows = 0;
  const long long RS = (long long)d->R * d->S;
  for (size_t ph = 0; ph < g.phase_taps.size(); ++ph) {
    PackDesc pd;
    memset(&pd, 0, sizeof(pd));
    pd.w = w; pd.gw = dw;
    pd.N = d->Cout; pd.Npad = rup(d->Cout, 32); pd.nseg = 1;
    if (!d->transposed) { pd.sn = d->Cin * RS; pd.sk = RS; } else { pd.sn = RS; pd.sk = (long long)d->Cout * RS; }
    pd.st = 1;
    fill_pack_seg(pd.seg[0], g.phase_taps[ph], d->Cin, g.Cst, 0, g.BK);
    const size_t elems = (size_t)pd.seg[0].nchunks * pd.Npad * g.BK;
    pd.dst = S.take(elems * g.esz);
    pd.dpack = (float*)S.take(elems * sizeof(float));
    prefix.push_back(total_rows);
    total_rows += pd.seg[0].nchunks * pd.Npad;
    packs.push_back(pd);
  }
  return S.off;
}
}  // namespace

size_t dmm_conv_scratch_bytes(const dmm_conv_desc* d) {
  OneConv g;
  if (!d || !geometry(d, g)) return 0;
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int tr;
  size_t fwd = layout_fwd(d, g, nullptr, nullptr, nullptr, packs, &dd, &dp, prefix, tr);
  // dgrad pack: [chunks][rup(Cin,32)][BK] with K' = R*S*rup(Cout,8)
  const size_t dg = (size_t)((d->R * d->S * rup(d->Cout, 8) + g.BK - 1) / g.BK + 16) * rup(d->Cin, 128) * g.BK * g.esz;
  // + the fp32 dgrad-shaped packed gradient of the transposed-form weight gradient, zero tables, descriptors
  return fwd + dg + 2 * dg + (size_t)rup(d->Cout, 8) * 8 + 8192 + (size_t)W5_SBUF64_FLOATS * sizeof(float);
}

static void fill_one_seg(Seg& s, const dmm_conv_desc* d, const OneConv& g, const void* x, const float* scale, const float* shift,
                         const std::vector<Tap>& taps) {
  memset(&s, 0, sizeof(s));
  s.src = x; s.ld = g.Cst; s.Hs = d->H; s.Ws = d->W; s.C = g.Cst; s.Cpad = g.Cst;
  s.mode = d->transposed ? 0 : d->mode;
  s.istride = g.istride;
  if (d->bn_relu) { s.scale = scale; s.shift = shift; }
  fill_seg_taps(s, taps, g.BK);
}

// the forward launch of phase `ph` (dmm_conv_forward, dmm_conv_forward_merged)
static void fill_fwd_phase(ConvArgs& a, const dmm_conv_desc* d, const OneConv& g, const void* x, const float* scale, const float* shift,
                           void* y, double* stats, const PackDesc& pack, size_t ph) {
  memset(&a, 0, sizeof(a));
  a.nseg = 1;
  fill_one_seg(a.seg[0], d, g, x, scale, shift, g.phase_taps[ph]);
  a.B = d->B; a.Ho = g.Ho; a.Wo = g.Wo; a.M = d->B * g.Ho * g.Wo;
  a.wpack = pack.dst; a.N = d->Cout; a.Npad = pack.Npad;
  a.out = y; a.ldo = d->Cout; a.Hout = g.Hout; a.Wout = g.Wout; a.ostride = g.ostride;
  a.py = g.phase_xy[ph].first; a.px = g.phase_xy[ph].second;
  if (stats) { a.stat_sum = stats; a.stat_sq = stats + d->Cout; }
}

int dmm_last_impl(void) { return g_last_impl; }
unsigned dmm_impl_mask(int reset) { const unsigned m = g_impl_mask; if (reset) g_impl_mask = 0; return m; }
const char* dmm_impl_name(int impl) { return impl >= 0 && impl < IMPL_COUNT ? kImplNames[impl] : "?"; }

int dmm_conv_forward(const dmm_conv_desc* d, const void* x, const float* w, const float* scale, const float* shift, void* y,
                     double* stats, void* scratch, void* stream) {
  OneConv g;
  if (!d || !geometry(d, g)) return fail(DMM_ERR_INVALID, "unsupported conv descriptor");
  hipStream_t st = (hipStream_t)stream;
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int total_rows;
  layout_fwd(d, g, (uint8_t*)scratch, w, nullptr, packs, &dd, &dp, prefix, total_rows);
  HIPCHK(upload(dd, packs.data(), packs.size() * sizeof(PackDesc), st));
  HIPCHK(upload(dp, prefix.data(), prefix.size() * sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(launch_pack(dd, dp, (int)packs.size(), total_rows, d->dtype, st));
  if (stats) HIPCHK(hipMemsetAsync(stats, 0, 2 * d->Cout * sizeof(double), st));
  for (size_t ph = 0; ph < packs.size(); ++ph) {
    ConvArgs a;
    fill_fwd_phase(a, d, g, x, scale, shift, y, stats, packs[ph], ph);
    HIPCHK(launch_igemm(a, d->dtype, EPI_STORE, d->use_mfma != 0, st, IMPL_AUTO, g_family_off));
  }
  return DMM_OK;
}

// The pooling launch a plan puts in front of a transition's 1x1 convolution (plan.cpp emit_transition_pool), on a channel window.
int dmm_avgpool2_bnrelu(int dtype, const void* x, int ld, int B, int H, int W, int C, const float* scale, const float* shift, void* out,
                        int ldo, void* stream) {
  const std::string who = "dmm_avgpool2_bnrelu: ";
  if (!x || !scale || !shift || !out) return fail(DMM_ERR_INVALID, who + "null argument");
  if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_BF16) return fail(DMM_ERR_INVALID, who + "unknown dtype");
  const int slot = dtype == DT_F32 ? 4 : 8;
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || H % 2 || W % 2 || C % slot || ld % slot || ldo % slot || ld < C || ldo < C)
    return fail(DMM_ERR_INVALID, who + "whole 2x2 windows and whole 16-byte channel slots only");
  AvgPool2Args a;
  a.x = x; a.ld = ld; a.H = H; a.W = W; a.B = B; a.C = C;
  a.scale = scale; a.shift = shift;
  a.out = out; a.ldo = ldo;
  HIPCHK(launch_avgpool2_fwd(a, dtype, (hipStream_t)stream));
  return DMM_OK;
}

// A ConvTranspose forward as the plan runs it (plan.cpp emit_conv_fwd): the four per-phase records of dmm_conv_forward, each picked,
// then merged into ONE launch by the plan's own eligibility / copy / accept functions (plan.h) - or, where those keep the phases
// apart, the four launches.  *launches: 1 or 4.
int dmm_conv_forward_merged(const dmm_conv_desc* d, const void* x, const float* w, const float* scale, const float* shift, void* y,
                            double* stats, void* scratch, void* stream, int* launches) {
  const std::string who = "dmm_conv_forward_merged: ";
  if (!d || !x || !w || !y || !scratch || !launches) return fail(DMM_ERR_INVALID, who + "null argument");
  if (!d->transposed) return fail(DMM_ERR_INVALID, who + "the merged launch is a ConvTranspose's (transposed = 1)");
  if (d->bn_relu && (!scale || !shift)) return fail(DMM_ERR_INVALID, who + "bn_relu needs scale and shift");
  OneConv g;
  if (!geometry(d, g) || g.phase_taps.size() != 4) return fail(DMM_ERR_INVALID, who + "unsupported conv descriptor");
  hipStream_t st = (hipStream_t)stream;
  const bool mfma = d->use_mfma != 0;
  const unsigned deny = g_family_off;
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int total_rows;
  layout_fwd(d, g, (uint8_t*)scratch, w, nullptr, packs, &dd, &dp, prefix, total_rows);
  HIPCHK(upload(dd, packs.data(), packs.size() * sizeof(PackDesc), st));
  HIPCHK(upload(dp, prefix.data(), prefix.size() * sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(launch_pack(dd, dp, (int)packs.size(), total_rows, d->dtype, st));
  if (stats) HIPCHK(hipMemsetAsync(stats, 0, 2 * d->Cout * sizeof(double), st));
  ConvArgs a[4];
  int impl[4];
  bool merge = true;
  for (int ph = 0; ph < 4; ++ph) {
    fill_fwd_phase(a[ph], d, g, x, scale, shift, y, stats, packs[ph], ph);
    impl[ph] = igemm_pick(a[ph], d->dtype, EPI_STORE, mfma, deny);
    merge = merge && convT_fwd_phase_eligible(a[ph], EPI_STORE, impl[ph], a[0]);
  }
  ConvArgs m = a[0];
  if (merge) {
    for (int ph = 0; ph < 4; ++ph) copy_convT_fwd_phase(m, a[ph], ph);
    merge = accept_convT_fwd_merged(m, d->dtype, mfma, deny);
  }
  if (merge) {
    HIPCHK(launch_igemm(m, d->dtype, EPI_STORE, mfma, st, IMPL_CVP));
  } else {
    for (int ph = 0; ph < 4; ++ph) HIPCHK(launch_igemm(a[ph], d->dtype, EPI_STORE, mfma, st, impl[ph]));
  }
  *launches = merge ? 1 : 4;
  return DMM_OK;
}

// The logits launch as plan.cpp builds it for dec_out_to_heat_maps.refine1: one plain segment at stride 1 with the full tap table,
// EPI_LOGITS, no statistics, the caller's fp32 NCHW tensor.  Everything the logits epilogues are not built for is refused before the
// runtime is asked anything.
int dmm_conv_logits(const dmm_conv_desc* d, const void* x, const float* w, const float* scale, const float* shift, float* logits,
                    void* scratch, void* stream) {
  const std::string who = "dmm_conv_logits: ";
  if (!d || !x || !w || !logits || !scratch) return fail(DMM_ERR_INVALID, who + "null argument");
  if (d->bn_relu && (!scale || !shift)) return fail(DMM_ERR_INVALID, who + "bn_relu needs scale and shift");
  if (d->transposed || d->mode != 0 || d->stride != 1) return fail(DMM_ERR_INVALID, who + "a logits launch is a plain convolution at stride 1");
  if (d->Cout < 1 || d->Cout > 32) return fail(DMM_ERR_INVALID, who + "the logits epilogues are built for at most 32 output channels");
  OneConv g;
  if (!geometry(d, g) || g.Ho < 1 || g.Wo < 1) return fail(DMM_ERR_INVALID, who + "unsupported conv descriptor");
  hipStream_t st = (hipStream_t)stream;
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int total_rows;
  layout_fwd(d, g, (uint8_t*)scratch, w, nullptr, packs, &dd, &dp, prefix, total_rows);
  HIPCHK(upload(dd, packs.data(), packs.size() * sizeof(PackDesc), st));
  HIPCHK(upload(dp, prefix.data(), prefix.size() * sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(launch_pack(dd, dp, (int)packs.size(), total_rows, d->dtype, st));
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.nseg = 1;
  fill_one_seg(a.seg[0], d, g, x, scale, shift, g.phase_taps[0]);
  a.B = d->B; a.Ho = g.Ho; a.Wo = g.Wo; a.M = d->B * g.Ho * g.Wo;
  a.wpack = packs[0].dst; a.N = d->Cout; a.Npad = packs[0].Npad;
  a.out = nullptr; a.logits = logits; a.ldo = d->Cout; a.Hout = g.Ho; a.Wout = g.Wo; a.ostride = 1;
  HIPCHK(launch_igemm(a, d->dtype, EPI_LOGITS, d->use_mfma != 0, st, IMPL_AUTO, g_family_off));
  return DMM_OK;
}

// dy_eff = dy + q[c] + r[c] * yfwd (the deferred BatchNorm-backward correction of the plan's gradient buffers) when q != NULL
static void set_eff_grad(Seg& s, const void* yfwd, int ldy, const float* q, const float* r, const float* zeros) {
  if (q == nullptr) return;
  s.src2 = yfwd; s.ld2 = ldy; s.q = q; s.r = r; s.ql = zeros; s.rl = zeros;
}

// the normal-form weight-gradient launch of phase `ph` (dmm_conv_wgrad_ex, dmm_conv_wgrad_merged)
static void fill_wgrad_phase(WgradArgs& a, const dmm_conv_desc* d, const OneConv& g, const void* x, const void* dy, const float* scale,
                             const float* shift, const void* yfwd, const float* q, const float* r, const float* zeros, const PackDesc& pack,
                             size_t ph) {
  memset(&a, 0, sizeof(a));
  a.nseg = 1;
  fill_one_seg(a.seg[0], d, g, x, scale, shift, g.phase_taps[ph]);
  a.B = d->B; a.Ho = g.Ho; a.Wo = g.Wo; a.M = d->B * g.Ho * g.Wo;
  a.dy.src = dy; a.dy.ld = d->Cout; a.dy.Hs = g.Hout; a.dy.Ws = g.Wout; a.dy.C = rup(d->Cout, 8); a.dy.Cpad = a.dy.C;
  a.dy.mode = G_PLAIN; a.dy.istride = g.ostride; a.dy.ntaps = 1; a.dy.nchunks = 1;
  a.dy.taps[0] = (short)((g.phase_xy[ph].first & 0xff) | ((g.phase_xy[ph].second & 0xff) << 8));
  set_eff_grad(a.dy, yfwd, d->Cout, q, r, zeros);
  a.N = d->Cout; a.Npad = pack.Npad;
  a.dpack = (float*)pack.dpack;
}

// the dgrad-shaped pack of a convolution: [chunks over (tap, output channel)][Npad input channels][BK]
static PackDesc dgrad_pack_desc(const dmm_conv_desc* d, const OneConv& g, const std::vector<Tap>& taps, const float* w, int npad) {
  PackDesc pd;
  memset(&pd, 0, sizeof(pd));
  const long long RS = (long long)d->R * d->S;
  pd.w = w;
  pd.N = d->Cin; pd.Npad = npad; pd.nseg = 1;
  if (!d->transposed) { pd.sn = RS; pd.sk = d->Cin * RS; } else { pd.sn = (long long)d->Cout * RS; pd.sk = RS; }
  pd.st = 1;
  fill_pack_seg(pd.seg[0], taps, d->Cout, rup(d->Cout, 8), 0, g.BK);
  return pd;
}

// The transposed form of a unit-stride multi-tap convolution's weight gradient (taps on the gradient side: wgrad.hip "transposed
// form", what the plan builds for thin outputs: plan.cpp finish_conv): lays the packed gradient and its descriptor out in `scratch`,
// uploads them and fills the launch `a`.  The result has the shape of the data-gradient pack and is scattered into the master layout
// through that descriptor (dd, dp; `rows` rows).
static int thin_wgrad_setup(const dmm_conv_desc* d, const OneConv& g, const void* x, const void* dy, const float* scale, const float* shift,
                            const void* yfwd, const float* q, const float* r, float* dw, void* scratch, hipStream_t st, WgradArgs& a,
                            PackDesc*& dd, int*& dp, int& rows) {
  const std::vector<Tap> taps = taps_conv_dgrad(d->R, d->S, d->pad);
  const int cs = g.Cst;
  const int npad = rup(cs, cs >= 384 || cs % 128 == 0 ? 128 : (cs >= 64 ? 64 : 32));
  Scratch S{(uint8_t*)scratch};
  dd = (PackDesc*)S.take(sizeof(PackDesc));
  dp = (int*)S.take(sizeof(int));
  float* zeros = (float*)S.take((size_t)rup(d->Cout, 8) * sizeof(float) + 64);
  PackDesc pd = dgrad_pack_desc(d, g, taps, dw, npad);
  const size_t elems = (size_t)pd.seg[0].nchunks * pd.Npad * g.BK;
  pd.dpack = (float*)S.take(elems * sizeof(float));
  pd.gw = dw;
  if (S.off > dmm_conv_scratch_bytes(d)) return fail(DMM_ERR_INVALID, "scratch too small");
  HIPCHK(hipMemsetAsync(scratch, 0, S.off, st));
  int zero = 0;
  HIPCHK(upload(dd, &pd, sizeof(pd), st));
  HIPCHK(upload(dp, &zero, sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  memset(&a, 0, sizeof(a));
  a.nseg = 1;
  Seg& sq = a.seg[0];  // Q: the output gradient under the flipped taps
  sq.src = dy; sq.ld = d->Cout; sq.Hs = g.Hout; sq.Ws = g.Wout; sq.C = rup(d->Cout, 8); sq.Cpad = sq.C; sq.mode = G_PLAIN; sq.istride = 1;
  set_eff_grad(sq, yfwd, d->Cout, q, r, zeros);
  fill_seg_taps(sq, taps, g.BK);
  a.B = d->B; a.Ho = g.Ho; a.Wo = g.Wo; a.M = d->B * g.Ho * g.Wo;
  fill_one_seg(a.dy, d, g, x, scale, shift, taps_conv(1, 1, 0));  // P: the activated input, once
  a.dy.istride = 1;
  a.N = g.Cst; a.Npad = pd.Npad;
  a.dpack = (float*)pd.dpack;
  rows = pd.seg[0].nchunks * pd.Npad;
  return DMM_OK;
}

int dmm_conv_wgrad_ex(const dmm_conv_desc* d, const void* x, const void* dy, const float* scale, const float* shift, const void* yfwd,
                      const float* q, const float* r, int transposed_form, float* dw, void* scratch, void* stream) {
  OneConv g;
  if (!d || !geometry(d, g)) return fail(DMM_ERR_INVALID, "unsupported conv descriptor");
  if ((q != nullptr) != (r != nullptr) || (q != nullptr && yfwd == nullptr)) return fail(DMM_ERR_INVALID, "q, r and yfwd come together");
  hipStream_t st = (hipStream_t)stream;
  const size_t wn = (size_t)d->Cin * d->Cout * d->R * d->S;
  if (transposed_form) {
    // taps on the gradient side (wgrad.hip "transposed form", what the plan builds for thin outputs: plan.cpp finish_conv):
    // the result has the shape of the data-gradient pack and is scattered into the master layout through that descriptor
    if (d->transposed || d->mode != 0 || d->stride != 1 || d->R * d->S <= 1 || !d->bn_relu)
      return fail(DMM_ERR_INVALID, "the transposed form serves unit-stride multi-tap convolutions behind BN+ReLU");
    WgradArgs a;
    PackDesc* dd; int* dp; int rows;
    const int rc = thin_wgrad_setup(d, g, x, dy, scale, shift, yfwd, q, r, dw, scratch, st, a, dd, dp, rows);
    if (rc) return rc;
    void* part = nullptr;
    Resolved wg3;
    const unsigned deny = g_family_off;
    if (d->use_mfma && !((deny >> IMPL_WG3) & 1u) && wg3_resolve(a, d->dtype, wg3)) {  // the plan gives the family its slots; so does this entry point
      HIPCHK(hipMallocAsync(&part, (size_t)W3_MAX_SLOTS * W3_SLOT_FLOATS * sizeof(float), st));
      a.part = (float*)part;
      a.part_slots = W3_MAX_SLOTS;
    }
    const hipError_t e1 = launch_wgrad(a, d->dtype, d->use_mfma != 0, st, IMPL_AUTO, deny);
    if (part != nullptr) hipFreeAsync(part, st);
    HIPCHK(e1);
    HIPCHK(hipMemsetAsync(dw, 0, wn * sizeof(float), st));
    HIPCHK(launch_unpack(dd, dp, 1, rows, d->dtype, 1.0f, st));
    return DMM_OK;
  }
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int total_rows;
  const size_t used = layout_fwd(d, g, (uint8_t*)scratch, dw /*unused as w*/, dw, packs, &dd, &dp, prefix, total_rows);
  Scratch S{(uint8_t*)scratch, used};
  float* zeros = (float*)S.take((size_t)rup(d->Cout, 8) * sizeof(float) + 64);
  if (S.off > dmm_conv_scratch_bytes(d)) return fail(DMM_ERR_INVALID, "scratch too small");
  HIPCHK(hipMemsetAsync(scratch, 0, S.off, st));
  HIPCHK(upload(dd, packs.data(), packs.size() * sizeof(PackDesc), st));
  HIPCHK(upload(dp, prefix.data(), prefix.size() * sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t ph = 0; ph < packs.size(); ++ph) {
    WgradArgs a;
    fill_wgrad_phase(a, d, g, x, dy, scale, shift, yfwd, q, r, zeros, packs[ph], ph);
    HIPCHK(launch_wgrad(a, d->dtype, d->use_mfma != 0, st, IMPL_AUTO, g_family_off));
  }
  HIPCHK(hipMemsetAsync(dw, 0, wn * sizeof(float), st));
  HIPCHK(launch_unpack(dd, dp, (int)packs.size(), total_rows, d->dtype, 1.0f, st));
  return DMM_OK;
}

// A ConvTranspose weight gradient (normal form) as the plan runs it (plan.cpp emit_wgrad_phases): the four per-phase records of
// dmm_conv_wgrad_ex, each picked, then merged into ONE launch by the plan's own eligibility / copy / accept functions (plan.h) - or,
// where those keep the phases apart (the deferred correction: mixed tap counts are wgpw.hip's, which takes the materialised gradient
// only), the four launches.  *launches: 1 or 4.
int dmm_conv_wgrad_merged(const dmm_conv_desc* d, const void* x, const void* dy, const float* scale, const float* shift, const void* yfwd,
                          const float* q, const float* r, float* dw, void* scratch, void* stream, int* launches) {
  const std::string who = "dmm_conv_wgrad_merged: ";
  if (!d || !x || !dy || !dw || !scratch || !launches) return fail(DMM_ERR_INVALID, who + "null argument");
  if (!d->transposed) return fail(DMM_ERR_INVALID, who + "the merged launch is a ConvTranspose's (transposed = 1)");
  if (d->bn_relu && (!scale || !shift)) return fail(DMM_ERR_INVALID, who + "bn_relu needs scale and shift");
  if ((q != nullptr) != (r != nullptr) || (q != nullptr) != (yfwd != nullptr)) return fail(DMM_ERR_INVALID, who + "q, r and yfwd come together");
  OneConv g;
  if (!geometry(d, g) || g.phase_taps.size() != 4) return fail(DMM_ERR_INVALID, who + "unsupported conv descriptor");
  hipStream_t st = (hipStream_t)stream;
  const bool mfma = d->use_mfma != 0;
  const unsigned deny = g_family_off;
  const size_t wn = (size_t)d->Cin * d->Cout * d->R * d->S;
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int total_rows;
  const size_t used = layout_fwd(d, g, (uint8_t*)scratch, dw /*unused as w*/, dw, packs, &dd, &dp, prefix, total_rows);
  Scratch S{(uint8_t*)scratch, used};
  float* zeros = (float*)S.take((size_t)rup(d->Cout, 8) * sizeof(float) + 64);
  if (S.off > dmm_conv_scratch_bytes(d)) return fail(DMM_ERR_INVALID, who + "scratch too small");
  HIPCHK(hipMemsetAsync(scratch, 0, S.off, st));
  HIPCHK(upload(dd, packs.data(), packs.size() * sizeof(PackDesc), st));
  HIPCHK(upload(dp, prefix.data(), prefix.size() * sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  WgradArgs a[4];
  int impl[4];
  bool merge = true;
  for (int ph = 0; ph < 4; ++ph) {
    fill_wgrad_phase(a[ph], d, g, x, dy, scale, shift, yfwd, q, r, zeros, packs[ph], ph);
    impl[ph] = wgrad_pick(a[ph], d->dtype, mfma, deny);
    merge = merge && wgrad_phase_eligible(a[ph], impl[ph], a[0]);
  }
  WgradArgs m = a[0];
  if (merge) {
    for (int ph = 0; ph < 4; ++ph) copy_wgrad_phase(m, a[ph], ph);
    merge = accept_wgrad_merged(m, d->dtype, mfma, deny);
  }
  if (merge) {
    HIPCHK(launch_wgrad(m, d->dtype, mfma, st, IMPL_WGP));
  } else {
    for (int ph = 0; ph < 4; ++ph) HIPCHK(launch_wgrad(a[ph], d->dtype, mfma, st, impl[ph]));
  }
  *launches = merge ? 1 : 4;
  HIPCHK(hipMemsetAsync(dw, 0, wn * sizeof(float), st));
  HIPCHK(launch_unpack(dd, dp, (int)packs.size(), total_rows, d->dtype, 1.0f, st));
  return DMM_OK;
}

int dmm_conv5_wgrad_stats(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale, const float* shift,
                          float* dw, double* red, void* scratch, void* stream) {
  OneConv g;
  if (!d || !geometry(d, g)) return fail(DMM_ERR_INVALID, "unsupported conv descriptor");
  if (d->transposed || d->mode != 0 || d->stride != 1 || d->R != 5 || d->S != 5 || d->pad != 2 || !d->bn_relu || d->Cin != 64 || d->Cout > 4 ||
      d->dtype == DMM_F32 || !d->use_mfma)
    return fail(DMM_ERR_INVALID, "serves the 5x5 convolution of 64 channels onto <= 4 behind BN+ReLU in 16-bit storage");
  hipStream_t st = (hipStream_t)stream;
  const size_t wn = (size_t)d->Cin * d->Cout * 25;
  const std::vector<Tap> taps = taps_conv_dgrad(5, 5, 2);
  Scratch S{(uint8_t*)scratch};
  PackDesc* dd = (PackDesc*)S.take(sizeof(PackDesc));
  int* dp = (int*)S.take(sizeof(int));
  PackDesc pd = dgrad_pack_desc(d, g, taps, dw, 64);
  const size_t elems = (size_t)pd.seg[0].nchunks * pd.Npad * g.BK;
  pd.dpack = (float*)S.take(elems * sizeof(float));
  pd.gw = dw;
  float* sbuf = (float*)S.take((size_t)W5_SBUF64_FLOATS * sizeof(float));
  if (S.off > dmm_conv_scratch_bytes(d)) return fail(DMM_ERR_INVALID, "scratch too small");
  HIPCHK(hipMemsetAsync(scratch, 0, S.off, st));
  HIPCHK(hipMemsetAsync(red, 0, 2 * (size_t)d->Cin * sizeof(double), st));
  int zero = 0;
  HIPCHK(upload(dd, &pd, sizeof(pd), st));
  HIPCHK(upload(dp, &zero, sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  WgradArgs a;
  memset(&a, 0, sizeof(a));
  a.nseg = 1;
  Seg& sq = a.seg[0];  // Q: the output gradient under the flipped taps
  sq.src = dy; sq.ld = d->Cout; sq.Hs = g.Hout; sq.Ws = g.Wout; sq.C = rup(d->Cout, 8); sq.Cpad = sq.C; sq.mode = G_PLAIN; sq.istride = 1;
  fill_seg_taps(sq, taps, g.BK);
  a.B = d->B; a.Ho = g.Ho; a.Wo = g.Wo; a.M = d->B * g.Ho * g.Wo;
  fill_one_seg(a.dy, d, g, x, scale, shift, taps_conv(1, 1, 0));  // P: the input, entered as the two factors of its activation
  a.dy.istride = 1;
  a.N = g.Cst; a.Npad = pd.Npad;
  a.dpack = (float*)pd.dpack;
  a.sbuf = sbuf;
  a.t_mean = shift + d->Cin; a.t_invstd = shift + 2 * d->Cin;
  HIPCHK(launch_wgrad(a, d->dtype, true, st, IMPL_AUTO, g_family_off));
  if (g_last_impl != IMPL_WG5) return fail(DMM_ERR_STATE, "the factor form is wg5.hip's");
  Fin64Args f;
  memset(&f, 0, sizeof(f));
  f.sbuf = sbuf; f.dpack = a.dpack; f.Npad = a.Npad;
  f.w = w; f.Kin = d->Cin; f.nreal = d->Cout; f.dtype = d->dtype;
  for (int t = 0; t < 25; ++t) f.tapw[t] = (unsigned char)(pd.seg[0].tapw[t] & 0xff);
  f.scale = scale; f.shift = shift; f.mean = shift + d->Cin; f.invstd = shift + 2 * d->Cin;
  f.red1 = red; f.red2 = red + d->Cin;
  HIPCHK(launch_wg5_fin64(f, st));
  HIPCHK(hipMemsetAsync(dw, 0, wn * sizeof(float), st));
  HIPCHK(launch_unpack(dd, dp, 1, pd.seg[0].nchunks * pd.Npad, d->dtype, 1.0f, st));
  return DMM_OK;
}

int dmm_conv_wgrad(const dmm_conv_desc* d, const void* x, const void* dy, const float* scale, const float* shift, float* dw, void* scratch,
                   void* stream) {
  return dmm_conv_wgrad_ex(d, x, dy, scale, shift, nullptr, nullptr, nullptr, 0, dw, scratch, stream);
}

// Fills the data-gradient launch of one convolution (EPI_BNBWD) and packs its weights; shared by dmm_conv_dgrad_ex and
// dmm_conv1x1_backward_fused.
static int build_dgrad(const dmm_conv_desc* d, const OneConv& g, const void* x, const void* dy, const float* w, const float* scale,
                       const float* shift, const void* yfwd, const float* q, const float* r, void* gx, int accumulate, double* red,
                       Scratch& S, int npad, ConvArgs& a, hipStream_t st) {
  std::vector<Tap> taps;
  int istride = 1, rH = d->H, rW = d->W, pool2 = 0, ostride = 1;
  if (d->transposed) { taps = taps_convT_dgrad(); istride = 2; }
  else if (d->mode == 2) { taps = taps_conv(1, 1, 0); rH = d->H / 2; rW = d->W / 2; pool2 = 1; ostride = 2; }
  else if (d->mode == 1) { taps = taps_up2_merged_dgrad(); istride = 2; }
  else taps = taps_conv_dgrad(d->R, d->S, d->pad);
  PackDesc* dd = (PackDesc*)S.take(sizeof(PackDesc));
  int* dp = (int*)S.take(sizeof(int));
  float* zeros = (float*)S.take((size_t)rup(d->Cout, 8) * sizeof(float) + 64);
  PackDesc pd = dgrad_pack_desc(d, g, taps, w, npad);
  pd.dst = S.take((size_t)pd.seg[0].nchunks * pd.Npad * g.BK * g.esz);
  if (S.off > dmm_conv_scratch_bytes(d)) return fail(DMM_ERR_INVALID, "scratch too small");
  int zero = 0;
  HIPCHK(hipMemsetAsync(zeros, 0, (size_t)rup(d->Cout, 8) * sizeof(float) + 64, st));
  HIPCHK(upload(dd, &pd, sizeof(pd), st));
  HIPCHK(upload(dp, &zero, sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(launch_pack(dd, dp, 1, pd.seg[0].nchunks * pd.Npad, d->dtype, st));
  HIPCHK(hipMemsetAsync(red, 0, 2 * d->Cin * sizeof(double), st));
  memset(&a, 0, sizeof(a));
  a.nseg = 1;
  Seg& s = a.seg[0];
  const int kc = rup(d->Cout, 8);
  s.src = dy; s.ld = d->Cout; s.Hs = g.Hout; s.Ws = g.Wout; s.C = kc; s.Cpad = kc; s.mode = G_PLAIN; s.istride = istride;
  set_eff_grad(s, yfwd, d->Cout, q, r, zeros);
  fill_seg_taps(s, taps, g.BK);
  a.B = d->B; a.Ho = rH; a.Wo = rW; a.M = d->B * rH * rW;
  a.wpack = pd.dst; a.N = d->Cin; a.Npad = pd.Npad;
  a.out = gx; a.ldo = d->Cin; a.Hout = d->H; a.Wout = d->W; a.ostride = ostride;
  a.bx = x; a.ldbx = d->Cin; a.bscale = scale; a.bshift = shift;
  a.bmean = shift + d->Cin; a.binvstd = shift + 2 * d->Cin;  // test entry point: mean / invstd follow `shift`
  a.red1 = red; a.red2 = red + d->Cin;
  a.accumulate = accumulate ? 1 : 0; a.pool2 = pool2;
  return DMM_OK;
}

int dmm_conv_dgrad_ex(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale, const float* shift,
                      const void* yfwd, const float* q, const float* r, void* gx, int accumulate, double* red, void* scratch,
                      void* stream) {
  OneConv g;
  if (!d || !geometry(d, g) || !d->bn_relu) return fail(DMM_ERR_INVALID, "unsupported conv descriptor (dgrad needs bn_relu)");
  if (d->mode == 0 && !d->transposed && d->stride != 1) return fail(DMM_ERR_INVALID, "strided conv dgrad is not on the hot path");
  if ((q != nullptr) != (r != nullptr) || (q != nullptr && yfwd == nullptr)) return fail(DMM_ERR_INVALID, "q, r and yfwd come together");
  hipStream_t st = (hipStream_t)stream;
  Scratch S{(uint8_t*)scratch};
  ConvArgs a;
  // column tile of the plan (plan.cpp add_pack): 128 once the padding waste is <= 25 %, else 64, else 32
  const int cs = g.Cst;
  const int npad = rup(cs, cs >= 384 || cs % 128 == 0 ? 128 : (cs >= 64 ? 64 : 32));
  const int rc = build_dgrad(d, g, x, dy, w, scale, shift, yfwd, q, r, gx, accumulate, red, S, npad, a, st);
  if (rc) return rc;
  HIPCHK(launch_igemm(a, d->dtype, EPI_BNBWD, d->use_mfma != 0, st, IMPL_AUTO, g_family_off));
  return DMM_OK;
}

int dmm_conv_dgrad(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale, const float* shift, void* gx,
                   double* red, void* scratch, void* stream) {
  return dmm_conv_dgrad_ex(d, x, dy, w, scale, shift, nullptr, nullptr, nullptr, gx, 0, red, scratch, stream);
}

int dmm_conv1x1_backward_fused(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale,
                               const float* shift, const void* yfwd, const float* q, const float* r, void* gx, int accumulate,
                               float* dw, double* red, void* scratch, void* stream) {
  OneConv g;
  if (!d || !geometry(d, g) || !d->bn_relu || d->R != 1 || d->S != 1 || d->stride != 1 || d->transposed || d->mode != 0)
    return fail(DMM_ERR_INVALID, "the fused backward serves 1x1 unit-stride convolutions behind BN+ReLU");
  if ((q != nullptr) != (r != nullptr) || (q != nullptr && yfwd == nullptr)) return fail(DMM_ERR_INVALID, "q, r and yfwd come together");
  hipStream_t st = (hipStream_t)stream;
  // forward-shaped packed gradient first (its descriptor scatters dW into the master layout), then the data-gradient launch
  std::vector<PackDesc> packs;
  std::vector<int> prefix;
  PackDesc* dd; int* dp; int total_rows;
  const size_t used = layout_fwd(d, g, (uint8_t*)scratch, dw, dw, packs, &dd, &dp, prefix, total_rows);
  HIPCHK(hipMemsetAsync(scratch, 0, used, st));
  HIPCHK(upload(dd, packs.data(), packs.size() * sizeof(PackDesc), st));
  HIPCHK(upload(dp, prefix.data(), prefix.size() * sizeof(int), st));
  Scratch S{(uint8_t*)scratch, used};
  Bw1Args b;
  memset(&b, 0, sizeof(b));
  const int cs = g.Cst;
  const int npad = rup(cs, cs >= 384 || cs % 128 == 0 ? 128 : (cs >= 64 ? 64 : 32));
  const int rc = build_dgrad(d, g, x, dy, w, scale, shift, yfwd, q, r, gx, accumulate, red, S, npad, b.c, st);
  if (rc) return rc;
  WgradArgs wa;  // the weight-gradient launch the plan would have emitted: only to test the pair's eligibility
  memset(&wa, 0, sizeof(wa));
  wa.nseg = 1;
  fill_one_seg(wa.seg[0], d, g, x, scale, shift, g.phase_taps[0]);
  wa.B = d->B; wa.Ho = g.Ho; wa.Wo = g.Wo; wa.M = d->B * g.Ho * g.Wo;
  wa.dy = b.c.seg[0];
  wa.N = d->Cout; wa.Npad = packs[0].Npad;
  wa.dpack = (float*)packs[0].dpack;
  if (!bw1_eligible(wa, b.c, d->dtype, g_family_off)) return fail(DMM_ERR_INVALID, "not a pair bw1.hip fuses (16-bit storage, 128 output channels, Cin % 32 == 0)");
  b.dpack = wa.dpack; b.dNpad = wa.Npad; b.wC = wa.seg[0].C;
  {  // the production form: per-workgroup slots + the reduction launch (stream-ordered scratch of this call)
    const Bw1Geom q = bw1_geometry(b.c);
    b.part_slots = q.nsplit * q.nct;
    void* part = nullptr;
    HIPCHK(hipMallocAsync(&part, (size_t)b.part_slots * B1_SLOT_FLOATS * sizeof(float), st));
    b.part = (float*)part;
    const hipError_t e1 = launch_bw1(b, d->dtype, st);
    const hipError_t e2 = e1 == hipSuccess ? launch_bw1_reduce(b, st) : e1;
    hipFreeAsync(part, st);
    HIPCHK(e2);
  }
  const size_t wn = (size_t)d->Cin * d->Cout;
  HIPCHK(hipMemsetAsync(dw, 0, wn * sizeof(float), st));
  HIPCHK(launch_unpack(dd, dp, (int)packs.size(), total_rows, d->dtype, 1.0f, st));
  return DMM_OK;
}

int dmm_conv_wgrad_grouped(const dmm_conv_desc* descs, int n, const void* const* x, const void* const* dy, const float* const* scale,
                           const float* const* shift, const void* const* yfwd, const float* const* q, const float* const* r,
                           float* const* dw, void* const* scratch, int grouped, int* launches, void* stream) {
  if (!descs || n < 1 || !x || !dy || !scale || !shift || !dw || !scratch) return fail(DMM_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  struct One { WgradArgs a; PackDesc* dd; int* dp; int rows; };
  std::vector<One> v((size_t)n);
  for (int i = 0; i < n; ++i) {
    const dmm_conv_desc* d = &descs[i];
    OneConv g;
    if (!geometry(d, g)) return fail(DMM_ERR_INVALID, "unsupported conv descriptor");
    const void* yf = yfwd ? yfwd[i] : nullptr;
    const float *qi = q ? q[i] : nullptr, *ri = r ? r[i] : nullptr;
    if ((qi != nullptr) != (ri != nullptr) || (qi != nullptr && yf == nullptr)) return fail(DMM_ERR_INVALID, "q, r and yfwd come together");
    if (d->transposed || d->mode != 0 || d->stride != 1 || d->R * d->S <= 1 || !d->bn_relu || !d->use_mfma)
      return fail(DMM_ERR_INVALID, "the transposed form serves unit-stride multi-tap convolutions behind BN+ReLU");
    const int rc = thin_wgrad_setup(d, g, x[i], dy[i], scale[i], shift[i], yf, qi, ri, dw[i], scratch[i], st, v[i].a, v[i].dd, v[i].dp, v[i].rows);
    if (rc) return rc;
    Resolved res;
    if (!wg3_resolve(v[i].a, d->dtype, res)) return fail(DMM_ERR_INVALID, "not a launch wg3.hip takes (16-bit storage, 128 -> 32 channels, 3x3)");
  }
  void* part = nullptr;   // one slot buffer for all of them, as in a plan
  HIPCHK(hipMallocAsync(&part, (size_t)W3_MAX_SLOTS * W3_SLOT_FLOATS * sizeof(float), st));
  for (One& o : v) { o.a.part = (float*)part; o.a.part_slots = W3_MAX_SLOTS; }
  hipError_t e = hipSuccess;
  int nl = 0;
  if (grouped) {
    Wg3Group G;
    for (int i = 0; i < n && e == hipSuccess; ++i) {
      if (wg3_group_add(G, v[i].a, descs[i].dtype)) continue;
      if (G.n > 0) { e = wg3_group_launch(G, st); ++nl; }
      if (e == hipSuccess && !wg3_group_add(G, v[i].a, descs[i].dtype)) e = hipErrorNotSupported;
    }
    if (e == hipSuccess && G.n > 0) { e = wg3_group_launch(G, st); ++nl; }
    if (e == hipSuccess) note_impl(IMPL_WG3);
  } else {
    for (int i = 0; i < n && e == hipSuccess; ++i, ++nl) e = launch_wgrad(v[i].a, descs[i].dtype, true, st, IMPL_WG3);
  }
  hipFreeAsync(part, st);
  HIPCHK(e);
  for (int i = 0; i < n; ++i) {
    const dmm_conv_desc* d = &descs[i];
    HIPCHK(hipMemsetAsync(dw[i], 0, (size_t)d->Cin * d->Cout * d->R * d->S * sizeof(float), st));
    HIPCHK(launch_unpack(v[i].dd, v[i].dp, 1, v[i].rows, d->dtype, 1.0f, st));
  }
  if (launches) *launches = nl;
  return DMM_OK;
}

int dmm_bw1_reduce_grouped(int n, const float* const* part, float* const* dpack, const int* nct, const int* nsplit, const int* wc,
                           int grouped, int* launches, void* stream) {
  if (n < 1 || !part || !dpack || !nct || !nsplit || !wc) return fail(DMM_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  Bw1RedGroup G;
  int nl = 0;
  for (int i = 0; i < n; ++i) {
    if (!part[i] || !dpack[i] || nct[i] < 1 || nsplit[i] < 1 || wc[i] < 1 || wc[i] > nct[i] * 128 || wc[i] <= (nct[i] - 1) * 128)
      return fail(DMM_ERR_INVALID, "a member needs slots, a packed gradient, nct, nsplit >= 1 and (nct - 1) * 128 < wc <= nct * 128");
    Bw1RedMember m;
    m.part = part[i]; m.dpack = dpack[i]; m.nct = nct[i]; m.nsplit = nsplit[i];
    m.nfloats = ((wc[i] + 31) / 32) * 128 * 32;
    if (!grouped) { HIPCHK(launch_bw1_reduce_member(m, st)); ++nl; continue; }
    if (G.n >= B1_RED_GROUP_MAX) { HIPCHK(bw1_reduce_group_launch(G, st)); ++nl; }
    G.m[G.n++] = m;
  }
  if (G.n > 0) { HIPCHK(bw1_reduce_group_launch(G, st)); ++nl; }
  if (launches) *launches = nl;
  return DMM_OK;
}

}  // extern "C"
