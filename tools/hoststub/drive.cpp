// Drives the HOST code of libdmmfods_hip.so (plan.cpp, capi.cpp and the launchers of every kernel file, built for the host with
// AddressSanitizer + UBSan against tools/hoststub/fake_hip.cpp) through the life of a plan:
//   create -> bind (workspace = host memory) -> training forward x2 -> loss + backward -> backward from an external gradient ->
//   eval forward -> loss metrics -> a profiled pass -> bucket waits -> destroy
// and checks what a GPU cannot show:  (a) host heap errors in the sizing and the bound pass (ASan), (b) every device pointer of
// every launch record lies inside the workspace or one of the caller's arenas, (c) the bound pass takes exactly the bytes the sizing
// pass reported, (d) the teardown contract: no stream or event is destroyed with unsynchronised work behind it, nothing is destroyed
// twice, and every stream / event made for a plan is either back in the process pool or destroyed when the plan is gone.
// Test infrastructure (tests/test_host_cpu.py runs it); environment switches (DMM_NO_PACK_TILES, ...) come from the caller's environment.
//
//   drive <arch> <dtype> <batch> <H> <W> [repeat]
//   arch: d121e d121m d169m d201m d121n tiny_mid tiny_early tiny_no g8_mid     dtype: f32 f16 bf16
// Three more modes check the kernel-family bookkeeping (Op::impl, dmm_last_impl) where no GPU test reaches - operands of 4 GiB and
// more cost only address space here:
//   drive picks <arch> <dtype> <batch> <H> <W>     every convolution launch of a bound plan, re-run through its launcher: the family
//                                                  that takes it must be the one the plan recorded (workspace: reserved, never touched)
//   drive single <fwd|logits|wgrad|dgrad|fused> <dtype> <B> <H> <W> <Cin> <Cout> <R> <pad> <transposed> <mode> [flags]
//                                                  flags (entry `logits`), comma-separated: thinoff, scalar, stride2, nullx, nullw, nulllogits, nullscratch
//                                                  one call of a single-kernel entry point on operands that are addresses only
//   drive refuse                                   launch_wgrad(..., IMPL_GENERIC) on arguments the generic kernel does not implement
// And one prints what a plan IS, so that two builds of the plan builder can be compared byte for byte without a GPU:
//   drive dump <arch> <dtype> <batch> <H> <W>      a bound plan (workspace reserved, never touched; nothing launched) as canonical text:
//                                                  sizes, every field of every launch record, pack / unpack tables, buckets.  Pointers
//                                                  are printed as region+offset, so the text does not depend on where anything is mapped
//                                                  (DRIVE_MAP_SHIFT_MIB=<n> moves the workspace and the three arenas, to show that).
// And one drives gradient accumulation (dmm_plan_set_grad_accumulate) on one plan:
//   drive accum <arch> <dtype> <batch> <H> <W>     create -> mode on (unbound) -> bind -> two training passes without a clear in between
//                                                  -> mode off -> one more pass -> mode on -> external-gradient backward -> destroy.
//                                                  Kernels do not run here but the runtime's memsets do: the gradient arena, filled with
//                                                  a pattern, must keep it while the mode is on and read as zero behind a pass with it off;
//                                                  both modes make the same launches from the same records.
// And one walks a hand-made table of launch records through the executor's pure predicates (plan.h: side_forks, batch_kind,
// flushes_batches, route) and prints what each answers:
//   drive route                                    one line per record and combination of mode flags (tests/test_enqueue_trace_cpu.py)
// DRIVE_TRACE_ENQUEUE=1 (any mode): every enqueue call the fake runtime's hook reports goes to stdout as one line -
//   T launch <kernel> <gx> <gy> s<k> | T record e<j> s<k> | T wait e<j> s<k> | T memset <bytes> s<k> | T memcpy <bytes> s<k>
// with streams and events numbered in the order they first appear (s0: the null stream), and a library call that fails as
// `T error <code> <message>`.  The lines of a run ARE its schedule: two builds of the executor are compared by their hash.
// DRIVE_OPTIONS_OFF=<name>[,<name>...] (any mode): dmm_set_option(name, 0) for each, before any plan is created.
// DRIVE_NO_MFMA=1 (any mode): the description asks for use_mfma = 0.
// DRIVE_DYN_SCALE=1 (life-cycle run and dump): the plan gets a dynamic loss scale (dmm_plan_set_dynamic_loss_scale, pointing into a
// guard state block the driver owns: region "guard"); the life-cycle run also takes the guarded optimiser step after every backward.
// DRIVE_FREEZE=1 (life-cycle run and dump): the plan is built with a frozen encoder (dmm_plan_set_encoder_frozen on the unbound plan; a
// null plan and the bound plan must be refused); the life-cycle run also takes the guarded step over two trainable ranges, one of
// them released late (dmm_adam_step_guarded_segmented, a class with t0 > 0), and checks that no bucket and no unpack descriptor touches an encoder tensor.
// DRIVE_EMA=1 (with DRIVE_FREEZE=1): behind each of those steps the two steps that keep a parameter average (dmm_adam_step_segmented_ema,
// dmm_adam_step_guarded_segmented_ema) run under the same table - a gap in front, then a class with t0 > 0 - and each of their own
// refusals is tried on both: a null struct, a null average, one that is or overlaps an arena, a decay of 1, below 0, above 1 and NaN, k < 1.
// DRIVE_HIST=1 (life-cycle run): behind the lives, dmm_logit_hist on three shapes with operands that are addresses only - the memset and
// the launch geometry of both accumulate modes - and every refusal of the entry point, each with nothing enqueued (hist_main).
// DRIVE_AUGMENT=1 (life-cycle run): behind the lives (and DRIVE_HIST's calls), one valid dmm_augment_batch call with 33 samples on operands
// that are addresses only - two launches - and every refusal of the entry point, each with nothing enqueued (augment_main).
// DRIVE_WARP=1 (life-cycle run): the same for dmm_warp_batch, behind DRIVE_AUGMENT's calls (warp_main).
// DRIVE_COMPONENTS=1 (life-cycle run): behind the lives (and the calls of the two switches above), dmm_heat_components on three shapes with
// operands that are addresses only - seven launches each, every grid against a restatement of the tiling, the workspace carve-up inside
// workspace_bytes - and every refusal of the entry point, each with nothing enqueued (components_main).
// DRIVE_PREPARE=1 (life-cycle run): behind the lives (and the calls of the three switches above), dmm_prep_image, dmm_prep_lidar and
// dmm_prep_heat_maps on B = 1, 33 and 65 samples at pool 10 and 1 - the launches counted, every grid against a restatement, the memset of
// the owner planes inside workspace_bytes - and every refusal of the three entry points, each with nothing enqueued (prepare_main).
// DRIVE_MATCH=1 (life-cycle run): behind the lives (and the calls of the four switches above), dmm_match_objects on three shapes, B * NC up
// to the entry point's limit, with operands that are addresses only and a real workspace between guard bands - three launches each,
// every grid against a restatement, the workspace carve-up inside workspace_bytes - and every refusal, each with nothing enqueued (match_main).
// Launch coalescing (dmm_set_option("batch_wgrad"), on by default; DRIVE_OPTIONS_OFF=batch_wgrad runs one launch per record,
// DRIVE_BATCH_WGRAD=<0|1|2> sets the option's value: 2 = grouped on the weight-gradient stream instead of the caller's): every
// life-cycle run watches the enqueue calls through the fake runtime's hook and checks, with the option on or off, that
//   * no batch is pending where the weight-gradient side is joined or a gradient bucket is signalled: at every record of a join or
//     bucket event, the members the reduction launches have served so far (a grouped launch: gridDim.y) are the records run_ops
//     has taken so far (dmm_plan::batch_counts);
//   * at the end of every call each dense 3x3 weight-gradient record and each bw1.reduce record with slots of the range it ran has
//     been served exactly once (counted from the plan's own records);
// and prints "batch life <n>: <records> wg3 records in <launches> launches, <records> bw1.reduce records in <launches> launches".
// DRIVE_GROUPS=1 (life-cycle run): the parameter-group step.  A segment table over the plan's own tensors (BatchNorm tensors one class,
// convolutions another, the tensors of the first quarter of the arena a third with t0 > 0, the first tensor left out as a gap) goes
// through dmm_adam_table_init into a heap block of exactly dmm_adam_table_bytes; the uploaded form is checked (segments, and the
// first-segment index of every chunk against a search); dmm_adam_step_segmented and dmm_adam_step_guarded_segmented run on it; an
// unsorted table, a class out of range, a table that was never initialised and a wrong nclasses must be refused.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <sys/mman.h>

#include "plan.h"        // dmmfods_amd/csrc, or the csrc directory build.sh was pointed at (DRIVE_SRC)
#include "pointwise.h"

extern "C" long fakehip_launches();
extern "C" void fakehip_skip_large_memset(int on);
extern "C" long fakehip_violations();
extern "C" long fakehip_live_objects();
extern "C" long fakehip_live_streams();
extern "C" long fakehip_live_events();
extern "C" long fakehip_stream_creates();
extern "C" long fakehip_event_creates();
extern "C" void fakehip_set_hook(void (*hook)(int, const char*, unsigned, unsigned, const void*, const void*));

using namespace dmm;

namespace {
struct Region { const uint8_t* lo; const uint8_t* hi; const char* name; };
std::vector<Region> g_regions;
long g_bad = 0, g_checked = 0;

void chk(const void* p, const char* what, const char* label) {
  if (p == nullptr) return;
  ++g_checked;
  const uint8_t* q = (const uint8_t*)p;
  for (auto& r : g_regions)
    if (q >= r.lo && q < r.hi) return;
  ++g_bad;
  if (g_bad <= 20) fprintf(stderr, "[drive] pointer %s of launch '%s' = %p lies in none of the caller's regions\n", what, label, p);
}
#define CHK(field) chk((const void*)(field), #field, o.label)

void chk_seg(const Seg& s, const Op& o) {
  CHK(s.src); CHK(s.src2); CHK(s.scale); CHK(s.shift); CHK(s.q); CHK(s.r); CHK(s.ql); CHK(s.rl);
}
void chk_conv(const ConvArgs& a, const Op& o) {
  for (int s = 0; s < a.nseg; ++s) chk_seg(a.seg[s], o);
  CHK(a.wpack); CHK(a.out); CHK(a.stat_sum); CHK(a.stat_sq); CHK(a.logits); CHK(a.bx); CHK(a.bscale); CHK(a.bshift); CHK(a.bmean);
  CHK(a.binvstd); CHK(a.red1); CHK(a.red2); CHK(a.eff_out); CHK(a.eq); CHK(a.er);
  for (int p = 0; p < a.nphase; ++p) CHK(a.ph_wpack[p]);
}
void chk_wgrad(const WgradArgs& a, const Op& o) {
  for (int s = 0; s < a.nseg; ++s) chk_seg(a.seg[s], o);
  chk_seg(a.dy, o);
  CHK(a.dpack); CHK(a.part);
  for (int p = 0; p < a.nphase; ++p) CHK(a.ph_dpack[p]);
}
void chk_ops(const std::vector<Op>& ops) {
  for (const Op& o : ops) {
    switch (o.kind) {
      case OP_MEMSET: CHK(o.ms.p); if (o.ms.bytes) chk((const uint8_t*)o.ms.p + o.ms.bytes - 1, "ms.p + bytes - 1", o.label); break;
      case OP_COPY: CHK(o.cp.dst); CHK(o.cp.src); break;
      case OP_CONVERT: CHK(o.cv.src1); CHK(o.cv.src2); CHK(o.cv.dst); CHK(o.cv.stat_sum); CHK(o.cv.stat_sq); CHK(o.cv.dyn_scale); break;
      case OP_IGEMM: chk_conv(o.c, o); break;
      case OP_WGRAD: chk_wgrad(o.w, o); break;
      case OP_BW1: case OP_BW1RED: chk_conv(o.b1.c, o); CHK(o.b1.dpack); CHK(o.b1.part); break;
      case OP_BNFIN: CHK(o.bf.sum); CHK(o.bf.sq); CHK(o.bf.gamma); CHK(o.bf.beta); CHK(o.bf.running_mean); CHK(o.bf.running_var);
                     CHK(o.bf.scale); CHK(o.bf.shift); CHK(o.bf.mean); CHK(o.bf.invstd); break;
      case OP_BNBWD: CHK(o.bb.red1); CHK(o.bb.red2); CHK(o.bb.mean); CHK(o.bb.invstd); CHK(o.bb.scale); CHK(o.bb.dgamma); CHK(o.bb.dbeta);
                     CHK(o.bb.qd); CHK(o.bb.rd); CHK(o.bb.q); CHK(o.bb.r); CHK(o.bb.ql); CHK(o.bb.rl); break;
      case OP_POOL: if (o.epi == POOL_AVG2) { CHK(o.ap.x); CHK(o.ap.scale); CHK(o.ap.shift); CHK(o.ap.out); break; }
                    CHK(o.mp.y0); CHK(o.mp.scale); CHK(o.mp.shift); CHK(o.mp.out); CHK(o.mp.argmax); CHK(o.mp.stat_sum); CHK(o.mp.stat_sq); break;
      case OP_POOLBWD: CHK(o.mpb.y0); CHK(o.mpb.scale); CHK(o.mpb.shift); CHK(o.mpb.gpool); CHK(o.mpb.xpool); CHK(o.mpb.q); CHK(o.mpb.r);
                       CHK(o.mpb.ql); CHK(o.mpb.rl); CHK(o.mpb.mean); CHK(o.mpb.invstd); CHK(o.mpb.argmax); CHK(o.mpb.gy0); CHK(o.mpb.red1);
                       CHK(o.mpb.red2); break;
      case OP_BCE: CHK(o.bce.logits); CHK(o.bce.target); CHK(o.bce.dlogits); CHK(o.bce.out); CHK(o.bce.loss_out); CHK(o.bce.dx_out); CHK(o.bce.dyn_scale); break;
      case OP_PACK: case OP_UNPACK: CHK(o.pk.descs); CHK(o.pk.prefix); CHK(o.pk.tdescs); CHK(o.pk.tiles); break;
      case OP_APPLYCORR: CHK(o.ac.g); CHK(o.ac.y); CHK(o.ac.q); CHK(o.ac.r); CHK(o.ac.ql); CHK(o.ac.rl); break;
      case OP_FIN64: CHK(o.f64.sbuf); CHK(o.f64.dpack); CHK(o.f64.w); CHK(o.f64.scale); CHK(o.f64.shift); CHK(o.f64.mean); CHK(o.f64.invstd); CHK(o.f64.red1); CHK(o.f64.red2); break;
      case OP_RAWFIN: CHK(o.rf.sbuf); CHK(o.rf.dpack); CHK(o.rf.w); CHK(o.rf.gamma); CHK(o.rf.beta); CHK(o.rf.red1); CHK(o.rf.red2); break;
      case OP_JOIN: break;
      default: ++g_bad; fprintf(stderr, "[drive] unknown op kind %d\n", o.kind);
    }
  }
}
// the pack / unpack descriptor tables as uploaded ("device" memory is host memory here)
void chk_descs(const dmm_plan* p) {
  Op o; snprintf(o.label, sizeof(o.label), "pack tables");
  for (auto& pd : p->packs) { CHK(pd.w); CHK(pd.dst); CHK(pd.gw); CHK(pd.dpack); }
  for (auto& pd : p->unpacks) { CHK(pd.w); CHK(pd.dst); CHK(pd.gw); CHK(pd.dpack); }
}

bool fill_desc(const std::string& arch, dmm_model_desc& d) {
  memset(&d, 0, sizeof(d));
  d.growth_rate = 32; d.num_init_features = 64; d.bn_size = 4; d.num_classes = 3;
  d.stream_1_in_channels = 3; d.loss_scale = 1.0f; d.bn_momentum = 0.1f; d.bn_eps = 1e-5f; d.iou_threshold = 0.7f; d.use_mfma = 1;
  auto cfg = [&](std::initializer_list<int> bc) { d.num_blocks = 0; for (int v : bc) d.block_config[d.num_blocks++] = v; };
  if (arch == "d121e") { cfg({6, 12, 24, 16}); d.concat_before_block_num = 1; d.stream_2_in_channels = 3; }
  else if (arch == "d121n") { cfg({6, 12, 24, 16}); d.concat_before_block_num = 1; d.stream_2_in_channels = 0; }
  else if (arch == "d121m") { cfg({6, 12, 24, 16}); d.concat_before_block_num = 3; d.stream_2_in_channels = 3; }
  else if (arch == "d121m2") { cfg({6, 12, 24, 16}); d.concat_before_block_num = 2; d.stream_2_in_channels = 3; }
  else if (arch == "d169m") { cfg({6, 12, 32, 32}); d.concat_before_block_num = 3; d.stream_2_in_channels = 3; }
  else if (arch == "d201m") { cfg({6, 12, 48, 32}); d.concat_before_block_num = 3; d.stream_2_in_channels = 3; }
  else if (arch == "d161m") { cfg({6, 12, 36, 24}); d.growth_rate = 48; d.num_init_features = 96; d.concat_before_block_num = 3; d.stream_2_in_channels = 3; }
  else if (arch == "tiny_mid") { cfg({2, 2, 2}); d.concat_before_block_num = 2; d.stream_2_in_channels = 3; }       // the A/B tests' net
  else if (arch == "tiny_early") { cfg({2, 2, 2}); d.concat_before_block_num = 1; d.stream_2_in_channels = 3; }
  else if (arch == "tiny_no") { cfg({2, 2, 2}); d.concat_before_block_num = 1; d.stream_2_in_channels = 0; }
  else if (arch == "g8_mid") { cfg({2, 2, 2, 2}); d.growth_rate = 8; d.num_init_features = 16; d.concat_before_block_num = 3; d.stream_2_in_channels = 3; }  // smoke()'s net
  else return false;
  if (getenv("DRIVE_NO_MFMA")) d.use_mfma = 0;
  return true;
}

// ---- launch coalescing, watched from the runtime's side (see the head of the file) ----
struct BatchWatch {
  const dmm_plan* plan = nullptr;
  long long w3_served = 0, rd_served = 0;      // members served by the reduction launches seen so far
  long long w3_launches = 0, rd_launches = 0;  // wg3 kernel launches (single or grouped), bw1 reduction launches
  long long w3_want = 0, rd_want = 0;          // records of the ranges run so far (from the plan's lists)
  long bad = 0, syncs = 0;
} g_watch;
void batch_complain(const char* where) {
  ++g_watch.bad;
  if (g_watch.bad <= 10)
    fprintf(stderr, "[drive] launch coalescing, %s: %lld wg3 / %lld bw1.reduce records served, run_ops has taken %lld / %lld\n", where, g_watch.w3_served,
            g_watch.rd_served, g_watch.plan->batch_counts[1], g_watch.plan->batch_counts[3]);
}
void batch_hook(int what, const char* kernel, unsigned, unsigned gy, const void*, const void* event) {
  BatchWatch& w = g_watch;
  if (w.plan == nullptr) return;
  if (what == 0) {
    const std::string k = kernel;
    if (k.find("wg3_group_reduce_kernel") != std::string::npos) w.w3_served += gy;
    else if (k.find("wg3_reduce_kernel") != std::string::npos) w.w3_served += 1;
    else if (k.find("bw1_reduce_group_kernel") != std::string::npos) { w.rd_served += gy; ++w.rd_launches; }
    else if (k.find("bw1_reduce_kernel") != std::string::npos) { w.rd_served += 1; ++w.rd_launches; }
    else if (k.find("wg3_group_kernel") != std::string::npos || k.find("wg3_kernel") != std::string::npos) ++w.w3_launches;
  } else if (what == 1) {   // a join or bucket event is recorded: nothing may be pending
    bool sync = false;
    for (void* e : w.plan->join_events) sync |= e == event;
    for (void* e : w.plan->bucket_events) sync |= e == event;
    if (!sync) return;
    ++w.syncs;
    if (w.w3_served != w.plan->batch_counts[1] || w.rd_served != w.plan->batch_counts[3]) batch_complain("at a join or bucket event");
  }
}
// the records of `ops` that a weight-gradient / reduction launch must serve
void batch_expect(const std::vector<Op>& ops) {
  for (const Op& o : ops) {
    if (o.kind == OP_WGRAD && o.impl == IMPL_WG3 && o.w.M > 0 && o.w.part != nullptr) ++g_watch.w3_want;
    if (o.kind == OP_BW1RED && o.b1.c.M > 0 && o.b1.part != nullptr) {
      const Bw1Geom q = bw1_geometry(o.b1.c);
      if (q.nsplit > 1 && q.nsplit * q.nct <= o.b1.part_slots) ++g_watch.rd_want;
    }
  }
}
bool batch_end_of_call(const char* what) {
  const BatchWatch& w = g_watch;
  const bool ok = w.w3_served == w.w3_want && w.rd_served == w.rd_want && w.w3_served == w.plan->batch_counts[1] && w.rd_served == w.plan->batch_counts[3] &&
                  w.w3_launches == w.plan->batch_counts[0] && w.rd_launches == w.plan->batch_counts[2];
  if (!ok) {
    batch_complain(what);
    fprintf(stderr, "[drive]   wanted %lld / %lld; launches seen %lld / %lld, counted %lld / %lld\n", w.w3_want, w.rd_want, w.w3_launches, w.rd_launches,
            w.plan->batch_counts[0], w.plan->batch_counts[2]);
  }
  return ok;
}

// ---- DRIVE_TRACE_ENQUEUE: the enqueue calls as text (see the head of the file) ----
struct EnqueueTrace {
  bool on = false;
  std::map<const void*, int> streams{{nullptr, 0}}, events;
  static int ordinal(std::map<const void*, int>& seen, const void* h) { return seen.emplace(h, (int)seen.size()).first->second; }
} g_enqueue;
// ---- DRIVE_HIST: what one dmm_logit_hist call enqueues (hist_main) ----
struct HistWatch {
  bool on = false;
  long launches = 0, memsets = 0, other = 0;
  std::string kernel;
  unsigned gx = 0, gy = 0;
  unsigned long long memset_bytes = 0;
} g_hist;
struct LaunchSeen { std::string kernel; unsigned gx, gy; };
std::vector<LaunchSeen> g_launch_log;   // (while g_hist.on: components_main reads seven launches of one call from it)
void drive_hook(int what, const char* kernel, unsigned gx, unsigned gy, const void* stream, const void* event) {
  if (g_enqueue.on) {
    const int s = EnqueueTrace::ordinal(g_enqueue.streams, stream);
    const unsigned long long bytes = gx | (unsigned long long)gy << 32;
    if (what == 0) printf("T launch %s %u %u s%d\n", kernel, gx, gy, s);
    else if (what == 1 || what == 2) printf("T %s e%d s%d\n", what == 1 ? "record" : "wait", EnqueueTrace::ordinal(g_enqueue.events, event), s);
    else printf("T %s %llu s%d\n", what == 3 ? "memset" : "memcpy", bytes, s);
  }
  batch_hook(what, kernel, gx, gy, stream, event);
  if (g_hist.on) {
    if (what == 0) { ++g_hist.launches; g_hist.kernel = kernel; g_hist.gx = gx; g_hist.gy = gy; g_launch_log.push_back({kernel, gx, gy}); }
    else if (what == 3) { ++g_hist.memsets; g_hist.memset_bytes = gx | (unsigned long long)gy << 32; }
    else ++g_hist.other;
  }
}

#define MUST(call)                                                                           \
  do {                                                                                       \
    const int rc__ = (call);                                                                 \
    if (rc__ != 0) {                                                                         \
      if (g_enqueue.on) printf("T error %d %s\n", rc__, dmm_last_error());                   \
      fprintf(stderr, "[drive] %s -> %d: %s\n", #call, rc__, dmm_last_error());              \
      return 2;                                                                              \
    }                                                                                        \
  } while (0)
}  // namespace

static int one_life(const dmm_model_desc& d, int life) {
  dmm_plan* plan = nullptr;
  MUST(dmm_plan_create(&d, &plan));
  const bool freeze = getenv("DRIVE_FREEZE") != nullptr;
  if (freeze) {
    const size_t wsb_default = dmm_plan_workspace_bytes(plan);
    if (dmm_plan_set_encoder_frozen(nullptr, 1) != DMM_ERR_INVALID) { fprintf(stderr, "[drive] a null plan was not refused\n"); return 2; }
    MUST(dmm_plan_set_encoder_frozen(plan, 0));   // nothing changes
    if (dmm_plan_workspace_bytes(plan) != wsb_default) { fprintf(stderr, "[drive] frozen = 0 changed a fresh plan\n"); return 2; }
    MUST(dmm_plan_set_encoder_frozen(plan, 1));
    if (dmm_plan_workspace_bytes(plan) > wsb_default) { fprintf(stderr, "[drive] the frozen plan's workspace is larger than the default's\n"); return 2; }
  }
  const size_t wsb = dmm_plan_workspace_bytes(plan);
  const int64_t np = dmm_plan_num_params(plan), nb = std::max<int64_t>(dmm_plan_num_buffer_elems(plan), 1);
  // 256-byte aligned workspace with nothing mapped... ASan red zones sit on either side of each allocation
  uint8_t* ws = (uint8_t*)aligned_alloc(256, (wsb + 255) / 256 * 256);
  float* params = (float*)malloc(np * 4); float* grads = (float*)malloc(np * 4); float* buffers = (float*)malloc(nb * 4);
  const size_t px = (size_t)d.batch * d.height * d.width;
  float* in1 = (float*)malloc(px * std::max(1, d.stream_1_in_channels) * 4);
  float* in2 = (float*)malloc(px * std::max(1, d.stream_2_in_channels) * 4);
  float* logits = (float*)malloc(px * d.num_classes * 4);
  float* target = (float*)malloc(px * d.num_classes * 4);
  const size_t nmet = 2 * d.num_classes + (size_t)d.batch * 2 * d.num_classes;
  double* metrics = (double*)malloc(nmet * 8);
  g_regions = {{ws, ws + wsb, "workspace"}, {(uint8_t*)params, (uint8_t*)(params + np), "params"}, {(uint8_t*)grads, (uint8_t*)(grads + np), "grads"},
               {(uint8_t*)buffers, (uint8_t*)(buffers + nb), "buffers"}, {(uint8_t*)in1, (uint8_t*)in1 + px * 3 * 4, "in1"},
               {(uint8_t*)in2, (uint8_t*)in2 + px * 3 * 4, "in2"}, {(uint8_t*)logits, (uint8_t*)logits + px * d.num_classes * 4, "logits"},
               {(uint8_t*)target, (uint8_t*)target + px * d.num_classes * 4, "target"}};
  // (a kernel family switched off between sizing and binding must NOT change what the plan reserves: buffers are reserved by shape)
  if (const char* t = getenv("DRIVE_TOGGLE_BETWEEN_CREATE_AND_BIND")) MUST(dmm_set_option(t, 0));
  // (test of the bind-time check: a plan whose switches were tampered with after it was sized reserves other bytes -> DMM_ERR_STATE)
  if (getenv("DRIVE_FLIP_SWITCH_BETWEEN_CREATE_AND_BIND")) plan->sw.no_eff_compact = !plan->sw.no_eff_compact;
  MUST(dmm_plan_bind(plan, ws, wsb, params, grads, buffers));
  int64_t enc_lo = 0, enc_hi = 0;   // the leading encoder range of the arena (`features`): [enc_lo, enc_hi)
  if (freeze) {
    if (!plan->encoder_frozen) { fprintf(stderr, "[drive] the frozen mode did not survive dmm_plan_bind\n"); return 2; }
    if (dmm_plan_set_encoder_frozen(plan, 0) != DMM_ERR_STATE) { fprintf(stderr, "[drive] a bound plan was not refused\n"); return 2; }
    auto enc = [](const std::string& n) { return n.rfind("features.", 0) == 0 || n.rfind("stream_2_features.", 0) == 0 || n.rfind("concat_module.", 0) == 0; };
    for (const TensorInfo& t : plan->tensors) {
      if (t.kind > DMM_T_BN_BIAS || !enc(t.name)) continue;
      int64_t n = 1;
      for (int k = 0; k < t.ndim; ++k) n *= t.shape[k];
      if (t.off == enc_hi) enc_hi = t.off + n;
      for (const GradBucket& b : plan->buckets)
        if (t.off < b.off + b.n && b.off < t.off + n) { fprintf(stderr, "[drive] a bucket overlaps the frozen tensor %s\n", t.name.c_str()); return 2; }
      for (const PackDesc& pd : plan->unpacks)
        if (pd.gw >= grads + t.off && pd.gw < grads + t.off + n) { fprintf(stderr, "[drive] an unpack descriptor scatters into the frozen tensor %s\n", t.name.c_str()); return 2; }
    }
    if (enc_hi <= 0 || enc_hi >= np) { fprintf(stderr, "[drive] no leading encoder range\n"); return 2; }
  }
  if (getenv("DRIVE_TOGGLE_BETWEEN_CREATE_AND_BIND")) {   // the families the bound plan recorded: "FAMILIES <name>=<launch records> ..." (a fused pair counts as bw1)
    int n[IMPL_COUNT] = {};
    for (const auto* ops : {&plan->fwd_train, &plan->fwd_eval, &plan->bwd})
      for (const Op& o : *ops) {
        if (o.kind == OP_IGEMM || o.kind == OP_WGRAD) ++n[o.impl];
        if (o.kind == OP_BW1) ++n[IMPL_BW1];
      }
    printf("FAMILIES");
    for (int f = 1; f < IMPL_COUNT; ++f) printf(" %s=%d", dmm_impl_name(f), n[f]);
    printf("\n");
  }
  // (test of the per-launch family check: a launch whose record names a family that will not take it - here a dense 3x3 weight
  // gradient recorded as wg5, which refuses it, so the generic kernel runs - makes the backward pass return DMM_ERR_STATE)
  if (getenv("DRIVE_TAMPER_RECORDED_FAMILY"))
    for (Op& o : plan->bwd)
      if (o.kind == OP_WGRAD && o.impl == IMPL_WG3) { o.impl = IMPL_WG5; break; }
  const long l0 = fakehip_launches();
  g_watch = BatchWatch();
  g_watch.plan = plan;   // (from here on drive_hook hands the enqueue calls to batch_hook)
  // (every backward call runs the whole list - the external-gradient one but for the loss record; no forward list has such records)
#define BACKWARD_DONE(what) do { batch_expect(plan->bwd); if (!batch_end_of_call(what)) return 2; } while (0)
  void* st = nullptr;  // the caller's stream: the null stream, as torch's default
  // the guarded optimiser step's state block, scratch and moment arenas ("device" memory = heap: ASan sees every host-side touch)
  const bool dyn = getenv("DRIVE_DYN_SCALE") != nullptr || freeze;
  dmm_guard_state* gstate = (dmm_guard_state*)aligned_alloc(64, sizeof(dmm_guard_state));
  void* gscratch = malloc(dmm_grad_guard_scratch_bytes(np));
  float* mom1 = (float*)malloc(np * 4); float* mom2 = (float*)malloc(np * 4);
  if (dyn) {
    g_regions.push_back({(uint8_t*)gstate, (uint8_t*)(gstate + 1), "guard"});
    MUST(dmm_guard_state_init(gstate, 65536.f, 0, 0, st));
    MUST(dmm_plan_set_dynamic_loss_scale(plan, &gstate->scale));
  }
  for (int rep = 0; rep < 2; ++rep) {
    MUST(dmm_plan_forward(plan, in1, d.stream_2_in_channels ? in2 : nullptr, logits, 1, st));
    MUST(dmm_plan_loss_backward(plan, logits, target, metrics, st));
    BACKWARD_DONE("end of a training step");
    if (freeze) {   // two trainable ranges: everything behind the leading encoder range from the start, that range released at step 1
      const dmm_adam_segment one[1] = {{enc_hi, np - enc_hi, 0}}, two[2] = {{enc_lo, enc_hi - enc_lo, 1}, {enc_hi, np - enc_hi, 0}};
      const dmm_adam_class origins[2] = {{1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 0, 0}, {1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 0, 1}};
      const int ns = rep == 0 ? 1 : 2;
      const size_t tb = dmm_adam_table_bytes(ns, np);
      if (tb == 0) { fprintf(stderr, "[drive] dmm_adam_table_bytes (freeze)\n"); return 2; }
      void* table = aligned_alloc(8, (tb + 7) / 8 * 8);
      MUST(dmm_adam_table_init(table, rep == 0 ? one : two, ns, np, ns, st));
      MUST(dmm_adam_step_guarded_segmented(params, grads, mom1, mom2, np, table, ns, origins, ns, 1.0f, 2.f, 0.5f, 2000, gstate, gscratch, st));
      const dmm_adam_segment bad[2] = {{0, enc_hi, 1}, {enc_hi - 1, np - enc_hi, 0}};
      if (dmm_adam_table_init(table, bad, 2, np, 2, st) != DMM_ERR_INVALID) { fprintf(stderr, "[drive] overlapping ranges were not refused\n"); return 2; }
      if (getenv("DRIVE_EMA")) {   // the two steps that keep a parameter average, on the table `bad` did not replace, then every refusal of theirs
        float* avg = (float*)malloc(np * 4);
        dmm_adam_ema e = {avg, 0.999f, 1, 1};
        MUST(dmm_adam_step_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 2, 1.f, st, &e));
        e.k_or_t0 = 0;           // guarded: the applied-step count at which averaging began
        MUST(dmm_adam_step_guarded_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 1.0f, 2.f, 0.5f, 2000, gstate, gscratch, st, &e));
        e.warmup = 0;
        MUST(dmm_adam_step_guarded_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 1.0f, 2.f, 0.5f, 2000, gstate, gscratch, st, &e));
        // (refused by both calls, with a message that names the argument)
        auto both_refuse = [&](const dmm_adam_ema* bad_ema, const char* what, const char* names) {
          const int a = dmm_adam_step_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 2, 1.f, st, bad_ema);
          const bool an = strstr(dmm_last_error(), names) != nullptr;
          const int b = dmm_adam_step_guarded_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 1.0f, 2.f, 0.5f, 2000, gstate, gscratch, st, bad_ema);
          const bool bn = strstr(dmm_last_error(), names) != nullptr;
          if (a == DMM_ERR_INVALID && b == DMM_ERR_INVALID && an && bn) return true;
          fprintf(stderr, "[drive] %s was not refused (%d, %d) or the message does not say '%s': %s\n", what, a, b, names, dmm_last_error());
          return false;
        };
        const dmm_adam_ema good = {avg, 0.999f, 1, 1};
        dmm_adam_ema b = good;
        if (!both_refuse(nullptr, "a null dmm_adam_ema", "ema is null")) return 2;
        b.ema = nullptr;
        if (!both_refuse(&b, "a null average", "ema->ema is null")) return 2;
        float* const arenas[4] = {params, grads, mom1, mom2};
        for (float* a : arenas) {
          b.ema = a;
          if (!both_refuse(&b, "an average that is one of the arenas", "ema->ema aliases")) return 2;
          b.ema = a + np - 1;
          if (!both_refuse(&b, "an average that overlaps an arena's end", "ema->ema aliases")) return 2;
        }
        b = good;
        const float decays[4] = {1.f, -0.1f, 1.5f, __builtin_nanf("")};
        for (float dk : decays) {
          b.decay = dk;
          if (!both_refuse(&b, "a decay outside [0, 1)", "ema->decay")) return 2;
        }
        b = good; b.k_or_t0 = 0;
        if (dmm_adam_step_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 2, 1.f, st, &b) != DMM_ERR_INVALID) { fprintf(stderr, "[drive] k = 0 was not refused\n"); return 2; }
        // ... and what the counterparts refuse: step 0, another nsegs, growth_factor < 1
        if (dmm_adam_step_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 0, 1.f, st, &good) != DMM_ERR_INVALID ||
            dmm_adam_step_segmented_ema(params, grads, mom1, mom2, np, table, ns + 1, origins, ns, 2, 1.f, st, &good) != DMM_ERR_INVALID ||
            dmm_adam_step_guarded_segmented_ema(params, grads, mom1, mom2, np, table, ns, origins, ns, 1.0f, 0.5f, 0.5f, 2000, gstate, gscratch, st, &good) != DMM_ERR_INVALID) {
          fprintf(stderr, "[drive] a refusal of the step without an average is missing from the one with it\n"); return 2;
        }
        free(avg);
      }
      free(table);
    } else if (dyn) {
      MUST(dmm_adam_step_guarded(params, grads, mom1, mom2, np, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.f, 1.0f, 2.f, 0.5f, 2000, gstate, gscratch, st));
      MUST(dmm_grad_sumsq(grads, np / 2, np - np / 2, 1, gscratch, st));
    }
  }
  if (getenv("DRIVE_GROUPS")) {
    std::vector<dmm_adam_segment> segs;
    bool first_tensor = true;
    for (const TensorInfo& t : plan->tensors) {
      if (t.kind > DMM_T_BN_BIAS) continue;
      int64_t n = 1;
      for (int k = 0; k < t.ndim; ++k) n *= t.shape[k];
      if (first_tensor) { first_tensor = false; continue; }   // a gap in front of the first segment
      const int cls = t.off < np / 4 ? 2 : (t.kind >= DMM_T_BN_WEIGHT ? 1 : 0);
      if (!segs.empty() && segs.back().begin + segs.back().count == t.off && segs.back().cls == cls) segs.back().count += n;
      else segs.push_back({t.off, n, cls});
    }
    std::sort(segs.begin(), segs.end(), [](const dmm_adam_segment& a, const dmm_adam_segment& b) { return a.begin < b.begin; });
    const int ns = (int)segs.size();
    const size_t tb = dmm_adam_table_bytes(ns, np);
    if (ns < 3 || tb == 0 || dmm_adam_table_bytes(0, np) != 0 || dmm_adam_table_bytes(ns, 0) != 0) { fprintf(stderr, "[drive] dmm_adam_table_bytes\n"); return 2; }
    uint8_t* table = (uint8_t*)aligned_alloc(8, (tb + 7) / 8 * 8);
    uint8_t* never = (uint8_t*)aligned_alloc(8, (tb + 7) / 8 * 8);
    MUST(dmm_adam_table_init(table, segs.data(), ns, np, 3, st));
    {   // the uploaded form
      const AdamSegDev* sd = (const AdamSegDev*)table;
      const int* first = (const int*)(table + (size_t)ns * sizeof(AdamSegDev));
      for (int i = 0; i < ns; ++i)
        if (sd[i].begin != segs[i].begin || sd[i].end != segs[i].begin + segs[i].count || sd[i].cls != segs[i].cls) { fprintf(stderr, "[drive] table segment %d\n", i); return 2; }
      const int64_t nch = (np + ADAM_SEG_CHUNK - 1) / ADAM_SEG_CHUNK;
      if ((size_t)ns * sizeof(AdamSegDev) + (size_t)nch * sizeof(int) != tb) { fprintf(stderr, "[drive] table size\n"); return 2; }
      for (int64_t ch = 0; ch < nch; ++ch) {
        int want = 0;
        while (want < ns && sd[want].end <= ch * ADAM_SEG_CHUNK) ++want;
        if (first[ch] != want) { fprintf(stderr, "[drive] first[%lld] = %d, want %d\n", (long long)ch, first[ch], want); return 2; }
      }
    }
    const dmm_adam_class classes[3] = {{1e-3f, 0.9f, 0.999f, 1e-8f, 0.01f, 0, 0}, {1e-3f, 0.9f, 0.999f, 1e-8f, 0.f, 0, 0}, {1e-4f, 0.8f, 0.99f, 1e-6f, 0.1f, 1, 2}};
    MUST(dmm_adam_step_segmented(params, grads, mom1, mom2, np, table, ns, classes, 3, 1, 1.f, st));
    MUST(dmm_adam_step_segmented(params, grads, mom1, mom2, np, table, ns, classes, 3, 3, 0.5f, st));
    if (!dyn) MUST(dmm_guard_state_init(gstate, 1.f, 0, 0, st));
    MUST(dmm_adam_step_guarded_segmented(params, grads, mom1, mom2, np, table, ns, classes, 3, 1.0f, 2.f, 0.5f, 2000, gstate, gscratch, st));
    auto refused = [&](int rc, const char* what) {
      if (rc == DMM_ERR_INVALID) return true;
      fprintf(stderr, "[drive] %s was not refused (%d)\n", what, rc);
      return false;
    };
    std::vector<dmm_adam_segment> bad = segs;
    std::swap(bad[0], bad[1]);
    if (!refused(dmm_adam_table_init(table, bad.data(), ns, np, 3, st), "an unsorted table")) return 2;
    bad = segs; bad[1].begin = bad[0].begin + bad[0].count - 1;
    if (!refused(dmm_adam_table_init(table, bad.data(), ns, np, 3, st), "overlapping segments")) return 2;
    bad = segs; bad[2].cls = 3;
    if (!refused(dmm_adam_table_init(table, bad.data(), ns, np, 3, st), "a class out of range")) return 2;
    bad = segs; bad[ns - 1].count = np - bad[ns - 1].begin + 1;
    if (!refused(dmm_adam_table_init(table, bad.data(), ns, np, 3, st), "a segment past n")) return 2;
    if (!refused(dmm_adam_step_segmented(params, grads, mom1, mom2, np, never, ns, classes, 3, 1, 1.f, st), "a table never initialised")) return 2;
    if (!refused(dmm_adam_step_segmented(params, grads, mom1, mom2, np, table, ns, classes, 2, 1, 1.f, st), "another nclasses")) return 2;
    if (!refused(dmm_adam_step_segmented(params, grads, mom1, mom2, np, table, ns - 1, classes, 3, 1, 1.f, st), "another nsegs")) return 2;
    if (!refused(dmm_adam_step_segmented(params, grads, mom1, mom2, np, table, ns, classes, 3, 0, 1.f, st), "step 0")) return 2;
    if (!refused(dmm_adam_step_guarded_segmented(params, grads, mom1, mom2, np, table, ns, classes, 3, 1.0f, 0.5f, 0.5f, 2000, gstate, gscratch, st), "growth_factor < 1")) return 2;
    free(table); free(never);
  }
  if (dyn && plan->bwd[plan->bce_op].bce.dyn_scale != &gstate->scale) { fprintf(stderr, "[drive] the loss record lost its dynamic scale\n"); return 2; }
  chk_ops(plan->fwd_train); chk_ops(plan->fwd_eval); chk_ops(plan->bwd); chk_descs(plan);
  MUST(dmm_plan_forward(plan, in1, d.stream_2_in_channels ? in2 : nullptr, logits, 1, st));
  MUST(dmm_plan_backward(plan, target /*stands for d(loss)/d(logit)*/, st));
  BACKWARD_DONE("end of the external-gradient backward");
  MUST(dmm_plan_forward(plan, in1, d.stream_2_in_channels ? in2 : nullptr, logits, 0, st));
  MUST(dmm_plan_loss_metrics(plan, logits, target, metrics, st));
  // the data-parallel hooks: wait for every bucket on the caller's stream
  for (int b = 0; b < dmm_plan_num_grad_buckets(plan); ++b) MUST(dmm_plan_grad_bucket_wait(plan, b, st));
  // a profiled pass (per-op events), then one bracketing a single class as bench.py does in its timed region
  MUST(dmm_plan_profile_begin(plan, 1));
  MUST(dmm_plan_forward(plan, in1, d.stream_2_in_channels ? in2 : nullptr, logits, 1, st));
  MUST(dmm_plan_loss_backward(plan, logits, target, metrics, st));
  BACKWARD_DONE("end of the profiled pass");
  {
    std::vector<double> ms(dmm_plan_profile_num_ops(plan, 1));
    int passes = 0;
    MUST(dmm_plan_profile_collect(plan, 1, ms.data(), (int)ms.size(), &passes));
  }
  MUST(dmm_plan_profile_filter(plan, "bw1."));
  MUST(dmm_plan_profile_begin(plan, 1));
  MUST(dmm_plan_forward(plan, in1, d.stream_2_in_channels ? in2 : nullptr, logits, 1, st));
  MUST(dmm_plan_loss_backward(plan, logits, target, metrics, st));
  BACKWARD_DONE("end of the filtered profile pass");
  MUST(dmm_plan_profile_begin(plan, 0));
  // one more step WITHOUT synchronising anything, then destroy: teardown must not rely on the caller having drained the device
  MUST(dmm_plan_forward(plan, in1, d.stream_2_in_channels ? in2 : nullptr, logits, 1, st));
  MUST(dmm_plan_loss_backward(plan, logits, target, metrics, st));
  BACKWARD_DONE("end of the last step");
#undef BACKWARD_DONE
  const BatchWatch watch = g_watch;
  g_watch.plan = nullptr;
  const long launches = fakehip_launches() - l0;
  const size_t nf = plan->fwd_train.size(), nbw = plan->bwd.size();
  MUST(dmm_plan_destroy(plan));
  free(ws); free(params); free(grads); free(buffers); free(in1); free(in2); free(logits); free(target); free(metrics);
  free(gstate); free(gscratch); free(mom1); free(mom2);
  printf("life %d: workspace %.1f MiB, %zu + %zu launch records, %ld launches, %ld pointers checked, %ld bad, streams alive %ld (created %ld), events alive %ld (created %ld), violations %ld\n",
         life, wsb / 1048576.0, nf, nbw, launches, g_checked, g_bad, fakehip_live_streams(), fakehip_stream_creates(), fakehip_live_events(),
         fakehip_event_creates(), fakehip_violations());
  printf("batch life %d: %lld wg3 records in %lld launches, %lld bw1.reduce records in %lld launches, %ld join / bucket events checked, %ld bad\n", life,
         watch.w3_served, watch.w3_launches, watch.rd_served, watch.rd_launches, watch.syncs, watch.bad);
  if (watch.bad) { fprintf(stderr, "[drive] FAIL: a batch was pending at a join or bucket event\n"); return 1; }
  return 0;
}

// ---- accum: one plan, gradient accumulation on and off ----
static int accum_main(int argc, char** argv) {
  if (argc < 7) return 64;
  dmm_model_desc d;
  if (!fill_desc(argv[2], d)) { fprintf(stderr, "unknown arch %s\n", argv[2]); return 64; }
  const std::string dt = argv[3];
  d.dtype = dt == "f32" ? DMM_F32 : (dt == "f16" ? DMM_F16 : DMM_BF16);
  d.batch = atoi(argv[4]); d.height = atoi(argv[5]); d.width = atoi(argv[6]);
  if (dmm_plan_set_grad_accumulate(nullptr, 1) != DMM_ERR_INVALID) { fprintf(stderr, "[drive] a null plan was not refused\n"); return 2; }
  dmm_plan* plan = nullptr;
  MUST(dmm_plan_create(&d, &plan));
  MUST(dmm_plan_set_grad_accumulate(plan, 1));   // on an unbound plan: must survive bind
  const size_t wsb = dmm_plan_workspace_bytes(plan);
  const int64_t np = dmm_plan_num_params(plan), nb = std::max<int64_t>(dmm_plan_num_buffer_elems(plan), 1);
  uint8_t* ws = (uint8_t*)aligned_alloc(256, (wsb + 255) / 256 * 256);
  float* params = (float*)malloc(np * 4); float* grads = (float*)malloc(np * 4); float* buffers = (float*)malloc(nb * 4);
  const size_t px = (size_t)d.batch * d.height * d.width;
  float* in1 = (float*)malloc(px * std::max(1, d.stream_1_in_channels) * 4);
  float* in2 = (float*)malloc(px * std::max(1, d.stream_2_in_channels) * 4);
  float* logits = (float*)malloc(px * d.num_classes * 4);
  float* target = (float*)malloc(px * d.num_classes * 4);
  double* metrics = (double*)malloc((2 * d.num_classes + (size_t)d.batch * 2 * d.num_classes) * 8);
  g_regions = {{ws, ws + wsb, "workspace"}, {(uint8_t*)params, (uint8_t*)(params + np), "params"}, {(uint8_t*)grads, (uint8_t*)(grads + np), "grads"},
               {(uint8_t*)buffers, (uint8_t*)(buffers + nb), "buffers"}, {(uint8_t*)in1, (uint8_t*)in1 + px * 3 * 4, "in1"},
               {(uint8_t*)in2, (uint8_t*)in2 + px * 3 * 4, "in2"}, {(uint8_t*)logits, (uint8_t*)logits + px * d.num_classes * 4, "logits"},
               {(uint8_t*)target, (uint8_t*)target + px * d.num_classes * 4, "target"}};
  MUST(dmm_plan_bind(plan, ws, wsb, params, grads, buffers));
  if (!plan->grad_accumulate) { fprintf(stderr, "[drive] the mode did not survive dmm_plan_bind\n"); return 2; }
  const int nops_on = dmm_plan_profile_num_ops(plan, 1);
  void* st = nullptr;
  float* s2 = d.stream_2_in_channels ? in2 : nullptr;
  auto arena_is = [&](unsigned char byte) {
    const unsigned char* g = (const unsigned char*)grads;
    for (size_t i = 0; i < (size_t)np * 4; ++i) if (g[i] != byte) return false;
    return true;
  };
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { printf("ACCUM %s %s\n", what, ok ? "ok" : "WRONG"); bad += !ok; };
  memset(grads, 0x5a, (size_t)np * 4);
  long l0 = fakehip_launches();
  for (int rep = 0; rep < 2; ++rep) {   // one window: two micro-batches, nothing cleared in between
    MUST(dmm_plan_forward(plan, in1, s2, logits, 1, st));
    MUST(dmm_plan_loss_backward(plan, logits, target, metrics, st));
  }
  const long launches_on = (fakehip_launches() - l0) / 2;
  expect(arena_is(0x5a), "mode on: the arena is not cleared");
  chk_ops(plan->bwd); chk_descs(plan);
  MUST(dmm_plan_set_grad_accumulate(plan, 0));
  expect(dmm_plan_profile_num_ops(plan, 1) == nops_on && nops_on > 0, "same launch records in both modes");
  l0 = fakehip_launches();
  MUST(dmm_plan_forward(plan, in1, s2, logits, 1, st));
  MUST(dmm_plan_loss_backward(plan, logits, target, metrics, st));
  expect(fakehip_launches() - l0 == launches_on, "same launches in both modes");
  expect(arena_is(0), "mode off: the arena is cleared");
  for (const Op& o : plan->bwd) if (o.kind == OP_BNBWD && o.bb.accumulate) { expect(false, "a launch record was rewritten"); break; }
  MUST(dmm_plan_set_grad_accumulate(plan, 1));
  memset(grads, 0x5a, (size_t)np * 4);
  MUST(dmm_plan_forward(plan, in1, s2, logits, 1, st));
  MUST(dmm_plan_backward(plan, target /*stands for d(loss)/d(logit)*/, st));
  expect(arena_is(0x5a), "mode on, external gradient: the arena is not cleared");
  MUST(dmm_plan_destroy(plan));
  free(ws); free(params); free(grads); free(buffers); free(in1); free(in2); free(logits); free(target); free(metrics);
  if (g_bad) { fprintf(stderr, "[drive] FAIL: %ld device pointers outside the caller's regions\n", g_bad); bad++; }
  if (fakehip_violations()) { fprintf(stderr, "[drive] FAIL: %ld teardown / handle violations\n", fakehip_violations()); bad++; }
  printf("accum: %d launch records, %ld launches per pass, %ld pointers checked\n", nops_on, launches_on, g_checked);
  printf("%s\n", bad ? "ACCUM FAILED" : "ACCUM OK");
  return bad ? 1 : 0;
}

// Address space without memory behind it: reserved, never committed; PROT_NONE where nothing at all may touch it.
static void* reserve(size_t bytes, int prot) {
  void* p = mmap(nullptr, bytes + 4096, prot, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (p == MAP_FAILED) { perror("[drive] mmap"); exit(3); }
  return p;
}
static double seg_bytes(int B, const Seg& s, int esz) { return (double)B * s.Hs * s.Ws * s.ld * esz; }

// ---- picks: the recorded family takes every launch ----
// One line per convolution launch ("PICK ..."), one per disagreement ("MISMATCH ..."); returns the number of disagreements.
// The test is capi.cpp's family_check, written out again on purpose: the recorded family is among those noted, and the generic family
// is noted beside another one only for wgp's two-segment launch (8-channel remainder).
static bool family_agrees(int kind, int impl, const WgradArgs* w, unsigned m) {
  const bool recorded_ran = (m >> impl) & 1u, generic_ran = (m >> IMPL_GENERIC) & 1u;
  const bool remainder = kind == OP_WGRAD && impl == IMPL_WGP && w->nseg == 2 && w->nphase == 0;
  return impl != IMPL_AUTO && recorded_ran && (impl == IMPL_GENERIC || !generic_ran || remainder);
}

static int check_list(const std::vector<Op>& ops, int dt, bool mfma, unsigned deny, const char* name) {
  int bad = 0, n = 0;
  const int esz = dt == DT_F32 ? 4 : 2;
  for (const Op& o : ops) {
    if (o.kind == OP_BW1) {   // decided by bw1_eligible when the plan was built: under the plan's mask the pair must still be eligible, and the launch must succeed
      WgradArgs w;
      memset(&w, 0, sizeof(w));
      const ConvArgs& c = o.b1.c;
      w.nseg = 1;
      Seg& x = w.seg[0];
      x.src = c.bx; x.ld = c.ldbx; x.scale = c.bscale; x.shift = c.bshift; x.mode = G_PLAIN; x.istride = 1; x.ntaps = 1; x.C = o.b1.wC; x.Cpad = o.b1.wC;
      x.Hs = c.Ho; x.Ws = c.Wo;
      w.dy = c.seg[0]; w.dy.C = 128;
      w.B = c.B; w.Ho = c.Ho; w.Wo = c.Wo; w.M = c.M; w.N = 128; w.Npad = o.b1.dNpad; w.dpack = o.b1.dpack;
      dmm_impl_mask(1);
      const hipError_t e = launch_bw1(o.b1, dt, nullptr);
      const unsigned m = dmm_impl_mask(1);
      ++n;
      if (e != hipSuccess || m != (1u << IMPL_BW1) || !bw1_eligible(w, c, dt, deny)) {
        ++bad;
        printf("%s MISMATCH %-40s recorded bw1 ran mask %#x rc %d eligible %d\n", name, o.label, m, (int)e, (int)bw1_eligible(w, c, dt, deny));
      }
      continue;
    }
    if (o.kind != OP_IGEMM && o.kind != OP_WGRAD) continue;
    dmm_impl_mask(1);
    const hipError_t e = o.kind == OP_IGEMM ? launch_igemm(o.c, dt, o.epi, mfma, nullptr, o.impl) : launch_wgrad(o.w, dt, mfma, nullptr, o.impl);
    const unsigned m = dmm_impl_mask(1);
    const int last = dmm_last_impl();
    ++n;
    const bool wg = o.kind == OP_WGRAD;
    const bool agree = e == hipSuccess && family_agrees(o.kind, o.impl, wg ? &o.w : nullptr, m);
    const int B = wg ? o.w.B : o.c.B;
    const double xb = seg_bytes(B, wg ? o.w.seg[0] : o.c.seg[0], esz), yb = wg ? seg_bytes(B, o.w.dy, esz) : 0.0;
    printf("%s PICK %s %s recorded %s mask %#x nphase %d x_bytes %.0f dy_bytes %.0f\n", name, wg ? "wgrad" : "igemm", o.label, dmm_impl_name(o.impl), m,
           wg ? o.w.nphase : o.c.nphase, xb, yb);
    if (!agree) {
      ++bad;
      printf("%s MISMATCH %-40s recorded %-8s ran-last %-8s mask %#x rc %d nphase %d\n", name, o.label, dmm_impl_name(o.impl), dmm_impl_name(last), m, (int)e,
             wg ? o.w.nphase : o.c.nphase);
    }
  }
  printf("%s: %d conv launches, %d disagree\n", name, n, bad);
  return bad;
}

static int picks_main(int argc, char** argv) {
  if (argc < 7) return 64;
  dmm_model_desc d;
  if (!fill_desc(argv[2], d)) { fprintf(stderr, "unknown arch %s\n", argv[2]); return 64; }
  const std::string dt = argv[3];
  d.dtype = dt == "f32" ? DMM_F32 : (dt == "f16" ? DMM_F16 : DMM_BF16);
  d.batch = atoi(argv[4]); d.height = atoi(argv[5]); d.width = atoi(argv[6]);
  dmm_plan* plan = nullptr;
  MUST(dmm_plan_create(&d, &plan));
  const size_t wsb = dmm_plan_workspace_bytes(plan);
  // (the op lists exist only in a BOUND plan: the sizing pass keeps none)
  void* ws = reserve(wsb, PROT_READ | PROT_WRITE);
  fakehip_skip_large_memset(1);   // (bind clears the workspace through the runtime: not this one)
  const int64_t np = dmm_plan_num_params(plan), nb = std::max<int64_t>(dmm_plan_num_buffer_elems(plan), 1);
  float* params = (float*)calloc(np, 4); float* grads = (float*)calloc(np, 4); float* buffers = (float*)calloc(nb, 4);
  MUST(dmm_plan_bind(plan, ws, wsb, params, grads, buffers));
  printf("workspace %.1f GiB, %zu + %zu + %zu launch records\n", wsb / 1073741824.0, plan->fwd_train.size(), plan->fwd_eval.size(), plan->bwd.size());
  const bool mfma = d.use_mfma != 0;
  const int bad = check_list(plan->fwd_train, d.dtype, mfma, plan->deny, "fwd") + check_list(plan->fwd_eval, d.dtype, mfma, plan->deny, "eval") +
                  check_list(plan->bwd, d.dtype, mfma, plan->deny, "bwd");
  MUST(dmm_plan_destroy(plan));
  munmap(ws, wsb + 4096);
  free(params); free(grads); free(buffers);
  printf("%s\n", bad ? "PICKS FAILED" : "PICKS OK");
  return bad ? 1 : 0;
}

// ---- dump: the plan as canonical text ----
// Every field of the argument struct a record's kind uses is printed (a Seg's taps up to ntaps, the ph_* arrays up to nphase, a
// PackSeg's tapw up to ntaps); every emitter assigns or zeroes every field of its struct, so no printed field is indeterminate.
// NOT printed: bytes of a record's union outside the member its kind uses, and the characters of `label` behind its terminator.
namespace {
struct Dumper {
  Region reg[5] = {};   // ws, params, grads, buffers, guard (the driver's guard state block; empty without DRIVE_DYN_SCALE)
  long outside = 0;
  void ptr(const char* name, const void* p) {
    if (p == nullptr) { printf(" %s=null", name); return; }
    const uint8_t* q = (const uint8_t*)p;
    for (auto& r : reg)
      if (q >= r.lo && q < r.hi) { printf(" %s=%s+%zu", name, r.name, (size_t)(q - r.lo)); return; }
    ++outside;
    printf(" %s=OUTSIDE", name);
  }
#define DP(f) ptr(#f, (const void*)(a.f))
#define DI(f) printf(" " #f "=%lld", (long long)(a.f))
#define DU(f) printf(" " #f "=%llu", (unsigned long long)(a.f))
#define DD(f) printf(" " #f "=%.17g", (double)(a.f))
  void seg(const char* name, const Seg& a) {
    printf("    %s:", name);
    DP(src); DP(src2); DP(scale); DP(shift); DP(q); DP(r); DP(ql); DP(rl); DI(ld); DI(ld2); DI(Hs); DI(Ws); DI(C); DI(Cpad); DI(ntaps); DI(nchunks);
    DI(mode); DI(istride);
    printf(" taps=");
    for (int t = 0; t < a.ntaps && t < MAX_TAPS; ++t) printf("%s%d", t ? "," : "", (int)a.taps[t]);
    printf("\n");
  }
  void conv(const ConvArgs& a) {
    for (int s = 0; s < a.nseg && s < 2; ++s) seg(s ? "seg1" : "seg0", a.seg[s]);
    printf("    conv:");
    DI(nseg); DI(B); DI(Ho); DI(Wo); DI(M); DP(wpack); DI(N); DI(Npad); DP(out); DI(ldo); DI(coff); DI(Hout); DI(Wout); DI(ostride); DI(py); DI(px);
    DP(stat_sum); DP(stat_sq); DP(logits); DP(bx); DI(ldbx); DP(bscale); DP(bshift); DP(bmean); DP(binvstd); DP(red1); DP(red2); DI(accumulate);
    DI(stat_stride); DI(pool2); DP(eff_out); DP(eq); DP(er); DI(nphase);
    printf("\n");
    for (int p = 0; p < a.nphase && p < 4; ++p) {
      printf("    phase%d:", p);
      DP(ph_wpack[p]); DI(ph_py[p]); DI(ph_px[p]); DI(ph_ntaps[p]);
      printf(" ph_taps0=");
      for (int t = 0; t < 4; ++t) printf("%s%d", t ? "," : "", (int)a.ph_taps0[p][t]);
      printf(" ph_taps1=");
      for (int t = 0; t < 9; ++t) printf("%s%d", t ? "," : "", (int)a.ph_taps1[p][t]);
      printf("\n");
    }
  }
  void wgrad(const WgradArgs& a) {
    for (int s = 0; s < a.nseg && s < 2; ++s) seg(s ? "seg1" : "seg0", a.seg[s]);
    seg("dy", a.dy);
    printf("    wgrad:");
    DI(nseg); DI(B); DI(Ho); DI(Wo); DI(M); DI(N); DI(Npad); DP(dpack); DI(rows_per_split); DI(kgroups); DP(part); DI(part_slots); DI(nphase);
    DP(t_mean); DP(t_invstd); DP(sbuf);
    printf("\n");
    for (int p = 0; p < a.nphase && p < 4; ++p) {
      printf("    phase%d:", p);
      DP(ph_dpack[p]); DI(ph_ytap[p]); DI(ph_ntaps[p]);
      printf(" ph_xtaps=");
      for (int t = 0; t < 4; ++t) printf("%s%d", t ? "," : "", (int)a.ph_xtaps[p][t]);
      printf("\n");
    }
  }
  void op(const Op& o) {
    printf("  op kind=%d epi=%d leaf=%d chain=%d signal=%d impl=%s label=%s flops=%.17g bytes=%.17g\n", o.kind, o.epi, o.leaf, o.chain, o.signal,
           dmm_impl_name(o.impl), o.label, o.flops, o.bytes);
    switch (o.kind) {
      case OP_MEMSET: { const MemsetArgs& a = o.ms; printf("    memset:"); DP(p); DU(bytes); printf("\n"); break; }
      case OP_COPY: { const CopyArgs& a = o.cp; printf("    copy:"); DP(dst); DP(src); DU(bytes); printf("\n"); break; }
      case OP_CONVERT: { const ConvertArgs& a = o.cv; printf("    convert:"); DP(src1); DP(src2); DI(C1); DI(C2); DP(dst); DI(B); DI(H); DI(W); DP(stat_sum);
                         DP(stat_sq); DD(scale); DP(dyn_scale); printf("\n"); break; }
      case OP_IGEMM: conv(o.c); break;
      case OP_WGRAD: wgrad(o.w); break;
      case OP_BW1: case OP_BW1RED: { conv(o.b1.c); const Bw1Args& a = o.b1; printf("    bw1:"); DP(dpack); DI(dNpad); DI(wC); DP(part); DI(part_slots); DI(nct);
                                     DI(ntiles); DI(tiles_per_wg); DI(xcd_group); DI(nsplit); printf("\n"); break; }
      case OP_BNFIN: { const BnFinalizeArgs& a = o.bf; printf("    bnfin:"); DP(sum); DP(sq); DI(stat_stride); DD(count); DD(count_unbiased); DP(gamma); DP(beta);
                       DP(running_mean); DP(running_var); DP(scale); DP(shift); DP(mean); DP(invstd); DI(C); DI(training); DD(momentum); DD(eps); printf("\n"); break; }
      case OP_BNBWD: { const BnBwdFinalizeArgs& a = o.bb; printf("    bnbwd:"); DP(red1); DP(red2); DI(stat_stride); DP(mean); DP(invstd); DP(scale); DP(dgamma);
                       DP(dbeta); DP(qd); DP(rd); DP(q); DP(r); DP(ql); DP(rl); DD(count); DD(grad_scale); DI(C); DI(accumulate); printf("\n"); break; }
      case OP_POOL: if (o.epi == POOL_AVG2) { const AvgPool2Args& a = o.ap; printf("    avgpool2:"); DP(x); DI(ld); DI(H); DI(W); DI(B); DI(C); DP(scale); DP(shift); DP(out);
                                      DI(ldo); printf("\n"); break; }
                    { const MaxpoolArgs& a = o.mp; printf("    pool:"); DP(y0); DI(ld0); DI(H0); DI(W0); DI(B); DI(C); DP(scale); DP(shift); DP(out); DI(ldo); DI(Hp);
                      DI(Wp); DP(argmax); DP(stat_sum); DP(stat_sq); DI(stat_stride); printf("\n"); break; }
      case OP_POOLBWD: { const MaxpoolBwdArgs& a = o.mpb; printf("    poolbwd:"); DP(y0); DI(ld0); DI(H0); DI(W0); DI(B); DI(C); DP(scale); DP(shift); DP(gpool);
                         DP(xpool); DP(q); DP(r); DP(ql); DP(rl); DP(mean); DP(invstd); DI(ldg); DI(Hp); DI(Wp); DP(argmax); DP(gy0); DP(red1); DP(red2);
                         DI(stat_stride); printf("\n"); break; }
      case OP_BCE: { const BceArgs& a = o.bce; printf("    bce:"); DP(logits); DP(target); DP(dlogits); DP(out); DI(B); DI(NC); DI(H); DI(W); DD(thr); DD(loss_scale);
                     DI(kind); DI(from_prob);
                     for (int k = 0; k < 8; ++k) { DD(alpha[k]); DD(gamma[k]); }
                     DP(loss_out); DP(dx_out); DI(metrics); DP(dyn_scale); printf("\n"); break; }
      case OP_PACK: case OP_UNPACK: { const PackArgs& a = o.pk; printf("    pack:"); DP(descs); DP(prefix); DI(ndesc); DI(total_rows); DD(grad_scale); DP(tdescs);
                                      DP(tiles); DI(nt1); DI(nt9); printf("\n"); break; }
      case OP_APPLYCORR: { const ApplyCorrArgs& a = o.ac; printf("    applycorr:"); DP(g); DP(y); DP(q); DP(r); DP(ql); DP(rl); DU(npix); DI(C); DI(ldg); DI(ldy);
                           printf("\n"); break; }
      case OP_FIN64: { const Fin64Args& a = o.f64; printf("    fin64:"); DP(sbuf); DP(dpack); DI(Npad); DP(w); DI(Kin); DI(nreal); DI(dtype); DP(scale); DP(shift);
                       DP(mean); DP(invstd); DP(red1); DP(red2); printf(" tapw=");
                       for (int t = 0; t < 28; ++t) printf("%s%d", t ? "," : "", (int)a.tapw[t]);
                       printf("\n"); break; }
      case OP_RAWFIN: { const RawFinArgs& a = o.rf; printf("    rawfin:"); DP(sbuf); DP(dpack); DI(Npad); DP(w); DI(Kin); DI(koff); DI(nreal); DP(gamma); DP(beta);
                        DP(red1); DP(red2); printf(" tapw=");
                        for (int t = 0; t < 9; ++t) printf("%s%d", t ? "," : "", a.tapw[t]);
                        printf("\n"); break; }
      case OP_JOIN: break;
      default: ++outside; printf("    UNKNOWN KIND OUTSIDE\n");
    }
  }
  void list(const char* name, const std::vector<Op>& ops) {
    printf("list %s records=%zu\n", name, ops.size());
    for (const Op& o : ops) op(o);
  }
  void descs(const char* name, const std::vector<PackDesc>& v) {
    printf("table %s entries=%zu\n", name, v.size());
    for (const PackDesc& a : v) {
      printf("  desc:");
      DP(w); DP(dst); DP(gw); DP(dpack); DI(N); DI(Npad); DI(nseg); DI(shared_master); DI(sn); DI(sk); DI(st); DI(rs); DI(tiled);
      printf("\n");
      for (int s = 0; s < a.nseg && s < 2; ++s) {
        const PackSeg& g = a.seg[s];
        printf("    packseg%d: Creal=%d Cpad=%d ntaps=%d nchunks=%d koff=%d tapw=", s, g.Creal, g.Cpad, g.ntaps, g.nchunks, g.koff);
        for (int t = 0; t < g.ntaps && t < MAX_TAPS; ++t) printf("%s%08x", t ? "," : "", g.tapw[t]);
        printf("\n");
      }
    }
  }
  static void ints(const char* name, const std::vector<int>& v) {
    printf("%s n=%zu:", name, v.size());
    for (int x : v) printf(" %d", x);
    printf("\n");
  }
  static void tiles(const char* name, const std::vector<PackTile>& v) {
    printf("table %s entries=%zu\n", name, v.size());
    for (const PackTile& t : v) printf("  tile desc=%d nsib=%d n0=%d cg=%d\n", t.desc, t.nsib, t.n0, t.cg);
  }
#undef DP
#undef DI
#undef DU
#undef DD
};
}  // namespace

static int dump_main(int argc, char** argv) {
  if (argc < 7) return 64;
  dmm_model_desc d;
  if (!fill_desc(argv[2], d)) { fprintf(stderr, "unknown arch %s\n", argv[2]); return 64; }
  const std::string dt = argv[3];
  d.dtype = dt == "f32" ? DMM_F32 : (dt == "f16" ? DMM_F16 : DMM_BF16);
  d.batch = atoi(argv[4]); d.height = atoi(argv[5]); d.width = atoi(argv[6]);
  const char* sh = getenv("DRIVE_MAP_SHIFT_MIB");
  const size_t shift = sh ? (size_t)atoi(sh) << 20 : 0;   // (whole MiB: the alignment of every region stays what it was)
  dmm_plan* plan = nullptr;
  MUST(dmm_plan_create(&d, &plan));
  if (getenv("DRIVE_FREEZE")) MUST(dmm_plan_set_encoder_frozen(plan, 1));
  const size_t wsb = dmm_plan_workspace_bytes(plan);
  uint8_t* ws0 = (uint8_t*)reserve(wsb + shift, PROT_READ | PROT_WRITE);
  fakehip_skip_large_memset(1);
  const int64_t np = dmm_plan_num_params(plan), nb = std::max<int64_t>(dmm_plan_num_buffer_elems(plan), 1);
  float* params0 = (float*)calloc(np + shift / 4, 4); float* grads0 = (float*)calloc(np + 2 * shift / 4, 4); float* buffers0 = (float*)calloc(nb + 3 * shift / 4, 4);
  uint8_t* ws = ws0 + shift;
  float *params = params0 + shift / 4, *grads = grads0 + 2 * shift / 4, *buffers = buffers0 + 3 * shift / 4;
  MUST(dmm_plan_bind(plan, ws, wsb, params, grads, buffers));
  Dumper D;
  D.reg[0] = {ws, ws + wsb, "ws"};
  D.reg[1] = {(uint8_t*)params, (uint8_t*)(params + np), "params"};
  D.reg[2] = {(uint8_t*)grads, (uint8_t*)(grads + np), "grads"};
  D.reg[3] = {(uint8_t*)buffers, (uint8_t*)(buffers + nb), "buffers"};
  static dmm_guard_state gstate;
  if (getenv("DRIVE_DYN_SCALE")) {
    D.reg[4] = {(uint8_t*)&gstate, (uint8_t*)(&gstate + 1), "guard"};
    MUST(dmm_plan_set_dynamic_loss_scale(plan, &gstate.scale));
  }
  printf("plan zero_bytes=%zu zero_bwd_bytes=%zu main_bytes=%zu nparams=%lld nbuf=%lld fwd_flops=%.17g metrics_bytes=%zu bucket_bytes=%zu\n", plan->zero_bytes,
         plan->zero_bwd_bytes, plan->main_bytes, (long long)plan->nparams, (long long)plan->nbuf, plan->fwd_flops, plan->metrics_bytes, plan->bucket_bytes);
  D.ptr("metrics", plan->metrics);
  printf(" logits_op_train=%d logits_op_eval=%d bce_op=%d\n", plan->logits_op_train, plan->logits_op_eval, plan->bce_op);
  Dumper::ints("convert_ops_train", plan->convert_ops_train);
  Dumper::ints("convert_ops_eval", plan->convert_ops_eval);
  D.list("fwd_train", plan->fwd_train);
  D.list("fwd_eval", plan->fwd_eval);
  D.list("bwd", plan->bwd);
  printf("bce_only\n");
  D.op(plan->bce_only);
  D.descs("packs", plan->packs);
  Dumper::ints("pack_prefix", plan->pack_prefix);
  D.descs("unpacks", plan->unpacks);
  Dumper::ints("unpack_prefix", plan->unpack_prefix);
  Dumper::tiles("pack_tiles", plan->pack_tiles);
  Dumper::tiles("unpack_tiles", plan->unpack_tiles);
  printf("table buckets entries=%zu\n", plan->buckets.size());
  for (const GradBucket& b : plan->buckets) printf("  bucket off=%lld n=%lld ev_main=%d ev_side=%d ready=%d\n", (long long)b.off, (long long)b.n, b.ev_main, b.ev_side, b.ready);
  MUST(dmm_plan_destroy(plan));
  munmap(ws0, wsb + shift + 4096);
  free(params0); free(grads0); free(buffers0);
  if (D.outside) { fprintf(stderr, "[drive] FAIL: %ld pointers of the plan lie in none of its regions\n", D.outside); return 1; }
  return 0;
}

// ---- single: one call of a single-kernel entry point; the large operands are addresses nothing may touch ----
static int single_main(int argc, char** argv) {
  if (argc < 13) return 64;
  const std::string entry = argv[2], dt = argv[3];
  dmm_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.dtype = dt == "f32" ? DMM_F32 : (dt == "f16" ? DMM_F16 : DMM_BF16);
  d.use_mfma = 1;
  d.B = atoi(argv[4]); d.H = atoi(argv[5]); d.W = atoi(argv[6]); d.Cin = atoi(argv[7]); d.Cout = atoi(argv[8]);
  d.R = d.S = atoi(argv[9]); d.stride = 1; d.pad = atoi(argv[10]); d.transposed = atoi(argv[11]); d.mode = atoi(argv[12]); d.bn_relu = 1;
  const size_t esz = d.dtype == DMM_F32 ? 4 : 2;
  const size_t up = (d.transposed || d.mode == 1) ? 4 : 1;
  const size_t xin = (size_t)d.B * d.H * d.W * d.Cin * esz, yout = (size_t)d.B * d.H * d.W * up * d.Cout * esz;
  void* x = reserve(xin, PROT_NONE); void* y = reserve(yout, PROT_NONE); void* gx = reserve(xin, PROT_NONE);
  // what the entry points zero or fill from the host side of the runtime is real memory
  const size_t wn = (size_t)d.Cin * d.Cout * d.R * d.S;
  float* w = (float*)calloc(wn, 4); float* dw = (float*)calloc(wn, 4);
  float* scale = (float*)calloc(d.Cin, 4); float* shift = (float*)calloc(3 * (size_t)d.Cin, 4);
  double* stats = (double*)calloc(2 * (size_t)d.Cout, 8); double* red = (double*)calloc(2 * (size_t)d.Cin, 8);
  const size_t sb = dmm_conv_scratch_bytes(&d);
  void* scratch = calloc(sb ? sb : 1, 1);
  const std::string flags = argc > 13 ? "," + std::string(argv[13]) + "," : ",";
  auto flag = [&](const char* f) { return flags.find("," + std::string(f) + ",") != std::string::npos; };
  if (flag("thinoff")) dmm_set_option("thin_logits", 0);
  if (flag("scalar")) d.use_mfma = 0;
  if (flag("stride2")) d.stride = 2;
  dmm_impl_mask(1);
  const long l0 = fakehip_launches();
  int rc = -99, merged = 0;   // merged: what the *_merged entry points report (1: one launch of four phases, 4: kept apart)
  if (entry == "fwd") rc = dmm_conv_forward(&d, x, w, scale, shift, y, stats, scratch, nullptr);
  else if (entry == "logits")   // the fp32 NCHW logits are an address only, as x
    rc = dmm_conv_logits(&d, flag("nullx") ? nullptr : x, flag("nullw") ? nullptr : w, scale, shift,
                         flag("nulllogits") ? nullptr : (float*)reserve((size_t)d.B * d.H * d.W * up * (d.Cout > 0 ? d.Cout : 1) * 4, PROT_NONE),
                         flag("nullscratch") ? nullptr : scratch, nullptr);
  else if (entry == "wgrad") rc = dmm_conv_wgrad_ex(&d, x, y, scale, shift, nullptr, nullptr, nullptr, 0, dw, scratch, nullptr);
  // the plan's merged four-phase launches of a ConvTranspose stage; withq: the deferred correction on the gradient (q, r real, yfwd an address)
  else if (entry == "fwdm")
    rc = dmm_conv_forward_merged(&d, flag("nullx") ? nullptr : x, w, scale, shift, y, stats, scratch, nullptr, flag("nullcount") ? nullptr : &merged);
  else if (entry == "wgradm") {
    float* qr = (float*)calloc(2 * (size_t)d.Cout + 16, 4);
    const bool wq = flag("withq");
    rc = dmm_conv_wgrad_merged(&d, x, flag("nulldy") ? nullptr : y, scale, shift, wq ? reserve(yout, PROT_NONE) : nullptr, (wq || flag("qonly")) ? qr : nullptr,
                               wq ? qr + d.Cout : nullptr, dw, scratch, nullptr, &merged);
  }
  else if (entry == "dgrad") rc = dmm_conv_dgrad_ex(&d, x, y, w, scale, shift, nullptr, nullptr, nullptr, gx, 0, red, scratch, nullptr);
  else if (entry == "fused") rc = dmm_conv1x1_backward_fused(&d, x, y, w, scale, shift, nullptr, nullptr, nullptr, gx, 0, dw, red, scratch, nullptr);
  else return 64;
  const unsigned m = dmm_impl_mask(1);
  std::string names;
  for (int f = 1; f < 32; ++f)
    if ((m >> f) & 1u) names += (names.empty() ? "" : "+") + std::string(dmm_impl_name(f));
  printf("SINGLE %s rc %d last %s ran %s launches %ld x_bytes %zu y_bytes %zu phases_as %d%s%s\n", entry.c_str(), rc, dmm_impl_name(dmm_last_impl()), names.empty() ? "none" : names.c_str(),
         fakehip_launches() - l0, xin, yout, merged, rc ? " error: " : "", rc ? dmm_last_error() : "");
  hipDeviceSynchronize();
  return fakehip_violations() ? 1 : 0;
}

// ---- refuse: the generic weight-gradient kernel implements one phase, the launch's own taps and a packed gradient - nothing else ----
// variant 0: plain (the control: must launch, noted as generic); 1: merged phases, 2: per-phase tap counts, 3: factor form - each refused with
// nothing launched and NOTHING noted; 4: the one launch where the generic kernel runs beside another family by design - wgp's two-segment
// form (a 128-channel segment with 2x2 taps + the 8-channel raw-input remainder) with the recorded family wgp: it succeeds, and the
// families noted must pass the per-launch check (today: wgp and its wave-specialised form, the remainder is not noted on its own).
static int refuse_main() {
  int bad = 0;
  static float dpack[64 * 64 * 32], sbuf[16], scale[128], shift[128];
  for (int variant = 0; variant < 5; ++variant) {
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.nseg = 1;
    Seg& x = a.seg[0];
    x.src = reserve(1 << 20, PROT_NONE); x.ld = 128; x.Hs = 8; x.Ws = 16; x.C = 128; x.Cpad = 128; x.ntaps = 1; x.nchunks = 4; x.mode = G_PLAIN; x.istride = 1;
    a.dy.src = reserve(1 << 20, PROT_NONE); a.dy.ld = 64; a.dy.Hs = 8; a.dy.Ws = 16; a.dy.C = 64; a.dy.Cpad = 64; a.dy.ntaps = 1; a.dy.nchunks = 1; a.dy.mode = G_PLAIN;
    a.dy.istride = 1;
    a.B = 1; a.Ho = 8; a.Wo = 16; a.M = 128; a.N = 64; a.Npad = 64; a.dpack = dpack;
    if (variant == 1) { a.nphase = 4; for (int ph = 0; ph < 4; ++ph) a.ph_dpack[ph] = dpack; }
    if (variant == 2) a.ph_ntaps[2] = 2;
    if (variant == 3) a.sbuf = sbuf;
    if (variant == 4) {
      x.scale = scale; x.shift = shift; x.ntaps = 4; x.nchunks = 16;
      const int t4[4][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 1}};
      for (int t = 0; t < 4; ++t) x.taps[t] = (short)((t4[t][0] & 0xff) | ((t4[t][1] & 0xff) << 8));
      a.nseg = 2;
      Seg& r = a.seg[1];
      r.src = reserve(1 << 20, PROT_NONE); r.ld = 8; r.Hs = 8; r.Ws = 16; r.C = 8; r.Cpad = 8; r.ntaps = 1; r.nchunks = 1; r.mode = G_PLAIN; r.istride = 1;
      r.scale = scale; r.shift = shift;
    }
    const int impl = variant == 4 ? IMPL_WGP : IMPL_GENERIC;
    const long l0 = fakehip_launches();
    dmm_impl_mask(1);
    const hipError_t e = launch_wgrad(a, DT_F16, true, nullptr, impl);
    const unsigned m = dmm_impl_mask(1);
    const long dl = fakehip_launches() - l0;
    bool ok;
    if (variant == 0) ok = e == hipSuccess && dl == 1 && m == (1u << IMPL_GENERIC);
    else if (variant == 4) ok = e == hipSuccess && dl >= 1 /* the remainder's launch at least */ && ((m >> IMPL_WGP) & 1u) && family_agrees(OP_WGRAD, impl, &a, m);
    else ok = e == hipErrorNotSupported && dl == 0 && m == 0;
    printf("REFUSE variant %d rc %d launches %ld mask %#x %s\n", variant, (int)e, dl, m, ok ? "ok" : "WRONG");
    bad += !ok;
  }
  hipDeviceSynchronize();
  return bad ? 1 : 0;
}

// ---- route: the executor's predicates over a table of records (built against a csrc that has none: the mode does not exist) ----
#ifdef DMM_EXECUTOR_PREDICATES
static int route_main() {
  static const char* const kinds[] = {"MEMSET", "CONVERT", "IGEMM", "WGRAD", "BNFIN", "BNBWD", "POOL", "POOLBWD", "BCE", "PACK", "UNPACK", "COPY", "APPLYCORR",
                                      "BW1", "JOIN", "BW1RED", "RAWFIN", "FIN64"};
  static const char* const batch[] = {"none", "W3", "RD"};
  static const char* const lanes[] = {"MAIN", "SIDE_CONTINUE", "SIDE_FORK", "PACK_FORK"};
  for (int kind = OP_MEMSET; kind <= OP_FIN64; ++kind)
    for (int leaf = 0; leaf < 4; ++leaf)
      for (int chain = 0; chain < 2; ++chain)
        for (int signal = -1; signal < 1; ++signal)
          for (int impl : {(int)IMPL_WG3, (int)IMPL_WG5})
            for (int epi = 0; epi < (kind == OP_JOIN ? 2 : 1); ++epi) {
              Op o;
              o.kind = kind; o.leaf = leaf; o.chain = chain; o.signal = signal; o.impl = impl; o.epi = epi;
              printf("R %s leaf=%d chain=%d signal=%d impl=%s epi=%d : forks=%d flushes=%d batch=%s,%s route=", kinds[kind], leaf, chain, signal,
                     impl == IMPL_WG3 ? "wg3" : "other", epi, (int)side_forks(o), (int)flushes_batches(o), batch[batch_kind(o, false)], batch[batch_kind(o, true)]);
              for (int m = 0; m < 8; ++m) printf("%s%s", m ? "," : "", lanes[route(o, (m & 4) != 0, (m & 2) != 0, (m & 1) != 0)]);   // (overlap, forked, batch_main)
              printf("\n");
            }
  return 0;
}
#endif

// ---- DRIVE_HIST: dmm_logit_hist (built against a csrc that has none: the case does not exist) ----
#ifdef DMM_HIST_MAX_THRESHOLDS
// Three shapes (a small one, one whose plane is no multiple of four, the C2 validation shape with 255 thresholds): logits and target
// are addresses only (reserved, PROT_NONE), counts is a heap block of exactly dmm_logit_hist_elems elements, so the runtime's
// memset is checked byte for byte.  Per shape: accumulate = 0 enqueues one memset of the whole block and one launch of the grid the
// launcher's rule gives, accumulate = 1 the launch alone and leaves the block as it is.  Then every refusal, each with nothing enqueued.
static int hist_main() {
  struct Shape { int B, NC, H, W, K; };
  const Shape shapes[3] = {{2, 3, 64, 96, 16}, {1, 1, 33, 35, 1}, {4, 3, 1280, 1920, 255}};
  float thr[DMM_HIST_MAX_THRESHOLDS + 1];
  for (int k = 0; k <= DMM_HIST_MAX_THRESHOLDS; ++k) thr[k] = -8.f + 0.0625f * k;
  int bad = 0;
  g_hist = HistWatch();
  g_hist.on = true;
  for (const Shape& s : shapes) {
    const size_t px = (size_t)s.B * s.NC * s.H * s.W, elems = dmm_logit_hist_elems(s.B, s.NC, s.K);
    const float* logits = (const float*)reserve(px * 4, PROT_NONE);
    const float* target = (const float*)reserve(px * 4, PROT_NONE);
    bool ok = elems == (size_t)s.B * s.NC * 2 * (s.K + 1);
    int64_t* counts = (int64_t*)malloc(elems * 8);
    memset(counts, 0x5a, elems * 8);
    const unsigned want_gx = (unsigned)logit_hist_grid_x(s.B * s.NC, (size_t)s.H * s.W);
    for (int acc = 0; acc < 2; ++acc) {
      if (acc) memset(counts, 0x5a, elems * 8);
      const HistWatch w0 = g_hist;
      MUST(dmm_logit_hist(logits, target, s.B, s.NC, s.H, s.W, thr, s.K, 0.7f, acc, counts, nullptr));
      ok = ok && g_hist.launches == w0.launches + 1 && g_hist.other == w0.other && g_hist.memsets == w0.memsets + (acc ? 0 : 1);
      ok = ok && g_hist.kernel.find("logit_hist_kernel") != std::string::npos && g_hist.gx == want_gx && g_hist.gy == (unsigned)(s.B * s.NC);
      ok = ok && want_gx >= 1 && (size_t)want_gx * 1024 < (size_t)s.H * s.W + 1024;   // no workgroup without a step of its own
      if (!acc) ok = ok && g_hist.memset_bytes == elems * 8;
      for (size_t i = 0; i < elems * 8; ++i) ok = ok && ((const unsigned char*)counts)[i] == (acc ? 0x5a : 0);
    }
    printf("HIST %d x %d x %d x %d K %d: grid %u x %u, %zu counts %s\n", s.B, s.NC, s.H, s.W, s.K, g_hist.gx, g_hist.gy, elems, ok ? "ok" : "WRONG");
    bad += !ok;
    free(counts);
  }
  // the refusals: nothing reaches the runtime, the message names the argument
  const float* x = (const float*)reserve(1 << 20, PROT_NONE);
  int64_t* c = (int64_t*)reserve(1 << 20, PROT_NONE);
  const HistWatch w0 = g_hist;
  auto refused = [&](int rc, const char* names) {
    if (rc == DMM_ERR_INVALID && strstr(dmm_last_error(), names) != nullptr) return;
    fprintf(stderr, "[drive] dmm_logit_hist: not refused (%d) or the message does not say '%s': %s\n", rc, names, dmm_last_error());
    ++bad;
  };
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
  refused(dmm_logit_hist(nullptr, x, 1, 1, 8, 8, thr, 4, 0.7f, 0, c, nullptr), "null");
  refused(dmm_logit_hist(x, nullptr, 1, 1, 8, 8, thr, 4, 0.7f, 0, c, nullptr), "null");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, nullptr, 4, 0.7f, 0, c, nullptr), "null");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, thr, 4, 0.7f, 0, nullptr, nullptr), "null");
  refused(dmm_logit_hist((const float*)((const char*)x + 2), x, 1, 1, 8, 8, thr, 4, 0.7f, 0, c, nullptr), "4-byte aligned");
  refused(dmm_logit_hist(x, (const float*)((const char*)x + 1), 1, 1, 8, 8, thr, 4, 0.7f, 0, c, nullptr), "4-byte aligned");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, thr, 4, 0.7f, 0, (int64_t*)((char*)c + 4), nullptr), "8-byte aligned");
  refused(dmm_logit_hist(x, x, 0, 1, 8, 8, thr, 4, 0.7f, 0, c, nullptr), ">= 1");
  refused(dmm_logit_hist(x, x, 1, 0, 8, 8, thr, 4, 0.7f, 0, c, nullptr), ">= 1");
  refused(dmm_logit_hist(x, x, 1, 1, 0, 8, thr, 4, 0.7f, 0, c, nullptr), ">= 1");
  refused(dmm_logit_hist(x, x, 1, 1, 8, -1, thr, 4, 0.7f, 0, c, nullptr), ">= 1");
  refused(dmm_logit_hist(x, x, 256, 256, 8, 8, thr, 4, 0.7f, 0, c, nullptr), "B * NC");
  refused(dmm_logit_hist(x, x, 1, 1, 65536, 32768, thr, 4, 0.7f, 0, c, nullptr), "H * W");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, thr, 0, 0.7f, 0, c, nullptr), "nthr");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, thr, DMM_HIST_MAX_THRESHOLDS + 1, 0.7f, 0, c, nullptr), "nthr");
  const float t_nan[3] = {0.f, nan, 2.f}, t_inf[3] = {0.f, 1.f, inf}, t_eq[3] = {0.f, 1.f, 1.f}, t_desc[3] = {0.f, 1.f, 0.5f};
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, t_nan, 3, 0.7f, 0, c, nullptr), "NaN or infinite");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, t_inf, 3, 0.7f, 0, c, nullptr), "NaN or infinite");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, t_eq, 3, 0.7f, 0, c, nullptr), "strictly ascending");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, t_desc, 3, 0.7f, 0, c, nullptr), "strictly ascending");
  refused(dmm_logit_hist(x, x, 1, 1, 8, 8, thr, 4, nan, 0, c, nullptr), "gt_threshold");
  if (g_hist.launches != w0.launches || g_hist.memsets != w0.memsets || g_hist.other != w0.other) { fprintf(stderr, "[drive] a refused dmm_logit_hist call reached the runtime\n"); ++bad; }
  if (dmm_logit_hist_elems(0, 3, 4) || dmm_logit_hist_elems(2, 0, 4) || dmm_logit_hist_elems(256, 256, 4) || dmm_logit_hist_elems(2, 3, 0) ||
      dmm_logit_hist_elems(2, 3, DMM_HIST_MAX_THRESHOLDS + 1) || dmm_logit_hist_elems(65535, 1, 255) != (size_t)65535 * 2 * 256) {
    fprintf(stderr, "[drive] dmm_logit_hist_elems\n"); ++bad;
  }
  g_hist.on = false;
  hipDeviceSynchronize();
  printf("%s\n", bad ? "HIST FAILED" : "HIST OK");
  return bad ? 1 : 0;
}
#endif

// ---- DRIVE_AUGMENT: dmm_augment_batch (built against a csrc that has none: the case does not exist) ----
#ifdef DMM_AUG_MAX_TENSORS
// One valid call: B = 33 samples of three tensors (3 + 1 + 3 channels, slices of one (33, 7, 37, 70) batch: addresses only) to 32 x 64
// outputs - two launches (32 samples, then 1) of the launcher's grid over all 7 channels.  Then every refusal, each with nothing enqueued.
static int augment_main() {
  int bad = 0;
  g_hist = HistWatch();
  g_hist.on = true;
  const int B = 33, Hs = 37, Ws = 70, Ho = 32, Wo = 64;
  const size_t sp = (size_t)Hs * Ws, dp = (size_t)Ho * Wo;
  float* src = (float*)reserve((size_t)B * 7 * sp * 4, PROT_NONE);
  float* dst = (float*)reserve((size_t)B * 7 * dp * 4, PROT_NONE);
  const dmm_aug_tensor good[3] = {{src, dst, (int64_t)(7 * sp), 3, 0},
                                  {src + 3 * sp, dst + (size_t)B * 3 * dp, (int64_t)(7 * sp), 1, 0},
                                  {src + 4 * sp, dst + (size_t)B * 4 * dp, (int64_t)(7 * sp), 3, 0}};
  std::vector<dmm_aug_sample> smp(B);
  for (int b = 0; b < B; ++b) {
    memset(&smp[b], 0, sizeof(dmm_aug_sample));
    smp[b].y0 = b % 7 - 3; smp[b].x0 = b % 11 - 5; smp[b].flip = b & 1;
    for (int c = 0; c < DMM_AUG_MAX_CHANNELS; ++c) { smp[b].gain[c] = c < 3 ? 1.f + 0.01f * b : 1.f; smp[b].bias[c] = 0.f; }
  }
  const float fill[DMM_AUG_MAX_CHANNELS] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
  {
    const HistWatch w0 = g_hist;
    MUST(dmm_augment_batch(good, 3, smp.data(), B, Hs, Ws, Ho, Wo, fill, nullptr));
    const bool ok = g_hist.launches == w0.launches + 2 && g_hist.memsets == w0.memsets && g_hist.other == w0.other &&
                    g_hist.kernel.find("augment_kernel") != std::string::npos && g_hist.gx == augment_grid_x(Ho, Wo) && g_hist.gx == 2 && g_hist.gy == 7;
    printf("AUGMENT %d samples: %ld launches, grid %u x %u %s\n", B, g_hist.launches - w0.launches, g_hist.gx, g_hist.gy, ok ? "ok" : "WRONG");
    bad += !ok;
  }
  const HistWatch w0 = g_hist;
  auto refused = [&](int rc, const char* names) {
    if (rc == DMM_ERR_INVALID && strstr(dmm_last_error(), names) != nullptr) return;
    fprintf(stderr, "[drive] dmm_augment_batch: not refused (%d) or the message does not say '%s': %s\n", rc, names, dmm_last_error());
    ++bad;
  };
  // one tensor / one sample changed at a time
  auto with_tensor = [&](int t, auto change, int nt = 3, int b = B, int hs = Hs, int ws = Ws, int ho = Ho, int wo = Wo) {
    dmm_aug_tensor T[3] = {good[0], good[1], good[2]};
    change(T[t]);
    return dmm_augment_batch(T, nt, smp.data(), b, hs, ws, ho, wo, fill, nullptr);
  };
  auto with_sample = [&](int b, auto change) {
    std::vector<dmm_aug_sample> s = smp;
    change(s[b]);
    return dmm_augment_batch(good, 3, s.data(), B, Hs, Ws, Ho, Wo, fill, nullptr);
  };
  auto same = [](dmm_aug_tensor&) {};
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
  refused(dmm_augment_batch(nullptr, 3, smp.data(), B, Hs, Ws, Ho, Wo, fill, nullptr), "null");
  refused(dmm_augment_batch(good, 3, nullptr, B, Hs, Ws, Ho, Wo, fill, nullptr), "null");
  refused(with_tensor(1, [](dmm_aug_tensor& T) { T.src = nullptr; }), "null src or dst");
  refused(with_tensor(2, [](dmm_aug_tensor& T) { T.dst = nullptr; }), "null src or dst");
  refused(with_tensor(0, same, 0), "ntensors");
  refused(with_tensor(0, same, DMM_AUG_MAX_TENSORS + 1), "ntensors");
  refused(with_tensor(1, [](dmm_aug_tensor& T) { T.channels = 0; }), "channels must be >= 1");
  refused(with_tensor(1, [](dmm_aug_tensor& T) { T.channels = 3; }), "sum to at most");
  refused(with_tensor(0, same, 3, 0), ">= 1");
  refused(with_tensor(0, same, 3, B, 0), ">= 1");
  refused(with_tensor(0, same, 3, B, Hs, -1), ">= 1");
  refused(with_tensor(0, same, 3, B, Hs, Ws, 0), ">= 1");
  refused(with_tensor(0, same, 3, B, Hs, Ws, Ho, 0), ">= 1");
  refused(with_tensor(0, same, 3, 1, 65536, 32768), "Hs * Ws");
  refused(with_tensor(0, same, 3, 1, Hs, Ws, 32768, 65536), "Ho * Wo");
  refused(with_tensor(0, [&](dmm_aug_tensor& T) { T.src_batch_stride = (int64_t)(3 * sp) - 1; }), "src_batch_stride");
  refused(with_tensor(2, [](dmm_aug_tensor& T) { T.src = (const float*)((const char*)T.src + 2); }), "4-byte aligned");
  refused(with_tensor(0, [](dmm_aug_tensor& T) { T.dst = (float*)((char*)T.dst + 1); }), "4-byte aligned");
  refused(with_tensor(1, [](dmm_aug_tensor& T) { T.reserved = 1; }), "reserved");
  refused(with_sample(32, [](dmm_aug_sample& s) { s.flip = 2; }), "flip");
  refused(with_sample(0, [](dmm_aug_sample& s) { s.flip = -1; }), "flip");
  refused(with_sample(5, [](dmm_aug_sample& s) { s.reserved = 7; }), "reserved");
  refused(with_sample(5, [](dmm_aug_sample& s) { s.y0 = (1 << 30) + 1; }), "2^30");
  refused(with_sample(5, [](dmm_aug_sample& s) { s.x0 = -(1 << 30) - 1; }), "2^30");
  refused(with_sample(32, [&](dmm_aug_sample& s) { s.gain[6] = nan; }), "NaN or infinite");
  refused(with_sample(1, [&](dmm_aug_sample& s) { s.bias[0] = -inf; }), "NaN or infinite");
  {
    float f[DMM_AUG_MAX_CHANNELS]; memcpy(f, fill, sizeof(f)); f[3] = inf;
    refused(dmm_augment_batch(good, 3, smp.data(), B, Hs, Ws, Ho, Wo, f, nullptr), "fill");
    f[3] = nan;
    refused(dmm_augment_batch(good, 3, smp.data(), B, Hs, Ws, Ho, Wo, f, nullptr), "fill");
  }
  // overlaps: in place, dst inside another tensor's src span (the last sample's planes), dst on another dst
  refused(with_tensor(0, [](dmm_aug_tensor& T) { T.dst = (float*)T.src; }), "overlaps src");
  refused(with_tensor(0, [&](dmm_aug_tensor& T) { T.dst = src + (size_t)(B - 1) * 7 * sp + 7 * sp - 1; }), "overlaps src");
  refused(with_tensor(1, [&](dmm_aug_tensor& T) { T.dst = dst + (size_t)B * 3 * dp - 1; }), "overlaps dst");
  // (an unused gain / bias entry and a null fill are fine, but those calls would launch: the GPU tests make them)
  if (g_hist.launches != w0.launches || g_hist.memsets != w0.memsets || g_hist.other != w0.other) { fprintf(stderr, "[drive] a refused dmm_augment_batch call reached the runtime\n"); ++bad; }
  g_hist.on = false;
  hipDeviceSynchronize();
  printf("%s\n", bad ? "AUGMENT FAILED" : "AUGMENT OK");
  return bad ? 1 : 0;
}
#endif

// ---- DRIVE_WARP: dmm_warp_batch (built against a csrc that has none: the case does not exist) ----
#ifdef DMM_WARP_LAUNCH_BATCH
// One valid call: B = 33 samples of three tensors (3 bilinear + 1 + 3 nearest channels, slices of one (33, 7, 37, 70) batch: addresses
// only) to 32 x 64 outputs - two launches (32 samples, then 1) of the launcher's grid over all 7 channels.  Then every refusal, each
// with nothing enqueued.
static int warp_main() {
  int bad = 0;
  g_hist = HistWatch();
  g_hist.on = true;
  const int B = 33, Hs = 37, Ws = 70, Ho = 32, Wo = 64;
  const size_t sp = (size_t)Hs * Ws, dp = (size_t)Ho * Wo;
  float* src = (float*)reserve((size_t)B * 7 * sp * 4, PROT_NONE);
  float* dst = (float*)reserve((size_t)B * 7 * dp * 4, PROT_NONE);
  const dmm_warp_tensor good[3] = {{src, dst, (int64_t)(7 * sp), 3, DMM_WARP_BILINEAR, {0, 0}},
                                   {src + 3 * sp, dst + (size_t)B * 3 * dp, (int64_t)(7 * sp), 1, DMM_WARP_NEAREST, {0, 0}},
                                   {src + 4 * sp, dst + (size_t)B * 4 * dp, (int64_t)(7 * sp), 3, DMM_WARP_NEAREST, {0, 0}}};
  const int32_t one = 1 << DMM_WARP_FRAC_BITS;
  std::vector<dmm_warp_sample> smp(B);
  for (int b = 0; b < B; ++b) {
    memset(&smp[b], 0, sizeof(dmm_warp_sample));
    smp[b].a00 = one - 1000 * b; smp[b].a01 = -777 * b; smp[b].a10 = 777 * b; smp[b].a11 = one - 1000 * b;
    smp[b].b0 = (int64_t)(b % 11 - 5) * one + 12345; smp[b].b1 = (int64_t)(b % 7 - 3) * one - 54321;
    for (int c = 0; c < DMM_AUG_MAX_CHANNELS; ++c) { smp[b].gain[c] = c < 3 ? 1.f + 0.01f * b : 1.f; smp[b].bias[c] = 0.f; }
  }
  const float fill[DMM_AUG_MAX_CHANNELS] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
  {
    const HistWatch w0 = g_hist;
    MUST(dmm_warp_batch(good, 3, smp.data(), B, Hs, Ws, Ho, Wo, fill, nullptr));
    const bool ok = g_hist.launches == w0.launches + 2 && g_hist.memsets == w0.memsets && g_hist.other == w0.other &&
                    g_hist.kernel.find("warp_kernel") != std::string::npos && g_hist.gx == warp_grid_x(Ho, Wo) && g_hist.gx == 2 && g_hist.gy == 7;
    printf("WARP %d samples: %ld launches, grid %u x %u %s\n", B, g_hist.launches - w0.launches, g_hist.gx, g_hist.gy, ok ? "ok" : "WRONG");
    bad += !ok;
  }
  const HistWatch w0 = g_hist;
  auto refused = [&](int rc, const char* names) {
    if (rc == DMM_ERR_INVALID && strstr(dmm_last_error(), names) != nullptr && strstr(dmm_last_error(), "dmm_warp_batch: ") == dmm_last_error()) return;
    fprintf(stderr, "[drive] dmm_warp_batch: not refused (%d) or the message does not say '%s': %s\n", rc, names, dmm_last_error());
    ++bad;
  };
  // one tensor / one sample changed at a time
  auto with_tensor = [&](int t, auto change, int nt = 3, int b = B, int hs = Hs, int ws = Ws, int ho = Ho, int wo = Wo) {
    dmm_warp_tensor T[3] = {good[0], good[1], good[2]};
    change(T[t]);
    return dmm_warp_batch(T, nt, smp.data(), b, hs, ws, ho, wo, fill, nullptr);
  };
  auto with_sample = [&](int b, auto change) {
    std::vector<dmm_warp_sample> s = smp;
    change(s[b]);
    return dmm_warp_batch(good, 3, s.data(), B, Hs, Ws, Ho, Wo, fill, nullptr);
  };
  auto same = [](dmm_warp_tensor&) {};
  const float nan = __builtin_nanf(""), inf = __builtin_inff();
  refused(dmm_warp_batch(nullptr, 3, smp.data(), B, Hs, Ws, Ho, Wo, fill, nullptr), "null");
  refused(dmm_warp_batch(good, 3, nullptr, B, Hs, Ws, Ho, Wo, fill, nullptr), "null");
  refused(with_tensor(1, [](dmm_warp_tensor& T) { T.src = nullptr; }), "null src or dst");
  refused(with_tensor(2, [](dmm_warp_tensor& T) { T.dst = nullptr; }), "null src or dst");
  refused(with_tensor(0, same, 0), "ntensors");
  refused(with_tensor(0, same, DMM_AUG_MAX_TENSORS + 1), "ntensors");
  refused(with_tensor(1, [](dmm_warp_tensor& T) { T.channels = 0; }), "channels must be >= 1");
  refused(with_tensor(1, [](dmm_warp_tensor& T) { T.channels = 3; }), "sum to at most");
  refused(with_tensor(0, same, 3, 0), ">= 1");
  refused(with_tensor(0, same, 3, B, 0), ">= 1");
  refused(with_tensor(0, same, 3, B, Hs, -1), ">= 1");
  refused(with_tensor(0, same, 3, B, Hs, Ws, 0), ">= 1");
  refused(with_tensor(0, same, 3, B, Hs, Ws, Ho, 0), ">= 1");
  refused(with_tensor(0, same, 3, 1, 65536, 32768), "Hs * Ws");
  refused(with_tensor(0, same, 3, 1, Hs, Ws, 32768, 65536), "Ho * Wo");
  refused(with_tensor(0, [&](dmm_warp_tensor& T) { T.src_batch_stride = (int64_t)(3 * sp) - 1; }), "src_batch_stride");
  refused(with_tensor(2, [](dmm_warp_tensor& T) { T.src = (const float*)((const char*)T.src + 2); }), "4-byte aligned");
  refused(with_tensor(0, [](dmm_warp_tensor& T) { T.dst = (float*)((char*)T.dst + 1); }), "4-byte aligned");
  refused(with_tensor(1, [](dmm_warp_tensor& T) { T.reserved[0] = 1; }), "reserved");
  refused(with_tensor(2, [](dmm_warp_tensor& T) { T.reserved[1] = -1; }), "reserved");
  refused(with_tensor(0, [](dmm_warp_tensor& T) { T.mode = 2; }), "mode");
  refused(with_tensor(2, [](dmm_warp_tensor& T) { T.mode = -1; }), "mode");
  refused(with_sample(32, [](dmm_warp_sample& s) { s.a00 = DMM_WARP_MAX_A + 1; }), "64 << 20");
  refused(with_sample(0, [](dmm_warp_sample& s) { s.a01 = -DMM_WARP_MAX_A - 1; }), "64 << 20");
  refused(with_sample(5, [](dmm_warp_sample& s) { s.a10 = INT32_MIN; }), "64 << 20");
  refused(with_sample(5, [](dmm_warp_sample& s) { s.a11 = INT32_MAX; }), "64 << 20");
  refused(with_sample(5, [](dmm_warp_sample& s) { s.b0 = DMM_WARP_MAX_B + 1; }), "2^50");
  refused(with_sample(32, [](dmm_warp_sample& s) { s.b1 = INT64_MIN; }), "2^50");
  refused(with_sample(32, [&](dmm_warp_sample& s) { s.gain[6] = nan; }), "NaN or infinite");
  refused(with_sample(1, [&](dmm_warp_sample& s) { s.bias[0] = -inf; }), "NaN or infinite");
  {
    float f[DMM_AUG_MAX_CHANNELS]; memcpy(f, fill, sizeof(f)); f[3] = inf;
    refused(dmm_warp_batch(good, 3, smp.data(), B, Hs, Ws, Ho, Wo, f, nullptr), "fill");
    f[3] = nan;
    refused(dmm_warp_batch(good, 3, smp.data(), B, Hs, Ws, Ho, Wo, f, nullptr), "fill");
  }
  // overlaps: in place, dst inside another tensor's src span (the last sample's planes), dst on another dst
  refused(with_tensor(0, [](dmm_warp_tensor& T) { T.dst = (float*)T.src; }), "overlaps src");
  refused(with_tensor(0, [&](dmm_warp_tensor& T) { T.dst = src + (size_t)(B - 1) * 7 * sp + 7 * sp - 1; }), "overlaps src");
  refused(with_tensor(1, [&](dmm_warp_tensor& T) { T.dst = dst + (size_t)B * 3 * dp - 1; }), "overlaps dst");
  if (g_hist.launches != w0.launches || g_hist.memsets != w0.memsets || g_hist.other != w0.other) { fprintf(stderr, "[drive] a refused dmm_warp_batch call reached the runtime\n"); ++bad; }
  g_hist.on = false;
  hipDeviceSynchronize();
  printf("%s\n", bad ? "WARP FAILED" : "WARP OK");
  return bad ? 1 : 0;
}
#endif

// ---- DRIVE_COMPONENTS: dmm_heat_components (built against a csrc that has none: the case does not exist) ----
#ifdef DMM_CC_TILE_H
// Three shapes: a plane smaller than a tile, one ragged in both directions, many planes.  maps, labels, records, counts and the
// workspace are addresses only (reserved, PROT_NONE): the call uploads nothing, clears nothing and touches none of them on the host.
// Per shape, with and without a labels array: seven launches and nothing else, each grid (x, B * NC) against the tiling restated here,
// and the two arrays the call carves from its workspace inside dmm_heat_components_workspace bytes.  Then every refusal.
static int components_main() {
  struct Shape { int B, NC, H, W, cap; };
  const Shape shapes[3] = {{1, 1, 7, 9, 16}, {2, 3, 3 * DMM_CC_TILE_H + 5, 2 * DMM_CC_TILE_W + 3, 1024}, {64, 300, 40, 50, 300}};
  const char* names[CC_LAUNCHES] = {"cc_local_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_scan_kernel", "cc_slots_kernel",
                                    "cc_stats_kernel", "cc_finish_kernel"};
  int bad = 0;
  g_hist = HistWatch();
  g_hist.on = true;
  for (const Shape& s : shapes) {
    const size_t planes = (size_t)s.B * s.NC, plane = (size_t)s.H * s.W, px = planes * plane;
    const size_t wsb = dmm_heat_components_workspace(s.B, s.NC, s.H, s.W, s.cap);
    const size_t tiles = (size_t)((s.H + DMM_CC_TILE_H - 1) / DMM_CC_TILE_H) * ((s.W + DMM_CC_TILE_W - 1) / DMM_CC_TILE_W);
    const size_t nseg = (plane + CC_SEG - 1) / CC_SEG;
    const unsigned want[CC_LAUNCHES] = {(unsigned)tiles, (unsigned)tiles, (unsigned)nseg, 1u, (unsigned)nseg, (unsigned)tiles, (unsigned)((s.cap + 255) / 256)};
    // the carve-up: labels at 0, the segment counts behind them, both 16-byte aligned, the end inside the workspace
    const ComponentsLayout lay = components_layout((int)planes, plane);
    bool ok = wsb != 0 && lay.total == wsb && lay.labels == 0 && lay.labels % 16 == 0 && lay.seg % 16 == 0 && lay.seg >= px * 4 &&
              lay.seg + planes * nseg * 4 <= wsb;
    const float* maps = (const float*)reserve(px * 4, PROT_NONE);
    int32_t* labels = (int32_t*)reserve(px * 4, PROT_NONE);
    dmm_component* records = (dmm_component*)reserve(planes * s.cap * sizeof(dmm_component), PROT_NONE);
    int32_t* counts = (int32_t*)reserve(planes * 4, PROT_NONE);
    void* ws = reserve(wsb, PROT_NONE);
    for (int with_labels = 0; with_labels < 2; ++with_labels) {
      const HistWatch w0 = g_hist;
      g_launch_log.clear();
      MUST(dmm_heat_components(maps, s.B, s.NC, s.H, s.W, 0.7f, with_labels ? 8 : 4, s.cap, ws, wsb, with_labels ? labels : nullptr, records, counts, nullptr));
      ok = ok && g_hist.launches == w0.launches + CC_LAUNCHES && g_hist.memsets == w0.memsets && g_hist.other == w0.other && g_launch_log.size() == (size_t)CC_LAUNCHES;
      for (int k = 0; ok && k < CC_LAUNCHES; ++k)
        ok = g_launch_log[k].kernel.find(names[k]) != std::string::npos && g_launch_log[k].gx == want[k] && g_launch_log[k].gy == (unsigned)planes;
    }
    printf("COMPONENTS %d x %d x %d x %d cap %d: %zu tiles, %zu segments, workspace %zu %s\n", s.B, s.NC, s.H, s.W, s.cap, tiles, nseg, wsb, ok ? "ok" : "WRONG");
    bad += !ok;
  }
  // the refusals: nothing reaches the runtime, the message names the argument
  const float* x = (const float*)reserve(1 << 20, PROT_NONE);
  int32_t* lab = (int32_t*)reserve(1 << 20, PROT_NONE);
  dmm_component* rec = (dmm_component*)reserve(1 << 20, PROT_NONE);
  int32_t* cnt = (int32_t*)reserve(1 << 20, PROT_NONE);
  void* ws = reserve(1 << 20, PROT_NONE);
  const size_t wsb = dmm_heat_components_workspace(1, 1, 8, 8, 4);
  const HistWatch w0 = g_hist;
  auto refused = [&](int rc, const char* names) {
    if (rc == DMM_ERR_INVALID && strncmp(dmm_last_error(), "dmm_heat_components: ", 21) == 0 && strstr(dmm_last_error(), names) != nullptr) return;
    fprintf(stderr, "[drive] dmm_heat_components: not refused (%d) or the message does not say '%s': %s\n", rc, names, dmm_last_error());
    ++bad;
  };
  auto off = [](auto* p, int bytes) { return (decltype(p))((char*)p + bytes); };
  const float nan = __builtin_nanf("");
  refused(dmm_heat_components(nullptr, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), "null");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, nullptr, wsb, lab, rec, cnt, nullptr), "null");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, nullptr, cnt, nullptr), "null");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, nullptr, nullptr), "null");
  refused(dmm_heat_components(off(x, 2), 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), "4-byte aligned");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, off(lab, 1), rec, cnt, nullptr), "4-byte aligned");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, off(cnt, 2), nullptr), "4-byte aligned");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, off(rec, 4), cnt, nullptr), "8-byte aligned");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, off(ws, 8), wsb, lab, rec, cnt, nullptr), "16-byte aligned");
  refused(dmm_heat_components(x, 0, 1, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), ">= 1");
  refused(dmm_heat_components(x, 1, 0, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), ">= 1");
  refused(dmm_heat_components(x, 1, 1, 0, 8, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), ">= 1");
  refused(dmm_heat_components(x, 1, 1, 8, -1, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), ">= 1");
  refused(dmm_heat_components(x, 256, 256, 8, 8, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), "B * NC");
  refused(dmm_heat_components(x, 1, 1, 65536, 32768, 0.f, 8, 4, ws, wsb, lab, rec, cnt, nullptr), "H * W");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 6, 4, ws, wsb, lab, rec, cnt, nullptr), "connectivity");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 0, 4, ws, wsb, lab, rec, cnt, nullptr), "connectivity");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 0, ws, wsb, lab, rec, cnt, nullptr), "max_per_plane");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, DMM_CC_MAX_PER_PLANE + 1, ws, wsb, lab, rec, cnt, nullptr), "max_per_plane");
  refused(dmm_heat_components(x, 1, 1, 8, 8, nan, 8, 4, ws, wsb, lab, rec, cnt, nullptr), "threshold is NaN");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, wsb - 1, lab, rec, cnt, nullptr), "workspace_bytes");
  refused(dmm_heat_components(x, 1, 1, 8, 8, 0.f, 8, 4, ws, 0, lab, rec, cnt, nullptr), "workspace_bytes");
  if (g_hist.launches != w0.launches || g_hist.memsets != w0.memsets || g_hist.other != w0.other) { fprintf(stderr, "[drive] a refused dmm_heat_components call reached the runtime\n"); ++bad; }
  if (wsb == 0 || dmm_heat_components_workspace(0, 1, 8, 8, 4) || dmm_heat_components_workspace(1, 1, 8, 0, 4) || dmm_heat_components_workspace(256, 256, 8, 8, 4) ||
      dmm_heat_components_workspace(1, 1, 65536, 32768, 4) || dmm_heat_components_workspace(1, 1, 8, 8, 0) || dmm_heat_components_workspace(1, 1, 8, 8, DMM_CC_MAX_PER_PLANE + 1)) {
    fprintf(stderr, "[drive] dmm_heat_components_workspace\n"); ++bad;
  }
  g_hist.on = false;
  hipDeviceSynchronize();
  printf("%s\n", bad ? "COMPONENTS FAILED" : "COMPONENTS OK");
  return bad ? 1 : 0;
}
#endif

// ---- DRIVE_PREPARE: dmm_prep_image / dmm_prep_lidar / dmm_prep_heat_maps (built against a csrc that has none: the case does not exist) ----
#ifdef DMM_PREP_LAUNCH_BATCH
// B = 1, 33 and 65 samples of 40 x 30 at pool 10 and 1, the three outputs slices of one (B, 7, Ho, Wo) batch.  src, points, boxes and dst
// are addresses only; the LiDAR workspace is real memory of exactly dmm_prep_lidar_workspace bytes with a guard band behind it, because
// the runtime's memset does run here: it must set B * H * W * 4 bytes to 0xFF and nothing behind them.  Per call the launches are
// counted and each grid is held against a restatement.  Samples 33 and up have no points: a chunk without points makes no splat launch.
// Then every refusal of the three entry points, each with nothing enqueued.
static int prepare_main() {
  int bad = 0;
  g_hist = HistWatch();
  g_hist.on = true;
  const int H = 40, W = 30, C = 3, K = 5;
  for (int B : {1, 33, 65})
    for (int p : {10, 1}) {
      const int Ho = H / p, Wo = W / p, chunks = (B + DMM_PREP_LAUNCH_BATCH - 1) / DMM_PREP_LAUNCH_BATCH;
      const size_t plane = (size_t)Ho * Wo;
      const uint8_t* src = (const uint8_t*)reserve((size_t)B * H * W * C, PROT_NONE);
      float* dst = (float*)reserve((size_t)B * 7 * plane * 4, PROT_NONE);
      std::vector<int32_t> po(B + 1), bo(B + 1);
      for (int b = 0; b <= B; ++b) { po[b] = 7 * std::min(b, 33); bo[b] = 3 * b; }   // samples 33 .. 64 have no points: the third chunk has none
      const float* pts = (const float*)reserve((size_t)po[B] * 12 + 4096, PROT_NONE);
      const dmm_prep_box* boxes = (const dmm_prep_box*)reserve((size_t)bo[B] * sizeof(dmm_prep_box) + 4096, PROT_NONE);
      const size_t wsb = dmm_prep_lidar_workspace(B, H, W);
      bool ok = wsb == ((size_t)B * H * W * 4 + 15) / 16 * 16;
      unsigned char* ws = (unsigned char*)aligned_alloc(16, wsb + 64);
      memset(ws, 0x5a, wsb + 64);
      {
        const HistWatch w0 = g_hist;
        g_launch_log.clear();
        MUST(dmm_prep_image(src, (int64_t)H * W * C, dst, (int64_t)(7 * plane), B, H, W, C, p, nullptr));
        ok = ok && g_hist.launches == w0.launches + chunks && g_hist.memsets == w0.memsets && g_hist.other == w0.other;
        for (const LaunchSeen& l : g_launch_log)
          ok = ok && l.kernel.find("prep_image_kernel") != std::string::npos && l.gx == (unsigned)((plane + 255) / 256) && l.gx == prep_plane_grid_x(Ho, Wo) && l.gy == (unsigned)C;
      }
      {
        const HistWatch w0 = g_hist;
        g_launch_log.clear();
        MUST(dmm_prep_lidar(pts, po.data(), dst + 3 * plane, (int64_t)(7 * plane), B, H, W, p, K, ws, wsb, nullptr));
        int splats = 0;   // chunks that own a point
        for (int b0 = 0; b0 < B; b0 += DMM_PREP_LAUNCH_BATCH) splats += po[std::min(B, b0 + DMM_PREP_LAUNCH_BATCH)] > po[b0];
        ok = ok && g_hist.launches == w0.launches + chunks + splats && g_hist.memsets == w0.memsets + 1 && g_hist.other == w0.other &&
             g_hist.memset_bytes == (unsigned long long)B * H * W * 4 && splats == std::min(chunks, 2);
        size_t n = 0;
        for (int b0 = 0; b0 < B && ok; b0 += DMM_PREP_LAUNCH_BATCH) {
          const int nb = std::min(DMM_PREP_LAUNCH_BATCH, B - b0), np = po[b0 + nb] - po[b0];
          if (np > 0) {
            ok = ok && n < g_launch_log.size() && g_launch_log[n].kernel.find("prep_lidar_splat_kernel") != std::string::npos &&
                 g_launch_log[n].gx == (unsigned)(((size_t)np * K * K + 255) / 256) && g_launch_log[n].gx == prep_splat_grid_x(np, K);
            ++n;
          }
          ok = ok && n < g_launch_log.size() && g_launch_log[n].kernel.find("prep_lidar_pool_kernel") != std::string::npos &&
               g_launch_log[n].gx == prep_plane_grid_x(Ho, Wo) && g_launch_log[n].gy == (unsigned)nb;
          ++n;
        }
        // the carve-up: the owner planes fill the front of the workspace, the guard band behind workspace_bytes is untouched
        for (size_t i = 0; i < (size_t)B * H * W * 4; ++i) ok = ok && ws[i] == 0xFF;
        for (size_t i = wsb; i < wsb + 64; ++i) ok = ok && ws[i] == 0x5a;
      }
      {
        const HistWatch w0 = g_hist;
        g_launch_log.clear();
        MUST(dmm_prep_heat_maps(boxes, bo.data(), dst + 4 * plane, (int64_t)(7 * plane), B, H, W, p, nullptr));
        ok = ok && g_hist.launches == w0.launches + chunks && g_hist.memsets == w0.memsets && g_hist.other == w0.other;
        const unsigned tiles = (unsigned)((Ho + 15) / 16) * (unsigned)((Wo + 15) / 16);
        int b0 = 0;
        for (const LaunchSeen& l : g_launch_log) {
          ok = ok && l.kernel.find("prep_heat_kernel") != std::string::npos && l.gx == tiles && l.gx == prep_heat_grid_x(Ho, Wo) &&
               l.gy == (unsigned)std::min(DMM_PREP_LAUNCH_BATCH, B - b0);
          b0 += DMM_PREP_LAUNCH_BATCH;
        }
      }
      printf("PREPARE %d samples pool %d: workspace %zu %s\n", B, p, wsb, ok ? "ok" : "WRONG");
      bad += !ok;
      free(ws);
    }
  // the refusals: nothing reaches the runtime, the message starts with the entry point's name and names the argument
  const uint8_t* src = (const uint8_t*)reserve(1 << 20, PROT_NONE);
  float* dst = (float*)reserve(1 << 20, PROT_NONE);
  const float* pts = (const float*)reserve(1 << 20, PROT_NONE);
  const dmm_prep_box* bx = (const dmm_prep_box*)reserve(1 << 20, PROT_NONE);
  void* ws = reserve(1 << 20, PROT_NONE);
  const int32_t off[3] = {0, 2, 5}, off_first[3] = {1, 2, 5}, off_desc[3] = {0, 3, 2}, off_big[3] = {0, 2, DMM_PREP_MAX_ITEMS + 1};
  const size_t wsb = dmm_prep_lidar_workspace(2, 40, 30);
  const HistWatch w0 = g_hist;
  const char* who = "";
  auto refused = [&](int rc, const char* names) {
    if (rc == DMM_ERR_INVALID && strncmp(dmm_last_error(), who, strlen(who)) == 0 && strstr(dmm_last_error(), names) != nullptr) return;
    fprintf(stderr, "[drive] %snot refused (%d) or the message does not say '%s': %s\n", who, rc, names, dmm_last_error());
    ++bad;
  };
  auto off_by = [](auto* p, int bytes) { return (decltype(p))((char*)p + bytes); };
  who = "dmm_prep_image: ";
  refused(dmm_prep_image(nullptr, 3600, dst, 36, 2, 40, 30, 3, 10, nullptr), "null");
  refused(dmm_prep_image(src, 3600, nullptr, 36, 2, 40, 30, 3, 10, nullptr), "null");
  refused(dmm_prep_image(src, 3600, off_by(dst, 2), 36, 2, 40, 30, 3, 10, nullptr), "4-byte aligned");
  refused(dmm_prep_image(src, 3600, dst, 36, 0, 40, 30, 3, 10, nullptr), ">= 1");
  refused(dmm_prep_image(src, 3600, dst, 36, 2, 0, 30, 3, 10, nullptr), ">= 1");
  refused(dmm_prep_image(src, 3600, dst, 36, 2, 40, -30, 3, 10, nullptr), ">= 1");
  refused(dmm_prep_image(src, 3600, dst, 36, 2, 40, 30, 3, 0, nullptr), ">= 1");
  refused(dmm_prep_image(src, 3600, dst, 36, 2, 45, 30, 3, 10, nullptr), "multiples of pool");
  refused(dmm_prep_image(src, 3600, dst, 36, 2, 40, 35, 3, 10, nullptr), "multiples of pool");
  refused(dmm_prep_image(src, 1ll << 33, dst, 1ll << 33, 1, 65536, 32768, 3, 1, nullptr), "H * W");
  refused(dmm_prep_image(src, 3600, dst, 36, 2, 40, 30, 0, 10, nullptr), "C must be");
  refused(dmm_prep_image(src, 6000, dst, 60, 2, 40, 30, 5, 10, nullptr), "C must be");
  refused(dmm_prep_image(src, 3599, dst, 36, 2, 40, 30, 3, 10, nullptr), "src_batch_stride");
  refused(dmm_prep_image(src, 3600, dst, 35, 2, 40, 30, 3, 10, nullptr), "dst_batch_stride");
  who = "dmm_prep_lidar: ";
  refused(dmm_prep_lidar(nullptr, off, dst, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "null points");
  refused(dmm_prep_lidar(pts, nullptr, dst, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "null");
  refused(dmm_prep_lidar(pts, off, nullptr, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "null");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, 5, nullptr, wsb, nullptr), "null");
  refused(dmm_prep_lidar(off_by(pts, 2), off, dst, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "4-byte aligned");
  refused(dmm_prep_lidar(pts, off, off_by(dst, 1), 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "4-byte aligned");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, 5, off_by(ws, 8), wsb, nullptr), "16-byte aligned");
  refused(dmm_prep_lidar(pts, off, dst, 12, 0, 40, 30, 10, 5, ws, wsb, nullptr), ">= 1");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 0, 10, 5, ws, wsb, nullptr), ">= 1");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, -1, 5, ws, wsb, nullptr), ">= 1");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 33, 10, 5, ws, wsb, nullptr), "multiples of pool");
  refused(dmm_prep_lidar(pts, off, dst, 3, 2, 10, 30, 10, 5, ws, wsb, nullptr), "2 * pool");
  refused(dmm_prep_lidar(pts, off, dst, 1ll << 33, 1, 65536, 32768, 1, 5, ws, wsb, nullptr), "H * W");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, 4, ws, wsb, nullptr), "kernel_size");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, 17, ws, wsb, nullptr), "kernel_size");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, -1, ws, wsb, nullptr), "kernel_size");
  refused(dmm_prep_lidar(pts, off, dst, 11, 2, 40, 30, 10, 5, ws, wsb, nullptr), "dst_batch_stride");
  refused(dmm_prep_lidar(pts, off_first, dst, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "offsets[0]");
  refused(dmm_prep_lidar(pts, off_desc, dst, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "must not decrease");
  refused(dmm_prep_lidar(pts, off_big, dst, 12, 2, 40, 30, 10, 5, ws, wsb, nullptr), "2^31 / 256");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, 5, ws, wsb - 1, nullptr), "workspace_bytes");
  refused(dmm_prep_lidar(pts, off, dst, 12, 2, 40, 30, 10, 5, ws, 0, nullptr), "workspace_bytes");
  who = "dmm_prep_heat_maps: ";
  refused(dmm_prep_heat_maps(nullptr, off, dst, 36, 2, 40, 30, 10, nullptr), "null boxes");
  refused(dmm_prep_heat_maps(bx, nullptr, dst, 36, 2, 40, 30, 10, nullptr), "null");
  refused(dmm_prep_heat_maps(bx, off, nullptr, 36, 2, 40, 30, 10, nullptr), "null");
  refused(dmm_prep_heat_maps(off_by(bx, 2), off, dst, 36, 2, 40, 30, 10, nullptr), "4-byte aligned");
  refused(dmm_prep_heat_maps(bx, off, off_by(dst, 3), 36, 2, 40, 30, 10, nullptr), "4-byte aligned");
  refused(dmm_prep_heat_maps(bx, off, dst, 36, -2, 40, 30, 10, nullptr), ">= 1");
  refused(dmm_prep_heat_maps(bx, off, dst, 36, 2, 0, 30, 10, nullptr), ">= 1");
  refused(dmm_prep_heat_maps(bx, off, dst, 36, 2, 40, 30, 0, nullptr), ">= 1");
  refused(dmm_prep_heat_maps(bx, off, dst, 36, 2, 40, 30, 7, nullptr), "multiples of pool");
  refused(dmm_prep_heat_maps(bx, off, dst, 1ll << 34, 1, 65536, 32768, 1, nullptr), "H * W");
  refused(dmm_prep_heat_maps(bx, off, dst, 35, 2, 40, 30, 10, nullptr), "dst_batch_stride");
  refused(dmm_prep_heat_maps(bx, off_first, dst, 36, 2, 40, 30, 10, nullptr), "offsets[0]");
  refused(dmm_prep_heat_maps(bx, off_desc, dst, 36, 2, 40, 30, 10, nullptr), "must not decrease");
  refused(dmm_prep_heat_maps(bx, off_big, dst, 36, 2, 40, 30, 10, nullptr), "2^31 / 256");
  if (g_hist.launches != w0.launches || g_hist.memsets != w0.memsets || g_hist.other != w0.other) { fprintf(stderr, "[drive] a refused dmm_prep_* call reached the runtime\n"); ++bad; }
  if (wsb != 2 * 40 * 30 * 4 || dmm_prep_lidar_workspace(0, 8, 8) || dmm_prep_lidar_workspace(1, 0, 8) || dmm_prep_lidar_workspace(1, 8, -8) ||
      dmm_prep_lidar_workspace(1, 65536, 32768) || dmm_prep_lidar_workspace(1, 3, 1) != 16) {
    fprintf(stderr, "[drive] dmm_prep_lidar_workspace\n"); ++bad;
  }
  g_hist.on = false;
  hipDeviceSynchronize();
  printf("%s\n", bad ? "PREPARE FAILED" : "PREPARE OK");
  return bad ? 1 : 0;
}
#endif

// ---- DRIVE_MATCH: dmm_match_objects (built against a csrc that has none: the case does not exist) ----
#ifdef DMM_MATCH_MAX_PER_PLANE
// Three shapes: one plane, a small batch at the detector's default cap, and B * NC at the entry point's own limit (there is no
// per-launch plane cap to go past: a plane is a workgroup of a one-dimensional grid).  Records, counts, matched, totals and entries
// are addresses only (reserved, PROT_NONE): the call uploads nothing, clears nothing and touches none of them on the host.  The
// workspace is real memory of exactly dmm_match_objects_workspace bytes between two guard bands, which the host code must leave as
// they are, workspace included.  Per shape, with and without `matched`: three launches and nothing else, each grid against the
// restatement here, and the three arrays the call carves from its workspace inside the query's bytes.  Then every refusal.
static int match_main() {
  struct Shape { int B, NC, cap_pred, cap_gt; };
  const Shape shapes[3] = {{1, 1, 1, 1}, {4, 3, 1024, 1000}, {21845, 3, DMM_MATCH_MAX_PER_PLANE, 7}};
  const char* names[MATCH_LAUNCHES] = {"match_count_kernel", "match_offsets_kernel", "match_plane_kernel"};
  int bad = 0;
  g_hist = HistWatch();
  g_hist.on = true;
  for (const Shape& s : shapes) {
    const size_t planes = (size_t)s.B * s.NC;
    const size_t wsb = dmm_match_objects_workspace(s.B, s.NC, s.cap_pred, s.cap_gt);
    const unsigned want[MATCH_LAUNCHES] = {(unsigned)planes, (unsigned)s.NC, (unsigned)planes};
    const MatchLayout lay = match_layout((int)planes);
    bool ok = wsb != 0 && lay.total == wsb && lay.np == 0 && lay.ng % 16 == 0 && lay.base % 16 == 0 && lay.ng >= planes * 4 &&
              lay.base >= lay.ng + planes * 4 && lay.base + planes * 8 <= wsb;
    const int64_t capacity = 1 << 20;
    const dmm_component* pred = (const dmm_component*)reserve(planes * s.cap_pred * sizeof(dmm_component), PROT_NONE);
    const dmm_component* gt = (const dmm_component*)reserve(planes * s.cap_gt * sizeof(dmm_component), PROT_NONE);
    const int32_t* pc = (const int32_t*)reserve(planes * 4, PROT_NONE);
    const int32_t* gc = (const int32_t*)reserve(planes * 4, PROT_NONE);
    uint8_t* matched = (uint8_t*)reserve(planes * s.cap_pred, PROT_NONE);
    int64_t* totals = (int64_t*)reserve((size_t)s.NC * 64, PROT_NONE);
    int32_t* entries = (int32_t*)reserve((size_t)s.NC * capacity * 8, PROT_NONE);
    unsigned char* block = (unsigned char*)aligned_alloc(16, 64 + wsb + 64);
    memset(block, 0x5a, 64 + wsb + 64);
    for (int with_matched = 0; with_matched < 2; ++with_matched) {
      const HistWatch w0 = g_hist;
      g_launch_log.clear();
      MUST(dmm_match_objects(pred, pc, s.cap_pred, gt, gc, s.cap_gt, s.B, s.NC, 1, 0.5, block + 64, wsb, with_matched ? matched : nullptr, totals, entries,
                             capacity, nullptr));
      ok = ok && g_hist.launches == w0.launches + MATCH_LAUNCHES && g_hist.memsets == w0.memsets && g_hist.other == w0.other && g_launch_log.size() == (size_t)MATCH_LAUNCHES;
      for (int k = 0; ok && k < MATCH_LAUNCHES; ++k)
        ok = g_launch_log[k].kernel.find(names[k]) != std::string::npos && g_launch_log[k].gx == want[k] && g_launch_log[k].gy == 1u;
    }
    for (size_t i = 0; i < 64 + wsb + 64; ++i) ok = ok && block[i] == 0x5a;
    printf("MATCH %d x %d caps %d / %d: %zu planes, workspace %zu %s\n", s.B, s.NC, s.cap_pred, s.cap_gt, planes, wsb, ok ? "ok" : "WRONG");
    bad += !ok;
    free(block);
  }
  // the refusals: nothing reaches the runtime, the message names the argument
  const dmm_component* p = (const dmm_component*)reserve(1 << 20, PROT_NONE);
  const dmm_component* g = (const dmm_component*)reserve(1 << 20, PROT_NONE);
  const int32_t* pc = (const int32_t*)reserve(1 << 20, PROT_NONE);
  const int32_t* gc = (const int32_t*)reserve(1 << 20, PROT_NONE);
  uint8_t* m = (uint8_t*)reserve(1 << 20, PROT_NONE);
  int64_t* tot = (int64_t*)reserve(1 << 20, PROT_NONE);
  int32_t* ent = (int32_t*)reserve(1 << 20, PROT_NONE);
  void* ws = reserve(1 << 20, PROT_NONE);
  const size_t wsb = dmm_match_objects_workspace(2, 3, 8, 8);
  const HistWatch w0 = g_hist;
  auto refused = [&](int rc, const char* names) {
    if (rc == DMM_ERR_INVALID && strncmp(dmm_last_error(), "dmm_match_objects: ", 19) == 0 && strstr(dmm_last_error(), names) != nullptr) return;
    fprintf(stderr, "[drive] dmm_match_objects: not refused (%d) or the message does not say '%s': %s\n", rc, names, dmm_last_error());
    ++bad;
  };
  auto off = [](auto* q, int bytes) { return (decltype(q))((char*)q + bytes); };
  const double nan = __builtin_nan("");
  refused(dmm_match_objects(nullptr, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "null");
  refused(dmm_match_objects(p, nullptr, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "null");
  refused(dmm_match_objects(p, pc, 8, nullptr, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "null");
  refused(dmm_match_objects(p, pc, 8, g, nullptr, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "null");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, nullptr, wsb, m, tot, ent, 100, nullptr), "null");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, nullptr, ent, 100, nullptr), "null");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, nullptr, 100, nullptr), "null");
  refused(dmm_match_objects(off(p, 4), pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "records must be 8-byte aligned");
  refused(dmm_match_objects(p, pc, 8, off(g, 4), gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "records must be 8-byte aligned");
  refused(dmm_match_objects(p, off(pc, 2), 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "counts must be 4-byte aligned");
  refused(dmm_match_objects(p, pc, 8, g, off(gc, 1), 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "counts must be 4-byte aligned");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, off(tot, 4), ent, 100, nullptr), "totals must be 8-byte aligned");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, off(ent, 2), 100, nullptr), "entries must be 4-byte aligned");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, off(ws, 8), wsb, m, tot, ent, 100, nullptr), "workspace must be 16-byte aligned");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 0, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), ">= 1");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, -3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), ">= 1");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 256, 256, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "B * NC");
  refused(dmm_match_objects(p, pc, 0, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "DMM_MATCH_MAX_PER_PLANE");
  refused(dmm_match_objects(p, pc, 8, g, gc, -1, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "DMM_MATCH_MAX_PER_PLANE");
  refused(dmm_match_objects(p, pc, DMM_MATCH_MAX_PER_PLANE + 1, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "DMM_MATCH_MAX_PER_PLANE");
  refused(dmm_match_objects(p, pc, 8, g, gc, DMM_CC_MAX_PER_PLANE, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "65536");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 0, 0.5, ws, wsb, m, tot, ent, 100, nullptr), "min_area");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.0, ws, wsb, m, tot, ent, 100, nullptr), "iou");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, -0.5, ws, wsb, m, tot, ent, 100, nullptr), "iou");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 1.0000001, ws, wsb, m, tot, ent, 100, nullptr), "iou");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, nan, ws, wsb, m, tot, ent, 100, nullptr), "iou");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 0, nullptr), "capacity");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb, m, tot, ent, 1ll << 31, nullptr), "capacity");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, wsb - 1, m, tot, ent, 100, nullptr), "workspace_bytes");
  refused(dmm_match_objects(p, pc, 8, g, gc, 8, 2, 3, 1, 0.5, ws, 0, m, tot, ent, 100, nullptr), "workspace_bytes");
  if (g_hist.launches != w0.launches || g_hist.memsets != w0.memsets || g_hist.other != w0.other) { fprintf(stderr, "[drive] a refused dmm_match_objects call reached the runtime\n"); ++bad; }
  if (wsb != 32 + 32 + 48 || dmm_match_objects_workspace(0, 1, 8, 8) || dmm_match_objects_workspace(1, 0, 8, 8) || dmm_match_objects_workspace(256, 256, 8, 8) ||
      dmm_match_objects_workspace(1, 1, 0, 8) || dmm_match_objects_workspace(1, 1, 8, DMM_MATCH_MAX_PER_PLANE + 1) || !dmm_match_objects_workspace(1, 1, DMM_MATCH_MAX_PER_PLANE, 1)) {
    fprintf(stderr, "[drive] dmm_match_objects_workspace\n"); ++bad;
  }
  g_hist.on = false;
  hipDeviceSynchronize();
  printf("%s\n", bad ? "MATCH FAILED" : "MATCH OK");
  return bad ? 1 : 0;
}
#endif

int main(int argc, char** argv) {
  g_enqueue.on =getenv("DRIVE_TRACE_ENQUEUE") != nullptr;
  fakehip_set_hook(drive_hook);
  if (const char* off = getenv("DRIVE_OPTIONS_OFF")) {   // before any plan exists, in every mode
    const std::string s = off;
    for (size_t b = 0, e; b <= s.size(); b = e + 1) {
      e = std::min(s.find(',', b), s.size());
      if (e > b) MUST(dmm_set_option(s.substr(b, e - b).c_str(), 0));
    }
  }
  if (const char* v = getenv("DRIVE_BATCH_WGRAD")) MUST(dmm_set_option("batch_wgrad", atoi(v)));
  if (argc > 1 && std::string(argv[1]) == "picks") return picks_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "dump") return dump_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "single") return single_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "refuse") return refuse_main();
  if (argc > 1 && std::string(argv[1]) == "accum") return accum_main(argc, argv);
#ifdef DMM_EXECUTOR_PREDICATES
  if (argc > 1 && std::string(argv[1]) == "route") return route_main();
#endif
  if (argc < 6) { fprintf(stderr, "usage: drive <arch> <dtype> <batch> <H> <W> [lives]\n"); return 64; }
  dmm_model_desc d;
  if (!fill_desc(argv[1], d)) { fprintf(stderr, "unknown arch %s\n", argv[1]); return 64; }
  const std::string dt = argv[2];
  d.dtype = dt == "f32" ? DMM_F32 : (dt == "f16" ? DMM_F16 : DMM_BF16);
  d.batch = atoi(argv[3]); d.height = atoi(argv[4]); d.width = atoi(argv[5]);
  const int lives = argc > 6 ? atoi(argv[6]) : 2;
  long streams_after_first = -1, events_after_first = -1;
  for (int life = 0; life < lives; ++life) {
    const int rc = one_life(d, life);
    if (rc) return rc;
    // the pool: what the first plan made is what every later plan uses - stream and event counts must not grow with the plans
    if (life == 0) { streams_after_first = fakehip_stream_creates(); events_after_first = fakehip_event_creates(); }
  }
  int rc = 0;
#ifdef DMM_HIST_MAX_THRESHOLDS
  if (getenv("DRIVE_HIST") && hist_main() != 0) rc = 1;
#endif
#ifdef DMM_AUG_MAX_TENSORS
  if (getenv("DRIVE_AUGMENT") && augment_main() != 0) rc = 1;
#endif
#ifdef DMM_WARP_LAUNCH_BATCH
  if (getenv("DRIVE_WARP") && warp_main() != 0) rc = 1;
#endif
#ifdef DMM_CC_TILE_H
  if (getenv("DRIVE_COMPONENTS") && components_main() != 0) rc = 1;
#endif
#ifdef DMM_PREP_LAUNCH_BATCH
  if (getenv("DRIVE_PREPARE") && prepare_main() != 0) rc = 1;
#endif
#ifdef DMM_MATCH_MAX_PER_PLANE
  if (getenv("DRIVE_MATCH") && match_main() != 0) rc = 1;
#endif
  if (g_bad) { fprintf(stderr, "[drive] FAIL: %ld device pointers outside the caller's regions\n", g_bad); rc = 1; }
  if (fakehip_violations()) { fprintf(stderr, "[drive] FAIL: %ld teardown / handle violations\n", fakehip_violations()); rc = 1; }
  if (lives > 1 && fakehip_stream_creates() != streams_after_first) {
    fprintf(stderr, "[drive] FAIL: streams are created per plan (%ld after the first plan, %ld after %d)\n", streams_after_first, fakehip_stream_creates(), lives);
    rc = 1;
  }
  if (lives > 1 && fakehip_event_creates() != events_after_first) {
    fprintf(stderr, "[drive] FAIL: events are created per plan (%ld after the first plan, %ld after %d)\n", events_after_first, fakehip_event_creates(), lives);
    rc = 1;
  }
  printf("%s\n", rc ? "DRIVE FAILED" : "DRIVE OK");
  return rc;
}
