// Host-side plan of the Dense_U_Net_lidar training step: topology -> buffers -> kernel launch list.
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dmmfods_hip.h"
#include "common.h"
#include "pointwise.h"

namespace dmm {

// plan_bind: the bound pass did not take the workspace bytes the sizing pass reported (dmm_plan_bind returns DMM_ERR_STATE)
struct plan_sizing_error : std::runtime_error { using std::runtime_error::runtime_error; };

struct TensorInfo {
  std::string name;
  int kind, ndim;
  int64_t shape[4];
  int64_t off;  // elements into the param arena / buffer arena, -1 for num_batches_tracked
};

struct Tap {
  int dy, dx;
  unsigned tapw;  // up to four master tap indices (8 bits each, 0xff = none)
};

// tap geometry helpers (shared with the single-kernel test entry points)
std::vector<Tap> taps_conv(int R, int S, int pad);            // forward stride-1/2 conv: (ky-pad, kx-pad)
std::vector<Tap> taps_conv_dgrad(int R, int S, int pad);      // data gradient of a stride-1 conv: (pad-ky, pad-kx)
std::vector<Tap> taps_convT_phase(int py, int px);            // ConvTranspose 3x3 s2 p1, output parity (py,px)
std::vector<Tap> taps_convT_dgrad();                          // stride-2 gather over the output gradient
std::vector<Tap> taps_up2_merged_dgrad();                     // 3x3 conv over a nearest-x2 source: 4x4 s2 merged taps
std::vector<Tap> taps_up2_phase(int e, int f);                // same conv, forward, output parity (e,f): 2x2 merged half-res taps
std::vector<Tap> taps_conv_phase_s2(int e, int f);            // 3x3 p1 conv sampled at output parity (e,f) from a full-res source
void fill_seg_taps(Seg& s, const std::vector<Tap>& taps, int BK);
void fill_pack_seg(PackSeg& p, const std::vector<Tap>& taps, int Creal, int Cpad, int koff, int BK);

// The four output-parity phases of a ConvTranspose stage as ONE launch: what the plan builder's merge (plan.cpp:
// merge_last_four_phases) decides and copies for the forward (cvp.hip / cvw.hip) and for the weight gradient (wgpw.hip), as free
// functions of the launches' argument records - shared with the entry points that build the same merged launch outside a plan
// (capi.cpp: dmm_conv_forward_merged, dmm_conv_wgrad_merged), so that those hold the launch the plan builds and not a restatement of it.
//   *_phase_eligible(record, family picked for it, record of the first phase)   may this per-phase launch join the merge?
//   copy_*_phase(merged, record, ph)                                             what differs between the phases -> the merged record's ph_*
//   accept_*_merged(merged, ...)                                                 does the pick still take the merged record?  (it refuses
//                                                                                e.g. operands of 4 GiB and more: the four launches stay)
inline bool convT_fwd_phase_eligible(const ConvArgs& po, int epi, int impl, const ConvArgs& first) {
  return epi == EPI_STORE && impl == IMPL_CVP && po.nseg == 1 && po.seg[0].ntaps <= 4 && po.nphase == 0 && po.out == first.out &&
         po.seg[0].src == first.seg[0].src;
}
inline void copy_fwd_phase(ConvArgs& m, const ConvArgs& po, int ph, int ntaps0) {  // what every merged forward launch carries per phase
  m.nphase = 4;
  for (int t = 0; t < 4; ++t) m.ph_taps0[ph][t] = po.seg[0].taps[t < ntaps0 ? t : 0];
  m.ph_wpack[ph] = po.wpack;
  m.ph_py[ph] = (signed char)po.py; m.ph_px[ph] = (signed char)po.px;
}
inline void copy_convT_fwd_phase(ConvArgs& m, const ConvArgs& po, int ph) {
  copy_fwd_phase(m, po, ph, po.seg[0].ntaps);
  m.ph_ntaps[ph] = (signed char)po.seg[0].ntaps;
}
inline bool accept_convT_fwd_merged(const ConvArgs& m, int dtype, bool mfma, unsigned deny) {
  return igemm_pick(m, dtype, EPI_STORE, mfma, deny) == IMPL_CVP;
}
inline bool wgrad_phase_eligible(const WgradArgs& po, int impl, const WgradArgs& first) {
  const int nt = po.seg[0].ntaps;
  return impl == IMPL_WGP && po.nseg == 1 && (nt == 1 || nt == 2 || nt == 4) && po.seg[0].src == first.seg[0].src && po.dy.src == first.dy.src;
}
inline void copy_wgrad_phase(WgradArgs& m, const WgradArgs& po, int ph) {
  m.nphase = 4;
  for (int t = 0; t < 4; ++t) m.ph_xtaps[ph][t] = po.seg[0].taps[t < po.seg[0].ntaps ? t : 0];
  m.ph_ntaps[ph] = (signed char)po.seg[0].ntaps;
  m.ph_ytap[ph] = po.dy.taps[0];
  m.ph_dpack[ph] = po.dpack;
}
inline bool accept_wgrad_merged(WgradArgs& m, int dtype, bool mfma, unsigned deny) {
  bool all4 = true;   // four taps in every phase: ph_ntaps stays 0 (= seg[0].ntaps each)
  for (int ph = 0; ph < 4; ++ph) all4 = all4 && m.ph_ntaps[ph] == 4;
  if (all4) m.ph_ntaps[0] = m.ph_ntaps[1] = m.ph_ntaps[2] = m.ph_ntaps[3] = 0;
  return wgrad_pick(m, dtype, mfma, deny) == IMPL_WGP;
}

enum OpKind { OP_MEMSET = 0, OP_CONVERT, OP_IGEMM, OP_WGRAD, OP_BNFIN, OP_BNBWD, OP_POOL, OP_POOLBWD, OP_BCE, OP_PACK, OP_UNPACK,
              OP_COPY, OP_APPLYCORR, OP_BW1, OP_JOIN, OP_BW1RED, OP_RAWFIN, OP_FIN64 };

// What an OP_POOL record launches (Op::epi, which is no epilogue on this kind): the stem's 3x3 stride-2 max pooling (MaxpoolArgs) or the
// 2x2 average pooling of a transition's BN+ReLU input (AvgPool2Args).
enum PoolMode { POOL_MAX3 = 0, POOL_AVG2 = 1 };

struct MemsetArgs { void* p; size_t bytes; };
struct CopyArgs { void* dst; const void* src; size_t bytes; };
struct PackArgs {
  const PackDesc* descs; const int* prefix; int ndesc, total_rows; float grad_scale;
  const PackDesc* tdescs; const PackTile* tiles; int nt1, nt9;  // tile kernels: descriptor array the tiles index, the range's 1x1 / 3x3 tiles
};

struct Op {
  int kind;
  int epi;
  int leaf;        // nothing on the data-gradient chain reads what this launch produces (may run beside it): 1 side stream, forked from
                   // the main stream; 3 side stream, continuing the chain of the launch in front of it there (no fork); 2 pack stream
  int chain;       // 1: a weight-gradient-side launch the data-gradient chain WAITS for (its results feed the next launch of the chain):
                   // it runs on the main stream although its kind says side stream
  int signal;      // gradient bucket event to record behind this launch on the stream it ran on (-1: none)
  int impl;        // kernel family (enum Impl) chosen for this launch when the plan was built
  double flops;    // algorithmic 2*MACs of this launch (reference formulation)
  double bytes;    // algorithmic HBM bytes: every operand read once, every result written once
  char label[56];  // kernel class / layer
  union {
    MemsetArgs ms;
    CopyArgs cp;
    ConvertArgs cv;
    ConvArgs c;
    WgradArgs w;
    BnFinalizeArgs bf;
    BnBwdFinalizeArgs bb;
    MaxpoolArgs mp;
    AvgPool2Args ap;   // OP_POOL with epi == POOL_AVG2: a transition's pooled operand (POOL_MAX3: the stem's max pooling, mp)
    MaxpoolBwdArgs mpb;
    BceArgs bce;
    PackArgs pk;
    ApplyCorrArgs ac;
    Bw1Args b1;
    RawFinArgs rf;
    Fin64Args f64;
  };
  // A record starts out all zero - the argument union included, so an emitter assigns only what its launch uses.
  Op() { memset(static_cast<void*>(this), 0, sizeof(*this)); signal = -1; impl = IMPL_AUTO; }
};

// What the launch-list executor (capi.cpp: run_ops) decides from a record ALONE: pure functions of the record and the mode flags of
// the call - no plan, no stream, no runtime call - so that each fact is written once and a table of records can be walked through
// them without a GPU (tools/hoststub/drive.cpp `route`, tests/test_enqueue_trace_cpu.py).
#define DMM_EXECUTOR_PREDICATES 1
enum BatchKind { BATCH_NONE = 0, BATCH_W3, BATCH_RD };   // the grouped launch a record may join: wg3.hip's, bw1.hip's reduction
enum Lane { LANE_MAIN = 0, LANE_SIDE_CONTINUE, LANE_SIDE_FORK, LANE_PACK_FORK };
bool side_forks(const Op& o);               // a record of the weight-gradient side that forks from the caller's stream
BatchKind batch_kind(const Op& o, bool mfma);
bool flushes_batches(const Op& o);          // the pending batches go out in front of this record (unless it joined one)
Lane route(const Op& o, bool overlap, bool forked, bool batch_main);   // forked: the side stream is forked in this call; batch_main: batch_wgrad 1

}  // namespace dmm

// A contiguous range of the gradient arena (whole tensors) whose gradients become final at a known point of the backward
// launch list: data-parallel training all-reduces it from there on, beside the rest of backward.
struct GradBucket {
  int64_t off = 0, n = 0;             // elements of the gradient arena
  int ev_main = -1, ev_side = -1;     // indices into dmm_plan::bucket_events (-1: nothing on that stream writes the bucket)
  int ready = -1;                     // index of the last launch that writes into it
};

// The run-time switches of a plan, read from the environment ONCE, by dmm_plan_create, and kept in the plan: the sizing pass
// (create) and the bound pass (bind) cannot disagree about them, and nothing in the library calls getenv while a plan is built or run.
// Each selects between two correct schedules of the same arithmetic and has an A/B test (tests/test_timed_kernels_gpu.py; the host
// harness of tests/test_host_cpu.py drives every one through create -> bind -> run -> destroy under AddressSanitizer):
//   DMM_NO_PACK_TILES=1     weights packed / gradients unpacked by the generic kernels only
//   DMM_NO_HF=1             the head's first convolution on conv3.hip's one-launch path instead of hf.hip (a bit of dmm_plan::deny)
//   DMM_NO_C3_MERGE=1       ... as four launches, one per output parity
//   DMM_NO_CVP_MERGE=1      a decoder ConvTranspose's four parity phases as four launches
//   DMM_NO_WGP_MERGE=1      the head's weight-gradient phases as four launches
//   DMM_NO_TWO_PASS=1       the 5x5 data gradient as one pass + apply_corr instead of two passes
//   DMM_NO_EFF_COMPACT=1    wg3.hip gathers its gradient operand from the block buffers instead of reading conv3.hip's compact copy
//   DMM_NO_S2_INTERLEAVE=1  mid fusion: the second encoder's launch records behind the first's instead of alternating
//   DMM_PACK_CUT=<n>        the forward record in front of which the late layers' weight pack is joined (1 = behind the stem)
//   DMM_NO_R1_STATS=1       the BatchNorm-backward sums of the head's norm1 from the reductions-only first pass of the 5x5 data gradient
//                           instead of from the 5x5 weight gradient's factor correlations (wg5.hip, PA = 3)
//   DMM_TRANSITION_POOL_ROWS=<n>  a transition of at least n pooled rows (B * H/2 * W/2) writes its pooled BN+ReLU input once and runs as
//                           a plain 1x1 layer over it (plan.cpp: transition_pools); 0 = every transition, a huge n = none.  Default:
//                           TRANSITION_POOL_MIN_ROWS
//   DMM_NO_RAW_STATS=1      the BatchNorm-backward sums of the head's raw-input channels from a data-gradient pass of their own
//                           (round 4) instead of from the weight gradient's factor correlations (wg5.hip, PY = 2)
// Process-wide (capi.cpp, read when the library is loaded; also dmm_set_option): DMM_NO_OVERLAP, DMM_GRAPH, DMM_GRAD_BUCKET_MB;
// dmm_set_option alone: the kernel-family switches, one word (capi.cpp: g_family_off), copied into dmm_plan::deny in front of each
// builder pass; diagnostics: DMM_TRACE_DESTROY.  Everything else that used to be an environment switch is a compile-time lab knob (common.h).
struct PlanSwitches {
  bool no_pack_tiles = false, no_hf = false, no_c3_merge = false, no_cvp_merge = false, no_wgp_merge = false, no_two_pass = false,
       no_eff_compact = false, no_s2_interleave = false, no_raw_stats = false, no_r1_stats = false;
  int pack_cut = 0;  // 0: by weight count
  long long transition_pool_rows = -1;  // -1: TRANSITION_POOL_MIN_ROWS (plan.cpp)
  static PlanSwitches from_environment();
};

struct dmm_plan {
  dmm_model_desc desc;
  PlanSwitches sw;
  unsigned deny = 0;  // kernel families ruled out (1 << family, dispatch.h): DMM_NO_HF + the dmm_set_option switches, as they stood when the
                      // builder pass in progress began (dmm_plan_create: sizing, dmm_plan_bind: the launch lists)
  std::vector<dmm::TensorInfo> tensors;
  int64_t nparams = 0, nbuf = 0;
  size_t zero_bytes = 0, zero_bwd_bytes = 0, main_bytes = 0;
  double fwd_flops = 0;
  bool bound = false;
  void* ws = nullptr;
  float *params = nullptr, *grads = nullptr, *buffers = nullptr;
  // launch lists (built by bind)
  std::vector<dmm::Op> fwd_train, fwd_eval, bwd;
  // indices of ops whose pointers are patched per call
  std::vector<int> convert_ops_train, convert_ops_eval;
  int logits_op_train = -1, logits_op_eval = -1;
  int bce_op = -1, bce_only_valid = 0;
  dmm::Op bce_only;     // loss + metrics without gradient
  int loss_kind = 0;          // 0 BCE, 1 focal (dmm_plan_set_loss)
  float loss_alpha[8] = {1, 1, 1, 1, 1, 1, 1, 1}, loss_gamma[8] = {2, 2, 2, 2, 2, 2, 2, 2};
  bool grad_accumulate = false;      // backward adds into the gradient arena instead of overwriting it (dmm_plan_set_grad_accumulate): a run-time
                                     // property of the SAME launch list - launch_record skips the arena's memset and launches the arena's writers
                                     // (OP_UNPACK, OP_BNBWD) in their accumulate form; survives dmm_plan_bind
  bool encoder_frozen = false;       // the encoder (features, stream_2_features, concat_module) is not trained (dmm_plan_set_encoder_frozen): the
                                     // backward list ends in front of the first encoder record, buckets and unpack tables hold trainable tensors
                                     // only.  Set on an unbound plan (the sizing pass runs again); survives dmm_plan_bind
  const float* dyn_scale = nullptr;  // device; the dynamic loss scale the loss kernel multiplies by (dmm_plan_set_dynamic_loss_scale), null = none
  double* metrics = nullptr;  // device, inside the zero region
  size_t metrics_bytes = 0;
  std::vector<dmm::PackDesc> packs;
  std::vector<int> pack_prefix;
  // unpack tables, grouped by gradient bucket
  std::vector<dmm::PackDesc> unpacks;
  std::vector<int> unpack_prefix;
  std::vector<dmm::PackTile> pack_tiles, unpack_tiles;  // tile-kernel work lists (pointwise.h PackTile)
  size_t bucket_bytes = 0;
  std::vector<GradBucket> buckets;       // in the order they become ready
  std::vector<void*> bucket_events;      // hipEvent_t, created on first use
  // profiling: per-op events on the launch stream, one set per recorded pass
  int prof_max_passes = 0;
  int prof_pass[2] = {0, 0};                       // passes recorded for [0] training forward, [1] backward
  std::vector<std::vector<void*>> prof_events[2];  // [which][pass] -> one (start, end) event pair per op
  std::string prof_filter;                         // only ops whose label starts with this are bracketed (empty: all)
  // Streams: the side stream (weight gradients, leaves, the second encoder), the pack stream and the capture stream belong to a
  // PROCESS-LIFETIME pool per device (capi.cpp: DevicePool) - a plan never creates or destroys a stream.  Events (fork / join /
  // bucket / profiling) are taken from that pool's free lists on first use and handed back by dmm_plan_destroy.
  int device = -1;                         // the device the plan was bound on
  bool used_side = false, used_capture = false;
  std::vector<void*> join_events;          // [0] side stream, [1] pack stream
  std::vector<void*> fork_events;
  // hipGraph replay of a launch list (capi.cpp: launch_list): the one instantiated graph of the list's replayed segment
  struct GraphCache {
    void* exec = nullptr;          // hipGraphExec_t (null: not captured)
    int nseen = 0;                 // the list has run eagerly since the last drop: the next run captures it
    unsigned long long epoch = 0;  // option epoch the graph was captured under (dmm_set_option and dmm_plan_bind invalidate it)
  };
  GraphCache graphs[2];          // [0] training forward, [1] loss + backward
  bool graph_failed = false;     // a capture did not work on this plan: stay eager
  bool dp_used = false;          // a data-parallel reducer waits for bucket events: backward stays eager (events must be real)
  long long graph_replays[2] = {0, 0};
  // launch coalescing (capi.cpp WgradBatches), summed over the plan's life: [0] wg3 launches (a grouped launch counts once; each comes with one
  // reduction), [1] the wg3 records they served, [2] bw1 reduction launches, [3] the bw1.reduce records they served (dmm_plan_wgrad_batch_counts)
  long long batch_counts[4] = {0, 0, 0, 0};
};
