// Argument blocks and launchers of the helper kernels (see pointwise.hip) and of the two GEMM kernels.
#pragma once
#include "../../include/dmmfods_hip.h"   // dmm_guard_state
#include "common.h"

namespace dmm {

struct ConvertArgs {
  const float* src1;  // (B, C1, H, W) fp32
  const float* src2;  // (B, C2, H, W) fp32 or null
  int C1, C2;         // C1 + C2 <= 8
  void* dst;          // T NHWC, 8 channels per pixel, zero padded
  int B, H, W;
  double* stat_sum;   // 8 doubles each (nullable)
  double* stat_sq;
  float scale;        // multiplies every value (1 for inputs; loss_scale for an external d(loss)/d(logit))
  const float* dyn_scale;  // device; multiplies on top of `scale` (the dynamic loss scale, dmm_plan_set_dynamic_loss_scale); null = none
};

struct BnFinalizeArgs {
  const double* sum;
  const double* sq;
  int stat_stride;  // doubles between the STAT_REPS replicas of sum / sq (0: a single copy)
  double count;           // positions the sums were taken over
  double count_unbiased;  // positions PyTorch's BatchNorm sees (differs for the nearest-upsampled head input)
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  float* scale;
  float* shift;
  float* mean;
  float* invstd;
  int C;
  int training;
  float momentum, eps;
};

struct BnBwdFinalizeArgs {
  const double* red1;  // sum dz
  const double* red2;  // sum dz*xhat
  int stat_stride;     // doubles between the STAT_REPS replicas of red1 / red2 (0: a single copy)
  const float* mean;
  const float* invstd;
  const float* scale;
  float* dgamma;
  float* dbeta;
  double* qd;  // deferred correction accumulators of the normalised tensor, fp64 (nullable)
  double* rd;
  float* q;    // float hi / lo split of the accumulators, rewritten after every update
  float* r;
  float* ql;
  float* rl;
  double count;      // positions of the normalised tensor
  float grad_scale;  // 1 / loss_scale
  int C;
  int accumulate;    // 0: dgamma / dbeta are stored; 1: added to what the arena holds (gradient accumulation, dmm_plan_set_grad_accumulate)
};

struct MaxpoolArgs {
  const void* y0;  // (B, H0, W0, ld0) conv0 output
  int ld0, H0, W0, B, C;
  const float* scale;
  const float* shift;
  void* out;  // (B, Hp, Wp, ldo), pre-offset to the destination channels
  int ldo, Hp, Wp;
  unsigned char* argmax;  // (B, Hp, Wp, C)
  double* stat_sum;
  double* stat_sq;
  int stat_stride;  // doubles between the STAT_REPS replicas of sum / sq (0: a single copy)
};

// p = avgpool2x2(relu(x * scale + shift)): the operand of a transition's 1x1 convolution, written once (pointwise.hip: avgpool2_kernel)
struct AvgPool2Args {
  const void* x;       // (B, H, W, ld), pre-offset to the first channel of the window; H and W even
  int ld, H, W, B, C;  // C: storage channels of the window, whole 16-byte slots
  const float* scale;  // C floats each
  const float* shift;
  void* out;           // (B, H / 2, W / 2, ldo), pre-offset
  int ldo;
};

struct MaxpoolBwdArgs {
  const void* y0;
  int ld0, H0, W0, B, C;
  const float* scale;
  const float* shift;
  const void* gpool;  // raw gradient of the pooled tensor (pre-offset), pixel stride ldg
  const void* xpool;  // pooled forward tensor (same layout) for the deferred correction
  const float* q;
  const float* r;
  const float* ql;
  const float* rl;
  const float* mean;    // norm0 batch statistics of y0
  const float* invstd;
  int ldg, Hp, Wp;
  const unsigned char* argmax;
  void* gy0;  // (B, H0, W0, ld0): s * dz0
  double* red1;
  double* red2;
  int stat_stride;  // doubles between the STAT_REPS replicas of red1 / red2 (0: a single copy)
};

struct BceArgs {
  const float* logits;  // (B, NC, H, W) fp32
  const float* target;
  void* dlogits;  // T NHWC8: (sigmoid(x) - t) * loss_scale   (nullable)
  double* out;    // [NC loss | NC equal | B x (NC inter, NC union)]
  int B, NC, H, W;
  float thr, loss_scale;
  // loss epilogue: 0 = BCE-with-logits (A:54); 1 = focal loss alpha[c]*(1-exp(-bce))^gamma[c]*bce on top of it
  // (reference graphs/losses/FocalLoss.py:41-50, class-wise :78-91).  from_prob: the input holds probabilities
  // (binary_cross_entropy with torch's log clamp at -100) instead of logits.
  int kind, from_prob;
  float alpha[8], gamma[8];
  float* loss_out;  // fp32 NCHW unreduced loss (nullable)
  float* dx_out;    // fp32 NCHW d(sum loss)/d(input), unscaled (nullable)
  int metrics;      // 0: skip the loss sums / metric counts (out may be null)
  const float* dyn_scale;  // device; dlogits = (sigmoid(x) - t) * loss_scale * (*dyn_scale) (the dynamic loss scale); null = none.
                           // loss_out, dx_out, the loss sums and the metric counts never see it
};

// ---- validation threshold sweep (lhist.hip) ----
constexpr int HIST_MAX_THRESHOLDS = DMM_HIST_MAX_THRESHOLDS;
struct LogitHistArgs {
  const float* logits;  // (B, NC, H, W) fp32
  const float* target;
  unsigned long long* counts;  // int64 [B][NC][2][K + 1]: counts[b][n][t >= gt][#{k : x >= thr[k]}] += 1
  int B, NC, H, W;             // H * W < 2^31, B * NC <= 65535 (gridDim.y)
  int K;                       // 1 .. HIST_MAX_THRESHOLDS
  float gt;
  float thr[HIST_MAX_THRESHOLDS];  // strictly ascending, finite; by value (1020 bytes), so a launch needs no upload
};

// ---- heat maps to objects (components.hip) ----
constexpr int CC_TILE_H = DMM_CC_TILE_H, CC_TILE_W = DMM_CC_TILE_W;
constexpr int CC_SEG = 4096;   // pixels of a plane, consecutive in raster order, whose roots one workgroup counts and then ranks
struct ComponentsArgs {
  const float* maps;        // (B, NC, H, W) fp32
  int* labels;              // (B, NC, H, W) int32: the caller's array, or the one carved from the workspace
  int* seg;                 // [B * NC][nseg]: roots per segment, then (scan) the roots in front of the segment
  dmm_component* records;   // [B * NC][cap]
  int* counts;              // [B * NC]
  int B, NC, H, W;          // H * W < 2^31, B * NC <= 65535 (gridDim.y)
  int tiles_x, tiles_y;     // ceil(W / CC_TILE_W), ceil(H / CC_TILE_H)
  int nseg;                 // ceil(H * W / CC_SEG)
  int cap;                  // max_per_plane
  int conn8;                // 1: 8-connectivity
  float thr;
};
// where the call's two arrays lie in its workspace (bytes from its start, each a multiple of 16) and the total
struct ComponentsLayout { size_t labels, seg, total; };
ComponentsLayout components_layout(int planes, size_t plane);
// the seven launches of one call, in order; each grid is (x, planes)
constexpr int CC_LAUNCHES = 7;
void components_grids(const ComponentsArgs& a, unsigned gx[CC_LAUNCHES]);
hipError_t launch_components(const ComponentsArgs& a, hipStream_t st);

// ---- object matching (match.hip) ----
struct MatchArgs {
  const dmm_component* pred;   // [B * NC][cap_pred]
  const dmm_component* gt;     // [B * NC][cap_gt]
  const int* pred_counts;      // [B * NC]
  const int* gt_counts;
  int* np;                     // workspace, [B * NC]: participating predictions of the plane
  int* ng;                     // workspace, [B * NC]: participating ground-truth records
  long long* base;             // workspace, [B * NC]: where the plane's entries start in its class
  unsigned char* matched;      // (B, NC, cap_pred), or null
  long long* totals;           // (NC, 8)
  int* entries;                // (NC, capacity, 2)
  long long capacity;          // 1 .. 2^31 - 1
  double iou;
  int B, NC;                   // B * NC <= 65535
  int cap_pred, cap_gt;        // 1 .. DMM_MATCH_MAX_PER_PLANE
  int min_area;
};
// where the call's three arrays lie in its workspace (bytes from its start, each a multiple of 16) and the total
struct MatchLayout { size_t np, ng, base, total; };
MatchLayout match_layout(int planes);
// the three launches of one call, in order; each grid is (x)
constexpr int MATCH_LAUNCHES = 3;
void match_grids(const MatchArgs& a, unsigned gx[MATCH_LAUNCHES]);
hipError_t launch_match(const MatchArgs& a, hipStream_t st);

// ---- batch augmentation (augment.hip) ----
constexpr int AUG_MAX_CHANNELS = DMM_AUG_MAX_CHANNELS;
constexpr int AUG_LAUNCH_BATCH = DMM_AUG_LAUNCH_BATCH;
struct AugChannel {        // one global channel: plane `c` of its tensor, for sample 0
  const float* src;        // tensor.src + c * Hs * Ws; sample b: + b * src_stride
  float* dst;              // tensor.dst + c * Ho * Wo; sample b: + b * dst_stride
  long long src_stride, dst_stride;   // elements
};
struct AugArgs {           // by value (about 2.9 KB), so a launch needs no upload
  AugChannel ch[AUG_MAX_CHANNELS];    // gridDim.y of them
  float fill[AUG_MAX_CHANNELS];
  int Hs, Ws, Ho, Wo;      // Hs * Ws, Ho * Wo < 2^31
  int b0;                  // sample of blockIdx.z == 0
  dmm_aug_sample s[AUG_LAUNCH_BATCH];   // gridDim.z of them: samples b0 ...
};

// ---- affine warp (warp.hip) ----
constexpr int WARP_LAUNCH_BATCH = DMM_WARP_LAUNCH_BATCH;
struct WarpArgs {          // by value (3416 bytes), so a launch needs no upload
  AugChannel ch[AUG_MAX_CHANNELS];    // gridDim.y of them
  float fill[AUG_MAX_CHANNELS];
  int mode[AUG_MAX_CHANNELS];         // DMM_WARP_NEAREST / DMM_WARP_BILINEAR, per global channel
  int Hs, Ws, Ho, Wo;      // Hs * Ws, Ho * Wo < 2^31
  int b0;                  // sample of blockIdx.z == 0
  int reserved;
  dmm_warp_sample s[WARP_LAUNCH_BATCH];   // gridDim.z of them: samples b0 ...
};
static_assert(sizeof(WarpArgs) == 3416 && 2 * sizeof(WarpArgs) > 4096, "DMM_WARP_LAUNCH_BATCH: the largest power of two that fits 4 KB");

// ---- raw frames to training tensors (prepare.hip) ----
constexpr int PREP_LAUNCH_BATCH = DMM_PREP_LAUNCH_BATCH;
constexpr int PREP_TILE = 16;          // a workgroup of the heat-map launch owns PREP_TILE x PREP_TILE output pixels
constexpr int PREP_BOX_CHUNK = 256;    // list entries it culls into LDS at a time
struct PrepImageArgs {
  const unsigned char* src;            // (B, H, W, C) uint8; sample b: + b * src_stride bytes
  float* dst;                          // (B, C, Ho, Wo); sample b: + b * dst_stride elements
  long long src_stride, dst_stride;
  int H, W, C, Ho, Wo, p;
  int b0;                              // sample of blockIdx.z == 0
};
struct PrepLidarArgs {
  const float* points;                 // (n, 3): x, y, d
  int* owner;                          // (B, H, W): the highest covering point index, -1 where none
  float* dst;                          // (B, 1, Ho, Wo)
  long long dst_stride;
  int H, W, Ho, Wo, p, k;
  int b0, nb;                          // samples b0 .. b0 + nb - 1
  int off[PREP_LAUNCH_BATCH + 1];      // their point ranges: sample b0 + s owns [off[s], off[s + 1])
};
struct PrepHeatArgs {
  const dmm_prep_box* boxes;
  float* dst;                          // (B, 3, Ho, Wo)
  long long dst_stride;
  int H, W, Ho, Wo, p;
  int b0, nb;
  int off[PREP_LAUNCH_BATCH + 1];      // box ranges, as above
};

struct ApplyCorrArgs {
  void* g;        // T gradient, pixel stride ldg: g += (q + ql) + (r + rl) * y
  const void* y;  // T forward tensor, pixel stride ldy
  const float* q;
  const float* r;
  const float* ql;
  const float* rl;
  size_t npix;
  int C, ldg, ldy;
};

// ---- guarded optimiser step (guard.hip) ----
constexpr int GUARD_PARTIALS = 512;  // workgroups of the arena reduction = fp64 partial sums in its scratch: two per compute unit
struct GradSumsqArgs {
  const float* g;     // a range of the gradient arena (any 4-byte alignment)
  size_t n;
  double* partials;   // GUARD_PARTIALS doubles; workgroup w owns partials[w]
  int accumulate;     // 0: partials[w] = sum of this range's share; 1: += (a later range of the same step, e.g. the next gradient bucket)
};
// ---- Adam: one kernel under a segment table (parameter groups in one launch) or over one whole range (guard.hip) ----
constexpr int ADAM_MAX_CLASSES = DMM_ADAM_MAX_CLASSES;
constexpr int ADAM_SEG_CHUNK = 1024;   // elements per chunk of the table = one 16-byte vector per thread of a workgroup
constexpr int ADAM_SEG_MAX_GRID = 2048;
struct AdamSegDev {      // device form of a segment: [begin, end) and its class
  long long begin, end;
  int cls, pad;
};
struct AdamSegClass {
  float lr, beta1, beta2, eps;
  float weight_decay;    // the L2 term's factor: 0 for a decoupled class
  float decay;           // decoupled: (float)(1 - lr * weight_decay), what p is multiplied by first
  float step_size, bc2_sqrt;   // plain path: formed on the host; guarded path: formed by the kernel from state->applied_steps - t0
  long long t0;
  int decoupled;
  int active;            // 0: the class's own step count is below 1 - nothing is written
};
struct AdamSegArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  size_t n;
  const AdamSegDev* segs;   // nsegs, sorted, disjoint, inside [0, n); nullptr: the whole-range form, one implicit segment [0, n) of
                            // class 0 (nsegs = 1, first is not read)
  const int* first;         // nchunks: index of the first segment whose end lies behind the chunk's first element (nsegs: none)
  int nsegs, nchunks, nclasses;
  int vec_ok;               // the four arenas (and ema, when it is on) are 16-byte aligned
  float grad_scale;         // plain path
  const dmm_guard_state* state;   // guarded path (else nullptr): found_inf, grad_scale, applied_steps
  AdamSegClass cls[ADAM_MAX_CLASSES];
  // Parameter average (guard.hip, ema_elem): e += omd * (p - e) wherever this launch writes p.  nullptr: off.
  float* ema;
  float ema_omd;            // plain path: (float)(1 - d_k), formed on the host from the caller's k
  float ema_decay;          // guarded path: the kernel forms omd itself, from k = state->applied_steps - ema_t0 (k < 1: no average is
  int ema_warmup;           //   written), d_k = ema_warmup ? min(ema_decay, (1 + k) / (10 + k)) : ema_decay, in double
  long long ema_t0;
};
struct GuardFinalizeArgs {
  const double* partials;
  dmm_guard_state* state;
  float lr, beta1, beta2;
  float max_norm;                       // <= 0: no clipping
  float growth_factor, backoff_factor;
  int growth_interval;                  // 0: the scale never grows
};

struct PackSeg {
  int Creal, Cpad, ntaps, nchunks, koff;
  unsigned tapw[MAX_TAPS];  // up to four master tap indices per packed tap, 0xff = none
};

struct PackDesc {
  const float* w;  // master weights
  void* dst;       // T packed [chunk][Npad][BK]
  float* gw;       // master gradient (nullable)
  const float* dpack;  // fp32 packed gradient (nullable)
  int N, Npad, nseg;
  int shared_master;  // several descriptors add into the same master elements
  long long sn, sk, st;  // master index = n*sn + k*sk + tap*st
  PackSeg seg[2];
  int rs;             // taps of the master tensor (R * S)
  int tiled;          // 0: generic pack / unpack kernels; 1: tile kernels, the master is contiguous along (k, tap) for a fixed n (sk == rs);
                      // 2: tile kernels, contiguous along (n, tap) for a fixed k (sn == rs)
};
// One workgroup of the tile kernels (pack_tiles_kernel / unpack_tiles_kernel): 32 rows n x 32 channels x all taps of a master tensor,
// for the `nsib` consecutive descriptors that share it (the parity phases of a ConvTranspose: together they cover every tap once).
struct PackTile { int desc, nsib, n0, cg; };   // nsib: count | 0x100 when no master tap is written twice by the group

// Fused backward of a dense layer's 1x1 bottleneck convolution (bw1.hip): the data-gradient launch `c` (EPI_BNBWD) plus the
// packed weight gradient of the same convolution.
struct Bw1Args {
  ConvArgs c;
  float* dpack;       // fp32 packed weight gradient [chunk = c / 32][dNpad][32]
  int dNpad, wC;      // its row pitch (128) and the real number of input channels
  // Weight-gradient partials (nullable).  Every workgroup ends with a 64 KB slice of the weight gradient in registers.  Added to
  // dpack with fp32 atomics that is 33 MB per launch at the atomics' 1.3 TB/s - 0.9 ms of the step on the data-gradient chain.
  // With `part` each workgroup STORES its slice to slot (row range * nct + channel slice) (plain stores: 6 TB/s) and a second
  // launch (launch_bw1_reduce, on the weight-gradient stream) adds the slots up into dpack.
  float* part;
  int part_slots;     // capacity of `part` in 64 KB slots
  int nct, ntiles, tiles_per_wg, xcd_group, nsplit;  // (filled by the launcher)
};
struct Bw1Geom { int nct, ntiles, tiles_per_wg, nsplit, xcd_group, nwg; };
Bw1Geom bw1_geometry(const ConvArgs& a);   // how launch_bw1 splits the launch (device-dependent: compute units)
constexpr int B1_SLOT_FLOATS = 4 * 128 * 32;  // one workgroup's slice: 4 chunks of 32 input channels x 128 bottleneck channels
bool bw1_eligible(const WgradArgs& w, const ConvArgs& d, int dtype, unsigned deny);  // deny: as igemm_pick
hipError_t launch_bw1(const Bw1Args& g, int dtype, hipStream_t st);
hipError_t launch_bw1_reduce(const Bw1Args& g, hipStream_t st);  // dpack = sum of the slots (no-op without `part`)
// Grouped launches (capi.cpp run_ops hands consecutive independent launches of a dense block over together).
// bw1.hip: the reductions of up to B1_RED_GROUP_MAX fused launches as ONE launch (gridDim.y = member); each member is added up exactly
// as launch_bw1_reduce does it alone - the same loads and additions in the same order.
constexpr int B1_RED_GROUP_MAX = 32;
struct Bw1RedMember { const float* part; float* dpack; int nct, nsplit, nfloats; };
struct Bw1RedGroup { int n = 0; Bw1RedMember m[B1_RED_GROUP_MAX]; };
bool bw1_reduce_group_add(Bw1RedGroup& G, const Bw1Args& g);  // false: the group is full (launch it first); a record without slots adds nothing
hipError_t bw1_reduce_group_launch(Bw1RedGroup& G, hipStream_t st);  // launches the members (if any) and empties the group
hipError_t launch_bw1_reduce_member(const Bw1RedMember& m, hipStream_t st);  // one member alone: launch_bw1_reduce's kernel
// wg3.hip: the dense 3x3 weight gradients of up to W3_GROUP_MAX layers as one wg3 launch + one reduction (slot index = workgroup index
// in the family's one slot buffer).  `block` holds the kernel argument being assembled (wg3.hip: Wg3GroupLaunch).
constexpr int W3_GROUP_MAX = 32;
struct Wg3Group {
  int n = 0, dtype = 0, pq = 0, part_slots = 0;
  long long tiles = 0;  // of the members so far
  alignas(16) unsigned char block[4096];
};
bool wg3_group_add(Wg3Group& G, const WgradArgs& a, int dtype);  // false: `a` does not fit (launch the group first; with G.n == 0: not a launch to group)
hipError_t wg3_group_launch(Wg3Group& G, hipStream_t st);        // launches the members (if any) and empties the group
// impl = IMPL_AUTO: the first family of the table that `deny` (1 << family) does not name and that resolves; otherwise the recorded family
hipError_t launch_igemm(const ConvArgs& a, int dtype, int epi, bool mfma, hipStream_t st, int impl = IMPL_AUTO, unsigned deny = 0);
hipError_t launch_wgrad(WgradArgs a, int dtype, bool mfma, hipStream_t st, int impl = IMPL_AUTO, unsigned deny = 0);
// the family (enum Impl) that launch_*(..., IMPL_AUTO, deny) would run; deny: 1 << family for the families switched off (dmm_plan::deny)
int igemm_pick(const ConvArgs& a, int dtype, int epi, bool mfma, unsigned deny);
int wgrad_pick(const WgradArgs& a, int dtype, bool mfma, unsigned deny);
hipError_t launch_wg5_rawfin(const RawFinArgs& a, hipStream_t st);
hipError_t launch_wg5_fin64(const Fin64Args& a, hipStream_t st);
hipError_t launch_convert_input(const ConvertArgs& a, int dtype, hipStream_t st);
hipError_t launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t st);
hipError_t launch_bn_bwd_finalize(const BnBwdFinalizeArgs& a, hipStream_t st);
hipError_t launch_maxpool_fwd(const MaxpoolArgs& a, int dtype, hipStream_t st);
hipError_t launch_maxpool_bwd(const MaxpoolBwdArgs& a, int dtype, hipStream_t st);
hipError_t launch_avgpool2_fwd(const AvgPool2Args& a, int dtype, hipStream_t st);   // hipErrorInvalidValue: not whole slots / windows
hipError_t launch_bce_metrics(const BceArgs& a, int dtype, hipStream_t st);
// accumulate == 0: a hipMemsetAsync of counts on `st` goes in front of the kernel; otherwise the kernel adds to what is there
hipError_t launch_logit_hist(const LogitHistArgs& a, int accumulate, hipStream_t st);
int logit_hist_grid_x(int planes, size_t plane);   // workgroups per (b, n) plane of that launch
// accumulate == 0: a hipMemsetAsync of counts on `st` goes in front of the kernel; otherwise the kernel adds to what is there
hipError_t launch_logit_hist(const LogitHistArgs& a, int accumulate, hipStream_t st);
int logit_hist_grid_x(int planes, size_t plane);   // workgroups per (b, n) plane of that launch
// one launch: gridDim = (augment_grid_x(Ho, Wo), nchannels, nsamples <= AUG_LAUNCH_BATCH)
hipError_t launch_augment(const AugArgs& a, int nchannels, int nsamples, hipStream_t st);
unsigned augment_grid_x(int Ho, int Wo);   // workgroups per plane: one lane per four output pixels of a row
// one launch: gridDim = (warp_grid_x(Ho, Wo), nchannels, nsamples <= WARP_LAUNCH_BATCH)
hipError_t launch_warp(const WarpArgs& a, int nchannels, int nsamples, hipStream_t st);
unsigned warp_grid_x(int Ho, int Wo);      // workgroups per plane: one per WARP_TILE_W x WARP_TILE_H output tile
// raw frames to training tensors: one launch each for nsamples / a.nb <= PREP_LAUNCH_BATCH samples (the LiDAR form: the splat, unless
// the samples have no point between them, then the pool; the owner planes are cleared by the caller)
hipError_t launch_prep_image(const PrepImageArgs& a, int nsamples, hipStream_t st);   // grid (prep_plane_grid_x, C, nsamples)
hipError_t launch_prep_lidar(const PrepLidarArgs& a, hipStream_t st);                 // (prep_splat_grid_x), then (prep_plane_grid_x, nb)
hipError_t launch_prep_heat(const PrepHeatArgs& a, hipStream_t st);                   // grid (prep_heat_grid_x, nb)
unsigned prep_plane_grid_x(int Ho, int Wo);        // one lane per output pixel
unsigned prep_splat_grid_x(int npoints, int k);    // one lane per (point, window pixel)
unsigned prep_heat_grid_x(int Ho, int Wo);         // one workgroup per PREP_TILE x PREP_TILE tile
hipError_t launch_grad_sumsq(const GradSumsqArgs& a, hipStream_t st);
hipError_t launch_guard_finalize(const GuardFinalizeArgs& a, hipStream_t st);
// the one Adam launch.  a.state == nullptr: every class's step_size / bc2_sqrt / active and a.grad_scale come filled; a.state set: the
// kernel reads grad_scale and the skip from *state and forms each class's step_size / bc2_sqrt at its own count, applied_steps - t0
hipError_t launch_adam_segmented(const AdamSegArgs& a, hipStream_t st);
hipError_t launch_guard_init(dmm_guard_state* dev, float scale, int64_t applied, int32_t tracker, hipStream_t st);
hipError_t launch_apply_corr(const ApplyCorrArgs& a, int dtype, hipStream_t st);
hipError_t launch_pack(const PackDesc* descs_dev, const int* prefix_dev, int ndesc, int total_rows, int dtype, hipStream_t st,
                       const PackDesc* tile_descs = nullptr, const PackTile* tiles_dev = nullptr, int nt1 = 0, int nt9 = 0);
// accumulate: every master gradient element is ADDED to (a read-modify-write where the plain form stores; the atomic adds of merged
// taps and shared masters are adds in both forms).  false runs the kernels and the stores of a library without the mode.
hipError_t launch_unpack(const PackDesc* descs_dev, const int* prefix_dev, int ndesc, int total_rows, int dtype, float grad_scale,
                         hipStream_t st, const PackDesc* tile_descs = nullptr, const PackTile* tiles_dev = nullptr, int nt1 = 0, int nt9 = 0,
                         bool accumulate = false);

#if defined(__HIPCC__)
// ---- the finalize steps, per channel: bodies of bn_finalize_kernel / bn_bwd_finalize_kernel ----
// COH: the sums were added by OTHER workgroups of the running launch (float atomics execute at the memory side and leave nothing in
// any L2; the loads bypass this CU's L1: agent-scope relaxed atomic loads = global_load ... sc1).  Only the round-3 experiment that ran
// the steps as the tail of the producing launch used it (profiles/r03/ablations.txt: 0.8 ms SLOWER per step than launches of their own).
template <bool COH>
__device__ __forceinline__ double stat_load(const double* p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}

template <bool COH>
__device__ __forceinline__ void bn_finalize_channel(const BnFinalizeArgs& a, int c) {
  float mean, var;
  if (a.training) {
    double su = stat_load<COH>(a.sum + c), sq = stat_load<COH>(a.sq + c);
    if (a.stat_stride)
      for (int k = 1; k < STAT_REPS; ++k) { su += stat_load<COH>(a.sum + c + (size_t)k * a.stat_stride); sq += stat_load<COH>(a.sq + c + (size_t)k * a.stat_stride); }
    const double m = su / a.count;
    double v = sq / a.count - m * m;
    if (v < 0) v = 0;
    mean = (float)m;
    var = (float)v;
    const double unb = a.count_unbiased > 1 ? v * (a.count_unbiased / (a.count_unbiased - 1.0)) : v;
    a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
    a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (float)unb;
  } else {
    mean = a.running_mean[c];
    var = a.running_var[c];
  }
  const float invstd = 1.0f / sqrtf(var + a.eps);
  const float s = a.gamma[c] * invstd;
  a.scale[c] = s;
  a.shift[c] = a.beta[c] - mean * s;
  a.mean[c] = mean;
  a.invstd[c] = invstd;
}

template <bool COH>
__device__ __forceinline__ void bn_bwd_finalize_channel(const BnBwdFinalizeArgs& a, int c) {
  double S1 = stat_load<COH>(a.red1 + c), S2 = stat_load<COH>(a.red2 + c);
  if (a.stat_stride)
    for (int k = 1; k < STAT_REPS; ++k) { S1 += stat_load<COH>(a.red1 + c + (size_t)k * a.stat_stride); S2 += stat_load<COH>(a.red2 + c + (size_t)k * a.stat_stride); }
  const double mu = a.mean[c], is = a.invstd[c];
  const double dotp = S2;  // sum dz * xhat, reduced in centred form by the producing kernel
  const float dg = (float)(dotp * a.grad_scale), db = (float)(S1 * a.grad_scale);
  if (a.accumulate) {   // (uniform over the launch) one fp32 add of the value the plain form stores
    a.dgamma[c] += dg;
    a.dbeta[c] += db;
  } else {
    a.dgamma[c] = dg;
    a.dbeta[c] = db;
  }
  if (a.qd != nullptr) {
    const double s = a.scale[c];
    const double c1 = S1 / a.count, c2 = dotp / a.count;
    // contribution of this consumer to d/dx:  s*dz (stored by the dgrad epilogue)  - s*c1 - s*c2*(x-mu)*is.
    // Accumulated in fp64 over all consumers of the channel (they cancel heavily inside dense blocks) and handed to
    // the gathers as a two-float split: a rounding error here would be a coherent per-channel gradient offset.
    const double q = a.qd[c] + (-s * c1 + s * c2 * mu * is);
    const double r = a.rd[c] + (-s * c2 * is);
    a.qd[c] = q;
    a.rd[c] = r;
    const float qh = (float)q, rh = (float)r;
    a.q[c] = qh; a.ql[c] = (float)(q - (double)qh);
    a.r[c] = rh; a.rl[c] = (float)(r - (double)rh);
  }
}

#endif

}  // namespace dmm
