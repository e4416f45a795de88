/* dmmfods_hip.h -- C ABI of libdmmfods_hip.so: the MI355X (gfx950) implementation of the DMMFODS
 * Dense_U_Net_lidar training hot path.
 *
 * The reference (p-mc-grath/DMMFODS) is pure Python on torch.nn and has NO FFI of its own; its drop-in
 * boundary is the Python surface of  dmmfods/graphs/models/Dense_U_Net_lidar.py  and
 * dmmfods/agents/Dense_U_Net_lidar_Agent.py.  Each entry point below names the reference interface it
 * stands behind (paths relative to the reference tree):
 *
 *   dmm_plan_create / dmm_plan_destroy ... Dense_U_Net_lidar.__init__   graphs/models/Dense_U_Net_lidar.py:29-208
 *   dmm_plan_tensor_*  .................... nn.Module.state_dict() key/shape layout   (same file, :71-192)
 *   dmm_plan_forward ..................... Dense_U_Net_lidar.forward    graphs/models/Dense_U_Net_lidar.py:210-267
 *   dmm_plan_loss_backward ............... BCEWithLogitsLoss(reduction='none') + metrics + backward(ones)
 *                                          agents/Dense_U_Net_lidar_Agent.py:247-264, utils/...helper.py:311-401
 *   dmm_plan_set_loss / dmm_loss_forward . FocalLoss / ClassWiseFocalLoss  graphs/losses/FocalLoss.py:9-91
 *   dmm_logit_hist ....................... nothing upstream: compute_IoU_whole_img_batch / calculate_accuracy
 *                                          (utils/Dense_U_Net_lidar_helper.py:311-401) at up to 255 thresholds in one pass
 *   dmm_augment_batch .................... nothing upstream (the reference feeds the model what the loader yields, :236-244): crop,
 *                                          flip, shift, per-channel gain and bias of a device batch in one launch
 *   dmm_warp_batch ....................... nothing upstream: scale and rotation of a device batch - a fixed-point affine map per sample,
 *                                          heat maps and LiDAR sampled nearest, the image bilinear - in one launch
 *   dmm_heat_components .................. nothing upstream (the reference cannot "compute IoU per bounding box", helper.py:311-315):
 *                                          connected components of a thresholded heat map, one record per object
 *   dmm_match_objects .................... nothing upstream: greedy IoU pairing of predicted and ground-truth records, the counts
 *                                          and the ranked (score, matched) list of an epoch kept on the device
 *   dmm_prep_image / dmm_prep_lidar / dmm_prep_heat_maps
 *                                          avgpool_tensor / lidar_array_to_image_like_tensor + pool_lidar_tensor /
 *                                          create_ground_truth_maps + maxpool_tensor  utils/Dense_U_Net_lidar_helper.py:233-305,430-515:
 *                                          the host-side preparation of a frame's seven planes, on the device and bit for bit
 *   dmm_adam_step ........................ torch.optim.Adam.step        agents/Dense_U_Net_lidar_Agent.py:57-61,265
 *   dmm_adam_table_* / dmm_adam_step_segmented / dmm_adam_step_guarded_segmented
 *                                          torch.optim.Adam built over PARAMETER GROUPS (the list-of-dicts form of the constructor
 *                                          called at agents/Dense_U_Net_lidar_Agent.py:57-61) and stepped at :265; the guarded form
 *                                          adds the rule of dmm_adam_step_guarded, which has nothing upstream
 *   dmm_adam_step_segmented_ema / dmm_adam_step_guarded_segmented_ema
 *                                          nothing upstream (the reference validates and saves the last iterate, :165-213): the
 *                                          segmented steps, keeping an exponential moving average of the parameters in the same launch
 *   dmm_adam_step_guarded / dmm_guard_* .. nothing upstream (the reference trains in fp32 with a bare Adam, :263-265); the rule is
 *                                          torch.amp.GradScaler's and the clip formula torch.nn.utils.clip_grad_norm_'s
 *   dmm_conv_forward / dmm_conv_wgrad .... single-kernel entry points for unit tests (torch.nn.functional.conv2d,
 *                                          conv_transpose2d as dispatched by the modules built at :72-131)
 *
 * Conventions: every function returns 0 on success and a negative dmm_status otherwise; dmm_last_error()
 * gives the message (thread-local).  The caller owns all buffers (device pointers are plain void*); the
 * library owns only the opaque plan.  A plan is bound to one device and is not thread-safe.  All launches go
 * to the hipStream_t passed as `stream` (a void* here so that the header needs no HIP include).
 */
#ifndef DMMFODS_HIP_H
#define DMMFODS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DMM_OK = 0,
  DMM_ERR_INVALID = -1,      /* bad argument / unsupported configuration (Python raises AttributeError/ValueError) */
  DMM_ERR_SHAPE = -2,        /* spatial size not a multiple of 32 (reference: ValueError from ConvTranspose2d) */
  DMM_ERR_HIP = -3,          /* a HIP call failed */
  DMM_ERR_STATE = -4,        /* plan not bound / wrong call order / a launch that the kernel family its plan recorded did not take */
  DMM_ERR_NO_DEVICE = -5
} dmm_status;

enum { DMM_F32 = 0, DMM_F16 = 1, DMM_BF16 = 2 };

/* tensor kinds in the state_dict table */
enum { DMM_T_CONV = 0, DMM_T_CONVT = 1, DMM_T_BN_WEIGHT = 2, DMM_T_BN_BIAS = 3, DMM_T_BN_MEAN = 4, DMM_T_BN_VAR = 5,
       DMM_T_BN_TRACKED = 6 };

/* Mirrors config.model.* of the reference (utils/Dense_U_Net_lidar_helper.py:110-123) plus the run shape. */
typedef struct {
  int32_t growth_rate;
  int32_t num_blocks;
  int32_t block_config[8];
  int32_t num_init_features;
  int32_t bn_size;
  int32_t num_classes;
  int32_t concat_before_block_num;
  int32_t stream_1_in_channels;
  int32_t stream_2_in_channels;
  int32_t batch, height, width; /* per-GPU minibatch and input size (H, W multiples of 32) */
  int32_t dtype;                /* DMM_F32 (parity), DMM_F16 or DMM_BF16 (storage/MFMA type; fp32 accumulate) */
  float loss_scale;             /* multiplies d(loss)/d(logit); gradients are un-scaled before they are returned */
  float bn_momentum, bn_eps;    /* 0.1, 1e-5 */
  float iou_threshold;          /* config.agent.iou_threshold, 0.7, applied to raw logits (reference quirk) */
  int32_t use_mfma;             /* 1 = MFMA kernels; 0 = scalar check kernels (bring-up / debugging) */
} dmm_model_desc;

typedef struct dmm_plan dmm_plan;

const char* dmm_last_error(void);
int dmm_version(void);
/* Switches for tests and A/B timing: "graph" (1 = replay captured launch lists, 2 = the forward list only; see dmm_plan_num_graph_replays), "overlap_wgrad" (1 = weight-gradient GEMMs on a second stream beside the
 * data-gradient chain, 0 = one stream; read at every call), "batch_wgrad" (the dense 3x3 weight gradients and the bw1 reductions of consecutive layers of a dense block
 * as grouped launches: 1, the default = on the caller's stream, 2 = on the weight-gradient stream, 0 = one launch per record as
 * without the option; read at every call, the same batches in every mode: see dmm_plan_wgrad_batch_counts), and the kernel families "thin_logits" (gather-once kernel for the
 * heat-map head's last convolution), "conv3" (LDS halo-tile kernels of the multi-tap convolutions), "wg3" (the growth convolution's
 * weight gradient), "wgp" (weight gradients of the parity-phase convolutions), "wg5" (of the 5x5 head / 7x7 stem convolutions),
 * "cvp" (the ConvTranspose kernels), "bw1" (fused backward of the 1x1 bottleneck convolutions), "pig" (persistent forward of the
 * 1x1 convolutions): 1 = on, 0 = generic kernels.  The family switches are one process-wide mask.
 * A plan chooses the family of each of its launches ONCE, in dmm_plan_bind, from the mask of that moment (it keeps a copy), and keeps it
 * (labels reported by dmm_plan_profile_op name the kernels that really run): toggle a switch BEFORE binding a plan.  The
 * single-kernel entry points below read the switches at every call.  "grad_bucket_mb": size of the data-parallel gradient
 * buckets of plans created afterwards.  Returns DMM_ERR_INVALID for an unknown name.  Results are identical up to the fp32
 * summation order. */
int dmm_set_option(const char* name, int value);

/* Plan construction needs no GPU: it derives the layer table, the state_dict layout and the workspace size. */
int dmm_plan_create(const dmm_model_desc* desc, dmm_plan** out);
/* Teardown (nothing upstream: the reference never frees a model explicitly, agents/Dense_U_Net_lidar_Agent.py:442-450).  The call
 * first SYNCHRONISES every helper stream the plan has launched on, so when it returns nothing the library enqueued outside the
 * caller's own stream still touches the workspace or the arenas; what was enqueued on the `stream` arguments of earlier calls is
 * the caller's to order before it frees those buffers.  The plan owns no stream: the helper streams belong to a per-device,
 * process-lifetime pool and the plan's events go back to it.  Returns DMM_OK, or DMM_ERR_HIP naming the first HIP call that
 * failed - the plan is gone either way and the handle must not be used again.  dmm_plan_destroy(NULL) is DMM_OK.
 * DMM_TRACE_DESTROY=1 in the environment writes one line per teardown step to stderr. */
int dmm_plan_destroy(dmm_plan* plan);

/* state_dict layout, in the reference's registration order */
int dmm_plan_num_tensors(const dmm_plan* plan);
/* shape has 4 entries (unused = 0), *arena_offset is in elements of the param arena (trainable tensors) or of the
 * buffer arena (running_mean / running_var); num_batches_tracked has no arena slot (offset -1). */
int dmm_plan_tensor_info(const dmm_plan* plan, int index, const char** name, int32_t* kind, int32_t* ndim,
                         int64_t shape[4], int64_t* arena_offset);
int64_t dmm_plan_num_params(const dmm_plan* plan);        /* elements of the param / grad arena */
int64_t dmm_plan_num_buffer_elems(const dmm_plan* plan);  /* elements of the running-stat arena */
size_t dmm_plan_workspace_bytes(const dmm_plan* plan);
double dmm_plan_forward_flops(const dmm_plan* plan);      /* 2*MACs of all convolutions, whole batch */

/* Bind device memory: workspace (>= workspace_bytes, 256-byte aligned), fp32 param arena, fp32 grad arena,
 * fp32 running-stat arena.  May be called again after a re-allocation. */
int dmm_plan_bind(dmm_plan* plan, void* workspace, size_t workspace_bytes, float* params, float* grads, float* buffers);

/* stream_1 (B,s1,H,W) and stream_2 (B,s2,H,W; may be NULL when s2 == 0) are fp32 NCHW device tensors;
 * logits_out is (B,num_classes,H,W) fp32 NCHW.  training != 0: batch statistics + running-stat update. */
int dmm_plan_forward(dmm_plan* plan, const float* stream_1, const float* stream_2, float* logits_out, int training,
                     void* stream);

/* After a training-mode forward: per-pixel BCE against target (B,num_classes,H,W fp32), metric counts, and the
 * backward pass of the SUM of all loss elements.  Gradients land in the bound grad arena: it is cleared first and every element
 * written (the default), or, with dmm_plan_set_grad_accumulate on, added to what the arena holds.
 * metrics_out (device, doubles): [NC loss sums | NC equal-counts | B x (NC intersections, NC unions)]. */
int dmm_plan_loss_backward(dmm_plan* plan, const float* logits, const float* target, double* metrics_out, void* stream);

/* Loss epilogue of dmm_plan_loss_backward / dmm_plan_loss_metrics.  DMM_LOSS_BCE (default): BCEWithLogitsLoss(reduction=
 * 'none'), agents/Dense_U_Net_lidar_Agent.py:54.  DMM_LOSS_FOCAL: alpha[c]*(1 - exp(-bce))**gamma[c]*bce per class c
 * (graphs/losses/FocalLoss.py:41-50 with equal entries, ClassWiseFocalLoss :78-91 otherwise); nclass = num_classes. */
enum { DMM_LOSS_BCE = 0, DMM_LOSS_FOCAL = 1 };
int dmm_plan_set_loss(dmm_plan* plan, int kind, const float* alpha, const float* gamma, int nclass);

/* The same loss kernel without a plan, on any (batch, nclass <= 8, height, width) fp32 NCHW tensors: unreduced loss
 * (loss_out, nullable) and d(sum of loss)/d(input) (dinput_out, nullable).  from_prob != 0: `input` holds probabilities
 * (FocalLoss(logits=False): F.binary_cross_entropy, graphs/losses/FocalLoss.py:43-44). */
int dmm_loss_forward(int kind, int from_prob, const float* alpha, const float* gamma, const float* input, const float* target,
                     float* loss_out, float* dinput_out, int batch, int nclass, int height, int width, void* stream);

/* ---- validation threshold sweep: per-class logit histograms in one pass ----
 * (Nothing upstream: the reference measures IoU and accuracy with raw logits cut at ONE number, config.agent.iou_threshold,
 * utils/Dense_U_Net_lidar_helper.py:311-401.  This is the same comparison at up to 255 numbers at once.)
 * logits and target are (B, NC, H, W) fp32 NCHW contiguous device tensors; thresholds are nthr strictly ascending finite fp32
 * values in HOST memory (they travel by value with the launch: nothing is uploaded and they may be stack memory).  Per element
 *   bin = #{k : x >= thresholds[k]}   0 .. nthr, compared in fp32; a NaN logit fails every comparison: bin 0
 *   g   = target >= gt_threshold      0 or 1; a NaN target: 0
 *   counts[b][n][g][bin] += 1         counts: int64 [B][NC][2][nthr + 1], device memory, dmm_logit_hist_elems elements
 * so that for threshold k   tp = sum_{j > k} counts[..][1][j],   fp = sum_{j > k} counts[..][0][j]   and every thresholded metric
 * follows from integers that are exact, independent of the launch geometry and add across batches and ranks.
 * accumulate == 0: counts is cleared on `stream` in front of the kernel; accumulate != 0: the kernel adds to what counts holds.
 * One launch, no plan, no synchronisation.  No limit on NC beyond B * NC <= 65535.
 * Refuses with DMM_ERR_INVALID, before any HIP call: a null pointer; logits or target not 4-byte aligned, counts not 8-byte
 * aligned; B, NC, H or W < 1; B * NC > 65535; H * W >= 2^31; nthr outside [1, DMM_HIST_MAX_THRESHOLDS]; a NaN or infinite
 * threshold; thresholds not strictly ascending; a NaN gt_threshold. */
#define DMM_HIST_MAX_THRESHOLDS 255
/* elements (int64) of the counts array: B * NC * 2 * (nthr + 1); 0 for arguments dmm_logit_hist would refuse */
size_t dmm_logit_hist_elems(int B, int NC, int nthr);
int dmm_logit_hist(const float* logits, const float* target, int B, int NC, int H, int W,
                   const float* thresholds /* host, nthr values */, int nthr, float gt_threshold,
                   int accumulate, int64_t* counts /* device */, void* stream);

/* ---- on-device batch augmentation: crop, flip, shift, gain and bias in one launch ----
 * (Nothing upstream: the reference trains on exactly what its loader yields, agents/Dense_U_Net_lidar_Agent.py:236-244.  These are
 * per-sample, label-preserving rearrangements of a batch that already sits on the device: image, LiDAR plane and heat maps move
 * together, so the pairing of input and label is kept.)
 * Up to DMM_AUG_MAX_TENSORS tensors of one batch - e.g. image, LiDAR, target, which may be channel slices of one (B, 7, H, W)
 * allocation - with at most DMM_AUG_MAX_CHANNELS channels between them, all of source size Hs x Ws and output size Ho x Wo.
 * Channels are numbered through the tensors in list order.  For sample b, channel c, output pixel (y, x):
 *   sy = y0 + y;   sx = x0 + (flip ? Wo - 1 - x : x)
 *   inside (0 <= sy < Hs and 0 <= sx < Ws):   v = src[b][c][sy][sx]
 *       gain[c] == 1 and bias[c] == 0 :  out = v, bit for bit (NaN payloads, -0 and infinities included)
 *       otherwise                      :  out = (gain[c] * v) + bias[c]     two fp32 roundings, never fused
 *   outside:                                  out = fill[c], untouched by gain and bias
 * Every element of every dst is written exactly once, nothing else is written, src is only read; no atomics, so the result does not
 * depend on the launch geometry.  All address arithmetic is 64-bit: only one plane (Hs * Ws, Ho * Wo) has to stay below 2^31.
 * samples and fill are HOST memory and travel by value with the launch (they may be stack memory; nothing is uploaded, nothing is
 * synchronised).  ceil(B / DMM_AUG_LAUNCH_BATCH) launches, each covering every tensor of the call; no plan.
 * Refuses with DMM_ERR_INVALID, before any HIP call: a null tensors or samples, a null src or dst; ntensors outside
 * [1, DMM_AUG_MAX_TENSORS]; channels < 1 or summing above DMM_AUG_MAX_CHANNELS; B, Hs, Ws, Ho or Wo < 1; Hs * Ws or Ho * Wo >= 2^31;
 * src_batch_stride < channels * Hs * Ws; a pointer that is not 4-byte aligned; flip other than 0 or 1; |y0| or |x0| above 2^30; a
 * NaN or infinite gain, bias (of a channel in use) or fill; a non-zero reserved field; a dst range that overlaps any tensor's src
 * span or another dst (in place is not supported). */
#define DMM_AUG_MAX_TENSORS   4
#define DMM_AUG_MAX_CHANNELS  8     /* summed over the tensors of one call */
#define DMM_AUG_LAUNCH_BATCH 32     /* samples whose parameters travel by value with one launch */
typedef struct dmm_aug_tensor {
  const float* src;          /*  0: (B, channels, Hs, Ws) fp32; planes and channels contiguous, samples src_batch_stride apart */
  float* dst;                /*  8: (B, channels, Ho, Wo) fp32 NCHW contiguous */
  int64_t src_batch_stride;  /* 16: elements, >= channels * Hs * Ws (a channel slice of an (N, 7, H, W) batch is such a tensor) */
  int32_t channels;          /* 24 */
  int32_t reserved;          /* 28: 0 */
} dmm_aug_tensor;            /* 32 bytes */
typedef struct dmm_aug_sample {
  int32_t y0, x0;            /*  0, 4: source position of the window's top-left corner; may be negative, the window may overhang */
  int32_t flip;              /*  8: 0 / 1: the window is read mirrored left-right */
  int32_t reserved;          /* 12: 0 */
  float gain[DMM_AUG_MAX_CHANNELS];   /* 16: per channel, numbered through the tensors in list order */
  float bias[DMM_AUG_MAX_CHANNELS];   /* 48 */
} dmm_aug_sample;            /* 80 bytes */
int dmm_augment_batch(const dmm_aug_tensor* tensors, int ntensors,
                      const dmm_aug_sample* samples /* host, B entries */, int B,
                      int Hs, int Ws, int Ho, int Wo,
                      const float* fill /* host, one value per channel; NULL = zeros */, void* stream);

/* ---- on-device affine warp: scale and rotation (and every window of dmm_augment_batch) in one launch ----
 * (Nothing upstream.)  The sibling of dmm_augment_batch for maps that do not land on whole pixels.  Tensors, channels, sizes, strides,
 * fill, the by-value travel of samples and fill, the 64-bit address arithmetic and the absence of a plan are dmm_augment_batch's; a
 * tensor also names how it is SAMPLED, and a sample carries an affine map in fixed point, F = DMM_WARP_FRAC_BITS, ONE = 1 << F,
 * HALF = ONE / 2, MASK = ONE - 1.  For sample b, channel c of a tensor, output pixel (x, y), all in int64 and exact:
 *   SX = a00 * x + a01 * y + b0          SY = a10 * x + a11 * y + b1
 * DMM_WARP_NEAREST:
 *   sx = (SX + HALF) >> F, sy = (SY + HALF) >> F          (arithmetic shifts: floors, so a half rounds up)
 *   inside (0 <= sx < Ws and 0 <= sy < Hs):  v = src[b][c][sy][sx], then the gain / bias rule of dmm_augment_batch:
 *       gain[c] == 1 and bias[c] == 0 :  out = v, bit for bit;     otherwise :  out = (gain[c] * v) + bias[c], two fp32 roundings
 *   outside:                                 out = fill[c], untouched by gain and bias
 * DMM_WARP_BILINEAR:
 *   x0 = SX >> F, fx = SX & MASK, wx = float(fx) * 2^-F (exact);  y0, fy, wy likewise.  Taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *   (x0 + 1, y0 + 1) have the values v00, v01, v10, v11; a tap outside the source has the value fill[c].
 *   fx == 0 and fy == 0:     the pixel is tap 00 alone, exactly as DMM_WARP_NEAREST treats (sx, sy) = (x0, y0): inside, the source's bits
 *                            and then the gain / bias rule; outside, fill[c] untouched.  A map whose six coefficients are multiples of
 *                            ONE is therefore a pure rearrangement and equals dmm_augment_batch on the same window bit for bit.
 *   all four taps outside:   out = fill[c], untouched by gain and bias
 *   otherwise, each operation one fp32 rounding, never fused, in this order:
 *       top = v00 + wx * (v01 - v00);   bot = v10 + wx * (v11 - v10);   v = top + wy * (bot - top);   then the gain / bias rule on v
 * Every element of every dst is written exactly once, nothing else is written, src is only read; no atomics, so the result does not
 * depend on the launch geometry.  ceil(B / DMM_WARP_LAUNCH_BATCH) launches.
 * Refuses with DMM_ERR_INVALID, before any HIP call, everything dmm_augment_batch refuses (with flip, y0 and x0 gone) and: a mode other
 * than 0 or 1; a matrix entry with |a| > DMM_WARP_MAX_A (64 in fixed point); an offset with |b| > DMM_WARP_MAX_B (2^50).
 * With x, y < 2^31 (a plane is smaller): |a * x| < 2^26 * 2^31 = 2^57, two such terms < 2^58, and with |b| + HALF <= 2^50 + 2^19 the sums
 * stay below 2^58 + 2^51 < 2^59: nothing wraps in int64, and a coordinate after the shift is below 2^39 in magnitude. */
#define DMM_WARP_NEAREST       0
#define DMM_WARP_BILINEAR      1
#define DMM_WARP_FRAC_BITS    20
#define DMM_WARP_LAUNCH_BATCH 32     /* 32 records of 96 bytes and 344 bytes of channels, fill, modes and sizes: 3416 of the 4096 bytes */
#define DMM_WARP_MAX_A  (64 << DMM_WARP_FRAC_BITS)
#define DMM_WARP_MAX_B  (1ll << 50)
typedef struct dmm_warp_tensor {
  const float* src;          /*  0: as dmm_aug_tensor */
  float* dst;                /*  8 */
  int64_t src_batch_stride;  /* 16 */
  int32_t channels;          /* 24 */
  int32_t mode;              /* 28: DMM_WARP_NEAREST / DMM_WARP_BILINEAR, for every channel of the tensor */
  int32_t reserved[2];       /* 32: 0 */
} dmm_warp_tensor;           /* 40 bytes */
typedef struct dmm_warp_sample {
  int32_t a00, a01, a10, a11;         /*  0, 4, 8, 12: the matrix, Q20 */
  int64_t b0, b1;                     /* 16, 24: the offsets, Q20 */
  float gain[DMM_AUG_MAX_CHANNELS];   /* 32 */
  float bias[DMM_AUG_MAX_CHANNELS];   /* 64 */
} dmm_warp_sample;           /* 96 bytes */
int dmm_warp_batch(const dmm_warp_tensor* tensors, int ntensors,
                   const dmm_warp_sample* samples /* host, B entries */, int B,
                   int Hs, int Ws, int Ho, int Wo,
                   const float* fill /* host, one value per channel; NULL = zeros */, void* stream);

/* ---- heat maps to objects: connected components and one record per component ----
 * (Nothing upstream: the reference measures whole-image pixel counts only, utils/Dense_U_Net_lidar_helper.py
 * compute_IoU_whole_img_per_class.  This turns a heat map - logits or a rendered target map - into the objects it shows.)
 * maps is a (B, NC, H, W) fp32 NCHW contiguous device tensor.  A pixel is foreground iff x >= threshold, compared in fp32: a value on
 * the threshold is foreground, NaN is not, -0.0 >= 0.0 holds.  Components are taken per (b, n) plane under 4- or 8-connectivity;
 * planes never touch and rows do not wrap.  A component's label is its ROOT, the smallest y * W + x among its pixels (plane-relative
 * int32); background pixels have label -1.  Per plane the records stand in ascending root order; when a plane has more components
 * than max_per_plane the max_per_plane smallest roots are kept, counts still holds the true number, and the slots behind
 * min(count, max_per_plane) are zero.  score is the component's largest value in the order that puts -0.0 below +0.0 (they compare
 * equal; the order is over the bit patterns), peak the first pixel in raster order that holds that value.  Every output is an
 * integer or a copied input value: exact, bit-reproducible, independent of the launch geometry.  No floating-point atomics.
 * Seven kernel launches on `stream`; no plan, no synchronisation, no memset, nothing uploaded from host memory.
 * workspace: dmm_heat_components_workspace bytes of device memory, 16-byte aligned, contents undefined before and after.
 * Refuses with DMM_ERR_INVALID, before any HIP call: a null maps, workspace, records or counts; maps, labels or counts not 4-byte
 * aligned, records not 8-byte aligned, workspace not 16-byte aligned; B, NC, H or W < 1; H * W >= 2^31; B * NC > 65535 (gridDim.y);
 * connectivity other than 4 or 8; max_per_plane outside [1, 65536]; a NaN threshold; workspace_bytes below
 * dmm_heat_components_workspace(...). */
#define DMM_CC_TILE_H 32   /* one workgroup labels a DMM_CC_TILE_H x DMM_CC_TILE_W tile in LDS; tiles are then merged along their borders */
#define DMM_CC_TILE_W 32
#define DMM_CC_MAX_PER_PLANE 65536
typedef struct dmm_component {   /* 32 bytes */
  int32_t root;                  /* y * W + x of the component's first pixel in raster order */
  int32_t x0, y0, x1, y1;        /* inclusive pixel box */
  int32_t area;                  /* pixels */
  float   score;                 /* largest value in the component */
  int32_t peak;                  /* linear index of the first pixel in raster order holding `score` */
} dmm_component;
size_t dmm_heat_components_workspace(int B, int NC, int H, int W, int max_per_plane);   /* bytes; 0 for refused arguments */
int dmm_heat_components(const float* maps, int B, int NC, int H, int W, float threshold, int connectivity /* 4 | 8 */,
                        int max_per_plane, void* workspace, size_t workspace_bytes,
                        int32_t* labels /* device, B*NC*H*W, may be NULL */,
                        dmm_component* records /* device, [B*NC][max_per_plane] */,
                        int32_t* counts /* device, [B*NC]: the TRUE number of components, may exceed max_per_plane */,
                        void* stream);

/* ---- object matching: greedy IoU pairing of the records of two dmm_heat_components calls ----
 * (Nothing upstream.  detect.match_plane / match_objects / ObjectMetrics of the Python package state the same rule on the host and
 * are this entry point's reference.)
 * pred and gt are the records, pred_counts and gt_counts the counts dmm_heat_components wrote for the predictions and for the targets
 * of one batch: (B, NC, cap, 8) int32 and (B, NC), with caps of their own.  A plane's kept records are its first min(count, cap)
 * slots (a negative count keeps none), in ascending root order; the slots behind them are never read.  A record TAKES PART iff it is
 * kept and area >= min_area, predictions and ground truth alike.  Per (b, n) plane the participating predictions are visited in
 * descending score - an fp32 compare: +0.0 and -0.0 tie, negative scores order correctly; ties go to the ascending root, which is the
 * lower slot; scores are never NaN, NaN is not foreground - and the visited prediction takes the still untaken participating
 * ground-truth record of highest IoU with IoU >= iou, ties to the lower root.  IoU is over the inclusive boxes in fp64:
 *   iw = min(x1) - max(x0) + 1, ih likewise; 0 unless both are positive; inter = double(iw) * double(ih);
 *   area = double(x1 - x0 + 1) * double(y1 - y0 + 1) from the corners (not the record's component area);
 *   v = inter / (area_a + area_b - inter): every operand an exact integer, ONE correctly rounded division; v >= iou and v > best
 *   are fp64 compares.  3 of 10 pixels match at iou = 0.3.
 * matched (may be NULL): (B, NC, cap_pred) uint8, 1 in the slot of a matched prediction, 0 in every other slot below cap_pred -
 *   filtered out, unmatched or unfilled; each element is written exactly once.
 * totals: (NC, 8) int64, the state of an epoch, which the call ADDS to: tp, fp, fn, num_pred, num_gt, overflowed_planes, cursor,
 *   reserved.  num_pred and num_gt count participating records, tp + fp = num_pred, tp + fn = num_gt; overflowed_planes counts the
 *   planes with count > cap on the prediction side plus those on the ground-truth side.  The caller zeroes it at the epoch's start.
 * entries: (NC, capacity, 2) int32, (score bits, matched) per participating prediction in order of arrival - call, then sample,
 *   then ascending root: the entry's position is totals[n].cursor before the call, plus the participating predictions of class n in
 *   the samples before this one, plus its index among those of its plane.  A position >= capacity is not written; cursor advances by
 *   the full number whatever the capacity, so max(0, cursor - capacity) predictions were dropped.
 * Every output is an integer or a copied input value and every reduction an integer add: exact, bit-reproducible, independent of the
 * launch geometry and of the order of arrival.  No floating-point atomics.  Three kernel launches on `stream`; no plan, no
 * synchronisation, no memset, nothing uploaded from host memory, nothing allocated.
 * workspace: dmm_match_objects_workspace bytes of device memory, 16-byte aligned, contents undefined before and after.
 * Refuses with DMM_ERR_INVALID, before any HIP call, "dmm_match_objects: " in front of the message: a null pred, pred_counts, gt,
 * gt_counts, workspace, totals or entries; records not 8-byte aligned, counts not 4-byte aligned, totals not 8-byte aligned, entries
 * not 4-byte aligned, workspace not 16-byte aligned; B or NC < 1; B * NC > 65535; cap_pred or cap_gt outside
 * [1, DMM_MATCH_MAX_PER_PLANE] (the walk is serial in the predictions and the rank quadratic: dmm_heat_components' own maximum of
 * 65536 records a plane is refused here); min_area < 1; iou NaN or outside (0, 1]; capacity < 1 or > 2^31 - 1; workspace_bytes below
 * dmm_match_objects_workspace(...). */
#define DMM_MATCH_MAX_PER_PLANE 4096
size_t dmm_match_objects_workspace(int B, int NC, int cap_pred, int cap_gt);   /* bytes; 0 for refused arguments */
int dmm_match_objects(const dmm_component* pred, const int32_t* pred_counts, int cap_pred,
                      const dmm_component* gt, const int32_t* gt_counts, int cap_gt,
                      int B, int NC, int min_area, double iou,
                      void* workspace, size_t workspace_bytes,
                      uint8_t* matched /* device, (B, NC, cap_pred), may be NULL */,
                      int64_t* totals /* device, (NC, 8) */, int32_t* entries /* device, (NC, capacity, 2) */, int64_t capacity,
                      void* stream);

/* ---- raw frames to training tensors: image, LiDAR points and boxes become the (B, 7, Ho, Wo) batch on the device ----
 * (Upstream this is host code: avgpool_tensor / lidar_array_to_image_like_tensor / pool_lidar_tensor / create_ground_truth_maps /
 * maxpool_tensor of utils/Dense_U_Net_lidar_helper.py, whose seven fp32 planes per frame the loader then copies to the device.)
 * Three independent entry points; p = pool, Ho = H / p, Wo = W / p, H and W multiples of p.  Each dst is fp32 (B, channels, Ho, Wo)
 * with planes contiguous and samples dst_batch_stride ELEMENTS apart, so the three outputs may be the channel slices 0:3, 3:4 and 4:7
 * of one (B, 7, Ho, Wo) allocation.  Plain launches on `stream`: no plan, no synchronisation, nothing uploaded - `offsets` are HOST
 * arrays of B + 1 entries that travel by value, DMM_PREP_LAUNCH_BATCH samples per launch.  Every dst element is written exactly once
 * and nothing else is written (dmm_prep_lidar also writes its workspace); inputs are only read.  Every output is exact: independent
 * of the launch geometry and bit-reproducible.  No floating-point atomics.  Address arithmetic is 64-bit: only H * W stays below 2^31.
 *
 * dmm_prep_image: src is uint8 (B, H, W, C), channel-last, C in 1..4, samples src_batch_stride BYTES apart.
 *   out[b][c][i][j] = fdiv_rn(float(S), float(p * p)),  S the exact integer sum of the p x p block: one correctly rounded division
 *   (torch.nn.AvgPool2d on the CPU; a multiplication with the reciprocal differs for p = 3, 10).  p == 1 is the plain cast.
 *   ceil(B / 32) launches.
 *
 * dmm_prep_lidar: points is fp32 (n, 3) of (x, y, d), concatenated over the batch; sample b owns [offsets[b], offsets[b + 1]).
 *   kernel_size k is odd, 1..15, s = (k - 1) / 2.  A point is valid iff x, y, d are finite and >= 0 (-0.0 is); any other writes nothing.
 *   With cx = (int)x, cy = (int)y it covers rows [max(cy - s, 0), min(cy + s + 1, H - 1)) and columns [max(cx - s, 0),
 *   min(cx + s + 1, W - 1)): the last row and column are never written (upstream's clip).  A pixel holds the d of the highest-indexed
 *   point of its sample that covers it, -1 where none does.  e = 76 where the value is -1, else min(v, 75);
 *   code = e <= 25 ? (e * -6.2f) + 255 : (e * -2) + 150, two fp32 roundings, never fused.  p >= 2 (needs H >= 2p): out[i][j] =
 *   max(0, max of code over rows [r * p, r * p + 2p), columns [j * p, j * p + p)), r = min(i, Ho - 2) - upstream's
 *   MaxPool2d((2p, p), stride p), one replicated bottom row and the clamp.  p == 1: out = max(0, code).
 *   workspace: dmm_prep_lidar_workspace bytes of device memory, 16-byte aligned: an int32 owner plane per sample.  One
 *   hipMemsetAsync, then per 32 samples the splat launch (an integer atomicMax per point and window pixel; none when those samples
 *   have no point) and the pool launch.
 *
 * dmm_prep_heat_maps: boxes is an array of dmm_prep_box, concatenated over the batch, ranges from offsets as above.  type 1 -> plane
 *   0, 2 -> plane 1, 4 -> plane 2; any other type and any box with width <= 0 or height <= 0 is ignored.  A full-resolution pixel
 *   (Y, X) of a plane takes the pattern value of the LAST box of that class in list order with x <= X < x + width and y <= Y < y +
 *   height (64-bit), 0 where there is none; boxes are clipped to the image, the pattern stays relative to the unclipped corner.
 *   Pattern at r = Y - y, c = X - x, hf = height / 5, wf = width / 4: types 1 and 4 give 1; type 2, side = (c < wf || c >= 3 * wf):
 *   r < hf && side -> 0.3f;  else r >= 3 * hf -> side ? 0.5f : 0.75f;  else 1.  The output pixel is the maximum over its p x p block.
 *   No cap on boxes per sample.  ceil(B / 32) launches.
 *
 * Each refuses with DMM_ERR_INVALID, before any HIP call, its own name in front of the message: a null pointer (points / boxes may be
 * null when the batch has none); src, dst, points, boxes not aligned to their element (1 / 4 bytes); B, H, W or pool < 1; H or W no
 * multiple of pool; H < 2 * pool for LiDAR with pool >= 2; H * W >= 2^31; C outside 1..4; kernel_size even or outside 1..15; a batch
 * stride below one sample; offsets[0] != 0, decreasing offsets, a total above 2^31 / 256; a workspace that is null, not 16-byte
 * aligned or smaller than dmm_prep_lidar_workspace. */
#define DMM_PREP_LAUNCH_BATCH 32   /* samples whose offsets travel by value with one launch */
#define DMM_PREP_MAX_ITEMS (1 << 23)   /* 2^31 / 256: points, or boxes, of one call */
typedef struct dmm_prep_box {
  int32_t type;            /*  0: 1 vehicle, 2 pedestrian, 4 cyclist (upstream's label dict) */
  int32_t x, y;            /*  4, 8: top-left corner, full-resolution pixels; may lie outside the image */
  int32_t width, height;   /* 12, 16 */
} dmm_prep_box;            /* 20 bytes */
int dmm_prep_image(const uint8_t* src, int64_t src_batch_stride /* bytes */, float* dst, int64_t dst_batch_stride,
                   int B, int H, int W, int C, int pool, void* stream);
size_t dmm_prep_lidar_workspace(int B, int H, int W);   /* bytes; 0 for refused arguments */
int dmm_prep_lidar(const float* points, const int32_t* offsets /* host, B + 1 */, float* dst, int64_t dst_batch_stride,
                   int B, int H, int W, int pool, int kernel_size, void* workspace, size_t workspace_bytes, void* stream);
int dmm_prep_heat_maps(const dmm_prep_box* boxes, const int32_t* offsets /* host, B + 1 */, float* dst, int64_t dst_batch_stride,
                       int B, int H, int W, int pool, void* stream);

/* Backward from an externally computed d(loss)/d(logit) (B,num_classes,H,W fp32), e.g. from torch autograd of any
 * loss on the returned logits (reference: loss.backward(...), agents/Dense_U_Net_lidar_Agent.py:264). */
int dmm_plan_backward(dmm_plan* plan, const float* dlogits, void* stream);

/* Gradient accumulation over micro-batches (torch's backward() contract; the reference always clears first,
 * agents/Dense_U_Net_lidar_Agent.py:263).  accumulate != 0: dmm_plan_loss_backward and dmm_plan_backward no longer clear the
 * gradient arena, and every launch that writes it (the weight-gradient unpack, the BatchNorm-backward finalize) adds to it; clearing
 * the arena between windows is the caller's job (one memset of num_params floats).  The loss is a sum, so the arena then holds the
 * gradient of the concatenated batch, with BatchNorm statistics per micro-batch.  0 (the default): the launches and the numbers of a
 * plan that never had the mode.  The launch list, its labels, gradient buckets and events are the same in both modes.  Changing
 * the mode drops the plan's captured backward graph (it is captured again, see dmm_plan_num_graph_replays); the setting survives
 * dmm_plan_bind.  Several plans bound to one arena (different input sizes) accumulate into it together when each has the mode on. */
int dmm_plan_set_grad_accumulate(dmm_plan* plan, int accumulate);

/* Frozen encoder: train the decoder and the head on an encoder that stays as it is (e.g. loaded from a pretrained checkpoint), as
 * requires_grad = False on every parameter under `features`, `stream_2_features` and `concat_module` does in torch.  frozen != 0:
 *   - the backward list is the default list up to and excluding the first encoder record (records are walked from the head back, so
 *     every decoder / head launch comes first and keeps its kernel family and arguments); no launch of it writes an encoder range of
 *     the gradient arena, which therefore reads zero behind a backward (the arena is still cleared whole) or, with
 *     dmm_plan_set_grad_accumulate on, keeps what it held;
 *   - dmm_plan_num_grad_buckets / dmm_plan_grad_bucket describe trainable tensors only; the unpack tables hold no encoder tensor;
 *   - the forward lists are unchanged: frozen BatchNorms still normalise with batch statistics and update their running statistics
 *     in a training forward, as torch's do with requires_grad = False.
 * Legal only between dmm_plan_create and dmm_plan_bind: the call runs the sizing pass again (dmm_plan_workspace_bytes is that of the
 * mode and never larger than the default's); a bound plan returns DMM_ERR_STATE, a null plan DMM_ERR_INVALID.  The setting survives
 * dmm_plan_bind.  0 on a fresh plan changes nothing.  The optimiser must leave the frozen ranges alone: the segmented
 * calls (dmm_adam_step_segmented / dmm_adam_step_guarded_segmented) under a table of the trainable ranges, one class per step origin
 * (they replace the guarded step over ranges that earlier versions of this header declared), or dmm_adam_step per range. */
int dmm_plan_set_encoder_frozen(dmm_plan* plan, int frozen);

/* Data-parallel training (new here; the reference's torch.distributed import, graphs/models/Dense_U_Net_lidar.py:7, is unused):
 * the gradient arena is cut into buckets of whole tensors (about dmm_set_option("grad_bucket_mb", 25) each, set before
 * dmm_plan_create) listed in the order in which backward finishes them (head, decoder, block 4 ... stems).
 * dmm_plan_grad_bucket_wait makes `stream` wait until bucket `index` of the most recently enqueued backward is final, so an
 * all-reduce enqueued on that stream runs beside the rest of backward. */
int dmm_plan_num_grad_buckets(const dmm_plan* plan);
int dmm_plan_grad_bucket(const dmm_plan* plan, int index, int64_t* offset, int64_t* count);
int dmm_plan_grad_bucket_wait(dmm_plan* plan, int index, void* stream);

/* Per-launch timing with HIP events recorded on the launch stream (used by bench.py for the roofline block).
 * which: 0 = training forward, 1 = loss + backward.  profile_begin(plan, n) arms recording for the next n passes of
 * each; profile_collect sums per-op milliseconds over the recorded passes (synchronise the stream first).
 * profile_filter(plan, "igemm.bnbwd.n128/") restricts the event pairs to the launches whose label starts with the prefix
 * (NULL or "" = every launch).  Unfiltered profiling serialises everything on one stream so that each pair brackets one
 * kernel alone; a filtered profile runs exactly as in production (weight gradients on the side stream) and costs two
 * event records per selected launch. */
int dmm_plan_profile_begin(dmm_plan* plan, int max_passes);
int dmm_plan_profile_filter(dmm_plan* plan, const char* label_prefix);
int dmm_plan_profile_num_ops(const dmm_plan* plan, int which);
int dmm_plan_profile_op(const dmm_plan* plan, int which, int index, const char** label, double* flops, double* bytes);
int dmm_plan_profile_collect(dmm_plan* plan, int which, double* ms_sum, int n, int* passes);

/* Loss + metrics only (validation). */
int dmm_plan_loss_metrics(dmm_plan* plan, const float* logits, const float* target, double* metrics_out, void* stream);

/* Launch-list replay.  dmm_plan_forward (training) and dmm_plan_loss_backward run their ~350 / ~750 launches eagerly the first time;
 * the second time, the part of the list that touches no caller pointer (everything between the stem convolution and the logits
 * kernel; everything behind the loss kernel; as one chain on one stream) is captured once into a hipGraph
 * and replayed by ONE call from then on, whatever tensors the caller passes.  OFF by default (dmm_set_option("graph", 1) /
 * DMM_GRAPH=1 turn it on): measured on MI355X it cuts the host's enqueue time of a step from 14-25 ms to 0.5 ms but not the GPU's
 * time, and the replayed chain is single-stream, i.e. slower than the eager two-stream schedule (capi.cpp, launch_list).  Any
 * dmm_set_option drops the captured graphs.  Not replayed: profiled passes, the eval forward,
 * dmm_plan_backward, and the backward of a plan whose gradient buckets are waited for (dmm_plan_grad_bucket_wait: data-parallel
 * overlap needs the bucket events at their place inside the list).  which: 0 training forward, 1 loss + backward. */
long long dmm_plan_num_graph_replays(const dmm_plan* plan, int which);
/* Launch coalescing ("batch_wgrad"), summed over every launch list the plan has run: counts[0] = launches of the dense 3x3 weight
 * gradient kernel (a grouped launch counts once; each is followed by one reduction launch), counts[1] = the launch records they
 * served, counts[2] = launches of the bw1 reduction, counts[3] = the bw1.reduce records they served.  With the option off
 * counts[0] == counts[1] and counts[2] == counts[3].  (Nothing upstream: the reference has no launch lists.) */
int dmm_plan_wgrad_batch_counts(const dmm_plan* plan, long long counts[4]);

/* Flat fused Adam over n fp32 elements, one parameter group (amsgrad unsupported): torch.optim.Adam's single-tensor arithmetic in
 * fp32, weight_decay added to the gradient (L2, not decoupled), the bias corrections of `step` (1-based) formed on the host in
 * double.  Every gradient is multiplied by grad_scale first.  One launch of the library's one Adam kernel in its
 * whole-range form (no table; 16-byte accesses when the four pointers are 16-byte aligned, element by element otherwise); several
 * groups, or frozen ranges in between: the segmented calls below, the same kernel under a table. */
int dmm_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* stream);

/* ---- guarded optimiser step: dynamic loss scale, skipped step on overflow, clipping by global norm ----
 * Everything is decided on the device; no call below synchronises with the host.  The state lives in one 64-byte device block owned
 * by the caller.  S = `scale` is the dynamic loss scale in force during the backward that filled the gradient arena, which therefore
 * holds S x the true gradients (the plan's static dmm_model_desc.loss_scale is applied and removed inside the plan as before; S
 * multiplies on top, see dmm_plan_set_dynamic_loss_scale).  Per step:
 *   sumsq = sum g^2 over the arena as stored (squares and sum in fp64);  found_inf = sumsq is inf or NaN
 *   found_inf:  params, exp_avg, exp_avg_sq, applied_steps unchanged;  scale = S * backoff_factor, growth_tracker = 0, skipped_steps += 1
 *   otherwise:  grad_norm = sqrt(sumsq) / S;  clip_coef = min(1, max_norm / (grad_norm + 1e-6)) (1 without max_norm);
 *               Adam on g * clip_coef / S with the bias corrections of step applied_steps + 1;  applied_steps += 1;
 *               growth_tracker += 1, and when it reaches growth_interval: scale = S * growth_factor, growth_tracker = 0.
 * A skipped step's forward has already updated the BatchNorm running statistics (as with torch.amp). */
typedef struct dmm_guard_state {
  float scale;            /*  0: dynamic loss scale S of the NEXT backward (what the plan's loss kernel reads); may fall below 1 */
  float grad_scale;       /*  4: clip_coef / S of the last step: what its Adam multiplied every gradient by (0 on a skipped step) */
  double sumsq;           /*  8: sum of squares of the arena as stored (scaled by S), fp64; inf / NaN on a skipped step */
  float grad_norm;        /* 16: sqrt(sumsq) / S, the global gradient norm before clipping (inf / NaN on a skipped step) */
  int32_t found_inf;      /* 20: 1 = the last step was skipped */
  int64_t applied_steps;  /* 24: optimiser steps applied so far (Adam's t) */
  int64_t skipped_steps;  /* 32: steps skipped since dmm_guard_state_init */
  int32_t growth_tracker; /* 40: applied steps since the scale last changed */
  float step_size;        /* 44: lr / (1 - beta1^t) of the last applied step */
  float bc2_sqrt;         /* 48: sqrt(1 - beta2^t) of the last applied step */
  float clip_coef;        /* 52: clip coefficient of the last step (1 = not clipped, 0 on a skipped step) */
  int32_t reserved[2];    /* 56: padding to 64 bytes */
} dmm_guard_state;

/* Bytes of the reduction scratch for an arena of n elements (one fp64 partial sum per workgroup; device memory, 8-byte aligned). */
size_t dmm_grad_guard_scratch_bytes(int64_t n);
/* Fills *dev (device memory, 8-byte aligned) on `stream`: start of training, checkpoint load.  init_scale > 0. */
int dmm_guard_state_init(dmm_guard_state* dev, float init_scale, int64_t applied_steps, int32_t growth_tracker, void* stream);
/* Enqueues three kernels: the arena reduction (16-byte loads, a workgroup owns its partial: no floating-point atomics, so the result
 * is bit-reproducible), the finalize kernel (partials added in a fixed order; the rule above; bias corrections computed in fp64 on the
 * device from applied_steps, which the host does not know without a synchronisation), and Adam, which reads its scalars from *state
 * and writes nothing on a skipped step.  max_norm <= 0: no clipping.  growth_interval 0: the scale never grows (it still backs off).
 * growth_factor >= 1, 0 < backoff_factor <= 1 (1 and 1 with growth_interval 0 keep S fixed, e.g. clipping alone with S = 1).
 * scratch: >= dmm_grad_guard_scratch_bytes(n). */
int dmm_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                          float beta2, float eps, float weight_decay, float max_norm, float growth_factor, float backoff_factor,
                          int32_t growth_interval, dmm_guard_state* state, void* scratch, void* stream);
/* The reduction alone, on elements [offset, offset + count) of `grads`: scratch = (accumulate ? scratch : 0) + partial sums of the
 * range.  dmm_adam_step_guarded runs it once over the whole arena; a data-parallel trainer can run it per gradient bucket behind
 * that bucket's all-reduce instead (not wired up yet).  Also what the unit tests and the cost measurement call. */
int dmm_grad_sumsq(const float* grads, int64_t offset, int64_t count, int accumulate, void* scratch, void* stream);
/* ---- parameter groups: segmented Adam, one launch ----
 * (torch.optim.Adam over parameter groups, agents/Dense_U_Net_lidar_Agent.py:57-61: each group has its own lr, betas, eps and
 * weight_decay; torch counts steps per parameter.)
 * A SEGMENT is a range [begin, begin + count) of the flat arenas (elements) with a class; segments are sorted by begin and disjoint.
 * Elements in no segment - frozen parameters - are neither read nor written, in params, exp_avg or exp_avg_sq (nor read in grads).
 * A CLASS is a (parameter group, step origin t0) pair: the hyper-parameters of the group and the applied-step count at which its
 * parameters began to train, so that a class is at its own step `step - t0`.  A class whose own step is below 1 writes nothing.
 * At most DMM_ADAM_MAX_CLASSES classes; they travel by value with every launch, so a changed lr needs no new table.
 * decoupled == 0: dmm_adam_step's arithmetic, expression for expression.  decoupled != 0 (AdamW): the parameter is first multiplied
 * by (float)(1.0 - (double)lr * weight_decay) and the gradient gets no weight_decay * p term; the rest is identical. */
#define DMM_ADAM_MAX_CLASSES 16
typedef struct dmm_adam_segment {
  int64_t begin, count;   /*  0, 8: elements */
  int32_t cls;            /* 16: index into the classes of the step call */
} dmm_adam_segment;       /* 24 bytes */
typedef struct dmm_adam_class {
  float lr, beta1, beta2, eps, weight_decay;   /* 0 .. 16 */
  int32_t decoupled;                           /* 20 */
  int64_t t0;                                  /* 24 */
} dmm_adam_class;                              /* 32 bytes */
/* Bytes of the device form of a table of nsegs segments over arenas of n elements (the segments, and for every chunk of 1024
 * elements the index of the first segment that reaches into it or lies behind it, so that a workgroup needs no search).
 * 0 for nsegs < 1 or n < 1. */
size_t dmm_adam_table_bytes(int nsegs, int64_t n);
/* Validates the segments on the host and uploads the table to table_dev (caller-owned device memory, 8-byte aligned,
 * >= dmm_adam_table_bytes(nsegs, n)).  Waits for `stream`, then copies: the upload is COMPLETE when the call returns (segs may be
 * stack memory), as with the single-kernel entry points.  The library remembers, per table_dev, the sizes and the maximal contiguous
 * runs of the table it uploaded there; the step calls refuse a table_dev they were not given by this call with the same nsegs and n.
 * Refuses, before any HIP call: a null or misaligned pointer, nsegs < 1, n < 1, nclasses outside [1, DMM_ADAM_MAX_CLASSES],
 * count < 1, a segment outside [0, n), unsorted or overlapping segments, cls outside [0, nclasses). */
int dmm_adam_table_init(void* table_dev, const dmm_adam_segment* segs, int nsegs, int64_t n, int nclasses, void* stream);
/* ONE launch over the arenas of n elements under the table: a capped grid walks the chunks with a grid-stride loop; a 4-element vector
 * that lies inside one segment moves with 16-byte loads and stores (when the four arenas are 16-byte aligned), segment edges go
 * element by element.  step_size and bc2_sqrt of each class are formed as in dmm_adam_step, on the host, in double, for step - t0.
 * Refuses, before any HIP call: null or misaligned (4-byte) pointers, nsegs < 1, a table_dev not initialised for (nsegs, n),
 * nclasses outside [1, DMM_ADAM_MAX_CLASSES] or other than the table's, betas outside [0, 1), a NaN or negative lr, eps or
 * weight_decay, t0 < 0, step < 1. */
int dmm_adam_step_segmented(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const void* table_dev,
                            int nsegs, const dmm_adam_class* classes, int nclasses, int64_t step, float grad_scale, void* stream);
/* The guarded step (the rule above dmm_guard_state) under a table: one reduction per maximal contiguous run of segments, whatever
 * their classes (the first assigns the partials, the rest add; nothing frozen: one reduction), ONE finalize fed classes[0]'s lr and
 * betas - so step_size and bc2_sqrt in the state block describe class 0 at t0 = 0 and are not what the other classes use - and the
 * one segmented Adam launch, which forms step_size and bc2_sqrt of every class on the device, in fp64, from
 * t = state->applied_steps - t0 - step_size = (float)(lr / (1 - beta1^t)), bc2_sqrt = (float)sqrt(1 - beta2^t), the finalize kernel's
 * expressions - and writes nothing on a skipped step or for a class with t < 1.
 * Refuses what dmm_adam_step_segmented and dmm_adam_step_guarded refuse (there is no step argument). */
int dmm_adam_step_guarded_segmented(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    const void* table_dev, int nsegs, const dmm_adam_class* classes, int nclasses, float max_norm,
                                    float growth_factor, float backoff_factor, int32_t growth_interval, dmm_guard_state* state,
                                    void* scratch, void* stream);
/* ---- parameter average (EMA), kept by the Adam launch ----
 * The two calls below are dmm_adam_step_segmented / dmm_adam_step_guarded_segmented with one more arena, `ema` (n fp32 elements):
 * wherever the launch writes a parameter p it also writes, from the p it holds in registers,
 *     e = fma(omd, p - e, e),   omd = (float)(1 - d_k)      (fp32; the difference and the fma round once each)
 * with d_k = decay, or with warmup != 0 d_k = min(decay, (1 + k) / (10 + k)), formed in double; k >= 1 numbers this averaging update.
 * Elements the launch does not write - in no segment, of a class whose own step is below 1, everything on a skipped step - keep
 * their average bit for bit.  p, exp_avg and exp_avg_sq come out bit-equal to the call without an average.  A whole arena is the
 * one-segment table [0, n) of class 0.
 * k_or_t0: plain call: the k of this update (the caller counts).  Guarded call: the applied-step count at which averaging began;
 * the kernel forms k = state->applied_steps - k_or_t0 (after this step's finalize) and omd itself, and writes no average while k < 1.
 * Both refuse, before any HIP call, what their counterparts refuse, and: a null `ema` struct, a null or misaligned (4 bytes)
 * ema->ema, an ema->ema whose n elements overlap params, grads, exp_avg or exp_avg_sq, a decay outside [0, 1) or NaN, and the
 * plain call k < 1. */
typedef struct dmm_adam_ema {
  float* ema;         /*  0: the average, n elements (device) */
  float decay;        /*  8 */
  int32_t warmup;     /* 12 */
  int64_t k_or_t0;    /* 16 */
} dmm_adam_ema;       /* 24 bytes */
int dmm_adam_step_segmented_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const void* table_dev,
                                int nsegs, const dmm_adam_class* classes, int nclasses, int64_t step, float grad_scale, void* stream,
                                const dmm_adam_ema* ema);
int dmm_adam_step_guarded_segmented_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                        const void* table_dev, int nsegs, const dmm_adam_class* classes, int nclasses, float max_norm,
                                        float growth_factor, float backoff_factor, int32_t growth_interval, dmm_guard_state* state,
                                        void* scratch, void* stream, const dmm_adam_ema* ema);
/* Points the plan's loss kernel and the external-gradient conversion of dmm_plan_backward at a device float (&state->scale):
 * d(loss)/d(logit) is multiplied by loss_scale * (*scale_dev), read on the device when the kernel runs.  NULL = off: the code path
 * and the numbers of a plan that never had one.  Loss sums, metric counts and the unreduced outputs stay unscaled.  Both kernels
 * are launched eagerly in FRONT of the replayed segment of the backward list (dmm_plan_num_graph_replays), so a captured graph
 * holds no copy of the pointer and replay is unaffected; the setting survives dmm_plan_bind. */
int dmm_plan_set_dynamic_loss_scale(dmm_plan* plan, const float* scale_dev);

/* ---- single-kernel entry points (unit tests) ---- */
typedef struct {
  int32_t dtype, use_mfma;
  int32_t B, H, W;         /* input spatial size */
  int32_t Cin, Cout;       /* real channels; Cin is a multiple of 8 */
  int32_t R, S, stride, pad;
  int32_t transposed;      /* 1: ConvTranspose2d(k=3, s=2, p=1, output_padding=1), weight (Cin, Cout, 3, 3) */
  int32_t mode;            /* 0 plain, 1 nearest-upsample x2 source, 2 avg-pool 2x2 then 1x1 */
  int32_t bn_relu;         /* apply relu(x*scale+shift) to the input first */
} dmm_conv_desc;

/* x: T NHWC (B,H,W,Cin); w: fp32 master weights; y: T NHWC output; stats: 2*Cout doubles (sum, sumsq; zeroed by the
 * callee) or NULL; scratch: >= dmm_conv_scratch_bytes. */
size_t dmm_conv_scratch_bytes(const dmm_conv_desc* d);
int dmm_conv_forward(const dmm_conv_desc* d, const void* x, const float* w, const float* scale, const float* shift, void* y,
                     double* stats, void* scratch, void* stream);
/* Test entry point, like the others of this section: where record `index` of a BOUND plan's training forward list (a storing convolution;
 * DMM_ERR_INVALID otherwise) leaves its result - byte offset into the workspace and dims = {B, H, W, N, pixel pitch in elements} of the
 * NHWC tensor in the storage type - so that a test can compare one layer's output between two plans.  (Every exported dmm_ symbol is
 * declared here: tests/test_accum_cpu.py.) */
int dmm_plan_record_output(const dmm_plan* plan, int index, int64_t* ws_offset, int32_t* dims);
/* The pooling pass in front of a transition's 1x1 convolution (torchvision _Transition: norm, relu, conv, AvgPool2d(2, 2), with the
 * pool moved in front of the linear conv) on its own: out[b, y, x, c] = 0.25 * sum of relu(x * scale[c] + shift[c]) over the 2x2 window,
 * summed in fp32 in raster order from 0 and rounded once to the storage type - what dmm_conv_forward with mode 2 feeds its matrix
 * core, bit for bit.  x: T NHWC with pixel pitch ld, pre-offset to a window of C channels; out: T (B, H/2, W/2) with pitch ldo,
 * pre-offset; bytes outside the window are not touched.  DMM_ERR_INVALID for odd H / W, C / ld / ldo that are not whole 16-byte slots,
 * pitches below C and null pointers. */
int dmm_avgpool2_bnrelu(int dtype, const void* x, int ld, int B, int H, int W, int C, const float* scale, const float* shift, void* out,
                        int ldo, void* stream);
/* The logits launch of the network's last convolution (dec_out_to_heat_maps.refine1; reference graphs/models/Dense_U_Net_lidar.py:128-131)
 * on its own: a plain convolution at stride 1 (optionally behind BN+ReLU) whose output is written UNROUNDED as fp32 NCHW
 * (B, Cout, Ho, Wo) - no statistics.  It dispatches as the plan's launch does: thin.hip (16-bit storage, 64 input channels, 1..3
 * classes), halo.hip (f16 / fp32 where the weights fit its LDS), else the generic kernel.  DMM_ERR_INVALID, before anything is
 * launched, for transposed / mode != 0 / stride != 1 descriptors, Cout > 32 and null pointers. */
int dmm_conv_logits(const dmm_conv_desc* d, const void* x, const float* w, const float* scale, const float* shift, float* logits,
                    void* scratch, void* stream);
/* dw: fp32, master layout, overwritten.  dy: T NHWC gradient of the conv output. */
int dmm_conv_wgrad(const dmm_conv_desc* d, const void* x, const void* dy, const float* scale, const float* shift, float* dw,
                   void* scratch, void* stream);
/* BN+ReLU-fused data gradient: gx (T, NHWC like x) = scale * relu'(x*scale+shift) * conv_dgrad(dy); red: 2*Cin doubles
 * (sum dz, sum dz*xhat with xhat = (x - mean)*invstd; zeroed by the callee).  `shift` points at 3*Cin floats:
 * shift, mean, invstd. */
int dmm_conv_dgrad(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale, const float* shift,
                   void* gx, double* red, void* scratch, void* stream);


/* The same two gradients as the plan's launches see them (autograd of torch.nn.functional.conv2d behind the reference's
 * BatchNorm2d + ReLU, graphs/models/Dense_U_Net_lidar.py:85-92 via torchvision _DenseLayer):
 *   - the incoming gradient may carry the deferred BatchNorm-backward correction of the layer behind it:
 *     dy_eff = dy + q[c] + r[c] * yfwd[.., c]  (yfwd: T NHWC forward output of this convolution; q, r: Cout floats; all NULL = none);
 *   - transposed_form != 0: the weight gradient with the taps on the gradient side, the form the plan uses for thin outputs
 *     (the dense layers' 3x3 growth convolution: wg3.hip in 16-bit storage);
 *   - accumulate != 0: gx += instead of gx =. */
int dmm_conv_wgrad_ex(const dmm_conv_desc* d, const void* x, const void* dy, const float* scale, const float* shift, const void* yfwd,
                      const float* q, const float* r, int transposed_form, float* dw, void* scratch, void* stream);
int dmm_conv_dgrad_ex(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale, const float* shift,
                      const void* yfwd, const float* q, const float* r, void* gx, int accumulate, double* red, void* scratch,
                      void* stream);
/* A decoder ConvTranspose stage (reference graphs/models/Dense_U_Net_lidar.py:155-160) as a PLAN launches it: the four output-parity
 * phases that dmm_conv_forward / dmm_conv_wgrad_ex launch one by one are each picked and then merged into ONE launch by the plan
 * builder's own functions (csrc/plan.h) - cvp.hip's cvp_multi_kernel or cvw.hip's four-phase walk for the forward, wgpw.hip's
 * wgpw_multi_kernel for the weight gradient - where those accept the merge; where they keep the phases apart (a phase on another
 * family, the deferred correction q / r on the gradient, operands of 4 GiB and more) the four launches run, each on the family picked
 * for it.  *launches: 1 or 4.  Arguments and results otherwise as dmm_conv_forward / dmm_conv_wgrad_ex (normal form).
 * DMM_ERR_INVALID, before the runtime is asked anything, for transposed == 0, a null pointer (stats may be NULL), and q, r, yfwd
 * not given together. */
int dmm_conv_forward_merged(const dmm_conv_desc* d, const void* x, const float* w, const float* scale, const float* shift, void* y,
                            double* stats, void* scratch, void* stream, int* launches);
int dmm_conv_wgrad_merged(const dmm_conv_desc* d, const void* x, const void* dy, const float* scale, const float* shift, const void* yfwd,
                          const float* q, const float* r, float* dw, void* scratch, void* stream, int* launches);
/* The head's last convolution (5x5, 64 channels onto <= 4 classes behind BatchNorm2d + ReLU; reference
 * graphs/models/Dense_U_Net_lidar.py:128-131), 16-bit storage: its weight gradient AND the BatchNorm-backward reductions of the norm
 * in front of it - red[0..64) = sum dz, red[64..128) = sum dz*xhat over all pixels, dz = relu'(x*scale+shift) * conv_dgrad(dy) with
 * the weights rounded to the storage type, as dmm_conv_dgrad reports them - from ONE pass over x and dy (wg5.hip, PA = 3: x enters as
 * the two factors of its activation; wg5_fin64_kernel).  w: fp32 master weights (Cout, 64, 5, 5); `shift` points at 3*64 floats:
 * shift, mean, invstd; dw: fp32, master layout, overwritten; red: 128 doubles, zeroed by the callee.  DMM_ERR_INVALID for any other
 * shape.  (Nothing upstream: autograd runs conv2d's and batch_norm's backward as separate ATen calls.) */
int dmm_conv5_wgrad_stats(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale, const float* shift,
                          float* dw, double* red, void* scratch, void* stream);
/* Data gradient AND weight gradient of a 1x1 bottleneck convolution in one pass (bw1.hip; 16-bit storage, Cout == 128,
 * Cin % 32 == 0; DMM_ERR_INVALID otherwise): the two results of dmm_conv_dgrad_ex and dmm_conv_wgrad_ex on the same operands. */
int dmm_conv1x1_backward_fused(const dmm_conv_desc* d, const void* x, const void* dy, const float* w, const float* scale,
                               const float* shift, const void* yfwd, const float* q, const float* r, void* gx, int accumulate,
                               float* dw, double* red, void* scratch, void* stream);

/* Test entry points of the grouped launches (wg3.hip, bw1.hip), as the executor issues them for consecutive layers of a dense block.
 * n dense 3x3 weight gradients in the transposed form (each as the same call with transposed_form != 0 of dmm_conv_wgrad_ex: 16-bit storage, 128 -> 32
 * channels, use_mfma; DMM_ERR_INVALID otherwise; descs, and every pointer array, have n entries; yfwd / q / r may be NULL or hold
 * NULLs) sharing one slot buffer: grouped != 0 = grouped launches of at most 32 members each, filled in order; 0 = one launch per
 * member.  *launches (nullable) = weight-gradient kernel launches made.  Members may differ in map size and batch, not in dtype or
 * in having q / r. */
int dmm_conv_wgrad_grouped(const dmm_conv_desc* descs, int n, const void* const* x, const void* const* dy, const float* const* scale,
                           const float* const* shift, const void* const* yfwd, const float* const* q, const float* const* r,
                           float* const* dw, void* const* scratch, int grouped, int* launches, void* stream);
/* n reductions of bw1.hip's weight-gradient slots: member i adds the nsplit[i] row ranges of part[i] (slot (k, ct) = 4 x 128 x 32
 * floats at (k * nct[i] + ct) slots) into dpack[i] (ceil(wc[i] / 32) x 128 x 32 floats, overwritten; (nct[i] - 1) * 128 < wc[i] <=
 * nct[i] * 128).  grouped != 0: one launch per 32 members; 0: one per member.  Both add in the same order: the results are equal
 * bit for bit.  *launches (nullable) = launches made. */
int dmm_bw1_reduce_grouped(int n, const float* const* part, float* const* dpack, const int* nct, const int* nsplit, const int* wc,
                           int grouped, int* launches, void* stream);

/* Which kernel family ran the calling thread's most recent single-kernel launch (dmm_conv_forward / _logits / _wgrad(_ex) / _dgrad(_ex) /
 * dmm_conv1x1_backward_fused / dmm_conv5_wgrad_stats; for multi-launch entry points: the last launch).  The single-kernel entry points dispatch like a
 * plan does and fall back to the generic implicit-GEMM kernels when no specialised family accepts the shape - silently, so a
 * per-kernel parity test asserts the family it names: dmm_impl_name(dmm_last_impl()) is one of
 * "generic", "thin", "conv3", "cvp", "halo", "wg3", "wg5", "wgp", "pig", "bw1"  ("auto": nothing launched yet).
 * (Nothing upstream: the reference has no kernel families; torch dispatches inside ATen.) */
int dmm_last_impl(void);
const char* dmm_impl_name(int impl);
/* Bit (1 << family) for every such launch of the calling thread since the mask was last reset (entry points that launch several
 * kernels - the parity phases of a ConvTranspose - leave more than one bit); reset != 0 clears it after reading. */
unsigned dmm_impl_mask(int reset);

#ifdef __cplusplus
}
#endif
#endif /* DMMFODS_HIP_H */
