"""ctypes binding of libdmmfods_hip.so.  There is no CPU fallback: if the library is missing or a call
fails, this raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DMM_LIB_PATH") or os.path.join(_HERE, "libdmmfods_hip.so")  # DMM_LIB_PATH: experiment builds

DMM_F32, DMM_F16, DMM_BF16 = 0, 1, 2
LOSS_BCE, LOSS_FOCAL = 0, 1
T_CONV, T_CONVT, T_BN_WEIGHT, T_BN_BIAS, T_BN_MEAN, T_BN_VAR, T_BN_TRACKED = range(7)
ERR_INVALID, ERR_SHAPE, ERR_HIP, ERR_STATE, ERR_NO_DEVICE = -1, -2, -3, -4, -5


class ModelDesc(C.Structure):
    _fields_ = [
        ("growth_rate", C.c_int32), ("num_blocks", C.c_int32), ("block_config", C.c_int32 * 8),
        ("num_init_features", C.c_int32), ("bn_size", C.c_int32), ("num_classes", C.c_int32),
        ("concat_before_block_num", C.c_int32), ("stream_1_in_channels", C.c_int32),
        ("stream_2_in_channels", C.c_int32), ("batch", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("dtype", C.c_int32), ("loss_scale", C.c_float), ("bn_momentum", C.c_float), ("bn_eps", C.c_float),
        ("iou_threshold", C.c_float), ("use_mfma", C.c_int32),
    ]


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "dtype", "use_mfma", "B", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad", "transposed", "mode", "bn_relu")]


class GuardState(C.Structure):
    """dmm_guard_state (include/dmmfods_hip.h): the 64-byte device block of the guarded optimiser step."""
    _fields_ = [("scale", C.c_float), ("grad_scale", C.c_float), ("sumsq", C.c_double), ("grad_norm", C.c_float),
                ("found_inf", C.c_int32), ("applied_steps", C.c_int64), ("skipped_steps", C.c_int64),
                ("growth_tracker", C.c_int32), ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("clip_coef", C.c_float),
                ("reserved", C.c_int32 * 2)]


assert C.sizeof(GuardState) == 64

ADAM_MAX_CLASSES = 16   # DMM_ADAM_MAX_CLASSES


class AdamSegment(C.Structure):
    """dmm_adam_segment: elements [begin, begin + count) of the arenas belong to class `cls`."""
    _fields_ = [("begin", C.c_int64), ("count", C.c_int64), ("cls", C.c_int32)]


class AdamClass(C.Structure):
    """dmm_adam_class: the hyper-parameters of a (parameter group, step origin) pair."""
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("decoupled", C.c_int32), ("t0", C.c_int64)]


class AdamEma(C.Structure):
    """dmm_adam_ema: the parameter average of the two `_ema` step calls; k_or_t0 is the update's k (plain) or the applied-step count
    at which averaging began (guarded)."""
    _fields_ = [("ema", C.c_void_p), ("decay", C.c_float), ("warmup", C.c_int32), ("k_or_t0", C.c_int64)]


assert C.sizeof(AdamSegment) == 24 and C.sizeof(AdamClass) == 32 and C.sizeof(AdamEma) == 24


AUG_MAX_TENSORS, AUG_MAX_CHANNELS, AUG_LAUNCH_BATCH = 4, 8, 32   # DMM_AUG_MAX_TENSORS, DMM_AUG_MAX_CHANNELS, DMM_AUG_LAUNCH_BATCH


class AugTensor(C.Structure):
    """dmm_aug_tensor: one tensor of a dmm_augment_batch call; src_batch_stride in elements."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_batch_stride", C.c_int64), ("channels", C.c_int32),
                ("reserved", C.c_int32)]


class AugSample(C.Structure):
    """dmm_aug_sample: one sample's window, mirror flag and per-channel gain / bias (channels numbered through the call's tensors)."""
    _fields_ = [("y0", C.c_int32), ("x0", C.c_int32), ("flip", C.c_int32), ("reserved", C.c_int32),
                ("gain", C.c_float * AUG_MAX_CHANNELS), ("bias", C.c_float * AUG_MAX_CHANNELS)]


assert C.sizeof(AugTensor) == 32 and C.sizeof(AugSample) == 80

# DMM_WARP_NEAREST, DMM_WARP_BILINEAR, DMM_WARP_FRAC_BITS, DMM_WARP_LAUNCH_BATCH, DMM_WARP_MAX_A, DMM_WARP_MAX_B
WARP_NEAREST, WARP_BILINEAR, WARP_FRAC_BITS, WARP_LAUNCH_BATCH, WARP_MAX_A, WARP_MAX_B = 0, 1, 20, 32, 64 << 20, 1 << 50


class WarpTensor(C.Structure):
    """dmm_warp_tensor: one tensor of a dmm_warp_batch call; as AugTensor, with the way it is sampled."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_batch_stride", C.c_int64), ("channels", C.c_int32), ("mode", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class WarpSample(C.Structure):
    """dmm_warp_sample: one sample's affine map (x, y) -> (a00 x + a01 y + b0, a10 x + a11 y + b1) in Q20 and per-channel gain / bias."""
    _fields_ = [("a00", C.c_int32), ("a01", C.c_int32), ("a10", C.c_int32), ("a11", C.c_int32), ("b0", C.c_int64), ("b1", C.c_int64),
                ("gain", C.c_float * AUG_MAX_CHANNELS), ("bias", C.c_float * AUG_MAX_CHANNELS)]


assert C.sizeof(WarpTensor) == 40 and C.sizeof(WarpSample) == 96

CC_TILE_H, CC_TILE_W, CC_MAX_PER_PLANE = 32, 32, 65536   # DMM_CC_TILE_H, DMM_CC_TILE_W, DMM_CC_MAX_PER_PLANE


class Component(C.Structure):
    """dmm_component: one connected component of a thresholded heat map."""
    _fields_ = [("root", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("area", C.c_int32), ("score", C.c_float), ("peak", C.c_int32)]


assert C.sizeof(Component) == 32

MATCH_MAX_PER_PLANE = 4096   # DMM_MATCH_MAX_PER_PLANE

PREP_LAUNCH_BATCH, PREP_MAX_ITEMS = 32, 1 << 23   # DMM_PREP_LAUNCH_BATCH, DMM_PREP_MAX_ITEMS


class PrepBox(C.Structure):
    """dmm_prep_box: one labelled box of a dmm_prep_heat_maps call; top-left corner, full-resolution pixels."""
    _fields_ = [("type", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


assert C.sizeof(PrepBox) == 20


class DmmError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C dmmfods_amd/csrc`).  dmmfods_amd has no CPU fallback.")
    # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so).  Device pointers and streams are only
    # meaningful inside ONE runtime, so make sure torch's copy is the one already loaded when our library's
    # NEEDED libamdhip64.so.7 is resolved (same SONAME -> the loader reuses it).
    import torch  # noqa: F401
    tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tl):
        C.CDLL(tl, mode=C.RTLD_GLOBAL)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    L.dmm_last_error.restype = C.c_char_p
    L.dmm_version.restype = C.c_int
    L.dmm_last_impl.restype = C.c_int
    L.dmm_impl_name.restype = C.c_char_p
    L.dmm_impl_name.argtypes = [C.c_int]
    L.dmm_impl_mask.restype = C.c_uint
    L.dmm_impl_mask.argtypes = [C.c_int]
    L.dmm_set_option.restype = C.c_int
    L.dmm_set_option.argtypes = [C.c_char_p, C.c_int]
    L.dmm_plan_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(vp)]
    L.dmm_plan_destroy.argtypes = [vp]
    L.dmm_plan_destroy.restype = C.c_int
    L.dmm_plan_num_tensors.argtypes = [vp]
    L.dmm_plan_tensor_info.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(i32), C.POINTER(i32),
                                       C.POINTER(i64 * 4), C.POINTER(i64)]
    L.dmm_plan_num_params.argtypes = [vp]
    L.dmm_plan_num_params.restype = i64
    L.dmm_plan_num_buffer_elems.argtypes = [vp]
    L.dmm_plan_num_buffer_elems.restype = i64
    L.dmm_plan_workspace_bytes.argtypes = [vp]
    L.dmm_plan_workspace_bytes.restype = sz
    L.dmm_plan_forward_flops.argtypes = [vp]
    L.dmm_plan_forward_flops.restype = C.c_double
    L.dmm_plan_bind.argtypes = [vp, vp, sz, vp, vp, vp]
    L.dmm_plan_forward.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    L.dmm_plan_loss_backward.argtypes = [vp, vp, vp, vp, vp]
    L.dmm_plan_backward.argtypes = [vp, vp, vp]
    L.dmm_plan_loss_metrics.argtypes = [vp, vp, vp, vp, vp]
    L.dmm_plan_set_loss.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    L.dmm_loss_forward.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.dmm_logit_hist_elems.argtypes = [C.c_int, C.c_int, C.c_int]
    L.dmm_logit_hist_elems.restype = sz
    L.dmm_logit_hist.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, f32, C.c_int, vp, vp]
    L.dmm_augment_batch.argtypes = [C.POINTER(AugTensor), C.c_int, C.POINTER(AugSample), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.POINTER(C.c_float), vp]
    L.dmm_warp_batch.argtypes = [C.POINTER(WarpTensor), C.c_int, C.POINTER(WarpSample), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_float), vp]
    L.dmm_heat_components_workspace.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dmm_heat_components_workspace.restype = sz
    L.dmm_heat_components.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, C.c_int, C.c_int, vp, sz, vp, vp, vp, vp]
    L.dmm_match_objects_workspace.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.dmm_match_objects_workspace.restype = sz
    L.dmm_match_objects.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, sz, vp, vp, vp, i64, vp]
    L.dmm_prep_image.argtypes = [vp, i64, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.dmm_prep_lidar_workspace.argtypes = [C.c_int, C.c_int, C.c_int]
    L.dmm_prep_lidar_workspace.restype = sz
    L.dmm_prep_lidar.argtypes = [vp, C.POINTER(i32), vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, vp]
    L.dmm_prep_heat_maps.argtypes = [vp, C.POINTER(i32), vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.dmm_plan_num_grad_buckets.argtypes = [vp]
    L.dmm_plan_num_graph_replays.argtypes = [vp, C.c_int]
    L.dmm_plan_num_graph_replays.restype = C.c_longlong
    L.dmm_plan_grad_bucket.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.dmm_plan_grad_bucket_wait.argtypes = [vp, C.c_int, vp]
    L.dmm_plan_profile_begin.argtypes = [vp, C.c_int]
    L.dmm_plan_profile_filter.restype = C.c_int
    L.dmm_plan_profile_filter.argtypes = [vp, C.c_char_p]
    L.dmm_plan_profile_num_ops.argtypes = [vp, C.c_int]
    L.dmm_plan_profile_op.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.dmm_plan_profile_collect.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.dmm_adam_step.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i64, f32, vp]
    L.dmm_grad_guard_scratch_bytes.argtypes = [i64]
    L.dmm_grad_guard_scratch_bytes.restype = sz
    L.dmm_guard_state_init.argtypes = [vp, f32, i64, i32, vp]
    L.dmm_adam_step_guarded.argtypes = [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, f32, f32, i32, vp, vp, vp]
    L.dmm_plan_set_encoder_frozen.argtypes = [vp, C.c_int]
    L.dmm_adam_table_bytes.argtypes = [C.c_int, i64]
    L.dmm_adam_table_bytes.restype = sz
    L.dmm_adam_table_init.argtypes = [vp, C.POINTER(AdamSegment), C.c_int, i64, C.c_int, vp]
    L.dmm_adam_step_segmented.argtypes = [vp, vp, vp, vp, i64, vp, C.c_int, C.POINTER(AdamClass), C.c_int, i64, f32, vp]
    L.dmm_adam_step_guarded_segmented.argtypes = [vp, vp, vp, vp, i64, vp, C.c_int, C.POINTER(AdamClass), C.c_int, f32, f32, f32, i32,
                                                  vp, vp, vp]
    L.dmm_adam_step_segmented_ema.argtypes = L.dmm_adam_step_segmented.argtypes + [C.POINTER(AdamEma)]
    L.dmm_adam_step_guarded_segmented_ema.argtypes = L.dmm_adam_step_guarded_segmented.argtypes + [C.POINTER(AdamEma)]
    L.dmm_grad_sumsq.argtypes = [vp, i64, i64, C.c_int, vp, vp]
    L.dmm_plan_set_dynamic_loss_scale.argtypes = [vp, vp]
    L.dmm_plan_set_grad_accumulate.argtypes = [vp, C.c_int]
    L.dmm_conv_scratch_bytes.argtypes = [C.POINTER(ConvDesc)]
    L.dmm_conv_scratch_bytes.restype = sz
    L.dmm_conv_forward.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp]
    L.dmm_conv_logits.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp]
    L.dmm_plan_record_output.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i32 * 5)]
    L.dmm_avgpool2_bnrelu.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
    L.dmm_conv_forward_merged.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.dmm_conv_wgrad_merged.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.dmm_conv_wgrad.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp]
    L.dmm_conv_dgrad.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dmm_conv_wgrad_ex.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.dmm_conv_dgrad_ex.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    L.dmm_conv1x1_backward_fused.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.dmm_conv5_wgrad_stats.argtypes = [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dmm_plan_wgrad_batch_counts.argtypes = [vp, C.POINTER(C.c_longlong * 4)]
    L.dmm_conv_wgrad_grouped.argtypes = [C.POINTER(ConvDesc), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int), vp]
    L.dmm_bw1_reduce_grouped.argtypes = [C.c_int, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                         C.POINTER(C.c_int), vp]
    _lib = L
    return L


EXPORTS = [
    "dmm_last_error", "dmm_version", "dmm_set_option", "dmm_plan_create", "dmm_plan_destroy", "dmm_plan_num_tensors",
    "dmm_plan_tensor_info", "dmm_plan_num_params", "dmm_plan_num_buffer_elems", "dmm_plan_workspace_bytes",
    "dmm_plan_forward_flops", "dmm_plan_bind", "dmm_plan_forward", "dmm_plan_loss_backward", "dmm_plan_backward",
    "dmm_plan_loss_metrics", "dmm_plan_num_graph_replays", "dmm_plan_set_loss", "dmm_loss_forward", "dmm_plan_num_grad_buckets", "dmm_plan_grad_bucket",
    "dmm_plan_grad_bucket_wait", "dmm_plan_profile_begin", "dmm_plan_profile_filter", "dmm_plan_profile_num_ops", "dmm_plan_profile_op",
    "dmm_plan_profile_collect", "dmm_adam_step", "dmm_conv_scratch_bytes", "dmm_conv_forward", "dmm_conv_logits", "dmm_conv_forward_merged", "dmm_conv_wgrad_merged", "dmm_conv_wgrad",
    "dmm_conv_dgrad", "dmm_conv_wgrad_ex", "dmm_conv_dgrad_ex", "dmm_conv1x1_backward_fused", "dmm_conv5_wgrad_stats", "dmm_last_impl", "dmm_impl_name", "dmm_impl_mask",
    "dmm_grad_guard_scratch_bytes", "dmm_guard_state_init", "dmm_adam_step_guarded", "dmm_grad_sumsq", "dmm_plan_set_dynamic_loss_scale",
    "dmm_plan_set_grad_accumulate", "dmm_plan_set_encoder_frozen",
    "dmm_adam_table_bytes", "dmm_adam_table_init", "dmm_adam_step_segmented", "dmm_adam_step_guarded_segmented",
    "dmm_adam_step_segmented_ema", "dmm_adam_step_guarded_segmented_ema",
    "dmm_plan_wgrad_batch_counts", "dmm_conv_wgrad_grouped", "dmm_bw1_reduce_grouped",
    "dmm_logit_hist_elems", "dmm_logit_hist", "dmm_augment_batch", "dmm_warp_batch",
    "dmm_heat_components_workspace", "dmm_heat_components", "dmm_match_objects_workspace", "dmm_match_objects",
    "dmm_prep_image", "dmm_prep_lidar_workspace", "dmm_prep_lidar", "dmm_prep_heat_maps",
    "dmm_avgpool2_bnrelu", "dmm_plan_record_output",
]
HIST_MAX_THRESHOLDS = 255   # DMM_HIST_MAX_THRESHOLDS


def check(rc):
    """Map a dmm_status to the exception type the reference raises for the same condition."""
    if rc == 0:
        return
    msg = lib().dmm_last_error().decode(errors="replace")
    if rc == ERR_SHAPE:
        raise ValueError(msg)          # reference: ValueError from ConvTranspose2d(output_size=...) (M:261)
    if rc == ERR_INVALID and "fusion" in msg:
        raise AttributeError(msg)      # reference: AttributeError for a bad fusion configuration (M:65)
    if rc == ERR_INVALID:
        raise ValueError(msg)
    raise DmmError(f"dmm status {rc}: {msg}")


def last_impl():
    """Name of the kernel family that ran this thread's most recent single-kernel launch ("wg3", "conv3", "generic", ...)."""
    L = lib()
    return L.dmm_impl_name(L.dmm_last_impl()).decode()


def impls_since_reset(reset=True):
    """Names of the kernel families that ran this thread's single-kernel launches since the last reset."""
    L = lib()
    m = L.dmm_impl_mask(1 if reset else 0)
    return {L.dmm_impl_name(i).decode() for i in range(32) if (m >> i) & 1}


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
