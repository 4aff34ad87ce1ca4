"""ctypes binding of libn3dt.so (C ABI: include/n3dt.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing
this module's `lib()` raises.  Build it with `make -C nerf-3dtalker-code_amd` (or
`python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("N3DT_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libn3dt.so")

F32, BF16, F16, BF16X3 = 0, 1, 2, 3
PRECISIONS = {"fp32": F32, "f32": F32, "bf16": BF16, "fp16": F16, "f16": F16, "bf16x3": BF16X3}
MLP_LAYERS = 12
MAX_BLOCKS = 8

MLP_ORDER = ["FeaExt_module_%d" % i for i in range(8)] + ["density_module", "RGB_layer_0", "RGB_layer_1", "RGB_layer_2"]


class Geom(ctypes.Structure):
    _fields_ = [
        ("batch", ctypes.c_int32), ("n_rays", ctypes.c_int32), ("n_samples", ctypes.c_int32),
        ("hidden", ctypes.c_int32), ("feat_nc", ctypes.c_int32), ("shape_dim", ctypes.c_int32),
        ("appea_dim", ctypes.c_int32), ("audio_dim", ctypes.c_int32), ("featmap_size", ctypes.c_int32),
        ("n_blocks", ctypes.c_int32), ("world_z1", ctypes.c_float), ("world_z2", ctypes.c_float),
        ("xy_stride_b", ctypes.c_int64), ("xy_stride_c", ctypes.c_int64), ("xy_stride_r", ctypes.c_int64),
        ("z_planes_given", ctypes.c_int32), ("bg_is_hwc", ctypes.c_int32), ("vd_dim", ctypes.c_int32),
    ]


VGG_CONVS = 10


class VggParams(ctypes.Structure):
    _fields_ = [("weight", ctypes.c_void_p * VGG_CONVS), ("bias", ctypes.c_void_p * VGG_CONVS)]


LPIPS_LAYERS = 5
LPIPS_INPUT_MODES = {"reference": 0, "standard": 1}


class LpipsParams(ctypes.Structure):
    _fields_ = [("weight", ctypes.c_void_p * LPIPS_LAYERS), ("bias", ctypes.c_void_p * LPIPS_LAYERS), ("lin", ctypes.c_void_p * LPIPS_LAYERS)]


SYNCNET_BLOCKS = 31


class SyncnetParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p * SYNCNET_BLOCKS) for name in ("weight", "bias", "bn_weight", "bn_bias", "bn_mean", "bn_var")]


WAV2LIP_BLOCKS = 51


class Wav2lipParams(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p * WAV2LIP_BLOCKS) for name in ("weight", "bias", "bn_weight", "bn_bias", "bn_mean", "bn_var")]


S3FD_PARAMS = 31
S3FD_BLOCKS = 33


class S3fdParams(ctypes.Structure):
    _fields_ = [("weight", ctypes.c_void_p * S3FD_PARAMS), ("bias", ctypes.c_void_p * S3FD_PARAMS), ("norm_weight", ctypes.c_void_p * 3)]


FACE_RECON_CONVS = 53
FACE_RECON_HEADS = 7
FACE_RECON_BLOCKS = 56
FACE_RECON_COEFFS = 257


class FaceReconParams(ctypes.Structure):
    _fields_ = ([(name, ctypes.c_void_p * FACE_RECON_CONVS) for name in ("weight", "bn_weight", "bn_bias", "bn_mean", "bn_var")] +
                [("bn_eps", ctypes.c_double * FACE_RECON_CONVS), ("head_weight", ctypes.c_void_p * FACE_RECON_HEADS),
                 ("head_bias", ctypes.c_void_p * FACE_RECON_HEADS)])


FAN_MAX_CONVS = 200
FAN_MAX_BLOCKS = 82


class FanParams(ctypes.Structure):
    _fields_ = ([("num_modules", ctypes.c_int32), ("num_landmarks", ctypes.c_int32)] +
                [(name, ctypes.c_void_p * FAN_MAX_CONVS) for name in ("weight", "bias", "bn_weight", "bn_bias", "bn_mean", "bn_var")] +
                [("coords256", ctypes.c_void_p), ("coords64", ctypes.c_void_p)])


HEAD_MASK_CONVS = 36
HEAD_MASK_BLOCKS = 37
HEAD_MASK_MAX_CLASSES = 32


class HeadMaskParams(ctypes.Structure):
    _fields_ = ([("n_classes", ctypes.c_int32), ("reserved", ctypes.c_int32)] +
                [(name, ctypes.c_void_p * HEAD_MASK_CONVS) for name in ("weight", "bn_weight", "bn_bias", "bn_mean", "bn_var")] +
                [("bn_eps", ctypes.c_double)])


class A2sParams(ctypes.Structure):
    _fields_ = [("w_ih", ctypes.c_void_p * 4), ("w_hh", ctypes.c_void_p * 4), ("b_ih", ctypes.c_void_p * 4), ("b_hh", ctypes.c_void_p * 4),
                ("lin_w", ctypes.c_void_p * 3), ("lin_b", ctypes.c_void_p * 3)]


class AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_int64), ("group", ctypes.c_int32), ("active", ctypes.c_int32)]


class AdamChunk(ctypes.Structure):
    _fields_ = [("start", ctypes.c_int64), ("tensor", ctypes.c_int32), ("length", ctypes.c_int32)]


class AdamGroup(ctypes.Structure):
    _fields_ = [("lr", ctypes.c_double), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("maximize", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AdamGuard(ctypes.Structure):
    """N3dtAdamGuard (include/n3dt_flat_adam_guard.h).  The host writes the first GUARD_HOST_BYTES only."""
    _fields_ = [("max_grad_norm", ctypes.c_float), ("skip_nonfinite", ctypes.c_int32), ("grad_norm", ctypes.c_float),
                ("clip_coef", ctypes.c_float), ("skip", ctypes.c_int32), ("skipped_steps", ctypes.c_int32),
                ("norm_done", ctypes.c_int32), ("reserved", ctypes.c_int32)]


GUARD_HOST_BYTES = 8
ADAM_MAX_GROUPS = 64
ADAM_COUNTER_INTS = 4

A2S_MAX_T = 256
A2S_GRAD_FLOATS = 20726784


class MlpParams(ctypes.Structure):
    _fields_ = [("weight", ctypes.c_void_p * MLP_LAYERS), ("bias", ctypes.c_void_p * MLP_LAYERS)]


class RenderParams(ctypes.Structure):
    _fields_ = [
        ("to_rgb_w", ctypes.c_void_p * (MAX_BLOCKS + 1)), ("to_rgb_b", ctypes.c_void_p * (MAX_BLOCKS + 1)),
        ("psu1_w", ctypes.c_void_p * MAX_BLOCKS), ("psu1_b", ctypes.c_void_p * MAX_BLOCKS),
        ("psu2_w", ctypes.c_void_p * MAX_BLOCKS), ("psu2_b", ctypes.c_void_p * MAX_BLOCKS),
        ("feat_w", ctypes.c_void_p * MAX_BLOCKS), ("feat_b", ctypes.c_void_p * MAX_BLOCKS),
    ]


STAGE_MAX = 12


class Stage(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p * STAGE_MAX), ("dst", ctypes.c_void_p * STAGE_MAX), ("count", ctypes.c_int64 * STAGE_MAX),
                ("view_dims", ctypes.c_int64 * 3), ("view_strides", ctypes.c_int64 * 3), ("n", ctypes.c_int32)]


def _signatures():
    """name -> (restype, [argtypes]) of every entry point of include/n3dt.h and include/n3dt_flat_adam_guard.h: the one place
    this package types the C ABI.  A new entry point is one row here (tests/test_host_cpu.py holds every row to the headers'
    prototypes, argument by argument, so a count such as [vp] * 15 cannot drift)."""
    vp, sz, ci, i64, f32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    gp, mp, rp = ctypes.POINTER(Geom), ctypes.POINTER(MlpParams), ctypes.POINTER(RenderParams)
    a2p = ctypes.POINTER(A2sParams)
    return {
        "n3dt_abi_version": (ci, []),
        "n3dt_last_error": (ctypes.c_char_p, []),
        "n3dt_mlp_packed_bytes": (sz, [gp, ci]),
        "n3dt_mlp_pack": (ci, [gp, ci, mp, vp, vp]),
        "n3dt_render_workspace_bytes": (sz, [gp, ci]),
        "n3dt_render_fwd": (ci, [gp, ci, vp, mp] + [vp] * 15 + [vp, sz, vp]),
        "n3dt_neural_render_workspace_bytes": (sz, [gp, ci]),
        "n3dt_neural_render_fwd": (ci, [gp, ci, ci, rp, vp, vp, vp, sz, vp]),
        "n3dt_chw_to_hwc": (ci, [ci, ci, vp, vp, vp]),
        "n3dt_prof_enable": (ci, [ci]),
        "n3dt_prof_collect": (ci, [ctypes.POINTER(f32), ci, ctypes.POINTER(ci)]),
        "n3dt_render_train_saved_bytes": (sz, [gp]),
        "n3dt_render_train_workspace_bytes": (sz, [gp]),
        "n3dt_render_train_fwd": (ci, [gp, ci, vp, mp] + [vp] * 14 + [vp, sz, vp, sz, vp]),
        "n3dt_render_bwd": (ci, [gp, ci, mp, mp] + [vp] * 7 + [vp, sz] + [vp] * 12 + [vp, sz, vp]),
        # n3dt_render_bwd + d_Kinv, d_xy behind d_T
        "n3dt_render_bwd_cam": (ci, [gp, ci, mp, mp] + [vp] * 7 + [vp, sz] + [vp] * 14 + [vp, sz, vp]),
        "n3dt_neural_render_train_saved_bytes": (sz, [gp, ci]),
        "n3dt_neural_render_train_workspace_bytes": (sz, [gp, ci]),
        "n3dt_neural_render_train_fwd": (ci, [gp, ci, ci, rp, vp, vp, vp, sz, vp, sz, vp]),
        "n3dt_neural_render_bwd": (ci, [gp, ci, ci, rp, rp, vp, vp, vp, sz, vp, vp, sz, vp]),
        "n3dt_loss_fwd": (ci, [ci, ci, vp, vp, vp, vp, f32, vp, vp, vp]),
        "n3dt_loss_bwd": (ci, [ci, ci, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp]),
        "n3dt_fine_sample": (ci, [gp, ci, vp, vp, vp, vp, vp, vp]),
        "n3dt_img_to_uint8": (ci, [ci, ci, vp, vp, vp]),
        "n3dt_sample_points": (ci, [gp] + [vp] * 10 + [vp]),
        "n3dt_embed": (ci, [ci, sz, vp, vp, vp]),
        "n3dt_mlp_points_workspace_bytes": (sz, [gp, sz]),
        "n3dt_mlp_points": (ci, [gp, sz, mp] + [vp] * 5 + [vp, sz, vp]),
        "n3dt_composite": (ci, [ci, ci, ci, ci] + [vp] * 8 + [vp]),
        "n3dt_ray_vd_bias": (ci, [gp, vp, i64, vp, vp, vp, vp, vp]),
        "n3dt_embed_freqs": (ci, [ci, sz, ci, vp, vp, vp]),
        "n3dt_neural_render_pack": (ci, [gp, ci, ci, rp, vp, sz, vp]),
        "n3dt_neural_render_fwd_reuse": (ci, [gp, ci, ci, rp, vp, vp, vp, sz, vp]),
        "n3dt_stage_inputs": (ci, [ctypes.POINTER(Stage), vp]),
        "n3dt_graph_begin": (ci, [vp]),
        "n3dt_graph_end": (ci, [vp, ctypes.POINTER(vp)]),
        "n3dt_graph_launch": (ci, [vp, vp]),
        "n3dt_graph_destroy": (ci, [vp]),
        "n3dt_vgg_packed_bytes": (sz, [ci]),
        "n3dt_vgg_pack": (ci, [ci, ctypes.POINTER(VggParams), vp, vp]),
        "n3dt_vgg_saved_bytes": (sz, [ci, ci]),
        "n3dt_vgg_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_vgg_loss_fwd": (ci, [ci, ci, ci, vp, vp, vp, vp, f32, vp, vp, sz, vp, sz, vp]),
        "n3dt_vgg_loss_bwd": (ci, [ci, ci, ci, vp, vp, vp, vp, sz, vp, vp, sz, vp]),
        "n3dt_vgg_conv_stage": (ci, [ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp]),
        "n3dt_a2s_saved_bytes": (sz, [ci]),
        "n3dt_a2s_workspace_bytes": (sz, [ci]),
        "n3dt_a2s_fwd": (ci, [ci, a2p, vp, vp, vp, vp, vp, vp, sz, vp, sz, vp]),
        "n3dt_a2s_bwd": (ci, [ci, a2p, vp, vp, sz, vp, vp, sz, vp]),
        "n3dt_flat_adam_record_bytes": (sz, [ci]),
        "n3dt_flat_adam_step": (ci, [vp, vp, ci, vp, ci, vp, vp]),
        "n3dt_render_fwd16": (ci, [gp, ci, vp, mp] + [vp] * 19 + [vp, sz, vp]),
        "n3dt_neural_render_fwd16_reuse": (ci, [gp, ci, ci, rp, vp, vp, vp, vp, sz, vp]),
        "n3dt_feat_to_rgb0": (ci, [ci, ci, vp, vp, vp, vp, vp]),
        "n3dt_x16_pack_probe": (ci, [ci, ci, sz, vp, vp, vp]),
        "n3dt_x16_pe_probe": (ci, [ci, ci, sz, vp, vp, vp]),
        "n3dt_eval_metrics_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_eval_metrics": (ci, [ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_lpips_packed_bytes": (sz, []),
        "n3dt_lpips_pack": (ci, [ctypes.POINTER(LpipsParams), vp, vp]),
        "n3dt_lpips_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_lpips": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_mel_workspace_bytes": (sz, []),
        "n3dt_mel_spectrogram": (ci, [i64, vp, i64, vp, i64, i64, ci, vp, vp, vp, i64, ci, vp, sz, vp]),
        "n3dt_mel_windows": (ci, [i64, vp, i64, ci, ci, vp, vp, vp]),
        "n3dt_syncnet_packed_bytes": (sz, []),
        "n3dt_syncnet_pack": (ci, [ctypes.POINTER(SyncnetParams), vp, vp]),
        "n3dt_syncnet_workspace_bytes": (sz, [ci]),
        "n3dt_syncnet_face_windows": (ci, [ci, ci, ci, vp, vp, ci, vp, vp]),
        "n3dt_syncnet_fwd": (ci, [ci, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
        "n3dt_syncnet_block": (ci, [ci, ci, vp, vp, vp, vp, sz, vp]),
        "n3dt_wav2lip_packed_bytes": (sz, []),
        "n3dt_wav2lip_pack": (ci, [ctypes.POINTER(Wav2lipParams), vp, vp]),
        "n3dt_wav2lip_workspace_bytes": (sz, [ci]),
        "n3dt_wav2lip_fwd": (ci, [ci, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_wav2lip_block": (ci, [ci, ci, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_wav2lip_face_inputs": (ci, [ci, ci, ci, vp, vp, vp, ci, vp, vp]),
        "n3dt_wav2lip_paste": (ci, [ci, ci, ci, vp, vp, vp, ci, vp, vp]),
        "n3dt_s3fd_packed_bytes": (sz, []),
        "n3dt_s3fd_pack": (ci, [ctypes.POINTER(S3fdParams), vp, vp]),
        "n3dt_s3fd_max_images": (ci, [ci, ci]),
        "n3dt_s3fd_positions": (ci, [ci, ci]),
        "n3dt_s3fd_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_s3fd_heads": (ci, [ci, ci, ci, vp, vp, ctypes.POINTER(vp), vp, sz, vp]),
        "n3dt_s3fd_detect": (ci, [ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_s3fd_boxes": (ci, [ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]),
        "n3dt_s3fd_block_workspace_bytes": (sz, [ci, ci, ci, ci]),
        "n3dt_s3fd_block": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
        "n3dt_face_recon_packed_bytes": (sz, []),
        "n3dt_face_recon_pack": (ci, [ctypes.POINTER(FaceReconParams), vp, vp]),
        "n3dt_face_recon_max_images": (ci, [ci, ci]),
        "n3dt_face_recon_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_face_recon_fwd": (ci, [ci, ci, ci, vp, vp, vp, vp, sz, vp]),
        "n3dt_face_recon_block_workspace_bytes": (sz, [ci, ci, ci, ci]),
        "n3dt_face_recon_block": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_face_recon_align": (ci, [ci, ci, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp]),
        "n3dt_fan_packed_bytes": (sz, [ci, ci]),
        "n3dt_fan_pack": (ci, [ctypes.POINTER(FanParams), vp, vp]),
        "n3dt_fan_max_images": (ci, [ci, ci]),
        "n3dt_fan_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_fan_fwd": (ci, [ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, sz, vp]),
        "n3dt_fan_block_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci]),
        "n3dt_fan_block": (ci, [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_fan_crops": (ci, [ci, ci, ci, vp, vp, vp, vp]),
        "n3dt_fan_points": (ci, [ci, ci, vp, i64, vp, vp, vp]),
        "n3dt_fan_tail": (ci, [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp]),
        "n3dt_head_mask_packed_bytes": (sz, []),
        "n3dt_head_mask_pack": (ci, [ctypes.POINTER(HeadMaskParams), vp, vp]),
        "n3dt_head_mask_max_images": (ci, [ci, ci]),
        "n3dt_head_mask_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_head_mask_fwd": (ci, [ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, sz, vp]),
        "n3dt_head_mask_block_workspace_bytes": (sz, [ci, ci, ci, ci, ci, ci]),
        "n3dt_head_mask_block": (ci, [ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "n3dt_head_mask_frames": (ci, [ci, ci, ci, vp, ci, vp, vp, vp]),
        "n3dt_head_mask_resize": (ci, [ci, ci, ci, ci, vp, ci, ci, vp, vp]),
        "n3dt_head_mask_labels": (ci, [ci, ci, ci, ci, ci, ci, vp, vp, vp]),
        "n3dt_head_mask_green": (ci, [ci, ci, ci, vp, ci, ci, vp, vp]),
        "n3dt_head_mask_postprocess_workspace_bytes": (sz, [ci, ci, ci]),
        "n3dt_head_mask_postprocess": (ci, [ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, sz, vp]),
        # the entry points include/n3dt_flat_adam_guard.h declares (n3dt.h includes that file)
        "n3dt_flat_adam_guard_bytes": (sz, []),
        "n3dt_flat_adam_guarded_step": (ci, [vp, vp, ci, vp, ci, vp, vp, vp, vp]),
    }


SIGNATURES = _signatures()
GUARD_EXPORTS = [name for name in SIGNATURES if name.startswith("n3dt_flat_adam_guard")]
EXPORTS = [name for name in SIGNATURES if name not in GUARD_EXPORTS]


_LIB = None


class N3dtError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise N3dtError("libn3dt.so not found at %s -- the HIP extension is required (no CPU fallback); "
                        "run `make -C nerf-3dtalker-code_amd`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.n3dt_abi_version() != 5:
        raise N3dtError("libn3dt.so ABI version mismatch")
    if L.n3dt_flat_adam_guard_bytes() != ctypes.sizeof(AdamGuard):
        raise N3dtError("libn3dt.so: N3dtAdamGuard differs from its ctypes mirror")
    for which, rec in enumerate((AdamTensor, AdamChunk, AdamGroup)):
        if L.n3dt_flat_adam_record_bytes(which) != ctypes.sizeof(rec):
            raise N3dtError("libn3dt.so: FlatAdam table record %d differs from its ctypes mirror" % which)
    _LIB = L
    return L


PROF_ACTIVE = False


def prof_enable(max_records):
    """The measurement hook of bench.py (n3dt_prof_enable).  While it is active forward() does not replay hipGraphs:
    the hook's events are recorded by the launching call, which a replay never executes."""
    global PROF_ACTIVE
    check(lib().n3dt_prof_enable(int(max_records)), "n3dt_prof_enable")
    PROF_ACTIVE = max_records > 0


def check(rc, what):
    if rc != 0:
        raise N3dtError("%s failed (%d): %s" % (what, rc, lib().n3dt_last_error().decode()))
