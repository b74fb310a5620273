"""ctypes binding of libuwie.so (include/uwie.h).  No CPU fallback: a missing library is an error."""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libuwie.so")
CSRC = os.path.join(_HERE, "csrc")

SURFACE_SIX, SURFACE_DICT = 0, 1
STATUS_DIFF_RANK = 16  # include/uwie.h UWIE_STATUS_DIFF_RANK
STATUS_CLASSIFY_NAN = 64  # include/uwie.h UWIE_STATUS_CLASSIFY_NAN
LOSS_IDENTITY, LOSS_VGG, LOSS_GATED = 0, 1, 2  # include/uwie.h UWIE_LOSS_*
VGG_F32, VGG_F16, VGG_PARAMS = 0, 1, 1735488  # include/uwie.h UWIE_VGG_F32, UWIE_VGG_F16, UWIE_VGG_PARAMS
PARAM_NET_PARAMS = {True: 8500100, False: 8459652}  # include/uwie.h UWIE_PARAM_NET_PARAMS(use_features)
MASKS_GIVEN, MASKS_DRAWN = 0, 1  # include/uwie.h UWIE_MASKS_*
TRAINER_PARAMS, TRAINER_GRADS, TRAINER_EXP_AVG, TRAINER_EXP_AVG_SQ = 0, 1, 2, 3  # include/uwie.h UWIE_TRAINER_*
FLIP_LR, FLIP_UD = 1, 2  # include/uwie.h UWIE_FLIP_LR, UWIE_FLIP_UD
RESIZE_MAX_SIDE, RESIZE_MAX_SRC = 4096, 32768  # include/uwie.h UWIE_RESIZE_MAX_SIDE, UWIE_RESIZE_MAX_SRC
INTER_F64, INTER_FX32, INTER_F32T = 0, 1, 2  # uwie_params.inter_dtype
DICT_STRATEGIES = {
    "strong_dehazing": 0,
    "medium_dehazing": 1,
    "light_enhancement": 2,
    "clahe_enhancement": 3,
    "histogram_equalization": 4,
}
CAST_KINDS = ("normal", "greenish", "bluish")


class UwieError(RuntimeError):
    pass


class UwieParams(ctypes.Structure):
    """Mirror of ``struct uwie_params`` (include/uwie.h)."""

    _fields_ = [
        ("surface", ctypes.c_int32),
        ("strategy", ctypes.c_int32),
        ("cast_correct", ctypes.c_int32),
        ("forced_cast", ctypes.c_int32),
        ("gray_shift", ctypes.c_int32),
        ("min_size", ctypes.c_int32),
        ("omega", ctypes.c_double),
        ("gf_ksize", ctypes.c_int32),
        ("gf_eps", ctypes.c_double),
        ("L_low", ctypes.c_double),
        ("L_high", ctypes.c_double),
        ("wb_percentile", ctypes.c_double),
        ("clip_limit", ctypes.c_double),
        ("tiles_x", ctypes.c_int32),
        ("tiles_y", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("apply_gamma", ctypes.c_int32),
        ("gf_exact", ctypes.c_int32),
        ("inter_dtype", ctypes.c_int32),
        ("dark_patch", ctypes.c_int32),
    ]


class UwieModelDesc(ctypes.Structure):
    """Mirror of ``struct uwie_model_desc`` (include/uwie.h): host arrays of one exported classifier."""

    _fields_ = [("kind", ctypes.c_int32), ("n_features", ctypes.c_int32), ("n_classes", ctypes.c_int32),
                ("n_trees", ctypes.c_int32), ("n_nodes", ctypes.c_int32), ("n_sv", ctypes.c_int32),
                ("mean", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("tree_offset", ctypes.c_void_p), ("left", ctypes.c_void_p), ("right", ctypes.c_void_p),
                ("feature", ctypes.c_void_p), ("threshold", ctypes.c_void_p), ("missing_left", ctypes.c_void_p),
                ("value", ctypes.c_void_p), ("learning_rate", ctypes.c_double), ("init", ctypes.c_void_p),
                ("sv", ctypes.c_void_p), ("dual_coef", ctypes.c_void_p), ("intercept", ctypes.c_void_p),
                ("n_support", ctypes.c_void_p), ("prob_a", ctypes.c_void_p), ("prob_b", ctypes.c_void_p),
                ("gamma", ctypes.c_double)]


class UwieClahePlan(ctypes.Structure):
    """Mirror of ``struct uwie_clahe_plan_info`` (include/uwie.h): how the CLAHE tail of a call is launched."""

    _fields_ = [(name, ctypes.c_int32) for name in ("tile_w", "tile_h", "padded", "clip_limit", "wide_lut", "nchunk",
                                                    "cells_walk", "cells_flat")]


def clahe_plan(batch, H, W, tiles=(8, 8), clip_limit=2.0, recomputed=False) -> UwieClahePlan:
    """uwie_clahe_plan: needs the library, not a device."""
    out = UwieClahePlan()
    check(load().uwie_clahe_plan(batch, H, W, int(tiles[0]), int(tiles[1]), float(clip_limit), int(bool(recomputed)),
                                 ctypes.byref(out)))
    return out


def dark_patch_plan(H, W, k) -> tuple[int, int]:
    """uwie_dark_patch_plan: (tile_w, tile_h) of one workgroup of the patched transmission kernel.  Needs the library, not a device."""
    tw, th = ctypes.c_int(), ctypes.c_int()
    check(load().uwie_dark_patch_plan(int(H), int(W), int(k), ctypes.byref(tw), ctypes.byref(th)))
    return tw.value, th.value


UW_SCORES = 8  # include/uwie.h UWIE_UW_SCORES


def underwater_plan(H, W) -> tuple[int, int]:
    """uwie_underwater_plan: (tile_w, tile_h) of one workgroup of the underwater scores' block pass.  Needs the library, not a device."""
    tw, th = ctypes.c_int(), ctypes.c_int()
    check(load().uwie_underwater_plan(int(H), int(W), ctypes.byref(tw), ctypes.byref(th)))
    return tw.value, th.value


REF_SCORES = 8  # include/uwie.h UWIE_REF_SCORES


def reference_plan(H, W) -> tuple[int, int]:
    """uwie_reference_plan: (tile_w, tile_h) in map points of one workgroup of the reference scores' SSIM pass.  Needs the library, not a device."""
    tw, th = ctypes.c_int(), ctypes.c_int()
    check(load().uwie_reference_plan(int(H), int(W), ctypes.byref(tw), ctypes.byref(th)))
    return tw.value, th.value


GW_STATS = 12  # include/uwie.h UWIE_GW_STATS


def gray_world_plan(H, W) -> tuple[int, int]:
    """uwie_gray_world_plan: (block_px, thread_px), the pixels per workgroup of the sum pass and per thread of the apply pass.
    Needs the library, not a device."""
    bp, tp = ctypes.c_int(), ctypes.c_int()
    check(load().uwie_gray_world_plan(int(H), int(W), ctypes.byref(bp), ctypes.byref(tp)))
    return bp.value, tp.value


def fusion_plan(H, W, levels=1) -> tuple[int, int]:
    """uwie_fusion_plan: (tile_w, tile_h), the level-0 tile one workgroup stages with its halo.  Needs the library, not a device."""
    tw, th = ctypes.c_int(), ctypes.c_int()
    check(load().uwie_fusion_plan(int(H), int(W), int(levels), ctypes.byref(tw), ctypes.byref(th)))
    return tw.value, th.value


def fusion_table(gamma):
    """uwie_fusion_table: G[v] = rint(255 (v / 255)^gamma) as 256 bytes (NumPy uint8).  Needs the library, not a device."""
    import numpy as np

    buf = (ctypes.c_uint8 * 256)()
    check(load().uwie_fusion_table(float(gamma), buf))
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy()


# name -> argument types (return type is int unless listed in _RESTYPES)
_VP, _SZ, _I, _D = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
_PP = ctypes.POINTER(UwieParams)
_PM = ctypes.POINTER(UwieModelDesc)
_PI = ctypes.POINTER(_I)
SIGNATURES = {
    "uwie_last_error": [],
    "uwie_version": [],
    "uwie_create": [_I, ctypes.POINTER(_VP)],
    "uwie_destroy": [_VP],
    "uwie_device_status": [_VP, _VP, ctypes.POINTER(ctypes.c_uint32)],
    "uwie_profile_enable": [_VP, _I],
    "uwie_profile_filter": [_VP, ctypes.c_char_p],
    "uwie_profile_collect": [_VP],
    "uwie_profile_row": [_VP, _I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_D), ctypes.POINTER(_I)],
    "uwie_params_init": [_PP, _I, _I],
    "uwie_set_tuning": [_VP, ctypes.c_char_p, _I],
    "uwie_get_tuning": [_VP, ctypes.c_char_p, ctypes.POINTER(_I)],
    "uwie_workspace_bytes": [_I, _I, _I, _PP],
    "uwie_workspace_bytes_ctx": [_VP, _I, _I, _I, _PP],
    "uwie_workspace_bytes_all": [_I, _I, _I, _VP],
    "uwie_workspace_bytes_float": [_I, _I, _I, _PP, _I],
    "uwie_enhance_f32": [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _PP, _VP, _SZ, _VP],
    "uwie_enhance_f64": [_VP, _VP, _VP, _VP, _I, _I, _I, _PP, _VP, _SZ, _VP],
    "uwie_cast_classify_f32": [_VP, _VP, _I, _I, _I, _VP, _VP, _VP],
    "uwie_color_correct_f32": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP],
    "uwie_guided_plan": [_I, _I, _I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "uwie_guided_fill": [_I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)],
    "uwie_clahe_plan": [_I, _I, _I, _I, _I, _D, _I, ctypes.POINTER(UwieClahePlan)],
    "uwie_dark_patch_plan": [_I, _I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "uwie_enhance_u8": [_VP, _VP, _VP, _VP, _I, _I, _I, _PP, _VP, _SZ, _VP],
    "uwie_enhance_u8_f64": [_VP, _VP, _VP, _VP, _I, _I, _I, _PP, _VP, _SZ, _VP],
    "uwie_enhance_percentiles": [_VP, _VP, _SZ, _I, _I, _I, _PP, _VP, _VP],
    "uwie_enhance_all_u8": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_workspace_bytes_select": [_I, _I, _I, _VP, _I, _I],
    "uwie_select_best_u8": [_VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_workspace_bytes_underwater": [_I, _I, _I],
    "uwie_underwater_plan": [_I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "uwie_underwater_scores_u8": [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_workspace_bytes_reference": [_I, _I, _I],
    "uwie_reference_plan": [_I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "uwie_reference_scores_u8": [_VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_workspace_bytes_gray_world": [_I, _I, _I],
    "uwie_gray_world_plan": [_I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "uwie_gray_world_u8": [_VP, _VP, _I, _I, _I, _D, _D, _D, _VP, _VP, _VP, _SZ, _VP],
    "uwie_workspace_bytes_fusion": [_I, _I, _I, _I],
    "uwie_fusion_plan": [_I, _I, _I, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)],
    "uwie_fusion_table": [_D, ctypes.POINTER(ctypes.c_uint8)],
    "uwie_fusion_u8": [_VP, _VP, _I, _I, _I, _D, _I, _I, _VP, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_pick_best_u8": [_VP, _VP, _I, _I, _I, _I, _VP, _I, _I, _VP, _VP, _VP],
    "uwie_diff_enhance_f32": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _SZ, _VP],
    "uwie_diff_enhance_save_f32": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _VP, _SZ, _VP],
    "uwie_diff_enhance_bwd_workspace_bytes": [_I, _I, _I],
    "uwie_workspace_bytes_diff_u8": [_I, _I, _I],
    "uwie_diff_enhance_u8": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _SZ, _VP],
    "uwie_diff_enhance_bwd_f32": [_VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_diff_gated_f32": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _SZ, _VP],
    "uwie_diff_gated_save_f32": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _VP, _SZ, _VP],
    "uwie_diff_gated_bwd_workspace_bytes": [_I, _I, _I],
    "uwie_workspace_bytes_diff_gated_u8": [_I],
    "uwie_diff_gated_u8": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _SZ, _VP],
    "uwie_diff_gated_bwd_f32": [_VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_ref_loss_workspace_bytes": [_I, _I, _I],
    "uwie_ref_loss_f32": [_VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_ref_loss_bwd_f32": [_VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_device_status_async": [_VP, _VP, _VP],
    "uwie_vgg_create": [_VP, _VP, _I, ctypes.POINTER(_VP)],
    "uwie_vgg_destroy": [_VP],
    "uwie_perceptual_workspace_bytes": [_I, _I, _I, _I],
    "uwie_perceptual_f32": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_perceptual_bwd_f32": [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _SZ, _VP],
    "uwie_param_net_create": [_VP, _VP, _I, ctypes.POINTER(_VP)],
    "uwie_param_net_destroy": [_VP],
    "uwie_param_net_workspace_bytes": [_I, _I, _I],
    "uwie_param_net_f32": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _SZ, _VP],
    "uwie_mlp_create": [_VP, _VP, _I, _I, _I, ctypes.POINTER(_VP)],
    "uwie_mlp_destroy": [_VP],
    "uwie_mlp_workspace_bytes": [_I, _I],
    "uwie_mlp_forward": [_VP, _VP, _VP, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_mlp_trainer_create": [_VP, _VP, _I, _I, _I, ctypes.POINTER(_VP)],
    "uwie_mlp_trainer_destroy": [_VP],
    "uwie_mlp_train_workspace_bytes": [_I, _I, _I],
    "uwie_mlp_train_forward": [_VP, _VP, _VP, _I, _I, _D, _I, _VP, ctypes.c_uint64, _VP, _VP, _SZ, _VP],
    "uwie_mlp_backward": [_VP, _VP, _VP, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_mlp_adam_step": [_VP, _VP, _D, _D, _D, _D, _D, _VP, _VP],
    "uwie_mlp_trainer_get": [_VP, _I, _VP],
    "uwie_mlp_trainer_set": [_VP, _I, _VP],
    "uwie_mlp_trainer_step_count": [_VP],
    "uwie_mlp_trainer_set_step_count": [_VP, ctypes.c_longlong],
    "uwie_mlp_trainer_eval": [_VP, _VP, _VP, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_u8_to_f32": [_VP, _VP, _VP, _SZ, _VP],
    "uwie_extract_features_u8": [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP],
    "uwie_feature_extractor_count": [_I, _I],
    "uwie_workspace_bytes_feature_extractor": [_I, _I, _I],
    "uwie_feature_extractor_u8": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _SZ, _VP],
    "uwie_model_check": [_PM],
    "uwie_model_create": [_VP, _PM, ctypes.POINTER(_VP)],
    "uwie_model_destroy": [_VP],
    "uwie_model_info": [_VP, _PI, _PI, _PI],
    "uwie_classify_f64": [_VP, _VP, _VP, _I, _I, _VP, _VP, _VP],
    "uwie_workspace_bytes_predict": [_I, _I, _I],
    "uwie_predict_strategy_u8": [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_resize_rgb_u8": [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "uwie_quality_scores": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _SZ, _VP],
    "uwie_cast_classify": [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _SZ, _VP],
    "uwie_normalise_correct": [_VP, _VP, _VP, _VP, _I, _I, _I, _VP],
    "uwie_atmospheric_light": [_VP, _VP, _VP, _I, _I, _I, _PP, _VP, _VP, _VP, _SZ, _VP],
    "uwie_transmission_init": [_VP, _VP, _VP, _VP, _I, _I, _I, _PP, _VP, _VP, _VP],
    "uwie_box_filter_f64": [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _SZ, _VP],
    "uwie_guided_filter": [_VP, _VP, _VP, _I, _I, _I, _I, _D, _I, _VP, _VP, _SZ, _VP],
    "uwie_restore": [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _VP, _VP],
    "uwie_percentiles_f32": [_VP, _VP, _I, _I, _I, ctypes.POINTER(_D), _I, _VP, _VP, _SZ, _VP],
    "uwie_percentiles_f64": [_VP, _VP, _I, _I, _I, ctypes.POINTER(_D), _I, _VP, _VP, _SZ, _VP],
    "uwie_stretch_f32": [_VP, _VP, _VP, _I, _I, _I, _D, _D, _VP, _SZ, _VP],
    "uwie_gamma_f32": [_VP, _VP, _VP, _SZ, _D, _I, _VP],
    "uwie_clahe_f32": [_VP, _VP, _VP, _I, _I, _I, _D, _I, _I, _VP, _SZ, _VP],
    "uwie_rgb2gray_u8": [_VP, _VP, _VP, _SZ, _I, _VP],
    "uwie_rgb2lab_u8": [_VP, _VP, _VP, _SZ, _VP],
    "uwie_lab2rgb_u8": [_VP, _VP, _VP, _SZ, _VP],
    "uwie_clahe_u8": [_VP, _VP, _VP, _I, _I, _I, _D, _I, _I, _VP, _SZ, _VP],
    "uwie_canny_u8": [_VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _SZ, _VP],
    "uwie_equalize_hist_u8": [_VP, _VP, _VP, _I, _I, _I, _VP, _SZ, _VP],
}
_RESTYPES = {
    "uwie_last_error": ctypes.c_char_p,
    "uwie_version": ctypes.c_char_p,
    "uwie_destroy": None,
    "uwie_workspace_bytes": ctypes.c_size_t,
    "uwie_workspace_bytes_ctx": ctypes.c_size_t,
    "uwie_workspace_bytes_all": ctypes.c_size_t,
    "uwie_workspace_bytes_float": ctypes.c_size_t,
    "uwie_workspace_bytes_select": ctypes.c_size_t,
    "uwie_workspace_bytes_underwater": ctypes.c_size_t,
    "uwie_workspace_bytes_reference": ctypes.c_size_t,
    "uwie_workspace_bytes_gray_world": ctypes.c_size_t,
    "uwie_workspace_bytes_fusion": ctypes.c_size_t,
    "uwie_diff_enhance_bwd_workspace_bytes": ctypes.c_size_t,
    "uwie_workspace_bytes_diff_u8": ctypes.c_size_t,
    "uwie_diff_gated_bwd_workspace_bytes": ctypes.c_size_t,
    "uwie_ref_loss_workspace_bytes": ctypes.c_size_t,
    "uwie_workspace_bytes_feature_extractor": ctypes.c_size_t,
    "uwie_workspace_bytes_predict": ctypes.c_size_t,
    "uwie_model_destroy": None,
    "uwie_perceptual_workspace_bytes": ctypes.c_size_t,
    "uwie_vgg_destroy": None,
    "uwie_param_net_workspace_bytes": ctypes.c_size_t,
    "uwie_param_net_destroy": None,
    "uwie_workspace_bytes_diff_gated_u8": ctypes.c_size_t,
    "uwie_mlp_workspace_bytes": ctypes.c_size_t,
    "uwie_mlp_destroy": None,
    "uwie_mlp_train_workspace_bytes": ctypes.c_size_t,
    "uwie_mlp_trainer_destroy": None,
    "uwie_mlp_trainer_step_count": ctypes.c_longlong,
}

_lib = None


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-j8"])
    return LIB_PATH


def load() -> ctypes.CDLL:
    """Load libuwie.so; raises UwieError when it has not been built (there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UwieError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(the enhancement path has no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means the .so does not match include/uwie.h
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().uwie_last_error()
        raise UwieError(f"libuwie error {rc}: {msg.decode() if msg else '?'}")
