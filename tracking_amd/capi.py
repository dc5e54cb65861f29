"""ctypes binding of libbgs_hip's C ABI (include/bgs_hip.h) — plumbing only.

This module never computes anything itself and has no CPU path: if the HIP library is
missing it raises at import of the symbols, and every call into a box without a GPU
fails with BgsError(BGS_ERR_HIP).
"""
import collections
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BGS_LIB_PATH") or os.path.join(_HERE, "lib", "libbgs_hip.so")  # BGS_LIB_PATH: A/B builds of the same ABI (tools/)

# bgs_algo (include/bgs_hip.h)
FRAME_DIFF, STATIC_FRAME_DIFF, WMM, WMV, ABL, ASBL, MOG2, MOG1, GMG, SUBSENSE, LBSP_DESC, SIGMA_DELTA = range(12)
DP_ZIVKOVIC_AGMM, DP_GRIMSON_GMM, DP_WREN_GA, DP_MEAN, DP_ADAPTIVE_MEDIAN = range(12, 17)
LOBSTER = 17
KDE = 18
DP_PRATI_MEDIOD, DP_TEXTURE = 19, 20
LB_SIMPLE_GAUSSIAN, LB_FUZZY_GAUSSIAN, LB_MOG, LB_ADAPTIVE_SOM, LB_FUZZY_ADAPTIVE_SOM = range(21, 26)
VUMETER = 27  # id 26 is a permanent hole (BGS_ALGO_END is frozen there)
ALGO_LIMIT = 28  # frozen, and id 28 is the second permanent hole
FUZZY_SUGENO, FUZZY_CHOQUET = 29, 30  # package_bgs/tb fuzzy integrals; their parameters are BgsFuzzyParams, not BgsParams
T2FGMM_UM, T2FGMM_UV = 32, 33  # package_bgs/tb type-2 fuzzy GMMs (id 31 is the third hole); their parameters are BgsT2fParams
DP_EIGENBACKGROUND = 34  # package_bgs/dp PCA background; its parameters are BgsEigenParams
IMBS = 35  # package_bgs/db IndependentMultimodalBGS; its parameters are BgsImbsParams
MULTILAYER = 36  # package_bgs/jmo MultiLayerBGS; its parameters are BgsMultilayerParams
ALGO_LAST = 37  # one past the last id
PRATI_MAX_HISTORY = 64  # BGS_PRATI_MAX_HISTORY
EIGEN_MAX_HISTORY = 32  # BGS_EIGEN_MAX_HISTORY
IMBS_MAX_SAMPLES = 63  # BGS_IMBS_MAX_SAMPLES
MULTILAYER_MAX_HALF_SIZE = 8  # BGS_MULTILAYER_MAX_HALF_SIZE
CANNY_MAX_PIXELS = 20480  # BGS_CANNY_MAX_PIXELS
MULTICUE_TEXTURE_SLOTS, MULTICUE_TEXTURE_CACHE_SLOTS, MULTICUE_COLOR_SLOTS, MULTICUE_COLOR_CACHE_SLOTS = 20, 16, 32, 16  # BGS_MULTICUE_*_SLOTS
MULTICUE_MAX_BOXES, MULTICUE_BOX_FIELDS = 300, 13  # BGS_MULTICUE_MAX_BOXES, BGS_MULTICUE_BOX_FIELDS
FG_VALID, BG_VALID = 1, 2
OPT_BORROW_FRAMES, OPT_MOG2_PIXELS_PER_LANE, OPT_MOG2_TILED, OPT_XCD_SWIZZLE, OPT_PLACEMENT_PROBE, OPT_MOG2_SPARSE, OPT_CLIP_FUSE, OPT_HOST_REGISTER, OPT_MODEL_CHUNK_MB, OPT_MODEL_CHUNK_MIN_MB = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10

OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_GEOMETRY, ERR_HIP, ERR_NOMEM, ERR_STATE = 0, -1, -2, -3, -4, -5, -6


class BgsParams(C.Structure):
    """struct bgs_params, field for field."""
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("enable_threshold", C.c_int32),
        ("threshold", C.c_int32),
        ("enable_weight", C.c_int32),
        ("alpha", C.c_double),
        ("limit", C.c_int32),
        ("learning_frames", C.c_int32),
        ("alpha_learn", C.c_double),
        ("alpha_detection", C.c_double),
        ("mog2_history", C.c_int32),
        ("mog2_nmixtures", C.c_int32),
        ("mog2_var_threshold", C.c_float),
        ("mog2_background_ratio", C.c_float),
        ("mog2_var_threshold_gen", C.c_float),
        ("mog2_var_init", C.c_float),
        ("mog2_var_min", C.c_float),
        ("mog2_var_max", C.c_float),
        ("mog2_ct", C.c_float),
        ("mog2_tau", C.c_float),
        ("mog2_detect_shadows", C.c_int32),
        ("mog2_shadow_value", C.c_int32),
        ("mog1_history", C.c_int32),
        ("mog1_nmixtures", C.c_int32),
        ("mog1_background_ratio", C.c_double),
        ("mog1_var_threshold", C.c_double),
        ("mog1_noise_sigma", C.c_double),
        ("lbsp_rel_threshold", C.c_float),
        ("lbsp_threshold_offset", C.c_int32),
        ("subsense_min_color_dist_threshold", C.c_int32),
        ("subsense_n_samples", C.c_int32),
        ("subsense_n_required", C.c_int32),
        ("subsense_samples_for_moving_avgs", C.c_int32),
        ("sd_amp_factor", C.c_int32),
        ("sd_min_var", C.c_int32),
        ("sd_max_var", C.c_int32),
        ("subsense_desc_dist_threshold_offset", C.c_int32),
        ("gmg_max_features", C.c_int32),
        ("gmg_init_frames", C.c_int32),
        ("gmg_quantization_levels", C.c_int32),
        ("gmg_smoothing_radius", C.c_int32),
        ("gmg_update_background_model", C.c_int32),
        ("dp_sampling_rate", C.c_int32),
        ("gmg_learning_rate", C.c_double),
        ("gmg_background_prior", C.c_double),
        ("gmg_decision_threshold", C.c_double),
        ("dp_threshold", C.c_float),
        ("dp_alpha", C.c_float),
        ("dp_gaussians", C.c_int32),
        ("kde_frames_to_learn", C.c_int32),
        ("kde_sequence_length", C.c_int32),
        ("kde_time_window", C.c_int32),
        ("kde_sd_estimation", C.c_int32),
        ("kde_color_ratios", C.c_int32),
        ("kde_update_model", C.c_int32),
        ("kde_threshold", C.c_double),
        ("kde_alpha", C.c_double),
        ("dp_history_size", C.c_int32),
        ("dp_weight", C.c_int32),
        ("lb_sensitivity", C.c_int32),
        ("lb_bg_threshold", C.c_int32),
        ("lb_learning_rate", C.c_int32),
        ("lb_noise_variance", C.c_int32),
        ("lb_training_sensitivity", C.c_int32),
        ("lb_training_learning_rate", C.c_int32),
        ("lb_training_steps", C.c_int32),
        ("vu_bin_size", C.c_int32),
        ("vu_enable_filter", C.c_int32),
        ("vu_alpha", C.c_double),
        ("vu_threshold", C.c_double),
    ]


class BgsFuzzyParams(C.Structure):
    """struct bgs_fuzzy_params, field for field (FuzzySugenoIntegral / FuzzyChoquetIntegral)."""
    _fields_ = [("struct_size", C.c_uint32), ("frames_to_learn", C.c_int32), ("alpha_learn", C.c_double), ("alpha_update", C.c_double),
                ("color_space", C.c_int32), ("option", C.c_int32), ("smooth", C.c_int32), ("reserved_", C.c_int32), ("threshold", C.c_double)]


class BgsT2fParams(C.Structure):
    """struct bgs_t2f_params, field for field (T2FGMM_UM / T2FGMM_UV)."""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_double), ("alpha", C.c_double), ("km", C.c_float), ("kv", C.c_float), ("gaussians", C.c_int32)]


class BgsEigenParams(C.Structure):
    """struct bgs_eigen_params, field for field (DPEigenbackground)."""
    _fields_ = [("struct_size", C.c_uint32), ("threshold", C.c_int32), ("history_size", C.c_int32), ("embedded_dim", C.c_int32)]


class BgsImbsParams(C.Structure):
    """struct bgs_imbs_params, field for field (IndependentMultimodalBGS)."""
    _fields_ = [("struct_size", C.c_uint32), ("fgThreshold", C.c_uint32), ("fps", C.c_double), ("associationThreshold", C.c_uint32), ("samplingPeriod", C.c_uint32),
                ("minBinHeight", C.c_uint32), ("numSamples", C.c_uint32), ("alpha", C.c_float), ("beta", C.c_float), ("tau_s", C.c_int32), ("tau_h", C.c_int32),
                ("minArea", C.c_double), ("persistencePeriod", C.c_uint32), ("morphologicalFiltering", C.c_int32)]


class BgsMultilayerParams(C.Structure):
    """struct bgs_multilayer_params, field for field (MultiLayerBGS)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_mode_num", C.c_int32), ("weight_updating_constant", C.c_float), ("texture_weight", C.c_float), ("bg_mode_percent", C.c_float),
                ("pattern_neig_half_size", C.c_int32), ("pattern_neig_gaus_sigma", C.c_float), ("bg_prob_threshold", C.c_float), ("bg_prob_updating_threshold", C.c_float),
                ("robust_LBP_constant", C.c_int32), ("min_noised_angle", C.c_float), ("shadow_rate", C.c_float), ("highlight_rate", C.c_float), ("frame_duration", C.c_float),
                ("learn_mode_learn_rate_per_second", C.c_float), ("learn_weight_learn_rate_per_second", C.c_float), ("learn_init_mode_weight", C.c_float),
                ("detect_mode_learn_rate_per_second", C.c_float), ("detect_weight_learn_rate_per_second", C.c_float), ("detect_init_mode_weight", C.c_float),
                ("status", C.c_int32), ("disable_detect_mode", C.c_int32), ("disable_learning", C.c_int32), ("detect_after", C.c_int32)]


class BgsMulticueParams(C.Structure):
    """struct bgs_multicue_params, field for field (SJN_MultiCueBGS; a bgs_multicue handle takes it at creation, no bgs_engine does)."""
    _fields_ = [("struct_size", C.c_uint32), ("training_period", C.c_int32), ("t_model_threshold", C.c_int32), ("c_model_threshold", C.c_int32), ("learning_rate", C.c_float),
                ("texture_train_vol_range", C.c_int32), ("color_train_vol_range", C.c_int32), ("absorption_enable", C.c_int32), ("absorption_period", C.c_int32),
                ("reduced_width", C.c_int32), ("reduced_height", C.c_int32), ("back_clear_period", C.c_int32), ("cache_clear_period", C.c_int32)]


class ParamBlock(collections.namedtuple("ParamBlock", "name struct classes check_takes_algo live")):
    """A class parameter block of the C ABI: struct bgs_<name>_params with bgs_<name>_default_params, bgs_set_<name>_params,
    bgs_get_<name>_params and bgs_<name>_check.  check_takes_algo: bgs_<name>_check's first argument is the algorithm (blocks that
    several classes share).  live: a set after the geometry acts from the next frame on; otherwise it is vetted and changes nothing."""


# One row per block.  From it come the blocks' entries of SYMBOLS, <name>_default_params(**kw) below and
# Engine.set_<name>_params / Engine.get_<name>_params (engine.py).
PARAM_BLOCKS = [
    ParamBlock("fuzzy", BgsFuzzyParams, "FUZZY_SUGENO / FUZZY_CHOQUET", True, True),
    ParamBlock("t2f", BgsT2fParams, "T2FGMM_UM / T2FGMM_UV", True, False),
    ParamBlock("eigen", BgsEigenParams, "DPEigenbackground", False, False),
    ParamBlock("imbs", BgsImbsParams, "IndependentMultimodalBGS", False, False),
    ParamBlock("multilayer", BgsMultilayerParams, "MultiLayerBGS", False, False),
]


class BgsError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libbgs_hip error %d: %s" % (code, text))
        self.code = code


# every symbol include/bgs_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("bgs_abi_version", C.c_int, []),
    ("bgs_default_params", C.c_int, [C.c_int, C.POINTER(BgsParams)]),
    ("bgs_create", C.c_int, [C.c_int, C.POINTER(BgsParams), C.c_int, C.c_int, C.POINTER(_P)]),
    ("bgs_set_params", C.c_int, [_P, C.POINTER(BgsParams)]),
    ("bgs_multilayer_constants", C.c_int, [C.POINTER(BgsMultilayerParams), C.POINTER(C.c_uint32)]),
    ("bgs_set_option", C.c_int, [_P, C.c_int, C.c_int64]),
    ("bgs_set_geometry", C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    ("bgs_process", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_uint32)]),
    ("bgs_process_batch_device", C.c_int, [_P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("bgs_process_range_device", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("bgs_process_clip_device", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("bgs_get_state", C.c_int64, [_P, C.c_int, C.c_char_p, _P, C.c_size_t]),
    ("bgs_frames_seen", C.c_int64, [_P, C.c_int]),
    ("bgs_enable_kernel_timing", C.c_int, [_P, C.c_int]),
    ("bgs_kernel_timing", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_char_p)]),
    ("bgs_kernel_timing_series", C.c_int64, [_P, C.POINTER(C.c_float), C.c_int64]),
    ("bgs_calibrate_copy", C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("bgs_calibrate_pcie", C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("bgs_destroy", None, [_P]),
    ("bgs_last_error", C.c_char_p, []),
    ("bgs_lbsp_describe_device", C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("bgs_lbsp_describe_batch_device", C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("bgs_mask_morph_device", C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("bgs_canny_device", C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("bgs_lbpmrf_mask_check", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float]),
    ("bgs_lbpmrf_mask_device", C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    ("bgs_lbpmrf_mask_counters", C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("bgs_multicue_default_params", C.c_int, [C.POINTER(BgsMulticueParams)]),
    ("bgs_multicue_check", C.c_int, [C.POINTER(BgsMulticueParams), C.c_int, C.c_int]),
    ("bgs_multicue_create", C.c_int, [C.c_int, C.c_int, C.POINTER(BgsMulticueParams), C.POINTER(_P)]),
    ("bgs_multicue_destroy", None, [_P]),
    ("bgs_multicue_train_device", C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    ("bgs_multicue_landmark_device", C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P, _P]),
    ("bgs_multicue_update_device", C.c_int, [_P, _P, C.c_int, _P]),
    ("bgs_multicue_get_state", C.c_int64, [_P, C.c_int, C.c_char_p, _P, C.c_size_t]),
    ("bgs_multicue_boxes_device", C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("bgs_multicue_process_device", C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    ("bgs_multicue_process_range_device", C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    ("bgs_multicue_reset_stream", C.c_int, [_P, C.c_int]),
    ("bgs_multicue_process", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_size_t, _P, C.c_size_t, C.c_int]),
    ("bgs_multicue_xyz_device", C.c_int, [C.c_int, _P, _P, C.c_size_t, _P]),
    ("bgs_mask_components_workspace", C.c_size_t, [C.c_int, C.c_int]),
    ("bgs_mask_components_device", C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    ("bgs_mask_components_batch_workspace", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("bgs_mask_components_batch_device", C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    ("bgs_mask_blobs_batch_device", C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    ("bgs_ingest_default", C.c_int, [_P]),
    ("bgs_ingest_size", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("bgs_ingest_workspace", C.c_size_t, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("bgs_ingest_device", C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, _P, _P, _P]),
    ("bgs_set_ingest", C.c_int, [_P, _P]),
    ("bgs_ingest_host", C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, _P, C.c_size_t]),
    ("bgs_group_create", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("bgs_group_destroy", None, [_P]),
    ("bgs_group_size", C.c_int, [_P]),
    ("bgs_group_is_fused", C.c_int, [_P, C.c_int]),
    ("bgs_group_set_params", C.c_int, [_P, C.c_int, _P]),
    ("bgs_group_set_option", C.c_int, [_P, C.c_int, C.c_int64]),
    ("bgs_group_set_geometry", C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    ("bgs_group_process_batch_device", C.c_int, [_P, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("bgs_group_process", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("bgs_group_get_state", C.c_int64, [_P, C.c_int, C.c_int, C.c_char_p, _P, C.c_size_t]),
    ("bgs_group_frames_seen", C.c_int64, [_P]),
    ("bgs_group_enable_kernel_timing", C.c_int, [_P, C.c_int]),
    ("bgs_group_kernel_timing", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    ("bgs_submit", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t]),
    ("bgs_wait", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32)]),
    ("bgs_host_arena", C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    ("bgs_reset_stream", C.c_int, [_P, C.c_int]),
    ("bgs_stream_flags", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32)]),
    ("bgs_last_mask_blobs", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
]
for _b in PARAM_BLOCKS:
    SYMBOLS += [
        ("bgs_%s_default_params" % _b.name, C.c_int, [C.POINTER(_b.struct)]),
        ("bgs_set_%s_params" % _b.name, C.c_int, [_P, C.POINTER(_b.struct)]),
        ("bgs_get_%s_params" % _b.name, C.c_int, [_P, C.POINTER(_b.struct)]),
        ("bgs_%s_check" % _b.name, C.c_int, ([C.c_int] if _b.check_takes_algo else []) + [C.POINTER(_b.struct), C.c_int, C.c_int, C.c_int]),
    ]

_lib = None


def lib():
    """Load libbgs_hip.so (built in-tree by __graft_entry__.build()).  No fallback of any kind."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libbgs_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` (%s)" % LIB_PATH)
        # torch ships its own copy of the HIP runtime (same soname, libamdhip64.so.7).  Whichever copy a process loads first serves
        # both; loaded in the other order - this library first, torch afterwards - torch came up with "No HIP GPUs are available"
        # on the GPU boxes (round 3, a test run that touched the C ABI before its first torch.cuda call).  So where torch exists
        # (tests, bench.py) it is imported first; a C++ host never has it and is not affected.
        try:
            import torch  # noqa: F401
        except Exception:  # noqa: BLE001
            pass
        l = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            if os.environ.get("BGS_LIB_PATH") and os.environ.get("BGS_LIB_PARTIAL_ABI") and not hasattr(l, name):
                continue  # A/B against an older build of the library (tools/): entry points it lacks simply stay unbound
            fn = getattr(l, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def last_error():
    return (lib().bgs_last_error() or b"").decode("utf-8", "replace")


def check(rc):
    if rc < 0:
        raise BgsError(rc, last_error())
    return rc


class BgsIngest(C.Structure):
    """struct bgs_ingest, field for field (N3 frame preparation)."""
    _fields_ = [("struct_size", C.c_uint32), ("resize_percent", C.c_int32), ("flip", C.c_int32), ("roi_x0", C.c_int32), ("roi_y0", C.c_int32),
                ("roi_x1", C.c_int32), ("roi_y1", C.c_int32), ("equalize_hist", C.c_int32), ("gaussian_blur", C.c_int32)]


def default_ingest(**kw):
    c = BgsIngest()
    check(lib().bgs_ingest_default(C.byref(c)))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def default_params(algo):
    p = BgsParams()
    p.struct_size = C.sizeof(BgsParams)
    check(lib().bgs_default_params(algo, C.byref(p)))
    return p


def _block_default_params(b):
    def default_params(**kw):
        p = b.struct()
        check(getattr(lib(), "bgs_%s_default_params" % b.name)(C.byref(p)))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    default_params.__name__ = default_params.__qualname__ = "%s_default_params" % b.name
    default_params.__doc__ = "bgs_%s_default_params (%s); keywords change single fields of the defaults." % (b.name, b.classes)
    return default_params


# fuzzy_default_params, t2f_default_params, eigen_default_params, imbs_default_params, multilayer_default_params
for _b in PARAM_BLOCKS:
    globals()["%s_default_params" % _b.name] = _block_default_params(_b)


def multicue_default_params(**kw):
    """bgs_multicue_default_params (the model stage of SJN_MultiCueBGS); keywords change single fields of the defaults."""
    p = BgsMulticueParams()
    check(lib().bgs_multicue_default_params(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def calibrate_copy(device, nbytes, chunk_mb, iters=5):
    """bgs_calibrate_copy: GB/s of a float4 copy over nbytes through a plain (chunk_mb = 0) or chunked allocation."""
    g = C.c_double(0)
    check(lib().bgs_calibrate_copy(device, nbytes, chunk_mb, iters, C.byref(g)))
    return g.value


def calibrate_pcie(device, nbytes, registered, iters=20):
    """bgs_calibrate_pcie: (H2D GB/s, D2H GB/s, hipHostRegister ms)"""
    u, d, r = C.c_double(0), C.c_double(0), C.c_double(0)
    check(lib().bgs_calibrate_pcie(device, nbytes, 1 if registered else 0, iters, C.byref(u), C.byref(d), C.byref(r)))
    return u.value, d.value, r.value
