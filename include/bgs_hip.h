/*
 * bgs_hip.h — C ABI of libbgs_hip, the MI355X (gfx950) foreground-detection engine.
 *
 * This is the drop-in boundary for the reference's package_bgs hot path.  The
 * reference's own surface is C++ with OpenCV types in the signature
 *     IBGS::process(const cv::Mat&, cv::Mat&, cv::Mat&)     package_bgs/IBGS.h:24
 *     USTC_BGS::Process(IplImage*) / GetMask()              ustc_src/ustc_bgs.cpp:79-113
 * so what crosses here is exactly what those calls carry once the cv::Mat /
 * IplImage header is peeled off: (data pointer, rows, cols, channels, row step)
 * for the input frame, the foreground mask and the background image.
 * No OpenCV, HIP or torch types appear in any signature; every function returns
 * 0 on success or a negative bgs_status, never throws.
 *
 * One engine owns the model state of n_streams independent camera streams of one
 * geometry, resident in HBM as SoA planes.  An engine is not
 * thread-safe (neither is an IBGS instance); use one per thread.
 */
#ifndef BGS_HIP_H
#define BGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BGS_ABI_VERSION 1

typedef struct bgs_engine bgs_engine;

/* One id per reference IBGS class on the hot path.  The comment
 * names the reference process() each one replaces. */
typedef enum bgs_algo {
  BGS_FRAME_DIFF = 0,        /* FrameDifferenceBGS::process        package_bgs/FrameDifferenceBGS.cpp:29-61 */
  BGS_STATIC_FRAME_DIFF = 1, /* StaticFrameDifferenceBGS::process  package_bgs/StaticFrameDifferenceBGS.cpp:29-57 */
  BGS_WMM = 2,               /* WeightedMovingMeanBGS::process     package_bgs/WeightedMovingMeanBGS.cpp:29-96 */
  BGS_WMV = 3,               /* WeightedMovingVarianceBGS::process package_bgs/WeightedMovingVarianceBGS.cpp:30-117 */
  BGS_ABL = 4,               /* AdaptiveBackgroundLearning::process package_bgs/AdaptiveBackgroundLearning.cpp:30-83 */
  BGS_ASBL = 5,              /* AdaptiveSelectiveBackgroundLearning::process package_bgs/AdaptiveSelectiveBackgroundLearning.cpp:31-105 */
  BGS_MOG2 = 6,              /* MixtureOfGaussianV2BGS::process    package_bgs/MixtureOfGaussianV2BGS.cpp:29-74 */
  BGS_MOG1 = 7,              /* MixtureOfGaussianV1BGS::process    package_bgs/MixtureOfGaussianV1BGS.cpp:29-71 */
  BGS_GMG = 8,               /* GMG::process                       package_bgs/GMG.cpp:35-77 */
  BGS_SUBSENSE = 9,          /* SuBSENSEBGS::process               package_bgs/pl/SuBSENSE.cpp:21-45 */
  BGS_LBSP_DESC = 10,        /* LBSP::computeRGBDescriptor         package_bgs/pl/LBSP.h:50-95 */
  BGS_SIGMA_DELTA = 11,      /* SigmaDeltaBGS::process             package_bgs/bl/SigmaDeltaBGS.cpp */
  /* the in-tree dp/ models (3-channel frames only; output = the high-threshold mask, no background image) */
  BGS_DP_ZIVKOVIC_AGMM = 12, /* DPZivkovicAGMMBGS::process         package_bgs/dp/DPZivkovicAGMMBGS.cpp:29-80 */
  BGS_DP_GRIMSON_GMM = 13,   /* DPGrimsonGMMBGS::process           package_bgs/dp/DPGrimsonGMMBGS.cpp:29-82 */
  BGS_DP_WREN_GA = 14,       /* DPWrenGABGS::process               package_bgs/dp/DPWrenGABGS.cpp:29-81 */
  BGS_DP_MEAN = 15,          /* DPMeanBGS::process                 package_bgs/dp/DPMeanBGS.cpp:29-82 */
  BGS_DP_ADAPTIVE_MEDIAN = 16, /* DPAdaptiveMedianBGS::process     package_bgs/dp/DPAdaptiveMedianBGS.cpp:29-81 */
  BGS_LOBSTER = 17,          /* LOBSTERBGS::process                package_bgs/pl/LOBSTER.cpp:20-45 */
  BGS_KDE = 18,              /* KDE::process (USTC_BGS type 32)    package_bgs/ae/KDE.cpp:34-96 */
  BGS_DP_PRATI_MEDIOD = 19,  /* DPPratiMediodBGS::process (USTC_BGS type 14) package_bgs/dp/DPPratiMediodBGS.cpp:29-81 */
  BGS_DP_TEXTURE = 20,       /* DPTextureBGS::process (USTC_BGS type 16)     package_bgs/dp/DPTextureBGS.cpp:39-134 */
  /* THE ID SPACE.  Four names below are pinned by the tests with the values they had when they were introduced, and none of them may
   * move again: BGS_ALGO_COUNT == 21 (the CPU restatement bounds its defaults table with it), BGS_ALGO_END == 26 (the end marker of
   * the lb/ round), BGS_ALGO_LIMIT == 28 (the end marker of the VuMeter round) and "ids 26 and 28 are not algorithms".  So none of
   * the three counts the classes, ids 26 and 28 are permanent holes, and the end marker every range check uses is BGS_ALGO_LAST,
   * through BGS_ALGO_KNOWN() below.  Id 31 is the third hole: the tests of the fuzzy-integral round pinned "id 31 is unknown" by
   * number, so the T2FGMM pair took 32 and 33.
   * TO ADD A CLASS: declare it after the last one with an explicit value (the old BGS_ALGO_LAST), raise BGS_ALGO_LAST by one, and
   * touch nothing else here - not BGS_ALGO_COUNT, not BGS_ALGO_END, not BGS_ALGO_LIMIT, not the holes.  The tests of the round that
   * adds the class must pin "id BGS_ALGO_LAST is unknown" through BGS_ALGO_KNOWN() and bgs_create ONLY, never the marker's value: a
   * pinned marker value is what made the two holes.  Parameters of a new class go into a struct of their own with its own
   * default / set / get calls (bgs_fuzzy_params below): tests pin sizeof(bgs_params) and its last fields. */
  BGS_ALGO_COUNT,
  /* Laurence Bender's package_bgs/lb/ models (3-channel frames only; double-precision per-pixel models; FG and BG from frame 1) */
  BGS_LB_SIMPLE_GAUSSIAN = 21,    /* LBSimpleGaussian::process (USTC_BGS type 25)     package_bgs/lb/LBSimpleGaussian.cpp:31-73 */
  BGS_LB_FUZZY_GAUSSIAN = 22,     /* LBFuzzyGaussian::process (USTC_BGS type 26)      package_bgs/lb/LBFuzzyGaussian.cpp:31-74 */
  BGS_LB_MOG = 23,                /* LBMixtureOfGaussians::process (USTC_BGS type 27) package_bgs/lb/LBMixtureOfGaussians.cpp:31-74 */
  BGS_LB_ADAPTIVE_SOM = 24,       /* LBAdaptiveSOM::process (USTC_BGS type 28)        package_bgs/lb/LBAdaptiveSOM.cpp:31-74 */
  BGS_LB_FUZZY_ADAPTIVE_SOM = 25, /* LBFuzzyAdaptiveSOM::process (USTC_BGS type 29)   package_bgs/lb/LBFuzzyAdaptiveSOM.cpp:31-74 */
  BGS_ALGO_END,                   /* FROZEN at 26 (see above); id 26 itself is a hole */
  BGS_VUMETER = 27,               /* VuMeter::process (USTC_BGS type 31)              package_bgs/av/VuMeter.cpp:33-86 */
  BGS_ALGO_LIMIT = 28,            /* FROZEN at 28 (see above); id 28 itself is a hole */
  /* package_bgs/tb fuzzy integrals (3-channel frames; float BGR background; no mask during the framesToLearn + 1 learning frames).
   * Their parameters are bgs_fuzzy_params, not bgs_params. */
  BGS_FUZZY_SUGENO = 29,          /* FuzzySugenoIntegral::process (USTC_BGS type 21)  package_bgs/tb/FuzzySugenoIntegral.cpp:31-173 */
  BGS_FUZZY_CHOQUET = 30,         /* FuzzyChoquetIntegral::process (USTC_BGS type 22) package_bgs/tb/FuzzyChoquetIntegral.cpp:31-173 */
  /* id 31 is a hole (see above) */
  /* package_bgs/tb type-2 fuzzy GMMs (3-channel frames; output = the high-threshold mask, no background image).  Their parameters
   * are bgs_t2f_params, not bgs_params. */
  BGS_T2FGMM_UM = 32,             /* T2FGMM_UM::process (USTC_BGS type 17)            package_bgs/tb/T2FGMM_UM.cpp:29-83 */
  BGS_T2FGMM_UV = 33,             /* T2FGMM_UV::process (USTC_BGS type 18)            package_bgs/tb/T2FGMM_UV.cpp:29-83 */
  /* package_bgs/dp's PCA background (3-channel frames; output = the high-threshold mask, no background image).  Its parameters are
   * bgs_eigen_params, not bgs_params. */
  BGS_DP_EIGENBACKGROUND = 34,    /* DPEigenbackgroundBGS::process (USTC_BGS type 15) package_bgs/dp/DPEigenbackgroundBGS.cpp:29-82 */
  /* package_bgs/db's IMBS (3-channel frames; output = the four-label mask 0 / 80 shadow / 180 persistence / 255 foreground and the BGR
   * background of the last model build).  Its parameters are bgs_imbs_params, not bgs_params. */
  BGS_IMBS = 35,                  /* IndependentMultimodalBGS::process (USTC_BGS type 33) package_bgs/db/IndependentMultimodalBGS.cpp:13-36 */
  /* package_bgs/jmo's multi-layer LBP + colour model (3-channel frames; output = the thresholded, smoothed distance map and the BGR
   * background of the first-ranked mode).  Its parameters are bgs_multilayer_params, not bgs_params. */
  BGS_MULTILAYER = 36,            /* MultiLayerBGS::process (USTC_BGS type 23) package_bgs/jmo/MultiLayerBGS.cpp:60-249 */
  BGS_ALGO_LAST = 37              /* one past the last id; moves with every class added */
} bgs_algo;

/* "id is an algorithm": the one range check (bgs_default_params, bgs_create, bgs_node_create) */
#define BGS_ALGO_KNOWN(id) (((int)(id) >= 0 && (int)(id) < 26) || (int)(id) == 27 || ((int)(id) >= 29 && (int)(id) < 31) || ((int)(id) >= 32 && (int)(id) < (int)BGS_ALGO_LAST))

typedef enum bgs_status {
  BGS_OK = 0,
  BGS_ERR_INVALID = -1,      /* bad argument (NULL, negative size, unknown enum) */
  BGS_ERR_UNSUPPORTED = -2,  /* input the reference would CV_Assert on (e.g. MOG2 background image of a 1-channel frame) */
  BGS_ERR_GEOMETRY = -3,     /* rows/cols/channels differ from the first frame of this engine */
  BGS_ERR_HIP = -4,          /* HIP runtime failure; text in bgs_last_error() */
  BGS_ERR_NOMEM = -5,
  BGS_ERR_STATE = -6         /* unknown state plane / buffer too small */
} bgs_status;

/* out_flags bits of bgs_process*: the reference leaves img_output / img_bgmodel
 * untouched on warm-up frames and for algorithms that never write a background
 * (SURVEY.md App. C 1-2); callers must not read a buffer whose bit is clear. */
#define BGS_FG_VALID 1u
#define BGS_BG_VALID 2u

/*
 * Parameters.  Field defaults are the values the reference's constructors and
 * loadConfig() fall back to when ./config/<Class>.xml is absent (file:line in
 * the comments).  Zero-initialise, set struct_size = sizeof(bgs_params), call
 * bgs_default_params(algo, &p), then override.
 */
typedef struct bgs_params {
  uint32_t struct_size;

  /* wrapper-level, shared by every IBGS class: cv::threshold(fg, threshold, 255, THRESH_BINARY) */
  int32_t enable_threshold;   /* 1   e.g. FrameDifferenceBGS.cpp:84 */
  int32_t threshold;          /* 15  (ASBL: 25, AdaptiveSelectiveBackgroundLearning.cpp:127) */

  /* WeightedMovingMeanBGS / WeightedMovingVarianceBGS */
  int32_t enable_weight;      /* 1   WeightedMovingMeanBGS.cpp:117 */

  /* AdaptiveBackgroundLearning, MixtureOfGaussianV1/V2 (learning rate) */
  double alpha;               /* 0.05  AdaptiveBackgroundLearning.cpp:103, MixtureOfGaussianV2BGS.cpp:92 ; MOG1: 0.05 */
  int32_t limit;              /* -1  AdaptiveBackgroundLearning.cpp:104 */

  /* AdaptiveSelectiveBackgroundLearning */
  int32_t learning_frames;    /* 90    AdaptiveSelectiveBackgroundLearning.cpp:124 */
  double alpha_learn;         /* 0.05  :125 */
  double alpha_detection;     /* 0.05  :126 */

  /* cv::BackgroundSubtractorMOG2 defaults */
  int32_t mog2_history;        /* 500 */
  int32_t mog2_nmixtures;      /* 5 (compile-time K of the kernel; other values -> BGS_ERR_UNSUPPORTED) */
  float mog2_var_threshold;    /* Tb = 16 */
  float mog2_background_ratio; /* TB = 0.9 */
  float mog2_var_threshold_gen;/* Tg = 9 */
  float mog2_var_init;         /* 15 */
  float mog2_var_min;          /* 4 */
  float mog2_var_max;          /* 75 */
  float mog2_ct;               /* 0.05 */
  float mog2_tau;              /* 0.5 */
  int32_t mog2_detect_shadows; /* 1 */
  int32_t mog2_shadow_value;   /* 127 */

  /* cv::BackgroundSubtractorMOG defaults */
  int32_t mog1_history;        /* 200 */
  int32_t mog1_nmixtures;      /* 5 */
  double mog1_background_ratio;/* 0.7 */
  double mog1_var_threshold;   /* 2.5*2.5 */
  double mog1_noise_sigma;     /* 15 (30*0.5) */

  /* LBSP descriptor / SuBSENSE (package_bgs/pl/SuBSENSE.cpp:8-14).  LOBSTER (package_bgs/pl/LOBSTER.cpp:5-12) uses the same
   * fields: lbsp_rel_threshold (0.365), lbsp_threshold_offset (0), subsense_min_color_dist_threshold = nColorDistThreshold (30),
   * subsense_n_samples = nBGSamples (35), subsense_n_required (2), subsense_desc_dist_threshold_offset = nDescDistThreshold (4). */
  float lbsp_rel_threshold;    /* 0.333 */
  int32_t lbsp_threshold_offset;/* 0 (base-ctor default) */
  int32_t subsense_min_color_dist_threshold; /* 30 */
  int32_t subsense_n_samples;  /* 50 */
  int32_t subsense_n_required; /* 2 */
  int32_t subsense_samples_for_moving_avgs; /* 100 */

  /* SigmaDelta (package_bgs/bl/SigmaDeltaBGS.cpp) */
  int32_t sd_amp_factor;       /* 1 */
  int32_t sd_min_var;          /* 15 */
  int32_t sd_max_var;          /* 255 */

  int32_t subsense_desc_dist_threshold_offset; /* 3 (BGSSUBSENSE_DEFAULT_DESC_DIST_THRESHOLD_OFFSET) */

  /* cv::BackgroundSubtractorGMG as GMG::process configures it (package_bgs/GMG.cpp:44-45) */
  int32_t gmg_max_features;        /* 64 (compile-time bound of the kernel: <= 64) */
  int32_t gmg_init_frames;         /* 20  GMG.cpp:19, :44 (OpenCV default 120) */
  int32_t gmg_quantization_levels; /* 16 */
  int32_t gmg_smoothing_radius;    /* 7 (cv::medianBlur kernel size; 0 = off) */
  int32_t gmg_update_background_model; /* 1 */
  int32_t dp_sampling_rate;        /* dp/ AdaptiveMedian: 7  DPAdaptiveMedianBGS.cpp:19 */
  double gmg_learning_rate;        /* 0.025 */
  double gmg_background_prior;     /* 0.8 */
  double gmg_decision_threshold;   /* 0.7  GMG.cpp:19, :45 (OpenCV default 0.8) */

  /* package_bgs/dp/ wrappers (DP*BGS.cpp:19 constructors): threshold = LowThreshold (HighThreshold = 2x, the mask that is
   * returned), alpha, gaussians = MaxModes (1..8).  learningFrames of WrenGA / Mean / AdaptiveMedian = learning_frames above
   * (default 30 for those three; it has no effect because the wrappers clear the update mask every frame).
   * DPMeanBGS and DPAdaptiveMedianBGS hold `int threshold` and their params classes narrow it: dp_threshold stands for that int,
   * (int)dp_threshold; Mean wraps it into an unsigned int (a negative one: no foreground), AdaptiveMedian into an unsigned char,
   * twice (130 -> high threshold 4; 256 = 0).  NaN or a value outside int's range: BGS_ERR_UNSUPPORTED from bgs_create. */
  float dp_threshold;   /* Zivkovic 25, Grimson 9, WrenGA 12.25, Mean 2700, AdaptiveMedian 40 */
  float dp_alpha;       /* Zivkovic 0.001, Grimson 0.01, WrenGA 0.005, Mean 1e-6 */
  int32_t dp_gaussians; /* 3 */

  /* KDE (package_bgs/ae/KDE.cpp:19-20, :114-126).  bgs_default_params fills these for BGS_KDE only (zero for every other
   * algorithm).  Like the wrapper, which hands them to its model once, on the first frame, every kde_* field except
   * kde_frames_to_learn and kde_update_model is fixed once the geometry is set: later bgs_set_params values are ignored.
   * kde_frames_to_learn is re-read every frame (loadConfig), kde_update_model too.
   * Limits: sequence_length 3..255, frames_to_learn >= 1, time_window >= 1 with time_window / sequence_length <= 255
   * (BGS_ERR_INVALID otherwise); colour ratios need 3-channel frames (BGS_ERR_UNSUPPORTED for gray with ratios on). */
  int32_t kde_frames_to_learn;  /* 10  framesToLearn: learning frames before the first mask */
  int32_t kde_sequence_length;  /* 50  SequenceLength: samples per pixel */
  int32_t kde_time_window;      /* 100 TimeWindowSize: samples are drawn from this many frames */
  int32_t kde_sd_estimation;    /* 1   SDEstimationFlag: per-pixel kernel bandwidth (0: every bin 1) */
  int32_t kde_color_ratios;     /* 1   lUseColorRatiosFlag: compare in (brightness, g/s, r/s) */
  int32_t kde_update_model;     /* 1   NPBGSubtractor::UpdateBGFlag (never initialised by the reference) */
  double kde_threshold;         /* 10e-8 th: probability threshold */
  double kde_alpha;             /* 0.3   alpha: brightness band of the colour-ratio gate */

  /* DPPratiMediodBGS (package_bgs/dp/DPPratiMediodBGS.cpp:19, :83-107).  bgs_default_params fills these for
   * BGS_DP_PRATI_MEDIOD only (zero for every other algorithm); it also sets dp_threshold = 30 (LowThreshold, truncated to an
   * integer; the returned mask uses HighThreshold = 2 x LowThreshold) and dp_sampling_rate = 5.  Like the wrapper, which copies
   * them into its model once, on the first frame, all four are fixed once the geometry is set.
   * Refused (BGS_ERR_UNSUPPORTED): dp_sampling_rate 0, dp_history_size outside 1..BGS_PRATI_MAX_HISTORY, a negative
   * dp_threshold (the reference's unsigned int wraps it), 1-channel frames.  BGS_DP_TEXTURE has no run-time parameters. */
  int32_t dp_history_size;      /* 16  historySize: samples in the circular buffer */
  int32_t dp_weight;            /* 5   weight: stored and saved by the reference, never read */

  /* package_bgs/lb/ wrappers (LB*.cpp:19-20 constructors).  bgs_default_params fills these for the five BGS_LB_* ids only (zero for
   * every other algorithm).  Each is the wrapper's 0..255 integer; the wrappers re-read their XML and call setBGModelParameter
   * with it on EVERY frame, so all seven are live through bgs_set_params.  The engine maps them to the model's doubles on the
   * host, in the reference's order of operations (value / 255.0, then squared / cubed / 100 x / 255^2 v^4 / over Wmax).
   *                                     SimpleGaussian FuzzyGaussian MixtureOfGaussians AdaptiveSOM FuzzyAdaptiveSOM
   *   lb_sensitivity                         66             72             81              75            90
   *   lb_bg_threshold                         -            162             83               -             -
   *   lb_learning_rate                       18             49             59              62            38
   *   lb_noise_variance                     162            195            206               -             -
   *   lb_training_sensitivity                 -              -              -             245           240
   *   lb_training_learning_rate               -              -              -             255           255
   *   lb_training_steps                       -              -              -              55            81
   * Refused (BGS_ERR_UNSUPPORTED): any value outside 0..255, 1-channel frames, lb_noise_variance 0 (Gaussians,
   * MoG), lb_bg_threshold 255 (MoG), lb_training_steps 0 (SOMs). */
  int32_t lb_sensitivity;
  int32_t lb_bg_threshold;
  int32_t lb_learning_rate;
  int32_t lb_noise_variance;
  int32_t lb_training_sensitivity;
  int32_t lb_training_learning_rate;
  int32_t lb_training_steps;

  /* VuMeter (package_bgs/av/VuMeter.cpp:19, :103-116).  bgs_default_params fills these for BGS_VUMETER only (zero for every other
   * algorithm).  The wrapper hands binSize, alpha and threshold to its model once, on the first frame, through setters that REPLACE
   * an out-of-range value instead of failing (binSize outside 1..254 -> 8, alpha / threshold outside (0,1) -> 0.995 / 0.03,
   * TBackgroundVuMeter.h:47-54); the engine applies the same rules and keeps the three once the geometry is set.  vu_enable_filter
   * (cv::erode 3x3 then cv::medianBlur 5 of the mask) is re-read every frame.  Mask and background image (1 channel: the gray
   * background) are valid from frame 1; the mask of a stream's first four frames is zero.  1-channel frames: BGS_ERR_UNSUPPORTED. */
  int32_t vu_bin_size;        /* 8     binSize: gray levels per histogram bin (binCount = 256 / binSize) */
  int32_t vu_enable_filter;   /* 1     enableFilter */
  double vu_alpha;            /* 0.995 alpha: every bin is scaled by it every frame */
  double vu_threshold;        /* 0.03  threshold: a pixel whose bin is below it is foreground */
} bgs_params;

/* FuzzySugenoIntegral / FuzzyChoquetIntegral (package_bgs/tb/Fuzzy*Integral.cpp:20-21, :191-205).  A struct of its own: bgs_params does
 * not grow any more (see THE ID SPACE).  bgs_create gives a fuzzy engine these defaults whatever bgs_params it was handed;
 * bgs_set_fuzzy_params may be called between any two frames and acts from the next frame on, as the wrapper's per-frame loadConfig
 * does: all seven values are live.  A stream learns while its own frame counter is <= frames_to_learn (frames_to_learn + 1 frames:
 * no mask, no background image, out_flags 0), then detects: mask (0 / 255) and the 3-channel background image, both valid.
 * Refused with BGS_ERR_UNSUPPORTED: color_space 2 (Ohta: a pixel with R == B gives -inf and a NaN background on the first detecting
 * frame), 3 and 4 (OpenCV's float cvCvtColor), option outside {1,2} (the reference's integral image is uninitialised then),
 * 1-channel frames, frames narrower or lower than 2 pixels; BGS_ERR_INVALID: frames_to_learn < 0. */
typedef struct bgs_fuzzy_params {
  uint32_t struct_size;     /* sizeof(bgs_fuzzy_params) */
  int32_t frames_to_learn;  /* 10   framesToLearn */
  double alpha_learn;       /* 0.1  alphaLearn: bg = alphaLearn * in + (1 - alphaLearn) * bg while learning */
  double alpha_update;      /* 0.01 alphaUpdate */
  int32_t color_space;      /* 1    colorSpace: 1 = RGB (the only one built) */
  int32_t option;           /* 2    1: three colour components, 2: texture + two colour components */
  int32_t smooth;           /* 1    smooth: medianBlur 3 of the integral image */
  int32_t reserved_;        /* 0 */
  double threshold;         /* 0.67 threshold */
} bgs_fuzzy_params;

/* T2FGMM_UM / T2FGMM_UV (package_bgs/tb/T2FGMM_UM.cpp:19, :99-111), in the wrapper's member types.  A struct of its own, as
 * bgs_fuzzy_params.  bgs_create gives a T2FGMM engine these defaults whatever bgs_params it was handed.  The wrapper hands the values
 * to its model object once, on the first frame: they are taken when the geometry is set, and a bgs_set_t2f_params after that
 * succeeds and leaves the values in force unchanged (bgs_get_t2f_params returns what is in force).  threshold and alpha are narrowed
 * to float on the way, as T2FGMMParams' accessors do; the high threshold is 2 * (float)threshold.
 * Refused with BGS_ERR_UNSUPPORTED, the class named: gaussians outside 1..5, a parameter that is not finite as a float, alpha
 * outside [0, 1) as a float (the reference's sort keys become NaN there and its mode order is qsort's accident), kv == 0 for
 * T2FGMM_UV, 1-channel frames. */
typedef struct bgs_t2f_params {
  uint32_t struct_size;  /* sizeof(bgs_t2f_params) = 40 */
  double threshold;      /* 9.0  threshold */
  double alpha;          /* 0.01 alpha */
  float km;              /* 1.5  km: T2FGMM_UM's factor */
  float kv;              /* 0.6  kv: T2FGMM_UV's factor */
  int32_t gaussians;     /* 3    gaussians: modes per pixel, 1..5 */
} bgs_t2f_params;

/* DPEigenbackgroundBGS (package_bgs/dp/DPEigenbackgroundBGS.cpp:19, :96-106), in the wrapper's member types.  A struct of its own, as
 * bgs_t2f_params.  bgs_create gives an Eigenbackground engine these defaults whatever bgs_params it was handed.  The wrapper fills its
 * params object once, on the first frame: the values are taken when the geometry is set, and a bgs_set_eigen_params after that
 * succeeds and leaves the values in force unchanged (bgs_get_eigen_params returns what is in force).  threshold is narrowed to float
 * on the way (LowThreshold() is a float&); the high threshold, the one the returned mask uses, is 2 * (float)threshold.
 * Refused with BGS_ERR_UNSUPPORTED, the class named: history_size outside 2..BGS_EIGEN_MAX_HISTORY, embedded_dim outside
 * 1..history_size - 1 (centred data has rank <= history_size - 1: at embedded_dim == history_size the reference projects onto a
 * normalised rounding residue, above it OpenCV asserts), 1-channel frames, the class inside a bgs_group. */
typedef struct bgs_eigen_params {
  uint32_t struct_size;  /* sizeof(bgs_eigen_params) = 16 */
  int32_t threshold;     /* 225 threshold */
  int32_t history_size;  /* 20  historySize: frames 0 .. historySize-1 are the PCA's samples */
  int32_t embedded_dim;  /* 10  embeddedDim: eigenvectors kept */
} bgs_eigen_params;

/* Largest history_size the Eigenbackground kernels are built for. */
#define BGS_EIGEN_MAX_HISTORY 32

/* IndependentMultimodalBGS (package_bgs/db/imbs.hpp:43-56): the full constructor's arguments, each in the type of the member it
 * lands in (samplingPeriod and persistencePeriod are unsigned int members, alpha and beta float, tau_s and tau_h uchar).  A struct
 * of its own, as bgs_eigen_params.  bgs_create gives an IMBS engine these defaults whatever bgs_params it was handed.  The model
 * sizes its arrays at its first frame: the values are taken when the geometry is set, and a bgs_set_imbs_params after that succeeds
 * and leaves the values in force unchanged (bgs_get_imbs_params returns what is in force).
 * Refused with BGS_ERR_UNSUPPORTED, the class named: fps <= 0 or not finite (0 means wall-clock time), minBinHeight 0, numSamples
 * outside 2..BGS_IMBS_MAX_SAMPLES, minBinHeight above numSamples (maxBgBins = numSamples / minBinHeight would be 0), tau_s /
 * tau_h outside 0..255, non-finite alpha / beta / minArea, 1-channel frames, the class inside a bgs_group.
 * Until the first model is built (bgModel[0].isValid[0]) the reference hands out a putText banner; the engine hands out what that
 * is with putText a no-op, an all-zero mask and background, both reported valid. */
typedef struct bgs_imbs_params {
  uint32_t struct_size;           /* sizeof(bgs_imbs_params) = 64 */
  uint32_t fgThreshold;           /* 15 */
  double fps;                     /* 10, as the wrapper passes: timestamp += 1000./fps per frame */
  uint32_t associationThreshold;  /* 5 */
  uint32_t samplingPeriod;        /* 500 ms */
  uint32_t minBinHeight;          /* 2 */
  uint32_t numSamples;            /* 30 */
  float alpha;                    /* 0.65 */
  float beta;                     /* 1.15 */
  int32_t tau_s;                  /* 60, 0..255 */
  int32_t tau_h;                  /* 40, 0..255 */
  double minArea;                 /* 30 */
  uint32_t persistencePeriod;     /* 10000 ms */
  int32_t morphologicalFiltering; /* 0 */
} bgs_imbs_params;

/* MultiLayerBGS (package_bgs/jmo/MultiLayerBGS.cpp:110-186, :292-331): the wrapper's parameters, each in the type of the member it
 * lands in.  A struct of its own, as bgs_imbs_params.  bgs_create gives a MultiLayerBGS engine the wrapper's loadDefaultParams
 * values whatever bgs_params it was handed.  The wrapper hands its values to the model at its first frame only: they are taken when
 * the geometry is set, and a bgs_set_multilayer_params after that succeeds and leaves the values in force unchanged.
 * status 0 = MLBGS_LEARN, 1 = MLBGS_DETECT; disable_detect_mode forces LEARN; at frame detect_after (> 0) the hard-coded DETECT values
 * 0.01 / 0.01 / 0.001 are installed, not the detect_* ones, and disable_learning applies.  The bilateral sigmas
 * of the reference's XML are no fields: LINUX_BILATERAL_FILTER is compiled out.  A model preload is not offered.
 * Refused with BGS_ERR_UNSUPPORTED, the class named: max_mode_num outside 1..5, pattern_neig_half_size above
 * BGS_MULTILAYER_MAX_HALF_SIZE, pattern_neig_gaus_sigma <= 0 while the half size is >= 0 (a negative half size means no
 * smoothing), non-finite values, frames that are not 3-channel, the class inside a bgs_group.  texture_weight <= 0 is accepted: LBP is
 * skipped and the patterns read as zero. */
typedef struct bgs_multilayer_params {
  uint32_t struct_size;                       /* sizeof(bgs_multilayer_params) = 96 */
  int32_t max_mode_num;                       /* 5 */
  float weight_updating_constant;             /* 5.0 */
  float texture_weight;                       /* 0.5 */
  float bg_mode_percent;                      /* 0.6 */
  int32_t pattern_neig_half_size;             /* 4 */
  float pattern_neig_gaus_sigma;              /* 3.0 */
  float bg_prob_threshold;                    /* 0.2 */
  float bg_prob_updating_threshold;           /* 0.2 */
  int32_t robust_LBP_constant;                /* 3 */
  float min_noised_angle;                     /* (float)(10.0 / 180.0 * PI), PI the float macro */
  float shadow_rate;                          /* 0.6 */
  float highlight_rate;                       /* 1.2 */
  float frame_duration;                       /* 0.1 */
  float learn_mode_learn_rate_per_second;     /* 0.5 */
  float learn_weight_learn_rate_per_second;   /* 0.5 */
  float learn_init_mode_weight;               /* 0.05 */
  float detect_mode_learn_rate_per_second;    /* 0.01 */
  float detect_weight_learn_rate_per_second;  /* 0.01 */
  float detect_init_mode_weight;              /* 0.001 */
  int32_t status;                             /* 0 */
  int32_t disable_detect_mode;                /* 1 */
  int32_t disable_learning;                   /* 0 */
  int32_t detect_after;                       /* 0 */
} bgs_multilayer_params;

/* Largest pattern_neig_half_size the MultiLayerBGS smoothing kernel is built for (a 17 x 17 Gaussian). */
#define BGS_MULTILAYER_MAX_HALF_SIZE 8

/* Largest numSamples the IMBS kernels are built for (bin heights and counters are packed into 6 bits). */
#define BGS_IMBS_MAX_SAMPLES 63

/* Largest dp_history_size the PratiMediod kernel is built for (every dist entry then fits in 16 bits: 64 x 255 < 65536). */
#define BGS_PRATI_MAX_HISTORY 64

int bgs_abi_version(void);

/* Fill *p (struct_size must be set) with the reference defaults for `algo`. */
int bgs_default_params(bgs_algo algo, bgs_params* p);

/* Create an engine for `n_streams` independent streams on HIP device `hip_device`.
 * params == NULL selects the reference defaults.  Model memory is allocated
 * lazily at the first frame (like every reference class) or by bgs_set_geometry. */
int bgs_create(bgs_algo algo, const bgs_params* params, int hip_device, int n_streams, bgs_engine** out);

/* Replace the wrapper-level parameters between frames.  The reference re-reads
 * ./config/<Class>.xml at the top of every process() (e.g. MixtureOfGaussianV2BGS.cpp:34),
 * so thresholds / alpha may change mid-stream; structural fields (nmixtures, n_samples)
 * must stay what they were at bgs_create. */
int bgs_set_params(bgs_engine* e, const bgs_params* params);

/* The fuzzy-integral classes' own parameters (bgs_fuzzy_params above); BGS_ERR_INVALID for an engine of any other class. */
int bgs_fuzzy_default_params(bgs_fuzzy_params* p);
int bgs_set_fuzzy_params(bgs_engine* e, const bgs_fuzzy_params* p);
int bgs_get_fuzzy_params(const bgs_engine* e, bgs_fuzzy_params* p);
/* Every refusal of the two classes without an engine and without a device: parameters (p == NULL: the defaults) and, where rows > 0,
 * the frame geometry.  bgs_set_fuzzy_params and bgs_set_geometry run the same checks.  The message names the class. */
int bgs_fuzzy_check(bgs_algo algo, const bgs_fuzzy_params* p, int rows, int cols, int channels);

/* The T2FGMM classes' own parameters (bgs_t2f_params above); BGS_ERR_INVALID for an engine of any other class. */
int bgs_t2f_default_params(bgs_t2f_params* p);
int bgs_set_t2f_params(bgs_engine* e, const bgs_t2f_params* p);
int bgs_get_t2f_params(const bgs_engine* e, bgs_t2f_params* p);
/* Every refusal of the two classes without an engine and without a device: parameters (p == NULL: the defaults) and, where rows > 0,
 * the frame geometry.  The message names the class. */
int bgs_t2f_check(bgs_algo algo, const bgs_t2f_params* p, int rows, int cols, int channels);

/* DPEigenbackground's own parameters (bgs_eigen_params above); BGS_ERR_INVALID for an engine of any other class. */
int bgs_eigen_default_params(bgs_eigen_params* p);
int bgs_set_eigen_params(bgs_engine* e, const bgs_eigen_params* p);
int bgs_get_eigen_params(const bgs_engine* e, bgs_eigen_params* p);
/* Every refusal of the class without an engine and without a device: parameters (p == NULL: the defaults) and, where rows > 0, the
 * frame geometry.  The message names the class. */
int bgs_eigen_check(const bgs_eigen_params* p, int rows, int cols, int channels);

/* IndependentMultimodalBGS's own parameters (bgs_imbs_params above); BGS_ERR_INVALID for an engine of any other class. */
int bgs_imbs_default_params(bgs_imbs_params* p);
int bgs_set_imbs_params(bgs_engine* e, const bgs_imbs_params* p);
int bgs_get_imbs_params(const bgs_engine* e, bgs_imbs_params* p);
/* Every refusal of the class without an engine and without a device: parameters (p == NULL: the defaults) and, where rows > 0, the
 * frame geometry.  The message names the class. */
int bgs_imbs_check(const bgs_imbs_params* p, int rows, int cols, int channels);

/* MultiLayerBGS's own parameters (bgs_multilayer_params above); BGS_ERR_INVALID for an engine of any other class. */
int bgs_multilayer_default_params(bgs_multilayer_params* p);
int bgs_set_multilayer_params(bgs_engine* e, const bgs_multilayer_params* p);
int bgs_get_multilayer_params(const bgs_engine* e, bgs_multilayer_params* p);
/* Every refusal of the class without an engine and without a device: parameters (p == NULL: the defaults) and, where rows > 0, the
 * frame geometry.  The message names the class. */
int bgs_multilayer_check(const bgs_multilayer_params* p, int rows, int cols, int channels);
/* The two constants the host computes for the kernels, as float bits, without a device: bits[0] = the constructor's sinf(3 degrees)
 * (m_fMinNoisedAngleSine, never recomputed), bits[1] = min_noised_angle of p (NULL: the defaults). */
int bgs_multilayer_constants(const bgs_multilayer_params* p, uint32_t bits[2]);

/* Engine options.
 *   BGS_OPT_BORROW_FRAMES  device path of the history-keeping classes (FrameDifference, WeightedMovingMean/Variance):
 *                          1 = use the caller's previous d_frames buffers as history instead of copying each frame
 *                          into the engine's ring; the buffers handed to the previous one (FD) or two (WMM/WMV)
 *                          whole-batch calls must then stay valid and unchanged.  Default 0 (private copy).
 *   BGS_OPT_MOG2_PIXELS_PER_LANE, BGS_OPT_MOG2_TILED  round-2 A/B knobs of the sorted-array MOG2 kernel; accepted and ignored since
 *                          round 3 (one pixel per lane, one model layout: ranked weights + fixed-slot records + summaries).
 *   BGS_OPT_XCD_SWIZZLE    XCD-aware workgroup order: 1 (default) = for the kernels that stream a multi-plane model
 *                          (MOG2, MOG1, dp/), 2 = also for the byte-stream kernels (slower there: A/B only), 0 = off.
 *   BGS_OPT_PLACEMENT_PROBE  rounds 1-2 looked for a fast physical placement of a multi-GB model by trial; accepted and ignored since
 *                          round 3, which places models deterministically (BGS_OPT_MODEL_CHUNK_MB).
 *   BGS_OPT_MODEL_CHUNK_MB multi-GB models (MOG2, MOG1, dp/) are ONE virtual range backed by separately created physical chunks of this
 *                          many MiB (default 256; any size from 2 MiB to 1 GiB avoids the slow placement - a physically contiguous run
 *                          above ~1 GiB - that one big hipMalloc of a long-lived process sometimes gets: 8-10 % on the MOG2 kernel; it is
 *                          not faster than a fresh plain allocation); 0 = one plain allocation; before the geometry is set. */
#define BGS_OPT_BORROW_FRAMES 1
#define BGS_OPT_MOG2_PIXELS_PER_LANE 2
#define BGS_OPT_MOG2_TILED 3
#define BGS_OPT_XCD_SWIZZLE 4
#define BGS_OPT_PLACEMENT_PROBE 5
#define BGS_OPT_MOG2_SPARSE 6   /* which MOG2 per-frame kernel runs (identical results, different traffic): 0 dense (everything read and
                                   written back: A/B, placement probe); 1 eager (every record read, only what changed written); 2 count
                                   (only the modes a pixel has are read); 4 filter (4-byte summaries first, then only the records they
                                   cannot rule out); 3 (default) automatic, from what sampled workgroups count */
#define BGS_OPT_CLIP_FUSE 7     /* 1 (default): bgs_process_clip_device runs 8 / 4 / 2 consecutive frames of a mixture model or of a
                                   package_bgs/lb model per launch with the model held in registers; 0: one launch per frame.  Identical
                                   results, only speed differs. */
#define BGS_OPT_MODEL_CHUNK_MB 9
#define BGS_OPT_MODEL_CHUNK_MIN_MB 10 /* models smaller than this many MiB take one plain allocation (default 768: below that a good part of the
                                   model sits in the 256 MiB Infinity Cache and placement does not matter); before the geometry is set.
                                   Lowered by the test that exercises the chunked construction and its release on a small model. */
#define BGS_OPT_HOST_REGISTER 8 /* bgs_process (host buffers): bit 0 input frame, bit 1 mask, bit 2 background image.  A buffer passed in an
                                   enabled role that comes back with the same address and size as in the previous call is page-locked once
                                   (hipHostRegister) and from then on read / written by the DMA engine in place - no staging copy by the
                                   CPU (OpenCV's capture loop hands IBGS::process the same frame buffer every frame, VideoCapture.cpp:158-218).
                                   Contract: such a buffer stays allocated until a different one is passed in that role or the engine is
                                   destroyed (the engine cannot see a buffer being freed and another mapped at the same address).
                                   Default 0: every image is staged through the engine's own pinned buffers.  Rows must be contiguous. */
int bgs_set_option(bgs_engine* e, int option, int64_t value);

/* Fix rows x cols x channels up front and allocate the model (device path). */
int bgs_set_geometry(bgs_engine* e, int rows, int cols, int channels);

/*
 * One frame of one stream, host buffers (the IBGS::process call).
 *   in       rows x cols x channels uint8, interleaved (BGR), row stride in_step bytes (>= cols*channels)
 *   fg       rows x cols uint8 mask or NULL; written only if BGS_FG_VALID is reported
 *   bg       rows x cols x channels (ASBL, VuMeter: x1) uint8 or NULL; written only if BGS_BG_VALID
 * in == NULL or rows*cols == 0 is the reference's `if(img_input.empty()) return;`:
 * returns BGS_OK with *out_flags = 0 and no state change.
 * Synchronous: the outputs are complete on return.
 */
int bgs_process(bgs_engine* e, int stream, const uint8_t* in, int rows, int cols, int channels, size_t in_step,
                uint8_t* fg, size_t fg_step, uint8_t* bg, size_t bg_step, uint32_t* out_flags);

/*
 * One frame of EVERY stream, device buffers, asynchronous on `hip_stream`
 * (a hipStream_t passed as void*; NULL = the default stream).  This is the
 * roofline path: no PCIe traffic, one launch over streams x pixels.
 *   d_frames  [n_streams][rows][cols][channels] uint8, contiguous
 *   d_fg      [n_streams][rows][cols] uint8 or NULL
 *   d_bg      [n_streams][rows][cols][channels] uint8 or NULL (ASBL, VuMeter: one channel)
 *   d_fg_bits [n_streams][W] uint64, W = ceil(rows*cols/64): bit i of word j of a stream = its pixel 64j+i is foreground; the bits of
 *             a stream's last word past pixel rows*cols-1 are zero; or NULL.  (rows*cols a multiple of 64 - 1080p, 4K, 720p, VGA,
 *             320x176 ... - is the fast case: the update kernels write the words from wave ballots; for any other size the words are
 *             made from the byte mask by one extra small launch, through an engine-owned buffer when d_fg is NULL.)
 * The streams need NOT be in lock-step: cameras join, drop frames and are reset independently (the reference creates and deletes
 * one IBGS object per stream whenever it likes, FrameProcessor.cpp:35-155, :342-482).  Streams whose next frame needs the same
 * kernel arguments share a launch - for the mixture models that is "first frame or not" plus the learning rate, i.e. every
 * stream past its first frame under the wrappers' fixed alpha; for the history classes the warm-up level; for SuBSENSE / LOBSTER
 * the frame index itself - so a batch fed by whole-batch calls is ONE launch, and a straggler costs one more.
 * out_flags: what holds for every stream of the call; per stream see bgs_stream_flags.
 * (BGS_OPT_BORROW_FRAMES still needs lock-step: the borrowed history is one buffer for the whole batch.)
 */
int bgs_process_batch_device(bgs_engine* e, const void* d_frames, void* d_fg, void* d_bg, void* d_fg_bits,
                             void* hip_stream, uint32_t* out_flags);

/* Same, restricted to streams [first, first+count): d_* point at the first of `count` images. */
int bgs_process_range_device(bgs_engine* e, int first, int count, const void* d_frames, void* d_fg, void* d_bg,
                             void* d_fg_bits, void* hip_stream, uint32_t* out_flags);

/*
 * A CLIP: `nframes` consecutive frames of each stream in [first, first+count) in one call - the file-fed case of the reference
 * (VideoCapture::start reads a video file, VideoCapture.cpp:158-207: frames are available ahead of the model), or a live
 * deployment that accepts nframes-1 frame times of latency.  Results are exactly those of nframes successive
 * bgs_process_range_device calls (masks, backgrounds, model state, frame counts).
 *   d_frames  [nframes][count][rows][cols][channels]   frame t of all streams, then frame t+1 ...
 *   d_fg      [nframes][count][rows][cols] or NULL;  d_bg [nframes][count][rows][cols][channels] or NULL
 *   d_fg_bits [nframes][count][ceil(rows*cols/64)] or NULL;  out_flags: nframes words or NULL
 * The mixture models (MixtureOfGaussianV2BGS, MixtureOfGaussianV1BGS, DPZivkovicAGMMBGS, DPGrimsonGMMBGS) and the five
 * package_bgs/lb classes (LBSimpleGaussian, LBFuzzyGaussian, LBMixtureOfGaussians, LBAdaptiveSOM, LBFuzzyAdaptiveSOM) take runs of 8 / 4 / 2
 * frames through ONE launch that loads each pixel's model once, applies the frames in order in registers and writes the model back
 * once (model traffic per frame / 8, / 4, / 2); FrameDifference / WeightedMovingMean / WeightedMovingVariance take their frame history
 * from the clip itself instead of copying every frame into the engine's ring; every other class runs the same launches as the
 * frame-by-frame calls.
 */
int bgs_process_clip_device(bgs_engine* e, int first, int count, int nframes, const void* d_frames, void* d_fg, void* d_bg,
                            void* d_fg_bits, void* hip_stream, uint32_t* out_flags);

/*
 * Copy one model plane of one stream to host memory, as a dense array in the
 * canonical order documented in DESIGN.md §3 (e.g. MOG2: "w" float[K][N],
 * "var" float[K][N], "mu" float[K][C][N], "nmodes" uint8[N]).  Returns the
 * number of bytes written (>= 0) or a negative status.  Parity tests only.
 */
int64_t bgs_get_state(bgs_engine* e, int stream, const char* plane, void* dst, size_t cap);

/* Number of frames stream `stream` has consumed so far (since bgs_create or its last bgs_reset_stream). */
int64_t bgs_frames_seen(const bgs_engine* e, int stream);

/*
 * GROUPS - several classes on the same frames.  FrameProcessor::process hands ONE pre-processed frame to every enabled IBGS, one
 * call after the other (FrameProcessor.cpp:169-340); BASELINE configs[2] is WeightedMovingVarianceBGS + AdaptiveBackgroundLearning
 * on the same 3840x2160 frames.  A group takes `n_algos` classes; the byte-stream ones among them - FrameDifference,
 * StaticFrameDifference, WeightedMovingMean, WeightedMovingVariance, AdaptiveBackgroundLearning, SigmaDelta, one instance each -
 * run as ONE kernel over one read of the frame and one shared history ring (17 B/pixel for configs[2] instead of 10 + 10; 26
 * instead of 47 for the five history / state classes together), every other class as a member engine fed the same device frame.
 * Masks, backgrounds, warm-up conventions and model states are those of n separate engines, bit for bit.
 *   params      NULL, or n_algos pointers (NULL entries = reference defaults)
 *   d_fg, d_bg  arrays of n_algos device pointers (entries may be NULL), each laid out as for bgs_process_batch_device
 *   out_flags   n_algos words (BGS_FG_VALID / BGS_BG_VALID per class)
 * The streams of a group advance in lock-step (whole-batch calls).  bgs_group_process is the host-buffer call for single-stream
 * groups - one upload of the frame for all classes - with per-class output pointers and row steps (NULL steps = packed rows).
 */
typedef struct bgs_group bgs_group;
int bgs_group_create(const bgs_algo* algos, const bgs_params* const* params, int n_algos, int hip_device, int n_streams, bgs_group** out);
void bgs_group_destroy(bgs_group* g);
int bgs_group_size(const bgs_group* g);
int bgs_group_is_fused(const bgs_group* g, int index); /* 1: class `index` runs inside the fused kernel; 0: member engine */
int bgs_group_set_params(bgs_group* g, int index, const bgs_params* params);
int bgs_group_set_option(bgs_group* g, int option, int64_t value); /* BGS_OPT_BORROW_FRAMES: the shared history too */
int bgs_group_set_geometry(bgs_group* g, int rows, int cols, int channels);
int bgs_group_process_batch_device(bgs_group* g, const void* d_frames, void* const* d_fg, void* const* d_bg, void* hip_stream, uint32_t* out_flags);
int bgs_group_process(bgs_group* g, const uint8_t* in, int rows, int cols, int channels, size_t in_step, uint8_t* const* fg, const size_t* fg_step,
                      uint8_t* const* bg, const size_t* bg_step, uint32_t* out_flags);
int64_t bgs_group_get_state(bgs_group* g, int index, int stream, const char* plane, void* dst, size_t cap);
int64_t bgs_group_frames_seen(const bgs_group* g);
int bgs_group_enable_kernel_timing(bgs_group* g, int on);
int bgs_group_kernel_timing(bgs_group* g, double* avg_ms, int64_t* launches); /* the fused launches, HIP events on the launch stream */

/*
 * Several cameras on the host path.  bgs_submit queues one frame of one stream - upload, kernels, download - on that stream's own
 * lane (HIP stream, pinned staging, device images) and returns; bgs_wait blocks until that submission is done and the outputs are
 * in the caller's images (out_flags as for bgs_process).  Submissions of different streams overlap: while camera A's frame is on
 * the bus camera B's kernel runs and camera C's mask comes back, where a synchronous bgs_process per camera takes turns.
 * Same arguments and results as bgs_process; the caller's buffers must stay valid and untouched until bgs_wait; one submission per
 * stream in flight (bgs_process on such a stream collects it first; the device-path calls - bgs_process_batch_device / _range_device /
 * _clip_device - REFUSE a range that covers a stream with a submission in flight, BGS_ERR_STATE: they run on the caller's HIP stream
 * and would race with the lane).  All bgs_submit / bgs_wait calls of one engine come from ONE host thread (an engine is not thread-safe,
 * like an IBGS instance).  Frames prepared by bgs_set_ingest go through bgs_process.
 */
int bgs_submit(bgs_engine* e, int stream, const uint8_t* in, int rows, int cols, int channels, size_t in_step, uint8_t* fg, size_t fg_step,
               uint8_t* bg, size_t bg_step);
int bgs_wait(bgs_engine* e, int stream, uint32_t* out_flags);

/* A caller that keeps the images of ALL its cameras in one allocation (a capture ring, a frame pool) registers that allocation once:
 * [ptr, ptr + bytes) is page-locked as a whole (one hipHostRegister instead of one per camera and role) and from then on every input
 * frame, mask or background image of bgs_process / bgs_submit that lies inside it with contiguous rows is read / written by the DMA
 * engine in place - whatever BGS_OPT_HOST_REGISTER says, and without the "same buffer as last call" test.  on = 0 drops the
 * registration (same ptr).  The arena stays allocated until then or until bgs_destroy. */
int bgs_host_arena(bgs_engine* e, void* ptr, size_t bytes, int on);

/* One camera of the batch starts over - what `delete bgs; bgs = new <Class>;` is for one stream in the reference
 * (FrameProcessor.cpp:342-482 / :35-155, ustc_src/ustc_bgs.cpp:75-77): its frame count returns to 0 and its NEXT frame, on the
 * HIP stream of that call and in order with everything queued before it, re-initialises its model and restarts its warm-up
 * exactly like a first frame.  No launch happens here; the other streams are not touched. */
int bgs_reset_stream(bgs_engine* e, int stream);

/* out_flags (BGS_FG_VALID / BGS_BG_VALID) of the stream's last frame: in a call over streams of different ages the call's own
 * out_flags word only holds what is true of all of them. */
int bgs_stream_flags(const bgs_engine* e, int stream, uint32_t* out_flags);

/* Average duration in ms of the dominant kernel of this engine since the last reset, measured
 * with HIP events on the launch stream when timing is enabled (bench.py's roofline leg). */
int bgs_enable_kernel_timing(bgs_engine* e, int on);
int bgs_kernel_timing(bgs_engine* e, double* avg_ms, int64_t* launches, const char** kernel_name);
/* The same measurement launch by launch: copies the durations (ms) of the first min(cap, launches) timed launches since the
 * last reset into ms[] and returns how many were written (negative = error).  bench.py commits the series behind its
 * burst / sustained figures from this (profiles/rNN_mog2_launch_series.csv). */
int64_t bgs_kernel_timing_series(bgs_engine* e, float* ms, int64_t cap);

/*
 * Measurement aids: what THIS box delivers, measured by the library in the process that benchmarks it (bench.py `calibration`,
 * `host_path`).  Boxes of one pool differ by several percent, and so does the physical placement of a multi-GB allocation; a figure
 * that is to be compared across boxes needs the box's own yardstick beside it.
 *   bgs_calibrate_copy  float4 copy kernel over `bytes` bytes (bytes/2 read + bytes/2 written per launch; mean of `iters` launches after
 *                       two warm-ups, HIP events): through ONE plain hipMalloc (chunk_mb = 0) or through one virtual range backed by
 *                       physical chunks of chunk_mb MiB - the construction the big models use (BGS_OPT_MODEL_CHUNK_MB).  *gbps in GB/s.
 *   bgs_calibrate_pcie  `iters` copies of `bytes` bytes each way between the device and page-locked host memory: hipHostMalloc
 *                       (registered = 0: the engine's own staging) or ordinary memory page-locked in place with hipHostRegister
 *                       (registered = 1: a caller buffer under BGS_OPT_HOST_REGISTER; *register_ms = what that call took).
 * bgs_get_state(e, 0, "hostpath", double[15]) returns an engine's host-path counters since creation: buffers currently page-locked in
 * place per role [0..2] (input, mask, background) and refused per role [3..5], hipHostRegister calls [6] and their total ms [7],
 * hipHostUnregister calls [8], frames [9], bytes host-to-device [10] and device-to-host [11], CPU ms spent copying into [12] and out
 * of [13] pinned staging, arenas registered [14].
 */
int bgs_calibrate_copy(int hip_device, size_t bytes, int chunk_mb, int iters, double* gbps);
int bgs_calibrate_pcie(int hip_device, size_t bytes, int registered, int iters, double* h2d_gbps, double* d2h_gbps, double* register_ms);

void bgs_destroy(bgs_engine* e);

/* Thread-local text of the last failure on this thread ("" if none). */
const char* bgs_last_error(void);

/* ---- stand-alone device primitives (rows §8a10, §8f N1) ------------------------------ */

/* State planes of the dp/ models (bgs_get_state): "modes" f32 [K*F][n] with F = 5 (sigma, mu0, mu1, mu2, weight) for
 * Zivkovic and 6 (variance, mu0, mu1, mu2, weight, significants) for Grimson, plane index k*F + f; "nmodes" u8 [n];
 * WrenGA "gauss" f32 [4][n] (mu0..2, var); Mean "mean" f32 [3][n]; AdaptiveMedian "median" u8 [n*3].
 * PratiMediod: "samples" u8 [historySize][n][3] in slot order (slots not yet filled hold 0), "dist" u16 [historySize][n] (the
 * L-inf sums, 0 for slots not yet filled), "median" u8 [n][3] (the medoid of the last sampled frame; 0 before the first);
 * bgs_get_state also answers "count" int64 [2] = {samples in the buffer, next slot to replace}.
 * Texture: "hist" u8 [n][3][64], the background histograms in the reference's r, g, b order (TextureHistogram); pixels outside
 * the processed interior (7 <= x < cols-7, 7 <= y < rows-7) hold 0.
 * Eigenbackground (H = history_size, M = embedded_dim): "history" u8 [H][n][3] (slots not yet filled read 0), "count" int64 [1] =
 * the stream's frame counter; once the model is built (after frame H): "avg" f32 [n][3], "eigenvalues" f64 [H] of the centred Gram
 * matrix, descending, "eigenvectors" f32 [M][n][3], "coeff" f32 [M] = the last frame's projection, "result" f32 [n][3] = that
 * frame's reconstruction (not stored per frame: recomputed on request from avg, coeff and the eigenvectors by a launch of its own).
 * IMBS (N = numSamples, M = maxBgBins = numSamples / minBinHeight), unpacked: "bins" u8 [n][N][5] = binValues B, G, R, binHeights, isFg;
 * "model" u8 [n][M][6] = values B, G, R, isValid, isFg, counter; "persistence" u32 [n]; "control" f64 [10] = timestamp,
 * prev_timestamp, prev_bg_frame_time, bg_frame_counter, numSamples, samplingPeriod, bg_reset, sudden_change, maxBgBins,
 * bgModel[0].isValid[0].  Slots the reference never wrote read 0.
 * MultiLayerBGS, unpacked in the reference's field order: "order" u8 [n][7] = num, bg_num, lbp_idxes[0..5) (entries at and past num read
 * 0); "modes" f32 [n][5][18] = bg_pattern[6], bg_intensity[3], max_intensity[3], min_intensity[3], weight, max_weight, bg_layer_num per
 * physical slot (slots that lbp_idxes[0..num) does not name read 0); "dist" f32 [n] = the last frame's smoothed distance map.
 * lb/ models, all f64 in the reference's memory order, colour fields in the byte order of the input pixel (B, G, R):
 * SimpleGaussian / FuzzyGaussian "mu", "var" f64 [n][3]; MixtureOfGaussians "w" f64 [n][3], "mu", "var" f64 [n][3][3] (pixel, slot,
 * colour), "sortkey" f64 [n][3], "k" int32 [n] (slots >= k read 0); AdaptiveSOM / FuzzyAdaptiveSOM "som" f64 [n][3][3][3] (pixel,
 * neuron row, neuron column, colour), "bg" u8 [n][3], "count" int64 [1] = the stream's training counter m_K.
 * VuMeter: "hist" f32 [binCount][n], the reference's dense histogram planes (whatever the engine keeps internally), "background"
 * u8 [n], "count" int64 [1] = the stream's m_nCount.
 * Fuzzy integrals: "background" f32 [n][3] (BGR), "integral" f32 [n] = the (blurred) integral image of the stream's last detecting
 * frame, "minmax" f32 [2] of that image, "count" int64 [1] = the stream's frameNumber.
 * T2FGMM_UM / T2FGMM_UV: "modes" f32 [gaussians*6][n] in the reference's struct order {variance, muR, muG, muB, weight,
 * significants} (the sixth is recomputed from the stored five for the modes below the pixel's count and reads 0 above it),
 * "nmodes" u8 [n]. */

/* LBSP 16-bit double-cross descriptors of a whole 8UC3 / 8UC1 image (LBSP.h:50-95,
 * LBSP_16bits_dbcross_{3ch3t,1ch}.i).  d_desc: [rows][cols][channels] uint16; the
 * 2-pixel border (LBSP::validateROI, LBSP.cpp:311-318) is written as 0.
 * t_lut: 256 absolute thresholds indexed by the centre value
 * (BackgroundSubtractorSuBSENSE.cpp:209-210, 227-228), host pointer. */
int bgs_lbsp_describe_device(int hip_device, const void* d_img, int rows, int cols, int channels,
                             const uint8_t* t_lut, void* d_desc, void* hip_stream);
/* the same for `images` frames stored back to back ([images][rows][cols][channels]) in one launch */
int bgs_lbsp_describe_batch_device(int hip_device, const void* d_img, int images, int rows, int cols, int channels,
                                   const uint8_t* t_lut, void* d_desc, void* hip_stream);

/* 3x3 morphology / median / hole-fill post-processing of a byte mask on device
 * (BackgroundSubtractorSuBSENSE.cpp:624-640). op: 0 erode3x3, 1 dilate3x3, 2 median(ksize),
 * 3 median(ksize) of a {0,255} mask (majority count, same result, faster), 4 cv::floodFill(img, Point(0,0), 255). */
int bgs_mask_morph_device(int hip_device, const void* d_src, void* d_dst, int rows, int cols, int op, int ksize,
                          int iterations, void* hip_stream);

/* cvCanny(src, dst, low, high) with aperture 3 and the L1 magnitude, on `images` 8-bit single-channel images stored back to back
 * ([images][rows][cols]); d_dst receives 0 / 255 in the same layout (SJN_MultiCueBGS.cpp:998, :1007 run it on every bounding box).
 * Definition: Sobel 3x3 with a replicated border, |dx| + |dy|, non-maximum suppression with the 15-bit
 * fixed-point tan 22.5 deg test, hysteresis from the pixels above max(low, high) through those above min(low, high), 8-connected.
 * One workgroup per image with the image's gradient in LDS, so rows * cols <= BGS_CANNY_MAX_PIXELS (BGS_ERR_UNSUPPORTED above).
 * Asynchronous on hip_stream; in-place operation is refused. */
#define BGS_CANNY_MAX_PIXELS 20480
int bgs_canny_device(int hip_device, const void* d_src, void* d_dst, int images, int rows, int cols, int low, int high,
                     void* hip_stream);

/* MotionDetection::GetMotionsMaskHU of LbpMrf (package_bgs/ck/MotionDetection.cpp:1256-1366) as a pure function, `images` maps at
 * once: the background-rate map of the node grid in, the class's foreground mask out.  A = histogram_area
 * (HUHistogramArea, 5), w = min_cut_weight (HUMinCutWeight, 8.0f); the node grid is NH = rows - A + 1 by NW = (cols - A + 1) / 2.
 * Per node: source capacity 1, sink capacity (short)(w * (1 - rate)) clamped to [0, 32767]; edges of capacity 1 each way from node
 * (x, y) to (x-1, y) and (x, y-1) only where x > 0 and y > 0 (row 0 has no horizontal edges, column 0 no vertical ones).  The exact
 * minimum cut: a node is SOURCE iff the source reaches it in the residual graph of a maximum flow, as Graph::what_segment says.
 * Then the mask of :1322-1342 (node row y on image row y + A - A / 2, node column on image column x + A / 2), cvFloodFill from
 * (0, 0) with the holes becoming foreground, and one 3 x 3 erosion.
 *   d_rate   f32 [images][NH][NW]      d_mask  u8 [images][rows][cols], 0 / 255
 *   d_labels u8 [images][NH][NW] or NULL, 1 = SINK      d_flow  i32 [images] or NULL: the value Graph::maxflow() returns
 * Asynchronous on hip_stream (its scratch memory is allocated and freed in stream order).  The cut converges through a fixed number
 * of launches; a call that needed more raises the device's sticky counter (bgs_lbpmrf_mask_counters) and its outputs are not the cut.
 * bgs_lbpmrf_mask_check states every refusal without a device, all BGS_ERR_UNSUPPORTED: an even A or A < 3, a frame with no node
 * (NH < 1 or NW < 1), a weight that is not finite, and an odd cols - A + 1: the reference indexes its node array with x / 2 for x up
 * to cols - A, past the array when that width is odd. */
int bgs_lbpmrf_mask_check(int rows, int cols, int histogram_area, float min_cut_weight);
int bgs_lbpmrf_mask_device(int hip_device, const void* d_rate, void* d_mask, void* d_labels, void* d_flow, int images, int rows,
                           int cols, int histogram_area, float min_cut_weight, void* hip_stream);
/* Waits for the device.  *not_converged: how many bgs_lbpmrf_mask_device calls on this device, since the library was loaded, were not
 * finished by their launches (sticky; 0 is the only healthy value).  *last_launches: the relaxation launches the last call used.
 * Either pointer may be NULL. */
int bgs_lbpmrf_mask_counters(int hip_device, uint64_t* not_converged, uint64_t* last_launches);

/* ---- the model stage of SJN_MultiCueBGS (package_bgs/sjn): everything the class does per pixel -------------
 * Frame reduction, the 7 x 7 blur, the HSV-cone conversion, the texture and colour codebooks with their cache-books, training,
 * the confidence and landmark maps and the model update with absorption, as SJN_MultiCueBGS.cpp's own functions define them.
 * The box stage between the landmark map and the update (morphology, labelling, bounding boxes, the Canny / Hausdorff ghost
 * test) is bgs_multicue_boxes_device below: bgs_multicue_update_device takes the update maps that stage produces, and
 * bgs_multicue_process_device chains everything.  The books are fixed-capacity slot
 * planes: an insert or an absorption into a full book is dropped and counted in the sticky "overflow" counter (the reference's
 * arrays grow without bound; the capacities are at least twice the largest book it was measured to reach). */
#define BGS_MULTICUE_TEXTURE_SLOTS 20
#define BGS_MULTICUE_TEXTURE_CACHE_SLOTS 16
#define BGS_MULTICUE_COLOR_SLOTS 32
#define BGS_MULTICUE_COLOR_CACHE_SLOTS 16
typedef struct bgs_multicue_params {
  uint32_t struct_size;            /* sizeof(bgs_multicue_params) */
  int32_t training_period;         /* g_iTrainingPeriod 20: frames 0 .. training_period train (training_period + 1 frames) */
  int32_t t_model_threshold;       /* g_iT_ModelThreshold 1: the landmark is 255 where confidence > t_model_threshold / 6.0f */
  int32_t c_model_threshold;       /* g_iC_ModelThreshold 10: read by nothing here; carried for the class */
  float learning_rate;             /* g_fLearningRate 0.05f; training runs at learning_rate * 4 */
  int32_t texture_train_vol_range; /* g_nTextureTrainVolRange 15 (a short in the reference) */
  int32_t color_train_vol_range;   /* g_nColorTrainVolRange 20 (a short) */
  int32_t absorption_enable;       /* g_bAbsorptionEnable 1: cache-books and absorption */
  int32_t absorption_period;       /* g_iAbsortionPeriod 200 */
  int32_t reduced_width;           /* g_iRWidth 160 */
  int32_t reduced_height;          /* g_iRHeight 120 */
  int32_t back_clear_period;       /* g_iBackClearPeriod 300 (handed over as a short) */
  int32_t cache_clear_period;      /* g_iCacheClearPeriod 30: read by nothing (the cache-book clear uses the literal 10) */
} bgs_multicue_params;
typedef struct bgs_multicue bgs_multicue; /* n_streams models, each with its own frame counter (per-stream lifetime: below) */
int bgs_multicue_default_params(bgs_multicue_params* p);
/* Every refusal, without a device (BGS_ERR_UNSUPPORTED, the class named): values that are not finite, periods and ranges
 * outside 1..32767 (ranges may be 0), reduced sides below 5, reduced_width * reduced_height > BGS_CANNY_MAX_PIXELS (the class's
 * per-box Canny runs on the reduced frame).  rows == 0 checks the parameters only; otherwise rows x cols is the frame. p NULL: the defaults. */
int bgs_multicue_check(const bgs_multicue_params* p, int rows, int cols);
int bgs_multicue_create(int hip_device, int n_streams, const bgs_multicue_params* p, bgs_multicue** m);
void bgs_multicue_destroy(bgs_multicue* m);
/* One BackgroundModeling_Par per stream on d_frames u8 [n_streams][rows][cols][3].  The first call fixes the geometry (another one
 * later: BGS_ERR_GEOMETRY); a call after the (training_period + 1)-th: BGS_ERR_STATE. */
int bgs_multicue_train_device(bgs_multicue* m, const void* d_frames, int rows, int cols, void* hip_stream);
/* PreProcessing, T_GetConfidenceMap_Par and CreateLandmarkArray_Par.  d_landmark u8 [n_streams][rh][rw] (0 / 125 / 255), d_conf f32 of
 * the same shape or NULL.  BGS_ERR_STATE before training is complete. */
int bgs_multicue_landmark_device(bgs_multicue* m, const void* d_frames, int rows, int cols, void* d_landmark, void* d_conf, void* hip_stream);
/* The model update on the XYZ frame and the landmark map of the last landmark call; d_update_map u8 [n_streams][rh][rw], its 2-pixel
 * border ignored.  ghost == 1, step 2 of EvaluateGhostRegion: pixels whose map is non-zero get construction on the background books at
 * learning_rate, then the clear with back_clear_period.  ghost == 0, step 2 of UpdateModel_Par with the map as g_aUpdateMap: non-zero
 * takes the background path, zero the cache-book path with absorption (when enabled); the cache-book clear follows either way.
 * BGS_ERR_STATE without a landmark call since the last ghost == 0 update. */
int bgs_multicue_update_device(bgs_multicue* m, const void* d_update_map, int ghost, void* hip_stream);
/* State of one stream, unpacked in the reference's field order (n = rh * rw; slots at and beyond m_iNumEntries read 0); returns the
 * bytes written.  "gauss", "xyz" u8 [n][3]; "conf" f32 [n]; "landmark" u8 [n]; "tbook", "tcache" i32 [n][6][2] = m_iTotal,
 * m_iNumEntries; "tmeans", "tcache_means" f32 [n][6][SLOTS]; "tmeta", "tcache_meta" i32 [n][6][SLOTS][3] = MNRL, first, last;
 * "tref", "tcnt" i16 [n][6]; "cbook", "ccache" i32 [n][2]; "cmeans", "ccache_means" f64 [n][SLOTS][3]; "cmeta", "ccache_meta"
 * i32 [n][SLOTS][3]; "cref", "ccnt" i16 [n]; "count" i64 [1] = the stream's g_iFrameCount; "overflow" i64 [1]; "box_overflow" i64 [1]
 * (below; both are the handle's, not the stream's).  Waits for the device. */
int64_t bgs_multicue_get_state(bgs_multicue* m, int stream, const char* plane, void* dst, size_t cap);
/* The box stage: PostProcessing (SJN_MultiCueBGS.cpp:335) and step 1 of UpdateModel_Par (:367-382) as a pure function
 * of (landmark map, frame), n_streams at once.  It reads the handle's parameters and geometry only (a first call fixes the geometry as
 * a training call would; another one later: BGS_ERR_GEOMETRY) and touches neither the books nor the frame counter.
 *   d_landmark u8 [n_streams][rh][rw]; d_frames u8 [n_streams][rows][cols][3]
 *   d_fore u8 [n_streams][rh][rw]        g_aResizedForeMap after RemovingInvalidForeRegions (0 / 255)
 *   d_ghost_map u8 [n_streams][rh][rw]   the aUpdateMap of EvaluateGhostRegion step 1: for bgs_multicue_update_device(..., ghost = 1)
 *   d_update_map u8 [n_streams][rh][rw]  g_aUpdateMap: for the ghost = 0 call
 *   d_count i32 [n_streams]              the label count of Labeling (it may exceed BGS_MULTICUE_MAX_BOXES)
 *   d_boxes i32 [n_streams][BGS_MULTICUE_MAX_BOXES][BGS_MULTICUE_BOX_FIELDS]: m_aRLeft, m_aRRight, m_aRUpper, m_aRBottom, m_aLeft,
 *     m_aRight, m_aUpper, m_aBottom, valid after EvaluateBoxSize, final m_ValidBox, frame-edge points, foreground-edge points,
 *     foreground-edge points within squared distance 100 of a frame-edge point; rows at and beyond the count read 0.
 * The reference has room for 300 boxes and writes past it; here the labels beyond BGS_MULTICUE_MAX_BOXES get no box, their pixels stay
 * as they are, and the sticky "box_overflow" counter of bgs_multicue_get_state goes up by one per stream and call.
 * Asynchronous on hip_stream; no allocation; the count never comes back to the host. */
#define BGS_MULTICUE_MAX_BOXES 300
#define BGS_MULTICUE_BOX_FIELDS 13
int bgs_multicue_boxes_device(bgs_multicue* m, const void* d_landmark, const void* d_frames, int rows, int cols, void* d_fore, void* d_ghost_map,
                              void* d_update_map, void* d_count, void* d_boxes, void* hip_stream);
/* process() (SJN_MultiCueBGS.cpp:85-99) per stream in one asynchronous call.  While the frame counter is <= training_period: a training
 * frame, and d_out is zeroed.  Afterwards the landmark call, the box stage, the ghost = 1 update with the ghost map, the ghost = 0
 * update with the update map, and GetForegroundMap(result, NULL): the foreground map resized bilinearly to rows x cols (values between
 * 0 and 255 are kept; the reference's three channels are equal).  d_out u8 [n_streams][rows][cols].  BGS_ERR_GEOMETRY for another
 * frame size; BGS_ERR_STATE when a bgs_multicue_landmark_device call is still waiting for its updates. */
int bgs_multicue_process_device(bgs_multicue* m, const void* d_frames, int rows, int cols, void* d_out, void* hip_stream);
/* ---- per-stream lifetime.  Every stream has a frame counter of its own ("count" of bgs_multicue_get_state); a handle's streams need not
 * be the same age.  bgs_multicue_process_device is the range [0, n_streams) of the call below.  The piecewise calls (train / landmark /
 * update / boxes) keep their meaning over all streams and return BGS_ERR_STATE, naming the range call, once the ages differ.
 * Calls on one handle from several host threads are not supported: the counters are not locked. */
/* process() for streams [first, first + count), which may be at different ages: d_frames u8 [count][rows][cols][3] and d_out u8
 * [count][rows][cols] point at stream `first`.  Neighbouring streams in the same phase (training frame, last training frame, detecting)
 * share one launch of each kernel.  A stream's frame 0, the first ever or the first after bgs_multicue_reset_stream, initialises that
 * stream's model on hip_stream before it trains.  Disjoint ranges may be in flight on different HIP streams at the same time.
 * BGS_ERR_INVALID for a range outside the handle, BGS_ERR_GEOMETRY for another frame size.  Asynchronous; no allocation. */
int bgs_multicue_process_range_device(bgs_multicue* m, int first, int count, const void* d_frames, int rows, int cols, void* d_out, void* hip_stream);
/* The stream's next frame is training frame 0.  Host-only: it neither touches nor waits for the device, and until that frame
 * bgs_multicue_get_state returns for this stream what a newly created handle returns.  The caller orders that next frame behind whatever
 * is still in flight for the stream on another HIP stream.  BGS_ERR_INVALID for a stream outside the handle. */
int bgs_multicue_reset_stream(bgs_multicue* m, int stream);
/* process() on one frame in host memory, for one stream, synchronous: `frame` is rows x cols x 3 bytes with a row pitch of `step` bytes,
 * `out` receives rows x cols x out_channels bytes (out_channels 1 or 3; the reference's img_output is 8UC3 with equal channels, which the
 * host writes: one channel crosses the bus) with a row pitch of out_step.  The call uses a HIP stream, page-locked staging and device buffers
 * of the handle's own, made by the first such call: the only call of the object that allocates.  Pitches below the row size and streams
 * outside the handle: BGS_ERR_INVALID; another frame size: BGS_ERR_GEOMETRY.  Ordering against device calls that step the same stream on
 * other HIP streams is the caller's responsibility. */
int bgs_multicue_process(bgs_multicue* m, int stream, const void* frame, int rows, int cols, size_t step, void* out, size_t out_step, int out_channels);
/* BGR2HSVxyz_Par on a flat array of pixels: d_bgr, d_xyz u8 [pixels][3].  Asynchronous on hip_stream. */
int bgs_multicue_xyz_device(int hip_device, const void* d_bgr, void* d_xyz, size_t pixels, void* hip_stream);

/* Connected-component seeding of a byte mask on device: what OpenCV-legacy's blob detector derives
 * from the mask right after IBGS::process (ustc_src/trackingMain.cpp:56-57, :166; cvFindContours + bounding rectangles;
 * in-tree kin: package_bgs/jmo/BlobExtraction.cpp).  Components are the maximal 8- (or 4-) connected sets of non-zero
 * pixels.  A component is named by `root`, the raster index (y*cols + x) of its first pixel; boxes are written sorted by
 * root, so the output is deterministic.  *d_count receives the number of components found (it may exceed max_boxes;
 * only the first max_boxes are written).  d_labels (optional, [rows*cols] int32): root of each pixel's component, -1 for
 * background.  d_work: bgs_mask_components_workspace(rows, cols) bytes of device scratch; with d_work the call is
 * asynchronous on hip_stream, with NULL it allocates, synchronises and frees (slow path). */
typedef struct bgs_box {
  int32_t x, y, w, h; /* bounding rectangle */
  int32_t area;       /* pixels in the component */
  int32_t root;       /* raster index of the component's first pixel */
} bgs_box;
size_t bgs_mask_components_workspace(int rows, int cols);
int bgs_mask_components_device(int hip_device, const void* d_mask, int rows, int cols, int connectivity,
                               int32_t* d_labels, bgs_box* d_boxes, int max_boxes, int32_t* d_count, void* d_work,
                               void* hip_stream);
/* The same for `images` masks stored back to back ([images][rows][cols], e.g. the d_fg of bgs_process_batch_device): one
 * set of launches for all of them.  Boxes are sorted by (image, root); d_offsets [images+1] receives the prefix sums of the
 * per-image component counts, so image k owns d_boxes[d_offsets[k] .. d_offsets[k+1]) (entries past max_boxes are not
 * written); roots and labels are relative to their own image. */
size_t bgs_mask_components_batch_workspace(int images, int rows, int cols);
int bgs_mask_components_batch_device(int hip_device, const void* d_masks, int images, int rows, int cols, int connectivity,
                                     int32_t* d_labels, bgs_box* d_boxes, int max_boxes, int32_t* d_offsets, void* d_work,
                                     void* hip_stream);

/* ---- N2: blob list hand-off (ustc_src/trackingMain.cpp:166: the blob detector consumes the mask right after FG detection) ----
 * OpenCV-legacy's detectors turn each foreground region into a CvBlob {x, y, w, h, ID} from the region's bounding rectangle
 * and its coordinate moments (centre = centroid, size = 4 sigma; recalled from modules/legacy/src/enteringblobdetection.cpp,
 * not in the tree).  Both are produced here, per component, so the caller can apply either convention
 * (tracking_amd/host/blob.h: blob_from_box / blob_from_moments). */
typedef struct bgs_moments {
  int64_t sx, sy;   /* sum of x, sum of y over the component's pixels (image coordinates) */
  int64_t sxx, syy; /* sum of x*x, sum of y*y */
} bgs_moments;
/* bgs_mask_components_batch_device plus the moments of every component (d_moments [max_boxes], same order as d_boxes;
 * NULL = not wanted).  No labels output. */
int bgs_mask_blobs_batch_device(int hip_device, const void* d_masks, int images, int rows, int cols, int connectivity,
                                bgs_box* d_boxes, bgs_moments* d_moments, int max_boxes, int32_t* d_offsets, void* d_work,
                                void* hip_stream);
/* Host path: components of the foreground mask that the LAST bgs_process call of `stream` produced, computed on the device
 * copy of that mask (bgs_process keeps it even when its `fg` argument is NULL, so a caller that only wants blobs moves no
 * mask over PCIe); components narrower than min_w or lower than min_h are dropped; host arrays boxes / moments (optional)
 * [max_boxes] receive the first max_boxes survivors in raster order of their first pixel, *count their number.  Synchronous.
 * BGS_ERR_STATE if that call produced no valid mask (warm-up frame) or another stream has been processed since. */
int bgs_last_mask_blobs(bgs_engine* e, int stream, int connectivity, int min_w, int min_h, bgs_box* boxes, bgs_moments* moments,
                        int max_boxes, int32_t* count);

/* ---- N3: frame preparation on the device (the step BEFORE the path) --------------------------------------------------------
 * What VideoCapture::start (VideoCapture.cpp:158-207: cvResize to input_resize_percent, cvFlip(frame, frame, 0), ROI view) and
 * PreProcessor::process (PreProcessor.cpp:46-77: optional cv::equalizeHist, optional cv::GaussianBlur 7x7 sigma 1.5) do to a
 * captured frame before FrameProcessor hands it to every IBGS::process, in that order, as one device pass over frames that
 * are already in HBM (a decoder's output) or as a host-buffer convenience.  Flip and ROI are exact by definition; resize,
 * equalizeHist and GaussianBlur restate OpenCV 2.4's 8-bit fixed-point arithmetic from recall (unpinned). */
typedef struct bgs_ingest {
  uint32_t struct_size;     /* sizeof(bgs_ingest) */
  int32_t resize_percent;   /* VideoCapture input_resize_percent; 100 = same size; output = (cols*pct/100, rows*pct/100) */
  int32_t flip;             /* VideoCapture enableFlip: rows reversed (cvFlip mode 0) */
  int32_t roi_x0, roi_y0, roi_x1, roi_y1; /* VideoCapture ROI in the resized, flipped frame; used when x1 > x0 and y1 > y0 */
  int32_t equalize_hist;    /* PreProcessor equalizeHist: 1-channel frames only (cv::equalizeHist asserts CV_8UC1) */
  int32_t gaussian_blur;    /* PreProcessor gaussianBlur */
} bgs_ingest;
int bgs_ingest_default(bgs_ingest* cfg); /* the reference's defaults: 100 %, nothing else */
/* geometry of the prepared frame; BGS_ERR_INVALID for a ROI outside the resized frame or an empty result */
int bgs_ingest_size(const bgs_ingest* cfg, int src_rows, int src_cols, int* rows, int* cols);
/* bytes of device scratch bgs_ingest_device needs for `images` frames (0 when the configuration needs none) */
size_t bgs_ingest_workspace(const bgs_ingest* cfg, int images, int src_rows, int src_cols, int channels);
/* d_src: [images] frames of src_rows x src_cols x channels uint8, rows src_step bytes apart, images src_rows*src_step apart.
 * d_dst: [images][rows][cols][channels] contiguous (bgs_ingest_size) - what bgs_process_batch_device takes.  Asynchronous on
 * hip_stream; d_work may be NULL when bgs_ingest_workspace is 0. */
int bgs_ingest_device(int hip_device, const bgs_ingest* cfg, const void* d_src, int images, int src_rows, int src_cols, int channels,
                      size_t src_step, void* d_dst, void* d_work, void* hip_stream);
/* Make the frame preparation part of the engine's host path: from now on bgs_process takes the RAW captured frame (any size, but
 * the same size every call) and fg / bg come out in the prepared geometry (bgs_ingest_size), which is also the engine's geometry.
 * Flip and ROI alone are folded into the pinned staging copy (no device work at all); resize / equalizeHist / GaussianBlur run
 * as bgs_ingest_device between the upload and the model kernel.  Must be called before the first frame; cfg NULL switches it off. */
int bgs_set_ingest(bgs_engine* e, const bgs_ingest* cfg);
/* Host buffers in, host buffers out (PreProcessor::process / VideoCapture's frame preparation as one call): uploads, runs
 * bgs_ingest_device, downloads.  dst: rows x cols x channels, rows dst_step bytes apart.  Synchronous. */
int bgs_ingest_host(int hip_device, const bgs_ingest* cfg, const uint8_t* src, int src_rows, int src_cols, int channels, size_t src_step,
                    uint8_t* dst, size_t dst_step);

#ifdef __cplusplus
}
#endif
#endif /* BGS_HIP_H */
