// bgs_classes.inc — the IBGS classes of the hot path, one per reference class: algorithm id and one description of its
// ./config/<Class>.xml (keys in the reference's order, each with its member and default; reference file:line beside it).
// HipBGSBase makes loadConfig() and saveConfig() of that description (bgs_describe.inc).  Written against HipBGSBase, XmlIo, params_
// and firstTime only, so the same list serves tracking_amd/host/bgs_host.h (bgs_hip::Image, own XML reader: compiled and tested in
// this repository) and tracking_amd/host/HipBGS.h (cv::Mat + CvFileStorage: what a maintainer adds to the reference tree, C++03).
// Include inside a namespace, after HipBGSBase / BGS_HIP_BANNER_DTOR are defined.  Every member a description names is set by the
// loadConfig() that process() starts with, before anything reads it.

// package_bgs/FrameDifferenceBGS.{h,cpp}
class FrameDifferenceBGS : public HipBGSBase {
 public:
  FrameDifferenceBGS() : HipBGSBase(BGS_FRAME_DIFF, "FrameDifferenceBGS") {}
  BGS_HIP_BANNER_DTOR(FrameDifferenceBGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // FrameDifferenceBGS.cpp:65-85
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/StaticFrameDifferenceBGS.{h,cpp}
class StaticFrameDifferenceBGS : public HipBGSBase {
 public:
  StaticFrameDifferenceBGS() : HipBGSBase(BGS_STATIC_FRAME_DIFF, "StaticFrameDifferenceBGS") {}
  BGS_HIP_BANNER_DTOR(StaticFrameDifferenceBGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/WeightedMovingMeanBGS.{h,cpp}
class WeightedMovingMeanBGS : public HipBGSBase {
 public:
  WeightedMovingMeanBGS() : HipBGSBase(BGS_WMM, "WeightedMovingMeanBGS") {}
  BGS_HIP_BANNER_DTOR(WeightedMovingMeanBGS)
 private:
  bool showOutput, showBackground;
  void describe(XmlIo& io) override {  // WeightedMovingMeanBGS.cpp:98-122
    io("enableWeight", params_.enable_weight, true);
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showOutput", showOutput, true);
    io("showBackground", showBackground, false);
  }
};

// package_bgs/WeightedMovingVarianceBGS.{h,cpp}
class WeightedMovingVarianceBGS : public HipBGSBase {
 public:
  WeightedMovingVarianceBGS() : HipBGSBase(BGS_WMV, "WeightedMovingVarianceBGS") {}
  BGS_HIP_BANNER_DTOR(WeightedMovingVarianceBGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // WeightedMovingVarianceBGS.cpp:139-161
    io("enableWeight", params_.enable_weight, true);
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/AdaptiveBackgroundLearning.{h,cpp}
class AdaptiveBackgroundLearning : public HipBGSBase {
 public:
  AdaptiveBackgroundLearning() : HipBGSBase(BGS_ABL, "AdaptiveBackgroundLearning") {}
  BGS_HIP_BANNER_DTOR(AdaptiveBackgroundLearning)
 private:
  bool showForeground, showBackground;
  void describe(XmlIo& io) override {  // AdaptiveBackgroundLearning.cpp:85-111
    io("alpha", params_.alpha, 0.05);
    io("limit", params_.limit, -1);
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showForeground", showForeground, true);
    io("showBackground", showBackground, true);
  }
};

// package_bgs/AdaptiveSelectiveBackgroundLearning.{h,cpp}: the background model is the gray image the class keeps
class AdaptiveSelectiveBackgroundLearning : public HipBGSBase {
 public:
  AdaptiveSelectiveBackgroundLearning() : HipBGSBase(BGS_ASBL, "AdaptiveSelectiveBackgroundLearning") {}
  BGS_HIP_BANNER_DTOR(AdaptiveSelectiveBackgroundLearning)
 private:
  bool showOutput;
  int bgChannels(int) const override { return 1; }
  void describe(XmlIo& io) override {  // AdaptiveSelectiveBackgroundLearning.cpp:107-131 (defaults 90 / 25 differ from the ctor's -1 / 15, SURVEY.md App. C 5)
    io("learningFrames", params_.learning_frames, 90);
    io("alphaLearn", params_.alpha_learn, 0.05);
    io("alphaDetection", params_.alpha_detection, 0.05);
    io("threshold", params_.threshold, 25);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/MixtureOfGaussianV2BGS.{h,cpp}
class MixtureOfGaussianV2BGS : public HipBGSBase {
 public:
  MixtureOfGaussianV2BGS() : HipBGSBase(BGS_MOG2, "MixtureOfGaussianV2BGS") {}
  BGS_HIP_BANNER_DTOR(MixtureOfGaussianV2BGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // MixtureOfGaussianV2BGS.cpp:76-98
    io("alpha", params_.alpha, 0.05);
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/MixtureOfGaussianV1BGS.{h,cpp}
class MixtureOfGaussianV1BGS : public HipBGSBase {
 public:
  MixtureOfGaussianV1BGS() : HipBGSBase(BGS_MOG1, "MixtureOfGaussianV1BGS", /*clears_bg=*/true) {}
  BGS_HIP_BANNER_DTOR(MixtureOfGaussianV1BGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // MixtureOfGaussianV1BGS.cpp:73-95
    io("alpha", params_.alpha, 0.05);
    io("enableThreshold", params_.enable_threshold, true);
    io("threshold", params_.threshold, 15);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/GMG.{h,cpp}
class GMG : public HipBGSBase {
 public:
  GMG() : HipBGSBase(BGS_GMG, "GMG", /*clears_bg=*/true) {}
  BGS_HIP_BANNER_DTOR(GMG)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // GMG.cpp:79-99
    io("initializationFrames", params_.gmg_init_frames, 20);
    io("decisionThreshold", params_.gmg_decision_threshold, 0.7);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/bl/SigmaDeltaBGS.{h,cpp}
class SigmaDeltaBGS : public HipBGSBase {
 public:
  SigmaDeltaBGS() : HipBGSBase(BGS_SIGMA_DELTA, "SigmaDeltaBGS") {}
  BGS_HIP_BANNER_DTOR(SigmaDeltaBGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // SigmaDeltaBGS.cpp:57-79
    io("ampFactor", params_.sd_amp_factor, 1);
    io("minVar", params_.sd_min_var, 15);
    io("maxVar", params_.sd_max_var, 255);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/pl/SuBSENSE.{h,cpp} (the class USTC_BGS type 36 instantiates, ustc_src/ustc_bgs.cpp:68)
class SuBSENSEBGS : public HipBGSBase {
 public:
  SuBSENSEBGS() : HipBGSBase(BGS_SUBSENSE, "SuBSENSEBGS") {}
  ~SuBSENSEBGS() override {}
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // SuBSENSE.cpp:47-75 (read every frame; the model itself is built once, on the first frame)
    io("fRelLBSPThreshold", params_.lbsp_rel_threshold, 0.333f);
    io("nDescDistThresholdOffset", params_.subsense_desc_dist_threshold_offset, 3);
    io("nMinColorDistThreshold", params_.subsense_min_color_dist_threshold, 30);
    io("nBGSamples", params_.subsense_n_samples, 50);
    io("nRequiredBGSamples", params_.subsense_n_required, 2);
    io("nSamplesForMovingAvgs", params_.subsense_samples_for_moving_avgs, 100);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/pl/LOBSTER.{h,cpp}: like SuBSENSEBGS, the parameters are handed to the model once, when it is built on the first frame
class LOBSTERBGS : public HipBGSBase {
 public:
  LOBSTERBGS() : HipBGSBase(BGS_LOBSTER, "LOBSTERBGS") {}
  ~LOBSTERBGS() override {}
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // LOBSTER.cpp:47-73
    io("fRelLBSPThreshold", params_.lbsp_rel_threshold, 0.365f);
    io("nLBSPThresholdOffset", params_.lbsp_threshold_offset, 0);
    io("nDescDistThreshold", params_.subsense_desc_dist_threshold_offset, 4);
    io("nColorDistThreshold", params_.subsense_min_color_dist_threshold, 30);
    io("nBGSamples", params_.subsense_n_samples, 35);
    io("nRequiredBGSamples", params_.subsense_n_required, 2);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/dp/DP*BGS.{h,cpp}: the wrapper reads its XML every frame but hands the values to the model only once, inside
// `if(firstTime)` (e.g. DPZivkovicAGMMBGS.cpp:48-65) - later edits of the file change what saveConfig would write, not the
// running model.  Mirrored: the values go into params_ only while firstTime is true.  Each class describes the three keys its
// wrapper has; the members it does not name keep the algorithm's own defaults.
class DPBase : public HipBGSBase {
 protected:
  DPBase(bgs_algo algo, const char* name) : HipBGSBase(algo, name) {
    threshold = params_.dp_threshold, alpha = params_.dp_alpha, gaussians = params_.dp_gaussians;
    learningFrames = params_.learning_frames, samplingRate = params_.dp_sampling_rate;
  }
  double threshold, alpha;
  int gaussians, learningFrames, samplingRate;
  bool showOutput;
  void loaded() override {
    if (!firstTime) return;
    params_.dp_threshold = (float)threshold, params_.dp_alpha = (float)alpha, params_.dp_gaussians = gaussians;
    params_.learning_frames = learningFrames, params_.dp_sampling_rate = samplingRate;
  }
};

class DPZivkovicAGMMBGS : public DPBase {
 public:
  DPZivkovicAGMMBGS() : DPBase(BGS_DP_ZIVKOVIC_AGMM, "DPZivkovicAGMMBGS") {}
  BGS_HIP_BANNER_DTOR(DPZivkovicAGMMBGS)
 private:
  void describe(XmlIo& io) override {  // DPZivkovicAGMMBGS.cpp:82-104
    io("threshold", threshold, 25.0f);
    io("alpha", alpha, 0.001f);
    io("gaussians", gaussians, 3);
    io("showOutput", showOutput, true);
  }
};

class DPGrimsonGMMBGS : public DPBase {
 public:
  DPGrimsonGMMBGS() : DPBase(BGS_DP_GRIMSON_GMM, "DPGrimsonGMMBGS") {}
  BGS_HIP_BANNER_DTOR(DPGrimsonGMMBGS)
 private:
  void describe(XmlIo& io) override {  // DPGrimsonGMMBGS.cpp:84-105
    io("threshold", threshold, 9.0);
    io("alpha", alpha, 0.01);
    io("gaussians", gaussians, 3);
    io("showOutput", showOutput, true);
  }
};

class DPWrenGABGS : public DPBase {
 public:
  DPWrenGABGS() : DPBase(BGS_DP_WREN_GA, "DPWrenGABGS") {}
  BGS_HIP_BANNER_DTOR(DPWrenGABGS)
 private:
  void describe(XmlIo& io) override {  // DPWrenGABGS.cpp:83-104
    io("threshold", threshold, 12.25f);
    io("alpha", alpha, 0.005f);
    io("learningFrames", learningFrames, 30);
    io("showOutput", showOutput, true);
  }
};

class DPMeanBGS : public DPBase {
 public:
  DPMeanBGS() : DPBase(BGS_DP_MEAN, "DPMeanBGS") {}
  BGS_HIP_BANNER_DTOR(DPMeanBGS)
 private:
  void describe(XmlIo& io) override {  // DPMeanBGS.cpp:84-105 (threshold is an int there)
    io.asInt("threshold", threshold, 2700);
    io("alpha", alpha, 1e-6f);
    io("learningFrames", learningFrames, 30);
    io("showOutput", showOutput, true);
  }
};

class DPAdaptiveMedianBGS : public DPBase {
 public:
  DPAdaptiveMedianBGS() : DPBase(BGS_DP_ADAPTIVE_MEDIAN, "DPAdaptiveMedianBGS") {}
  BGS_HIP_BANNER_DTOR(DPAdaptiveMedianBGS)
 private:
  void describe(XmlIo& io) override {  // DPAdaptiveMedianBGS.cpp:83-104
    io.asInt("threshold", threshold, 40);
    io("samplingRate", samplingRate, 7);
    io("learningFrames", learningFrames, 30);
    io("showOutput", showOutput, true);
  }
};
