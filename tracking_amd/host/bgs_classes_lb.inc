// bgs_classes_lb.inc — Laurence Bender's five per-pixel models of package_bgs/lb (USTC_BGS types 25-29), in the form bgs_classes.inc
// describes.
//
// Every wrapper re-reads ./config/<Class>.xml at the top of process() and hands the 0..255 integers to its model with
// setBGModelParameter on every frame (LB*.cpp:31-56): mirrored, the keys are described straight on params_, so every load reaches the
// model through the bgs_set_params the base class calls each frame.  The wrappers return cv::Mat(m_pBGModel->GetFG()), an 8UC3 image
// whose three channels hold the mask byte: fg_channels_ = 3 makes the base class replicate the engine's one-byte mask the same way.

// package_bgs/lb/LBSimpleGaussian.{h,cpp} (USTC_BGS type 25)
class LBSimpleGaussian : public HipBGSBase {
 public:
  LBSimpleGaussian() : HipBGSBase(BGS_LB_SIMPLE_GAUSSIAN, "LBSimpleGaussian") { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBSimpleGaussian)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // LBSimpleGaussian.cpp:78-99
    io("sensitivity", params_.lb_sensitivity, 66);
    io("noiseVariance", params_.lb_noise_variance, 162);
    io("learningRate", params_.lb_learning_rate, 18);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/lb/LBFuzzyGaussian.{h,cpp} (USTC_BGS type 26)
class LBFuzzyGaussian : public HipBGSBase {
 public:
  LBFuzzyGaussian() : HipBGSBase(BGS_LB_FUZZY_GAUSSIAN, "LBFuzzyGaussian") { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBFuzzyGaussian)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // LBFuzzyGaussian.cpp:79-104
    io("sensitivity", params_.lb_sensitivity, 72);
    io("bgThreshold", params_.lb_bg_threshold, 162);
    io("learningRate", params_.lb_learning_rate, 49);
    io("noiseVariance", params_.lb_noise_variance, 195);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/lb/LBMixtureOfGaussians.{h,cpp} (USTC_BGS type 27)
class LBMixtureOfGaussians : public HipBGSBase {
 public:
  LBMixtureOfGaussians() : HipBGSBase(BGS_LB_MOG, "LBMixtureOfGaussians") { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBMixtureOfGaussians)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // LBMixtureOfGaussians.cpp:79-104
    io("sensitivity", params_.lb_sensitivity, 81);
    io("bgThreshold", params_.lb_bg_threshold, 83);
    io("learningRate", params_.lb_learning_rate, 59);
    io("noiseVariance", params_.lb_noise_variance, 206);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/lb/LBAdaptiveSOM.{h,cpp} (USTC_BGS type 28)
class LBAdaptiveSOM : public HipBGSBase {
 public:
  LBAdaptiveSOM() : HipBGSBase(BGS_LB_ADAPTIVE_SOM, "LBAdaptiveSOM") { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBAdaptiveSOM)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // LBAdaptiveSOM.cpp:81-108
    io("sensitivity", params_.lb_sensitivity, 75);
    io("trainingSensitivity", params_.lb_training_sensitivity, 245);
    io("learningRate", params_.lb_learning_rate, 62);
    io("trainingLearningRate", params_.lb_training_learning_rate, 255);
    io("trainingSteps", params_.lb_training_steps, 55);
    io("showOutput", showOutput, true);
  }
};

// package_bgs/lb/LBFuzzyAdaptiveSOM.{h,cpp} (USTC_BGS type 29)
class LBFuzzyAdaptiveSOM : public HipBGSBase {
 public:
  LBFuzzyAdaptiveSOM() : HipBGSBase(BGS_LB_FUZZY_ADAPTIVE_SOM, "LBFuzzyAdaptiveSOM") { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBFuzzyAdaptiveSOM)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // LBFuzzyAdaptiveSOM.cpp:81-108
    io("sensitivity", params_.lb_sensitivity, 90);
    io("trainingSensitivity", params_.lb_training_sensitivity, 240);
    io("learningRate", params_.lb_learning_rate, 38);
    io("trainingLearningRate", params_.lb_training_learning_rate, 255);
    io("trainingSteps", params_.lb_training_steps, 81);
    io("showOutput", showOutput, true);
  }
};
