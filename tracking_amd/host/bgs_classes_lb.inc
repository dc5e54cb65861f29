// bgs_classes_lb.inc — Laurence Bender's five per-pixel models of package_bgs/lb (USTC_BGS types 25-29), written against the same
// four names as bgs_classes.inc and included right after bgs_classes_dp2.inc by tracking_amd/host/bgs_host.h and
// tracking_amd/host/HipBGS.h.  A file of its own: the tests pin the class lists of bgs_classes.inc, bgs_classes_kde.inc and
// bgs_classes_dp2.inc as they stand.
//
// Every wrapper re-reads ./config/<Class>.xml at the top of process() and hands the 0..255 integers to its model with
// setBGModelParameter on every frame (LB*.cpp:31-56): mirrored, loadConfig copies them into params_ every frame and the base
// class passes them on through bgs_set_params.  The wrappers return cv::Mat(m_pBGModel->GetFG()), an 8UC3 image whose three
// channels hold the mask byte: fg_channels_ = 3 makes the base class replicate the engine's one-byte mask the same way.

// package_bgs/lb/LBSimpleGaussian.{h,cpp} (USTC_BGS type 25)
class LBSimpleGaussian : public HipBGSBase {
 public:
  LBSimpleGaussian() : HipBGSBase(BGS_LB_SIMPLE_GAUSSIAN, "LBSimpleGaussian"), showOutput(true), sensitivity(66), noiseVariance(162), learningRate(18) { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBSimpleGaussian)
 private:
  bool showOutput;
  int sensitivity, noiseVariance, learningRate;
  void saveConfig() override {  // LBSimpleGaussian.cpp:78-88
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("sensitivity", sensitivity);
    fs.writeInt("noiseVariance", noiseVariance);
    fs.writeInt("learningRate", learningRate);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :90-99
    XmlConfig fs;
    fs.load(configPath());
    sensitivity = fs.readInt("sensitivity", 66);
    noiseVariance = fs.readInt("noiseVariance", 162);
    learningRate = fs.readInt("learningRate", 18);
    showOutput = fs.readInt("showOutput", true);
    params_.lb_sensitivity = sensitivity, params_.lb_noise_variance = noiseVariance, params_.lb_learning_rate = learningRate;
  }
};

// package_bgs/lb/LBFuzzyGaussian.{h,cpp} (USTC_BGS type 26)
class LBFuzzyGaussian : public HipBGSBase {
 public:
  LBFuzzyGaussian() : HipBGSBase(BGS_LB_FUZZY_GAUSSIAN, "LBFuzzyGaussian"), showOutput(true), sensitivity(72), bgThreshold(162), learningRate(49), noiseVariance(195) { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBFuzzyGaussian)
 private:
  bool showOutput;
  int sensitivity, bgThreshold, learningRate, noiseVariance;
  void saveConfig() override {  // LBFuzzyGaussian.cpp:79-91
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("sensitivity", sensitivity);
    fs.writeInt("bgThreshold", bgThreshold);
    fs.writeInt("learningRate", learningRate);
    fs.writeInt("noiseVariance", noiseVariance);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :93-104
    XmlConfig fs;
    fs.load(configPath());
    sensitivity = fs.readInt("sensitivity", 72);
    bgThreshold = fs.readInt("bgThreshold", 162);
    learningRate = fs.readInt("learningRate", 49);
    noiseVariance = fs.readInt("noiseVariance", 195);
    showOutput = fs.readInt("showOutput", true);
    params_.lb_sensitivity = sensitivity, params_.lb_bg_threshold = bgThreshold, params_.lb_learning_rate = learningRate, params_.lb_noise_variance = noiseVariance;
  }
};

// package_bgs/lb/LBMixtureOfGaussians.{h,cpp} (USTC_BGS type 27)
class LBMixtureOfGaussians : public HipBGSBase {
 public:
  LBMixtureOfGaussians() : HipBGSBase(BGS_LB_MOG, "LBMixtureOfGaussians"), showOutput(true), sensitivity(81), bgThreshold(83), learningRate(59), noiseVariance(206) { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBMixtureOfGaussians)
 private:
  bool showOutput;
  int sensitivity, bgThreshold, learningRate, noiseVariance;
  void saveConfig() override {  // LBMixtureOfGaussians.cpp:79-91
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("sensitivity", sensitivity);
    fs.writeInt("bgThreshold", bgThreshold);
    fs.writeInt("learningRate", learningRate);
    fs.writeInt("noiseVariance", noiseVariance);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :93-104
    XmlConfig fs;
    fs.load(configPath());
    sensitivity = fs.readInt("sensitivity", 81);
    bgThreshold = fs.readInt("bgThreshold", 83);
    learningRate = fs.readInt("learningRate", 59);
    noiseVariance = fs.readInt("noiseVariance", 206);
    showOutput = fs.readInt("showOutput", true);
    params_.lb_sensitivity = sensitivity, params_.lb_bg_threshold = bgThreshold, params_.lb_learning_rate = learningRate, params_.lb_noise_variance = noiseVariance;
  }
};

// package_bgs/lb/LBAdaptiveSOM.{h,cpp} (USTC_BGS type 28)
class LBAdaptiveSOM : public HipBGSBase {
 public:
  LBAdaptiveSOM() : HipBGSBase(BGS_LB_ADAPTIVE_SOM, "LBAdaptiveSOM"), showOutput(true), sensitivity(75), trainingSensitivity(245), learningRate(62), trainingLearningRate(255), trainingSteps(55) { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBAdaptiveSOM)
 private:
  bool showOutput;
  int sensitivity, trainingSensitivity, learningRate, trainingLearningRate, trainingSteps;
  void saveConfig() override {  // LBAdaptiveSOM.cpp:81-94
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("sensitivity", sensitivity);
    fs.writeInt("trainingSensitivity", trainingSensitivity);
    fs.writeInt("learningRate", learningRate);
    fs.writeInt("trainingLearningRate", trainingLearningRate);
    fs.writeInt("trainingSteps", trainingSteps);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :96-108
    XmlConfig fs;
    fs.load(configPath());
    sensitivity = fs.readInt("sensitivity", 75);
    trainingSensitivity = fs.readInt("trainingSensitivity", 245);
    learningRate = fs.readInt("learningRate", 62);
    trainingLearningRate = fs.readInt("trainingLearningRate", 255);
    trainingSteps = fs.readInt("trainingSteps", 55);
    showOutput = fs.readInt("showOutput", true);
    params_.lb_sensitivity = sensitivity, params_.lb_training_sensitivity = trainingSensitivity, params_.lb_learning_rate = learningRate, params_.lb_training_learning_rate = trainingLearningRate, params_.lb_training_steps = trainingSteps;
  }
};

// package_bgs/lb/LBFuzzyAdaptiveSOM.{h,cpp} (USTC_BGS type 29)
class LBFuzzyAdaptiveSOM : public HipBGSBase {
 public:
  LBFuzzyAdaptiveSOM() : HipBGSBase(BGS_LB_FUZZY_ADAPTIVE_SOM, "LBFuzzyAdaptiveSOM"), showOutput(true), sensitivity(90), trainingSensitivity(240), learningRate(38), trainingLearningRate(255), trainingSteps(81) { fg_channels_ = 3; }
  BGS_HIP_BANNER_DTOR(LBFuzzyAdaptiveSOM)
 private:
  bool showOutput;
  int sensitivity, trainingSensitivity, learningRate, trainingLearningRate, trainingSteps;
  void saveConfig() override {  // LBFuzzyAdaptiveSOM.cpp:81-94
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("sensitivity", sensitivity);
    fs.writeInt("trainingSensitivity", trainingSensitivity);
    fs.writeInt("learningRate", learningRate);
    fs.writeInt("trainingLearningRate", trainingLearningRate);
    fs.writeInt("trainingSteps", trainingSteps);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :96-108
    XmlConfig fs;
    fs.load(configPath());
    sensitivity = fs.readInt("sensitivity", 90);
    trainingSensitivity = fs.readInt("trainingSensitivity", 240);
    learningRate = fs.readInt("learningRate", 38);
    trainingLearningRate = fs.readInt("trainingLearningRate", 255);
    trainingSteps = fs.readInt("trainingSteps", 81);
    showOutput = fs.readInt("showOutput", true);
    params_.lb_sensitivity = sensitivity, params_.lb_training_sensitivity = trainingSensitivity, params_.lb_learning_rate = learningRate, params_.lb_training_learning_rate = trainingLearningRate, params_.lb_training_steps = trainingSteps;
  }
};
