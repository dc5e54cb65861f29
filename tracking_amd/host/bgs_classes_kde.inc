// bgs_classes_kde.inc — the IBGS class of package_bgs/ae (KDE), written against the same four names as bgs_classes.inc and
// included right after it by tracking_amd/host/bgs_host.h and tracking_amd/host/HipBGS.h.  A file of its own: bgs_classes.inc is
// the class list of USTC_BGS types 0-13 and 35-37 (tests/test_capi_cpu.py pins it as it stands); type 32 came later.

// package_bgs/ae/KDE.{h,cpp} (USTC_BGS type 32).  loadConfig runs every frame, but the wrapper hands SequenceLength,
// TimeWindowSize, SDEstimationFlag, lUseColorRatiosFlag, th and alpha to its model once, on the first frame (KDE.cpp:40-66); the
// engine keeps them from then on (bgs_set_params) and re-reads only framesToLearn, as the wrapper does.  The model always adapts
// (kde_update_model 1): the reference leaves NPBGSubtractor::UpdateBGFlag uninitialised (DESIGN.md §5).
class KDE : public HipBGSBase {
 public:
  KDE() : HipBGSBase(BGS_KDE, "KDE"), showOutput(true) {}
  BGS_HIP_BANNER_DTOR(KDE)
 private:
  bool showOutput;
  void saveConfig() override {  // KDE.cpp:98-112
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("framesToLearn", params_.kde_frames_to_learn);
    fs.writeInt("SequenceLength", params_.kde_sequence_length);
    fs.writeInt("TimeWindowSize", params_.kde_time_window);
    fs.writeInt("SDEstimationFlag", params_.kde_sd_estimation);
    fs.writeInt("lUseColorRatiosFlag", params_.kde_color_ratios);
    fs.writeReal("th", params_.kde_threshold);
    fs.writeReal("alpha", params_.kde_alpha);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :114-126
    XmlConfig fs;
    fs.load(configPath());
    params_.kde_frames_to_learn = fs.readInt("framesToLearn", 10);
    params_.kde_sequence_length = fs.readInt("SequenceLength", 50);
    params_.kde_time_window = fs.readInt("TimeWindowSize", 100);
    params_.kde_sd_estimation = fs.readInt("SDEstimationFlag", 1);
    params_.kde_color_ratios = fs.readInt("lUseColorRatiosFlag", 1);
    params_.kde_threshold = fs.readReal("th", 10e-8);
    params_.kde_alpha = fs.readReal("alpha", 0.3);
    showOutput = fs.readInt("showOutput", true);
  }
};
