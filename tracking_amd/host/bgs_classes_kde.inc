// bgs_classes_kde.inc — the IBGS class of package_bgs/ae (KDE), in the form bgs_classes.inc describes.

// package_bgs/ae/KDE.{h,cpp} (USTC_BGS type 32).  loadConfig runs every frame, but the wrapper hands SequenceLength,
// TimeWindowSize, SDEstimationFlag, lUseColorRatiosFlag, th and alpha to its model once, on the first frame (KDE.cpp:40-66); the
// engine keeps them from then on (bgs_set_params) and re-reads only framesToLearn, as the wrapper does.  The model always adapts
// (kde_update_model 1): the reference leaves NPBGSubtractor::UpdateBGFlag uninitialised (DESIGN.md §5).
class KDE : public HipBGSBase {
 public:
  KDE() : HipBGSBase(BGS_KDE, "KDE") {}
  BGS_HIP_BANNER_DTOR(KDE)
 private:
  bool showOutput;
  void describe(XmlIo& io) override {  // KDE.cpp:98-126
    io("framesToLearn", params_.kde_frames_to_learn, 10);
    io("SequenceLength", params_.kde_sequence_length, 50);
    io("TimeWindowSize", params_.kde_time_window, 100);
    io("SDEstimationFlag", params_.kde_sd_estimation, 1);
    io("lUseColorRatiosFlag", params_.kde_color_ratios, 1);
    io("th", params_.kde_threshold, 10e-8);
    io("alpha", params_.kde_alpha, 0.3);
    io("showOutput", showOutput, true);
  }
};
