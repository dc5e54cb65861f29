// bgs_classes_multilayer.inc — the IBGS class of package_bgs/jmo's MultiLayerBGS, in the form bgs_classes.inc describes.

// package_bgs/jmo/MultiLayerBGS.{h,cpp} (USTC_BGS type 23).  loadConfig runs every frame, but the values reach CMultiLayerBGS once,
// `if(firstTime)`: they travel in bgs_multilayer_params, which the engine takes when its model is built and keeps (a later
// bgs_set_multilayer_params succeeds and changes nothing), so setStatus after the first frame changes nothing either, as in the
// reference.  With loadDefaultParams (the default) the hard-coded block of MultiLayerBGS.cpp:110-186 replaces what the XML holds.
// The switch at detectAfter is the engine's: it counts the stream's frames as the wrapper's frameNumber does.  8UC1 mask, zero on the
// first frame, and the BGR background of the first-ranked mode.  Not offered: preloadModel / saveModel (refused when set), the
// bilateral sigmas (read and written for the XML's sake; LINUX_BILATERAL_FILTER is compiled out in the reference).  The preloadModel
// string is read and written where the including header's XmlConfig has strings (bgs_host.h: BGS_HIP_XML_HAS_STRINGS); HipBGS.h's has
// integers and reals only and leaves the key alone.
class MultiLayerBGS : public HipBGSBase {
 public:
  enum Status { MLBGS_NONE = -1, MLBGS_LEARN = 0, MLBGS_DETECT = 1 };
  MultiLayerBGS() : HipBGSBase(BGS_MULTILAYER, "MultiLayerBGS"), status(MLBGS_NONE) {}
  BGS_HIP_BANNER_DTOR(MultiLayerBGS)
  void setStatus(Status _status) { status = _status; }  // MultiLayerBGS.cpp:31-34

 protected:
  Status status;
  bool showOutput, saveModel, disableDetectMode, disableLearning;
  int detectAfter;
  std::string bg_model_preload;
  bool loadDefaultParams;
  int max_mode_num;
  float weight_updating_constant, texture_weight, bg_mode_percent;
  int pattern_neig_half_size;
  float pattern_neig_gaus_sigma, bg_prob_threshold, bg_prob_updating_threshold;
  int robust_LBP_constant;
  float min_noised_angle, shadow_rate, highlight_rate, bilater_filter_sigma_s, bilater_filter_sigma_r, frame_duration;
  float learn_mode_learn_rate_per_second, learn_weight_learn_rate_per_second, learn_init_mode_weight;
  float detect_mode_learn_rate_per_second, detect_weight_learn_rate_per_second, detect_init_mode_weight;
  int applyClassParams(bgs_engine* engine) override {
    if (!bg_model_preload.empty() || saveModel) {  // CMultiLayerBGS::Load / Save and their file format are out of scope
      std::cout << "MultiLayerBGS: preloadModel / saveModel are not offered" << std::endl;
      return BGS_ERR_UNSUPPORTED;
    }
    bgs_multilayer_params p;
    bgs_multilayer_default_params(&p);  // the loadDefaultParams block
    if (!loadDefaultParams) {
      p.max_mode_num = max_mode_num, p.weight_updating_constant = weight_updating_constant, p.texture_weight = texture_weight, p.bg_mode_percent = bg_mode_percent;
      p.pattern_neig_half_size = pattern_neig_half_size, p.pattern_neig_gaus_sigma = pattern_neig_gaus_sigma;
      p.bg_prob_threshold = bg_prob_threshold, p.bg_prob_updating_threshold = bg_prob_updating_threshold, p.robust_LBP_constant = robust_LBP_constant;
      p.min_noised_angle = min_noised_angle, p.shadow_rate = shadow_rate, p.highlight_rate = highlight_rate, p.frame_duration = frame_duration;
      p.learn_mode_learn_rate_per_second = learn_mode_learn_rate_per_second, p.learn_weight_learn_rate_per_second = learn_weight_learn_rate_per_second;
      p.learn_init_mode_weight = learn_init_mode_weight, p.detect_mode_learn_rate_per_second = detect_mode_learn_rate_per_second;
      p.detect_weight_learn_rate_per_second = detect_weight_learn_rate_per_second, p.detect_init_mode_weight = detect_init_mode_weight;
    }
    p.status = status == MLBGS_DETECT, p.disable_detect_mode = disableDetectMode, p.disable_learning = disableLearning, p.detect_after = detectAfter;
    return bgs_set_multilayer_params(engine, &p);
  }

 private:
  void describe(XmlIo& io) override {  // MultiLayerBGS.cpp:251-331
#ifdef BGS_HIP_XML_HAS_STRINGS
    io("preloadModel", bg_model_preload, "");
#endif
    io("saveModel", saveModel, false);
    io("detectAfter", detectAfter, 0);
    io("disableDetectMode", disableDetectMode, true);
    io("disableLearningInDetecMode", disableLearning, false);
    io("loadDefaultParams", loadDefaultParams, true);
    io("max_mode_num", max_mode_num, 5);
    io("weight_updating_constant", weight_updating_constant, 5.0);
    io("texture_weight", texture_weight, 0.5);
    io("bg_mode_percent", bg_mode_percent, 0.6);
    io("pattern_neig_half_size", pattern_neig_half_size, 4);
    io("pattern_neig_gaus_sigma", pattern_neig_gaus_sigma, 3.0);
    io("bg_prob_threshold", bg_prob_threshold, 0.2);
    io("bg_prob_updating_threshold", bg_prob_updating_threshold, 0.2);
    io("robust_LBP_constant", robust_LBP_constant, 3);
    io("min_noised_angle", min_noised_angle, 0.01768);
    io("shadow_rate", shadow_rate, 0.6);
    io("highlight_rate", highlight_rate, 1.2);
    io("bilater_filter_sigma_s", bilater_filter_sigma_s, 3.0);
    io("bilater_filter_sigma_r", bilater_filter_sigma_r, 0.1);
    io("frame_duration", frame_duration, 0.1);
    io("learn_mode_learn_rate_per_second", learn_mode_learn_rate_per_second, 0.5);
    io("learn_weight_learn_rate_per_second", learn_weight_learn_rate_per_second, 0.5);
    io("learn_init_mode_weight", learn_init_mode_weight, 0.05);
    io("detect_mode_learn_rate_per_second", detect_mode_learn_rate_per_second, 0.01);
    io("detect_weight_learn_rate_per_second", detect_weight_learn_rate_per_second, 0.01);
    io("detect_init_mode_weight", detect_init_mode_weight, 0.001);
    io("showOutput", showOutput, true);
  }
  void loaded() override {
    if (loadDefaultParams) {  // :110-128, :147-152: the hard-coded block replaces what was read, and is what the first frame saves
      max_mode_num = 5, weight_updating_constant = 5.0f, texture_weight = 0.5f, bg_mode_percent = 0.6f, pattern_neig_half_size = 4;
      pattern_neig_gaus_sigma = 3.0f, bg_prob_threshold = 0.2f, bg_prob_updating_threshold = 0.2f, robust_LBP_constant = 3;
      min_noised_angle = (float)(10.0 / 180.0 * 3.141592653589793f), shadow_rate = 0.6f, highlight_rate = 1.2f;
      bilater_filter_sigma_s = 3.0f, bilater_filter_sigma_r = 0.1f, frame_duration = 1.0f / 10.0f;
    }
  }
};
