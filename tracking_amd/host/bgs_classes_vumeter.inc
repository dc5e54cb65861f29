// bgs_classes_vumeter.inc — the IBGS class of package_bgs/av (VuMeter), in the form bgs_classes.inc describes.

// package_bgs/av/VuMeter.{h,cpp} (USTC_BGS type 31).  loadConfig runs every frame, but the wrapper hands binSize, alpha and
// threshold to its model once, on the first frame, through setters that replace out-of-range values (VuMeter.cpp:42-47,
// TBackgroundVuMeter.h:47-54); the engine does both (bgs_set_params keeps the three) and re-reads only enableFilter, as the wrapper
// does.  Mask and background model are 8UC1 (the background is the gray image the model keeps).
class VuMeter : public HipBGSBase {
 public:
  VuMeter() : HipBGSBase(BGS_VUMETER, "VuMeter") {}
  BGS_HIP_BANNER_DTOR(VuMeter)
 private:
  bool showOutput;
  int bgChannels(int) const override { return 1; }
  void describe(XmlIo& io) override {  // VuMeter.cpp:88-116
    io("enableFilter", params_.vu_enable_filter, true);
    io("binSize", params_.vu_bin_size, 8);
    io("alpha", params_.vu_alpha, 0.995);
    io("threshold", params_.vu_threshold, 0.03);
    io("showOutput", showOutput, true);
  }
};
