// bgs_classes_vumeter.inc — the IBGS class of package_bgs/av (VuMeter), written against the same four names as bgs_classes.inc and
// included after bgs_classes_lb.inc by tracking_amd/host/bgs_host.h and tracking_amd/host/HipBGS.h.  A file of its own: the tests
// pin the class lists of the other .inc files as they stand; type 31 came later.

// package_bgs/av/VuMeter.{h,cpp} (USTC_BGS type 31).  loadConfig runs every frame, but the wrapper hands binSize, alpha and
// threshold to its model once, on the first frame, through setters that replace out-of-range values (VuMeter.cpp:42-47,
// TBackgroundVuMeter.h:47-54); the engine does both (bgs_set_params keeps the three) and re-reads only enableFilter, as the wrapper
// does.  Mask and background model are 8UC1 (the background is the gray image the model keeps).
class VuMeter : public HipBGSBase {
 public:
  VuMeter() : HipBGSBase(BGS_VUMETER, "VuMeter"), showOutput(true) {}
  BGS_HIP_BANNER_DTOR(VuMeter)
 private:
  bool showOutput;
  void saveConfig() override {  // VuMeter.cpp:88-101
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("enableFilter", params_.vu_enable_filter);
    fs.writeInt("binSize", params_.vu_bin_size);
    fs.writeReal("alpha", params_.vu_alpha);
    fs.writeReal("threshold", params_.vu_threshold);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :103-116
    XmlConfig fs;
    fs.load(configPath());
    params_.vu_enable_filter = fs.readInt("enableFilter", true);
    params_.vu_bin_size = fs.readInt("binSize", 8);
    params_.vu_alpha = fs.readReal("alpha", 0.995);
    params_.vu_threshold = fs.readReal("threshold", 0.03);
    showOutput = fs.readInt("showOutput", true);
  }
};
