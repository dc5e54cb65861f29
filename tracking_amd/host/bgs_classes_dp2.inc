// bgs_classes_dp2.inc — the two package_bgs/dp IBGS classes with a neighbourhood step (USTC_BGS types 14 and 16), written against
// the same four names as bgs_classes.inc and included right after bgs_classes_kde.inc by tracking_amd/host/bgs_host.h and
// tracking_amd/host/HipBGS.h.  A file of its own: tests/test_capi_cpu.py pins bgs_classes.inc and tests/test_kde_cpu.py
// bgs_classes_kde.inc as they stand.

// package_bgs/dp/DPPratiMediodBGS.{h,cpp} (USTC_BGS type 14).  loadConfig runs every frame, but the wrapper hands threshold,
// samplingRate, historySize and weight to its model once, on the first frame (DPPratiMediodBGS.cpp:48-65); mirrored: they go into
// params_ only while firstTime is true (the engine keeps them from then on anyway).  weight is saved and never read.
class DPPratiMediodBGS : public HipBGSBase {
 public:
  DPPratiMediodBGS()
      : HipBGSBase(BGS_DP_PRATI_MEDIOD, "DPPratiMediodBGS"), threshold(30), samplingRate(5), historySize(16), weight(5), showOutput(true) {}
  BGS_HIP_BANNER_DTOR(DPPratiMediodBGS)
 private:
  int threshold, samplingRate, historySize, weight;
  bool showOutput;
  void saveConfig() override {  // DPPratiMediodBGS.cpp:83-94
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("threshold", threshold);
    fs.writeInt("samplingRate", samplingRate);
    fs.writeInt("historySize", historySize);
    fs.writeInt("weight", weight);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :96-107
    XmlConfig fs;
    fs.load(configPath());
    threshold = fs.readInt("threshold", 30);
    samplingRate = fs.readInt("samplingRate", 5);
    historySize = fs.readInt("historySize", 16);
    weight = fs.readInt("weight", 5);
    showOutput = fs.readInt("showOutput", true);
    if (firstTime) {
      params_.dp_threshold = (float)threshold, params_.dp_sampling_rate = samplingRate;
      params_.dp_history_size = historySize, params_.dp_weight = weight;
    }
  }
};

// package_bgs/dp/DPTextureBGS.{h,cpp} (USTC_BGS type 16): no run-time parameters (REGION_R, HYSTERSIS, ALPHA and THRESHOLD are
// constants of TextureBGS.h); the XML holds showOutput only.
class DPTextureBGS : public HipBGSBase {
 public:
  DPTextureBGS() : HipBGSBase(BGS_DP_TEXTURE, "DPTextureBGS"), showOutput(true) {}
  BGS_HIP_BANNER_DTOR(DPTextureBGS)
 private:
  bool showOutput;
  void saveConfig() override {  // DPTextureBGS.cpp:136-145
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :147-156
    XmlConfig fs;
    fs.load(configPath());
    showOutput = fs.readInt("showOutput", true);
  }
};
