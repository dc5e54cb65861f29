// bgs_classes_dp2.inc — the two package_bgs/dp IBGS classes with a neighbourhood step (USTC_BGS types 14 and 16), in the form
// bgs_classes.inc describes.

// package_bgs/dp/DPPratiMediodBGS.{h,cpp} (USTC_BGS type 14).  loadConfig runs every frame, but the wrapper hands threshold,
// samplingRate, historySize and weight to its model once, on the first frame (DPPratiMediodBGS.cpp:48-65); mirrored: they go into
// params_ only while firstTime is true (the engine keeps them from then on anyway).  weight is saved and never read.
class DPPratiMediodBGS : public HipBGSBase {
 public:
  DPPratiMediodBGS() : HipBGSBase(BGS_DP_PRATI_MEDIOD, "DPPratiMediodBGS") {}
  BGS_HIP_BANNER_DTOR(DPPratiMediodBGS)
 private:
  int threshold, samplingRate, historySize, weight;
  bool showOutput;
  void describe(XmlIo& io) override {  // DPPratiMediodBGS.cpp:83-107
    io("threshold", threshold, 30);
    io("samplingRate", samplingRate, 5);
    io("historySize", historySize, 16);
    io("weight", weight, 5);
    io("showOutput", showOutput, true);
  }
  void loaded() override {
    if (!firstTime) return;
    params_.dp_threshold = (float)threshold, params_.dp_sampling_rate = samplingRate;
    params_.dp_history_size = historySize, params_.dp_weight = weight;
  }
};

// package_bgs/dp/DPTextureBGS.{h,cpp} (USTC_BGS type 16): no run-time parameters (REGION_R, HYSTERSIS, ALPHA and THRESHOLD are
// constants of TextureBGS.h); the XML holds showOutput only.
class DPTextureBGS : public HipBGSBase {
 public:
  DPTextureBGS() : HipBGSBase(BGS_DP_TEXTURE, "DPTextureBGS") {}
  BGS_HIP_BANNER_DTOR(DPTextureBGS)
 private:
  bool showOutput;
  void describe(XmlIo& io) override { io("showOutput", showOutput, true); }  // DPTextureBGS.cpp:136-156
};
