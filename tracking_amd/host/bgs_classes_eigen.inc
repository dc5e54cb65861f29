// bgs_classes_eigen.inc — the IBGS class of package_bgs/dp's Eigenbackground, in the form bgs_classes.inc describes.

// package_bgs/dp/DPEigenbackgroundBGS.{h,cpp} (USTC_BGS type 15).  loadConfig runs every frame into the wrapper's int members, but the
// values reach the params object once, `if(firstTime)`: they travel in bgs_eigen_params, which the engine takes when its model is
// built and keeps (a later bgs_set_eigen_params succeeds and changes nothing).  8UC1 high-threshold mask, all background for the
// first historySize frames; img_bgmodel is never written.
class DPEigenbackgroundBGS : public HipBGSBase {
 public:
  DPEigenbackgroundBGS() : HipBGSBase(BGS_DP_EIGENBACKGROUND, "DPEigenbackgroundBGS") {}
  BGS_HIP_BANNER_DTOR(DPEigenbackgroundBGS)

 protected:
  int threshold, historySize, embeddedDim;
  bool showOutput;
  int applyClassParams(bgs_engine* engine) override {
    bgs_eigen_params p;
    bgs_eigen_default_params(&p);
    p.threshold = threshold, p.history_size = historySize, p.embedded_dim = embeddedDim;
    return bgs_set_eigen_params(engine, &p);
  }

 private:
  void describe(XmlIo& io) override {  // DPEigenbackgroundBGS.cpp:84-106
    io("threshold", threshold, 225);
    io("historySize", historySize, 20);
    io("embeddedDim", embeddedDim, 10);
    io("showOutput", showOutput, true);
  }
};
