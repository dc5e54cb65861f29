// bgs_classes_eigen.inc — the IBGS class of package_bgs/dp's Eigenbackground, written against the same names as bgs_classes.inc and
// included after bgs_classes_t2f.inc by tracking_amd/host/bgs_host.h and tracking_amd/host/HipBGS.h.  A file of its own: the tests
// pin the class lists of the other .inc files as they stand.

// package_bgs/dp/DPEigenbackgroundBGS.{h,cpp} (USTC_BGS type 15).  loadConfig runs every frame into the wrapper's int members, but the
// values reach the params object once, `if(firstTime)`: they travel in bgs_eigen_params, which the engine takes when its model is
// built and keeps (a later bgs_set_eigen_params succeeds and changes nothing).  8UC1 high-threshold mask, all background for the
// first historySize frames; img_bgmodel is never written.
class DPEigenbackgroundBGS : public HipBGSBase {
 public:
  DPEigenbackgroundBGS() : HipBGSBase(BGS_DP_EIGENBACKGROUND, "DPEigenbackgroundBGS"), threshold(225), historySize(20), embeddedDim(10), showOutput(true) {}
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
  void saveConfig() override {  // DPEigenbackgroundBGS.cpp:84-94
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("threshold", threshold);
    fs.writeInt("historySize", historySize);
    fs.writeInt("embeddedDim", embeddedDim);
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :96-106
    XmlConfig fs;
    fs.load(configPath());
    threshold = fs.readInt("threshold", 225);
    historySize = fs.readInt("historySize", 20);
    embeddedDim = fs.readInt("embeddedDim", 10);
    showOutput = fs.readInt("showOutput", true);
  }
};
