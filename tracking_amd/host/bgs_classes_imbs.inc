// bgs_classes_imbs.inc — the IBGS class of package_bgs/db's IMBS, written against the same names as bgs_classes.inc and included
// after bgs_classes_eigen.inc by tracking_amd/host/bgs_host.h and tracking_amd/host/HipBGS.h.  A file of its own: the tests pin the
// class lists of the other .inc files as they stand.

// package_bgs/db/IndependentMultimodalBGS.{h,cpp} (USTC_BGS type 33).  The wrapper constructs BackgroundSubtractorIMBS(fps) with
// fps 10 and every other argument at the full constructor's default; its XML holds showOutput only.  8UC1 mask with the four labels
// 0 / 80 / 180 / 255 and the BGR background of the last model build; zero images until the first model is built (the reference
// shows a putText banner there).
class IndependentMultimodalBGS : public HipBGSBase {
 public:
  IndependentMultimodalBGS() : HipBGSBase(BGS_IMBS, "IndependentMultimodalBGS"), fps(10), showOutput(true) {}
  BGS_HIP_BANNER_DTOR(IndependentMultimodalBGS)

 protected:
  double fps;
  bool showOutput;
  int applyClassParams(bgs_engine* engine) override {
    bgs_imbs_params p;
    bgs_imbs_default_params(&p);
    p.fps = fps;
    return bgs_set_imbs_params(engine, &p);
  }

 private:
  void saveConfig() override {  // IndependentMultimodalBGS.cpp:38-45
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("showOutput", showOutput);
    fs.save(configPath());
  }
  void loadConfig() override {  // :47-54
    XmlConfig fs;
    fs.load(configPath());
    showOutput = fs.readInt("showOutput", true);
  }
};
