// bgs_classes_fuzzy.inc — the IBGS classes of package_bgs/tb's fuzzy integrals, written against the same names as bgs_classes.inc and
// included after bgs_classes_vumeter.inc by tracking_amd/host/bgs_host.h and tracking_amd/host/HipBGS.h.  A file of its own: the tests
// pin the class lists of the other .inc files as they stand; types 21 and 22 came later.

// package_bgs/tb/FuzzySugenoIntegral.{h,cpp} and FuzzyChoquetIntegral.{h,cpp} (USTC_BGS types 21 and 22): the same file twice, the one
// difference being getFuzzyIntegralSugeno / getFuzzyIntegralChoquet.  loadConfig runs every frame and all seven values act on that
// frame; they travel in bgs_fuzzy_params (bgs_set_fuzzy_params before every frame), not in bgs_params.  No mask and no background
// model during the framesToLearn + 1 learning frames (img_output / img_bgmodel untouched); then an 8UC1 mask and an 8UC3 model.
class FuzzyIntegralBase : public HipBGSBase {
 protected:
  FuzzyIntegralBase(bgs_algo algo, const char* name) : HipBGSBase(algo, name), showOutput(true) { bgs_fuzzy_default_params(&fuzzy_); }
  bgs_fuzzy_params fuzzy_;
  bool showOutput;
  int applyClassParams(bgs_engine* engine) override { return bgs_set_fuzzy_params(engine, &fuzzy_); }

 private:
  void saveConfig() override {  // Fuzzy*Integral.cpp:175-189
    XmlConfig fs;
    fs.beginWrite();
    fs.writeInt("showOutput", showOutput);
    fs.writeInt("framesToLearn", fuzzy_.frames_to_learn);
    fs.writeReal("alphaLearn", fuzzy_.alpha_learn);
    fs.writeReal("alphaUpdate", fuzzy_.alpha_update);
    fs.writeInt("colorSpace", fuzzy_.color_space);
    fs.writeInt("option", fuzzy_.option);
    fs.writeInt("smooth", fuzzy_.smooth);
    fs.writeReal("threshold", fuzzy_.threshold);
    fs.save(configPath());
  }
  void loadConfig() override {  // :191-205
    XmlConfig fs;
    fs.load(configPath());
    showOutput = fs.readInt("showOutput", true);
    fuzzy_.frames_to_learn = fs.readInt("framesToLearn", 10);
    fuzzy_.alpha_learn = fs.readReal("alphaLearn", 0.1);
    fuzzy_.alpha_update = fs.readReal("alphaUpdate", 0.01);
    fuzzy_.color_space = fs.readInt("colorSpace", 1);
    fuzzy_.option = fs.readInt("option", 2);
    fuzzy_.smooth = fs.readInt("smooth", true);
    fuzzy_.threshold = fs.readReal("threshold", 0.67);
  }
};

class FuzzySugenoIntegral : public FuzzyIntegralBase {
 public:
  FuzzySugenoIntegral() : FuzzyIntegralBase(BGS_FUZZY_SUGENO, "FuzzySugenoIntegral") {}
  BGS_HIP_BANNER_DTOR(FuzzySugenoIntegral)
};

class FuzzyChoquetIntegral : public FuzzyIntegralBase {
 public:
  FuzzyChoquetIntegral() : FuzzyIntegralBase(BGS_FUZZY_CHOQUET, "FuzzyChoquetIntegral") {}
  BGS_HIP_BANNER_DTOR(FuzzyChoquetIntegral)
};
