// bgs_classes_fuzzy.inc — the IBGS classes of package_bgs/tb's fuzzy integrals, in the form bgs_classes.inc describes.

// package_bgs/tb/FuzzySugenoIntegral.{h,cpp} and FuzzyChoquetIntegral.{h,cpp} (USTC_BGS types 21 and 22): the same file twice, the one
// difference being getFuzzyIntegralSugeno / getFuzzyIntegralChoquet.  loadConfig runs every frame and all seven values act on that
// frame; they travel in bgs_fuzzy_params (bgs_set_fuzzy_params before every frame), not in bgs_params.  No mask and no background
// model during the framesToLearn + 1 learning frames (img_output / img_bgmodel untouched); then an 8UC1 mask and an 8UC3 model.
class FuzzyIntegralBase : public HipBGSBase {
 protected:
  FuzzyIntegralBase(bgs_algo algo, const char* name) : HipBGSBase(algo, name) { bgs_fuzzy_default_params(&fuzzy_); }
  bgs_fuzzy_params fuzzy_;
  bool showOutput;
  int applyClassParams(bgs_engine* engine) override { return bgs_set_fuzzy_params(engine, &fuzzy_); }

 private:
  void describe(XmlIo& io) override {  // Fuzzy*Integral.cpp:175-205
    io("showOutput", showOutput, true);
    io("framesToLearn", fuzzy_.frames_to_learn, 10);
    io("alphaLearn", fuzzy_.alpha_learn, 0.1);
    io("alphaUpdate", fuzzy_.alpha_update, 0.01);
    io("colorSpace", fuzzy_.color_space, 1);
    io("option", fuzzy_.option, 2);
    io("smooth", fuzzy_.smooth, true);
    io("threshold", fuzzy_.threshold, 0.67);
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
