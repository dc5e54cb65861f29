// bgs_classes_t2f.inc — the IBGS classes of package_bgs/tb's type-2 fuzzy GMMs, in the form bgs_classes.inc describes.

// package_bgs/tb/T2FGMM_UM.{h,cpp} and T2FGMM_UV.{h,cpp} (USTC_BGS types 17 and 18): the same file twice, the one difference being
// params.Type().  loadConfig runs every frame into members of the wrapper's own types (double threshold / alpha, float km / kv, int
// gaussians), but the values reach the model object once, `if(firstTime)`: they travel in bgs_t2f_params, which the engine takes
// when its model is built and keeps (a later bgs_set_t2f_params succeeds and changes nothing).  8UC1 high-threshold mask from the
// first frame on; img_bgmodel is never written.
class T2FGMMBase : public HipBGSBase {
 protected:
  T2FGMMBase(bgs_algo algo, const char* name) : HipBGSBase(algo, name) {}
  double threshold, alpha;
  float km, kv;
  int gaussians;
  bool showOutput;
  int applyClassParams(bgs_engine* engine) override {
    bgs_t2f_params p;
    bgs_t2f_default_params(&p);
    p.threshold = threshold, p.alpha = alpha, p.km = km, p.kv = kv, p.gaussians = gaussians;
    return bgs_set_t2f_params(engine, &p);
  }

 private:
  void describe(XmlIo& io) override {  // T2FGMM_U*.cpp:85-111
    io("threshold", threshold, 9.0);
    io("alpha", alpha, 0.01);
    io("km", km, 1.5);
    io("kv", kv, 0.6);
    io("gaussians", gaussians, 3);
    io("showOutput", showOutput, true);
  }
};

class T2FGMM_UM : public T2FGMMBase {
 public:
  T2FGMM_UM() : T2FGMMBase(BGS_T2FGMM_UM, "T2FGMM_UM") {}
  BGS_HIP_BANNER_DTOR(T2FGMM_UM)
};

class T2FGMM_UV : public T2FGMMBase {
 public:
  T2FGMM_UV() : T2FGMMBase(BGS_T2FGMM_UV, "T2FGMM_UV") {}
  BGS_HIP_BANNER_DTOR(T2FGMM_UV)
};
