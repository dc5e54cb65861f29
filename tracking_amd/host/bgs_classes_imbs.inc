// bgs_classes_imbs.inc — the IBGS class of package_bgs/db's IMBS, in the form bgs_classes.inc describes.

// package_bgs/db/IndependentMultimodalBGS.{h,cpp} (USTC_BGS type 33).  The wrapper constructs BackgroundSubtractorIMBS(fps) with
// fps 10 and every other argument at the full constructor's default; its XML holds showOutput only.  8UC1 mask with the four labels
// 0 / 80 / 180 / 255 and the BGR background of the last model build; zero images until the first model is built (the reference
// shows a putText banner there).
class IndependentMultimodalBGS : public HipBGSBase {
 public:
  IndependentMultimodalBGS() : HipBGSBase(BGS_IMBS, "IndependentMultimodalBGS"), fps(10) {}
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
  void describe(XmlIo& io) override { io("showOutput", showOutput, true); }  // IndependentMultimodalBGS.cpp:38-54
};
