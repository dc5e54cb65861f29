// bgs_classes_multicue.inc — the IBGS class of package_bgs/sjn's SJN_MultiCueBGS.  Unlike the classes of the other files this one has no
// bgs_algo and no bgs_engine: it holds a one-stream bgs_multicue (include/bgs_hip.h), so it derives from IBGS itself and shares only
// the description of its XML (bgs_describe.inc).  The including header names its image type, the 8UC3 type code of that image's
// create() and its one way to fail: BGS_HIP_MAT, BGS_HIP_8UC3, BGS_HIP_FAIL(code, what).

// package_bgs/sjn/SJN_MultiCueBGS.{h,cpp} (USTC_BGS type 34).  The parameters are the constructor's (SJN_MultiCueBGS.cpp:30-48) and no XML
// key changes them; ./config/MultiCueBGS.xml holds showOutput only.  8UC3 mask with three equal channels, zero while the model trains
// (frames 0 .. 20); img_bgmodel is left untouched, as the reference leaves it.  The reference prints no constructor or destructor banner.
class SJN_MultiCueBGS : public IBGS, protected XmlDescribed {
 public:
  SJN_MultiCueBGS() : firstTime(true), device_(0), model_(0) {}
  ~SJN_MultiCueBGS() {
    if (model_) bgs_multicue_destroy(model_);
  }
  void process(const BGS_HIP_MAT& img_input, BGS_HIP_MAT& img_output, BGS_HIP_MAT& img_bgmodel) {  // SJN_MultiCueBGS.cpp:69-113
    (void)img_bgmodel;
    if (img_input.empty()) return;
    loadConfig();
    if (firstTime) saveConfig();
    if (img_input.channels() != 3) BGS_HIP_FAIL(BGS_ERR_UNSUPPORTED, std::string("SJN_MultiCueBGS: 3-channel frames only"));
    if (!model_) {
      bgs_multicue_params p;
      bgs_multicue_default_params(&p);
      int rc = bgs_multicue_create(device_, 1, &p, &model_);
      if (rc) BGS_HIP_FAIL(rc, std::string("SJN_MultiCueBGS: ") + bgs_last_error());
    }
    img_output.create(img_input.rows, img_input.cols, BGS_HIP_8UC3);  // temp.copyTo(img_output), :102-103
    int rc = bgs_multicue_process(model_, 0, img_input.data, img_input.rows, img_input.cols, (size_t)img_input.step, img_output.data, (size_t)img_output.step, 3);
    if (rc) BGS_HIP_FAIL(rc, std::string("SJN_MultiCueBGS: ") + bgs_last_error());
    firstTime = false;
  }
  void setDevice(int d) { device_ = d; }  // which HIP device the lazily created model uses (default 0); the reference has no such notion

 private:
  bool firstTime, showOutput;
  int device_;
  bgs_multicue* model_;
  void describe(XmlIo& io) override { io("showOutput", showOutput, true); }  // :115-131
  void saveConfig() { saveDescribed("./config/MultiCueBGS.xml"); }
  void loadConfig() { loadDescribed("./config/MultiCueBGS.xml"); }
  SJN_MultiCueBGS(const SJN_MultiCueBGS&);  // owns the handle: not copied
  SJN_MultiCueBGS& operator=(const SJN_MultiCueBGS&);
};
