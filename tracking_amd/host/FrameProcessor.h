// FrameProcessor.h — host-side mirror of bgslibrary::FrameProcessor (FrameProcessor.{h,cpp}) for the classes on the hot path.
//
//   IFrameProcessor::process(const Image&)            IFrameProcessor.h:23-28
//   FrameProcessor::init / process / finish           FrameProcessor.cpp:35-155, 169-340, 342-482
//   per-algorithm helper with tic/toc                 FrameProcessor.cpp:157-167, 484-494
//   ./config/FrameProcessor.xml (tictoc + enable*)    FrameProcessor.cpp:496-610
//
// Same control flow as the reference: one IBGS instance per enabled class, created in init(), fed the same
// pre-processed frame in the reference's order, one mask per class kept in a member image.  The PreProcessor (PreProcessor.h:
// copy, optional equalizeHist / GaussianBlur from ./config/PreProcessor.xml) is created in init() like the reference's (:37-38).
// What the reference spells out per class in seven places is one line of FrameProcessor::classes here (FrameProcessor.cpp);
// the constructor, init(), process(), finish() and the XML description loop over it.
#pragma once
#include <chrono>
#include <string>

#include "bgs_host.h"
#include "PreProcessor.h"

namespace bgs_hip {

class IFrameProcessor {  // IFrameProcessor.h:23-28
 public:
  virtual void process(const Image& input) = 0;
  virtual ~IFrameProcessor() {}
};

class FrameProcessor : public IFrameProcessor, protected XmlDescribed {
 public:
  FrameProcessor();
  ~FrameProcessor() override;
  long frameToStop;
  std::string imgref;

  void init();
  void process(const Image& img_input) override;
  void finish();

  // the masks the reference keeps as img_framediff, img_staticfdiff, ... (FrameProcessor.h:99-170)
  Image img_prep, img_framediff, img_staticfdiff, img_wmovmean, img_movvar, img_mog1, img_mog2, img_bkgl_fgmask, img_asbl;
  Image img_gmg, img_adpmed, img_grigmm, img_zivgmm, img_tmpmean, img_wrenga, img_pramed, img_texbgs, img_kde, img_sdbgs, img_ssbgs, img_lobgs;  // FrameProcessor.h:120-236
  Image img_eigbkg;  // FrameProcessor.h (reference): img_eigbkg
  Image img_imbs;  // FrameProcessor.h:221 (reference): img_imbs
  Image img_mcbgs;  // FrameProcessor.h:225 (reference): img_mcbgs, 8UC3 with equal channels
  Image img_mlbgs;  // FrameProcessor.h (reference): img_mlbgs
  Image img_t2fgmm_um, img_t2fgmm_uv;  // FrameProcessor.h (reference): img_t2fgmm_um / img_t2fgmm_uv
  Image img_fsi, img_fci;  // FrameProcessor.h (reference): FuzzySugenoIntegral / FuzzyChoquetIntegral masks
  Image img_vumeter;  // FrameProcessor.h (reference): img_vumeter
  Image img_lb_sg, img_lb_fg, img_lb_mog, img_lb_som, img_lb_fsom;  // 8UC3 masks, equal channels (the lb/ wrappers' own convention)
  // One line per class, in the reference's order (the order of init(), process() and the XML keys).
  struct Class {
    const char* name;              // process(name, ...), the XML key "enable" + name, what tictoc names
    bool enabled;                  // the XML key's default
    IBGS* (*make)();               // new <Class>
    Image FrameProcessor::*image;  // where the mask is kept
    int teardown;                  // finish() deletes in descending order of this (:342-482: not quite the reverse of init())
    const char* file;              // bgs_demo writes the masks to <out_prefix>.<file>.raw
  };
  enum { kClasses = 34 };
  static const Class classes[kClasses];
  double lastDuration() const { return duration; }
  int groupedClasses() const { return (int)grouped_.size(); }  // how many classes share the fused launch (0: none)

 private:
  bool firstTime;
  long frameNumber;
  std::string processname;
  double duration;
  std::chrono::steady_clock::time_point t0;
  std::string tictoc;

  PreProcessor* preProcessor;
  bool enablePreProcessor;
  IBGS* bgs_[kClasses];     // classes[i]'s object while it is enabled, between init() and finish()
  bool enabled_[kClasses];  // ./config/FrameProcessor.xml: enable<classes[i].name>

  // the enabled byte-stream classes share ONE launch per frame (bgs_group) when there are at least two of them
  bgs_group* group_ = nullptr;
  std::vector<HipBGSBase*> grouped_;
  void runGroup(const Image& img_input);

  void process(std::string name, IBGS* bgs, const Image& img_input, Image& img_bgs);
  void tic(std::string value);
  void toc();
  void describe(XmlIo& io) override;
  void saveConfig() { saveDescribed("./config/FrameProcessor.xml"); }
  void loadConfig() { loadDescribed("./config/FrameProcessor.xml"); }
};

}  // namespace bgs_hip
