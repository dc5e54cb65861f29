// FrameProcessor.cpp — see FrameProcessor.h.  Statement order follows FrameProcessor.cpp of the reference.
#include "FrameProcessor.h"

#include <cstdlib>
#include <iomanip>

namespace bgs_hip {

template <class T>
static IBGS* make() {
  return new T;
}

// class, default of its enable key, mask, teardown position; reference lines of init() beside the rows.  Two classes go by another
// name in FrameProcessor.cpp than their own, so their rows are spelled out: {name, default, factory, mask, teardown, demo file}.
#define ROW(Class, on, image, teardown) {#Class, on, &make<Class>, &FrameProcessor::image, teardown, #Class}
const FrameProcessor::Class FrameProcessor::classes[FrameProcessor::kClasses] = {
    ROW(FrameDifferenceBGS, true, img_framediff, 0),
    ROW(StaticFrameDifferenceBGS, false, img_staticfdiff, 1),
    ROW(WeightedMovingMeanBGS, false, img_wmovmean, 2),
    ROW(WeightedMovingVarianceBGS, false, img_movvar, 3),
    ROW(MixtureOfGaussianV1BGS, false, img_mog1, 4),
    ROW(MixtureOfGaussianV2BGS, false, img_mog2, 5),
    ROW(AdaptiveBackgroundLearning, false, img_bkgl_fgmask, 6),
    ROW(GMG, false, img_gmg, 7),
    ROW(DPAdaptiveMedianBGS, false, img_adpmed, 8),
    ROW(DPGrimsonGMMBGS, false, img_grigmm, 9),
    ROW(DPZivkovicAGMMBGS, false, img_zivgmm, 10),
    ROW(DPMeanBGS, false, img_tmpmean, 11),
    ROW(DPWrenGABGS, false, img_wrenga, 12),
    ROW(DPPratiMediodBGS, false, img_pramed, 13),  // :81-88
    ROW(DPEigenbackgroundBGS, false, img_eigbkg, 14),
    ROW(DPTextureBGS, false, img_texbgs, 15),
    ROW(T2FGMM_UM, false, img_t2fgmm_um, 16),  // :90-94
    ROW(T2FGMM_UV, false, img_t2fgmm_uv, 17),
    ROW(FuzzySugenoIntegral, false, img_fsi, 18),  // :102-106
    ROW(FuzzyChoquetIntegral, false, img_fci, 19),
    ROW(LBSimpleGaussian, false, img_lb_sg, 20),  // :108-122
    ROW(LBFuzzyGaussian, false, img_lb_fg, 21),
    ROW(LBMixtureOfGaussians, false, img_lb_mog, 22),
    ROW(LBAdaptiveSOM, false, img_lb_som, 23),
    ROW(LBFuzzyAdaptiveSOM, false, img_lb_fsom, 24),
    ROW(VuMeter, false, img_vumeter, 25),  // :132
    ROW(KDE, false, img_kde, 26),  // after VuMeter, before IMBS (:135)
    {"IMBS", false, &make<IndependentMultimodalBGS>, &FrameProcessor::img_imbs, 28, "IndependentMultimodalBGS"},  // :138-139; deleted at :377-378
    {"MultiCueBGS", false, &make<SJN_MultiCueBGS>, &FrameProcessor::img_mcbgs, 29, "MultiCueBGS"},  // :141-142; deleted at :374-375
    ROW(MultiLayerBGS, false, img_mlbgs, 27),  // :126-127; deleted after the two above
    ROW(SigmaDeltaBGS, false, img_sdbgs, 30),
    ROW(SuBSENSEBGS, false, img_ssbgs, 31),
    ROW(LOBSTERBGS, false, img_lobgs, 32),
    // not in the reference's FrameProcessor (Demo.cpp / USTC_BGS type 7 only)
    ROW(AdaptiveSelectiveBackgroundLearning, false, img_asbl, 33),
};
#undef ROW

FrameProcessor::FrameProcessor() : frameToStop(0), firstTime(true), frameNumber(0), duration(0), tictoc(""), preProcessor(nullptr), enablePreProcessor(true) {
  for (int i = 0; i < kClasses; ++i) bgs_[i] = nullptr, enabled_[i] = false;
  std::cout << "FrameProcessor()" << std::endl;
  loadConfig();  // FrameProcessor.cpp:26-27
  saveConfig();
}

FrameProcessor::~FrameProcessor() { std::cout << "~FrameProcessor()" << std::endl; }

void FrameProcessor::init() {  // FrameProcessor.cpp:35-155
  if (enablePreProcessor) preProcessor = new PreProcessor;
  for (int i = 0; i < kClasses; ++i)
    if (enabled_[i]) bgs_[i] = classes[i].make();
  // Every enabled class gets the same pre-processed frame (:169-340).  The byte-stream classes among them run as ONE fused launch
  // over one upload and one read of that frame (bgs_group) when at least two are enabled; the reference's call shape - one
  // process(name, bgs, img_prep, img_xxx) per class, in its order - stays, each call then just delivers its class's share.
  // BGS_HOST_NO_GROUP=1 keeps every class on its own engine (A/B).
  const char* cand[] = {"FrameDifferenceBGS", "StaticFrameDifferenceBGS", "WeightedMovingMeanBGS", "WeightedMovingVarianceBGS", "AdaptiveBackgroundLearning", "SigmaDeltaBGS"};
  for (const char* c : cand)
    for (int i = 0; i < kClasses; ++i)
      if (bgs_[i] && std::string(classes[i].name) == c) grouped_.push_back(static_cast<HipBGSBase*>(bgs_[i]));
  const char* no_group = std::getenv("BGS_HOST_NO_GROUP");
  if (grouped_.size() < 2 || (no_group && no_group[0] == '1')) {
    grouped_.clear();
  } else {
    std::vector<bgs_algo> algos;
    for (HipBGSBase* c : grouped_) algos.push_back(c->algo());
    int rc = bgs_group_create(algos.data(), nullptr, (int)algos.size(), 0, 1, &group_);
    if (rc) throw Exception(rc, std::string("FrameProcessor: ") + bgs_last_error());
    for (size_t i = 0; i < grouped_.size(); ++i) grouped_[i]->attachGroup(group_, (int)i);
    std::cout << "FrameProcessor: " << grouped_.size() << " byte-stream classes share one launch per frame" << std::endl;
  }
}

void FrameProcessor::runGroup(const Image& img_input) {
  if (!group_ || img_input.empty()) return;
  const size_t n = grouped_.size();
  std::vector<uint8_t*> fg(n), bg(n);
  std::vector<size_t> fgs(n), bgs(n);
  std::vector<uint32_t> flags(n, 0);
  for (size_t i = 0; i < n; ++i) {
    grouped_[i]->groupPrepare(img_input);
    grouped_[i]->groupBuffers(&fg[i], &fgs[i], &bg[i], &bgs[i]);
  }
  int rc = bgs_group_process(group_, img_input.data, img_input.rows, img_input.cols, img_input.channels(), img_input.step, fg.data(), fgs.data(), bg.data(), bgs.data(),
                             flags.data());
  if (rc) throw Exception(rc, std::string("FrameProcessor: ") + bgs_last_error());
  for (size_t i = 0; i < n; ++i) grouped_[i]->groupDone(flags[i]);
}

void FrameProcessor::process(std::string name, IBGS* bgs, const Image& img_input, Image& img_bgs) {  // :157-167
  if (tictoc == name) tic(name);
  Image img_bkgmodel;
  bgs->process(img_input, img_bgs, img_bkgmodel);
  if (tictoc == name) toc();
}

void FrameProcessor::process(const Image& img_input) {  // :169-340
  frameNumber++;
  if (enablePreProcessor) preProcessor->process(img_input, img_prep);  // :173-174
  // with enablePreProcessor = 0 img_prep stays empty and every class returns at `if(img_input.empty()) return;`
  runGroup(img_prep);
  for (int i = 0; i < kClasses; ++i) {
    if (!enabled_[i]) continue;
    if (classes[i].image == &FrameProcessor::img_mlbgs) static_cast<MultiLayerBGS*>(bgs_[i])->setStatus(MultiLayerBGS::MLBGS_LEARN);  // :262-266
    process(classes[i].name, bgs_[i], img_prep, this->*classes[i].image);
  }
  firstTime = false;
}

void FrameProcessor::finish() {  // :342-482 (reverse order of init, but for MultiLayerBGS)
  for (int t = kClasses - 1; t >= 0; --t)
    for (int i = 0; i < kClasses; ++i)
      if (classes[i].teardown == t) delete bgs_[i], bgs_[i] = nullptr;
  delete preProcessor, preProcessor = nullptr;  // :480-481
  if (group_) bgs_group_destroy(group_), group_ = nullptr;
  grouped_.clear();
}

void FrameProcessor::tic(std::string value) {  // :484-488
  processname = value;
  t0 = std::chrono::steady_clock::now();
}

void FrameProcessor::toc() {  // :490-494, same line format
  duration = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::cout << processname << "\ttime(sec):" << std::fixed << std::setprecision(6) << duration << std::endl;
}

void FrameProcessor::describe(XmlIo& io) {  // :496-610 (keys of the classes this build provides; defaults: PreProcessor and FrameDifferenceBGS on)
  io("tictoc", tictoc, "");
  io("enablePreProcessor", enablePreProcessor, true);
  for (int i = 0; i < kClasses; ++i) io((std::string("enable") + classes[i].name).c_str(), enabled_[i], classes[i].enabled);
}

}  // namespace bgs_hip
