// host_classes_main.cpp — runs the host layer (tracking_amd/host: the 34 IBGS classes, FrameProcessor, USTC_BGS) on a machine without a
// device and prints what it does; the ./config/*.xml files it leaves in the working directory and its stdout are compared byte for
// byte with tests/golden/host_config/ by tests/test_host_classes_cpu.py.  Every class writes its XML before it asks for an engine
// (loadConfig(); if (firstTime) saveConfig();), so the one "no HIP device visible" exception ends each process() call after the
// observable is on disk.  Refuses to run where a device is visible: the test hides it.
//     host_classes classes [Class]   construct each class (or the one named), process() a 4 x 4 x 3 frame, print what it throws
//     host_classes fp                FrameProcessor: constructor, init(), finish(), destructor
//     host_classes ustc              USTC_BGS(t) for t = -1 .. 38: built or the exception's text
#include <cstring>
#include <iostream>
#include <string>

#include "FrameProcessor.h"
#include "ustc_bgs.h"

using namespace bgs_hip;

static const char* g_only = nullptr;

template <class T>
static void one(const char* name) {
  if (g_only && std::strcmp(g_only, name)) return;
  std::cout << "-- " << name << std::endl;
  T* c = new T;
  Image in(4, 4, 3), fg, bg;
  try {
    c->process(in, fg, bg);
    std::cout << "process() returned" << std::endl;
  } catch (const std::exception& ex) {
    std::cout << "std::exception:" << ex.what() << std::endl;
  }
  delete c;
}
#define ONE(Class) one<Class>(#Class)

static void classes() {
  ONE(FrameDifferenceBGS), ONE(StaticFrameDifferenceBGS), ONE(WeightedMovingMeanBGS), ONE(WeightedMovingVarianceBGS), ONE(AdaptiveBackgroundLearning);
  ONE(AdaptiveSelectiveBackgroundLearning), ONE(MixtureOfGaussianV2BGS), ONE(MixtureOfGaussianV1BGS), ONE(GMG), ONE(SigmaDeltaBGS), ONE(SuBSENSEBGS), ONE(LOBSTERBGS);
  ONE(DPZivkovicAGMMBGS), ONE(DPGrimsonGMMBGS), ONE(DPWrenGABGS), ONE(DPMeanBGS), ONE(DPAdaptiveMedianBGS), ONE(KDE), ONE(DPPratiMediodBGS), ONE(DPTextureBGS);
  ONE(LBSimpleGaussian), ONE(LBFuzzyGaussian), ONE(LBMixtureOfGaussians), ONE(LBAdaptiveSOM), ONE(LBFuzzyAdaptiveSOM), ONE(VuMeter);
  ONE(FuzzySugenoIntegral), ONE(FuzzyChoquetIntegral), ONE(T2FGMM_UM), ONE(T2FGMM_UV), ONE(DPEigenbackgroundBGS), ONE(IndependentMultimodalBGS);
  ONE(MultiLayerBGS), ONE(SJN_MultiCueBGS);
}

static void frame_processor() {
  FrameProcessor* fp = new FrameProcessor;
  fp->init();
  std::cout << "groupedClasses " << fp->groupedClasses() << std::endl;
  fp->finish();
  delete fp;
}

static void ustc() {
  for (int t = -1; t <= 38; ++t) {
    std::cout << "-- type " << t << std::endl;
    try {
      USTC_BGS u(t);
      std::cout << "built" << std::endl;
      u.Release();
    } catch (const std::exception& ex) {
      std::cout << "std::exception:" << ex.what() << std::endl;
    }
  }
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  bgs_engine* probe = nullptr;
  if (bgs_create(BGS_FRAME_DIFF, nullptr, 0, 1, &probe) == 0) {
    bgs_destroy(probe);
    std::cerr << "a device is visible: this program checks the host layer alone" << std::endl;
    return 3;
  }
  if (argc > 2) g_only = argv[2];
  if (what == "classes")
    classes();
  else if (what == "fp")
    frame_processor();
  else if (what == "ustc")
    ustc();
  else
    return 2;
  return 0;
}
