// ref_dp_cli - TEST INFRASTRUCTURE ONLY.  Drives the reference's own package_bgs/dp/ models (ZivkovicAGMM, GrimsonGMM, WrenGA,
// MeanBGS, AdaptiveMedianBGS: compiled unmodified from the reference tree behind oracle/ref_stub/opencv2/opencv.hpp, see
// oracle/Makefile) the way the DP*BGS wrappers' process() drives them, one case per process.
//
//   ref_dp_cli CLASS T H W [threshold=V] [alpha=V] [gaussians=V] [rate=V] [learn=V] [planes=1] < T*H*W*3 bytes > masks [+ model]
//   ref_dp_cli env          prints which overload an unqualified sqrt(float) resolves to behind the stand-in header
//
// CLASS is ziv, grim, wren, mean or median.  Every parameter is held in the wrapper's own type (threshold: double for ziv, grim
// and wren, int for mean and median; alpha: double; the rest int) and handed to the model through the params object's typed
// accessors, so every narrowing on the way (double -> float, int -> unsigned int, int -> unsigned char, 2 * unsigned char ->
// unsigned char) is performed by the reference's own declarations.  On frame 0: SetFrameSize, LowThreshold() = threshold,
// HighThreshold() = 2 * LowThreshold(), the class's other parameters, Initalize, InitModel.  On every frame t (0-based):
// Subtract(t, frame, low, high), low.Clear(), Update(t, frame, low); the output is the high-threshold mask, written row by row
// without padding.  With planes=1 the model after the last frame follows the masks, pixel by pixel:
//   ziv    n*K*5 floats (sigma, muR, muG, muB, weight per mode), then the mode count bytes
//   grim   n*K*6 floats (variance, muR, muG, muB, weight, significants per mode), then the mode count bytes
//   wren   6 floats per pixel (mu[3], var[3]);   mean  3 floats per pixel;   median  3 bytes per pixel
#include <stdio.h>
#include <string>
#include <vector>

#include "AdaptiveMedianBGS.h"
#include "GrimsonGMM.h"
#include "MeanBGS.h"
#include "WrenGA.h"
#include "ZivkovicAGMM.h"

using namespace Algorithms::BackgroundSubtraction;

const char* ref_dp_sqrt_overload();  // ref_dp_env.cpp: a translation unit that sees the headers GrimsonGMM.cpp sees, no more

// The models keep their state in private members.  An explicit instantiation may name them (access checks do not apply to
// its arguments), and the friend it defines hands out the member's address; nothing in the reference's headers is redefined.
template <class Tag, class Ptr, Ptr member>
struct Expose {
  friend void* member_address(Tag, typename Tag::owner* o) { return (void*)&(o->*member); }
};
#define EXPOSE(tag, cls, name)                            \
  struct tag {                                            \
    typedef cls owner;                                    \
    friend void* member_address(tag, cls*);               \
  };                                                      \
  template struct Expose<tag, decltype(&cls::name), &cls::name>
EXPOSE(ZivModes, ZivkovicAGMM, m_modes);
EXPOSE(ZivCounts, ZivkovicAGMM, m_modes_per_pixel);
EXPOSE(GrimModes, GrimsonGMM, m_modes);
EXPOSE(GrimCounts, GrimsonGMM, m_modes_per_pixel);
EXPOSE(WrenGauss, WrenGA, m_gaussian);
EXPOSE(MeanPlane, MeanBGS, m_mean);

struct Args {
  std::string cls;
  int T, H, W;
  std::string threshold, alpha;  // parsed into the wrapper's type per class
  int gaussians, rate, learn, planes;
};

static void put(const void* p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, stdout) != bytes) exit(3);
}

// rows of `img` without their padding
static void put_rows(const IplImage* img) {
  for (int r = 0; r < img->height; ++r) put(img->imageData + (size_t)r * img->widthStep, (size_t)img->width * img->nChannels * (img->depth / 8));
}

template <class Model, class Params, class Dump>
static int run(const Args& a, Params& params, Model& bgs, Dump dump) {
  const size_t row = (size_t)a.W * 3;
  std::vector<unsigned char> buf(row);
  RgbImage frame_data(cvCreateImage(cvSize(a.W, a.H), IPL_DEPTH_8U, 3));
  BwImage low(cvCreateImage(cvSize(a.W, a.H), IPL_DEPTH_8U, 1)), high(cvCreateImage(cvSize(a.W, a.H), IPL_DEPTH_8U, 1));
  for (int t = 0; t < a.T; ++t) {
    for (int r = 0; r < a.H; ++r) {
      if (row && fread(buf.data(), 1, row, stdin) != row) return fprintf(stderr, "ref_dp_cli: short input at frame %d\n", t), 2;
      memcpy(frame_data.Ptr()->imageData + (size_t)r * frame_data.Ptr()->widthStep, buf.data(), row);
    }
    if (t == 0) {
      bgs.Initalize(params);
      bgs.InitModel(frame_data);
    }
    bgs.Subtract(t, frame_data, low, high);
    low.Clear();
    bgs.Update(t, frame_data, low);
    put_rows(high.Ptr());
  }
  if (a.planes) dump(bgs);
  return 0;
}

static void dump_ziv(ZivkovicAGMM& m, size_t n, int K) {
  put(*(void**)member_address(ZivModes(), &m), n * K * 5 * sizeof(float));
  put(*(void**)member_address(ZivCounts(), &m), n);
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "env") {
    printf("sqrt(float) -> %s\n", ref_dp_sqrt_overload());
    return 0;
  }
  if (argc < 5) return fprintf(stderr, "usage: ref_dp_cli CLASS T H W [key=value ...] < frames > masks\n"), 1;
  Args a;
  a.cls = argv[1], a.T = atoi(argv[2]), a.H = atoi(argv[3]), a.W = atoi(argv[4]);
  a.gaussians = 3, a.rate = 7, a.learn = 30, a.planes = 0;
  for (int i = 5; i < argc; ++i) {
    const std::string kv = argv[i];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return fprintf(stderr, "ref_dp_cli: %s is not key=value\n", argv[i]), 1;
    const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
    if (k == "threshold") a.threshold = v;
    else if (k == "alpha") a.alpha = v;
    else if (k == "gaussians") a.gaussians = atoi(v.c_str());
    else if (k == "rate") a.rate = atoi(v.c_str());
    else if (k == "learn") a.learn = atoi(v.c_str());
    else if (k == "planes") a.planes = atoi(v.c_str());
    else return fprintf(stderr, "ref_dp_cli: unknown parameter %s\n", k.c_str()), 1;
  }
  if (a.threshold.empty() || (a.alpha.empty() && a.cls != "median")) return fprintf(stderr, "ref_dp_cli: threshold and alpha are required\n"), 1;
  const size_t n = (size_t)a.H * a.W;
  const double alpha = a.alpha.empty() ? 0.0 : strtod(a.alpha.c_str(), 0);
  if (a.cls == "ziv" || a.cls == "grim" || a.cls == "wren") {
    const double threshold = strtod(a.threshold.c_str(), 0);
    if (a.cls == "ziv") {
      ZivkovicParams params;
      params.SetFrameSize(a.W, a.H);
      params.LowThreshold() = threshold;
      params.HighThreshold() = 2 * params.LowThreshold();
      params.Alpha() = alpha;
      params.MaxModes() = a.gaussians;
      ZivkovicAGMM bgs;
      const int K = a.gaussians;
      return run(a, params, bgs, [n, K](ZivkovicAGMM& m) { dump_ziv(m, n, K); });
    }
    if (a.cls == "grim") {
      GrimsonParams params;
      params.SetFrameSize(a.W, a.H);
      params.LowThreshold() = threshold;
      params.HighThreshold() = 2 * params.LowThreshold();
      params.Alpha() = alpha;
      params.MaxModes() = a.gaussians;
      GrimsonGMM bgs;
      const int K = a.gaussians;
      return run(a, params, bgs, [n, K](GrimsonGMM& m) {
        put(*(void**)member_address(GrimModes(), &m), n * K * 6 * sizeof(float));
        put_rows(((BwImage*)member_address(GrimCounts(), &m))->Ptr());
      });
    }
    WrenParams params;
    params.SetFrameSize(a.W, a.H);
    params.LowThreshold() = threshold;
    params.HighThreshold() = 2 * params.LowThreshold();
    params.Alpha() = alpha;
    params.LearningFrames() = a.learn;
    WrenGA bgs;
    return run(a, params, bgs, [n](WrenGA& m) { put(*(void**)member_address(WrenGauss(), &m), n * 6 * sizeof(float)); });
  }
  const int threshold = (int)strtol(a.threshold.c_str(), 0, 10);
  if (a.cls == "mean") {
    MeanParams params;
    params.SetFrameSize(a.W, a.H);
    params.LowThreshold() = threshold;
    params.HighThreshold() = 2 * params.LowThreshold();
    params.Alpha() = alpha;
    params.LearningFrames() = a.learn;
    MeanBGS bgs;
    return run(a, params, bgs, [](MeanBGS& m) { put_rows(((RgbImageFloat*)member_address(MeanPlane(), &m))->Ptr()); });
  }
  if (a.cls == "median") {
    AdaptiveMedianParams params;
    params.SetFrameSize(a.W, a.H);
    params.LowThreshold() = threshold;
    params.HighThreshold() = 2 * params.LowThreshold();
    params.SamplingRate() = a.rate;
    params.LearningFrames() = a.learn;
    AdaptiveMedianBGS bgs;
    return run(a, params, bgs, [](AdaptiveMedianBGS& m) { put_rows(m.Background()->Ptr()); });
  }
  return fprintf(stderr, "ref_dp_cli: unknown class %s\n", a.cls.c_str()), 1;
}
