// Fixture driver for MultiLayerBGS: restates the call sequence of package_bgs/jmo/MultiLayerBGS.cpp:60-249 around the reference's
// unmodified CMultiLayerBGS, with the parameters handed in instead of read from ./config (the loadDefaultParams = false path).
// Built as a shared object next to the reference's model files (README.md here) and driven by make_fixture.py.
// Not restated: the XML, the windows, GetForegroundImage / GetForegroundProbabilityImage / MergeImages (they reach no output of
// process()), and the preload path.
#include "CMultiLayerBGS.h"

#include <cstdint>

static long g_expf_calls, g_expf_mismatch;

// -Wl,--wrap=expf: the model's expf becomes the correctly rounded one, and the calls where libm's own differs are counted
extern "C" float __real_expf(float);
extern "C" float __wrap_expf(float x) {
  const float r = (float)exp((double)x);
  ++g_expf_calls;
  if (__real_expf(x) != r) ++g_expf_mismatch;
  return r;
}

struct MlParams {  // bgs_multilayer_params without struct_size
  int32_t max_mode_num;
  float weight_updating_constant, texture_weight, bg_mode_percent;
  int32_t pattern_neig_half_size;
  float pattern_neig_gaus_sigma, bg_prob_threshold, bg_prob_updating_threshold;
  int32_t robust_LBP_constant;
  float min_noised_angle, shadow_rate, highlight_rate, frame_duration;
  float learn_mode_learn_rate_per_second, learn_weight_learn_rate_per_second, learn_init_mode_weight;
  float detect_mode_learn_rate_per_second, detect_weight_learn_rate_per_second, detect_init_mode_weight;
  int32_t status, disable_detect_mode, disable_learning, detect_after;
};

enum { MLBGS_LEARN = 0, MLBGS_DETECT = 1 };

// frames [T][rows][cols][3] -> masks [T][rows][cols], bgs [T][rows][cols][3]; after the last frame order [n][7], modes [n][5][18],
// dist [n]; consts[0..1] = the bits of m_fMinNoisedAngleSine and m_fMinNoisedAngle; counts[0..1] = expf calls and mismatches
extern "C" int ml_run(const MlParams* p, int rows, int cols, int T, const uint8_t* frames, uint8_t* masks, uint8_t* bgs, uint8_t* order, float* modes,
                      float* dist, uint32_t* consts, long* counts) {
  g_expf_calls = g_expf_mismatch = 0;
  const CvSize size = cvSize(cols, rows);
  IplImage* img = cvCreateImage(size, IPL_DEPTH_8U, 3);
  IplImage* bg_img = cvCreateImage(size, IPL_DEPTH_8U, 3);
  IplImage* fg_mask_img = cvCreateImage(size, IPL_DEPTH_8U, 1);
  int status = p->status;
  if (p->disable_detect_mode) status = MLBGS_LEARN;  // :71-72
  CMultiLayerBGS* BGS = new CMultiLayerBGS();
  BGS->Init(cols, rows);
  BGS->SetForegroundMaskImage(fg_mask_img);
  // cur_pattern is new float[6], never written when texture_weight <= 0 (ComputeLBP is skipped) and then copied into the modes: the
  // fixture defines those patterns as zero
  for (size_t i = 0; i < (size_t)rows * cols; ++i) memset(BGS->m_pPixelLBPs[i].cur_pattern, 0, 6 * sizeof(float));
  if (status == MLBGS_DETECT) BGS->m_disableLearning = p->disable_learning != 0;  // :100-108
  BGS->m_nMaxLBPModeNum = p->max_mode_num;  // :132-145
  BGS->m_fWeightUpdatingConstant = p->weight_updating_constant;
  BGS->m_fTextureWeight = p->texture_weight;
  BGS->m_fBackgroundModelPercent = p->bg_mode_percent;
  BGS->m_nPatternDistSmoothNeigHalfSize = p->pattern_neig_half_size;
  BGS->m_fPatternDistConvGaussianSigma = p->pattern_neig_gaus_sigma;
  BGS->m_fPatternColorDistBgThreshold = p->bg_prob_threshold;
  BGS->m_fPatternColorDistBgUpdatedThreshold = p->bg_prob_updating_threshold;
  BGS->m_fRobustColorOffset = p->robust_LBP_constant;
  BGS->m_fMinNoisedAngle = p->min_noised_angle;
  BGS->m_fRobustShadowRate = p->shadow_rate;
  BGS->m_fRobustHighlightRate = p->highlight_rate;
  BGS->SetFrameRate(p->frame_duration);  // :154
  float mode_rate, weight_rate, init_weight;
  if (status == MLBGS_LEARN) mode_rate = p->learn_mode_learn_rate_per_second, weight_rate = p->learn_weight_learn_rate_per_second, init_weight = p->learn_init_mode_weight;
  else mode_rate = p->detect_mode_learn_rate_per_second, weight_rate = p->detect_weight_learn_rate_per_second, init_weight = p->detect_init_mode_weight;
  BGS->SetParameters(p->max_mode_num, mode_rate, weight_rate, init_weight);  // :188
  const size_t n = (size_t)rows * cols;
  for (int t = 0; t < T; ++t) {  // t is the wrapper's frameNumber
    if (p->detect_after > 0 && p->detect_after == t) {  // :200-218, the hard-coded DETECT values
      status = MLBGS_DETECT;
      BGS->SetParameters(p->max_mode_num, 0.01f, 0.01f, 0.001f);
      BGS->m_disableLearning = p->disable_learning != 0;
    }
    for (int y = 0; y < rows; ++y) memcpy(img->imageData + (size_t)img->widthStep * y, frames + ((size_t)t * n + (size_t)y * cols) * 3, (size_t)cols * 3);
    BGS->SetRGBInputImage(img);
    BGS->Process();
    BGS->GetBackgroundImage(bg_img);
    BGS->GetForegroundMaskImage(fg_mask_img);
    for (int y = 0; y < rows; ++y) {
      memcpy(masks + (size_t)t * n + (size_t)y * cols, fg_mask_img->imageData + (size_t)fg_mask_img->widthStep * y, cols);
      memcpy(bgs + ((size_t)t * n + (size_t)y * cols) * 3, bg_img->imageData + (size_t)bg_img->widthStep * y, (size_t)cols * 3);
    }
  }
  // the model after the last frame, in the reference's field order; list entries at and past num, and slots the list does not name, read 0
  memset(order, 0, n * 7);
  memset(modes, 0, n * 5 * 18 * sizeof(float));
  for (size_t i = 0; i < n; ++i) {
    const PixelLBPStruct& P = BGS->m_pPixelLBPs[i];
    order[i * 7] = (uint8_t)P.num, order[i * 7 + 1] = (uint8_t)P.bg_num;
    for (unsigned a = 0; a < P.num; ++a) {
      const unsigned s = P.lbp_idxes[a];
      order[i * 7 + 2 + a] = (uint8_t)s;
      const LBPStruct& L = P.LBPs[s];
      float* m = modes + (i * 5 + s) * 18;
      for (int k = 0; k < 6; ++k) m[k] = L.bg_pattern[k];
      for (int k = 0; k < 3; ++k) m[6 + k] = L.bg_intensity[k], m[9 + k] = L.max_intensity[k], m[12 + k] = L.min_intensity[k];
      m[15] = L.weight, m[16] = L.max_weight, m[17] = (float)L.bg_layer_num;
    }
  }
  for (int y = 0; y < rows; ++y) memcpy(dist + (size_t)y * cols, BGS->m_pBgDistImg->imageData + (size_t)BGS->m_pBgDistImg->widthStep * y, (size_t)cols * 4);
  memcpy(&consts[0], &BGS->m_fMinNoisedAngleSine, 4);
  memcpy(&consts[1], &BGS->m_fMinNoisedAngle, 4);
  counts[0] = g_expf_calls, counts[1] = g_expf_mismatch;
  // the model is leaked on purpose: ~CMultiLayerBGS deletes new[] arrays with delete and its base-class images twice
  cvReleaseImage(&img), cvReleaseImage(&bg_img), cvReleaseImage(&fg_mask_img);
  return 0;
}
