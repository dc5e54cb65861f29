// Fixture driver for the box stage and the whole-frame step of SJN_MultiCueBGS: the reference's unmodified class, its
// member functions called in process()'s order (SJN_MultiCueBGS.cpp:85-99) with only loadConfig / saveConfig / imshow left out.
//   mcb_run    training frame   BackgroundModeling_Par, g_iFrameCount++
//              detecting frame  ForegroundExtraction, UpdateModel_Par, GetForegroundMap(result, NULL)
//   mcb_post   PostProcessing alone on a hand-made landmark map (after Initialize and PreProcessing, so that UpdateModel_Par, which
//              builds g_aUpdateMap, runs on defined data)
// What the class keeps to itself is recovered from the stand-in's cvCanny log: the boxes that passed EvaluateBoxSize are those with a
// pair of calls, in order (checked against the reference's own EvaluateBoxSize on a copy of the boxes); the distance of a box is the
// reference's CalculateHausdorffDist on the two logged edge maps; the ghost map is the exclusive rectangle of every box that passed the
// size test and is invalid afterwards.  Built as a shared object like driver.cpp (README.md here), driven by make_box_fixture.py.
#include "SJN_MultiCueBGS.h"

#include <cstdint>

enum { kMaxBoxes = 300, kBoxFields = 13 };

struct McParams {  // bgs_multicue_params without struct_size
  int32_t training_period, t_model_threshold, c_model_threshold;
  float learning_rate;
  int32_t texture_train_vol_range, color_train_vol_range, absorption_enable, absorption_period, reduced_width, reduced_height, back_clear_period, cache_clear_period;
};

struct BoxOut {       // one detecting frame (or one mcb_post call)
  uint8_t* landmark;  // [rh][rw]
  uint8_t* fore0;     // [rh][rw] the map after MorphologicalOpearions where the logged foreground windows cover it, 0 elsewhere
  uint8_t* fore;      // [rh][rw] g_aResizedForeMap after RemovingInvalidForeRegions
  uint8_t* ghost;     // [rh][rw]
  uint8_t* update;    // [rh][rw] g_aUpdateMap
  int32_t* boxes;     // [kMaxBoxes][kBoxFields]
  double* dist;       // [kMaxBoxes] CalculateHausdorffDist of the boxes that passed the size test, -1 elsewhere
  int32_t* count;     // [1]
};

static IplImage* image_of(int rows, int cols, int ch, const uint8_t* data) {
  IplImage* im = cvCreateImage(cvSize(cols, rows), IPL_DEPTH_8U, ch);
  for (int y = 0; y < rows; ++y) memcpy(im->imageData + (size_t)im->widthStep * y, data + (size_t)y * cols * ch, (size_t)cols * ch);
  return im;
}

static IplImage* edges_of(const StandInCannyCall& c) { return image_of(c.rows, c.cols, 1, c.out.data()); }

// after PostProcessing: everything of one frame but g_aUpdateMap
static int record(SJN_MultiCueBGS* B, int rw, int rh, size_t log_from, BoxOut* o) {
  const std::vector<StandInCannyCall>& log = standInCannyLog();
  BoundingBoxInfo* bb = B->g_BoundBoxInfo;
  const int nb = bb->m_iBoundBoxNum;
  o->count[0] = nb;
  if (nb > kMaxBoxes) return 3;  // the reference has written past its arrays
  BoundingBoxInfo sz = *bb;  // the reference's own size test on a copy of the boxes
  std::vector<BOOL> flags(nb ? nb : 1);
  sz.m_ValidBox = flags.data();
  B->EvaluateBoxSize(&sz);
  size_t at = log_from;
  for (int i = 0; i < rh; ++i)
    for (int j = 0; j < rw; ++j) o->fore[(size_t)i * rw + j] = B->g_aResizedForeMap[i][j], o->ghost[(size_t)i * rw + j] = 0, o->fore0[(size_t)i * rw + j] = 0;
  for (int k = 0; k < nb; ++k) {
    int32_t* q = o->boxes + (size_t)k * kBoxFields;
    q[0] = bb->m_aRLeft[k], q[1] = bb->m_aRRight[k], q[2] = bb->m_aRUpper[k], q[3] = bb->m_aRBottom[k];
    q[4] = bb->m_aLeft[k], q[5] = bb->m_aRight[k], q[6] = bb->m_aUpper[k], q[7] = bb->m_aBottom[k];
    q[8] = flags[k] == TRUE, q[9] = bb->m_ValidBox[k] == TRUE;
    o->dist[k] = -1;
    if (!q[8]) continue;
    if (at + 2 > log.size()) return 4;
    const StandInCannyCall &cf = log[at], &cm = log[at + 1];
    at += 2;
    if (cf.cols != q[1] - q[0] || cf.rows != q[3] - q[2] || cm.cols != cf.cols || cm.rows != cf.rows) return 5;
    IplImage *ef = edges_of(cf), *em = edges_of(cm);
    o->dist[k] = B->CalculateHausdorffDist(ef, em);
    cvReleaseImage(&ef), cvReleaseImage(&em);
    int na = 0, nm = 0, near = 0;
    for (size_t i = 0; i < cf.out.size(); ++i) na += cf.out[i] != 0;
    for (int y = 0; y < cm.rows; ++y)
      for (int x = 0; x < cm.cols; ++x) {
        o->fore0[(size_t)(y + q[2]) * rw + x + q[0]] = cm.in[(size_t)y * cm.cols + x];
        if (!cm.out[(size_t)y * cm.cols + x]) continue;
        ++nm;
        bool hit = false;
        for (int yy = 0; yy < cf.rows && !hit; ++yy)
          for (int xx = 0; xx < cf.cols && !hit; ++xx)
            hit = cf.out[(size_t)yy * cf.cols + xx] && (yy - y) * (yy - y) + (xx - x) * (xx - x) <= 100;
        near += hit;
      }
    q[10] = na, q[11] = nm, q[12] = near;
    if (!q[9])
      for (int i = q[2]; i < q[3]; ++i)
        for (int j = q[0]; j < q[1]; ++j) o->ghost[(size_t)i * rw + j] = 1;
  }
  return at == log.size() ? 0 : 6;
}

static void record_update(SJN_MultiCueBGS* B, int rw, int rh, BoxOut* o) {
  for (int i = 0; i < rh; ++i)
    for (int j = 0; j < rw; ++j) o->update[(size_t)i * rw + j] = B->g_aUpdateMap[i][j] == TRUE;
}

static SJN_MultiCueBGS* model_of(const McParams* p) {
  SJN_MultiCueBGS* B = new SJN_MultiCueBGS();
  B->g_iTrainingPeriod = p->training_period, B->g_iT_ModelThreshold = p->t_model_threshold, B->g_iC_ModelThreshold = p->c_model_threshold;
  B->g_fLearningRate = p->learning_rate;
  B->g_nTextureTrainVolRange = (short)p->texture_train_vol_range, B->g_nColorTrainVolRange = (short)p->color_train_vol_range;
  B->g_bAbsorptionEnable = p->absorption_enable ? TRUE : FALSE, B->g_iAbsortionPeriod = p->absorption_period;
  B->g_iRWidth = p->reduced_width, B->g_iRHeight = p->reduced_height;
  B->g_iBackClearPeriod = p->back_clear_period, B->g_iCacheClearPeriod = p->cache_clear_period;
  B->g_fConfidenceThre = B->g_iT_ModelThreshold / (float)B->g_nNeighborNum;  // the constructor's line, :54, on the values just set
  return B;
}

struct McState {  // as driver.cpp's McIo, the state planes only
  uint8_t *gauss, *xyz;
  int32_t *tbook, *tcache;
  float *tmeans, *tcache_means;
  int32_t *tmeta, *tcache_meta;
  int16_t *tref, *tcnt;
  int32_t *cbook, *ccache;
  double *cmeans, *ccache_means;
  int32_t *cmeta, *ccache_meta;
  int16_t *cref, *ccnt;
  int64_t* info;  // [0] g_iFrameCount, [1] entries beyond cap
};

static void put_t(const TextureModel* m, size_t b, int cap, int32_t* book, float* means, int32_t* meta, int64_t* info) {
  book[b * 2] = m->m_iTotal, book[b * 2 + 1] = m->m_iNumEntries;
  for (int e = 0; e < m->m_iNumEntries; ++e) {
    if (e >= cap) { ++info[1]; continue; }
    const TextureCodeword* c = m->m_Codewords[e];
    means[b * cap + e] = c->m_fMean;
    int32_t* q = meta + (b * cap + e) * 3;
    q[0] = c->m_iMNRL, q[1] = c->m_iT_first_time, q[2] = c->m_iT_last_time;
  }
}
static void put_c(const ColorModel* m, size_t b, int cap, int32_t* book, double* means, int32_t* meta, int64_t* info) {
  book[b * 2] = m->m_iTotal, book[b * 2 + 1] = m->m_iNumEntries;
  for (int e = 0; e < m->m_iNumEntries; ++e) {
    if (e >= cap) { ++info[1]; continue; }
    const ColorCodeword* c = m->m_Codewords[e];
    for (int k = 0; k < 3; ++k) means[(b * cap + e) * 3 + k] = c->m_dMean[k];
    int32_t* q = meta + (b * cap + e) * 3;
    q[0] = c->m_iMNRL, q[1] = c->m_iT_first_time, q[2] = c->m_iT_last_time;
  }
}

// frames [T][rows][cols][3]; outs: one BoxOut per detecting frame; images [T][rows][cols] = channel 0 of process()'s output
extern "C" int mcb_run(const McParams* p, int rows, int cols, int T, const uint8_t* frames, const int* caps, BoxOut* outs, uint8_t* images, McState* st) {
  SJN_MultiCueBGS* B = model_of(p);
  const int rw = p->reduced_width, rh = p->reduced_height;
  standInCannyLog().clear();
  int d = 0;
  for (int t = 0; t < T; ++t) {
    IplImage* frame = image_of(rows, cols, 3, frames + (size_t)t * rows * cols * 3);
    IplImage* result = cvCreateImage(cvGetSize(frame), IPL_DEPTH_8U, 3);
    cvSetZero(result);
    if (B->g_iFrameCount <= B->g_iTrainingPeriod) {  // :85-88
      B->BackgroundModeling_Par(frame);
      B->g_iFrameCount++;
    } else {  // :91-99
      B->g_bForegroundMapEnable = FALSE;
      const size_t from = standInCannyLog().size();
      B->ForegroundExtraction(frame);
      BoxOut* o = outs + d++;
      for (int i = 0; i < rh; ++i)
        for (int j = 0; j < rw; ++j) o->landmark[(size_t)i * rw + j] = B->g_aLandmarkArray[i][j];
      const int rc = record(B, rw, rh, from, o);
      if (rc) return rc;
      B->UpdateModel_Par();
      record_update(B, rw, rh, o);
      B->GetForegroundMap(result, NULL);
    }
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) {
        const uint8_t* q = (const uint8_t*)result->imageData + (size_t)y * result->widthStep + (size_t)x * 3;
        if (q[0] != q[1] || q[0] != q[2]) return 7;  // the three channels are equal by construction
        images[((size_t)t * rows + y) * cols + x] = q[0];
      }
    cvReleaseImage(&frame), cvReleaseImage(&result);
  }
  st->info[0] = B->g_iFrameCount;
  for (int i = 0; i < rh; ++i)
    for (int j = 0; j < rw; ++j) {
      const size_t px = (size_t)i * rw + j;
      for (int c = 0; c < 3; ++c) st->gauss[px * 3 + c] = B->g_aGaussFilteredFrame[i][j][c], st->xyz[px * 3 + c] = B->g_aXYZFrame[i][j][c];
      for (int k = 0; k < 6; ++k) {
        put_t(B->g_TextureModel[i][j][k], px * 6 + k, caps[0], st->tbook, st->tmeans, st->tmeta, st->info);
        st->tref[px * 6 + k] = -1, st->tcnt[px * 6 + k] = 0;
        if (B->g_bAbsorptionEnable) {
          put_t(B->g_TCacheBook[i][j][k], px * 6 + k, caps[1], st->tcache, st->tcache_means, st->tcache_meta, st->info);
          st->tref[px * 6 + k] = B->g_aTReferredIndex[i][j][k], st->tcnt[px * 6 + k] = B->g_aTContinuousCnt[i][j][k];
        }
      }
      put_c(B->g_ColorModel[i][j], px, caps[2], st->cbook, st->cmeans, st->cmeta, st->info);
      st->cref[px] = -1, st->ccnt[px] = 0;
      if (B->g_bAbsorptionEnable) {
        put_c(B->g_CCacheBook[i][j], px, caps[3], st->ccache, st->ccache_means, st->ccache_meta, st->info);
        st->cref[px] = B->g_aCReferredIndex[i][j], st->ccnt[px] = B->g_aCContinuousCnt[i][j];
      }
    }
  delete B;
  return 0;
}

// PostProcessing alone: frame [rows][cols][3], landmark [rh][rw]
extern "C" int mcb_post(const McParams* p, int rows, int cols, const uint8_t* frame_data, const uint8_t* landmark, BoxOut* o) {
  SJN_MultiCueBGS* B = model_of(p);
  const int rw = p->reduced_width, rh = p->reduced_height;
  IplImage* frame = image_of(rows, cols, 3, frame_data);
  B->Initialize(frame);
  B->PreProcessing(frame);
  for (int i = 0; i < rh; ++i)
    for (int j = 0; j < rw; ++j) B->g_aLandmarkArray[i][j] = o->landmark[(size_t)i * rw + j] = landmark[(size_t)i * rw + j];
  standInCannyLog().clear();
  B->PostProcessing(frame);
  const int rc = record(B, rw, rh, 0, o);
  if (rc) return rc;
  B->UpdateModel_Par();
  record_update(B, rw, rh, o);
  cvReleaseImage(&frame);
  delete B;
  return 0;
}

// the cvCanny calls since the last clear, flattened: per call rows, cols (int32 each), then the input and the output bytes
extern "C" int64_t mcb_log(uint8_t* dst, int64_t cap) {
  int64_t need = 0;
  for (const StandInCannyCall& c : standInCannyLog()) need += 8 + 2 * (int64_t)c.in.size();
  if (!dst || cap < need) return need;
  for (const StandInCannyCall& c : standInCannyLog()) {
    const int32_t hw[2] = {c.rows, c.cols};
    memcpy(dst, hw, 8), dst += 8;
    memcpy(dst, c.in.data(), c.in.size()), dst += c.in.size();
    memcpy(dst, c.out.data(), c.out.size()), dst += c.out.size();
  }
  return need;
}
