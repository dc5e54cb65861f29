// Fixture driver for the model stage of SJN_MultiCueBGS: calls the member functions of the reference's unmodified
// class one by one, as process() would (SJN_MultiCueBGS.cpp:85-99), with the box stage between the landmark map and the update
// replaced by scripted inputs.  Built as a shared object next to the reference's files (README.md here), driven by make_fixture.py.
//   training frame   BackgroundModeling_Par, g_iFrameCount++                                             (:85-88)
//   detecting frame  PreProcessing, T_GetConfidenceMap_Par, CreateLandmarkArray_Par                      (:315-325)
//                    the ghost loop of :1032-1046 over a scripted map
//                    UpdateModel_Par with g_BoundBoxInfo filled from scripted boxes; g_aUpdateMap is recorded
#include "SJN_MultiCueBGS.h"

#include <cstdint>

struct McParams {  // bgs_multicue_params without struct_size
  int32_t training_period, t_model_threshold, c_model_threshold;
  float learning_rate;
  int32_t texture_train_vol_range, color_train_vol_range, absorption_enable, absorption_period, reduced_width, reduced_height, back_clear_period, cache_clear_period;
};

struct McIo {
  const uint8_t* frames;  // [T][rows][cols][3]
  const uint8_t* ghost;   // [T - train][rh][rw], non-zero = aUpdateMap TRUE
  const int16_t* boxes;   // [T - train][nbox][5] = RLeft, RRight, RUpper, RBottom, valid
  uint8_t* landmark;      // [T - train][rh][rw]
  float* conf;            // [T - train][rh][rw]
  uint8_t* update;        // [T - train][rh][rw] = g_aUpdateMap
  uint8_t *gauss, *xyz;   // [n][3] of the last frame
  int32_t *tbook, *tcache;            // [n][6][2] = m_iTotal, m_iNumEntries
  float *tmeans, *tcache_means;       // [n][6][cap]
  int32_t *tmeta, *tcache_meta;       // [n][6][cap][3] = MNRL, first, last
  int16_t *tref, *tcnt;               // [n][6]
  int32_t *cbook, *ccache;            // [n][2]
  double *cmeans, *ccache_means;      // [n][cap][3]
  int32_t *cmeta, *ccache_meta;       // [n][cap][3]
  int16_t *cref, *ccnt;               // [n]
  int64_t* info;  // [0] g_iFrameCount, [1..4] largest m_iNumEntries of tbook, tcache, cbook, ccache, [5] codewords whose stored thresholds are not mean -/+ (float)range, [6] entries beyond cap
};

static void watch(SJN_MultiCueBGS& b, int rw, int rh, int range, int64_t* info) {
  for (int i = 0; i < rh; ++i)
    for (int j = 0; j < rw; ++j) {
      for (int k = 0; k < 6; ++k) {
        const TextureModel* m = b.g_TextureModel[i][j][k];
        if (m->m_iNumEntries > info[1]) info[1] = m->m_iNumEntries;
        for (int e = 0; e < m->m_iNumEntries; ++e) {
          const TextureCodeword* c = m->m_Codewords[e];
          if (c->m_fLowThre != c->m_fMean - (float)range || c->m_fHighThre != c->m_fMean + (float)range) ++info[5];
        }
        if (b.g_bAbsorptionEnable) {
          m = b.g_TCacheBook[i][j][k];
          if (m->m_iNumEntries > info[2]) info[2] = m->m_iNumEntries;
          for (int e = 0; e < m->m_iNumEntries; ++e) {
            const TextureCodeword* c = m->m_Codewords[e];
            if (c->m_fLowThre != c->m_fMean - (float)range || c->m_fHighThre != c->m_fMean + (float)range) ++info[5];
          }
        }
      }
      if (b.g_ColorModel[i][j]->m_iNumEntries > info[3]) info[3] = b.g_ColorModel[i][j]->m_iNumEntries;
      if (b.g_bAbsorptionEnable && b.g_CCacheBook[i][j]->m_iNumEntries > info[4]) info[4] = b.g_CCacheBook[i][j]->m_iNumEntries;
    }
}

static void put_t(const TextureModel* m, size_t b, int cap, int32_t* book, float* means, int32_t* meta, int64_t* info) {
  book[b * 2] = m->m_iTotal, book[b * 2 + 1] = m->m_iNumEntries;
  for (int e = 0; e < m->m_iNumEntries; ++e) {
    if (e >= cap) { ++info[6]; continue; }
    const TextureCodeword* c = m->m_Codewords[e];
    means[b * cap + e] = c->m_fMean;
    int32_t* q = meta + (b * cap + e) * 3;
    q[0] = c->m_iMNRL, q[1] = c->m_iT_first_time, q[2] = c->m_iT_last_time;
  }
}
static void put_c(const ColorModel* m, size_t b, int cap, int32_t* book, double* means, int32_t* meta, int64_t* info) {
  book[b * 2] = m->m_iTotal, book[b * 2 + 1] = m->m_iNumEntries;
  for (int e = 0; e < m->m_iNumEntries; ++e) {
    if (e >= cap) { ++info[6]; continue; }
    const ColorCodeword* c = m->m_Codewords[e];
    for (int k = 0; k < 3; ++k) means[(b * cap + e) * 3 + k] = c->m_dMean[k];
    int32_t* q = meta + (b * cap + e) * 3;
    q[0] = c->m_iMNRL, q[1] = c->m_iT_first_time, q[2] = c->m_iT_last_time;
  }
}

// caps: slots of tbook, tcache, cbook, ccache in the state arrays (zero-filled by the caller)
extern "C" int mc_run(const McParams* p, int rows, int cols, int T, int nbox, const int* caps, McIo* io) {
  SJN_MultiCueBGS* B = new SJN_MultiCueBGS();
  B->g_iTrainingPeriod = p->training_period, B->g_iT_ModelThreshold = p->t_model_threshold, B->g_iC_ModelThreshold = p->c_model_threshold;
  B->g_fLearningRate = p->learning_rate;
  B->g_nTextureTrainVolRange = (short)p->texture_train_vol_range, B->g_nColorTrainVolRange = (short)p->color_train_vol_range;
  B->g_bAbsorptionEnable = p->absorption_enable ? TRUE : FALSE, B->g_iAbsortionPeriod = p->absorption_period;
  B->g_iRWidth = p->reduced_width, B->g_iRHeight = p->reduced_height;
  B->g_iBackClearPeriod = p->back_clear_period, B->g_iCacheClearPeriod = p->cache_clear_period;
  B->g_fConfidenceThre = B->g_iT_ModelThreshold / (float)B->g_nNeighborNum;  // the constructor's line, :54, on the values just set
  const int rw = p->reduced_width, rh = p->reduced_height;
  const size_t n = (size_t)rw * rh;
  IplImage* frame = cvCreateImage(cvSize(cols, rows), IPL_DEPTH_8U, 3);
  int d = 0;
  for (int t = 0; t < T; ++t) {
    for (int y = 0; y < rows; ++y) memcpy(frame->imageData + (size_t)frame->widthStep * y, io->frames + ((size_t)t * rows + y) * cols * 3, (size_t)cols * 3);
    if (B->g_iFrameCount <= B->g_iTrainingPeriod) {  // :85-88
      B->BackgroundModeling_Par(frame);
      B->g_iFrameCount++;
      watch(*B, rw, rh, p->texture_train_vol_range, io->info);
      continue;
    }
    B->PreProcessing(frame);  // :318-325
    B->T_GetConfidenceMap_Par(B->g_aXYZFrame, B->g_aTextureConfMap, B->g_aNeighborDirection, B->g_TextureModel);
    B->CreateLandmarkArray_Par(B->g_fConfidenceThre, B->g_nColorTrainVolRange, B->g_aTextureConfMap, B->g_nNeighborNum, B->g_aXYZFrame, B->g_aNeighborDirection,
                               B->g_TextureModel, B->g_ColorModel, B->g_aLandmarkArray);
    for (int i = 0; i < rh; ++i)
      for (int j = 0; j < rw; ++j) io->landmark[d * n + (size_t)i * rw + j] = B->g_aLandmarkArray[i][j], io->conf[d * n + (size_t)i * rw + j] = B->g_aTextureConfMap[i][j];
    const float fLearningRate = B->g_fLearningRate;  // :1030-1046
    for (int i = 0; i < rh; ++i)
      for (int j = 0; j < rw; ++j)
        if (io->ghost[d * n + (size_t)i * rw + j]) {
          point center;
          center.m_nX = j, center.m_nY = i;
          B->T_ModelConstruction(B->g_nTextureTrainVolRange, fLearningRate, B->g_aXYZFrame, center, B->g_aNeighborDirection[i][j], B->g_TextureModel[i][j]);
          B->C_CodebookConstruction(B->g_aXYZFrame[i][j], j, i, B->g_nColorTrainVolRange, fLearningRate, B->g_ColorModel[i][j]);
          B->T_ClearNonEssentialEntries(B->g_iBackClearPeriod, B->g_TextureModel[i][j]);
          B->C_ClearNonEssentialEntries(B->g_iBackClearPeriod, B->g_ColorModel[i][j]);
        }
    BoundingBoxInfo* bb = B->g_BoundBoxInfo;
    if (nbox > bb->m_iArraySize) return 2;
    bb->m_iBoundBoxNum = nbox;
    for (int k = 0; k < nbox; ++k) {
      const int16_t* q = io->boxes + ((size_t)d * nbox + k) * 5;
      bb->m_aRLeft[k] = q[0], bb->m_aRRight[k] = q[1], bb->m_aRUpper[k] = q[2], bb->m_aRBottom[k] = q[3], bb->m_ValidBox[k] = q[4] ? TRUE : FALSE;
    }
    B->UpdateModel_Par();
    for (int i = 0; i < rh; ++i)
      for (int j = 0; j < rw; ++j) io->update[d * n + (size_t)i * rw + j] = B->g_aUpdateMap[i][j] == TRUE;
    watch(*B, rw, rh, p->texture_train_vol_range, io->info);
    ++d;
  }
  io->info[0] = B->g_iFrameCount;
  for (int i = 0; i < rh; ++i)
    for (int j = 0; j < rw; ++j) {
      const size_t px = (size_t)i * rw + j;
      for (int c = 0; c < 3; ++c) io->gauss[px * 3 + c] = B->g_aGaussFilteredFrame[i][j][c], io->xyz[px * 3 + c] = B->g_aXYZFrame[i][j][c];
      for (int k = 0; k < 6; ++k) {
        put_t(B->g_TextureModel[i][j][k], px * 6 + k, caps[0], io->tbook, io->tmeans, io->tmeta, io->info);
        io->tref[px * 6 + k] = -1, io->tcnt[px * 6 + k] = 0;  // without absorption the reference has no such arrays: what they would start as
        if (B->g_bAbsorptionEnable) {
          put_t(B->g_TCacheBook[i][j][k], px * 6 + k, caps[1], io->tcache, io->tcache_means, io->tcache_meta, io->info);
          io->tref[px * 6 + k] = B->g_aTReferredIndex[i][j][k], io->tcnt[px * 6 + k] = B->g_aTContinuousCnt[i][j][k];
        }
      }
      put_c(B->g_ColorModel[i][j], px, caps[2], io->cbook, io->cmeans, io->cmeta, io->info);
      io->cref[px] = -1, io->ccnt[px] = 0;
      if (B->g_bAbsorptionEnable) {
        put_c(B->g_CCacheBook[i][j], px, caps[3], io->ccache, io->ccache_means, io->ccache_meta, io->info);
        io->cref[px] = B->g_aCReferredIndex[i][j], io->ccnt[px] = B->g_aCContinuousCnt[i][j];
      }
    }
  cvReleaseImage(&frame);
  delete B;
  return 0;
}
