// kernel_multilayer.h — package_bgs/jmo MultiLayerBGS (Yao and Odobez: LBP + colour layers, BGS_MULTILAYER; host side in
// engine_multilayer.h).
//
// CMultiLayerBGS::BackgroundSubtractionProcess (CMultiLayerBGS.cpp:375-801) per stream and frame, on the caller's stream:
//   ml_model_kernel   one pixel per lane: BGR2GRAY of the pixel and its six LBP neighbours on the fly (no gray plane), the first form
//                     of RemoveBackgroundLayers, the match over the listed modes, the update, the re-rank, the raw distance and the
//                     background byte
//   ml_smooth_kernel  cvSmooth(CV_GAUSSIAN) of the distance plane through an LDS tile with a halo of h, replicate border per stream
//                     image, fused with cvThreshold and the byte mask
// The quirks of the reference that are kept, and the two places where the contract is the fixture's stand-in (the summation order
// of the Gaussian, expf as the correctly rounded value), are DESIGN.md §5.11.
//
// State, one dword per pixel and plane, plane-major ([stream][plane][pixel]): plane 0 = num | bg_num << 3 | lbp_idxes[r] << (6 + 3 r),
// plane 1 = bg_layer_num of slot s << 3 s, then 13 planes per physical slot: bg_pattern[6], bg_intensity[3], weight, max_weight,
// max_intensity as bytes, min_intensity as bytes (both are integer-valued: MIN / MAX of bytes).  A mode never moves: the rank order
// lives in the header.  Slots the header does not list are never read, so only the header needs clearing at a stream's first frame.
// The per-slot arrays below are indexed by compile-time constants only (unrolled loops; a lane-varying slot goes through select
// chains), so nothing lands in scratch.
#pragma once
#include "bgs_device.h"

namespace bgs {

constexpr int kMlSlots = 5;        // MAX_LBP_MODE_NUM: the reference allocates five before it learns max_mode_num
constexpr int kMlSlotPlanes = 13;
constexpr int kMlPlanes = 2 + kMlSlots * kMlSlotPlanes;
constexpr int kMlMaxHalf = 8;      // largest pattern_neig_half_size the smoothing tile is built for
constexpr int kMlTileW = 32, kMlTileH = 8;
constexpr int kMlUnlisted = 7;

struct MlArgs {
  const uint8_t* cur;   // [count][n][3]
  uint8_t *fg, *bgout;  // [count][n], [count][n][3] (both nullable)
  uint32_t* model;      // [count][kMlPlanes][n]
  float *raw, *dist;    // [count][n]: this frame's distances, the smoothed map
  uint32_t* empty_last; // [count]: bFirstFrame as the pixel loop leaves it, written by the model kernel, read by the smoothing kernel
  uint32_t n;
  int rows, cols;
  int max_modes, learn, first, texture;  // m_nMaxLBPModeNum; !m_disableLearning; the streams' first frame (host side only); m_fTextureWeight > 0
  float tw, wc, percent, thr, upd_thr, offset, min_sine, min_angle, shadow, high;
  float mrate, m1, wrate, init_w;        // m_fModeUpdatingLearnRate, 1 - it, m_fWeightUpdatingLearnRate, m_fLowInitialModeWeight
  int half;                              // taps = 2 half + 1 (0: the map is copied)
  float k[2 * kMlMaxHalf + 1];
};

// a[i] for a lane-varying i without an indexed access: the OR of the masked elements.  (A chain of selects between the elements
// themselves is folded back into one load at a variable address, which puts the array into scratch.)
__device__ __forceinline__ uint32_t ml_get_bits(const uint32_t (&b)[kMlSlots], int i) {
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < kMlSlots; ++j) v |= i == j ? b[j] : 0u;
  return v;
}
__device__ __forceinline__ float ml_get(const float (&a)[kMlSlots], int i) {
  uint32_t b[kMlSlots];
#pragma unroll
  for (int j = 0; j < kMlSlots; ++j) b[j] = __float_as_uint(a[j]);
  return __uint_as_float(ml_get_bits(b, i));
}
__device__ __forceinline__ int ml_get(const int (&a)[kMlSlots], int i) {
  uint32_t b[kMlSlots];
#pragma unroll
  for (int j = 0; j < kMlSlots; ++j) b[j] = (uint32_t)a[j];
  return (int)ml_get_bits(b, i);
}
template <class T>
__device__ __forceinline__ void ml_put(T (&a)[kMlSlots], int i, T v) {
#pragma unroll
  for (int j = 0; j < kMlSlots; ++j) a[j] = i == j ? v : a[j];
}

// CMultiLayerBGS::QuickSort(pData, pIdxes, 0, cnt - 1, false) with an explicit stack: the two halves of a partition are disjoint,
// so the order in which they are finished does not matter.
__device__ __forceinline__ void ml_quicksort_desc(float (&d)[kMlSlots], int (&ix)[kMlSlots], int cnt) {
  uint32_t stack = 0;  // 6 bits per pending range
  int depth = 0, low = 0, high = cnt - 1;
  for (;;) {
    int i = low, j = high;
    const float z = ml_get(d, (low + high) >> 1);
    do {
      while (i < kMlSlots - 1 && ml_get(d, i) > z) ++i;
      while (j > 0 && ml_get(d, j) < z) --j;
      if (i <= j) {
        const float di = ml_get(d, i), dj = ml_get(d, j);
        const int xi = ml_get(ix, i), xj = ml_get(ix, j);
        ml_put(d, i, dj), ml_put(d, j, di), ml_put(ix, i, xj), ml_put(ix, j, xi);
        ++i, --j;
      }
    } while (i <= j);
    if (i < high) stack = (stack << 6) | ((uint32_t)i << 3) | (uint32_t)high, ++depth;
    if (low < j) {
      high = j;
      continue;
    }
    if (!depth) break;
    low = (int)((stack >> 3) & 7), high = (int)(stack & 7), stack >>= 6, --depth;
  }
}

// "sort the list of modes based on the weights of modes" (:725-747 and RemoveBackgroundLayers :1540-1564): the total in list
// order, the sort, then the first prefix above percent * total.  Returns that prefix's length, 0 when there is none.
__device__ __forceinline__ int ml_rerank(int (&rank)[kMlSlots], const float (&w)[kMlSlots], int num, float percent) {
  float d[kMlSlots];
  int ix[kMlSlots];
#pragma unroll
  for (int r = 0; r < kMlSlots; ++r) {
    d[r] = 0.f, ix[r] = 0;
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s)
      if (rank[s] == r) d[r] = w[s], ix[r] = s;
  }
  float tot = 0.f;
  bool sorted = true;  // strictly descending: the sort swaps nothing but an element with itself
#pragma unroll
  for (int r = 0; r < kMlSlots; ++r) {
    if (r < num) tot += d[r];
    if (r + 1 < kMlSlots && r + 1 < num && !(d[r] > d[r + 1])) sorted = false;
  }
  if (!sorted) {
    ml_quicksort_desc(d, ix, num);
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s) {
      if (rank[s] == kMlUnlisted) continue;
#pragma unroll
      for (int r = 0; r < kMlSlots; ++r)
        if (r < num && ix[r] == s) rank[s] = r;
    }
  }
  const float thr = percent * tot;
  float cum = 0.f;
  int found = 0;
#pragma unroll
  for (int r = 0; r < kMlSlots; ++r)
    if (r < num) {
      cum += d[r];
      if (!found && cum > thr) found = r + 1;
    }
  return found;
}

// the tail of RemoveBackgroundLayers (:1568-1587): an ascending sort of the layer numbers of the listed modes, which are distinct
// (DESIGN.md §5.11), renumbered 1, 2, ...: each becomes its rank among them
__device__ __forceinline__ void ml_renumber_layers(const int (&rank)[kMlSlots], int (&lay)[kMlSlots]) {
  int out[kMlSlots];
#pragma unroll
  for (int s = 0; s < kMlSlots; ++s) {
    int below = 0;
#pragma unroll
    for (int t = 0; t < kMlSlots; ++t) below += (rank[t] != kMlUnlisted && lay[t] > 0 && lay[t] < lay[s]) ? 1 : 0;
    out[s] = (rank[s] != kMlUnlisted && lay[s] > 0) ? below + 1 : lay[s];
  }
#pragma unroll
  for (int s = 0; s < kMlSlots; ++s) lay[s] = out[s];
}

__device__ __forceinline__ float ml_max(float a, float b) { return a < b ? b : a; }  // OpenCV's MAX(a, b)
__device__ __forceinline__ float ml_min(float a, float b) { return a > b ? b : a; }  // OpenCV's MIN(a, b)
__device__ __forceinline__ float ml_decay(float wrate, float wc, float mw) { return 1.0f - wrate / (1.0f + wc * mw); }
// the fixture's expf: the correctly rounded value, up to the last bit of the double exp
__device__ __forceinline__ float ml_expf(float x) { return (float)exp((double)x); }

// CalColorBgDist (:984-1002) with CalColorRangeDist, CalVectorsAngle and CalVectorsNoisedAngle (:1085-1217)
__device__ __forceinline__ float ml_color_dist(const MlArgs& a, const float (&c)[3], const float (&bg)[3], uint32_t mxw, uint32_t mnw) {
  bool out = false;
  float dot = 0.f, n1 = 0.f, n2 = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float lo = ml_min((float)byte_of(mnw, ch), bg[ch] * a.shadow - 5.0f), hi = ml_max((float)byte_of(mxw, ch), bg[ch] * a.high + 5.0f);
    out = out || c[ch] > hi || c[ch] < lo;
    dot += bg[ch] * c[ch], n1 += bg[ch] * bg[ch], n2 += c[ch] * c[ch];
  }
  if (out) return 1.0f;
  const float nn = n1 * n2;
  const float org = nn == 0.f ? 0.f : sqrt_rn(ml_max(1.0f - dot * dot / nn, 0.f));  // a sine, not an angle
  const float norm = sqrt_rn(n1);
  float noised = 3.141592653589793f;
  if (norm != 0.f) {
    const float s = a.offset / norm;
    if (s < a.min_sine) noised = a.min_angle;
    else if (!(s >= 1.f)) noised = s;
  }
  float ang = org - noised;
  if (ang < 0.f) ang = 0.f;
  return 1.0f - ml_expf(-100.0f * ang * ang);
}

__device__ __forceinline__ uint32_t ml_pixel(const uint8_t* cur, size_t p) {
  const uint8_t* q = cur + p * 3;
  return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

__global__ __launch_bounds__(kBlock) void ml_model_kernel(const MlArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n) return;
  const size_t k = blockIdx.y, n = a.n;
  const uint8_t* cur = a.cur + k * n * 3;  // this stream's image: every neighbour read below stays inside it
  uint32_t* M = a.model + k * (size_t)kMlPlanes * n + p;
  const uint32_t px = ml_pixel(cur, p);
  const float c[3] = {(float)byte_of(px, 0), (float)byte_of(px, 1), (float)byte_of(px, 2)};

  // ComputeLBP: one level, radius 2, 6 points; a neighbour outside the image reads 0; the noise offset is ROBUST_COLOR_OFFSET
  float cp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a.texture) {
    constexpr int ox[6] = {2, 1, -1, -2, -1, 1}, oy[6] = {0, -2, -2, 0, 2, 2};
    const int y = (int)(p / (uint32_t)a.cols), x = (int)(p - (uint32_t)y * (uint32_t)a.cols);
    const float g = (float)gray_bgr_dword(px);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int xx = x + ox[i], yy = y + oy[i];
      float nb = 0.f;
      if (xx >= 0 && xx < a.cols && yy >= 0 && yy < a.rows) nb = (float)gray_bgr_dword(ml_pixel(cur, (size_t)yy * a.cols + xx));
      cp[i] = (g - nb + 6.0f > 0.f) ? 1.f : 0.f;
    }
  }

  const uint32_t hdr = M[0], lw = M[n];
  int num = (int)(hdr & 7u), bgn = (int)((hdr >> 3) & 7u);
  int rank[kMlSlots], lay[kMlSlots];
  float w[kMlSlots], mw[kMlSlots];
#pragma unroll
  for (int s = 0; s < kMlSlots; ++s) rank[s] = kMlUnlisted;
#pragma unroll
  for (int r = 0; r < kMlSlots; ++r) {
    const int slot = (int)((hdr >> (6 + 3 * r)) & 7u);
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s)
      if (r < num && slot == s) rank[s] = r;
  }
#pragma unroll
  for (int s = 0; s < kMlSlots; ++s) {
    const bool listed = rank[s] != kMlUnlisted;
    lay[s] = listed ? (int)((lw >> (3 * s)) & 7u) : 0;
    w[s] = listed ? __uint_as_float(M[(size_t)(2 + s * kMlSlotPlanes + 9) * n]) : 0.f;
    mw[s] = listed ? __uint_as_float(M[(size_t)(2 + s * kMlSlotPlanes + 10) * n]) : 0.f;
  }

  if (a.learn && num > 0) {  // RemoveBackgroundLayers(PLBP): the first layered mode in list order whose weight fell below 1e-4
    int cr = kMlUnlisted, rl = 0;
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s)
      if (rank[s] != kMlUnlisted && lay[s] != 0 && w[s] < 0.0001f && rank[s] < cr) cr = rank[s], rl = lay[s];
    if (cr != kMlUnlisted) {
#pragma unroll
      for (int s = 0; s < kMlSlots; ++s) {
        if (rank[s] == cr) rank[s] = kMlUnlisted, lay[s] = 0;
        else if (rank[s] != kMlUnlisted) {
          if (rank[s] > cr) --rank[s];
          if (lay[s] > rl) --lay[s];
        }
      }
      --num;
      bgn = ml_rerank(rank, w, num, a.percent);
    }
    ml_renumber_layers(rank, lay);
  }

  // bFirstFrame (:456, :754) is assigned per pixel and ends as "the last pixel's list was empty here".  That is every stream's
  // first frame, and any later frame on which the removal above took the last pixel's only mode.
  if (p == a.n - 1) a.empty_last[k] = num == 0 ? 1u : 0u;

  float raw = 0.f;
  int wslot = -1;  // the slot whose colour and pattern planes are rewritten
  float npat[6], nbg[3];
  uint32_t nmx = px & 0xffffffu, nmn = px & 0xffffffu;
#pragma unroll
  for (int i = 0; i < 6; ++i) npat[i] = cp[i];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) nbg[ch] = c[ch];
  bool changed = a.learn != 0;  // weights, layers and the header are rewritten

  if (num == 0) {  // the empty list (:474-505): a first mode in slot 0, whether learning is disabled or not
    rank[0] = 0, lay[0] = 0, w[0] = a.init_w, mw[0] = a.init_w, num = 1, bgn = 1, wslot = 0, changed = true;
  } else {
    // the best match: the first strictly smaller distance in list order = the smallest (distance, rank)
    float bestd = 999.0f, bpat[6], bbg[3];
    int bestr = kMlUnlisted, bests = 0;
    uint32_t bmx = 0, bmn = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) bpat[i] = 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) bbg[ch] = 0.f;
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s) {
      if (rank[s] == kMlUnlisted) continue;
      const uint32_t* S = M + (size_t)(2 + s * kMlSlotPlanes) * n;
      float pat[6], bg[3];
#pragma unroll
      for (int i = 0; i < 6; ++i) pat[i] = __uint_as_float(S[(size_t)i * n]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) bg[ch] = __uint_as_float(S[(size_t)(6 + ch) * n]);
      const uint32_t mxw = S[(size_t)11 * n], mnw = S[(size_t)12 * n];
      float pd = 0.f;
      if (a.texture) {
#pragma unroll
        for (int i = 0; i < 6; ++i) pd += fabsf(cp[i] - pat[i]) > (1.0f - 0.1f) ? 1.f : 0.f;
        pd /= 6.0f;
      }
      const float d = 0.5f * ml_color_dist(a, c, bg, mxw, mnw) + a.tw * pd;  // m_fColorWeight stays 1 - 0.5
      if (d < bestd || (d == bestd && rank[s] < bestr)) {
        bestd = d, bestr = rank[s], bests = s, bmx = mxw, bmn = mnw;
#pragma unroll
        for (int i = 0; i < 6; ++i) bpat[i] = pat[i];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) bbg[ch] = bg[ch];
      }
    }
    const int bgn0 = bgn;
    const bool updating = bestd < a.upd_thr;
    raw = bestd;
    if (bestr >= bgn && ml_get(mw, bests) < 0.9f) raw = ml_max(raw, a.thr * 2.5f);

    if (a.learn && !updating) {  // no match (:566-655)
#pragma unroll
      for (int s = 0; s < kMlSlots; ++s)
        if (rank[s] != kMlUnlisted) w[s] *= ml_decay(a.wrate, a.wc, mw[s]);
      int t = 0;
      if (num < a.max_modes) {  // the first free physical slot
        bool found = false;
#pragma unroll
        for (int s = 0; s < kMlSlots; ++s)
          if (!found && s < a.max_modes && rank[s] == kMlUnlisted) t = s, found = true;
        ml_put(rank, t, num);
        ++num;
      } else {  // the last of the list
#pragma unroll
        for (int s = 0; s < kMlSlots; ++s)
          if (rank[s] == a.max_modes - 1) t = s;
      }
      ml_put(w, t, a.init_w), ml_put(mw, t, a.init_w), ml_put(lay, t, 0);
      wslot = t;
    } else if (a.learn) {  // match (:656-723)
      const int t = bests;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) nbg[ch] = a.m1 * bbg[ch] + a.mrate * c[ch];
      nmx = nmn = 0;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int v = byte_of(px, ch);
        nmx |= (uint32_t)max(v, byte_of(bmx, ch)) << (8 * ch), nmn |= (uint32_t)min(v, byte_of(bmn, ch)) << (8 * ch);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) npat[i] = a.texture ? a.m1 * bpat[i] + a.mrate * cp[i] : bpat[i];
      float wt = ml_get(w, t), mwt = ml_get(mw, t);
      const float inc = a.wrate * (1.0f + a.wc * mwt);
      wt = (1.0f - inc) * wt + inc;
      mwt = ml_max(wt, mwt);
      ml_put(w, t, wt), ml_put(mw, t, mwt);
      const int lt = ml_get(lay, t);
      if (lt > 0) {
        uint32_t rem = 0;  // by slot
        if (wt > mwt * 0.2f) {
#pragma unroll
          for (int s = 0; s < kMlSlots; ++s)
            if (rank[s] != kMlUnlisted && lay[s] > lt && w[s] < mw[s] * 0.9f) rem |= 1u << s;
        }
        if (rem) {  // RemoveBackgroundLayers(PLBP, removed_modes)
          // the decrements, one removed layer after the other in list order, each against the running value (:1532-1537)
#pragma unroll
          for (int r = 0; r < kMlSlots; ++r) {
            int rl = 0;
#pragma unroll
            for (int s = 0; s < kMlSlots; ++s)
              if (rank[s] == r && (rem >> s & 1u)) rl = lay[s];
            if (rl) {
#pragma unroll
              for (int s = 0; s < kMlSlots; ++s)
                if (rank[s] != kMlUnlisted && !(rem >> s & 1u) && lay[s] > rl) --lay[s];
            }
          }
          int nr[kMlSlots];
#pragma unroll
          for (int s = 0; s < kMlSlots; ++s) {
            int before = 0;
#pragma unroll
            for (int u = 0; u < kMlSlots; ++u) before += ((rem >> u & 1u) && rank[u] < rank[s]) ? 1 : 0;
            nr[s] = (rank[s] == kMlUnlisted || (rem >> s & 1u)) ? kMlUnlisted : rank[s] - before;
          }
#pragma unroll
          for (int s = 0; s < kMlSlots; ++s) {
            rank[s] = nr[s];
            if (rem >> s & 1u) lay[s] = 0;
          }
          num -= __popc(rem);
          bgn = ml_rerank(rank, w, num, a.percent);
          ml_renumber_layers(rank, lay);
        }
      } else if (mwt > 0.9f) {  // a new layer on top
        int top = 0;
#pragma unroll
        for (int s = 0; s < kMlSlots; ++s)
          if (rank[s] != kMlUnlisted) top = max(top, lay[s]);
        ml_put(lay, t, top + 1);
      }
      // "decrease the weights of non-best matched modes" by list position: after a removal bestr is stale, as in the reference
#pragma unroll
      for (int s = 0; s < kMlSlots; ++s)
        if (rank[s] != kMlUnlisted && rank[s] != bestr) w[s] *= ml_decay(a.wrate, a.wc, mw[s]);
      wslot = t;
    }
    if (a.learn && num > 1) {
      const int found = ml_rerank(rank, w, num, a.percent);
      bgn = found ? found : bgn0;
    }
  }

  if (changed) {
    uint32_t h = (uint32_t)num | ((uint32_t)bgn << 3), l = 0;
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s) {
      if (rank[s] == kMlUnlisted) continue;
      h |= (uint32_t)s << (6 + 3 * rank[s]);
      l |= (uint32_t)lay[s] << (3 * s);
      M[(size_t)(2 + s * kMlSlotPlanes + 9) * n] = __float_as_uint(w[s]);
      M[(size_t)(2 + s * kMlSlotPlanes + 10) * n] = __float_as_uint(mw[s]);
    }
    M[0] = h, M[n] = l;
    if (wslot >= 0) {
      uint32_t* S = M + (size_t)(2 + wslot * kMlSlotPlanes) * n;
#pragma unroll
      for (int i = 0; i < 6; ++i) S[(size_t)i * n] = __float_as_uint(npat[i]);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) S[(size_t)(6 + ch) * n] = __float_as_uint(nbg[ch]);
      S[(size_t)11 * n] = nmx, S[(size_t)12 * n] = nmn;
    }
  }
  a.raw[k * n + p] = raw;
  if (a.bgout) {  // GetBackgroundImage after the update: cvRound of the first-ranked mode's bg_intensity
    int top = 0;
#pragma unroll
    for (int s = 0; s < kMlSlots; ++s)
      if (rank[s] == 0) top = s;
    float b[3];
    if (top == wslot) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[ch] = nbg[ch];
    } else {
      const uint32_t* S = M + (size_t)(2 + top * kMlSlotPlanes) * n;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) b[ch] = __uint_as_float(S[(size_t)(6 + ch) * n]);
    }
    uint8_t* o = a.bgout + (k * n + p) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch] = (uint8_t)__float2int_rn(b[ch]);
  }
}

// cvSmooth(CV_GAUSSIAN, 2h+1, 2h+1, sigma, BORDER_REPLICATE) + cvThreshold(BINARY, 255).  Rows: s = k[0] x[0]; s += k[i] x[i] with
// ascending i; columns, the symmetric form: s = k[h] x[c]; s += k[h + i] (x[c + i] + x[c - i]).  float, no contraction.
__global__ __launch_bounds__(kBlock) void ml_smooth_kernel(const MlArgs a) {
  constexpr int W = kMlTileW, H = kMlTileH, MH = kMlMaxHalf;
  __shared__ float in[H + 2 * MH][W + 2 * MH + 1];
  __shared__ float rowp[H + 2 * MH][W + 1];
  const size_t k = blockIdx.z, n = a.n;
  const int bx = blockIdx.x * W, by = blockIdx.y * H, h = a.half, taps = 2 * h + 1, tid = threadIdx.x;
  const int tx = tid % W, ty = tid / W, x = bx + tx, y = by + ty;
  const bool inside = x < a.cols && y < a.rows;
  if (a.empty_last[k]) {  // bFirstFrame: a zero mask and a zero map (uniform over the block)
    if (inside) {
      a.dist[k * n + (size_t)y * a.cols + x] = 0.f;
      if (a.fg) a.fg[k * n + (size_t)y * a.cols + x] = 0;
    }
    return;
  }
  const float* raw = a.raw + k * n;
  const int iw = W + 2 * h, ih = H + 2 * h;
  for (int i = tid; i < iw * ih; i += kBlock) {
    const int ry = i / iw, rx = i - ry * iw;
    const int gy = min(max(by + ry - h, 0), a.rows - 1), gx = min(max(bx + rx - h, 0), a.cols - 1);
    in[ry][rx] = raw[(size_t)gy * a.cols + gx];
  }
  __syncthreads();
  for (int i = tid; i < W * ih; i += kBlock) {
    const int ry = i / W, rx = i - ry * W;
    float s = a.k[0] * in[ry][rx];
    for (int t = 1; t < taps; ++t) s += a.k[t] * in[ry][rx + t];
    rowp[ry][rx] = s;
  }
  __syncthreads();
  float s = a.k[h] * rowp[ty + h][tx];
  for (int t = 1; t <= h; ++t) s += a.k[h + t] * (rowp[ty + h + t][tx] + rowp[ty + h - t][tx]);
  if (inside) {
    a.dist[k * n + (size_t)y * a.cols + x] = s;
    if (a.fg) a.fg[k * n + (size_t)y * a.cols + x] = s > a.thr ? 255 : 0;
  }
}

}  // namespace bgs
