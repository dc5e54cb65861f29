// kernel_multicue.h — the model stage of package_bgs/sjn SJN_MultiCueBGS: everything the class does per pixel.
//
//   mc_reduce_kernel    ReduceImageSize           SJN_MultiCueBGS.cpp:545     src = (int)(i * ((double)H / rh)), a gather
//   (ingest_blur7_kernel with the sigma 0.7 taps)  GaussianFiltering :508     kernel_ingest.h
//   mc_xyz_kernel       BGR2HSVxyz_Par            :568                        double arithmetic as written, PI = 3.14159, (uchar) truncation
//   mc_update_kernel    T_ModelConstruction :1320, C_CodebookConstruction :1804, T_/C_ClearNonEssentialEntries :1423 / :1901,
//                       T_/C_ClearNonEssentialEntriesForCachebook :1494 / :1965, T_/C_Absorption :1612 / :2025, in the orders of
//                       BackgroundModeling_Par :274, EvaluateGhostRegion :1029-1046 and UpdateModel_Par :384-427: ONE launch per call
//   mc_landmark_kernel  T_GetConfidenceMap_Par :1567, CreateLandmarkArray_Par :434
//   mc_reset_kernel     what Initialize :136 leaves of a model, for the streams whose next frame is frame 0, on the launch stream
//
// The books are fixed-capacity slot planes, [stream][book][slot][field][pixel]: every access of a wave is to consecutive pixels of one
// plane.  A pixel has seven independent background books (six texture neighbours and the colour book) and as many cache-books, so the
// update runs one lane per (pixel, book) with the book as blockIdx.y: seven times the waves of a lane per pixel (a 160 x 120 frame
// has only 300 waves of pixels), a seventh of the serial chain per lane, and every wave is all texture or all colour, so the float
// and the double code never share a wave.  The landmark map needs all seven books of a pixel at once and runs one lane per pixel.
// No float atomics and no cross-lane sums: every path gives the same bytes.  The library is built with -ffp-contract=off, so the
// float and double multiplies and adds below round where the reference's scalar code rounds.
#pragma once
#include "bgs_device.h"

namespace bgs {

constexpr int kMcTSlots = 20, kMcTCacheSlots = 16, kMcCSlots = 32, kMcCCacheSlots = 16;  // at least twice the largest books measured (§5.13)
constexpr int kMcBooks = 7;  // per pixel: texture neighbours 0..5, colour 6

// One kind of book, all streams: head i32 [S][K][2][n] = m_iTotal, m_iNumEntries; mean V [S][K][cap][NM][n]; meta i32 [S][K][cap][3][n] =
// MNRL, first, last (K = 6 texture, 1 colour; NM = 1 float mean, 3 double means)
struct McPlanes {
  int* head;
  void* mean;
  int* meta;
  int cap;
};

struct McArgs {
  const uint8_t* xyz;       // [S][n][3]
  const uint8_t* map;       // [S][n] update map (modes 2, 3)
  const uint8_t* landmark;  // [S][n] (mode 3)
  McPlanes tb, tc, cb, cc;  // texture book, texture cache-book, colour book, colour cache-book
  int16_t *tref, *tcnt;     // [S][6][n]
  int16_t *cref, *ccnt;     // [S][n]
  unsigned long long* overflow;
  uint8_t* landmark_out;    // mc_landmark_kernel: [S][n]
  float* conf_out;          // [S][n]
  uint8_t* landmark_copy;   // the caller's d_landmark / d_conf (conf may be null)
  float* conf_copy;
  uint32_t n;
  int rw, rh;
  int mode;                 // 0 training frame, 1 the last training frame (clear with clear_period), 2 ghost, 3 update
  float rate, conf_thr;
  int trange, crange, absorb, absorb_period, clear_period;
};

// the book of one (stream, k, pixel): element (slot j, field f) is f-th plane of slot j, planes n apart
template <class V, int NM>
struct McBook {
  int* head;
  V* mean;
  int* meta;
  size_t n;
  int cap;
  __device__ McBook(const McPlanes& p, size_t book, size_t n_, size_t i) : n(n_), cap(p.cap) {
    head = p.head + book * 2 * n + i;
    mean = (V*)p.mean + book * (size_t)cap * NM * n + i;
    meta = p.meta + book * (size_t)cap * 3 * n + i;
  }
  __device__ int total() const { return head[0]; }
  __device__ int num() const { return min(max(head[n], 0), cap); }
  __device__ V& m(int j, int c) { return mean[((size_t)j * NM + c) * n]; }
  __device__ int& q(int j, int f) { return meta[((size_t)j * 3 + f) * n]; }
  __device__ void move(int from, int to) {
    if (from == to) return;
#pragma unroll
    for (int c = 0; c < NM; ++c) m(to, c) = m(from, c);
#pragma unroll
    for (int f = 0; f < 3; ++f) q(to, f) = q(from, f);
  }
};

struct McSample {
  float d;       // texture: (float)(Z centre - Z neighbour)
  uint8_t p[3];  // colour: X, Y, Z
};

template <class V, int NM>
__device__ __forceinline__ bool mc_match(McBook<V, NM>& b, int j, const McSample& s, int range) {
  if constexpr (NM == 1) {
    const float mu = b.m(j, 0);
    return mu - (float)range <= s.d && s.d <= mu + (float)range;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double mu = b.m(j, c), v = (double)s.p[c];
      if (!(mu - (double)range <= v && v <= mu + (double)range)) return false;
    }
    return true;
  }
}

// T_ModelConstruction / C_CodebookConstruction on one book.  BG: m_bID == 1
template <class V, int NM, bool BG>
__device__ __forceinline__ void mc_construct(McBook<V, NM>& b, const McSample& s, int range, float rate, int16_t* ref, int16_t* cnt, int absorb, unsigned long long* overflow) {
  int num = b.num();
  int matched = -1;
  for (int j = 0; j < num; ++j)
    if (mc_match(b, j, s, range)) {
      matched = j;
      break;
    }
  const int total = b.total() + 1;  // m_iTotal++ before the insert
  b.head[0] = total;
  if (matched < 0) {
    if (num >= b.cap) {  // the reference would grow its array: dropped and counted
      atomicAdd(overflow, 1ull);
      if (!BG) *ref = -1, *cnt = 0;
    } else {
      if constexpr (NM == 1) {
        b.m(num, 0) = s.d;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) b.m(num, c) = (double)s.p[c];
      }
      b.q(num, 0) = BG ? total - 1 : 0, b.q(num, 1) = total, b.q(num, 2) = total;
      b.head[b.n] = ++num;
      if (!BG) *ref = (int16_t)(num - 1), *cnt = 1;
    }
  } else {
    const float neg = 1 - rate;
    if constexpr (NM == 1) {
      const float mu = b.m(matched, 0);
      b.m(matched, 0) = rate * s.d + neg * mu;
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float in = rate * (float)s.p[c];  // a float product
        b.m(matched, c) = (double)in + (double)neg * b.m(matched, c);
      }
    }
    b.q(matched, 2) = total;
    if (!BG) {
      if (matched == (int)*ref)
        *cnt = (int16_t)(*cnt + 1);
      else
        *ref = (int16_t)matched, *cnt = 1;
    }
  }
  if (BG) {
    for (int j = 0; j < num; ++j) {
      const int neg = total - b.q(j, 2) + b.q(j, 1) - 1;
      if (b.q(j, 0) < neg) b.q(j, 0) = neg;
    }
    if (absorb) *ref = -1;
  }
}

// T_/C_ClearNonEssentialEntries
template <class V, int NM>
__device__ __forceinline__ void mc_clear(McBook<V, NM>& b, int period) {
  if (b.total() < period) return;
  const int num = b.num(), stale = (int)(period * 0.5);
  int keep = 0;
  for (int j = 0; j < num; ++j) keep += b.q(j, 0) <= stale;
  int w = 0;
  for (int j = 0; j < num; ++j) {
    if (keep != 0 && keep != num && b.q(j, 0) > stale) continue;
    b.move(j, w);
    b.q(w, 0) = 0, b.q(w, 1) = 1, b.q(w, 2) = 1;
    ++w;
  }
  b.head[b.n] = w;
  b.head[0] = 0;
}

// T_/C_ClearNonEssentialEntriesForCachebook: the literal period 10 and stale threshold 5
template <class V, int NM>
__device__ __forceinline__ void mc_cache_clear(McBook<V, NM>& b, bool lm255, int ref) {
  const int num = b.num(), total = b.total();
  if (total < 10) {
    for (int j = 0; j < num; ++j) b.q(j, 0) = (lm255 && j == ref) ? 0 : b.q(j, 0) + 1;
    b.head[0] = total + 1;
    return;
  }
  int w = 0;
  for (int j = 0; j < num; ++j) {
    if (b.q(j, 0) >= 5) continue;
    b.move(j, w);
    b.q(w, 0) = 0;
    ++w;
  }
  b.head[b.n] = w;
  b.head[0] = 0;
}

// T_/C_Absorption: the referred codeword moves to the end of the background book; the referred index and the count stay as they are
template <class V, int NM>
__device__ __forceinline__ void mc_absorb(McBook<V, NM>& model, McBook<V, NM>& cache, int ref, int cnt, int period, unsigned long long* overflow) {
  if (cnt < period) return;
  const int cnum = cache.num(), mnum = model.num();
  if (ref < 0 || ref >= cnum) return;  // cannot happen after a construction on the cache-book; keeps the index inside the planes
  if (mnum >= model.cap) {
    atomicAdd(overflow, 1ull);
    return;
  }
  const int total = model.total() + 1;
  model.head[0] = total;
#pragma unroll
  for (int c = 0; c < NM; ++c) model.m(mnum, c) = cache.m(ref, c);
  model.q(mnum, 0) = total - 1, model.q(mnum, 1) = total, model.q(mnum, 2) = total;
  model.head[model.n] = mnum + 1;
  for (int j = ref + 1; j < cnum; ++j) cache.move(j, j - 1);
  cache.head[cache.n] = cnum - 1;
}

template <class V, int NM>
__device__ __forceinline__ void mc_book_step(const McArgs& a, McBook<V, NM>& bg, McBook<V, NM>& ca, const McSample& s, int range, int16_t* ref, int16_t* cnt, bool on, bool lm255) {
  if (a.mode <= 1) {  // BackgroundModeling_Par
    mc_construct<V, NM, true>(bg, s, range, a.rate, ref, cnt, a.absorb, a.overflow);
    if (a.mode == 1) mc_clear(bg, a.clear_period);
    return;
  }
  if (on) {
    mc_construct<V, NM, true>(bg, s, range, a.rate, ref, cnt, a.absorb, a.overflow);
    mc_clear(bg, a.clear_period);
  } else if (a.mode == 3 && a.absorb) {
    mc_construct<V, NM, false>(ca, s, range, a.rate, ref, cnt, a.absorb, a.overflow);
    mc_absorb(bg, ca, (int)*ref, (int)*cnt, a.absorb_period, a.overflow);
  }
  if (a.mode == 3 && a.absorb) mc_cache_clear(ca, lm255, (int)*ref);
}

__device__ __forceinline__ bool mc_interior(int x, int y, int rw, int rh) { return x >= 2 && x < rw - 2 && y >= 2 && y < rh - 2; }

// grid (blocks of pixels, kMcBooks, streams)
__global__ __launch_bounds__(kBlock) void mc_update_kernel(const McArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const int y = (int)(i / (uint32_t)a.rw), x = (int)(i - (uint32_t)y * a.rw);
  if (!mc_interior(x, y, a.rw, a.rh)) return;
  const size_t n = a.n, st = blockIdx.z, k = blockIdx.y;
  const uint8_t* xyz = a.xyz + st * n * 3;
  const bool on = a.mode >= 2 && a.map[st * n + i] != 0;
  if (a.mode == 2 && !on) return;
  const bool lm255 = a.mode == 3 && a.landmark[st * n + i] == 255;
  McSample s;
  if (k < 6) {
    constexpr int dx[6] = {-2, -1, 1, 2, 1, -1}, dy[6] = {0, -2, -2, 0, 2, 2};
    const size_t j = (size_t)(y + dy[k]) * a.rw + (x + dx[k]);  // inside the frame: the pixel is interior
    s.d = (float)((int)xyz[(size_t)i * 3 + 2] - (int)xyz[j * 3 + 2]);
    const size_t book = st * 6 + k;
    McBook<float, 1> bg(a.tb, book, n, i), ca(a.tc, book, n, i);
    mc_book_step(a, bg, ca, s, a.trange, a.tref + book * n + i, a.tcnt + book * n + i, on, lm255);
  } else {
    s.d = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s.p[c] = xyz[(size_t)i * 3 + c];
    McBook<double, 3> bg(a.cb, st, n, i), ca(a.cc, st, n, i);
    mc_book_step(a, bg, ca, s, a.crange, a.cref + st * n + i, a.ccnt + st * n + i, on, lm255);
  }
}

// grid (blocks of pixels, streams): what a stream's frame 0 must find, written on the stream that frame is launched on (a new handle
// and a stream after bgs_multicue_reset_stream alike).  The planes a later kernel reads before it writes them:
//   the four heads (m_iTotal, m_iNumEntries)  0: mc_construct reads both; with m_iNumEntries 0 no slot of mean / meta is read, and
//                                             bgs_multicue_get_state shows slots at and beyond it as 0, so those planes stay as they are
//   tref / cref -1, tcnt / ccnt 0             the cache-book path of mode 3 compares and counts them; training writes tref / cref only with
//                                             absorption on, and never the counts
//   conf / landmark 0                         read by no kernel before mc_landmark_kernel writes every pixel of them (the 2-pixel border
//                                             included), but a training stream shows them through bgs_multicue_get_state
// Everything else is written whole before it is read: red / gauss / xyz by the three PreProcessing launches of every frame, the scratch
// maps, the counts and the boxes of the whole-frame step by mc_landmark_kernel, mc_box_prepare_kernel and mc_box_label_kernel.
__global__ __launch_bounds__(kBlock) void mc_reset_kernel(const McArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const size_t n = a.n, st = blockIdx.y;
#pragma unroll
  for (size_t k = 0; k < 6; ++k) {
    const size_t book = st * 6 + k;
    a.tb.head[book * 2 * n + i] = 0, a.tb.head[(book * 2 + 1) * n + i] = 0;
    a.tc.head[book * 2 * n + i] = 0, a.tc.head[(book * 2 + 1) * n + i] = 0;
    a.tref[book * n + i] = -1, a.tcnt[book * n + i] = 0;
  }
  a.cb.head[st * 2 * n + i] = 0, a.cb.head[(st * 2 + 1) * n + i] = 0;
  a.cc.head[st * 2 * n + i] = 0, a.cc.head[(st * 2 + 1) * n + i] = 0;
  a.cref[st * n + i] = -1, a.ccnt[st * n + i] = 0;
  a.conf_out[st * n + i] = 0.f, a.landmark_out[st * n + i] = 0;
}

// grid (blocks of pixels, streams): T_GetConfidenceMap_Par and CreateLandmarkArray_Par
__global__ __launch_bounds__(kBlock) void mc_landmark_kernel(const McArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const size_t n = a.n, st = blockIdx.y;
  const int y = (int)(i / (uint32_t)a.rw), x = (int)(i - (uint32_t)y * a.rw);
  float conf = 0.f;
  uint8_t lm = 0;
  if (mc_interior(x, y, a.rw, a.rh)) {
    constexpr int dx[6] = {-2, -1, 1, 2, 1, -1}, dy[6] = {0, -2, -2, 0, 2, 2};
    const uint8_t* xyz = a.xyz + st * n * 3;
    const int z = xyz[(size_t)i * 3 + 2];
    const float tr = (float)a.trange;
    int matched = 0;
    double back = 0, cntd = 0, input = 0;
    for (int k = 0; k < 6; ++k) {
      const size_t j = (size_t)(y + dy[k]) * a.rw + (x + dx[k]);
      const int di = z - (int)xyz[j * 3 + 2];
      const float d = (float)di;
      input += (double)abs(di);
      McBook<float, 1> b(a.tb, st * 6 + k, n, i);
      const int num = b.num();
      bool hit = false;
      for (int e = 0; e < num; ++e) {
        const float mu = b.m(e, 0);
        back += (double)mu;
        cntd += 1.0;
        if (!hit && (mu - tr) - 5.f <= d && d <= (mu + tr) + 5.f) hit = true;
      }
      matched += hit;
    }
    conf = 1 - (float)matched / 6.f;
    if (conf > a.conf_thr) {
      lm = 255;
    } else {
      back /= cntd;  // no entries: NaN, which is not below 50
      if (back < 50 && input < 50) {
        McBook<double, 3> c(a.cb, st, n, i);
        const int num = c.num();
        bool m = false;
        for (int e = 0; e < num && !m; ++e) {
          int ok = 0;
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const double mu = c.m(e, q), v = (double)xyz[(size_t)i * 3 + q];
            ok += (mu - (double)a.crange - 10 <= v && v <= mu + (double)a.crange + 10);
          }
          m = ok == 3;
        }
        lm = m ? 125 : 255;
      }
    }
  }
  a.landmark_out[st * n + i] = lm;
  a.conf_out[st * n + i] = conf;
  a.landmark_copy[st * n + i] = lm;
  if (a.conf_copy) a.conf_copy[st * n + i] = conf;
}

// ReduceImageSize: one lane per reduced pixel; grid (blocks of pixels, streams).  fh = (double)H / rh, fw = (double)W / rw
__global__ __launch_bounds__(kBlock) void mc_reduce_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int cols, int rh, int rw, double fh, double fw) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x, n = (uint32_t)rh * rw;
  if (i >= n) return;
  const int y = (int)(i / (uint32_t)rw), x = (int)(i - (uint32_t)y * rw);
  const int sy = min(max((int)(y * fh), 0), rows - 1), sx = min(max((int)(x * fw), 0), cols - 1);  // the clamps never bind: (int)(i * (H / rh)) < H
  const uint8_t* s = src + ((size_t)blockIdx.y * rows * cols + (size_t)sy * cols + sx) * 3;
  uint8_t* d = dst + ((size_t)blockIdx.y * n + i) * 3;
  d[0] = s[0], d[1] = s[1], d[2] = s[2];
}

// BGR2HSVxyz_Par on one pixel
__device__ __forceinline__ void mc_xyz(const uint8_t* bgr, uint8_t* out) {
  const double dB = (double)bgr[0] / 255, dG = (double)bgr[1] / 255, dR = (double)bgr[2] / 255;
  const double dMin = fmin(fmin(dR, dG), dB), dMax = fmax(fmax(dR, dG), dB);  // MIN3 / MAX3 pick a value; which operand is immaterial
  const double dV = dMax;
  double dS = 0, dH = 0;
  if (dV != 0) {
    dS = (dMax - dMin) / dMax;
    if (dS != 0) {
      if (dMax == dR) {
        dH = 60 * (dG - dB) / dS;
        if (dH < 0) dH = 360 + dH;
      } else if (dMax == dG) {
        dH = 120 + 60 * (dB - dR) / dS;
      } else {
        dH = 240 + 60 * (dR - dG) / dS;
      }
    }
  }
  dH = dH * ((2 * 3.14159) / 360);
  out[0] = (uint8_t)(int)((dV * dS * cos(dH) * 127.5) + 127.5);
  out[1] = (uint8_t)(int)((dV * dS * sin(dH) * 127.5) + 127.5);
  out[2] = (uint8_t)(int)(dV * 255);
}

__global__ __launch_bounds__(kBlock) void mc_xyz_kernel(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ xyz, size_t pixels) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= pixels) return;
  uint8_t o[3];
  mc_xyz(bgr + i * 3, o);
  xyz[i * 3] = o[0], xyz[i * 3 + 1] = o[1], xyz[i * 3 + 2] = o[2];
}

}  // namespace bgs
