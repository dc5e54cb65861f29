// kernel_lb.h — Laurence Bender's package_bgs/lb/ models on gfx950, one fused launch per frame and class over streams x pixels
// (lb_*_kernel), and for clip calls one launch per 8 / 4 / 2 frames that keeps the pixel's model in registers (lb_*_clip_kernel):
//   LBSimpleGaussian     (BGS_LB_SIMPLE_GAUSSIAN, USTC_BGS type 25)     lb/BGModelGauss.cpp:125-198
//   LBFuzzyGaussian      (BGS_LB_FUZZY_GAUSSIAN, type 26)               lb/BGModelFuzzyGauss.cpp:130-208
//   LBMixtureOfGaussians (BGS_LB_MOG, type 27)                          lb/BGModelMog.cpp:144-307
//   LBAdaptiveSOM        (BGS_LB_ADAPTIVE_SOM, type 28)                 lb/BGModelSom.cpp:185-289
//   LBFuzzyAdaptiveSOM   (BGS_LB_FUZZY_ADAPTIVE_SOM, type 29)           lb/BGModelFuzzySom.cpp:185-296
// Every model value is an IEEE double and every expression is written in the reference's order of operations; the library is
// built with -ffp-contract=off, `/` and sqrt on doubles are correctly rounded on gfx950 and double denormals are never flushed, so
// the three classes without exp() equal the reference bit for bit - masks, background bytes and every model plane - and the two
// fuzzy ones up to the last bit of exp().  The reference names its colour fields Blue, Green, Red over B, G, R
// bytes and sums every distance Red term first: (byte 2 + byte 1) + byte 0.
//
// Model layout: planar doubles, stream-major, [S][P][n], so consecutive lanes read consecutive 8-byte words and a
// run of streams [first, first + count) is one contiguous slab:
//   Gaussians  P = 6   plane c = mu[c], 3 + c = var[c]                     (c = byte of the pixel: 0 B, 1 G, 2 R)
//   MoG        P = 21  plane 7 k = w of slot k, 7 k + 1 + c = mu, 7 k + 4 + c = var;  K in an int32 plane [S][n] of its own.
//                      sortKey is not stored: after every frame it is w / sqrt(var sum) of the stored values.  Slots >= K are
//                      never read or written.
//   SOMs       P = 27  plane (3 l + k) 3 + c = neuron row l, column k;  the background bytes in a u8 plane [S][n][3] of their own
//                      (a foreground pixel keeps the bytes of the last frame it was background).  The reference's padding cells
//                      between pixels are written by its update and never read by a BMU search: not modelled.
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgs_device.h"

namespace bgs {

constexpr int kLbGaussPlanes = 6, kLbMogPlanes = 21, kLbSomPlanes = 27;
constexpr int kLbTable = 16;  // streams one launch can give their own (alpha, epsilon)

struct LbArgs {
  const uint8_t* cur;  // [npix][3] frames of the run's streams
  uint8_t* fg;         // [npix] byte masks (nullable)
  uint8_t* bg;         // [npix][3] background images (nullable)
  uint64_t* fg_bits;   // packed masks (nullable; npix % 64 == 0 then)
  double* model;       // the run's first stream: [count][P][n]
  int32_t* k;          // MoG: [count][n]
  uint8_t* bgplane;    // SOMs: [count][n][3]
  uint32_t npix, n;
  uint32_t bps;        // SOMs: workgroups per stream, ceil(n / kBlock)
  int init;            // first frame of these streams: Init() from the frame, then the same frame's Update()
  double threshold;    // Gaussians / MoG: m_threshold (squared Mahalanobis distance)
  double noise;        // m_noise of this frame
  double noise0;       // m_noise as the constructor left it: what Init() sees (it runs before the first setBGModelParameter)
  double alpha;        // m_alpha / m_alphamax
  double bg_threshold; // FuzzyGaussian m_threshBG, MoG m_T
  int uniform;         // SOMs: every stream of the launch uses alpha_s[0] / eps_s[0]
  double alpha_s[kLbTable], eps_s[kLbTable];  // SOMs: alpha and epsilon of each stream of the launch (its own training counter)
};

// A run of T = 8 / 4 / 2 consecutive frames of the same streams (bgs_process_clip_device).  `a` describes frame 0; frame t of the
// run lies t strides further in every input and output.  a.init applies to frame 0 only; a.alpha_s / a.eps_s are not read.
struct LbClipArgs {
  LbArgs a;
  size_t frame_stride;          // bytes from one frame to the next in cur and bg: 3 x the pixels of the caller's slab
  size_t fg_stride;             // bytes in fg
  size_t bits_stride;           // words in fg_bits
  double alpha_t[8], eps_t[8];  // SOMs: alpha and epsilon of every frame of the run (the streams of a run share m_K)
};

// `m += a * d` behind the reference's "speed hack" guard
__device__ __forceinline__ double lb_step(double m, double a, double d) { return d * d > DBL_MIN ? m + a * d : m; }

// element of a plane: wave-uniform base + 32-bit lane byte offset (the scalar-base addressing mode)
__device__ __forceinline__ double* lb_lane(double* plane, uint32_t byte_off) { return reinterpret_cast<double*>(reinterpret_cast<char*>(plane) + byte_off); }

__device__ __forceinline__ void lb_write_mask(uint8_t* fg, uint64_t* fg_bits, uint32_t p, bool active, uint8_t m) {
  if (active && fg) fg[p] = m;
  if (fg_bits) {  // npix % 64 == 0 is checked on the host: a wave is either all active or all idle
    const unsigned long long w = __ballot(active && m != 0);
    if ((threadIdx.x & (kWave - 1)) == 0 && active) fg_bits[p >> 6] = w;
  }
}
__device__ __forceinline__ void lb_write_mask(const LbArgs& a, uint32_t p, bool active, uint8_t m) { lb_write_mask(a.fg, a.fg_bits, p, active, m); }
// frame t of a clip run
__device__ __forceinline__ void lb_write_mask(const LbClipArgs& c, int t, uint32_t p, bool active, uint8_t m) {
  lb_write_mask(c.a.fg ? c.a.fg + t * c.fg_stride : nullptr, c.a.fg_bits ? c.a.fg_bits + t * c.bits_stride : nullptr, p, active, m);
}

// One pixel of BGModelGauss::Update / BGModelFuzzyGauss::Update.  mu, var in pixel byte order; returns the mask byte.
template <bool FUZZY>
__device__ __forceinline__ uint8_t lb_gauss_pixel(const LbArgs& a, const double (&src)[3], double (&mu)[3], double (&var)[3]) {
  const double dr = src[2] - mu[2], dg = src[1] - mu[1], db = src[0] - mu[0];
  const double d2 = dr * dr / var[2] + dg * dg / var[1] + db * db / var[0];
  double alpha = a.alpha, fuzzy = 1.0;
  if constexpr (FUZZY) {
    if (d2 < a.threshold) fuzzy = d2 / a.threshold;
    alpha = a.alpha * exp(-5.0 * fuzzy);
  }
  mu[2] = lb_step(mu[2], alpha, dr), mu[1] = lb_step(mu[1], alpha, dg), mu[0] = lb_step(mu[0], alpha, db);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double e = src[c] - mu[c], d = e * e - var[c];
    var[c] = lb_step(var[c], alpha, d);
    var[c] = FUZZY ? fmax(var[c], a.noise) : fmin(var[c], a.noise);  // BGModelGauss.cpp:182-184 is a ceiling, the fuzzy model a floor
  }
  if constexpr (FUZZY) return fuzzy >= a.bg_threshold ? 255 : 0;
  return d2 < a.threshold ? 0 : 255;
}

// The six planes of PX pixels of a lane (PX = 2: one double2 per plane).
template <int PX>
__device__ __forceinline__ void lb_gauss_load(const double* base, uint32_t n, double (&mu)[PX][3], double (&var)[PX][3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (PX == 2) {
      const double2 m = *reinterpret_cast<const double2*>(base + (size_t)c * n), v = *reinterpret_cast<const double2*>(base + (size_t)(3 + c) * n);
      mu[0][c] = m.x, mu[1][c] = m.y, var[0][c] = v.x, var[1][c] = v.y;
    } else {
      mu[0][c] = base[(size_t)c * n], var[0][c] = base[(size_t)(3 + c) * n];
    }
  }
}
template <int PX>
__device__ __forceinline__ void lb_gauss_put(double* base, uint32_t n, const double (&mu)[PX][3], const double (&var)[PX][3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (PX == 2) {
      *reinterpret_cast<double2*>(base + (size_t)c * n) = make_double2(mu[0][c], mu[1][c]);
      *reinterpret_cast<double2*>(base + (size_t)(3 + c) * n) = make_double2(var[0][c], var[1][c]);
    } else {
      base[(size_t)c * n] = mu[0][c], base[(size_t)(3 + c) * n] = var[0][c];
    }
  }
}
// background image and byte mask of the lane's PX pixels (either nullable)
template <int PX>
__device__ __forceinline__ void lb_gauss_out(uint8_t* bg, uint8_t* fg, uint32_t p0, const double (&mu)[PX][3], uint32_t nib) {
  if (bg) {
    uint8_t* o = bg + (size_t)p0 * 3;
#pragma unroll
    for (int q = 0; q < PX; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[q * 3 + c] = (uint8_t)(int)mu[q][c];  // (unsigned char) of a double in 0..255: truncation
  }
  if (fg) {
#pragma unroll
    for (int q = 0; q < PX; ++q) fg[p0 + q] = (nib >> q) & 1u ? 255 : 0;
  }
}
template <int PX>
__device__ __forceinline__ void lb_gauss_bits(uint64_t* fg_bits, uint32_t p0, uint32_t nib, bool active) {
  if constexpr (PX == 1) {
    const unsigned long long w = __ballot(active && nib != 0);
    if ((threadIdx.x & (kWave - 1)) == 0 && active) fg_bits[p0 >> 6] = w;
  } else {
    store_packed_mask<PX>(fg_bits, p0, nib, active);
  }
}

// PX pixels per lane: 8 or 16 bytes per lane and plane (DESIGN.md §6.3c has both measured).  PX = 2 needs an even n.
template <bool FUZZY, int PX>
__global__ __launch_bounds__(kBlock) void lb_gauss_kernel(const LbArgs a) {
  const uint32_t p0 = (uint32_t)(blockIdx.x * kBlock + threadIdx.x) * PX;
  const bool active = p0 < a.npix;
  uint32_t nib = 0;
  if (active) {
    const uint32_t s = p0 / a.n, i = p0 - s * a.n;
    double* base = a.model + (size_t)s * kLbGaussPlanes * a.n + i;
    double src[PX][3], mu[PX][3], var[PX][3];
    const uint8_t* px = a.cur + (size_t)p0 * 3;
#pragma unroll
    for (int q = 0; q < PX; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) src[q][c] = (double)px[q * 3 + c];
    if (a.init) {
#pragma unroll
      for (int q = 0; q < PX; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[q][c] = src[q][c], var[q][c] = a.noise0;
    } else {
      lb_gauss_load<PX>(base, a.n, mu, var);
    }
#pragma unroll
    for (int q = 0; q < PX; ++q) nib |= (lb_gauss_pixel<FUZZY>(a, src[q], mu[q], var[q]) ? 1u : 0u) << q;
    lb_gauss_put<PX>(base, a.n, mu, var);
    lb_gauss_out<PX>(a.bg, a.fg, p0, mu, nib);
  }
  if (a.fg_bits) lb_gauss_bits<PX>(a.fg_bits, p0, nib, active);
}

// T frames of the same pixels in one launch: the T frames' bytes are loaded first, the six planes are read once, the frames are
// applied in order in registers, every frame's mask and background go out at their own strides, and the planes are written once.
template <bool FUZZY, int PX, int T>
__global__ __launch_bounds__(kBlock) void lb_gauss_clip_kernel(const LbClipArgs c) {
  const LbArgs& a = c.a;
  const uint32_t p0 = (uint32_t)(blockIdx.x * kBlock + threadIdx.x) * PX;
  const bool active = p0 < a.npix;
  uint32_t nibs = 0;  // PX mask bits per frame, frame t at bit PX t
  if (active) {
    const uint32_t s = p0 / a.n, i = p0 - s * a.n;
    double* base = a.model + (size_t)s * kLbGaussPlanes * a.n + i;
    uint8_t raw[T][PX * 3];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const uint8_t* px = a.cur + t * c.frame_stride + (size_t)p0 * 3;
#pragma unroll
      for (int j = 0; j < PX * 3; ++j) raw[t][j] = px[j];
    }
    double mu[PX][3], var[PX][3];
    if (a.init) {  // Init() from the run's first frame
#pragma unroll
      for (int q = 0; q < PX; ++q)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) mu[q][ch] = (double)raw[0][q * 3 + ch], var[q][ch] = a.noise0;
    } else {
      lb_gauss_load<PX>(base, a.n, mu, var);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      uint32_t nib = 0;
#pragma unroll
      for (int q = 0; q < PX; ++q) {
        const double src[3] = {(double)raw[t][q * 3], (double)raw[t][q * 3 + 1], (double)raw[t][q * 3 + 2]};
        nib |= (lb_gauss_pixel<FUZZY>(a, src, mu[q], var[q]) ? 1u : 0u) << q;
      }
      nibs |= nib << (PX * t);
      lb_gauss_out<PX>(a.bg ? a.bg + t * c.frame_stride : nullptr, a.fg ? a.fg + t * c.fg_stride : nullptr, p0, mu, nib);
    }
    lb_gauss_put<PX>(base, a.n, mu, var);
  }
  if (a.fg_bits) {
#pragma unroll
    for (int t = 0; t < T; ++t) lb_gauss_bits<PX>(a.fg_bits + t * c.bits_stride, p0, (nibs >> (PX * t)) & ((1u << PX) - 1u), active);
  }
}

// One frame of BGModelMog::Update for one pixel whose K modes are in registers; returns the mask byte.  Slot arrays are indexed by
// unrolled loops only (registers, no scratch).  dirty[k] is set for every slot whose mu / var changed and never cleared here, so
// over several frames it is the union of their write sets.
__device__ __forceinline__ uint8_t lb_mog_pixel(const LbArgs& a, const double (&src)[3], int& K, double (&w)[3], double (&mu)[3][3], double (&var)[3][3], bool (&dirty)[3]) {
  // the first mode within the threshold, not the nearest one (BGModelMog.cpp:168-181)
  int hit = -1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < K && hit < 0) {
      const double dr = src[2] - mu[k][2], dg = src[1] - mu[k][1], db = src[0] - mu[k][0];
      const double d2 = dr * dr / var[k][2] + dg * dg / var[k][1] + db * db / var[k][0];
      if (d2 < a.threshold) hit = k;
    }
  }
  if (hit >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k >= K) continue;
      if (k == hit) {
        w[k] = w[k] + a.alpha * (1.0 - w[k]);
#pragma unroll
        for (int c = 2; c >= 0; --c) mu[k][c] = lb_step(mu[k][c], a.alpha, src[c] - mu[k][c]);
#pragma unroll
        for (int c = 2; c >= 0; --c) {
          const double e = src[c] - mu[k][c], d = e * e - var[k][c];
          var[k][c] = fmax(lb_step(var[k][c], a.alpha, d), a.noise);
        }
        dirty[k] = true;
      } else {
        w[k] = (1.0 - a.alpha) * w[k];
      }
    }
  } else {  // a new mode; with all three in use the last one is replaced
    if (K < 3) ++K;
    hit = K - 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k != hit) continue;
      w[k] = K == 1 ? 1.0 : (double)0.001f;  // LEARNINGRATEMOG, not m_alpha (BGModelMog.cpp:236-239)
#pragma unroll
      for (int c = 0; c < 3; ++c) mu[k][c] = src[c], var[k][c] = a.noise;
      dirty[k] = true;
    }
  }
  double wsum = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < K) wsum += w[k];
  const double wf = 1.0 / wsum;
  double key[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < K) {
      w[k] *= wf;
      key[k] = w[k] / __builtin_sqrt(var[k][2] + var[k][1] + var[k][0]);
    }
  // one swap towards the front (BGModelMog.cpp:267-274)
  double key_hit = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k == hit) key_hit = key[k];
  int sw = -1;
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (k < hit && sw < 0 && key_hit > key[k]) sw = k;
  if (sw >= 0) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 1; y < 3; ++y)
        if (x == sw && y == hit) {
          double t = w[x];
          w[x] = w[y], w[y] = t;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            t = mu[x][c], mu[x][c] = mu[y][c], mu[y][c] = t;
            t = var[x][c], var[x][c] = var[y][c], var[y][c] = t;
          }
          dirty[x] = dirty[y] = true;
        }
  }
  // background modes: the first k whose cumulative weight passes m_T (m_T < 1 and the weights sum to 1: always found).  kHit is
  // still the slot index from before the swap - std::swap moved the data, not the index (BGModelMog.cpp:271, :291)
  int kbg = 2;
  double acc = 0.0;
  bool found = false;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < K && !found) {
      acc += w[k];
      if (acc > a.bg_threshold) kbg = k, found = true;
    }
  return hit > kbg ? 255 : 0;
}

// The pixel's modes into registers: Init() from `src` (one mode at the pixel, the constructor's variance) or the K stored slots.
__device__ __forceinline__ void lb_mog_load(const LbArgs& a, const double* base, uint32_t p, const double (&src)[3], int& K, double (&w)[3], double (&mu)[3][3],
                                            double (&var)[3][3], bool (&dirty)[3]) {
  if (a.init) {
    K = 1, w[0] = 1.0, dirty[0] = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[0][c] = src[c], var[0][c] = a.noise0;
  } else {
    K = a.k[p];
  }
  const int K0 = a.init ? 0 : K;  // slots that exist in memory
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < K0) {
      w[k] = base[(size_t)(7 * k) * a.n];
#pragma unroll
      for (int c = 0; c < 3; ++c) mu[k][c] = base[(size_t)(7 * k + 1 + c) * a.n], var[k][c] = base[(size_t)(7 * k + 4 + c) * a.n];
    } else if (k >= K) {
#pragma unroll
      for (int c = 0; c < 3; ++c) mu[k][c] = 0.0, var[k][c] = 1.0;
    }
  }
}

// K, the weights of the live slots and mu / var of the dirty ones
__device__ __forceinline__ void lb_mog_put(const LbArgs& a, double* base, uint32_t p, int K, const double (&w)[3], const double (&mu)[3][3], const double (&var)[3][3],
                                             const bool (&dirty)[3]) {
  a.k[p] = K;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < K) {
      base[(size_t)(7 * k) * a.n] = w[k];
      if (dirty[k]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) base[(size_t)(7 * k + 1 + c) * a.n] = mu[k][c], base[(size_t)(7 * k + 4 + c) * a.n] = var[k][c];
      }
    }
}

__global__ __launch_bounds__(kBlock) void lb_mog_kernel(const LbArgs a) {
  const uint32_t p = (uint32_t)(blockIdx.x * kBlock + threadIdx.x);
  const bool active = p < a.npix;
  uint8_t m = 0;
  if (active) {
    const uint32_t s = p / a.n, i = p - s * a.n;
    double* base = a.model + (size_t)s * kLbMogPlanes * a.n + i;
    const uint8_t* px = a.cur + (size_t)p * 3;
    const double src[3] = {(double)px[0], (double)px[1], (double)px[2]};
    double w[3] = {0, 0, 0}, mu[3][3], var[3][3];
    bool dirty[3] = {false, false, false};  // slots whose mu / var must be written back
    int K;
    lb_mog_load(a, base, p, src, K, w, mu, var, dirty);
    m = lb_mog_pixel(a, src, K, w, mu, var, dirty);
    lb_mog_put(a, base, p, K, w, mu, var, dirty);
    if (a.bg) {
      uint8_t* o = a.bg + (size_t)p * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(int)mu[0][c];
    }
  }
  lb_write_mask(a, p, active, m);
}

// T frames in one launch: the modes are read once, K and the weights are written once, and mu / var of the slots that any of
// the T frames changed (a slot that came to life during the run is dirty from the frame that made it).
template <int T>
__global__ __launch_bounds__(kBlock) void lb_mog_clip_kernel(const LbClipArgs c) {
  const LbArgs& a = c.a;
  const uint32_t p = (uint32_t)(blockIdx.x * kBlock + threadIdx.x);
  const bool active = p < a.npix;
  uint32_t ms = 0;  // bit t: frame t's pixel is foreground
  if (active) {
    const uint32_t s = p / a.n, i = p - s * a.n;
    double* base = a.model + (size_t)s * kLbMogPlanes * a.n + i;
    uint8_t raw[T][3];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const uint8_t* px = a.cur + t * c.frame_stride + (size_t)p * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) raw[t][j] = px[j];
    }
    double w[3] = {0, 0, 0}, mu[3][3], var[3][3];
    bool dirty[3] = {false, false, false};
    int K;
    {
      const double src[3] = {(double)raw[0][0], (double)raw[0][1], (double)raw[0][2]};
      lb_mog_load(a, base, p, src, K, w, mu, var, dirty);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const double src[3] = {(double)raw[t][0], (double)raw[t][1], (double)raw[t][2]};
      if (lb_mog_pixel(a, src, K, w, mu, var, dirty)) ms |= 1u << t;
      if (a.bg) {
        uint8_t* o = a.bg + t * c.frame_stride + (size_t)p * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch] = (uint8_t)(int)mu[0][ch];
      }
    }
    lb_mog_put(a, base, p, K, w, mu, var, dirty);
  }
#pragma unroll
  for (int t = 0; t < T; ++t) lb_write_mask(c, t, p, active, (ms >> t) & 1u ? 255 : 0);
}

// One frame of BGModelSom::Update / BGModelFuzzySom::Update for one pixel whose 27 doubles are in registers (unrolled indexing
// only).  Returns whether the pixel is background; hitc = the best-matching unit after the update; bit j of `touched` is set for
// every neuron inside the 3 x 3 window around that unit - 4 for a corner, 6 for an edge, 9 for the centre - and never cleared
// here, so over several frames it is the union of their write sets.  The plain SOM leaves a foreground pixel's model untouched.
template <bool FUZZY>
__device__ __forceinline__ bool lb_som_pixel(double alpha, double eps, const double (&src)[3], double (&som)[9][3], uint32_t& touched, double (&hitc)[3]) {
  // best-matching unit: the first strict minimum in row-major order
  double d2min = DBL_MAX;
  int hit = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const double dr = src[2] - som[j][2], dg = src[1] - som[j][1], db = src[0] - som[j][0];
    const double d2 = dr * dr + dg * dg + db * db;
    if (d2 < d2min) d2min = d2, hit = j;
  }
  const int hl = hit / 3, hk = hit - 3 * hl;
  bool update, isbg;
  double rate = alpha;
  if constexpr (FUZZY) {
    double fuzzy = 1.0;
    if (d2min < eps) fuzzy = d2min / eps;
    rate = alpha * exp(-5.0 * fuzzy);
    update = true, isbg = !(fuzzy >= 0.8);
  } else {
    update = isbg = d2min <= eps;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) hitc[c] = 0;
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int j = 3 * l + k, dl = l - hl, dk = k - hk;
      const bool in = update && dl >= -1 && dl <= 1 && dk >= -1 && dk <= 1;
      // Pascal kernel (1 2 1) x (1 2 1): 4 at the unit, 2 beside it, 1 diagonally
      const double wgt = (dl == 0 ? 2.0 : 1.0) * (dk == 0 ? 2.0 : 1.0);
      const double g = rate * wgt;
      if (in) {
#pragma unroll
        for (int c = 0; c < 3; ++c) som[j][c] = lb_step(som[j][c], g, src[c] - som[j][c]);
        touched |= 1u << j;
      }
      if (j == hit) {
#pragma unroll
        for (int c = 0; c < 3; ++c) hitc[c] = som[j][c];
      }
    }
  return isbg;
}

// The nine neurons into registers: Init() puts all of them at the pixel (and all of them are written back), else 27 independent
// loads in flight.  Plane access is wave-uniform base + one 32-bit lane offset (see lb_som_kernel).
__device__ __forceinline__ void lb_som_load(const LbArgs& a, double* base, uint32_t off, const double (&src)[3], double (&som)[9][3], uint32_t& touched) {
  if (a.init) {
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) som[j][c] = src[c];
    touched = 0x1ffu;
  } else {
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) som[j][c] = *lb_lane(base + (size_t)(3 * j + c) * a.n, off);
    touched = 0;
  }
}
__device__ __forceinline__ void lb_som_put(const LbArgs& a, double* base, uint32_t off, const double (&som)[9][3], uint32_t touched) {
#pragma unroll
  for (int j = 0; j < 9; ++j)
    if ((touched >> j) & 1u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *lb_lane(base + (size_t)(3 * j + c) * a.n, off) = som[j][c];
    }
}

template <bool FUZZY>
__global__ __launch_bounds__(kBlock) void lb_som_kernel(const LbArgs a) {
  // A workgroup never straddles two streams (grid = streams x bps): the stream index and with it the 27 plane bases are wave-uniform,
  // so every plane access is scalar base + one 32-bit lane offset instead of 27 address pairs held in vector registers.
  const uint32_t s = blockIdx.x / a.bps, i = (blockIdx.x - s * a.bps) * kBlock + threadIdx.x;
  const bool active = i < a.n;
  const uint32_t p = s * a.n + i;
  uint8_t m = 0;
  if (active) {
    const int ti = a.uniform ? 0 : (int)s;
    const double alpha = a.alpha_s[ti], eps = a.eps_s[ti];
    double* base = a.model + (size_t)s * kLbSomPlanes * a.n;
    const uint32_t off = i * 8u;  // n < 2^29 (engine_lb.h): the byte offset inside a plane fits 32 bits
    const uint8_t* px = a.cur + (size_t)p * 3;
    const double src[3] = {(double)px[0], (double)px[1], (double)px[2]};
    double som[9][3], hitc[3];
    uint32_t touched;
    lb_som_load(a, base, off, src, som, touched);
    const bool isbg = lb_som_pixel<FUZZY>(alpha, eps, src, som, touched, hitc);
    lb_som_put(a, base, off, som, touched);
    uint8_t* keep = a.bgplane + (size_t)p * 3;
    uint8_t out[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = isbg ? (uint8_t)(int)hitc[c] : (a.init ? (uint8_t)0 : keep[c]);
    if (isbg || a.init) {
#pragma unroll
      for (int c = 0; c < 3; ++c) keep[c] = out[c];
    }
    if (a.bg) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.bg[(size_t)p * 3 + c] = out[c];
    }
    m = isbg ? 0 : 255;
  }
  lb_write_mask(a, p, active, m);
}

// T frames in one launch, frame t with (alpha_t[t], eps_t[t]): the 27 doubles are read once and the neurons that any of the T
// frames' windows covered are written once; the kept background bytes are read once and written once if any frame was background.
// The frame loop is not unrolled (eight copies of the nine-neuron update, with the fuzzy model's exp() in each, take the compiler
// minutes): the T frames' bytes wait in three 64-bit registers, byte t of pk[ch] = channel ch of frame t, and leave by a shift.
template <bool FUZZY, int T>
__global__ __launch_bounds__(kBlock) void lb_som_clip_kernel(const LbClipArgs c) {
  static_assert(T <= 8, "one byte per frame in a 64-bit word");
  const LbArgs& a = c.a;
  const uint32_t s = blockIdx.x / a.bps, i = (blockIdx.x - s * a.bps) * kBlock + threadIdx.x;
  const bool active = i < a.n;
  const uint32_t p = s * a.n + i;
  uint32_t ms = 0;  // bit t: frame t's pixel is foreground
  if (active) {
    double* base = a.model + (size_t)s * kLbSomPlanes * a.n;
    const uint32_t off = i * 8u;
    uint64_t pk[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const uint8_t* px = a.cur + t * c.frame_stride + (size_t)p * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) pk[ch] |= (uint64_t)px[ch] << (8 * t);
    }
    uint8_t* keep = a.bgplane + (size_t)p * 3;
    uint8_t kept[3] = {0, 0, 0};
    bool kept_new = a.init;
    if (!a.init) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) kept[ch] = keep[ch];
    }
    double som[9][3], hitc[3];
    uint32_t touched;
    {
      const double src[3] = {(double)(uint32_t)(pk[0] & 255u), (double)(uint32_t)(pk[1] & 255u), (double)(uint32_t)(pk[2] & 255u)};
      lb_som_load(a, base, off, src, som, touched);
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const double src[3] = {(double)(uint32_t)((pk[0] >> (8 * t)) & 255u), (double)(uint32_t)((pk[1] >> (8 * t)) & 255u), (double)(uint32_t)((pk[2] >> (8 * t)) & 255u)};
      const bool isbg = lb_som_pixel<FUZZY>(c.alpha_t[t], c.eps_t[t], src, som, touched, hitc);
      if (isbg) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) kept[ch] = (uint8_t)(int)hitc[ch];
        kept_new = true;
      } else {
        ms |= 1u << t;
      }
      if (a.bg) {
        uint8_t* o = a.bg + t * c.frame_stride + (size_t)p * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch] = kept[ch];
      }
    }
    lb_som_put(a, base, off, som, touched);
    if (kept_new) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) keep[ch] = kept[ch];
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) lb_write_mask(c, t, p, active, (ms >> t) & 1u ? 255 : 0);
}

}  // namespace bgs
