// kernel_fuzzy.h — package_bgs/tb FuzzySugenoIntegral / FuzzyChoquetIntegral (BGS_FUZZY_SUGENO / BGS_FUZZY_CHOQUET, USTC_BGS types 21
// and 22) on gfx950, the RGB path (colorSpace 1): Fuzzy*Integral.cpp:31-173 over FuzzyUtils.cpp / PixelUtils.cpp.
//
// State: the float BGR background, [stream][pixel][3], 12 B/pixel.  Everything else is per-frame scratch.
//
// A detecting frame is NOT a per-pixel function of its inputs: the reference sets Indice = (0,1,2) once per frame and Trier permutes
// it further at every pixel, columns outer, rows inner.  Pixel q = x*H + y contributes a permutation pi_q in S3 that depends on its own
// three similarities only, the state after it is sigma_q = pi_0 o ... o pi_q, (A o B)[k] = A[B[k]], and the integral indexes the
// pixel's ALREADY SORTED values by sigma_q.  The kernels compute sigma as a prefix product in logarithmic depth:
//
//   fuzzy_prep_kernel    streams x pixels, row-major.  Learning streams: bg = in (first frame) or in*a + bg*b.  Detecting streams:
//                        float gray of input and background into two planes.
//   fuzzy_pixel_kernel   16x16 tiles.  LBP of both gray planes (256-entry table, the column/row quirk of getNeighberhoodGrayPixel),
//                        the similarities, Trier.  Writes the sorted values hs[3] and the 6-bit code of pi in COLUMN-MAJOR order
//                        (index q): the tile is turned through LDS, so reads run along x and writes along y, both in 64-byte runs.
//   fuzzy_scan_block_kernel   product of each run of kFzScan = 1024 consecutive codes (4 per lane, ordered wave and block reduction).
//   fuzzy_scan_top_kernel     exclusive prefix of the block products of a stream: one 1024-lane block, Hillis-Steele in the wave,
//                        wave totals through LDS; frames past 2^20 pixels take one more trip per 2^20.
//   fuzzy_apply_kernel   the prefix inside each run of 1024 (same partition), sigma_q, the integral; writes the integral plane, still
//                        column-major (contiguous).
//   fuzzy_median_kernel  16x16 tiles + halo read along y from the column-major plane into LDS, 3x3 median (replicated borders, from
//                        the unblurred plane), written row-major with the mask; per-stream min / max by one atomic pair per block
//                        on an order-preserving integer image of the float (NaN takes no part, as it loses every < and >).
//   fuzzy_update_kernel  streams x pixels, row-major: the background bytes (before the update), then
//                        AdaptativeSelectiveBackgroundModelUpdate with the stream's min / max.
//
// Arithmetic: every operation is a single correctly rounded f32 operation in the reference's order (the library is built with
// -ffp-contract=off, IEEE division, denormals kept).  No libm.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgs_device.h"

namespace bgs {

constexpr int kFzStreams = 64;   // streams one launch covers: one bit each in learn_mask / init_mask
constexpr int kFzTile = 16;      // pixel / median kernels: 16 x 16 pixels per block
constexpr int kFzPerLane = 4;    // scan kernels: codes per lane
constexpr int kFzScan = kBlock * kFzPerLane;  // codes per scan block
constexpr int kFzTop = 1024;     // lanes of the top-level scan block
constexpr uint32_t kFzIdentity = 0x24;  // (0,1,2): entry k in bits 2k, 2k+1

struct FzArgs {
  const uint8_t* cur;    // [count][n][3] frames of the launch's streams (BGR)
  uint8_t* fg;           // [count][n] mask (nullable)
  uint8_t* bgout;        // [count][n][3] background image (nullable)
  float* bg;             // [count][n][3] state
  float* gray_in;        // [count][n]
  float* gray_bg;        // [count][n]
  float* hs;             // [3][plane] sorted similarities, column-major inside a stream
  uint8_t* code;         // [count][n] pi codes, column-major
  float* iq;             // [count][n] integral, column-major
  float* I;              // [count][n] blurred integral, row-major
  uint8_t* bprod;        // [count][nb] block products, then (in place) their exclusive prefix
  uint32_t* minmax;      // [count][2] order-preserving images of min and max
  const float* tab;      // 256 interior LBP values + 8 corner values
  size_t plane;          // floats between hs planes
  uint32_t n, nb;
  int W, H;
  uint64_t learn_mask;   // bit k: stream k of the launch learns this frame
  uint64_t init_mask;    // bit k: stream k is on its first frame (background = input)
  float a_learn, b_learn;  // (float)alphaLearn, (float)(1 - alphaLearn)
  float a_update, thr;     // (float)alphaUpdate, (float)threshold
  float G[3];
  int choquet, colours, smooth;  // colours: HI = the three colour similarities (Choquet, option 1)
};

__device__ __forceinline__ uint32_t fz_compose(uint32_t A, uint32_t B) {  // (A o B)[k] = A[B[k]]
  return ((A >> (2 * (B & 3))) & 3) | (((A >> (2 * ((B >> 2) & 3))) & 3) << 2) | (((A >> (2 * ((B >> 4) & 3))) & 3) << 4);
}
__device__ __forceinline__ uint32_t fz_key(float v) {  // monotone: a < b  <=>  key(a) < key(b) (no NaN)
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float fz_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
__device__ __forceinline__ float fz_in(uint8_t b) { return (float)b * (float)(1. / 255.); }  // convertTo(CV_32F, 1./255.)
__device__ __forceinline__ float fz_gray(float b, float g, float r) { return (b * 0.114f + g * 0.587f) + r * 0.299f; }
// RatioPixels.  An unordered pair (NaN background): the reference writes nothing and reads uninitialised heap; NaN here
__device__ __forceinline__ float fz_ratio(float c, float b) { return c < b ? c / b : c > b ? b / c : c == b ? 1.0f : __uint_as_float(0x7fc00000u); }

// FuzzyUtils::LBP at (x, y) of a W x H gray plane
__device__ __forceinline__ float fz_lbp(const float* g, int x, int y, int W, int H, const float* tab) {
  if (x == 0 && y == 0) {
    const float c = g[0];
    const int k = (g[W] >= c ? 1 : 0) + (g[1] >= c ? 2 : 0) + (g[W + 1] >= c ? 4 : 0);
    return tab[256 + k];
  }
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return 0.0f;
  float s[9];
  if (H >= W + 2 && y == W) {  // `last column` branch: six slots refilled, slots 6..8 stale from pixel (W-2, W-1): column W-3, rows W-2..W
    s[0] = g[(y - 1) * W + x + 1], s[1] = g[y * W + x + 1], s[2] = g[(y - 1) * W + x], s[3] = g[y * W + x];
    s[4] = g[(y - 1) * W + x - 1], s[5] = g[y * W + x - 1];
    s[6] = g[(W - 2) * W + W - 3], s[7] = g[(W - 1) * W + W - 3], s[8] = g[W * W + W - 3];
  } else {
    if (W >= H + 2 && x == H) x = H - 1;  // `last line` branch: the three stale slots make it the neighbourhood of column H-1
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) s[3 * a + b] = g[(y - 1 + b) * W + x + 1 - a];
  }
  int code = 0;
#pragma unroll
  for (int l = 0; l < 9; ++l)
    if (l != 4) code |= (s[l] >= s[4] ? 1 : 0) << (l < 4 ? l : l - 1);
  return tab[code];
}

__global__ __launch_bounds__(kBlock) void fuzzy_prep_kernel(const FzArgs a, uint32_t npix) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const uint32_t s = p / a.n;
  const uint8_t* px = a.cur + (size_t)p * 3;
  float* bg = a.bg + (size_t)p * 3;
  const float i0 = fz_in(px[0]), i1 = fz_in(px[1]), i2 = fz_in(px[2]);
  if ((a.learn_mask >> s) & 1) {
    if ((a.init_mask >> s) & 1) {
      bg[0] = i0, bg[1] = i1, bg[2] = i2;
    } else {  // addWeighted on 32F: in*a + bg*b + 0
      bg[0] = (i0 * a.a_learn + bg[0] * a.b_learn) + 0.0f;
      bg[1] = (i1 * a.a_learn + bg[1] * a.b_learn) + 0.0f;
      bg[2] = (i2 * a.a_learn + bg[2] * a.b_learn) + 0.0f;
    }
    return;
  }
  a.gray_in[p] = fz_gray(i0, i1, i2);
  a.gray_bg[p] = fz_gray(bg[0], bg[1], bg[2]);
  if (p - s * a.n == 0) a.minmax[2 * s] = fz_key(255.0f), a.minmax[2 * s + 1] = fz_key(0.0f);  // Minimum = 255, Maximum = 0
}

__global__ __launch_bounds__(kFzTile* kFzTile) void fuzzy_pixel_kernel(const FzArgs a) {
  const uint32_t s = blockIdx.z;
  if ((a.learn_mask >> s) & 1) return;
  __shared__ float l_hs[3][kFzTile][kFzTile + 1];
  __shared__ uint8_t l_code[kFzTile][kFzTile + 1];
  const int tx = threadIdx.x, ty = threadIdx.y, W = a.W, H = a.H;
  const int x0 = blockIdx.x * kFzTile, y0 = blockIdx.y * kFzTile;
  const int x = x0 + tx, y = y0 + ty;
  const size_t so = (size_t)s * a.n;
  if (x < W && y < H) {
    const size_t p = so + (size_t)y * W + x;
    const uint8_t* px = a.cur + p * 3;
    const float* bg = a.bg + p * 3;
    const float c0 = fz_ratio(fz_in(px[0]), bg[0]), c1 = fz_ratio(fz_in(px[1]), bg[1]);
    float h0, h1, h2;
    if (a.colours) {
      h0 = c0, h1 = c1, h2 = fz_ratio(fz_in(px[2]), bg[2]);
    } else {
      h0 = fz_ratio(fz_lbp(a.gray_in + so, x, y, W, H, a.tab), fz_lbp(a.gray_bg + so, x, y, W, H, a.tab)), h1 = c0, h2 = c1;
    }
    // Trier: three compare-exchanges, strict <, the same swaps on the index triple
    uint32_t p0 = 0, p1 = 1, p2 = 2, t;
    float f;
    if (h1 < h2) f = h1, h1 = h2, h2 = f, t = p1, p1 = p2, p2 = t;
    if (h0 < h1) f = h0, h0 = h1, h1 = f, t = p0, p0 = p1, p1 = t;
    if (h1 < h2) f = h1, h1 = h2, h2 = f, t = p1, p1 = p2, p2 = t;
    l_hs[0][ty][tx] = h0, l_hs[1][ty][tx] = h1, l_hs[2][ty][tx] = h2;
    l_code[ty][tx] = (uint8_t)(p0 | p1 << 2 | p2 << 4);
  }
  __syncthreads();
  const int ox = x0 + ty, oy = y0 + tx;  // the lanes of a row now run along y
  if (ox < W && oy < H) {
    const size_t q = so + (size_t)ox * H + oy;
    a.hs[q] = l_hs[0][tx][ty], a.hs[a.plane + q] = l_hs[1][tx][ty], a.hs[2 * a.plane + q] = l_hs[2][tx][ty];
    a.code[q] = l_code[tx][ty];
  }
}

// the lane's kFzPerLane codes of scan block `blk` of a stream (identity past the stream's end), and their product
__device__ __forceinline__ uint32_t fz_load_codes(const uint8_t* code, uint32_t n, uint32_t blk, uint32_t (&c)[kFzPerLane]) {
  const uint32_t q0 = blk * kFzScan + threadIdx.x * kFzPerLane;
  uint32_t v = kFzIdentity;
#pragma unroll
  for (int j = 0; j < kFzPerLane; ++j) {
    c[j] = q0 + j < n ? (uint32_t)code[q0 + j] : kFzIdentity;
    v = fz_compose(v, c[j]);
  }
  return v;
}
// inclusive prefix over the wave, lane order
__device__ __forceinline__ uint32_t fz_wave_scan(uint32_t v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t t = __shfl_up(v, off, kWave);
    if (lane >= off) v = fz_compose(t, v);
  }
  return v;
}

__global__ __launch_bounds__(kBlock) void fuzzy_scan_block_kernel(const FzArgs a) {
  const uint32_t s = blockIdx.y;
  if ((a.learn_mask >> s) & 1) return;
  __shared__ uint32_t tot[kBlock / kWave];
  uint32_t c[kFzPerLane];
  const uint32_t v = fz_wave_scan(fz_load_codes(a.code + (size_t)s * a.n, a.n, blockIdx.x, c));
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) tot[threadIdx.x / kWave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = tot[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) r = fz_compose(r, tot[w]);
    a.bprod[(size_t)s * a.nb + blockIdx.x] = (uint8_t)r;
  }
}

__global__ __launch_bounds__(kFzTop) void fuzzy_scan_top_kernel(const FzArgs a) {
  const uint32_t s = blockIdx.x;
  if ((a.learn_mask >> s) & 1) return;
  __shared__ uint32_t tot[kFzTop / kWave];
  __shared__ uint32_t carry_s;
  uint8_t* bp = a.bprod + (size_t)s * a.nb;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint32_t carry = kFzIdentity;
  for (uint32_t base = 0; base < a.nb; base += kFzTop) {  // one trip per 2^20 pixels
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = fz_wave_scan(i < a.nb ? (uint32_t)bp[i] : kFzIdentity);
    if (lane == kWave - 1) tot[wave] = v;
    __syncthreads();
    uint32_t pre = carry;
    for (int w = 0; w < wave; ++w) pre = fz_compose(pre, tot[w]);  // at most 15
    const uint32_t up = __shfl_up(v, 1, kWave);
    if (i < a.nb) bp[i] = (uint8_t)(lane ? fz_compose(pre, up) : pre);  // exclusive
    if (threadIdx.x == kFzTop - 1) carry_s = fz_compose(pre, v);
    __syncthreads();
    carry = carry_s;
  }
}

__global__ __launch_bounds__(kBlock) void fuzzy_apply_kernel(const FzArgs a) {
  const uint32_t s = blockIdx.y;
  if ((a.learn_mask >> s) & 1) return;
  __shared__ uint32_t tot[kBlock / kWave];
  const size_t so = (size_t)s * a.n;
  uint32_t c[kFzPerLane];
  const uint32_t v = fz_wave_scan(fz_load_codes(a.code + so, a.n, blockIdx.x, c));
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == kWave - 1) tot[wave] = v;
  __syncthreads();
  uint32_t sg = (uint32_t)a.bprod[(size_t)s * a.nb + blockIdx.x];  // everything before this block
  for (int w = 0; w < wave; ++w) sg = fz_compose(sg, tot[w]);
  const uint32_t up = __shfl_up(v, 1, kWave);
  if (lane) sg = fz_compose(sg, up);
  const uint32_t q0 = blockIdx.x * kFzScan + threadIdx.x * kFzPerLane;
#pragma unroll
  for (int j = 0; j < kFzPerLane; ++j) {
    const uint32_t q = q0 + j;
    if (q >= a.n) break;
    sg = fz_compose(sg, c[j]);  // sigma_q
    const float hs[3] = {a.hs[so + q], a.hs[a.plane + so + q], a.hs[2 * a.plane + so + q]};
    const uint32_t k0 = sg & 3, k1 = (sg >> 2) & 3, k2 = (sg >> 4) & 3;
    const float v0 = hs[k0], v1 = hs[k1], v2 = hs[k2], g2 = a.G[k2];
    const float xx = a.G[k1] + g2;  // XiXj
    float r;
    if (a.choquet) {
      r = (v0 * (1.0f - xx) + v1 * (xx - g2)) + v2 * g2;
    } else {  // FuzzyUtils::min: a >= b ? b : a;  FuzzyUtils::max: from 0, >=
      const float m0 = v0 >= 1.0f ? 1.0f : v0, m1 = v1 >= xx ? xx : v1, m2 = v2 >= g2 ? g2 : v2;
      r = 0.0f;
      if (m0 >= r) r = m0;
      if (m1 >= r) r = m1;
      if (m2 >= r) r = m2;
    }
    a.iq[so + q] = r;
  }
}

__device__ __forceinline__ void fz_mm(float& x, float& y) {  // OpenCV's float median exchange: std::min / std::max
  const float t = x;
  x = y < x ? y : x;
  y = t < y ? y : t;
}

__global__ __launch_bounds__(kFzTile* kFzTile) void fuzzy_median_kernel(const FzArgs a) {
  const uint32_t s = blockIdx.z;
  if ((a.learn_mask >> s) & 1) return;
  constexpr int T = kFzTile + 2;
  __shared__ float tile[T][T + 1];  // [column][row]
  __shared__ uint32_t red[2][kFzTile * kFzTile / kWave];
  const int tx = threadIdx.x, ty = threadIdx.y, W = a.W, H = a.H;
  const int x0 = blockIdx.x * kFzTile, y0 = blockIdx.y * kFzTile;
  const size_t so = (size_t)s * a.n;
  const int tid = ty * kFzTile + tx;
  for (int e = tid; e < T * T; e += kFzTile * kFzTile) {  // consecutive lanes read consecutive rows of one column: contiguous
    const int lx = e / T, ly = e - lx * T;
    const int xc = min(max(x0 - 1 + lx, 0), W - 1), yc = min(max(y0 - 1 + ly, 0), H - 1);
    tile[lx][ly] = a.iq[so + (size_t)xc * H + yc];
  }
  __syncthreads();
  const int x = x0 + tx, y = y0 + ty;
  const bool in = x < W && y < H;
  float v = tile[tx + 1][ty + 1];
  if (a.smooth) {
    float p[9];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) p[3 * dy + dx] = tile[tx + dx][ty + dy];
    fz_mm(p[1], p[2]), fz_mm(p[4], p[5]), fz_mm(p[7], p[8]), fz_mm(p[0], p[1]);
    fz_mm(p[3], p[4]), fz_mm(p[6], p[7]), fz_mm(p[1], p[2]), fz_mm(p[4], p[5]);
    fz_mm(p[7], p[8]), fz_mm(p[0], p[3]), fz_mm(p[5], p[8]), fz_mm(p[4], p[7]);
    fz_mm(p[3], p[6]), fz_mm(p[1], p[4]), fz_mm(p[2], p[5]), fz_mm(p[4], p[7]);
    fz_mm(p[4], p[2]), fz_mm(p[6], p[4]), fz_mm(p[4], p[2]);
    v = p[4];
  }
  uint32_t kmin = 0xffffffffu, kmax = 0u;
  if (in) {
    const size_t p = so + (size_t)y * W + x;
    a.I[p] = v;
    if (a.fg) a.fg[p] = v > a.thr ? 0 : 255;  // THRESH_BINARY_INV, then x255 saturated
    if (v == v) kmin = kmax = fz_key(v);
  }
#pragma unroll
  for (int off = kWave / 2; off; off >>= 1) {
    kmin = min(kmin, (uint32_t)__shfl_xor(kmin, off, kWave));
    kmax = max(kmax, (uint32_t)__shfl_xor(kmax, off, kWave));
  }
  if ((tid & (kWave - 1)) == 0) red[0][tid / kWave] = kmin, red[1][tid / kWave] = kmax;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kFzTile * kFzTile / kWave; ++w) kmin = min(kmin, red[0][w]), kmax = max(kmax, red[1][w]);
    atomicMin(a.minmax + 2 * s, kmin);
    atomicMax(a.minmax + 2 * s + 1, kmax);
  }
}

__global__ __launch_bounds__(kBlock) void fuzzy_update_kernel(const FzArgs a, uint32_t npix) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const uint32_t s = p / a.n;
  if ((a.learn_mask >> s) & 1) return;
  const float mn = fz_unkey(a.minmax[2 * s]), mx = fz_unkey(a.minmax[2 * s + 1]);
  const float I = a.I[p];
  // beta = 1 - (I - ((Min / (Min - Max)) * I - (Min * Max / (Min - Max))));  Min == Max: 0/0, NaN from here on, as in the reference
  const float d = mn - mx;
  const float beta = 1.0f - (I - ((mn / d) * I - ((mn * mx) / d)));
  const float ob = 1.0f - beta, oa = 1.0f - a.a_update;
  const uint8_t* px = a.cur + (size_t)p * 3;
  float* bg = a.bg + (size_t)p * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float b = bg[k];
    if (a.bgout) {  // convertTo(CV_8U, 255): the background BEFORE this frame's update; NaN -> 0
      const float u = b * 255.0f + 0.0f;
      a.bgout[(size_t)p * 3 + k] = u != u ? 0 : (uint8_t)sat_u8(u);
    }
    bg[k] = beta * b + ob * (a.a_update * fz_in(px[k]) + oa * b);
  }
}

}  // namespace bgs
