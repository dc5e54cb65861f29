// kernel_dp2.h — the two package_bgs/dp classes with a neighbourhood step, on gfx950:
//   DPPratiMediodBGS (BGS_DP_PRATI_MEDIOD, USTC_BGS type 14): temporal medoid of a circular buffer of sampled frames, low / high
//                    thresholds and a hysteresis over the 8 neighbours (dp/PratiMediodBGS.cpp, dp/DPPratiMediodBGS.cpp:29-81);
//   DPTextureBGS     (BGS_DP_TEXTURE, USTC_BGS type 16): 6-point LBP codes, an 11x11 histogram of 3 x 64 bins per pixel and
//                    histogram intersection against the model (dp/TextureBGS.cpp, dp/DPTextureBGS.cpp:39-134).
// Everything is integer arithmetic; the masks and the model planes equal the reference's bit for bit.
//
// Model layout, stream-major so that a run of streams [first, first+count) is one contiguous slab of each plane:
//   PratiMediod  samples  uint32 [S][H][n]   b | g << 8 | r << 16 per (slot, pixel); one coalesced 256-byte load per wave
//                dist     uint16 [S][H][n]   the slot's sum of L-inf distances (<= H * 255 <= 16320 for H <= 64: DESIGN.md §5.4)
//                median   uint32 [2][S][n]   ping-pong: a sampled frame reads plane `par` for its mask and writes plane par ^ 1
//   Texture      hist_r   uint32 [S][16][n]  the r histogram, 4 bins per dword (bin b in byte b & 3 of dword b >> 2)
//                hist_gb  uint32 [S][32][n]  g (dwords 0..15) and b (16..31): fixed after the first frame (UpdateModel only
//                                            touches r)
//                mask     uint8  [S][n]      this frame's mask: the next launch's transposed update gate reads it
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgs_device.h"

namespace bgs {

constexpr int kPratiMaxHistory = 64;  // BGS_PRATI_MAX_HISTORY

// L-inf distance of two packed b | g << 8 | r << 16 pixels
__device__ __forceinline__ uint32_t linf3(uint32_t a, uint32_t b) {
  const int d0 = abs(byte_of(a, 0) - byte_of(b, 0)), d1 = abs(byte_of(a, 1) - byte_of(b, 1)), d2 = abs(byte_of(a, 2) - byte_of(b, 2));
  return (uint32_t)max(d0, max(d1, d2));
}

__device__ __forceinline__ uint32_t load_px3(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }

struct PratiArgs {
  const uint8_t* cur;     // [npix][3] frames of the run's streams
  uint8_t* fg;            // [npix] byte masks (nullable)
  uint64_t* fg_bits;      // packed masks (nullable; npix % 64 == 0 then)
  uint32_t* samples;      // the run's first stream: [count][H][n]
  uint16_t* dist;         // [count][H][n]
  const uint32_t* med_in; // [count][n] plane `par`: the medoid of the last sampled frame (read by the masks)
  uint32_t* med_out;      // [count][n] plane par ^ 1: written by a sampled frame
  uint32_t npix, n;
  int rows, cols;
  int H;                  // HistorySize
  int cnt, pos;           // samples in the buffer before this frame, the slot a full buffer replaces (the same for every pixel)
  int sample;             // frame_num % SamplingRate == 0: Update runs
  int masks;              // frame_num >= HistorySize: Subtract computes masks (all zero before)
  int low, high;          // LowThreshold / HighThreshold clamped to 255 (the L-inf distance is a byte)
};

// One frame of DPPratiMediodBGS::process per pixel: Subtract (CalculateMasks + Combine with the pre-update medoids of the 3x3
// neighbourhood), then Update (PratiMediodBGS.cpp:70-140) of the pixel's own buffer.  Neighbours' medoids are read from med_in and
// the new medoid goes to med_out, so no workgroup reads a medoid that another one has already rewritten in this launch.
__global__ __launch_bounds__(kBlock) void prati_kernel(const PratiArgs a) {
  const uint32_t p = (uint32_t)(blockIdx.x * kBlock + threadIdx.x);
  const bool active = p < a.npix;
  uint8_t m = 0;
  if (active) {
    const uint32_t s = p / a.n, i = p - s * a.n;
    const int y = (int)(i / (uint32_t)a.cols), x = (int)(i - (uint32_t)y * (uint32_t)a.cols);
    const uint32_t me = load_px3(a.cur + (size_t)p * 3);
    if (a.masks && y > 0 && x > 0 && y < a.rows - 1 && x < a.cols - 1) {  // Combine: the one-pixel border stays BACKGROUND
      const uint32_t dme = linf3(me, a.med_in[p]);
      if ((int)dme > a.high) {
        m = 255;
      } else if ((int)dme > a.low) {  // low only: foreground if 8-connected to a high pixel
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const uint32_t q = p + (uint32_t)(dy * a.cols + dx);
            if ((int)linf3(load_px3(a.cur + (size_t)q * 3), a.med_in[q]) > a.high) m = 255;
          }
      }
    }
    if (a.fg) a.fg[p] = m;
    if (a.sample) {
      // Update: a full buffer first takes L-inf(old, s) off every sum, then UpdateMediod adds L-inf(s, new) to every slot - the
      // slot being replaced included, still holding the old pixel - and picks the first strict minimum in slot order; the new
      // pixel wins only if its own sum is strictly smaller.  Then the slot takes the new pixel and that full sum.
      uint32_t* smp = a.samples + (size_t)s * a.H * a.n + i;
      uint16_t* dst = a.dist + (size_t)s * a.H * a.n + i;
      const bool full = a.cnt == a.H;
      const uint32_t old = full ? smp[(size_t)a.pos * a.n] : 0u;
      uint32_t best = 0xffffffffu, med = 0, L = 0;
      for (int k = 0; k < a.cnt; ++k) {
        const uint32_t sv = smp[(size_t)k * a.n];
        uint32_t dv = dst[(size_t)k * a.n];
        if (full) dv -= linf3(old, sv);
        const uint32_t d = linf3(sv, me);
        dv += d, L += d;
        if (dv < best) best = dv, med = sv;
        dst[(size_t)k * a.n] = (uint16_t)dv;
      }
      if (L < best) med = me;
      const int slot = full ? a.pos : a.cnt;
      dst[(size_t)slot * a.n] = (uint16_t)L;
      smp[(size_t)slot * a.n] = me;
      a.med_out[p] = med;
    }
  }
  if (a.fg_bits) {  // npix % 64 == 0 is checked on the host: a wave is either all active or all idle
    const unsigned long long w = __ballot(active && m != 0);
    if ((threadIdx.x & (kWave - 1)) == 0 && active) a.fg_bits[p >> 6] = w;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Texture.  One workgroup per 64 x 4 tile of one stream's image (a wave is one 64-pixel row segment, so every model plane access is
// one coalesced 256-byte load).  The tile's frame (+7 halo) goes to LDS, then its LBP codes (+5 halo), then every lane counts its
// 11x11 window into a private column of byte-packed bins, laid out [dword][lane] so that a wave's 64 increments hit 64 distinct
// banks whatever the codes.
constexpr int kTexTW = 64, kTexTH = 4;                   // output tile
constexpr int kTexFW = kTexTW + 14, kTexFH = kTexTH + 14;  // frame tile: REGION_R + TEXTURE_R = 7 on each side
constexpr int kTexCW = kTexTW + 10, kTexCH = kTexTH + 10;  // code tile: REGION_R = 5 on each side
constexpr int kTexInterior = 7;                           // only 7 <= x < W-7, 7 <= y < H-7 are processed
static_assert(kTexTW * kTexTH == kBlock, "one lane per output pixel");

struct TexArgs {
  const uint8_t* cur;      // [count][n][3]
  uint8_t* fg;             // [count][n] caller's byte masks (nullable)
  uint8_t* mask;           // [count][n] the engine's mask plane
  uint32_t* hist_r;        // [count][16][n]
  uint32_t* hist_gb;       // [count][32][n]
  uint32_t n;
  int rows, cols;
  int ws;                  // widthStep of the reference's 1-channel mask image: (cols + 3) & ~3
  int tiles_x, tiles_per_img;
  int init;                // first frame: the model becomes this frame's histograms
};

// DPTextureBGS's r update, (unsigned char)(ALPHA*cur + (1-ALPHA)*bg + 0.5) in double with ALPHA = 0.05f widened: every term is
// exact in double (ALPHA = 13421773 / 2^28), so it equals bg + floor((13421773 (cur - bg) + 2^27) / 2^28) - checked for every
// (cur, bg) pair against the double expression in tests/test_dp2_cpu.py.
__device__ __forceinline__ uint32_t tex_update_byte(int bg, int cur) {
  const long long d = (long long)(cur - bg) * 13421773LL + (1LL << 27);
  return (uint32_t)(bg + (int)(d >> 28));  // arithmetic shift = floor
}

// The frame tile and then the code tile of the channels [CH0, 3) (the update pass only needs r, channel 2).  Returns with the
// codes in `codes` ([3][kTexCH][kTexCW]); `frame` may be reused once this returns.
template <int CH0>
__device__ __forceinline__ void tex_codes(const TexArgs& a, const uint8_t* img, int ty0, int tx0, uint8_t* frame, uint8_t* codes) {
  const int tid = threadIdx.x;
  for (int k = tid; k < kTexFH * kTexFW; k += kBlock) {
    const int r = k / kTexFW, c = k - r * kTexFW, y = ty0 - 7 + r, x = tx0 - 7 + c;
    const bool in = y >= 0 && x >= 0 && y < a.rows && x < a.cols;
    const uint8_t* px = img + ((size_t)(in ? y : 0) * a.cols + (in ? x : 0)) * 3;
#pragma unroll
    for (int ch = CH0; ch < 3; ++ch) frame[(ch * kTexFH + r) * kTexFW + c] = in ? px[ch] : 0;
  }
  __syncthreads();
  // LBP (TextureBGS.cpp:20-47): code at frame-tile (r+2, c+2); positions nearer than 2 to the image border hold codes of the
  // zero fill, which no processed pixel's window reaches
  for (int k = tid; k < kTexCH * kTexCW; k += kBlock) {
    const int r = k / kTexCW, c = k - r * kTexCW;
#pragma unroll
    for (int ch = CH0; ch < 3; ++ch) {
      const uint8_t* f = frame + (ch * kTexFH + r + 2) * kTexFW + c + 2;
      const int v = f[0] + 3;  // + HYSTERSIS
      const int code = (v >= f[-2 * kTexFW]) | (v >= f[-kTexFW - 2]) << 1 | (v >= f[-kTexFW + 2]) << 2 | (v >= f[kTexFW - 2]) << 3 |
                       (v >= f[kTexFW + 2]) << 4 | (v >= f[2 * kTexFW]) << 5;
      codes[(ch * kTexCH + r) * kTexCW + c] = (uint8_t)code;
    }
  }
  __syncthreads();
}

// Count the 11x11 window of lane (ly, lx) into hist[d * kBlock + lane], dwords [16 * h0, 48) of histogram order r, g, b
// (r = code channel 2, g = 1, b = 0).  The lane owns its column: the no-return LDS add needs no atomicity, only one instruction.
template <int CH0>
__device__ __forceinline__ void tex_count(const uint8_t* codes, uint32_t* hist, int ly, int lx) {
  const int tid = threadIdx.x;
  for (int j = 0; j < 11; ++j)
    for (int i = 0; i < 11; ++i) {
#pragma unroll
      for (int ch = CH0; ch < 3; ++ch) {
        const int code = codes[(ch * kTexCH + ly + j) * kTexCW + lx + i];
        const int h = 2 - ch;
        atomicAdd(&hist[(h * 16 + (code >> 2)) * kBlock + tid], 1u << (8 * (code & 3)));
      }
    }
}

// Pass 1: LBP, histograms, BgsCompare (proximity = sum of min over 192 bins, foreground if < 181.5), the mask; on the first frame
// also the model itself.  sum min(bg, cur) = (sum bg + sum cur - sum |bg - cur|) / 2 with sum cur = 3 * 121 in the interior, so
// foreground <=> sum bg + 363 - SAD(bg, cur) < 363, with v_sad_u8 covering 4 bins per instruction.
__global__ __launch_bounds__(kBlock) void tex_compare_kernel(const TexArgs a) {
  __shared__ uint32_t hist[48 * kBlock];                 // 48 KiB; the frame tile lives in it until the codes are made
  __shared__ uint8_t codes[3 * kTexCH * kTexCW];
  static_assert(3 * kTexFH * kTexFW <= (int)sizeof(hist), "frame tile fits in the histogram space");
  const int tid = threadIdx.x;
  const int s = blockIdx.x / a.tiles_per_img, t = blockIdx.x - s * a.tiles_per_img;
  const int ty0 = (t / a.tiles_x) * kTexTH, tx0 = (t % a.tiles_x) * kTexTW;
  const int ly = tid / kTexTW, lx = tid % kTexTW, y = ty0 + ly, x = tx0 + lx;
  const uint8_t* img = a.cur + (size_t)s * a.n * 3;
  tex_codes<0>(a, img, ty0, tx0, (uint8_t*)hist, codes);
#pragma unroll
  for (int d = 0; d < 48; ++d) hist[d * kBlock + tid] = 0;
  const bool in = y < a.rows && x < a.cols;
  const bool interior = y >= kTexInterior && x >= kTexInterior && y < a.rows - kTexInterior && x < a.cols - kTexInterior;
  if (interior) tex_count<0>(codes, hist, ly, lx);
  if (!in) return;
  const size_t i = (size_t)y * a.cols + x, p = (size_t)s * a.n + i;
  uint8_t m = 0;
  if (interior) {
    uint32_t* hr = a.hist_r + (size_t)s * 16 * a.n + i;
    uint32_t* hgb = a.hist_gb + (size_t)s * 32 * a.n + i;
    if (a.init) {  // bgModel = curTextureHist (DPTextureBGS.cpp:79-93); proximity 363 then: background
#pragma unroll
      for (int d = 0; d < 16; ++d) hr[(size_t)d * a.n] = hist[d * kBlock + tid];
#pragma unroll
      for (int d = 0; d < 32; ++d) hgb[(size_t)d * a.n] = hist[(16 + d) * kBlock + tid];
    } else {
      uint32_t sad = 0, sbg = 0;
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        const uint32_t bg = hr[(size_t)d * a.n];
        sad = __builtin_amdgcn_sad_u8(bg, hist[d * kBlock + tid], sad), sbg = __builtin_amdgcn_sad_u8(bg, 0u, sbg);
      }
#pragma unroll
      for (int d = 0; d < 32; ++d) {
        const uint32_t bg = hgb[(size_t)d * a.n];
        sad = __builtin_amdgcn_sad_u8(bg, hist[(16 + d) * kBlock + tid], sad), sbg = __builtin_amdgcn_sad_u8(bg, 0u, sbg);
      }
      m = sbg < sad ? 255 : 0;  // 2 * proximity = sbg + 363 - sad < 363
    }
  }
  a.mask[p] = m;
  if (a.fg) a.fg[p] = m;
}

// Pass 2 (every frame but the first): UpdateModel (TextureBGS.cpp:108-127) gated by fgMask(x, y) - row x, column y of the mask
// image, i.e. flat byte x * widthStep + y of it.  A byte past the image or in a row's padding reads as 0, so the model updates
// there.  Only the r histogram is updated.  The gate is written by other workgroups of pass 1: hence two launches.
__global__ __launch_bounds__(kBlock) void tex_update_kernel(const TexArgs a) {
  __shared__ uint32_t hist[16 * kBlock];
  __shared__ uint8_t codes[3 * kTexCH * kTexCW];
  __shared__ uint8_t frame[3 * kTexFH * kTexFW];
  const int tid = threadIdx.x;
  const int s = blockIdx.x / a.tiles_per_img, t = blockIdx.x - s * a.tiles_per_img;
  const int ty0 = (t / a.tiles_x) * kTexTH, tx0 = (t % a.tiles_x) * kTexTW;
  const int ly = tid / kTexTW, lx = tid % kTexTW, y = ty0 + ly, x = tx0 + lx;
  const uint8_t* img = a.cur + (size_t)s * a.n * 3;
  tex_codes<2>(a, img, ty0, tx0, frame, codes);
  const bool interior = y >= kTexInterior && x >= kTexInterior && y < a.rows - kTexInterior && x < a.cols - kTexInterior;
  bool upd = false;
  if (interior) {
    const size_t flat = (size_t)x * a.ws + y, gr = flat / a.ws, gc = flat - gr * a.ws;
    upd = !(gr < (size_t)a.rows && gc < (size_t)a.cols) || a.mask[(size_t)s * a.n + gr * a.cols + gc] == 0;
  }
  if (!upd) return;  // no barrier follows
#pragma unroll
  for (int d = 0; d < 16; ++d) hist[d * kBlock + tid] = 0;
  tex_count<2>(codes, hist, ly, lx);
  uint32_t* hr = a.hist_r + (size_t)s * 16 * a.n + (size_t)y * a.cols + x;
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    const uint32_t bg = hr[(size_t)d * a.n], cur = hist[d * kBlock + tid];
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) out |= tex_update_byte(byte_of(bg, k), byte_of(cur, k)) << (8 * k);
    hr[(size_t)d * a.n] = out;
  }
}

}  // namespace bgs
