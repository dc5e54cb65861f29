// kernel_vumeter.h — package_bgs/av/VuMeter (BGS_VUMETER, USTC_BGS type 31) on gfx950: TBackgroundVuMeter::UpdateBackground
// (av/TBackgroundVuMeter.cpp:260-319) behind the wrapper's cvCvtColor(CV_RGB2GRAY), one fused launch per frame over streams x
// pixels, one pixel per lane.
//
// Model: per pixel a float histogram of binCount = 256 / binSize bins.  Every frame the reference scales ALL bins by alpha
// (cvConvertScale on 32F images: float working type, h = fl32(h * (float)alpha)), adds (float)(1.0 - alpha) to the bin of the
// frame's gray byte, masks the pixel when that bin (promoted to double) is below the double threshold, and replaces the background
// byte when its bin is below the frame's bin.  A bin index >= binCount maps to bin 0.  The multiply and the add are written with
// __fmul_rn / __fadd_rn (never contracted), and the library is built with f32 denormals kept: a bin runs through the denormal
// range on its way down, and - for alpha >= 0.5 - never leaves it: the smallest denormal times alpha rounds back to itself
// (DESIGN.md §5.6).
//
// Layout: planes [bin][stream][pixel] of f32, so a lane's neighbours in a plane are its neighbours in the image and a
// run of streams [first, first + count) is contiguous inside every plane; the background bytes [stream][pixel]; for the live-bin
// variants a u32 bitmap [stream][pixel] whose bit b says "bin b is not 0".
//
// Three variants, bit-identical in every output and in the dense form of the state (BGS_VU_SPARSE):
//   0 dense      every bin read, scaled, written: 8 binCount bytes per pixel.  The only path for binCount > 32.
//   1 live-bin   0 * alpha is exactly 0 and histograms start at 0, so a bin whose bit is clear is neither read nor written.  The bin
//                loop is wave-uniform: bin b is skipped when no lane of the wave has it live or hits it.  Otherwise the lanes that
//                have it live load it, and EVERY lane of the wave stores (the others store the 0 the plane holds by definition), so
//                each store instruction writes its 256-byte run whole.
//   2 live-bin, masked stores: as 1, but only the lanes that hold the bin store (partly written lines).
// A stream's first frame (init) reads nothing: the bitmap counts as 0 and the background is the frame's gray image.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgs_device.h"

namespace bgs {

constexpr int kVuTable = 64;      // streams one launch covers: one bit each in init_mask / quiet_mask
constexpr int kVuLiveMaxBins = 32;  // the bitmap is one u32 per pixel

struct VuArgs {
  const uint8_t* cur;   // [npix][3] frames of the launch's streams (BGR)
  uint8_t* fg;          // [npix] byte mask before the post-filter (nullable)
  uint64_t* fg_bits;    // packed mask (nullable; npix % 64 == 0 then, and no post-filter)
  uint8_t* bgout;       // [npix] background image out (nullable)
  float* hist;          // element (bin 0, first pixel of the launch); bin b is `plane` floats further
  uint8_t* bg;          // [npix] background bytes (state)
  uint32_t* live;       // [npix] live-bin bitmaps (variants 1, 2)
  size_t plane;         // floats per bin plane: streams of the engine x n
  uint32_t npix, n;
  int bin_size, bin_count;
  float alpha, inc;     // (float)alpha, (float)(1.0 - alpha)
  double threshold;
  uint64_t init_mask;   // bit k: stream k of the launch is on its first frame
  uint64_t quiet_mask;  // bit k: m_nCount < 5 for stream k after this frame: its mask is zero
};

// BINS = 32 (the default binSize 8): the bin loop is unrolled, the histogram sits in 32 registers, every load of the pixel is issued
// before the first is used and every store after the last was computed - without that the live-bin variants are latency-bound
// (one load -> multiply -> store round trip per live bin).  BINS = 0: any bin count, the plain loop.
template <int MODE, int BINS>
__global__ __launch_bounds__(kBlock) void vumeter_kernel(const VuArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool active = p < a.npix;
  const uint32_t q = active ? p : a.npix - 1;  // idle lanes of the last wave compute on a valid pixel and store nothing
  const uint32_t s = q / a.n;
  const bool init = (a.init_mask >> s) & 1, quiet = (a.quiet_mask >> s) & 1;
  const uint8_t* px = a.cur + (size_t)q * 3;
  const int g = gray_bgr(px[2], px[1], px[0]);  // CV_RGB2GRAY of a BGR pixel: byte 0 takes the R weight
  int i = g / a.bin_size;
  if (i >= a.bin_count) i = 0;
  int bgv = init ? g : (int)a.bg[q];
  int j = bgv / a.bin_size;
  if (j >= a.bin_count) j = 0;
  // element of bin b: workgroup-uniform base + the lane's small offset (scalar-base addressing)
  float* blk = a.hist + (size_t)blockIdx.x * kBlock;
  const uint32_t lq = q - blockIdx.x * kBlock;
  float hi = 0.0f, hj = 0.0f;
  uint32_t bits = 0;
  if constexpr (MODE != 0) bits = (init || !active) ? 0u : a.live[q];
  if constexpr (BINS != 0) {
    const uint32_t need = MODE == 0 ? ~0u : (active ? bits | (1u << i) : 0u);
    float h[BINS];
#pragma unroll
    for (int b = 0; b < BINS; ++b) {
      const bool rd = MODE == 0 ? !init : (bits >> b) & 1u;
      h[b] = rd ? (blk + (size_t)b * a.plane)[lq] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < BINS; ++b) {
      h[b] = __fmul_rn(h[b], a.alpha);
      if (b == i) h[b] = __fadd_rn(h[b], a.inc), hi = h[b];
      if (b == j) hj = h[b];
      bits = h[b] != 0.0f ? bits | (1u << b) : bits & ~(1u << b);
    }
#pragma unroll
    for (int b = 0; b < BINS; ++b) {
      const bool mine = (need >> b) & 1u;
      bool st;
      if constexpr (MODE == 0) st = active;
      else if constexpr (MODE == 1) st = active && __ballot(mine) != 0;  // the whole wave stores or skips
      else st = mine;
      if (st) (blk + (size_t)b * a.plane)[lq] = h[b];
    }
  } else if constexpr (MODE == 0) {
#pragma unroll 4
    for (int b = 0; b < a.bin_count; ++b) {
      float* e = blk + (size_t)b * a.plane;
      float h = init ? 0.0f : e[lq];
      h = __fmul_rn(h, a.alpha);
      if (b == i) h = __fadd_rn(h, a.inc), hi = h;
      if (b == j) hj = h;
      if (active) e[lq] = h;
    }
  } else {
    for (int b = 0; b < a.bin_count; ++b) {
      const bool old = (bits >> b) & 1u, need = active && (old || b == i);
      if (__ballot(need) == 0) continue;  // wave-uniform
      float* e = blk + (size_t)b * a.plane;
      float h = old ? e[lq] : 0.0f;
      h = __fmul_rn(h, a.alpha);
      if (b == i) h = __fadd_rn(h, a.inc), hi = h;
      if (b == j) hj = h;
      bits = h != 0.0f ? bits | (1u << b) : bits & ~(1u << b);
      if (MODE == 1 ? active : need) e[lq] = h;
    }
  }
  if constexpr (MODE != 0)
    if (active) a.live[q] = bits;
  const bool fgd = !quiet && (double)hi < a.threshold;
  if (hj < hi) bgv = g;
  if (active) {
    a.bg[q] = (uint8_t)bgv;
    if (a.bgout) a.bgout[q] = (uint8_t)bgv;
    if (a.fg) a.fg[q] = fgd ? 255 : 0;
  }
  if (a.fg_bits) {  // npix % 64 == 0 is checked on the host: a wave is either all active or all idle
    const unsigned long long w = __ballot(active && fgd);
    if ((threadIdx.x & (kWave - 1)) == 0 && active) a.fg_bits[p >> 6] = w;
  }
}

}  // namespace bgs
