// kernel_kde.h — KDE (package_bgs/ae: Elgammal's non-parametric kernel-density model, USTC_BGS type 32) on gfx950.
//
// Model layout, every plane stream-major so that a stream's planes are contiguous and a run of streams
// [first, first+count) is one contiguous slab of each:
//   samples  uint32 [S][SL][n]   one 4-byte record per (slot, pixel): converted bytes c0 | c1 << 8 | c2 << 16 (gray: c0 only).
//                                Trip j of a wave is one coalesced 256-byte load.  Slots never learnt hold 0 (the reference
//                                zero-fills Sequence and evaluates those slots like real samples).
//   meta     uint32 [S][n]       sd0 | sd1 << 8 | sd2 << 16 | PixelQTop << 24
//   tb       uint32 [S][TBL][n]  temporal buffer: converted bytes c0..c2 | the stored mask (0 / 255) << 24
//   acc      uint32 [S][n]       AccMask (consecutive foreground frames)
// The reference's running |diff| histogram (AbsDiffHist) is not kept: with UpdateSDRate = 0 (NPBGSubtractor.cpp:286) its
// upkeep in SequenceBGUpdate_Pairs is write-only; the SD bins are estimated once, by kde_estimate_kernel.
//
// Numerics are the reference's, in double, in its order, without contraction (the reference is built for x86-64, where
// nothing fuses a*b+c): the kernel table and the colour-ratio brightness gate are built on the host (bgs_hip.hip) and
// uploaded; the density loop is `while (j < SL && sum < th*SL) sum += ...; j++`, then p = sum / j and FG = p > th ? 0 : 255.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgs_device.h"

namespace bgs {

constexpr int kKdeHalf = 255;                 // KERNELHALFWIDTH
constexpr int kKdeWidth = 2 * kKdeHalf + 1;   // 511 doubles per SD bin
constexpr int kKdeBins = 80;                  // SEGMABINS
constexpr int kKdeAbsBins = 20;               // Estimation(): Abshistbins
constexpr uint32_t kKdeResetMaskTh = 500;     // NPBGmodel bg_suppression_time

enum KdeMode { kKdeGray = 0, kKdeRatios = 1, kKdeRgb = 2 };

struct KdeArgs {
  const uint8_t* cur;        // [npix][C] input frames of the run's streams
  uint8_t* fg;               // [npix] byte masks (nullable)
  uint64_t* fg_bits;         // packed masks (nullable; npix % 64 == 0 then)
  uint32_t* samples;         // the run's first stream: [count][SL][n]
  uint32_t* meta;            // [count][n]
  uint32_t* tb;              // [count][TBL][n]
  uint32_t* acc;             // [count][n]
  const double* lut;         // [80][511]
  const int2* gate;          // [256] (x1, x2) of the colour-ratio gate per sample brightness
  unsigned long long* trips; // optional: += density-loop trips of every lane
  uint32_t npix, n;
  double th, th_sum;         // Threshold, Threshold * SampleSize
  int SL, TBL, C, mode;
  int top;                   // learning: the slot the frame goes to
  int tb_top, tb_next;       // update: temporal buffer Top and Next
  int update, sample;        // update: run SequenceBGUpdate_Pairs; sample: this call is a sampling event
  int sd_fixed;              // estimation: >= 0 -> every bin is this (SDEstimationFlag 0), < 0 -> estimate
  int xcd_swizzle;
};

// BGR2SnGnRn (NPBGSubtractor.cpp:64-90) of one pixel, or the bytes as they are; packed c0 | c1 << 8 | c2 << 16.
__device__ __forceinline__ uint32_t kde_convert(const uint8_t* px, int C, bool ratios) {
#pragma clang fp contract(off)
  if (C == 1) return px[0];
  const unsigned b = px[0], g = px[1], r = px[2];
  if (!ratios) return b | g << 8 | r << 16;
  const double s = 255.0 / (double)(b + g + r + 30);
  const unsigned r2 = (unsigned)((double)(g + 10) * s), r3 = (unsigned)((double)(r + 10) * s);
  return ((b + g + r) / 3) | (r2 > 255 ? 255u : r2) << 8 | (r3 > 255 ? 255u : r3) << 16;
}

// Learning frame (AddFrame, NPBGSubtractor.cpp:292-298 + NPBGmodel.cpp:115-124): converted frame into slot `top` and into
// temporal slot 0, PixelQTop = top + 1 (mod SL).  The temporal mask byte is written 0: Estimation clears every mask before
// any update reads one.
__global__ __launch_bounds__(kBlock) void kde_learn_kernel(const KdeArgs a) {
  const uint32_t p = (uint32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= a.npix) return;
  const uint32_t s = p / a.n, i = p - s * a.n;
  const uint32_t x = kde_convert(a.cur + (size_t)p * a.C, a.C, a.mode == kKdeRatios);
  a.samples[((size_t)s * a.SL + a.top) * a.n + i] = x;
  a.tb[(size_t)s * a.TBL * a.n + i] = x;
  uint32_t* m = a.meta + p;
  *m = (*m & 0xffffffu) | (uint32_t)((a.top + 1) % a.SL) << 24;
}

// Estimation (NPBGSubtractor.cpp:313-348): per pixel and channel the 20-bin histogram of |slot k - slot k-1| over the whole
// sequence, its median bin interpolated (EstimateSDsFromAbsDiffHist) and turned into a kernel-table bin; clears the
// temporal masks and AccMask.  The counts (<= 254) are packed four to a register; every index into them is a constant.
__device__ __forceinline__ void kde_hist_add(uint32_t (&h)[5], int d) {
  const int b = d < kKdeAbsBins ? d : kKdeAbsBins - 1;
  const uint32_t inc = 1u << (8 * (b & 3));
#pragma unroll
  for (int w = 0; w < 5; ++w) h[w] += (b >> 2) == w ? inc : 0u;
}

__device__ __forceinline__ int kde_sd_bin(const uint32_t (&h)[5], int SL) {
#pragma clang fp contract(off)
  const int mc = (SL - 1) / 2;  // medianCount = histsum / 2, histsum = SL - 1
  int cum = 0, bin = 0, x1 = 0, x2 = 0;
  bool found = false;
#pragma unroll
  for (int b = 0; b < kKdeAbsBins; ++b) {
    const int cnt = byte_of(h[b >> 2], b & 3);
    if (!found) {
      cum += cnt;
      if (cum >= mc) found = true, bin = b, x2 = cum, x1 = cum - cnt;
    }
  }
  const double minsd = 0.5, maxsd = 36.5, factor = (double)(kKdeBins - 1) / (maxsd - minsd);
  double v = 1.04 * ((double)bin - (double)(x2 - mc) / (double)(x2 - x1));
  v = v <= minsd ? minsd : v;
  return v >= maxsd ? kKdeBins - 1 : (int)floor((v - minsd) * factor + .5);
}

__global__ __launch_bounds__(kBlock) void kde_estimate_kernel(const KdeArgs a) {
  const uint32_t p = (uint32_t)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= a.npix) return;
  const uint32_t s = p / a.n, i = p - s * a.n;
  uint32_t sd;
  if (a.sd_fixed >= 0) {
    sd = (uint32_t)a.sd_fixed * (a.C == 3 ? 0x010101u : 1u);
  } else {
    uint32_t h0[5] = {0, 0, 0, 0, 0}, h1[5] = {0, 0, 0, 0, 0}, h2[5] = {0, 0, 0, 0, 0};
    const uint32_t* q = a.samples + (size_t)s * a.SL * a.n + i;
    uint32_t prev = q[0];
    for (int k = 1; k < a.SL; ++k) {
      const uint32_t cur = q[(size_t)k * a.n];
      kde_hist_add(h0, abs(byte_of(cur, 0) - byte_of(prev, 0)));
      if (a.C == 3) {
        kde_hist_add(h1, abs(byte_of(cur, 1) - byte_of(prev, 1)));
        kde_hist_add(h2, abs(byte_of(cur, 2) - byte_of(prev, 2)));
      }
      prev = cur;
    }
    sd = (uint32_t)kde_sd_bin(h0, a.SL);
    if (a.C == 3) sd |= (uint32_t)kde_sd_bin(h1, a.SL) << 8 | (uint32_t)kde_sd_bin(h2, a.SL) << 16;
  }
  a.meta[p] = (a.meta[p] & 0xff000000u) | sd;
  a.acc[p] = 0;
  uint32_t* t = a.tb + (size_t)s * a.TBL * a.n + i;
  for (int k = 0; k < a.TBL; ++k) t[(size_t)k * a.n] &= 0xffffffu;
}

// One frame of one run of streams: NBBGSubtraction (NPBGSubtraction_Subset_Kernel, NPBGSubtractor.cpp:873-1132) and then, in
// the same lane, Update -> SequenceBGUpdate_Pairs (:664-851).  A pixel's update reads and writes only its own records, and
// its subtraction has read every sample before the update replaces any.
__global__ __launch_bounds__(kBlock) void kde_frame_kernel(const KdeArgs a) {
#pragma clang fp contract(off)
  __shared__ int2 gate[256];
  if (a.mode == kKdeRatios) gate[threadIdx.x] = a.gate[threadIdx.x];  // kBlock == 256
  __syncthreads();
  const uint32_t p = (uint32_t)(xcd_block(a.xcd_swizzle) * kBlock + threadIdx.x);
  const bool active = p < a.npix;
  uint32_t fgv = 0;
  int j = 0;
  if (active) {
    const uint32_t s = p / a.n, i = p - s * a.n;
    const uint32_t x = kde_convert(a.cur + (size_t)p * a.C, a.C, a.mode == kKdeRatios);
    uint32_t meta = a.meta[p];
    const uint32_t* q = a.samples + (size_t)s * a.SL * a.n + i;
    const int x0 = byte_of(x, 0), x1 = byte_of(x, 1), x2 = byte_of(x, 2);
    // K[sd][g - x + 255] = row(sd, x)[g]
    const double* k0 = a.lut + byte_of(meta, 0) * kKdeWidth + kKdeHalf - x0;
    const double* k1 = a.lut + byte_of(meta, 1) * kKdeWidth + kKdeHalf - x1;
    const double* k2 = a.lut + byte_of(meta, 2) * kKdeWidth + kKdeHalf - x2;
    double sum = 0;
    if (a.mode == kKdeGray) {
      while (j < a.SL && sum < a.th_sum) {
        sum += k0[byte_of(q[(size_t)j * a.n], 0)];
        ++j;
      }
    } else if (a.mode == kKdeRatios) {
      while (j < a.SL && sum < a.th_sum) {
        const uint32_t r = q[(size_t)j * a.n];
        const int2 g = gate[byte_of(r, 0)];
        if (g.x < x0 && x0 < g.y) sum += k1[byte_of(r, 1)] * k2[byte_of(r, 2)];
        ++j;
      }
    } else {
      while (j < a.SL && sum < a.th_sum) {
        const uint32_t r = q[(size_t)j * a.n];
        sum += (k0[byte_of(r, 0)] * k1[byte_of(r, 1)]) * k2[byte_of(r, 2)];
        ++j;
      }
    }
    const double prob = sum / (double)j;
    fgv = prob > a.th ? 0u : 255u;
    if (a.update) {
      uint32_t* t = a.tb + (size_t)s * a.TBL * a.n + i;
      if (a.sample) {
        const uint32_t rt = t[(size_t)a.tb_top * a.n], rn = t[(size_t)a.tb_next * a.n];
        if (((rt | rn) >> 24) == 0) {  // neither temporal frame was foreground
          uint32_t* w = a.samples + (size_t)s * a.SL * a.n + i;
          const int qt = (int)(meta >> 24);
          w[(size_t)qt * a.n] = rt;
          w[(size_t)((qt + 1) % a.SL) * a.n] = rn;
          meta = (meta & 0xffffffu) | (uint32_t)((qt + 2) % a.SL) << 24;
          a.meta[p] = meta;
        }
      }
      uint32_t acc = fgv ? a.acc[p] + 1 : 0u;
      a.acc[p] = acc;
      if (acc > kKdeResetMaskTh) fgv = 0;
      t[(size_t)a.tb_top * a.n] = x | fgv << 24;
    }
    if (a.fg) a.fg[p] = (uint8_t)fgv;
  }
  if (a.fg_bits) store_packed_mask<1>(a.fg_bits, p, fgv ? 1u : 0u, active);
  if (a.trips) {  // diagnostics (BGS_KDE_TRIPS=1): one atomic per wave
    uint32_t v = (uint32_t)j;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(a.trips, (unsigned long long)v);
  }
}

}  // namespace bgs
