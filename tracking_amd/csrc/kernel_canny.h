// kernel_canny.h — cvCanny (aperture 3, L1 magnitude) of a small 8-bit image, one workgroup per image.
//
//   canny_image   the device routine: Sobel 3x3 with a replicated border -> |dx| + |dy| -> non-maximum suppression with the
//                 15-bit fixed-point tan 22.5 deg test -> hysteresis from the pixels above `high` through those above `low`,
//                 8-connected -> 0 / 255.  What SJN_MultiCueBGS::EvaluateGhostRegion asks of cvCanny for each bounding box
//                 (package_bgs/sjn/SJN_MultiCueBGS.cpp:998, :1007); written as a routine of one workgroup so that a per-box
//                 kernel can call it on a region of interest.
//   canny_kernel  bgs_canny_device: blockIdx.x = image of the batch.
//
// The gradient words and the edge map live in LDS (3 bytes per pixel), so an image has at most kCannyMaxPixels pixels: the
// reference's reduced frame (160 x 120) fits.  Every loop is bounded by the pixel count; the workgroup waits on nobody else.
#pragma once
#include "bgs_device.h"

namespace bgs {

constexpr int kCannyBlock = 1024;         // 16 waves: one image is latency-bound, not throughput-bound
constexpr int kCannyMaxPixels = 20480;    // 3 bytes of LDS per pixel: 60 KiB; a multiple of 4
constexpr int kCannyTg22 = 13573;         // (int)(0.4142135623730950488 * (1 << 15) + 0.5)

struct CannyLds {
  uint16_t grad[kCannyMaxPixels];  // magnitude (<= 2040, bits 0..11) | direction class (bits 12..13)
  alignas(4) uint8_t map[kCannyMaxPixels];  // 0 no edge, 1 candidate above low, 2 edge; read as dwords by the hysteresis
  int changed[3];                  // one word per sweep, three in rotation: set in sweep s, read after it, cleared during s + 1 for s + 2
};

// src: rows x cols bytes, rows `step` bytes apart.  dst: rows x cols, rows `dstep` apart.  Called by every thread of the workgroup.
__device__ __forceinline__ void canny_image(const uint8_t* __restrict__ src, size_t step, uint8_t* __restrict__ dst, size_t dstep, int rows, int cols, int low,
                                            int high, CannyLds& L) {
  const int n = rows * cols, tid = threadIdx.x, nt = blockDim.x;
  if (tid < 3) L.changed[tid] = 0;
  // Sobel with a replicated border; direction class 0 = along the row, 1 = along the column, 2 = diagonal, 3 = anti-diagonal
  for (int i = tid; i < n; i += nt) {
    const int y = i / cols, x = i - y * cols;
    const int xm = max(x - 1, 0), xp = min(x + 1, cols - 1);
    const uint8_t *r0 = src + (size_t)max(y - 1, 0) * step, *r1 = src + (size_t)y * step, *r2 = src + (size_t)min(y + 1, rows - 1) * step;
    const int a = r0[xm], b = r0[x], c = r0[xp], d = r1[xm], f = r1[xp], g = r2[xm], h = r2[x], k = r2[xp];
    const int dx = (c + 2 * f + k) - (a + 2 * d + g), dy = (g + 2 * h + k) - (a + 2 * b + c);
    const int ax = abs(dx), ay = abs(dy) << 15, tg22x = ax * kCannyTg22, tg67x = tg22x + (ax << 16);
    const int dir = ay < tg22x ? 0 : ay > tg67x ? 1 : ((dx ^ dy) < 0 ? 3 : 2);
    L.grad[i] = (uint16_t)((ax + abs(dy)) | (dir << 12));
  }
  __syncthreads();
  // non-maximum suppression; the magnitude outside the image is 0
  for (int i = tid; i < n; i += nt) {
    const int y = i / cols, x = i - y * cols;
    const int w = L.grad[i], m = w & 0xfff, dir = w >> 12;
    auto mag = [&](int yy, int xx) { return (yy < 0 || yy >= rows || xx < 0 || xx >= cols) ? 0 : (L.grad[yy * cols + xx] & 0xfff); };
    int keep = 0;
    if (m > low) {
      if (dir == 0)
        keep = m > mag(y, x - 1) && m >= mag(y, x + 1);
      else if (dir == 1)
        keep = m > mag(y - 1, x) && m >= mag(y + 1, x);
      else {
        const int s = dir == 3 ? -1 : 1;
        keep = m > mag(y - 1, x - s) && m > mag(y + 1, x + s);
      }
    }
    L.map[i] = keep ? (m > high ? 2 : 1) : 0;
  }
  if (tid < 3 && n + tid < ((n + 3) & ~3)) L.map[n + tid] = 0;  // the rest of the last dword (kCannyMaxPixels is a multiple of 4)
  __syncthreads();
  // hysteresis: a candidate beside an edge becomes an edge.  Values only rise (1 -> 2), so the fixed point does not depend on the order
  // in which lanes see each other's writes.  A sweep reads the map four pixels at a time; a lane that promotes a pixel follows the
  // candidates hanging on it, one step per promotion, so a long thin chain costs steps of one lane instead of sweeps of the whole
  // workgroup.  Every sweep that sets `changed` promoted at least one pixel, and every step promotes one: at most n of either.
  const uint32_t* map32 = reinterpret_cast<const uint32_t*>(L.map);
  const int nw = (n + 3) >> 2;
  for (int sweep = 0; sweep < n; ++sweep) {
    int any = 0;
    for (int w = tid; w < nw; w += nt) {
      const uint32_t v = map32[w] ^ 0x01010101u;
      if (!((v - 0x01010101u) & ~v & 0x80808080u)) continue;  // no byte of the four is 1
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * w + j;
        if (((v >> (8 * j)) & 0xffu) != 0 || L.map[i] != 1) continue;
        int y = i / cols, x = i - y * cols, e = 0;
        for (int yy = max(y - 1, 0); yy <= min(y + 1, rows - 1); ++yy)
          for (int xx = max(x - 1, 0); xx <= min(x + 1, cols - 1); ++xx) e |= L.map[yy * cols + xx] == 2;
        if (!e) continue;
        L.map[i] = 2, any = 1;
        for (int step = 0; step < n; ++step) {
          int ny = -1, nx = -1;
          for (int yy = max(y - 1, 0); yy <= min(y + 1, rows - 1); ++yy)
            for (int xx = max(x - 1, 0); xx <= min(x + 1, cols - 1); ++xx)
              if (L.map[yy * cols + xx] == 1) ny = yy, nx = xx;
          if (ny < 0) break;
          L.map[ny * cols + nx] = 2, y = ny, x = nx;
        }
      }
    }
    const int slot = sweep % 3;
    if (any) L.changed[slot] = 1;
    if (tid == 0) L.changed[(sweep + 1) % 3] = 0;
    __syncthreads();
    if (!L.changed[slot]) break;  // the same word for every thread: the whole workgroup leaves together
  }
  for (int i = tid; i < n; i += nt) {
    const int y = i / cols, x = i - y * cols;
    dst[(size_t)y * dstep + x] = L.map[i] == 2 ? 255 : 0;
  }
}

#ifndef BGS_CANNY_IMAGE_ONLY  // a translation unit that wants canny_image alone (bgs_multicue_box.hip) leaves the kernel to bgs_hip.hip
__global__ __launch_bounds__(kCannyBlock) void canny_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int cols, int low, int high) {
  __shared__ CannyLds L;
  const size_t off = (size_t)blockIdx.x * rows * cols;
  canny_image(src + off, (size_t)cols, dst + off, (size_t)cols, rows, cols, low, high, L);
}
#endif

}  // namespace bgs
