// kernel_multicue_box.h — the box stage of package_bgs/sjn SJN_MultiCueBGS: from the landmark map and the frame to the
// foreground map, the two update maps and the boxes.  Three launches over all streams:
//
//   mc_box_prepare_kernel  MorphologicalOpearions(0.5, 5) SJN_MultiCueBGS.cpp:671; cvResize(CV_INTER_NN) + cvCvtColor(BGR2GRAY) of :990-995
//                          for the whole reduced frame; the ghost map starts as 0 and the update map as 1 (:367-372)
//   mc_box_label_kernel    Labeling :720, SetBoundingBox :807, EvaluateBoxSize :886: one workgroup per stream
//   mc_box_verify_kernel   EvaluateGhostRegion step 1 :983-1027 with CalculateHausdorffDist :1056, RemovingInvalidForeRegions :1117 and
//                          the valid boxes of :374-382: one workgroup per (stream, box) over a fixed grid, early exit
//
// Labeling is not a connected-component labelling: a merge copies one table entry once (aTable1[larger] = aTable1[smaller]) and is never
// resolved, so the result depends on the raster order.  What can be done in parallel without changing it:
//   pass 1  the labels do not read the table at all.  Rows are a chain (a pixel reads the label above it); within a row the label of a run
//           is the running minimum of its first pixel's value (the label above, or a new one) and the non-zero labels above the run, and
//           a new label is the count so far plus the number of run starts with nothing above: ONE segmented scan per row.
//   merges  a pixel is a merge when the labels above and to the left are non-zero and differ - known once pass 1 is done.  They are
//           compacted in raster order, a chunk of pixels at a time, and ONE lane replays them in that order.
//   pass 2  aTable2 numbers the table values by first appearance: an LDS atomicMin of the first position of every value, then a count of
//           the first positions in raster order.
// Every loop is bounded by the pixel count; no workgroup waits for another.
//
// This header is compiled by bgs_multicue_box.hip alone, a translation unit of its own inside libbgs_hip.so: the code object that holds
// every other kernel of the library is the one it was before these kernels existed.  multicue_box.h is what the host side sees.
#pragma once
#include "bgs_device.h"
#define BGS_CANNY_IMAGE_ONLY  // canny_kernel itself is emitted by bgs_hip.hip
#include "kernel_canny.h"
#include "multicue_box.h"

namespace bgs {

constexpr int kMcLabelBlock = 256;  // 4 waves: the row chain costs one barrier per row, the whole-image passes 80 chunks of a 160 x 120 frame
constexpr int kMcLabelWaves = kMcLabelBlock / kWave;
constexpr int kMcMaxLabels = kCannyMaxPixels / 2;  // a new label needs a background pixel to its left: at most half of a row
constexpr int kMcGhostDist2 = 100;  // dThreshold 10, squared

// grid (blocks of pixels, streams)
__global__ __launch_bounds__(kBlock) void mc_box_prepare_kernel(const McBoxArgs a) {
  const uint32_t n = (uint32_t)a.rw * a.rh, i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const size_t st = blockIdx.y, o = st * n + i;
  const int y = (int)(i / (uint32_t)a.rw), x = (int)(i - (uint32_t)y * a.rw);
  int v = 0;
  if (x >= 2 && x < a.rw - 2 && y >= 2 && y < a.rh - 2) {
    const uint8_t* lm = a.landmark + st * n;
    int c = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) c += lm[(y + dy) * a.rw + (x + dx)] == 255;
    v = c >= 12 ? 255 : 0;  // (int)(5 * 5 * 0.5)
  }
  a.fore0[o] = (uint8_t)v, a.fore[o] = (uint8_t)v, a.ghost[o] = 0, a.update[o] = 1;
  const int sy = min((int)floor(y * a.inv_fy), a.rows - 1), sx = min((int)floor(x * a.inv_fx), a.cols - 1);
  const uint8_t* p = a.frames + (st * a.rows * a.cols + (size_t)sy * a.cols + sx) * 3;
  a.grey[o] = (uint8_t)gray_bgr(p[0], p[1], p[2]);
}

// An element of the row scan: nw = run starts with nothing above so far; fv = value (bits 0..15) | "a run starts here or later" (bit 16).
// Values: a label, kMcScanNew for a new label (above every label, so the minimum keeps it only while nothing smaller joined), kMcScanNone
struct McScan {
  int nw, fv;
};
constexpr int kMcScanNew = 0xfffe, kMcScanNone = 0xffff, kMcScanStart = 0x10000;

__device__ __forceinline__ McScan mc_scan_join(McScan a, McScan b) {  // a lies to the left of b
  McScan r;
  r.nw = a.nw + b.nw;
  r.fv = (b.fv & kMcScanStart) ? b.fv : ((a.fv & kMcScanStart) | min(a.fv & 0xffff, b.fv & 0xffff));
  return r;
}

struct McLabelLds {
  uint16_t pass1[kCannyMaxPixels];       // aPass1; before the row chain reaches a pixel: non-zero = foreground
  uint16_t table[kMcMaxLabels + 1];      // aTable1
  uint32_t first[kMcMaxLabels + 1];      // per table value: raster index of its first pixel, then 0x80000000 | its final label (aTable2)
  uint32_t events[kMcLabelBlock];        // the merges of one chunk: larger << 16 | smaller
  McScan wave_total[2][kMcLabelWaves], carry[2];
  int wave_count[2][kMcLabelWaves];
  int box[4][kMcMaxBoxes];               // left, right, upper, bottom
};

// exclusive position of the lanes with `flag` among all lanes of the workgroup in lane order; `total` is the number of them.
// Ends with a barrier; `par` alternates between consecutive calls so that a fast wave never overwrites what a slow one still reads.
__device__ __forceinline__ int mc_block_rank(bool flag, int par, McLabelLds& L, int& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) L.wave_count[par][wave] = __popcll(b);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kMcLabelWaves; ++w) {
    const int c = L.wave_count[par][w];
    base += w < wave ? c : 0, total += c;
  }
  return base + __popcll(b & ((1ull << lane) - 1ull));
}

// grid (streams)
__global__ __launch_bounds__(kMcLabelBlock) void mc_box_label_kernel(const McBoxArgs a) {
  __shared__ McLabelLds L;
  const int tid = threadIdx.x, nt = kMcLabelBlock, lane = tid & (kWave - 1), wave = tid / kWave;
  const int rw = a.rw, rh = a.rh, n = rw * rh;
  const size_t st = blockIdx.x;
  const uint8_t* fore = a.fore0 + st * n;
  for (int i = tid; i < n; i += nt) {
    const int y = i / rw, x = i - y * rw;
    L.pass1[i] = (y >= 1 && x >= 1 && fore[i] == 255) ? 0xffff : 0;  // the scans start at (1, 1)
  }
  for (int i = tid; i <= kMcMaxLabels; i += nt) L.table[i] = (uint16_t)i, L.first[i] = 0xffffffffu;
  __syncthreads();

  // ---- pass 1: one segmented scan per row (and per kMcLabelBlock columns of it)
  int cnt = 0, it = 0;
  for (int y = 1; y < rh; ++y) {
    McScan full{0, 0};
    for (int x0 = 0; x0 < rw; x0 += nt, ++it) {
      const int x = x0 + tid, par = it & 1;
      McScan e{0, kMcScanStart | kMcScanNone};
      bool fg = false;
      if (x < rw && L.pass1[y * rw + x]) {
        fg = true;
        const int up = L.pass1[(y - 1) * rw + x];
        const bool run = L.pass1[y * rw + x - 1] != 0;  // the pixel to the left is foreground (x >= 1 here): labelled or about to be
        e.nw = !run && up == 0;
        e.fv = (run ? 0 : kMcScanStart) | (up ? up : run ? kMcScanNone : kMcScanNew);
      }
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        McScan o;
        o.nw = __shfl_up(e.nw, off, kWave), o.fv = __shfl_up(e.fv, off, kWave);
        if (lane >= off) e = mc_scan_join(o, e);
      }
      if (lane == kWave - 1) L.wave_total[par][wave] = e;
      __syncthreads();
      McScan left = x0 == 0 ? McScan{0, kMcScanStart | kMcScanNone} : L.carry[par];
      full = left;
#pragma unroll
      for (int w = 0; w < kMcLabelWaves; ++w) {
        if (w == wave) left = full;
        full = mc_scan_join(full, L.wave_total[par][w]);
      }
      const McScan r = mc_scan_join(left, e);
      if (fg) L.pass1[y * rw + x] = (uint16_t)((r.fv & 0xffff) == kMcScanNew ? cnt + r.nw : (r.fv & 0xffff));
      if (tid == 0) L.carry[par ^ 1] = full;
    }
    cnt += full.nw;  // the same in every lane
  }
  __syncthreads();

  // ---- the merges, in raster order: aTable1[larger] = aTable1[smaller], one level, as it stands at that moment
  for (int i0 = 0; i0 < n; i0 += nt, ++it) {
    const int i = i0 + tid;
    int hi = 0, lo = 0;
    if (i < n && i >= rw && L.pass1[i]) {
      const int up = L.pass1[i - rw], le = L.pass1[i - 1];  // column 0 holds no label, so le of column 1 is 0
      if (up && le && up != le) hi = max(up, le), lo = min(up, le);
    }
    int total;
    const int at = mc_block_rank(hi != 0, it & 1, L, total);
    if (total == 0) continue;  // the same in every lane
    if (hi) L.events[at] = ((uint32_t)hi << 16) | (uint32_t)lo;
    __syncthreads();
    if (tid == 0)
      for (int k = 0; k < total; ++k) {
        const uint32_t ev = L.events[k];
        L.table[ev >> 16] = L.table[ev & 0xffffu];
      }
    __syncthreads();
  }
  __syncthreads();

  // ---- pass 2: number the table values by first appearance
  for (int i = tid; i < n; i += nt)
    if (L.pass1[i]) atomicMin(&L.first[L.table[L.pass1[i]]], (uint32_t)i);
  __syncthreads();
  int labels = 0;
  for (int i0 = 0; i0 < n; i0 += nt, ++it) {
    const int i = i0 + tid;
    int v = 0;
    if (i < n && L.pass1[i]) {
      v = L.table[L.pass1[i]];
      if (L.first[v] != (uint32_t)i) v = 0;
    }
    int total;
    const int at = mc_block_rank(v != 0, it & 1, L, total);
    if (v) L.first[v] = 0x80000000u | (uint32_t)(labels + at + 1);  // no raster index has bit 31: nobody mistakes it for a position
    labels += total;
  }
  __syncthreads();

  // ---- SetBoundingBox on the first kMcMaxBoxes labels; the rest is dropped and counted
  const int kept = min(labels, kMcMaxBoxes);
  for (int k = tid; k < kMcMaxBoxes; k += nt) L.box[0][k] = 9999, L.box[1][k] = 0, L.box[2][k] = 9999, L.box[3][k] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += nt) {
    if (!L.pass1[i]) continue;
    const int k = (int)(L.first[L.table[L.pass1[i]]] & 0x7fffffffu) - 1;
    if (k >= kMcMaxBoxes) continue;
    const int y = i / rw, x = i - y * rw;
    atomicMin(&L.box[0][k], x), atomicMax(&L.box[1][k], x), atomicMin(&L.box[2][k], y), atomicMax(&L.box[3][k], y);
  }
  __syncthreads();
  const int bw = rw / 80, bh = rh / 60;
  const int lo_w = max(rw / 32, 5), lo_h = max(rh / 24, 5);
  for (int k = tid; k < kMcMaxBoxes; k += nt) {
    int* q = a.boxes + (st * kMcMaxBoxes + k) * kMcBoxFields;
    int f[kMcBoxFields] = {0};
    if (k < kept) {
      int le = L.box[0][k] - bw, ri = L.box[1][k] + bw, up = L.box[2][k] - bh, bo = L.box[3][k] + bh;
      if (le < 2) le = 2;
      if (ri >= rw - 2) ri = rw - 3;
      if (up < 2) up = 2;
      if (bo >= rh - 2) bo = rh - 3;
      f[0] = le, f[1] = ri, f[2] = up, f[3] = bo;
      f[4] = (short)(int)(le * a.fw), f[5] = (short)(int)(ri * a.fw), f[6] = (short)(int)(up * a.fh), f[7] = (short)(int)(bo * a.fh);
      const int w = ri - le, h = bo - up;
      f[8] = f[9] = lo_w <= w && w <= rw && lo_h <= h && h <= rh;
    }
#pragma unroll
    for (int j = 0; j < kMcBoxFields; ++j) q[j] = f[j];
  }
  if (tid == 0) {
    a.count[st] = labels;
    if (labels > kMcMaxBoxes) atomicAdd(a.box_overflow, 1ull);
  }
}

struct McVerifyLds {
  CannyLds canny;
  alignas(4) uint8_t frame_edges[kCannyMaxPixels], fore_edges[kCannyMaxPixels];
  int sums[3];
};

// grid (kMcMaxBoxes, streams).  The windows are cut from fore0, the map before any removal, so no box depends on another.
__global__ __launch_bounds__(kCannyBlock) void mc_box_verify_kernel(const McBoxArgs a) {
  __shared__ McVerifyLds L;
  const int k = blockIdx.x, tid = threadIdx.x, nt = kCannyBlock;
  const size_t st = blockIdx.y, n = (size_t)a.rw * a.rh;
  if (k >= min(a.count[st], kMcMaxBoxes)) return;
  int* q = a.boxes + (st * kMcMaxBoxes + k) * kMcBoxFields;
  const int le = q[0], ri = q[1], up = q[2], bo = q[3], rw = a.rw;
  const int w = ri - le, h = bo - up;  // the right column and the bottom row stay outside
  bool valid = q[8] != 0, is_ghost = false;
  if (valid) {  // the size test passed: 5 <= w, h and the window lies inside the frame, so w * h < n <= kCannyMaxPixels
    const size_t off = st * n + (size_t)up * rw + le;
    if (tid < 3) L.sums[tid] = 0;
    canny_image(a.grey + off, (size_t)rw, L.frame_edges, (size_t)w, h, w, 100, 150, L.canny);
    __syncthreads();
    canny_image(a.fore0 + off, (size_t)rw, L.fore_edges, (size_t)w, h, w, 100, 150, L.canny);
    __syncthreads();
    int na = 0, nb = 0, near = 0;
    for (int i = tid; i < w * h; i += nt) {
      na += L.frame_edges[i] != 0;
      if (!L.fore_edges[i]) continue;
      ++nb;
      const int y = i / w, x = i - y * w;
      bool hit = false;
      for (int yy = max(y - 10, 0); yy <= min(y + 10, h - 1) && !hit; ++yy) {
        const int dy2 = (yy - y) * (yy - y);
        for (int xx = max(x - 10, 0); xx <= min(x + 10, w - 1); ++xx)
          if ((xx - x) * (xx - x) + dy2 <= kMcGhostDist2 && L.frame_edges[yy * w + xx]) {
            hit = true;
            break;
          }
      }
      near += hit;
    }
    if (na) atomicAdd(&L.sums[0], na);
    if (nb) atomicAdd(&L.sums[1], nb);
    if (near) atomicAdd(&L.sums[2], near);
    __syncthreads();
    na = L.sums[0], nb = L.sums[1], near = L.sums[2];
    // CalculateHausdorffDist > 10: an empty set gives the size of the other; otherwise the (int)(0.9 nb)-th smallest of nb integer squared
    // distances is above 100 exactly when at most (int)(0.9 nb) of them are <= 100
    is_ghost = (na == 0 || nb == 0) ? max(na, nb) > 10 : near <= (int)(0.9 * (double)nb);
    if (is_ghost) valid = false;
    if (tid == 0) q[9] = valid, q[10] = na, q[11] = nb, q[12] = near;
  }
  uint8_t *fore = a.fore + st * n, *ghost = a.ghost + st * n, *update = a.update + st * n;
  if (valid) {  // :374-382, the inclusive rectangle
    const int ww = w + 1, hh = h + 1;
    for (int i = tid; i < ww * hh; i += nt) update[(up + i / ww) * rw + le + i % ww] = 0;
  } else {      // :1014-1018 and :1121-1130, the exclusive rectangle; other boxes store the same values
    for (int i = tid; i < w * h; i += nt) {
      const int p = (up + i / w) * rw + le + i % w;
      if (is_ghost) ghost[p] = 1;
      if (fore[p] == 255) fore[p] = 0;
    }
  }
}

// PostProcessing and step 1 of UpdateModel_Par: three launches over all streams
void mc_box_launch(const McBoxArgs& a, unsigned streams, hipStream_t s) {
  const unsigned n = (unsigned)a.rw * (unsigned)a.rh;
  hipLaunchKernelGGL(mc_box_prepare_kernel, dim3((n + kBlock - 1) / kBlock, streams), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(mc_box_label_kernel, dim3(streams), dim3(kMcLabelBlock), 0, s, a);
  hipLaunchKernelGGL(mc_box_verify_kernel, dim3((unsigned)kMcMaxBoxes, streams), dim3(kCannyBlock), 0, s, a);
}

}  // namespace bgs
