// kernel_imbs.h — package_bgs/db IndependentMultimodalBGS (Bloisi and Iocchi's IMBS, BGS_IMBS; host side in engine_imbs.h).
//
// BackgroundSubtractorIMBS::apply (imbs.cpp:164-209) statement by statement.  Per stream and frame, all on the caller's stream and
// with nothing read back by the host:
//   imbs_detect_kernel    getFg (:448-505) + hsvSuppression (:243-293) + filterFg's 255-plane and its count (:674-683)
//   morph_box_kernel x 4  open + close 3x3 when morphologicalFiltering (:689-693)
//   imbs_area_*           areaThresholding (:507-534), see below
//   imbs_final_kernel     filterFg's tail (:697-706)
//   imbs_control_kernel   the scalars of apply / changeBg / filterFg's sudden_change / updateBg / createBg's tail for one stream
//   imbs_sample_kernel    createBg (:295-446) where the control block planned one
//   imbs_out_kernel       the images the caller gets (zero while bgModel[0].isValid[0] is false)
// A frame's scalars live in an ImbsCtl in device memory.  The detect kernel needs only what it can derive itself (the gate is the
// valid bit of pixel 0's first model slot, dt is (timestamp + 1000./fps) - timestamp), so the control kernel runs after it and sees
// this frame's 255-count: sudden_change set by filterFg acts on createBg's tail of the same frame, as in the reference.
//
// State, one dword per pixel and slot, plane-major ([stream][slot][pixel], so a wave reads 256 contiguous bytes per slot):
//   bins   bytes 0..2 binValues (B, G, R), byte 3 = binHeights (bits 0..5) | isFg << 7
//   model  bytes 0..2 values, byte 3 = counter (bits 0..5) | isValid << 6 | isFg << 7
// Everything is integer except the HSV test, which is the reference's float sequence (IEEE divide, no contraction: the library's
// build flags).  Atomics are integer only, so every run gives the same bytes.
//
// The area filter.  OpenCV's findContours / moments / drawContours are not in the tree; the contract is DESIGN.md §5.10.  The device
// form needs no border following: label the ones (8-connected) and the zeros (4-connected) with kernel_cc.h, split every 2 x 2
// quad's unit area between the regions in it (half units, integer atomics), and a contour's area is its region's share plus the
// shares of everything nested in it.  The nesting needs no search: a component's parent is the zero region of the pixel left of its
// first raster pixel, a hole's parent is the component of the pixel above its first raster pixel, the region of pixel 0 is the root.
#pragma once
#include "bgs_device.h"
#include "kernel_cc.h"

namespace bgs {

struct ImbsCtl {
  double ts, prev_ts;        // timestamp, prev_timestamp (ms)
  unsigned long long pbft;   // prev_bg_frame_time (unsigned long)
  uint32_t bfc, ns, sp;      // bg_frame_counter, numSamples, samplingPeriod (all unsigned int in the reference)
  uint32_t bg_reset, sudden;
  uint32_t count255;         // 255-labelled pixels of this frame before the filter (detect kernel), cleared by the control kernel
  uint32_t plan, plan_k, plan_ns;  // createBg of this frame: bit 0 run, bit 1 copy the frame into bgSample first; its argument; numSamples at the call
  uint32_t pad;
};

constexpr uint32_t kImbsValid = 1u << 30, kImbsFg = 1u << 31, kImbsCount = 0x3f000000u;

struct ImbsArgs {
  const uint8_t* cur;        // [count][n][3]
  uint8_t *fg, *bgout;       // nullable
  uint32_t *bins, *model, *persist, *smp, *bgimg;
  uint8_t *lab, *plane, *ones, *zeros;
  int *L1, *L0, *Q, *A;
  ImbsCtl* ctl;
  uint32_t n, cap, M;        // pixels, bin slots (numSamples as given), model slots (maxBgBins)
  int rows, cols;
  uint32_t fg_thr, assoc, min_bin, persist_period;
  float alpha, beta;
  int tau_s, tau_h;
  double step, min_area, max_area;  // 1000./fps; minArea; 0.6 * numPixels
};

__device__ __forceinline__ int imbs_dist(uint32_t a, uint32_t b) {  // max over the channels of |a - b|
  const int d0 = abs(byte_of(a, 0) - byte_of(b, 0)), d1 = abs(byte_of(a, 1) - byte_of(b, 1)), d2 = abs(byte_of(a, 2) - byte_of(b, 2));
  return max(max(d0, d1), d2);
}

// The reference's RGB -> HSV on full bytes (imbs.cpp:539-665) for one pixel; bytes 0..2 of the result are H, S, V.  Only the order
// of the float operations matters for the bits: channels scaled by the constant 1.0f / 255.0f, value = the largest channel,
// saturation = (max - min) / max, hue = sector offset + channel difference * (1 / (6 * (max - min))), the sector chosen by
// "largest == red" first, then green, wrapped into [0, 1); each of the three rounded as (int)(0.5f + x * 255.0f) and clipped.
__device__ __forceinline__ int imbs_unit_to_byte(float x) {
  const float t = 0.5f + x * 255.0f;
  if (t != t) return 0;  // (int) of a NaN is INT_MIN on the reference's machine and the clip makes it 0
  return min(max((int)t, 0), 255);
}
__device__ __forceinline__ uint32_t imbs_hsv(uint32_t px) {
  const float scale = 1.0f / 255.0f;
  const int b = byte_of(px, 0), g = byte_of(px, 1), r = byte_of(px, 2);
  const int hi = max(max(b, g), r), lo = min(min(b, g), r);
  const float fb = b * scale, fg = g * scale, fr = r * scale, vmax = hi * scale, vmin = lo * scale;
  float hue = 0.0f, sat = 0.0f;
  if (hi != 0) {  // not pure black
    const float span = vmax - vmin;
    sat = span / vmax;
    const float unit = 1.0f / (6.0f * span);  // a gray pixel: inf, and its hue 0 * inf = NaN, which comes out as byte 0
    if (hi == r) hue = (fg - fb) * unit;
    else if (hi == g) hue = (2.0f / 6.0f) + (fb - fr) * unit;
    else hue = (4.0f / 6.0f) + (fr - fg) * unit;
    if (hue < 0.0f) hue += 1.0f;
    if (hue >= 1.0f) hue -= 1.0f;
  }
  return (uint32_t)imbs_unit_to_byte(hue) | ((uint32_t)imbs_unit_to_byte(sat) << 8) | ((uint32_t)imbs_unit_to_byte(vmax) << 16);
}

__device__ __forceinline__ uint32_t imbs_pixel(const uint8_t* cur, size_t p) {
  const uint8_t* q = cur + p * 3;
  return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
}

// a stream's first frame: initialize() (imbs.cpp:98-162); the planes are cleared by the host's memsets on the same stream
__global__ void imbs_ctl_init_kernel(ImbsCtl* ctl, int count, uint32_t ns, uint32_t sp) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  ImbsCtl c{};
  c.ns = ns, c.sp = sp;
  ctl[k] = c;
}

__global__ __launch_bounds__(kBlock) void imbs_detect_kernel(const ImbsArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const size_t k = blockIdx.y, n = a.n;
  const bool in = p < n;
  uint32_t* model = a.model + k * a.M * n;
  // bgModel[0].isValid[0].  Pixel 0's lane may store to this word in this launch (it clears isFg past persistencePeriod); the store
  // is one dword and never changes the valid bit, so whichever value a lane reads gives the same gate.
  const bool gate = (model[0] & kImbsValid) != 0;
  int label = 0;
  if (in && gate) {
    const double ts0 = a.ctl[k].ts, dt = (ts0 + a.step) - ts0;  // timestamp - prev_timestamp
    const uint32_t px = imbs_pixel(a.cur, k * n + p);
    uint32_t* pm = a.persist + k * n + p;
    bool isFg = true, cond = false;
    for (uint32_t s = 0; s < a.M; ++s) {  // getFg
      const uint32_t w = model[s * n + p];
      if (!(w & kImbsValid)) {
        if (s == 0) isFg = false;
        break;
      }
      if ((uint32_t)imbs_dist(w, px) < a.fg_thr) {
        if (w & kImbsFg) {
          cond = true;
          break;
        }
        isFg = false;
        *pm = 0;
      }
    }
    if (isFg) {
      if (cond) {
        label = 180;
        const uint32_t pv = (uint32_t)((double)*pm + dt);
        *pm = pv;
        if (pv > a.persist_period)
          for (uint32_t s = 0; s < a.M; ++s) {
            const uint32_t w = model[s * n + p];
            if (!(w & kImbsValid)) break;
            model[s * n + p] = w & ~kImbsFg;
          }
      } else {
        label = 255;
        *pm = 0;
      }
    }
    if (label) {  // hsvSuppression
      const uint32_t hi = imbs_hsv(px);
      const int h_i = byte_of(hi, 0), s_i = byte_of(hi, 1), v_i = byte_of(hi, 2);
      for (uint32_t s = 0; s < a.M; ++s) {
        const uint32_t w = model[s * n + p];
        if (!(w & kImbsValid)) break;
        if (w & kImbsFg) continue;
        const uint32_t hb = imbs_hsv(w);
        const int h_b = byte_of(hb, 0), s_b = byte_of(hb, 1), v_b = byte_of(hb, 2);
        const float v_ratio = (float)v_i / (float)v_b;
        const int s_diff = abs(s_i - s_b), h_diff = min(abs(h_i - h_b), 255 - abs(h_i - h_b));
        if (h_diff <= a.tau_h && s_diff <= a.tau_s && v_ratio >= a.alpha && v_ratio < a.beta) {
          label = 80;
          break;
        }
      }
    }
  }
  if (in) a.lab[k * n + p] = (uint8_t)label, a.plane[k * n + p] = label == 255 ? 255 : 0;
  const unsigned long long b = __ballot(label == 255);
  if ((threadIdx.x & (kWave - 1)) == 0 && b) atomicAdd(&a.ctl[k].count255, (uint32_t)__popcll(b));
}

// findContours zeroes the image's one-pixel frame first: `ones` is the 255-plane without it, `zeros` its complement
__global__ __launch_bounds__(kBlock) void imbs_area_prep_kernel(const ImbsArgs a, const uint8_t* plane) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n) return;
  const size_t g = (size_t)blockIdx.y * a.n + p;
  const int y = (int)(p / (uint32_t)a.cols), x = (int)(p - (uint32_t)y * a.cols);
  const bool o = plane[g] != 0 && y > 0 && y < a.rows - 1 && x > 0 && x < a.cols - 1;
  a.ones[g] = o ? 255 : 0, a.zeros[g] = o ? 0 : 255;
  a.Q[g] = 0, a.A[g] = 0;
}

// `amount` half units for region `root` (< 0: nothing) from every lane of a wave: lanes that name the same region add up first,
// so a region that fills the wave costs one atomic, not 64.  Every lane of the wave must call it.
__device__ __forceinline__ void imbs_wave_add(int* Q, int root, int amount) {
  const int lane = threadIdx.x & (kWave - 1);
  unsigned long long pending = __ballot(root >= 0);
  while (pending) {  // wave-uniform
    const int leader = __ffsll((long long)pending) - 1;
    const int r = __shfl(root, leader);
    const bool mine = root == r;
    int v = mine ? amount : 0;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == leader) atomicAdd(&Q[r], v);
    pending &= ~__ballot(mine);
  }
}

// every 2 x 2 quad's unit area, in half units, to the regions in it (labels are roots: after cc_compress_kernel).  The outside
// region (pixel 0's) has no contour and takes no share: most quads of a frame lie in it, and they would all meet in one address.
__global__ __launch_bounds__(kBlock) void imbs_area_quads_kernel(const ImbsArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const int y = (int)(p / (uint32_t)a.cols), x = (int)(p - (uint32_t)y * a.cols);
  const int base = (int)((size_t)blockIdx.y * a.n);
  int r0 = -1, a0 = 0, r1 = -1, a1 = 0;
  if (p < a.n && y < a.rows - 1 && x < a.cols - 1) {
    const size_t g = (size_t)base + p;
    const size_t q[4] = {g, g + 1, g + (size_t)a.cols, g + (size_t)a.cols + 1};
    bool o[4];
    int cnt = 0, one = -1, z0 = -1, z1 = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = a.ones[q[i]] != 0;
      cnt += o[i];
      if (o[i]) one = i;
      else if (z0 < 0) z0 = i;
      else z1 = i;
    }
    if (cnt == 4) {
      r0 = a.L1[q[0]], a0 = 2;
    } else if (cnt == 3) {
      r0 = a.L1[q[one]], a0 = 1, r1 = a.L0[q[z0]], a1 = 1;
    } else if (cnt == 2 && o[0] == o[3]) {  // the ones on a diagonal: the two zeros may be different regions
      r0 = a.L0[q[z0]], a0 = 1, r1 = a.L0[q[z1]], a1 = 1;
    } else {
      r0 = a.L0[q[z0]], a0 = 2;
    }
    if (r0 == base) r0 = -1;
    if (r1 == base) r1 = -1;
  }
  imbs_wave_add(a.Q, r0, a0);
  imbs_wave_add(a.Q, r1, a1);
}

// A[region] = its own share + the shares of everything nested in it: every region adds its share to itself and to all its ancestors
__global__ __launch_bounds__(kBlock) void imbs_area_push_kernel(const ImbsArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n) return;
  const int base = (int)((size_t)blockIdx.y * a.n), g = base + (int)p;
  const bool one = a.ones[g] != 0;
  if ((one ? a.L1[g] : a.L0[g]) != g || g == base) return;  // roots only; the region of pixel 0 is the outside and has no contour
  const int own = a.Q[g];
  if (!own) return;
  int c, z;
  if (one) {
    c = g;
  } else {
    atomicAdd(&a.A[g], own);
    c = a.L1[g - a.cols];
  }
  for (int depth = 0; depth < a.rows && c > base; ++depth) {  // nesting is at most rows / 4 deep: the bound only keeps a wrong label from looping
    atomicAdd(&a.A[c], own);
    z = a.L0[c - 1];
    if (z <= base) break;
    atomicAdd(&a.A[z], own);
    c = a.L1[z - a.cols];
  }
}

__device__ __forceinline__ bool imbs_kept(const ImbsArgs& a, int half_units) {
  const double area = half_units * 0.5;
  return !(area < a.min_area || area >= a.max_area);
}

// per component: is some contour on its chain outer(C), hole(parent), outer(grandparent), ... kept?  -> Q[root] (its shares are spent)
__global__ __launch_bounds__(kBlock) void imbs_area_chain_kernel(const ImbsArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n) return;
  const int base = (int)((size_t)blockIdx.y * a.n), g = base + (int)p;
  if (a.ones[g] == 0 || a.L1[g] != g) return;
  int c = g, kept = 0;
  for (int depth = 0; depth < a.rows && c > base; ++depth) {
    if (imbs_kept(a, a.A[c])) {
      kept = 1;
      break;
    }
    const int z = a.L0[c - 1];
    if (z <= base) break;
    if (imbs_kept(a, a.A[z])) {
      kept = 1;
      break;
    }
    c = a.L1[z - a.cols];
  }
  a.Q[g] = kept;
}

// filterFg's tail: what the area filter leaves of the 255-plane, then the 180 / 80 labels on top; the result is fgmask
__global__ __launch_bounds__(kBlock) void imbs_final_kernel(const ImbsArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n) return;
  const int base = (int)((size_t)blockIdx.y * a.n), g = base + (int)p;
  const int v = a.lab[g];
  if (v == 180 || v == 80) return;
  int s = 0;
  if (a.ones[g]) {  // never a frame pixel: its four neighbours exist
    const int c = a.L1[g];
    s = a.Q[c];
    if (!s) {  // a pixel on the border of one of C's own holes survives with that hole's contour
      const int parent = a.L0[c - 1];
      const int nb[4] = {g - 1, g + 1, g - a.cols, g + a.cols};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (!a.ones[nb[i]]) {
          const int z = a.L0[nb[i]];
          if (z != parent && imbs_kept(a, a.A[z])) s = 1;
        }
    }
  }
  a.lab[g] = s ? 255 : 0;
}

// One lane per stream: apply's clock, changeBg, filterFg's sudden_change, updateBg and createBg's tail (imbs.cpp:181-236, :424-433, :709-724)
__global__ void imbs_control_kernel(const ImbsArgs a, int count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  ImbsCtl c = a.ctl[k];
  const bool gate = (a.model[(size_t)k * a.M * a.n] & kImbsValid) != 0;
  c.prev_ts = c.ts;
  c.ts = c.ts + a.step;
  if (c.sudden && !c.bg_reset) {  // changeBg
    c.ns = (uint32_t)(c.ns / 3.);
    c.sp = (uint32_t)(c.sp / 2.);
    c.bfc = 0, c.bg_reset = 1;
  }
  if (gate && (double)c.count255 > a.n * 0.5) c.sudden = 1;  // filterFg
  c.count255 = 0;
  // updateBg
  if (c.bg_reset && c.bfc > c.ns - 1) c.bfc = c.ns - 1;
  if ((double)c.pbft > c.ts) c.pbft = (unsigned long long)c.ts;
  c.plan = 0, c.plan_ns = c.ns;
  bool built = false;
  if (c.bfc == c.ns - 1) {
    c.plan = 1, c.plan_k = c.bfc, built = true;  // the last sample is used twice: bgSample is the previous frame's
    c.bfc = 0;
  } else if ((c.ts - (double)c.pbft) >= (double)c.sp) {
    c.pbft = (unsigned long long)c.ts;
    c.plan = 3, c.plan_k = c.bfc;
    c.bfc++;
  }
  if (built) {  // createBg's tail
    const bool shrunk = c.bg_reset != 0;
    c.bg_reset = 0;
    if (c.sudden) {
      // a sudden change first seen on a build frame finds numSamples undivided; the reference then triples it past its arrays.
      // The engine restores only what changeBg divided.
      if (shrunk) c.ns = (uint32_t)(c.ns * 3.), c.sp = (uint32_t)(c.sp * 2.);
      c.sudden = 0;
    }
  }
  a.ctl[k] = c;
}

// createBg(plan_k) (imbs.cpp:295-446); fgmask is `lab` (all zero on a frame that did not detect)
__global__ __launch_bounds__(kBlock) void imbs_sample_kernel(const ImbsArgs a) {
  const size_t k = blockIdx.y, n = a.n;
  const ImbsCtl& c = a.ctl[k];
  if (!(c.plan & 1)) return;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t bk = c.plan_k, ns = c.plan_ns;
  uint32_t px;
  if (c.plan & 2) px = imbs_pixel(a.cur, k * n + p), a.smp[k * n + p] = px;
  else px = a.smp[k * n + p];
  const int fgv = a.lab[k * n + p];
  uint32_t* bins = a.bins + k * a.cap * n + p;
  uint32_t* model = a.model + k * a.M * n + p;
  const uint32_t nsc = min(ns, a.cap);  // the reference's arrays hold `cap` slots
  if (bk == 0) {
    bins[0] = px | (1u << 24) | (fgv == 255 ? kImbsFg : 0u);
    for (uint32_t s = 1; s < nsc; ++s) bins[s * n] &= ~kImbsCount;  // binHeights[s] = 0; values and isFg stay
  } else {
    const uint32_t lim = min(bk, a.cap);
    for (uint32_t s = 0; s < lim; ++s) {
      uint32_t w = bins[s * n];
      const uint32_t h = (w >> 24) & 0x3fu;
      if ((uint32_t)imbs_dist(w, px) <= a.assoc) {
        const uint32_t den = h + 1;
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) v |= (((uint32_t)byte_of(w, j) * h + (uint32_t)byte_of(px, j)) / den) << (8 * j);
        w = v | (min(h + 1, 63u) << 24) | (w & kImbsFg);
        if (fgv == 255) w |= kImbsFg;
        bins[s * n] = w;
        break;
      } else if (h == 0) {
        bins[s * n] = px | (1u << 24) | (fgv == 255 ? kImbsFg : 0u);
        break;
      }
    }
    if (bk == ns - 1) {  // build the model
      uint32_t index = 0;
      int max_height = -1;
      for (uint32_t s = 0; s < nsc; ++s) {
        uint32_t w = bins[s * n];
        const int h = (int)((w >> 24) & 0x3fu);
        if (h == 0) {
          if (index < a.M) model[index * n] &= ~kImbsValid;
          break;
        }
        if (index == a.M) break;
        if ((uint32_t)h >= a.min_bin) {
          if (fgv == 180) {
            for (uint32_t m = 0; m < a.M; ++m) {
              const uint32_t mw = model[m * n];
              if (!(mw & kImbsValid)) break;
              if ((uint32_t)imbs_dist(mw, w) < a.fg_thr) {
                model[m * n] = mw & ~kImbsFg;
                w &= ~kImbsFg;
                bins[s * n] = w;
              }
            }
          }
          const uint32_t entry = (w & 0x00ffffffu) | ((uint32_t)h << 24) | kImbsValid | (w & kImbsFg);
          if (h > max_height) {
            max_height = h;
            model[index * n] = model[0] | kImbsValid;  // slot 0 moves to `index`, the taller bin takes slot 0
            model[0] = entry;
          } else {
            model[index * n] = entry;
          }
          ++index;
        }
      }
    }
  }
  if (bk == ns - 1) {
    a.persist[k * n + p] = 0;
    a.bgimg[k * n + p] = model[0] & 0x00ffffffu;
  }
}

// what apply and getBackgroundImage hand out: zero images (the banner without its text) until bgModel[0].isValid[0]
__global__ __launch_bounds__(kBlock) void imbs_out_kernel(const ImbsArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const size_t k = blockIdx.y, n = a.n;
  if (p >= n) return;
  const bool gate = (a.model[k * a.M * n] & kImbsValid) != 0;
  const size_t g = k * n + p;
  if (a.fg) a.fg[g] = gate ? a.lab[g] : 0;
  if (a.bgout) {
    const uint32_t v = gate ? a.bgimg[g] : 0u;
    uint8_t* o = a.bgout + g * 3;
    o[0] = (uint8_t)v, o[1] = (uint8_t)(v >> 8), o[2] = (uint8_t)(v >> 16);
  }
}

}  // namespace bgs
