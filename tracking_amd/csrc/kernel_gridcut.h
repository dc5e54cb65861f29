// kernel_gridcut.h — the exact minimum cut of LbpMrf's node grid (package_bgs/ck/MotionDetection.cpp:1279-1318) and the
// mask the class paints from it (:1322-1342).
//
// The problem.  Node (x, y) of an nh x nw grid has source capacity 1 and sink capacity t = (short)(w * (1 - rate)); edges of capacity 1
// each way join (x, y) to (x-1, y) and (x, y-1), only where x > 0 and y > 0.  The class reads what_segment(): SOURCE iff the node is
// reachable from the source in the residual graph of a maximum flow - the same set for every maximum flow.
//
// The route.  Push-relabel on the REVERSED problem (source and sink swapped; the edges are symmetric), as a preflow: a node starts with
// excess t - 1 (set_tweights' cancellation); a negative excess is a reversed sink with that much room.  Under a maximum preflow "can reach
// a reversed sink with room" is exactly the reference's SOURCE set, and the call ends with an exact breadth-first relabelling towards
// those sinks, so the labels are simply "height is finite".  Whatever order the waves pushed in, the call is DONE only in a state where
// (a) the heights are the exact distances (a BFS launch changed nothing) and (b) no node with excess has a finite height - no augmenting
// path is left, the preflow is maximum, and the finite heights are the canonical set.  Everything is integer arithmetic.
//
// No grid-wide wait.  The host enqueues a fixed budget of gc_step_kernel launches (gridcut.h); launch k works out its phase from what launch
// k - 1 left in `ctl` (stream order makes that final): RESET (heights 0 at sinks with room, infinite elsewhere), BFS (relax the heights,
// kGcIters times per node; "changed" flag), PUSH (the lock-free push / relabel step of Hong, kGcIters times per node, kGcPushLaunches
// launches), DONE (every block returns at once).  Within a launch nodes read each other's words with agent-scope atomic loads: a stale
// read only delays a monotone relaxation, and in PUSH every word has one writer per direction (a node alone lowers its own excess, its
// own outgoing residuals and raises its own height), which is what Hong's argument needs.  Every loop has a constant trip count.
#pragma once
#include "bgs_device.h"
#include "gridcut.h"

namespace bgs {

constexpr int kGcInf = 1 << 29;
constexpr int kGcBX = 32, kGcBY = 8;  // a workgroup's tile of nodes
enum { kGcReset = 0, kGcBfs = 1, kGcPush = 2, kGcDone = 3 };

__device__ __forceinline__ int gc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gc_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int gc_add(int* p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (short)(w * (1 - r)) in float arithmetic, truncated toward zero, clamped to [0, 32767] (NaN: 0)
__device__ __forceinline__ int gc_sink_weight(float w, float r) {
  const float v = w * (1.0f - r);
  return v >= 32767.0f ? 32767 : (v > 0.0f ? (int)v : 0);
}

// the state of launch k from launch k - 1's: phase in bits 0-3, PUSH launches left in the bits above
__device__ __forceinline__ int gc_next_state(const int* ctl, int budget, int k) {
  if (k == 0) return kGcReset;
  const int prev = ctl[k - 1], phase = prev & 15, left = prev >> 4;
  if (phase == kGcReset) return kGcBfs;
  if (phase == kGcBfs) return ctl[budget + k - 1] ? kGcBfs : (ctl[2 * budget + k - 1] ? (kGcPush | (kGcPushLaunches << 4)) : kGcDone);
  if (phase == kGcPush) return left > 1 ? (kGcPush | ((left - 1) << 4)) : kGcReset;
  return kGcDone;
}

__global__ __launch_bounds__(kGcBX* kGcBY) void gc_init_kernel(const GcArgs a) {
  const int x = blockIdx.x * kGcBX + threadIdx.x, y = blockIdx.y * kGcBY + threadIdx.y;
  if (x >= a.nw || y >= a.nh) return;
  const size_t u = ((size_t)blockIdx.z * a.nh + y) * a.nw + x;
  a.excess[u] = gc_sink_weight(a.weight, a.rate[u]) - 1;
  a.height[u] = kGcInf;
  a.resid[u] = (x > 0 && y > 0) ? (1 | (1 << 2)) : 0;
}

// one node's share of launch k in the given phase (RESET, BFS or PUSH)
__device__ __forceinline__ void gc_node(const GcArgs& a, int phase, int k, int x, int y, int img) {
  const size_t u = ((size_t)img * a.nh + y) * a.nw + x;
  int* const ex = a.excess + u;
  int* const hu = a.height + u;
  int* const ru = a.resid + u;
  if (phase == kGcReset) {
    *hu = *ex < 0 ? 0 : kGcInf;
    return;
  }
  // the four neighbours: left and up exist where x > 0 and y > 0; right is the right node's left edge, down the lower node's up edge
  const bool hasL = x > 0 && y > 0, hasU = hasL, hasR = y > 0 && x + 1 < a.nw, hasD = x > 0 && y + 1 < a.nh;
  const ptrdiff_t oL = -1, oU = -(ptrdiff_t)a.nw, oR = 1, oD = a.nw;
  if (phase == kGcBfs) {
    // residuals stand still during a BFS phase
    const int w = *ru;
    const bool rL = hasL && (w & 3) > 0, rU = hasU && ((w >> 2) & 3) > 0;
    const bool rR = hasR && (ru[oR] & 3) < 2, rD = hasD && ((ru[oD] >> 2) & 3) < 2;
    int h = *hu;
    bool changed = false;
    if (h != 0 && (rL || rU || rR || rD)) {
      for (int it = 0; it < kGcIters; ++it) {
        int best = kGcInf;
        if (rL) best = min(best, gc_ld(hu + oL));
        if (rU) best = min(best, gc_ld(hu + oU));
        if (rR) best = min(best, gc_ld(hu + oR));
        if (rD) best = min(best, gc_ld(hu + oD));
        if (best + 1 < h) {
          h = best + 1;
          gc_st(hu, h);
          changed = true;
        }
      }
    }
    if (changed) a.ctl[a.budget + k] = 1;
    if (*ex > 0 && h < kGcInf) a.ctl[2 * a.budget + k] = 1;
    return;
  }
  // PUSH: Hong's lock-free step.  Only this thread lowers *ex, lowers the residuals out of u and writes *hu.
  for (int it = 0; it < kGcIters; ++it) {
    const int e = gc_ld(ex);
    if (e <= 0) continue;
    const int h = gc_ld(hu);
    if (h >= kGcInf) continue;
    int best = kGcInf, dir = -1, cap = 0;
    if (hasL || hasU) {
      const int w = gc_ld(ru);
      if (hasL && (w & 3) > 0) {
        const int hv = gc_ld(hu + oL);
        if (hv < best) best = hv, dir = 0, cap = w & 3;
      }
      if (hasU && ((w >> 2) & 3) > 0) {
        const int hv = gc_ld(hu + oU);
        if (hv < best) best = hv, dir = 1, cap = (w >> 2) & 3;
      }
    }
    if (hasR) {
      const int c = 2 - (gc_ld(ru + oR) & 3);
      if (c > 0) {
        const int hv = gc_ld(hu + oR);
        if (hv < best) best = hv, dir = 2, cap = c;
      }
    }
    if (hasD) {
      const int c = 2 - ((gc_ld(ru + oD) >> 2) & 3);
      if (c > 0) {
        const int hv = gc_ld(hu + oD);
        if (hv < best) best = hv, dir = 3, cap = c;
      }
    }
    if (dir < 0 || best >= kGcInf) {  // nowhere to go until the next exact relabelling says otherwise
      gc_st(hu, kGcInf);
      continue;
    }
    if (h > best) {
      const int d = min(e, cap);
      if (dir == 0) gc_add(ru, -d), gc_add(ex + oL, d);
      else if (dir == 1) gc_add(ru, -(d << 2)), gc_add(ex + oU, d);
      else if (dir == 2) gc_add(ru + oR, d), gc_add(ex + oR, d);
      else gc_add(ru + oD, d << 2), gc_add(ex + oD, d);
      gc_add(ex, -d);
    } else {
      gc_st(hu, best + 1);
    }
  }
}

// The grid is capped (kGcMaxBlocks workgroups, each walking its tiles with the grid's stride), so the launches behind DONE cost what a
// few thousand empty workgroups cost, whatever the batch.  Nothing waits for another workgroup, resident or not.
constexpr unsigned kGcMaxBlocks = 2048;

__global__ __launch_bounds__(kGcBX* kGcBY) void gc_step_kernel(const GcArgs a, int k, unsigned tiles_x, unsigned tiles_y, size_t tiles) {
  __shared__ int s_state;
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const int st = gc_next_state(a.ctl, a.budget, k);
    s_state = st;
    if (blockIdx.x == 0) {
      a.ctl[k] = st;
      if ((st & 15) == kGcDone && k > 0 && (a.ctl[k - 1] & 15) != kGcDone) a.stats[1] = (unsigned long long)k;
    }
  }
  __syncthreads();
  const int phase = s_state & 15;
  if (phase == kGcDone) return;
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned tx = (unsigned)(tile % tiles_x), ty = (unsigned)((tile / tiles_x) % tiles_y), img = (unsigned)(tile / ((size_t)tiles_x * tiles_y));
    const int x = tx * kGcBX + threadIdx.x, y = ty * kGcBY + threadIdx.y;
    if (x < a.nw && y < a.nh) gc_node(a, phase, k, x, y, (int)img);
  }
}

// labels (1 = SINK: no finite height), the count of sinks left with room, and the sticky counter when the budget was not enough
__global__ __launch_bounds__(kGcBX* kGcBY) void gc_finish_kernel(const GcArgs a) {
  const int x = blockIdx.x * kGcBX + threadIdx.x, y = blockIdx.y * kGcBY + threadIdx.y;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0 && threadIdx.y == 0;
  if (first && (a.ctl[a.budget - 1] & 15) != kGcDone) {  // the last launch still worked: was it the BFS launch that proved the end?
    if ((gc_next_state(a.ctl, a.budget, a.budget) & 15) != kGcDone) atomicAdd(a.stats, 1ull);
    a.stats[1] = (unsigned long long)a.budget;
  }
  bool neg = false;
  if (x < a.nw && y < a.nh) {
    const size_t u = ((size_t)blockIdx.z * a.nh + y) * a.nw + x;
    a.labels[u] = a.height[u] < kGcInf ? 0 : 1;
    neg = a.excess[u] < 0;
  }
  const int c = __syncthreads_count(neg);
  if (threadIdx.x == 0 && threadIdx.y == 0 && c) atomicAdd(a.negatives + blockIdx.z, c);
}

__global__ __launch_bounds__(kBlock) void gc_flow_kernel(const int* negatives, int* flow, int images, int nodes) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < images) flow[i] = nodes - negatives[i];
}

// :1322-1342.  Node row y lands on image row y + area - area / 2, column x of the doubled grid on image column x + area / 2.
__global__ __launch_bounds__(kBlock) void lm_node_mask_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ mask, int rows, int cols, int area, int nh, int nw) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (size_t)rows * cols) return;
  const int y = (int)(p / cols) - (area - area / 2), x = (int)(p % cols) - area / 2;
  const uint8_t* sink = labels + (size_t)blockIdx.z * nh * nw;
  bool v = false;
  if (y >= 0 && y < nh && x >= 0 && x < 2 * nw) {
    const int n = x / 2;
    if (y % 2 == (x + 1) % 2) {
      v = sink[(size_t)y * nw + n] != 0;
    } else {
      int c = 0;
      if (x > 1) c += sink[(size_t)y * nw + n - 1];
      if (x < cols - area - 1) c += sink[(size_t)y * nw + n + 1];
      if (y > 0) c += sink[(size_t)(y - 1) * nw + n];
      if (y < rows - area) c += sink[(size_t)(y + 1) * nw + n];
      v = c > 1;
    }
  }
  mask[(size_t)blockIdx.z * rows * cols + p] = v ? 255 : 0;
}

__global__ __launch_bounds__(kBlock) void lm_paint_kernel(const uint64_t* __restrict__ reached, uint8_t* __restrict__ dst, int rows, int cols, int W64) {
  const size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (size_t)rows * cols) return;
  const int y = (int)(p / cols), x = (int)(p % cols);
  const uint64_t w = reached[((size_t)blockIdx.z * rows + y) * W64 + (x >> 6)];
  dst[(size_t)blockIdx.z * rows * cols + p] = ((w >> (x & 63)) & 1ull) ? 0 : 255;
}

void gc_solve_launch(const GcArgs& a, hipStream_t s) {
  const dim3 grid((a.nw + kGcBX - 1) / kGcBX, (a.nh + kGcBY - 1) / kGcBY, a.images), block(kGcBX, kGcBY);
  hipLaunchKernelGGL(gc_init_kernel, grid, block, 0, s, a);
  const size_t tiles = (size_t)grid.x * grid.y * grid.z;
  const dim3 sgrid((unsigned)(tiles < kGcMaxBlocks ? tiles : kGcMaxBlocks));
  for (int k = 0; k < a.budget; ++k) hipLaunchKernelGGL(gc_step_kernel, sgrid, block, 0, s, a, k, grid.x, grid.y, tiles);
  hipLaunchKernelGGL(gc_finish_kernel, grid, block, 0, s, a);
  if (a.flow) hipLaunchKernelGGL(gc_flow_kernel, dim3((a.images + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const int*)a.negatives, a.flow, a.images, a.nh * a.nw);
}

void lm_node_mask_launch(const uint8_t* labels, uint8_t* mask, int images, int rows, int cols, int area, int nh, int nw, hipStream_t s) {
  const dim3 grid((unsigned)(((size_t)rows * cols + kBlock - 1) / kBlock), 1, images);
  hipLaunchKernelGGL(lm_node_mask_kernel, grid, dim3(kBlock), 0, s, labels, mask, rows, cols, area, nh, nw);
}

void lm_paint_launch(const uint64_t* reached, uint8_t* dst, int images, int rows, int cols, int W64, hipStream_t s) {
  const dim3 grid((unsigned)(((size_t)rows * cols + kBlock - 1) / kBlock), 1, images);
  hipLaunchKernelGGL(lm_paint_kernel, grid, dim3(kBlock), 0, s, reached, dst, rows, cols, W64);
}

}  // namespace bgs
