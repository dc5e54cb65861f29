// gridcut.h — what the host side of the LbpMrf mask stage (bgs_lbpmrf_mask_device in bgs_hip.hip) sees of
// kernel_gridcut.h: the argument block, the launch budget and the calls that enqueue the stage's own launches.  The kernels themselves are
// compiled in bgs_gridcut.hip, a translation unit of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bgs {

constexpr int kGcIters = 32;        // relaxations (BFS) or push / relabel steps (PUSH) of a node per launch
constexpr int kGcPushLaunches = 6;  // PUSH launches between two exact relabellings
constexpr int kGcMaxLaunches = 2048;

// The fixed number of gc_step_kernel launches a call enqueues.  A round is 1 RESET + b BFS + kGcPushLaunches PUSH launches; a BFS launch
// moves every label's wavefront by at least one node (kGcIters inside a wave), a PUSH launch moves a unit of excess by at least one edge
// along exact labels.  256 launches cover the rounds every measured input needed many times over; the second term lets a label or a unit
// cross the grid's half perimeter a few times.  Nothing waits for more: what is not DONE after the budget raises the sticky counter.
inline int gc_launch_budget(int nh, int nw) {
  const int n = 256 + (nh + nw) / 4;
  return n < kGcMaxLaunches ? n : kGcMaxLaunches;
}

struct GcArgs {
  const float* rate;  // [images][nh][nw]
  int* excess;        // [images][nh][nw] the reversed problem's excess: t - 1 at first; below 0 = a sink that still has room
  int* height;        // [images][nh][nw] distance label towards a sink with room; kGcInf = none
  int* resid;         // [images][nh][nw] bits 0-1: residual of (node -> left), bits 2-3: of (node -> up); the opposite directions are 2 - these
  int* ctl;           // [3][budget] state, changed, active per launch
  uint8_t* labels;    // [images][nh][nw] 1 = SINK
  int* negatives;     // [images] sinks left with room: flow = nodes - negatives
  int* flow;          // [images] or NULL
  unsigned long long* stats;  // [0] sticky "did not converge" counter, [1] launches the last call used
  int images, nh, nw, budget;
  float weight;
};

// bytes of ctl
inline size_t gc_ctl_bytes(int budget) { return (size_t)3 * budget * sizeof(int); }

// init, `budget` step launches, finish (labels, flow, counter): asynchronous on s.  ctl and negatives must be zero.
void gc_solve_launch(const GcArgs& a, hipStream_t s);
// MotionDetection.cpp:1322-1342: labels -> the node mask u8 [images][rows][cols]
void lm_node_mask_launch(const uint8_t* labels, uint8_t* mask, int images, int rows, int cols, int area, int nh, int nw, hipStream_t s);
// the hole filling after cvFloodFill(…, 128): 0 where the fill from (0, 0) reached, 255 elsewhere (reached: bit planes [images][rows][W64])
void lm_paint_launch(const uint64_t* reached, uint8_t* dst, int images, int rows, int cols, int W64, hipStream_t s);

}  // namespace bgs
