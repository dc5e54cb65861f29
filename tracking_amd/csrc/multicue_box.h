// multicue_box.h — what the host side of the box stage of SJN_MultiCueBGS (engine_multicue.h) sees of
// kernel_multicue_box.h: the argument block and one call that enqueues the stage's three launches.  The kernels themselves are compiled in
// bgs_multicue_box.hip, a translation unit of their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bgs {

constexpr int kMcMaxBoxes = 300;   // BGS_MULTICUE_MAX_BOXES, the reference's iElementNum (:175)
constexpr int kMcBoxFields = 13;   // BGS_MULTICUE_BOX_FIELDS

struct McBoxArgs {
  const uint8_t* landmark;  // [S][n]
  const uint8_t* frames;    // [S][rows][cols][3]
  uint8_t* fore0;           // [S][n] scratch: the foreground map before any removal
  uint8_t* grey;            // [S][n] scratch: grey of the nearest-neighbour reduced frame
  uint8_t *fore, *ghost, *update;  // [S][n] outputs
  int* count;               // [S]
  int* boxes;               // [S][kMcMaxBoxes][kMcBoxFields]
  unsigned long long* box_overflow;
  int rows, cols, rw, rh;
  double inv_fy, inv_fx;    // 1.0 / ((double)rh / rows), 1.0 / ((double)rw / cols): cvResize's nearest-neighbour factors
  double fh, fw;            // (double)rows / rh, (double)cols / rw: SetBoundingBox's
};

// mc_box_prepare_kernel, mc_box_label_kernel and mc_box_verify_kernel over `streams` streams, asynchronous on s
void mc_box_launch(const McBoxArgs& a, unsigned streams, hipStream_t s);

}  // namespace bgs
