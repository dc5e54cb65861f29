// frame_history.h — the arithmetic of the frame history ring of FrameDifference (2 slots) and WeightedMovingMean / Variance (3), for the
// engines of those classes and a group's shared ring (FrameHistory in bgs_hip.hip).  No HIP and no state, so it compiles, and is tested,
// with a plain C++ compiler (tests/frame_history_main.cpp).  Needs <cstdint> and <cstring>; included inside bgs_hip.hip's anonymous namespace.
// A stream's frames go round the `nring` slots: the one it receives at position `pos` lives in slot pos % nring.  The position only counts
// up; `t`, the frames the stream has seen since it (re)started, says how many slots behind `pos` hold frames of its own (bgs_reset_stream
// sets t to 0 and leaves pos alone; a group, which has no reset, passes its frame count for both).
#pragma once
constexpr int kNoSlot = -1;

// the slot that takes the frame received at `pos`
inline int history_cur(int nring, int64_t pos) { return (int)(pos % nring); }

// The slot of the k-th last frame before `pos`, k = 1, 2; kNoSlot while the stream has not seen it (warm-up) or when the ring does
// not keep it (2 slots: k = 2).  Before a frame is processed these are the kernel's h1 / h2, after it the planes prev1 / prev2.
inline int history_prev(int nring, int64_t pos, int64_t t, int k) { return (k < nring && t >= k) ? (int)((pos + nring - k) % nring) : kNoSlot; }

// the slot a state plane names, kNoSlot for every other plane
inline int history_plane(int nring, int64_t pos, int64_t t, const char* plane) {
  return !std::strcmp(plane, "prev1") ? history_prev(nring, pos, t, 1) : !std::strcmp(plane, "prev2") ? history_prev(nring, pos, t, 2) : kNoSlot;
}

// A clip call reads its history from the clip's own frames and writes no slot while it runs.  After `done` frames of a clip that
// started at `pos0`: the copies (clip frame -> slot, at most nring - 1 of them; older frames are in the ring already) that leave every
// slot history_prev can name as `done` per-frame calls would have.  Returns their number.
struct HistoryCopy { int frame, slot; };
inline int history_clip_plan(int nring, int64_t pos0, int done, HistoryCopy out[2]) {
  int n = 0;
  for (int k = 1; k < nring && k <= done; ++k) out[n++] = {done - k, (int)((pos0 + done - k) % nring)};
  return n;
}
