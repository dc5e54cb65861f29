// frame_history_main.cpp — the slot arithmetic of the frame history ring (tracking_amd/csrc/frame_history.h) against a naive simulation:
// a vector that records which frame number each slot holds.  A stand-alone program built with -fsanitize=address,undefined by
// tests/test_frame_history_cpu.py.  Prints one line per failed check and returns their number.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../tracking_amd/csrc/frame_history.h"

static int failures = 0, checks = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    ++checks;                               \
    if (!(cond)) {                          \
      ++failures;                           \
      std::printf("FAILED %s: ", #cond);    \
      std::printf(__VA_ARGS__);             \
      std::printf("\n");                    \
    }                                       \
  } while (0)

// One stream of one ring.  Frames are numbered by the stream's own age (frame t is the one it receives after having seen t); a slot
// that never took a frame of this life of the stream holds a number below zero, different for every slot.
struct Sim {
  int nring;
  int64_t pos, t;
  std::vector<int64_t> slot;
  // a stream at position pos0 that has seen t0 frames since its restart: it received them at positions pos0 - t0 .. pos0 - 1
  // (shifted by 6, a multiple of both ring sizes, where that would be negative: only pos % nring matters)
  Sim(int nring_, int64_t pos0, int64_t t0) : nring(nring_), pos(pos0), t(t0), slot((size_t)nring_) {
    for (int i = 0; i < nring; ++i) slot[(size_t)i] = -100 - i;
    for (int64_t j = 0; j < t0; ++j) slot[(size_t)((pos0 - t0 + j + 6) % nring)] = j;
  }
  void step() { slot[(size_t)(pos % nring)] = t, ++pos, ++t; }  // what a per-frame call does: keep the frame, move on
};

// `s` names the slot that holds frame `want`, or none when the ring cannot hold it (before the stream's first frames; two slots keep one)
static void check_names(const Sim& sim, int s, int64_t want, int k, const char* what) {
  const bool exists = want >= 0 && k < sim.nring;
  if (!exists)
    CHECK(s == kNoSlot, "%s: nring %d pos %lld t %lld names slot %d, there is no such frame", what, sim.nring, (long long)sim.pos, (long long)sim.t, s);
  else
    CHECK(s >= 0 && s < sim.nring && sim.slot[(size_t)s] == want, "%s: nring %d pos %lld t %lld names slot %d, frame %lld expected there", what, sim.nring,
          (long long)sim.pos, (long long)sim.t, s, (long long)want);
}

static void check_planes(const Sim& sim) {  // prev1 / prev2: frames t-1 and t-2 of a stream that has seen t
  check_names(sim, history_plane(sim.nring, sim.pos, sim.t, "prev1"), sim.t - 1, 1, "prev1");
  check_names(sim, history_plane(sim.nring, sim.pos, sim.t, "prev2"), sim.t - 2, 2, "prev2");
  CHECK(history_plane(sim.nring, sim.pos, sim.t, "bg") == kNoSlot && history_plane(sim.nring, sim.pos, sim.t, "prev") == kNoSlot, "another plane names a slot");
}

// `steps` per-frame calls: before each, h1 / h2 name frames t-1 / t-2; the frame goes where the simulation keeps it; after each, the planes
static void check_steps(Sim& sim, int steps) {
  check_planes(sim);
  for (int i = 0; i < steps; ++i) {
    const int cur = history_cur(sim.nring, sim.pos);
    const int h1 = history_prev(sim.nring, sim.pos, sim.t, 1), h2 = history_prev(sim.nring, sim.pos, sim.t, 2);
    CHECK(cur >= 0 && cur < sim.nring && cur != h1 && cur != h2, "the current frame's slot %d is out of range or one of its history's (%d, %d)", cur, h1, h2);
    check_names(sim, h1, sim.t - 1, 1, "h1");
    check_names(sim, h2, sim.t - 2, 2, "h2");
    const int64_t frame = sim.t;
    sim.step();
    CHECK(sim.slot[(size_t)cur] == frame, "frame %lld went to slot %d, the per-frame call keeps it elsewhere", (long long)frame, cur);
    check_planes(sim);
  }
}

// `done` frames of a clip: the planned copies against `done` per-frame steps.  Every slot a later call can name (history_prev at the
// position and age after the clip, k = 1 .. nring - 1) holds the same frame; the one slot left over is the one the NEXT frame
// overwrites before anything reads it, so per-frame calls leave an older frame there that the clip need not copy.
static void check_clip(int nring, int64_t pos0, int64_t t0, int nframes, int done) {
  Sim frames(nring, pos0, t0), clip(nring, pos0, t0);
  for (int i = 0; i < done; ++i) frames.step();
  HistoryCopy plan[2];
  const int n = history_clip_plan(nring, pos0, done, plan);
  CHECK(n >= 0 && n <= nring - 1 && n <= done, "nring %d done %d: %d copies", nring, done, n);
  for (int i = 0; i < n; ++i) {
    CHECK(plan[i].frame >= 0 && plan[i].frame < done && plan[i].slot >= 0 && plan[i].slot < nring, "copy %d: clip frame %d of %d (%d done) to slot %d", i, plan[i].frame, nframes, done, plan[i].slot);
    if (plan[i].slot >= 0 && plan[i].slot < nring) clip.slot[(size_t)plan[i].slot] = t0 + plan[i].frame;
  }
  clip.pos += done, clip.t += done;
  const int next = history_cur(nring, clip.pos);
  for (int s = 0; s < nring; ++s)
    CHECK(s == next || clip.slot[(size_t)s] == frames.slot[(size_t)s], "nring %d pos0 %lld t0 %lld, %d of %d frames: slot %d holds frame %lld, per-frame calls leave %lld", nring,
          (long long)pos0, (long long)t0, done, nframes, s, (long long)clip.slot[(size_t)s], (long long)frames.slot[(size_t)s]);
  check_steps(clip, 2);  // and the calls after the clip find their history
}

int main() {
  for (int nring : {2, 3})
    for (int64_t pos0 = 0; pos0 <= 5; ++pos0)
      for (int64_t t0 = 0; t0 <= 4; ++t0) {  // pos0 != t0: a stream after a reset (or, for t0 > pos0, positions that wrapped)
        for (int steps = 1; steps <= 9; ++steps) {
          Sim sim(nring, pos0, t0);
          check_steps(sim, steps);
        }
        for (int nframes = 1; nframes <= 9; ++nframes)
          for (int done = 0; done <= nframes; ++done) check_clip(nring, pos0, t0, nframes, done);
      }
  std::printf("%d checks, %d checks failed\n", checks, failures);
  return failures ? 1 : 0;
}
