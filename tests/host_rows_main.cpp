// host_rows_main.cpp — the row functions of the host path (tracking_amd/csrc/host_rows.h) against naive loops, as a stand-alone program
// built with -fsanitize=address,undefined by tests/test_host_rows_cpu.py: an out-of-bounds row is the sanitizer's to report, a wrong
// byte this program's.  Prints one line per failed check and returns their number.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../tracking_amd/csrc/host_rows.h"

static int failures = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      ++failures;                           \
      std::printf("FAILED %s: ", #cond);    \
      std::printf(__VA_ARGS__);             \
      std::printf("\n");                    \
    }                                       \
  } while (0)

static const uint8_t kGuard = 0xA5;

// a strided image whose byte at (y, x) is a function of both, with kGuard in the padding of every row
static std::vector<uint8_t> source(int rows, size_t row, size_t step) {
  std::vector<uint8_t> v((size_t)rows * step, kGuard);
  for (int y = 0; y < rows; ++y)
    for (size_t x = 0; x < row; ++x) v[(size_t)y * step + x] = (uint8_t)(y * 31 + x * 7 + 1);
  return v;
}

static void check_bands() {
  for (int rows : {1, 7, 63, 64, 67, 1080}) {
    const int bands = band_count(rows);
    CHECK(bands == (rows >= 64 ? 8 : 1), "rows %d: %d bands", rows, bands);
    int next = 0;
    for (int b = 0; b < bands; ++b) {
      const Band k = band_of(rows, bands, b);
      CHECK(k.y0 == next && k.y1 >= k.y0, "rows %d band %d is [%d, %d), expected to start at %d", rows, b, k.y0, k.y1, next);
      next = k.y1;
    }
    CHECK(next == rows, "rows %d: the bands end at %d", rows, next);
  }
}

// pack band by band into a dense image with `guard` bytes of kGuard before and after it
static void check_pack(int src_rows, int src_cols, int ch, int rows, int cols, const RowMap* map, const char* what) {
  const size_t src_row = (size_t)src_cols * ch, step = src_row + 5, rb = (size_t)cols * ch, guard = 64;
  const std::vector<uint8_t> src = source(src_rows, src_row, step);
  std::vector<uint8_t> buf(guard + (size_t)rows * rb + guard, kGuard);
  uint8_t* dense = buf.data() + guard;
  const int bands = band_count(rows);
  for (int b = 0; b < bands; ++b) {
    const Band k = band_of(rows, bands, b);
    pack_rows(dense, src.data(), step, rb, k.y0, k.y1, map);
  }
  for (int y = 0; y < rows; ++y) {
    const int sy = map ? (map->flip ? map->rh - 1 - (y + map->y0) : y + map->y0) : y;
    const size_t sx = map ? map->x_bytes : 0;
    for (size_t x = 0; x < rb; ++x)
      if (dense[(size_t)y * rb + x] != src[(size_t)sy * step + sx + x]) {
        CHECK(false, "%s: byte (%d, %zu) is %d, source row %d has %d", what, y, x, dense[(size_t)y * rb + x], sy, src[(size_t)sy * step + sx + x]);
        return;
      }
  }
  for (size_t i = 0; i < guard; ++i) CHECK(buf[i] == kGuard && buf[guard + (size_t)rows * rb + i] == kGuard, "%s: guard byte %zu overwritten", what, i);
}

// unpack band by band into a padded destination; channels 3 = the gray image written to three equal channels
static void check_unpack(int rows, int cols, int out_ch, const char* what) {
  const size_t rb = (size_t)cols, out_row = rb * out_ch, step = out_row + 9;
  const std::vector<uint8_t> dense = source(rows, rb, rb);
  std::vector<uint8_t> dst((size_t)rows * step, kGuard);
  const int bands = band_count(rows);
  for (int b = 0; b < bands; ++b) {
    const Band k = band_of(rows, bands, b);
    if (out_ch == 1)
      unpack_rows(dst.data(), step, dense.data(), rb, k.y0, k.y1);
    else
      unpack_rows_gray3(dst.data(), step, dense.data(), cols, k.y0, k.y1);
  }
  for (int y = 0; y < rows; ++y) {
    for (size_t x = 0; x < out_row; ++x) CHECK(dst[(size_t)y * step + x] == dense[(size_t)y * rb + x / out_ch], "%s: byte (%d, %zu)", what, y, x);
    for (size_t x = out_row; x < step; ++x) CHECK(dst[(size_t)y * step + x] == kGuard, "%s: padding byte (%d, %zu) overwritten", what, y, x);
  }
}

int main() {
  check_bands();
  for (int rows : {1, 7, 63, 64, 67}) check_pack(rows, 53, 3, rows, 53, nullptr, "pack");
  // a 40 x 31 window at (3, 5) of a 67-row frame
  const RowMap roi{false, 67, 5, 3 * 3}, flip{true, 67, 0, 0}, both{true, 67, 5, 3 * 3};
  check_pack(67, 53, 3, 31, 40, &roi, "pack, ROI");
  check_pack(67, 53, 3, 67, 53, &flip, "pack, flip");
  check_pack(67, 53, 3, 31, 40, &both, "pack, flip and ROI");
  for (int rows : {7, 67}) {
    check_unpack(rows, 53, 1, "unpack");
    check_unpack(rows, 53, 3, "unpack to three channels");
  }
  std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
