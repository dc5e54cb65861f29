// host_rows.h — the row arithmetic of the host path (host_path.h): how a frame is split into bands, and the copies between a caller's
// image (any row step) and a dense staging image.  No HIP and no state, so it compiles, and is tested, with a plain C++ compiler
// (tests/host_rows_main.cpp).  Needs <cstdint>, <cstddef> and <cstring>; included inside bgs_hip.hip's anonymous namespace.
#pragma once

// A frame crosses the bus in bands, so that the CPU copies band k+1 while the DMA engine moves band k.  Below 64 rows a frame is one band.
struct Band { int y0, y1; };  // rows [y0, y1)
inline int band_count(int rows) { return rows >= 64 ? 8 : 1; }
inline Band band_of(int rows, int bands, int b) { return {(int)((int64_t)rows * b / bands), (int)((int64_t)rows * (b + 1) / bands)}; }

// Where dense row y of a prepared frame comes from in the raw one (bgs_set_ingest's flip and ROI): row y + y0 of the resized frame of
// rh rows, counted from the bottom when flipped, x_bytes into the row.
struct RowMap { bool flip; int rh, y0; size_t x_bytes; };

// rows [y0, y1) of `src` (src_step bytes from row to row) into the dense image (row_bytes from row to row)
inline void pack_rows(uint8_t* dense, const uint8_t* src, size_t src_step, size_t row_bytes, int y0, int y1, const RowMap* map = nullptr) {
  for (int y = y0; y < y1; ++y) {
    size_t sy = (size_t)y, sx = 0;
    if (map) sy = (size_t)(map->flip ? map->rh - 1 - (y + map->y0) : y + map->y0), sx = map->x_bytes;
    std::memcpy(dense + (size_t)y * row_bytes, src + sy * src_step + sx, row_bytes);
  }
}

// rows [y0, y1) of the dense image into `dst` (dst_step bytes from row to row)
inline void unpack_rows(uint8_t* dst, size_t dst_step, const uint8_t* dense, size_t row_bytes, int y0, int y1) {
  for (int y = y0; y < y1; ++y) std::memcpy(dst + (size_t)y * dst_step, dense + (size_t)y * row_bytes, row_bytes);
}

// the same for a one-channel dense image of `cols` columns, every byte written to three equal channels
inline void unpack_rows_gray3(uint8_t* dst, size_t dst_step, const uint8_t* dense, int cols, int y0, int y1) {
  for (int y = y0; y < y1; ++y) {
    uint8_t* d = dst + (size_t)y * dst_step;
    const uint8_t* q = dense + (size_t)y * cols;
    for (int x = 0; x < cols; ++x) d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = q[x];
  }
}
