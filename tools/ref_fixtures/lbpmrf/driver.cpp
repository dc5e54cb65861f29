// Fixture driver for the LbpMrf mask stage: the reference's unmodified MotionDetection::GetMotionsMaskHU
// (package_bgs/ck/MotionDetection.cpp:1256-1366) on a background-rate map of the caller's.  MotionDetection.cpp is included as it
// stands, because MEPixelDataType is defined inside it; the build passes -Dprivate=public (README.md here).
//   lm_run   fills HULBPPixelData[x][y]->BackgroundRate, sets the state to ps_Successful, calls GetMotionsMaskHU and returns the mask and
//            the labels the call left in BackgroundRate (0.0 = SINK).
// GetMotionsMaskHU throws the value of Graph::maxflow() away.  The link wraps that symbol (-Wl,--wrap, README.md here): the call inside
// GetMotionsMaskHU lands in __wrap_..., which runs the reference's own maxflow() on the reference's own graph, times it and keeps what
// it returns.
#include "MotionDetection.cpp"

#include <chrono>
#include <cstdint>

static int g_flow, g_calls;
static double g_seconds;

extern "C" int __real__ZN2ck5Graph7maxflowEv(Graph* g);
extern "C" int __wrap__ZN2ck5Graph7maxflowEv(Graph* g) {
  const auto t0 = std::chrono::steady_clock::now();
  g_flow = __real__ZN2ck5Graph7maxflowEv(g);
  g_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  ++g_calls;
  return g_flow;
}

extern "C" int lm_run(int rows, int cols, int area, float weight, const float* rate, uint8_t* mask, uint8_t* labels, int32_t* flow, double* maxflow_seconds) {
  const int hw = cols - area + 1, nh = rows - area + 1, nw = hw / 2;
  if (area < 3 || area % 2 == 0 || nh < 1 || nw < 1 || hw % 2) return 1;
  MotionDetection md(MotionDetection::md_LBPHistograms);
  md.HUHistogramArea = area, md.HUMinCutWeight = weight, md.HUImageWidth = hw, md.HUImageHeight = nh;
  md.HULBPPixelData = new MEPixelDataType**[nw];
  for (int x = 0; x < nw; ++x) {
    md.HULBPPixelData[x] = new MEPixelDataType*[nh];
    for (int y = 0; y < nh; ++y) {
      MEPixelDataType* p = new MEPixelDataType();
      p->BackgroundRate = rate[(size_t)y * nw + x];
      md.HULBPPixelData[x][y] = p;
    }
  }
  md.MDDataState = ps_Successful;

  g_calls = 0;
  MEImage out(16, 16, 3);  // another geometry: the call reallocates it, as the class's own caller makes it do on the first frame
  md.GetMotionsMaskHU(out);
  if (g_calls != 1) return 4;
  *flow = g_flow, *maxflow_seconds = g_seconds;
  if (out.GetWidth() != cols || out.GetHeight() != rows || out.GetLayers() != 1) return 2;
  for (int y = 0; y < rows; ++y) memcpy(mask + (size_t)y * cols, out.GetImageData() + (size_t)y * out.GetRowWidth(), cols);
  for (int x = 0; x < nw; ++x) {
    for (int y = 0; y < nh; ++y) {
      const float r = md.HULBPPixelData[x][y]->BackgroundRate;
      if (r != 0.0f && r != 1.0f) return 3;
      labels[(size_t)y * nw + x] = r == 0.0f;
      delete md.HULBPPixelData[x][y];
    }
    delete[] md.HULBPPixelData[x];
  }
  delete[] md.HULBPPixelData;
  md.HULBPPixelData = NULL;
  md.MDMode = MotionDetection::md_NotDefined;  // nothing of the class's own allocation exists: the destructor has nothing to release
  return 0;
}
