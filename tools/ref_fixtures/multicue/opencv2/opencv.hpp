// Stand-in for <opencv2/opencv.hpp>: the part of OpenCV 2.4 that package_bgs/sjn/SJN_MultiCueBGS.{h,cpp} names, written for the
// fixture generator (README.md here).  The model stage calls cvCreateImage / cvReleaseImage, the two cv::Mat <->
// IplImage constructors of SJN_MultiCueBGS.cpp:523-528 and cv::GaussianBlur(7 x 7, sigma 0.7) on 8-bit data; the blur is DEFINED
// here as OpenCV 2.4's 8-bit fixed-point filter (integer taps lrintf(k * 256), exact row pass, column pass (sum + 2^15) >> 16,
// BORDER_REFLECT_101).  The box stage adds cvSetImageROI / cvResetImageROI, cvResize (nearest neighbour and
// bilinear), cvCvtColor(CV_BGR2GRAY) from a region of interest and cvCanny, each DEFINED here as DESIGN.md 5.14 states it (recalled
// from OpenCV 2.4, unpinned); every cvCanny call is kept in standInCannyLog() for the driver.  The file storage and imshow abort.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned char uchar;

#define IPL_DEPTH_8U 8
#define CV_BGR2GRAY 6
#define CV_INTER_NN 0
#define CV_INTER_LINEAR 1
#define CV_STORAGE_READ 0
#define CV_STORAGE_WRITE 1

[[noreturn]] inline void cvStandInAbort(const char* what) {
  fprintf(stderr, "opencv stand-in: %s is not on the driven path\n", what);
  abort();
}

struct CvSize { int width, height; };
struct CvRect { int x, y, width, height; };
struct CvScalar { double val[4]; };
struct CvFileStorage;
namespace cv { class Mat; }

struct IplImage {
  int nChannels, depth, width, height, widthStep;
  char* imageData;
  int roiX, roiY, roiW, roiH;  // the region of interest; roiW == 0: none
  IplImage() : nChannels(0), depth(0), width(0), height(0), widthStep(0), imageData(NULL), roiX(0), roiY(0), roiW(0), roiH(0) {}
  IplImage(const cv::Mat& m);  // a header over the matrix's data, as in OpenCV 2.4: nothing is copied
};

inline CvSize cvSize(int w, int h) { CvSize s = {w, h}; return s; }
inline CvRect cvRect(int x, int y, int w, int h) { CvRect r = {x, y, w, h}; return r; }
inline IplImage* cvCreateImage(CvSize s, int depth, int ch) {
  if (depth != IPL_DEPTH_8U) cvStandInAbort("cvCreateImage of another depth");
  IplImage* im = new IplImage;
  im->nChannels = ch, im->depth = depth, im->width = s.width, im->height = s.height;
  im->widthStep = (s.width * ch + 3) & ~3;  // rows padded to 4 bytes
  im->imageData = (char*)calloc((size_t)im->widthStep * s.height + 4, 1);
  return im;
}
inline void cvReleaseImage(IplImage** im) {
  if (!im || !*im) return;
  free((*im)->imageData);
  delete *im;
  *im = NULL;
}
inline CvSize cvGetSize(const IplImage* im) { return cvSize(im->width, im->height); }
inline void cvSetZero(IplImage* im) { memset(im->imageData, 0, (size_t)im->widthStep * im->height); }
inline void cvSetImageROI(IplImage* im, CvRect r) {
  if (r.x < 0 || r.y < 0 || r.width <= 0 || r.height <= 0 || r.x + r.width > im->width || r.y + r.height > im->height) cvStandInAbort("cvSetImageROI outside the image");
  im->roiX = r.x, im->roiY = r.y, im->roiW = r.width, im->roiH = r.height;
}
inline void cvResetImageROI(IplImage* im) { im->roiX = im->roiY = im->roiW = im->roiH = 0; }

inline int standInSatShort(float v) {
  const long r = lrintf(v);
  return (int)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

// cvResize on whole 8-bit images.  CV_INTER_NN: source = min(floor(i * (1.0 / ((double)dst / src))), src - 1).  CV_INTER_LINEAR: 11-bit
// coefficients, and the 2 x 2 mean for an exact 2x reduction (the arithmetic of the project's frame preparation).
inline void cvResize(const IplImage* src, IplImage* dst, int mode = CV_INTER_LINEAR) {
  if (src->roiW || dst->roiW || src->nChannels != dst->nChannels) cvStandInAbort("cvResize with a region of interest or a change of channels");
  const int ch = src->nChannels, sw = src->width, sh = src->height, dw = dst->width, dh = dst->height;
  const uchar* S = (const uchar*)src->imageData;
  uchar* D = (uchar*)dst->imageData;
  const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
  if (mode == CV_INTER_NN) {
    for (int y = 0; y < dh; ++y) {
      int sy = (int)floor(y * scale_y);
      if (sy > sh - 1) sy = sh - 1;
      for (int x = 0; x < dw; ++x) {
        int sx = (int)floor(x * scale_x);
        if (sx > sw - 1) sx = sw - 1;
        for (int c = 0; c < ch; ++c) D[(size_t)y * dst->widthStep + x * ch + c] = S[(size_t)sy * src->widthStep + sx * ch + c];
      }
    }
    return;
  }
  if (mode != CV_INTER_LINEAR) cvStandInAbort("cvResize of another mode");
  if (sw == 2 * dw && sh == 2 * dh) {
    for (int y = 0; y < dh; ++y)
      for (int x = 0; x < dw; ++x)
        for (int c = 0; c < ch; ++c) {
          const uchar* s = S + (size_t)(2 * y) * src->widthStep + (size_t)(2 * x) * ch + c;
          D[(size_t)y * dst->widthStep + x * ch + c] = (uchar)((s[0] + s[ch] + s[src->widthStep] + s[src->widthStep + ch] + 2) >> 2);
        }
    return;
  }
  std::vector<int> xofs(dw), ia(2 * dw);
  for (int dx = 0; dx < dw; ++dx) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0) fx = 0, sx = 0;
    if (sx >= sw - 1) fx = 0, sx = sw - 1;
    xofs[dx] = sx, ia[2 * dx] = standInSatShort((1.f - fx) * 2048.f), ia[2 * dx + 1] = standInSatShort(fx * 2048.f);
  }
  for (int dy = 0; dy < dh; ++dy) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= sy;
    const int b0 = standInSatShort((1.f - fy) * 2048.f), b1 = standInSatShort(fy * 2048.f);
    const int y0 = sy < 0 ? 0 : sy > sh - 1 ? sh - 1 : sy, y1 = sy + 1 < 0 ? 0 : sy + 1 > sh - 1 ? sh - 1 : sy + 1;
    const uchar *S0 = S + (size_t)y0 * src->widthStep, *S1 = S + (size_t)y1 * src->widthStep;
    for (int dx = 0; dx < dw; ++dx)
      for (int c = 0; c < ch; ++c) {
        const int sx = xofs[dx], sx1 = sx + 1 < sw ? sx + 1 : sx;
        const int r0 = S0[sx * ch + c] * ia[2 * dx] + S0[sx1 * ch + c] * ia[2 * dx + 1], r1 = S1[sx * ch + c] * ia[2 * dx] + S1[sx1 * ch + c] * ia[2 * dx + 1];
        D[(size_t)dy * dst->widthStep + dx * ch + c] = (uchar)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
      }
  }
}

// cvCvtColor(CV_BGR2GRAY) from the source's region of interest into an image of that size: (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14
inline void cvCvtColor(const IplImage* src, IplImage* dst, int code) {
  if (code != CV_BGR2GRAY || src->nChannels != 3 || dst->nChannels != 1 || dst->roiW) cvStandInAbort("cvCvtColor other than BGR2GRAY");
  const int x0 = src->roiX, y0 = src->roiY, w = src->roiW ? src->roiW : src->width, h = src->roiW ? src->roiH : src->height;
  if (w != dst->width || h != dst->height) cvStandInAbort("cvCvtColor between different sizes");
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const uchar* p = (const uchar*)src->imageData + (size_t)(y + y0) * src->widthStep + (size_t)(x + x0) * 3;
      dst->imageData[(size_t)y * dst->widthStep + x] = (char)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14);
    }
}

struct StandInCannyCall {
  int rows, cols;
  std::vector<uchar> in, out;  // rows x cols, back to back
};
inline std::vector<StandInCannyCall>& standInCannyLog() {
  static std::vector<StandInCannyCall> log;
  return log;
}

// cvCanny with aperture 3 and the L1 magnitude, as DESIGN.md 5.12 states it: Sobel 3 x 3 with a replicated border, non-maximum
// suppression with the 15-bit fixed-point tan 22.5 deg test (the magnitude outside the image is 0), hysteresis over 8 neighbours
inline void cvCanny(const IplImage* src, IplImage* dst, double t1, double t2, int aperture = 3) {
  if (aperture != 3 || src->nChannels != 1 || dst->nChannels != 1 || src->roiW || dst->roiW || src->width != dst->width || src->height != dst->height)
    cvStandInAbort("cvCanny other than aperture 3 on whole single-channel images");
  int low = (int)floor(t1), high = (int)floor(t2);
  if (low > high) { const int t = low; low = high; high = t; }
  const int R = src->height, W = src->width, TG22 = (int)(0.4142135623730950488016887242097 * (1 << 15) + 0.5);
  StandInCannyCall call;
  call.rows = R, call.cols = W, call.in.resize((size_t)R * W), call.out.assign((size_t)R * W, 0);
  for (int y = 0; y < R; ++y) memcpy(&call.in[(size_t)y * W], src->imageData + (size_t)y * src->widthStep, W);
  std::vector<int> mag((size_t)R * W), dir((size_t)R * W);
  std::vector<uchar> cand((size_t)R * W, 0);
  auto px = [&](int y, int x) { return (int)call.in[(size_t)(y < 0 ? 0 : y > R - 1 ? R - 1 : y) * W + (x < 0 ? 0 : x > W - 1 ? W - 1 : x)]; };
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) {
      const int dx = (px(y - 1, x + 1) + 2 * px(y, x + 1) + px(y + 1, x + 1)) - (px(y - 1, x - 1) + 2 * px(y, x - 1) + px(y + 1, x - 1));
      const int dy = (px(y + 1, x - 1) + 2 * px(y + 1, x) + px(y + 1, x + 1)) - (px(y - 1, x - 1) + 2 * px(y - 1, x) + px(y - 1, x + 1));
      const int ax = abs(dx), ay = abs(dy) << 15, tg22x = ax * TG22, tg67x = tg22x + (ax << 16);
      mag[(size_t)y * W + x] = ax + abs(dy);
      dir[(size_t)y * W + x] = ay < tg22x ? 0 : ay > tg67x ? 1 : ((dx ^ dy) < 0 ? 3 : 2);
    }
  auto m = [&](int y, int x) { return (y < 0 || y >= R || x < 0 || x >= W) ? 0 : mag[(size_t)y * W + x]; };
  std::vector<int> stack;
  for (int y = 0; y < R; ++y)
    for (int x = 0; x < W; ++x) {
      const int v = mag[(size_t)y * W + x], d = dir[(size_t)y * W + x];
      bool keep = false;
      if (v > low) {
        if (d == 0) keep = v > m(y, x - 1) && v >= m(y, x + 1);
        else if (d == 1) keep = v > m(y - 1, x) && v >= m(y + 1, x);
        else { const int s = d == 3 ? -1 : 1; keep = v > m(y - 1, x - s) && v > m(y + 1, x + s); }
      }
      if (!keep) continue;
      cand[(size_t)y * W + x] = 1;
      if (v > high) call.out[(size_t)y * W + x] = 255, stack.push_back(y * W + x);
    }
  while (!stack.empty()) {
    const int i = stack.back(), y = i / W, x = i - y * W;
    stack.pop_back();
    for (int yy = y - 1 < 0 ? 0 : y - 1; yy <= (y + 1 > R - 1 ? R - 1 : y + 1); ++yy)
      for (int xx = x - 1 < 0 ? 0 : x - 1; xx <= (x + 1 > W - 1 ? W - 1 : x + 1); ++xx)
        if (cand[(size_t)yy * W + xx] && !call.out[(size_t)yy * W + xx]) call.out[(size_t)yy * W + xx] = 255, stack.push_back(yy * W + xx);
  }
  for (int y = 0; y < R; ++y) memcpy(dst->imageData + (size_t)y * dst->widthStep, &call.out[(size_t)y * W], W);
  standInCannyLog().push_back(call);
}
inline CvFileStorage* cvOpenFileStorage(const char*, void*, int) { cvStandInAbort("cvOpenFileStorage"); }
inline void cvReleaseFileStorage(CvFileStorage**) { cvStandInAbort("cvReleaseFileStorage"); }
inline void cvWriteInt(CvFileStorage*, const char*, int) { cvStandInAbort("cvWriteInt"); }
inline int cvReadIntByName(CvFileStorage*, void*, const char*, int = 0) { cvStandInAbort("cvReadIntByName"); }

namespace cv {

struct Size {
  int width, height;
  Size(int w, int h) : width(w), height(h) {}
};

class Mat {  // 8-bit, 3 channels, rows back to back
 public:
  int rows, cols;
  size_t step;
  std::vector<uchar> buf;
  uchar* data;
  Mat() : rows(0), cols(0), step(0), data(NULL) {}
  Mat(const IplImage* im, bool copyData) : rows(im->height), cols(im->width), step((size_t)im->width * 3), buf((size_t)im->height * im->width * 3) {
    if (!copyData || im->nChannels != 3 || im->depth != IPL_DEPTH_8U) cvStandInAbort("cv::Mat(IplImage*) other than a copy of an 8-bit 3-channel image");
    for (int y = 0; y < rows; ++y) memcpy(&buf[(size_t)y * step], im->imageData + (size_t)y * im->widthStep, step);
    data = buf.data();
  }
  Mat(const Mat& o) : rows(o.rows), cols(o.cols), step(o.step), buf(o.buf), data(buf.empty() ? NULL : buf.data()) {}
  Mat& operator=(const Mat& o) {
    rows = o.rows, cols = o.cols, step = o.step, buf = o.buf, data = buf.empty() ? NULL : buf.data();
    return *this;
  }
  bool empty() const { return buf.empty(); }
  void copyTo(Mat& o) const { o = *this; }
};

inline void imshow(const char*, const Mat&) { cvStandInAbort("cv::imshow"); }

// cv::getGaussianKernel(n, sigma, CV_32F) for sigma > 0 (imgproc/src/smooth.cpp)
inline void standInGaussianKernel(int n, double sigma, float* k) {
  const double scale2X = -0.5 / (sigma * sigma);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    k[i] = (float)std::exp(scale2X * x * x);
    sum += k[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
}

inline int standInReflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

inline void GaussianBlur(const Mat& src, Mat& dst, Size ksize, double sigma) {
  if (ksize.width != 7 || ksize.height != 7 || !(sigma > 0) || src.empty()) cvStandInAbort("cv::GaussianBlur other than 7 x 7 with sigma > 0");
  float cf[7];
  int k[7];
  standInGaussianKernel(7, sigma, cf);
  for (int i = 0; i < 7; ++i) k[i] = (int)lrintf(cf[i] * 256.f);
  const int H = src.rows, W = src.cols;
  std::vector<int> row((size_t)H * W * 3);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) {
        int s = 0;
        for (int j = 0; j < 7; ++j) s += k[j] * src.buf[(size_t)y * src.step + (size_t)standInReflect101(x + j - 3, W) * 3 + c];
        row[((size_t)y * W + x) * 3 + c] = s;
      }
  Mat out(src);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) {
        int s = 0;
        for (int j = 0; j < 7; ++j) s += k[j] * row[((size_t)standInReflect101(y + j - 3, H) * W + x) * 3 + c];
        const int v = (s + (1 << 15)) >> 16;
        out.buf[(size_t)y * out.step + (size_t)x * 3 + c] = (uchar)(v < 0 ? 0 : v > 255 ? 255 : v);
      }
  dst = out;
}

}  // namespace cv

inline IplImage::IplImage(const cv::Mat& m) : nChannels(3), depth(IPL_DEPTH_8U), width(m.cols), height(m.rows), widthStep((int)m.step), imageData((char*)m.data), roiX(0), roiY(0), roiW(0), roiH(0) {}
