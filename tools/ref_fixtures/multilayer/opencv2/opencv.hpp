// Stand-in for <opencv2/opencv.hpp>: the part of OpenCV 2.4's C interface that package_bgs/jmo's model code names, written for the
// fixture generator (README.md here).  What the live path of CMultiLayerBGS calls is defined as tests/multilayer_numpy.py and
// DESIGN.md 5.11 state it; everything else aborts.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned char uchar;

#define IPL_DEPTH_8U 8
#define IPL_DEPTH_16S 16
#define IPL_DEPTH_32F 32
#define CV_BGR2GRAY 6
#define CV_GAUSSIAN 2
#define CV_THRESH_BINARY 0
#define CV_THRESH_BINARY_INV 1
#define CV_MOP_OPEN 2
#define CV_MOP_CLOSE 3
#ifndef MIN
#define MIN(a, b) ((a) > (b) ? (b) : (a))
#endif
#ifndef MAX
#define MAX(a, b) ((a) < (b) ? (b) : (a))
#endif

struct CvSize { int width, height; };
struct CvPoint { int x, y; };
struct CvRect { int x, y, width, height; };
struct CvScalar { double val[4]; };
struct CvMat {
  int width, height, step;
  union { uchar* ptr; float* fl; } data;
};
struct IplROI { int coi, xOffset, yOffset, width, height; };
struct IplImage {
  int nChannels, depth, width, height, widthStep;
  IplROI* roi;
  char* imageData;
};

inline CvSize cvSize(int w, int h) { CvSize s = {w, h}; return s; }
inline CvRect cvRect(int x, int y, int w, int h) { CvRect r = {x, y, w, h}; return r; }
inline CvScalar cvScalar(double a, double b = 0, double c = 0, double d = 0) { CvScalar s = {{a, b, c, d}}; return s; }
#define CV_RGB(r, g, b) cvScalar((b), (g), (r), 0)
inline int cvRound(double v) { return (int)lrint(v); }
inline float cvSqrt(float v) { return sqrtf(v); }

[[noreturn]] inline void cvStandInAbort(const char* what) {
  fprintf(stderr, "opencv stand-in: %s is not on the live path\n", what);
  abort();
}

inline int cvElemSize(const IplImage* im) { return (im->depth / 8) * im->nChannels; }
inline IplImage* cvCreateImage(CvSize s, int depth, int ch) {
  IplImage* im = new IplImage;
  im->nChannels = ch, im->depth = depth, im->width = s.width, im->height = s.height;
  im->widthStep = (s.width * ch * (depth / 8) + 3) & ~3;  // rows padded to 4 bytes, so widthStep != width * elemSize at odd widths
  im->roi = NULL;
  im->imageData = (char*)calloc((size_t)im->widthStep * s.height + 4, 1);
  return im;
}
inline void cvReleaseImage(IplImage** im) {
  if (!im || !*im) return;
  free((*im)->imageData);
  delete (*im)->roi;
  delete *im;
  *im = NULL;
}
inline CvRect cvGetImageROI(const IplImage* im) { return im->roi ? cvRect(im->roi->xOffset, im->roi->yOffset, im->roi->width, im->roi->height) : cvRect(0, 0, im->width, im->height); }
inline CvSize cvGetSize(const IplImage* im) { CvRect r = cvGetImageROI(im); return cvSize(r.width, r.height); }
inline void cvSetImageROI(IplImage* im, CvRect r) {
  if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > im->width || r.y + r.height > im->height) cvStandInAbort("cvSetImageROI outside the image");
  if (!im->roi) im->roi = new IplROI;
  im->roi->coi = 0, im->roi->xOffset = r.x, im->roi->yOffset = r.y, im->roi->width = r.width, im->roi->height = r.height;
}
inline void cvResetImageROI(IplImage* im) { delete im->roi, im->roi = NULL; }
inline char* cvRowPtr(const IplImage* im, const CvRect& r, int y) { return im->imageData + (size_t)im->widthStep * (r.y + y) + (size_t)r.x * cvElemSize(im); }

inline void cvCopy(const IplImage* src, IplImage* dst, const IplImage* mask = NULL) {
  const CvRect a = cvGetImageROI(src), b = cvGetImageROI(dst);
  if (a.width != b.width || a.height != b.height || src->depth != dst->depth || src->nChannels != dst->nChannels) cvStandInAbort("cvCopy with unequal sizes or types");
  const int es = cvElemSize(src);
  for (int y = 0; y < a.height; ++y) {
    const char* s = cvRowPtr(src, a, y);
    char* d = cvRowPtr(dst, b, y);
    if (!mask) { memcpy(d, s, (size_t)a.width * es); continue; }
    const uchar* m = (const uchar*)cvRowPtr(mask, cvGetImageROI(mask), y);
    for (int x = 0; x < a.width; ++x)
      if (m[x]) memcpy(d + (size_t)x * es, s + (size_t)x * es, es);
  }
}
inline void cvCopy(const IplImage*, CvMat*) { cvStandInAbort("cvCopy to a CvMat"); }
inline void cvCopyImage(const IplImage* src, IplImage* dst) { cvCopy(src, dst); }
inline IplImage* cvCloneImage(const IplImage* src) {
  IplImage* im = cvCreateImage(cvSize(src->width, src->height), src->depth, src->nChannels);
  memcpy(im->imageData, src->imageData, (size_t)src->widthStep * src->height);
  return im;
}
inline void cvSet(IplImage* im, CvScalar v) {
  const CvRect r = cvGetImageROI(im);
  for (int y = 0; y < r.height; ++y) {
    char* d = cvRowPtr(im, r, y);
    for (int x = 0; x < r.width; ++x)
      for (int c = 0; c < im->nChannels; ++c) {
        if (im->depth == IPL_DEPTH_8U) ((uchar*)d)[x * im->nChannels + c] = (uchar)std::min(255., std::max(0., (double)cvRound(v.val[c])));
        else if (im->depth == IPL_DEPTH_32F) ((float*)d)[x * im->nChannels + c] = (float)v.val[c];
        else cvStandInAbort("cvSet on this depth");
      }
  }
}
inline void cvSet(IplImage*, CvScalar, const IplImage*) { cvStandInAbort("cvSet with a mask"); }
inline void cvSetZero(IplImage* im) { cvSet(im, cvScalar(0)); }

// OpenCV 2.4 BGR2GRAY on bytes: fixed point, 14 fractional bits (imgproc/src/color.cpp, RGB2Gray<uchar>: B 1868, G 9617, R 4899)
inline void cvCvtColor(const IplImage* src, IplImage* dst, int code) {
  if (code != CV_BGR2GRAY || src->depth != IPL_DEPTH_8U || src->nChannels != 3 || dst->depth != IPL_DEPTH_8U || dst->nChannels != 1) cvStandInAbort("cvCvtColor other than 8-bit BGR2GRAY");
  const CvRect a = cvGetImageROI(src), b = cvGetImageROI(dst);
  for (int y = 0; y < a.height; ++y) {
    const uchar* s = (const uchar*)cvRowPtr(src, a, y);
    uchar* d = (uchar*)cvRowPtr(dst, b, y);
    for (int x = 0; x < a.width; ++x) d[x] = (uchar)((s[3 * x] * 1868 + s[3 * x + 1] * 9617 + s[3 * x + 2] * 4899 + (1 << 13)) >> 14);
  }
}

// cv::getGaussianKernel(n, sigma, CV_32F) for sigma > 0 (imgproc/src/smooth.cpp)
inline std::vector<float> cvStandInGaussianKernel(int n, double sigma) {
  if (!(sigma > 0)) cvStandInAbort("a Gaussian with sigma <= 0");
  std::vector<float> k(n);
  const double scale2X = -0.5 / (sigma * sigma);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    k[i] = (float)std::exp(scale2X * x * x);
    sum += k[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
  return k;
}

// cvSmooth(CV_GAUSSIAN) on a one-channel float image, in place, BORDER_REPLICATE: rows first (s = k[0] x[0]; s += k[i] x[i]), then
// columns in the symmetric form (s = k[c] x[c]; s += k[c + i] (x[c + i] + x[c - i])), all in float without contraction.
inline void cvSmooth(IplImage* src, IplImage* dst, int type, int p1, int p2, double sigma) {
  if (type != CV_GAUSSIAN || src != dst || src->depth != IPL_DEPTH_32F || src->nChannels != 1 || p1 != p2 || p1 < 1 || !(p1 & 1) || src->roi) cvStandInAbort("cvSmooth other than an in-place square Gaussian on a float plane");
  if (p1 == 1) return;  // GaussianBlur: a 1 x 1 kernel copies
  const std::vector<float> k = cvStandInGaussianKernel(p1, sigma);
  const int h = p1 / 2, W = src->width, H = src->height;
  std::vector<float> row((size_t)W * H);
  for (int y = 0; y < H; ++y) {
    const float* s = (const float*)(src->imageData + (size_t)src->widthStep * y);
    for (int x = 0; x < W; ++x) {
      volatile float acc = k[0] * s[std::min(std::max(x - h, 0), W - 1)];
      for (int i = 1; i < p1; ++i) {
        volatile float t = k[i] * s[std::min(std::max(x - h + i, 0), W - 1)];
        acc = acc + t;
      }
      row[(size_t)y * W + x] = acc;
    }
  }
  for (int y = 0; y < H; ++y) {
    float* d = (float*)(dst->imageData + (size_t)dst->widthStep * y);
    for (int x = 0; x < W; ++x) {
      volatile float acc = k[h] * row[(size_t)y * W + x];
      for (int i = 1; i <= h; ++i) {
        volatile float pair = row[(size_t)std::min(y + i, H - 1) * W + x] + row[(size_t)std::max(y - i, 0) * W + x];
        volatile float t = k[h + i] * pair;
        acc = acc + t;
      }
      d[x] = acc;
    }
  }
}

inline void cvThreshold(const IplImage* src, IplImage* dst, double thresh, double maxval, int type) {
  if (type != CV_THRESH_BINARY || dst->depth != IPL_DEPTH_8U || src->nChannels != 1 || dst->nChannels != 1) cvStandInAbort("cvThreshold other than BINARY to bytes");
  const CvRect a = cvGetImageROI(src), b = cvGetImageROI(dst);
  const uchar mv = (uchar)std::min(255., std::max(0., (double)cvRound(maxval)));
  for (int y = 0; y < a.height; ++y) {
    uchar* d = (uchar*)cvRowPtr(dst, b, y);
    if (src->depth == IPL_DEPTH_32F) {
      const float* s = (const float*)cvRowPtr(src, a, y);
      const float t = (float)thresh;  // thresh_32f compares against (float)thresh
      for (int x = 0; x < a.width; ++x) d[x] = s[x] > t ? mv : 0;
    } else if (src->depth == IPL_DEPTH_8U) {
      const uchar* s = (const uchar*)cvRowPtr(src, a, y);
      const int t = (int)std::floor(thresh);
      for (int x = 0; x < a.width; ++x) d[x] = s[x] > t ? mv : 0;
    } else cvStandInAbort("cvThreshold on this depth");
  }
}

inline void cvSplit(const IplImage* src, IplImage* d0, IplImage* d1, IplImage* d2, IplImage* d3) {
  IplImage* d[4] = {d0, d1, d2, d3};
  const CvRect a = cvGetImageROI(src);
  for (int c = 0; c < src->nChannels && c < 4; ++c) {
    if (!d[c]) continue;
    const CvRect b = cvGetImageROI(d[c]);
    for (int y = 0; y < a.height; ++y)
      for (int x = 0; x < a.width; ++x) ((uchar*)cvRowPtr(d[c], b, y))[x] = ((const uchar*)cvRowPtr(src, a, y))[x * src->nChannels + c];
  }
}

inline void cvSobel(const IplImage*, IplImage*, int, int, int) { cvStandInAbort("cvSobel"); }
inline void cvErode(const IplImage*, IplImage*, void*, int) { cvStandInAbort("cvErode"); }
inline void cvDilate(const IplImage*, IplImage*, void*, int) { cvStandInAbort("cvDilate"); }
inline void cvMorphologyEx(const IplImage*, IplImage*, IplImage*, void*, int, int) { cvStandInAbort("cvMorphologyEx"); }
inline void cvAnd(const IplImage*, const IplImage*, IplImage*) { cvStandInAbort("cvAnd"); }
inline void cvNamedWindow(const char*, int = 1) { cvStandInAbort("cvNamedWindow"); }
inline void cvShowImage(const char*, const IplImage*) { cvStandInAbort("cvShowImage"); }
inline int cvWaitKey(int = 0) { cvStandInAbort("cvWaitKey"); }
