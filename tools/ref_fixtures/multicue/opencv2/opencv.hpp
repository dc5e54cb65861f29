// Stand-in for <opencv2/opencv.hpp>: the part of OpenCV 2.4 that package_bgs/sjn/SJN_MultiCueBGS.{h,cpp} names, written for the
// fixture generator (README.md here).  The model stage calls cvCreateImage / cvReleaseImage, the two cv::Mat <->
// IplImage constructors of SJN_MultiCueBGS.cpp:523-528 and cv::GaussianBlur(7 x 7, sigma 0.7) on 8-bit data; the blur is DEFINED
// here as OpenCV 2.4's 8-bit fixed-point filter (integer taps lrintf(k * 256), exact row pass, column pass (sum + 2^15) >> 16,
// BORDER_REFLECT_101).  Everything else the file names belongs to the box stage or the wrapper and aborts.
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
  IplImage() : nChannels(0), depth(0), width(0), height(0), widthStep(0), imageData(NULL) {}
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
inline void cvSetImageROI(IplImage*, CvRect) { cvStandInAbort("cvSetImageROI"); }
inline void cvResetImageROI(IplImage*) { cvStandInAbort("cvResetImageROI"); }
inline void cvResize(const IplImage*, IplImage*, int = CV_INTER_LINEAR) { cvStandInAbort("cvResize"); }
inline void cvCvtColor(const IplImage*, IplImage*, int) { cvStandInAbort("cvCvtColor"); }
inline void cvCanny(const IplImage*, IplImage*, double, double, int = 3) { cvStandInAbort("cvCanny"); }
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

inline IplImage::IplImage(const cv::Mat& m) : nChannels(3), depth(IPL_DEPTH_8U), width(m.cols), height(m.rows), widthStep((int)m.step), imageData((char*)m.data) {}
