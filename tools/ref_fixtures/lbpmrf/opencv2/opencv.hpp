// Stand-in for <opencv2/opencv.hpp> and <opencv/cvaux.h>: the part of OpenCV 2.4 that package_bgs/ck/MotionDetection.cpp, MEImage.cpp,
// MEHistogram.cpp and MEDefs.cpp name, written for the fixture generator (README.md here).  The driven path, GetMotionsMaskHU
// (MotionDetection.cpp:1256-1366) and the MEImage constructors, assignment and Erode it needs, calls cvCreateImage / cvReleaseImage /
// cvCloneImage / cvSetZero / cvFloodFill / cvErode; those are DEFINED here as DESIGN.md 5.15 states them (recalled from OpenCV 2.4,
// unpinned): rows padded to 4 bytes; cvFloodFill with zero tolerances = the 4-connected region of the seed's own value; cvErode with a
// NULL element = the 3 x 3 minimum, cells outside the image taking no part.  Everything else aborts: it is not on the driven path.
#pragma once
#include <math.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned char uchar;

#define IPL_DEPTH_8U 8
#define IPL_DEPTH_16S 16
enum {
  CV_BGR2GRAY, CV_RGB2GRAY, CV_GRAY2RGB, CV_RGB2BGR, CV_RGB2XYZ, CV_XYZ2RGB, CV_RGB2HSV, CV_HSV2RGB, CV_RGB2HLS, CV_HLS2RGB, CV_RGB2Lab, CV_Lab2RGB, CV_RGB2Luv,
  CV_Luv2RGB, CV_INTER_NN, CV_BLUR, CV_MEDIAN, CV_GAUSSIAN, CV_THRESH_BINARY, CV_ADAPTIVE_THRESH_GAUSSIAN_C, CV_TERMCRIT_ITER = 1, CV_TERMCRIT_EPS = 2
};

[[noreturn]] inline void cvStandInAbort(const char* what) {
  fprintf(stderr, "opencv stand-in: %s is not on the driven path\n", what);
  abort();
}

struct CvSize { int width, height; };
struct CvRect { int x, y, width, height; };
struct CvPoint { int x, y; };
struct CvPoint2D32f { float x, y; };
struct CvScalar { double val[4]; };
struct CvTermCriteria { int type, max_iter; double epsilon; };
struct CvBGStatModel;

struct IplImage {
  int nChannels, depth, width, height, widthStep, origin;
  char* imageData;
};

inline CvSize cvSize(int w, int h) { CvSize s = {w, h}; return s; }
inline CvRect cvRect(int x, int y, int w, int h) { CvRect r = {x, y, w, h}; return r; }
inline CvPoint cvPoint(int x, int y) { CvPoint p = {x, y}; return p; }
inline CvScalar cvScalar(double a, double b = 0, double c = 0, double d = 0) { CvScalar s = {{a, b, c, d}}; return s; }
#define CV_RGB(r, g, b) cvScalar((b), (g), (r), 0)
inline CvTermCriteria cvTermCriteria(int t, int n, double e) { CvTermCriteria c = {t, n, e}; return c; }

inline IplImage* cvCreateImage(CvSize s, int depth, int ch) {
  if (depth != IPL_DEPTH_8U) cvStandInAbort("cvCreateImage of another depth");
  IplImage* im = new IplImage;
  im->nChannels = ch, im->depth = depth, im->width = s.width, im->height = s.height, im->origin = 0;
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
inline IplImage* cvCloneImage(const IplImage* src) {
  IplImage* im = cvCreateImage(cvSize(src->width, src->height), src->depth, src->nChannels);
  memcpy(im->imageData, src->imageData, (size_t)src->widthStep * src->height);
  im->origin = src->origin;
  return im;
}
inline CvSize cvGetSize(const void* arr) { const IplImage* im = (const IplImage*)arr; return cvSize(im->width, im->height); }
inline void cvSetZero(IplImage* im) { memset(im->imageData, 0, (size_t)im->widthStep * im->height); }

// cvFloodFill(img, seed, value, lo = 0, up = 0): 4-connected, the pixels equal to the seed pixel's value, one channel
inline void cvFloodFill(void* image, CvPoint seed, CvScalar value, CvScalar lo, CvScalar up) {
  IplImage* im = (IplImage*)image;
  if (im->nChannels != 1 || lo.val[0] != 0 || up.val[0] != 0) cvStandInAbort("cvFloodFill with tolerances or channels");
  uchar* d = (uchar*)im->imageData;
  const int w = im->width, h = im->height, ws = im->widthStep;
  const uchar from = d[(size_t)seed.y * ws + seed.x], to = (uchar)value.val[0];
  if (from == to) return;  // as OpenCV: nothing to repaint, and a fill that would never stop
  std::vector<CvPoint> stack(1, seed);
  d[(size_t)seed.y * ws + seed.x] = to;
  while (!stack.empty()) {
    const CvPoint p = stack.back();
    stack.pop_back();
    const int nx[4] = {p.x - 1, p.x + 1, p.x, p.x}, ny[4] = {p.y, p.y, p.y - 1, p.y + 1};
    for (int k = 0; k < 4; ++k)
      if (nx[k] >= 0 && nx[k] < w && ny[k] >= 0 && ny[k] < h && d[(size_t)ny[k] * ws + nx[k]] == from) {
        d[(size_t)ny[k] * ws + nx[k]] = to;
        stack.push_back(cvPoint(nx[k], ny[k]));
      }
  }
}

// cvErode(src, dst, NULL, iterations): the 3 x 3 minimum per iteration; cells outside the image take no part
inline void cvErode(const IplImage* src, IplImage* dst, void* element, int iterations) {
  if (element || src->nChannels != 1 || iterations < 1) cvStandInAbort("cvErode with an element or channels");
  const int w = src->width, h = src->height;
  std::vector<uchar> a((size_t)w * h), b((size_t)w * h);
  for (int y = 0; y < h; ++y) memcpy(&a[(size_t)y * w], src->imageData + (size_t)y * src->widthStep, w);
  for (int it = 0; it < iterations; ++it) {
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        uchar m = 255;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx)
            if (y + dy >= 0 && y + dy < h && x + dx >= 0 && x + dx < w && a[(size_t)(y + dy) * w + x + dx] < m) m = a[(size_t)(y + dy) * w + x + dx];
        b[(size_t)y * w + x] = m;
      }
    a.swap(b);
  }
  for (int y = 0; y < h; ++y) memcpy(dst->imageData + (size_t)y * dst->widthStep, &a[(size_t)y * w], w);
}

// named by the files, never called on the driven path
#define CV_STAND_IN_ABORTS(name) \
  template <class... A>          \
  inline void name(A...) { cvStandInAbort(#name); }
CV_STAND_IN_ABORTS(cvCvtColor) CV_STAND_IN_ABORTS(cvSmooth) CV_STAND_IN_ABORTS(cvSetImageCOI) CV_STAND_IN_ABORTS(cvFree) CV_STAND_IN_ABORTS(cvEqualizeHist)
CV_STAND_IN_ABORTS(cvCopy) CV_STAND_IN_ABORTS(cvSetImageROI) CV_STAND_IN_ABORTS(cvResetImageROI) CV_STAND_IN_ABORTS(cvFlip) CV_STAND_IN_ABORTS(cvCircle)
CV_STAND_IN_ABORTS(cvSplit) CV_STAND_IN_ABORTS(cvMerge) CV_STAND_IN_ABORTS(cvResize) CV_STAND_IN_ABORTS(cvRectangle) CV_STAND_IN_ABORTS(cvLine)
CV_STAND_IN_ABORTS(cvLaplace) CV_STAND_IN_ABORTS(cvGoodFeaturesToTrack) CV_STAND_IN_ABORTS(cvEllipse) CV_STAND_IN_ABORTS(cvDilate) CV_STAND_IN_ABORTS(cvConvertScale)
CV_STAND_IN_ABORTS(cvCanny) CV_STAND_IN_ABORTS(cvCalcOpticalFlowPyrLK) CV_STAND_IN_ABORTS(cvAdaptiveThreshold)
template <class... A>
inline void* cvAlloc(A...) { cvStandInAbort("cvAlloc"); }
