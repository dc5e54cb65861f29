// Stand-in for <opencv2/opencv.hpp>: TEST INFRASTRUCTURE ONLY, used to compile the reference's own package_bgs/dp/ model files
// unmodified into oracle/_ref/ref_dp_cli (oracle/Makefile).  It declares the OpenCV C names dp/Image.h and the five model files
// use and nothing else: IplImage, CvSize / cvSize, CvScalar / CV_RGB, cvCreateImage (8U and 32F), cvReleaseImage, cvZero, cvSet.
//   * widthStep is rounded up to 4 bytes, as OpenCV's cvInitImageHeader does with its default alignment.
//   * cvCreateImage leaves the buffer POISONED (OpenCV leaves it uninitialised): every byte, row padding included, is the value of
//     the environment variable REF_STUB_POISON (default 0xCD), so a read of memory the reference never wrote changes the result
//     between two runs with different values.
//   * cvZero / cvSet touch width x channels x depth/8 bytes of every row, never the padding.
//   * <math.h>, <stdlib.h>, <string.h> and <assert.h> come along as they do from OpenCV 2.4's core/types_c.h; nothing here
//     brings namespace std into scope.  REF_STUB_SQRT_DOUBLE (a build variant, never the pinned one) sends every unqualified
//     sqrt(x) to the double overload, to measure what that choice would change.
#ifndef REF_STUB_OPENCV_HPP
#define REF_STUB_OPENCV_HPP

#include <assert.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#ifdef REF_STUB_SQRT_DOUBLE
static inline double ref_stub_sqrt_double(double x) { return sqrt(x); }
#define sqrt(x) ref_stub_sqrt_double((double)(x))
#endif

#define IPL_DEPTH_8U 8
#define IPL_DEPTH_32F 32
#define IPL_ORIGIN_TL 0
#define IPL_ORIGIN_BL 1

typedef struct _IplImage {
  int nChannels, depth, origin, width, height, widthStep, imageSize;
  char* imageData;
} IplImage;

typedef struct CvSize {
  int width, height;
} CvSize;

typedef struct CvScalar {
  double val[4];
} CvScalar;

static inline CvSize cvSize(int width, int height) {
  CvSize s = {width, height};
  return s;
}

static inline CvScalar cvScalar(double v0, double v1, double v2, double v3) {
  CvScalar s = {{v0, v1, v2, v3}};
  return s;
}

#define CV_RGB(r, g, b) cvScalar((b), (g), (r), 0)

static inline IplImage* cvCreateImage(CvSize size, int depth, int channels) {
  assert((depth == IPL_DEPTH_8U || depth == IPL_DEPTH_32F) && channels >= 1 && channels <= 4);
  IplImage* img = (IplImage*)malloc(sizeof(IplImage));
  img->nChannels = channels, img->depth = depth, img->origin = IPL_ORIGIN_TL;
  img->width = size.width, img->height = size.height;
  img->widthStep = (size.width * channels * (depth / 8) + 3) & ~3;
  img->imageSize = img->widthStep * size.height;
  img->imageData = (char*)malloc(img->imageSize ? img->imageSize : 1);
  const char* poison = getenv("REF_STUB_POISON");
  memset(img->imageData, poison ? (int)strtol(poison, 0, 0) : 0xCD, img->imageSize);
  return img;
}

static inline void cvReleaseImage(IplImage** img) {
  if (img && *img) {
    free((*img)->imageData);
    free(*img);
    *img = 0;
  }
}

static inline void cvZero(IplImage* img) {
  for (int r = 0; r < img->height; ++r) memset(img->imageData + (size_t)r * img->widthStep, 0, (size_t)img->width * img->nChannels * (img->depth / 8));
}

static inline void cvSet(IplImage* img, CvScalar value) {
  for (int r = 0; r < img->height; ++r)
    for (int c = 0; c < img->width; ++c)
      for (int ch = 0; ch < img->nChannels; ++ch) {
        char* p = img->imageData + (size_t)r * img->widthStep + (size_t)(c * img->nChannels + ch) * (img->depth / 8);
        if (img->depth == IPL_DEPTH_32F) {
          const float f = (float)value.val[ch];
          memcpy(p, &f, sizeof f);
        } else {
          const double v = value.val[ch];
          *(unsigned char*)p = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : (int)lrint(v));
        }
      }
}

#endif
