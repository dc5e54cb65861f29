// HipFGDetector.h — reference-side FG detector over libbgs_hip with the blob list hand-off.  Add next to HipBGS.h in the
// USTC-Computer-Vision/tracking tree; replaces USTC_BGS (ustc_src/ustc_bgs.{h,cpp}) in ustc_src/trackingMain.cpp:
//
//     HipFGDetector* bgs = new HipFGDetector(type);      // trackingMain.cpp:35   was: USTC_BGS* bgs = new USTC_BGS(type);
//     param.pFG = bgs;                                    // :613                  unchanged
//
// Process / GetMask / Release are USTC_BGS's, statement for statement (ustc_bgs.cpp:75-113), over the hipbgs:: classes of HipBGS.h
// for the types on the hot path (0-13 except the three dp classes outside it, 35-37).  GetBlobs() is the addition: the foreground
// regions of the last mask as CvBlob {x, y, w, h, ID}, found on the device copy of the mask, so a blob-detection module can seed
// from rectangles instead of re-scanning the mask on the CPU (CvBlobDetector::DetectNewBlob receives the mask at :166).
// Types 15, 23, 33 and 34 have a class in HipBGS.h (DPEigenbackgroundBGS, MultiLayerBGS, IndependentMultimodalBGS, SJN_MultiCueBGS)
// and are not offered by number, as in ustc_bgs.h (see there).
//
// Needs OpenCV 2.4 with the legacy module (opencv2/legacy/blobtrack.hpp), which this repository's build image does not have:
// checked for syntax against the declaration-only mock under tests/mock_opencv (tests/test_capi_cpu.py), as gnu++0x like the
// reference's CMakeLists.txt:5.  The logic is shared with the tested mirror tracking_amd/host/ustc_bgs.h.
#pragma once
#include <vector>

#include "opencv2/legacy/blobtrack.hpp"
#include <opencv2/core/core.hpp>
#include <opencv2/imgproc/imgproc.hpp>

#include "HipBGS.h"
#include "blob_convert.h"

class HipFGDetector : public CvFGDetector {
 public:
  int frameNum;
  IplImage* c_mask;
  IBGS* bgs;
  cv::Mat img_mask;
  cv::Mat img_bkgmodel;
  cv::Mat img_input;
  IplImage b;
  int nextBlobID;

  explicit HipFGDetector(int type) : frameNum(0), c_mask(0), bgs(0), nextBlobID(0) {  // ustc_bgs.cpp:3-69
    const int i = type;
    CV_Assert(i >= 0 && i <= 37);
    switch (i) {
      case 0: bgs = new hipbgs::FrameDifferenceBGS; break;
      case 1: bgs = new hipbgs::StaticFrameDifferenceBGS; break;
      case 2: bgs = new hipbgs::WeightedMovingMeanBGS; break;
      case 3: bgs = new hipbgs::WeightedMovingVarianceBGS; break;
      case 4: bgs = new hipbgs::MixtureOfGaussianV1BGS; break;
      case 5: bgs = new hipbgs::MixtureOfGaussianV2BGS; break;
      case 6: bgs = new hipbgs::AdaptiveBackgroundLearning; break;
      case 7: bgs = new hipbgs::AdaptiveSelectiveBackgroundLearning; break;
      case 8: bgs = new hipbgs::GMG; break;
      case 9: bgs = new hipbgs::DPAdaptiveMedianBGS; break;
      case 10: bgs = new hipbgs::DPGrimsonGMMBGS; break;
      case 11: bgs = new hipbgs::DPZivkovicAGMMBGS; break;
      case 12: bgs = new hipbgs::DPMeanBGS; break;
      case 13: bgs = new hipbgs::DPWrenGABGS; break;
      case 14: bgs = new hipbgs::DPPratiMediodBGS; break;
      case 16: bgs = new hipbgs::DPTextureBGS; break;
      case 17: bgs = new hipbgs::T2FGMM_UM; break;
      case 18: bgs = new hipbgs::T2FGMM_UV; break;
      case 21: bgs = new hipbgs::FuzzySugenoIntegral; break;
      case 22: bgs = new hipbgs::FuzzyChoquetIntegral; break;
      case 25: bgs = new hipbgs::LBSimpleGaussian; break;
      case 26: bgs = new hipbgs::LBFuzzyGaussian; break;
      case 27: bgs = new hipbgs::LBMixtureOfGaussians; break;
      case 28: bgs = new hipbgs::LBAdaptiveSOM; break;
      case 29: bgs = new hipbgs::LBFuzzyAdaptiveSOM; break;
      case 31: bgs = new hipbgs::VuMeter; break;
      case 32: bgs = new hipbgs::KDE; break;
      case 35: bgs = new hipbgs::SigmaDeltaBGS; break;
      case 36: bgs = new hipbgs::SuBSENSEBGS; break;
      case 37: bgs = new hipbgs::LOBSTERBGS; break;
      default: break;  // 15, 19, 20, 23, 24, 30, 33, 34: refused below
    }
    if (!bgs) CV_Error(CV_StsBadArg, "HipFGDetector: this type is outside the package_bgs hot path libbgs_hip covers");
  }
  ~HipFGDetector() {}
  void Release() { delete bgs, bgs = 0; }  // :75-77

  IplImage* GetMask() {  // :79-85
    if (frameNum == 0) return NULL;
    return c_mask;
  }

  void Process(IplImage* pImg) {  // :87-113
    img_input = cv::Mat(pImg);
    bgs->process(img_input, img_mask, img_bkgmodel);
    if (!img_mask.empty()) {
      b = img_mask.operator IplImage();
      c_mask = &b;
      frameNum++;
    } else {
      std::cout << "img_mask is empty " << frameNum << std::endl;
      frameNum++;
    }
  }

  // One CvBlob per 8- (or 4-) connected foreground region of the last mask that is at least CV_BLOB_MINW x CV_BLOB_MINH pixels,
  // in raster order of the regions' first pixels; IDs count up from nextBlobID.  fromMoments: centre = centroid, size = 4 sigma
  // (what the legacy detectors compute from cvMoments); otherwise centre and size of the bounding rectangle.
  int GetBlobs(CvBlobSeq* pBlobs, int connectivity = 8, bool fromMoments = true) {
    pBlobs->Clear();
    if (frameNum == 0 || img_mask.empty()) return 0;
    hipbgs::HipBGSBase* h = dynamic_cast<hipbgs::HipBGSBase*>(bgs);
    CV_Assert(h != 0);
    h->lastMaskBlobs(connectivity, CV_BLOB_MINW, CV_BLOB_MINH, boxes_, moments_);
    for (size_t k = 0; k < boxes_.size(); ++k) {
      CvBlob B = cvBlob(0, 0, 0, 0);
      if (fromMoments)
        bgs_hip_convert::blob_from_moments(boxes_[k], moments_[k], B);
      else
        bgs_hip_convert::blob_from_box(boxes_[k], B);
      B.ID = nextBlobID++;
      pBlobs->AddBlob(&B);
    }
    return pBlobs->GetBlobNum();
  }

 private:
  std::vector<bgs_box> boxes_;
  std::vector<bgs_moments> moments_;
};
