// Stand-in for package_bgs/jmo's blob library: CMultiLayerBGS names it in Postprocessing and GetLayeredBackgroundImage only, which
// the live path never reaches.  Every body aborts.
#pragma once
#include <opencv2/opencv.hpp>
namespace Blob {
enum { B_INCLUDE = 1, B_GREATER = 2 };
struct CBlobGetArea {};
struct CBlob {
  void FillBlob(IplImage*, CvScalar) { cvStandInAbort("CBlob::FillBlob"); }
};
struct CBlobResult {
  CBlobResult() {}
  CBlobResult(IplImage*, IplImage*, int, bool) { cvStandInAbort("CBlobResult"); }
  void Filter(CBlobResult&, int, CBlobGetArea, int, double) { cvStandInAbort("CBlobResult::Filter"); }
  int GetNumBlobs() { cvStandInAbort("CBlobResult::GetNumBlobs"); }
  CBlob GetBlob(int) { cvStandInAbort("CBlobResult::GetBlob"); }
  void GetNthBlob(CBlobGetArea, int, CBlob&) { cvStandInAbort("CBlobResult::GetNthBlob"); }
};
}  // namespace Blob
