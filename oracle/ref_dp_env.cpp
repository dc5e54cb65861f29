// Part of ref_dp_cli (TEST INFRASTRUCTURE ONLY): includes exactly what dp/GrimsonGMM.cpp includes (GrimsonGMM.h -> Bgs.h ->
// Image.h -> the stand-in opencv2/opencv.hpp) and reports which overload its unqualified sqrt(float) resolves to there.
#include "GrimsonGMM.h"

template <class T> struct SqrtResult;
template <> struct SqrtResult<float> { static const char* name() { return "float"; } };
template <> struct SqrtResult<double> { static const char* name() { return "double"; } };

const char* ref_dp_sqrt_overload() { return SqrtResult<decltype(sqrt(1.0f))>::name(); }
