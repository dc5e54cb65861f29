// <opencv/cvaux.h> for MotionDetection.cpp: the same stand-in
#pragma once
#include "../opencv2/opencv.hpp"
