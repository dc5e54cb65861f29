// Stand-in for <opencv2/legacy/compat.hpp>: nothing of it is needed beyond opencv.hpp here.
#pragma once
#include "../opencv.hpp"
