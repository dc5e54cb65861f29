// bgs_multicue_box.hip — the second translation unit of libbgs_hip.so: the three kernels of the box stage of SJN_MultiCueBGS
// (kernel_multicue_box.h) and bgs::mc_box_launch, which engine_multicue.h calls.  Kept apart from bgs_hip.hip so that the
// code object of every other kernel is built exactly as before.
#include "kernel_multicue_box.h"
