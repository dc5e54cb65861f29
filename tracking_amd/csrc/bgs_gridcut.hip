// bgs_gridcut.hip — the third translation unit of libbgs_hip.so: the grid min-cut and the mask painting of the LbpMrf mask stage
// (kernel_gridcut.h) and the launch calls of gridcut.h, which bgs_lbpmrf_mask_device (bgs_hip.hip) uses.  Kept apart from
// bgs_hip.hip so that the code object of every other kernel is built exactly as before.
#include "kernel_gridcut.h"
