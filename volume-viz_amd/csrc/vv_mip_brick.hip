// vv_mip_brick.hip -- the MIP kernels instantiated on the bricked copy of the volume (VolumeView::bricks), as vv_raymarch_brick.hip.
#define VV_BRICKED 1
#include "vv_mip.hip"
