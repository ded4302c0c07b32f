// vv_proj_brick.hip -- the projection kernels instantiated on the bricked copy of the volume (VolumeView::bricks), as vv_mip_brick.hip.
#define VV_BRICKED 1
#include "vv_proj.hip"
