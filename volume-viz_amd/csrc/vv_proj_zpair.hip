// vv_proj_zpair.hip -- the projection kernels instantiated on the z-pair copy (VolumeView::zpair), as vv_mip_zpair.hip.
#define VV_ZPAIR 1
#include "vv_proj.hip"
