// vv_proj_zfast.hip -- the projection kernels instantiated on the z-fastest copy (VolumeView::zfast), as vv_mip_zfast.hip.
#define VV_ZFAST 1
#include "vv_proj.hip"
