// vv_mip_zfast.hip -- the MIP kernels instantiated on the z-fastest copy (VolumeView::zfast), as vv_raymarch_zfast.hip.
#define VV_ZFAST 1
#include "vv_mip.hip"
