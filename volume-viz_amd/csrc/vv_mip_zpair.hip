// vv_mip_zpair.hip -- the MIP kernels instantiated on the z-pair copy (VolumeView::zpair), as vv_raymarch_zpair.hip.
#define VV_ZPAIR 1
#include "vv_mip.hip"
