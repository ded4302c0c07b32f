// vv_proj_xpair.hip -- the projection kernels instantiated on the x-pair copy (handed over in VolumeView::zpair), as vv_mip_xpair.hip.
#define VV_ZPAIR 1
#define VV_XPAIR 1
#include "vv_proj.hip"
