// vv_proj_big.hip -- the projection kernels instantiated for volumes above 4 GiB (64-bit slice base per sample), as vv_mip_big.hip.
#define VV_BIG_VOLUME 1
#include "vv_proj.hip"
