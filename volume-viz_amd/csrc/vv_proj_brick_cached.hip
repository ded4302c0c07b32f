// vv_proj_brick_cached.hip -- vv_proj_brick.hip once more for volumes that live in the caches (namespace brickc, compiled without the
// SLP vectoriser), as vv_mip_brick_cached.hip.
#define VV_BRICKED 1
#define VV_BRICKED_CACHED 1
#include "vv_proj.hip"
