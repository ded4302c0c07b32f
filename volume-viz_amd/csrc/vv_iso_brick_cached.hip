// vv_iso_brick_cached.hip -- vv_iso_brick.hip once more for volumes that live in the caches (namespace brickc, compiled without the
// SLP vectoriser), as vv_raymarch_brick_cached.hip.
#define VV_BRICKED 1
#define VV_BRICKED_CACHED 1
#include "vv_iso.hip"
