// vv_iso_brick.hip -- the isosurface kernels instantiated on the bricked copy of the volume (VolumeView::bricks), as vv_raymarch_brick.hip.
#define VV_BRICKED 1
#include "vv_iso.hip"
