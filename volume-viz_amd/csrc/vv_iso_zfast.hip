// vv_iso_zfast.hip -- the isosurface kernels instantiated on the z-fastest copy (VolumeView::zfast), as vv_raymarch_zfast.hip.
#define VV_ZFAST 1
#include "vv_iso.hip"
