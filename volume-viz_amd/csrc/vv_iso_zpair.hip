// vv_iso_zpair.hip -- the isosurface kernels instantiated on the z-pair copy (VolumeView::zpair), as vv_raymarch_zpair.hip.
#define VV_ZPAIR 1
#include "vv_iso.hip"
