// vv_iso_xpair.hip -- the isosurface kernels instantiated on the x-pair copy (handed over in VolumeView::zpair), as vv_raymarch_xpair.hip.
#define VV_ZPAIR 1
#define VV_XPAIR 1
#include "vv_iso.hip"
