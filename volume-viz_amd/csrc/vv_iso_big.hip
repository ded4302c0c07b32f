// vv_iso_big.hip -- the isosurface kernels instantiated for volumes above 4 GiB (64-bit slice base per sample), as vv_raymarch_big.hip.
#define VV_BIG_VOLUME 1
#include "vv_iso.hip"
