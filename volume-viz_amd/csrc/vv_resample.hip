// vv_resample.hip -- the loaded volume sampled on another grid for gfx950: every voxel of an output grid is the trilinear (or nearest) sample of the
// volume at an affinely mapped position, written as a dense volume (no reference counterpart; the contract is the comment on vv_resample_volume
// in include/volviz.h).
//
//   resample_kernel<SRC, OUT, FILTER, BIG>     one launch per call; BIG: the 64-bit slice bases of volumes above 4 GiB (LAYOUT_LINEAR_BIG)
//
// Work.  The box of the output grid is cut into tiles of kRsTX x resample_tile_y() x kRsTZ = 32 x 8 x 4 voxels (u8 sources, NEAREST) or 32 x 4 x 4
// (trilinear samples of f32 sources).  A block of four waves takes a tile: wave w takes the tile's plane w, its lanes lie 8 x 8
// (16 x 4) over the plane and each owns 4 (2) voxels consecutive in x.  This is the first gather among the volume-to-volume kernels: writes are
// dense whatever the matrix, reads follow the mapped lattice.  A wave's plane of outputs maps onto a parallelogram of the source whose lines
// are shared along both of its sides, and the four waves of the block add the third direction, so a source line fetched by one lane serves
// its neighbours in all three out of the CU's L1.
// Order.  Tiles are numbered x fastest, then y, then z; one block per tile (VV_RESAMPLE_BLOCKS caps the grid; the loop then takes blockIdx.x,
// + gridDim.x, ...).  Blocks are dealt to the part's eight XCDs round-robin by blockIdx.x, and each XCD has an L2 of its own: item i is tile
// (i % 8) * chunk + i / 8 with chunk = ceil(tiles / 8), so that the blocks of one XCD walk one contiguous eighth of the tiles and neighbouring
// tiles, which share source lines, meet in one L2 (for any gridDim.x that is a multiple of 8; any other is correct and merely loses the locality).
// Sampling is the texture model of vv_device.h, not restated: fetch_corners issues the loads of a sample, finish_corners turns them into the
// value.  A lane issues the loads of all its samples before it finishes the first.  Coordinates are clamped where fetch_corners makes the
// address; a sample outside [0, 1)^3 loads nothing and takes `fill`.  NEAREST addresses one voxel by min((uint32_t)(p n), n - 1) per axis.
// Each output voxel has one writer: no atomics, no LDS.  A lane whose voxels all lie in the box and start on a boundary of their size together
// (16 or 8 bytes of f32, 4 or 2 of u8) stores them at once; the row's tail and unaligned starts are stored voxel by voxel.  The output offset is formed in 64 bits.
// Arithmetic: binary32 in the contract's order under contract(off); results leave as integer bit patterns.
#include "vv_device.h"
#include "vv_kernels.h"

namespace vv {

// Output voxels per lane, consecutive in x (1, 2 or 4), and with them the wave's plane of the tile: 32 x 8 with four voxels per lane, 32 x 4 with two.
// Measured: trilinear samples of an f32 volume, whose four corner pairs are 32 bytes of loads in flight per voxel, run
// 14-23 % faster with two; u8 sources (dword loads shared by neighbouring voxels) and NEAREST (one load per voxel) with four.  -DVV_RESAMPLE_VPL=n
// forces one value on every instantiation (experiment knob).
constexpr int resample_vpl(int src_type, int filter)
{
#ifdef VV_RESAMPLE_VPL
    return VV_RESAMPLE_VPL;
#else
    return (src_type == VV_VOXEL_F32 && filter != VV_RESAMPLE_NEAREST) ? 2 : 4;
#endif
}
#ifndef VV_RESAMPLE_XCD
#define VV_RESAMPLE_XCD 1            // 0: item i is tile i (experiment knob)
#endif
#ifndef VV_RESAMPLE_ORDER
#define VV_RESAMPLE_ORDER 0          // 1: tiles numbered in groups of 4 x 4 x 4 (experiment knob)
#endif
constexpr int kRsTX = 32, kRsTZ = 4;                                    // the tile: a wave's plane of 32 x resample_tile_y(), four waves in z
constexpr int resample_tile_y(int vpl) { return 64 / (kRsTX / vpl); }   // 8 rows with four voxels per lane, 4 with two
constexpr int kRsThreads = 64 * kRsTZ;
constexpr int kRsXcds = 8;

struct ResampleKernelArgs {
    ResampleArgs R;
    uint32_t ntx, plane;            // tiles per row of tiles, per plane of tiles
    uint64_t tiles, chunk, items;   // tiles of the box; tiles per XCD; items = kRsXcds * chunk
};

__device__ __forceinline__ bool resample_inside(float x, float y, float z)      // slice_kernel's test (vv_aux.hip): false for a NaN, true for -0
{
    return x < 1.0f && x >= 0.0f && y < 1.0f && y >= 0.0f && z < 1.0f && z >= 0.0f;
}
__device__ __forceinline__ uint32_t resample_nearest(float p, int n)
{
#pragma clang fp contract(off)
    return min((uint32_t)(p * (float)n), (uint32_t)(n - 1));
}

template <int SRC, int OUT, int FILTER, bool BIG>
__global__ __launch_bounds__(kRsThreads) void resample_kernel(ResampleKernelArgs A)
{
#pragma clang fp contract(off)
    constexpr bool F32 = SRC == VV_VOXEL_F32, OF32 = OUT == VV_VOXEL_F32, NEAREST = FILTER == VV_RESAMPLE_NEAREST;
    constexpr int SIZE = F32 ? 4 : 1, OSIZE = OF32 ? 4 : 1;
    constexpr int VPL = resample_vpl(SRC, FILTER), LANES_X = kRsTX / VPL, TILE_Y = resample_tile_y(VPL);
    static_assert(VPL == 1 || VPL == 2 || VPL == 4, "a lane stores 1, 2 or 4 voxels at once");
    const ResampleArgs &R = A.R;
    const VolumeView &V = R.V;
    const uint32_t lane = threadIdx.x & 63u, wz = threadIdx.x >> 6;
    const uint32_t lx = lane % LANES_X, ly = lane / LANES_X;
    const uint32_t fill_out = voxel_out<F32, OF32>(R.fill);

    for (uint64_t i = blockIdx.x; i < A.items; i += gridDim.x) {
#if VV_RESAMPLE_XCD
        const uint64_t tile = (i % kRsXcds) * A.chunk + i / kRsXcds;
#else
        const uint64_t tile = i;
#endif
        if (tile >= A.tiles) continue;
#if VV_RESAMPLE_ORDER
        // groups of 4 x 4 x 4 tiles, x fastest inside a group and among the groups (ntx, plane: groups per row and per plane of groups; tiles past the box fall out below)
        const uint64_t grp = tile >> 6;
        const uint32_t sub = (uint32_t)tile & 63u, gz = (uint32_t)(grp / A.plane), grem = (uint32_t)(grp - (uint64_t)gz * A.plane), gy = grem / A.ntx, gx = grem - gy * A.ntx;
        const uint32_t tx = gx * 4 + (sub & 3u), ty = gy * 4 + ((sub >> 2) & 3u), tz = gz * 4 + (sub >> 4);
#else
        const uint32_t tz = (uint32_t)(tile / A.plane), rem = (uint32_t)(tile - (uint64_t)tz * A.plane), ty = rem / A.ntx, tx = rem - ty * A.ntx;
#endif
        const uint32_t ox = tx * kRsTX + lx * VPL, oy = ty * TILE_Y + ly, oz = tz * kRsTZ + wz;       // the lane's first voxel, in the box
        if (ox >= R.b[0] || oy >= R.b[1] || oz >= R.b[2]) continue;
        const uint32_t nvox = min((uint32_t)VPL, R.b[0] - ox);
        // rule 1: q of the grid's voxel, p = ((m0 q_x + m1 q_y) + m2 q_z) + m3
        const float qy = ((float)(R.lo[1] + (int)oy) + 0.5f) * R.inv[1], qz = ((float)(R.lo[2] + (int)oz) + 0.5f) * R.inv[2];
        const float ay[3] = {R.m[1] * qy, R.m[5] * qy, R.m[9] * qy}, az[3] = {R.m[2] * qz, R.m[6] * qz, R.m[10] * qz};
        bool in[VPL];
        uint32_t raw[VPL];
        Corners<SRC> Cn[VPL];
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            in[k] = false;
            if ((uint32_t)k < nvox) {
                const float qx = ((float)(R.lo[0] + (int)ox + k) + 0.5f) * R.inv[0];
                const float px = ((R.m[0] * qx + ay[0]) + az[0]) + R.m[3];
                const float py = ((R.m[4] * qx + ay[1]) + az[1]) + R.m[7];
                const float pz = ((R.m[8] * qx + ay[2]) + az[2]) + R.m[11];
                in[k] = resample_inside(px, py, pz);
                if (in[k]) {
                    if constexpr (NEAREST) {
                        const uint32_t ix = resample_nearest(px, V.nx), iy = resample_nearest(py, V.ny), iz = resample_nearest(pz, V.nz);
                        const char *at = (const char *)V.data + ((uint64_t)iz * V.slice_bytes + (uint64_t)iy * V.row_bytes + (uint64_t)ix * SIZE);
                        if constexpr (F32) raw[k] = *(const uint32_t *)at; else raw[k] = (uint32_t)*(const uint8_t *)at;
                    } else {
                        fetch_corners<SRC, FILTER == VV_RESAMPLE_TEX8, BIG ? LAYOUT_LINEAR_BIG : LAYOUT_LINEAR>(V, px, py, pz, Cn[k]);
                    }
                }
            }
        }
        uint32_t v[VPL];
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            v[k] = fill_out;
            if (in[k]) {
                if constexpr (NEAREST) v[k] = voxel_out_copy<F32, OF32>(raw[k]);
                else v[k] = voxel_out<F32, OF32>(finish_corners<SRC>(Cn[k]));
            }
        }
        char *at = (char *)R.out + (((uint64_t)oz * R.b[1] + oy) * R.b[0] + ox) * OSIZE;
        if (VPL > 1 && nvox == (uint32_t)VPL && ((uintptr_t)at & (uintptr_t)(VPL * OSIZE - 1)) == 0) {
            if constexpr (VPL == 4) {
                if constexpr (OF32) *(uint4 *)at = make_uint4(v[0], v[1], v[2], v[3]);
                else *(uint32_t *)at = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else if constexpr (VPL == 2) {
                if constexpr (OF32) *(uint2 *)at = make_uint2(v[0], v[1]);
                else *(uint16_t *)at = (uint16_t)(v[0] | (v[1] << 8));
            }
        } else {
#pragma unroll
            for (int k = 0; k < VPL; ++k)
                if ((uint32_t)k < nvox) {
                    if constexpr (OF32) *(uint32_t *)(at + k * 4) = v[k]; else *(uint8_t *)(at + k) = (uint8_t)v[k];
                }
        }
    }
}

// The grid: one block per item, unless `max_blocks` caps it (or the items outnumber a grid: 2^31 - 1); the loop over items takes the rest.  A grid of
// as many blocks as the part holds at once, each looping over its share, was measured and lost.
template <class K>
static void launch_resample_kernel(K kernel, const ResampleKernelArgs &a, int n_cu, int max_blocks, hipStream_t s)
{
    (void)n_cu;
    uint64_t grid = a.items;
    if (max_blocks > 0 && grid > (uint64_t)max_blocks) grid = (uint64_t)max_blocks;
    if (grid > 0x7FFFFFFFull) grid = 0x7FFFFFFFull;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kRsThreads), 0, s, a);
}
template <int SRC, int OUT, int FILTER>
static void launch_resample_big(const ResampleKernelArgs &a, int n_cu, int max_blocks, hipStream_t s)
{
    if constexpr (FILTER != VV_RESAMPLE_NEAREST) {
        if (a.R.V.big) { launch_resample_kernel(resample_kernel<SRC, OUT, FILTER, true>, a, n_cu, max_blocks, s); return; }
    }
    launch_resample_kernel(resample_kernel<SRC, OUT, FILTER, false>, a, n_cu, max_blocks, s);      // (NEAREST forms its one address in 64 bits on every volume)
}
template <int SRC, int OUT>
static void launch_resample_filter(const ResampleKernelArgs &a, int n_cu, int max_blocks, hipStream_t s)
{
    switch (a.R.filter) {
        case VV_RESAMPLE_TEX8:  launch_resample_big<SRC, OUT, VV_RESAMPLE_TEX8>(a, n_cu, max_blocks, s); break;
        case VV_RESAMPLE_EXACT: launch_resample_big<SRC, OUT, VV_RESAMPLE_EXACT>(a, n_cu, max_blocks, s); break;
        default:                launch_resample_big<SRC, OUT, VV_RESAMPLE_NEAREST>(a, n_cu, max_blocks, s); break;
    }
}

void launch_resample(const ResampleArgs &r, int n_cu, int max_blocks, hipStream_t s)
{
    ResampleKernelArgs a;
    a.R = r;
    const uint32_t ty = (uint32_t)resample_tile_y(resample_vpl(r.src_type, r.filter));
    const uint32_t g = VV_RESAMPLE_ORDER ? 4 : 1;                       // tiles per group and axis
    a.ntx = (r.b[0] + kRsTX * g - 1) / (kRsTX * g);
    a.plane = a.ntx * ((r.b[1] + ty * g - 1) / (ty * g));         // (at most 512 x 2048)
    a.tiles = (uint64_t)a.plane * ((r.b[2] + kRsTZ * g - 1) / (kRsTZ * g)) * (g * g * g);
    a.chunk = (a.tiles + kRsXcds - 1) / kRsXcds;
    a.items = VV_RESAMPLE_XCD ? a.chunk * kRsXcds : a.tiles;
    const bool sf = r.src_type == VV_VOXEL_F32, of = r.out_type == VV_VOXEL_F32;
    if (sf && of)       launch_resample_filter<VV_VOXEL_F32, VV_VOXEL_F32>(a, n_cu, max_blocks, s);
    else if (sf)        launch_resample_filter<VV_VOXEL_F32, VV_VOXEL_U8>(a, n_cu, max_blocks, s);
    else if (of)        launch_resample_filter<VV_VOXEL_U8, VV_VOXEL_F32>(a, n_cu, max_blocks, s);
    else                launch_resample_filter<VV_VOXEL_U8, VV_VOXEL_U8>(a, n_cu, max_blocks, s);
}

} // namespace vv
