// vv_tiles.h -- the tile grid of the unshaded march kernels (march_kernel, mip_kernel, iso_kernel, proj_kernel): the one definition of which block marches which tile, which pixel a lane
// of it owns, how many blocks a launch has, and the format of the `order` table (internal; included from vv_kernels.h).
//
// rad_kernel (writer of the table), the four march kernels (its readers), their launchers and render_frame (which sizes the table) all go
// through the functions below.  choose_launch and render_frame's rectangle and tile-order stages fill the map in.  Everything here compiles for the host as well: host/tile_grid_check.cpp walks whole grids on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vv {

// blockIdx.x -> pixel strip and tile column of a shard
struct StripMap { int y0, strips_per_band, band_stride_px, tile_log2w, n_strips, xcd_band;
                  int tail_batch;     // march_kernel: chunks that hold at most one sample per lane (rays past the ERT threshold) are taken U at a time
                  int blk_log2w;      // a block covers 2^blk_log2w x (256 >> blk_log2w) pixels (5: 32 x 8; 32 x 2 tiles also 64 x 4 / 128 x 2, 8 x 8 tiles 16 x 16 / 8 x 32); strips are that high
                  // march_kernel launches the tiles of columns [tx0, tx0 + wr) of strips [s0, s1) only: the tiles under the volume's screen rectangle
                  // (vv_render: screen_rect) -- or all of them: tx0 = 0, wr = tile columns of the frame, s0 = 0, s1 = n_strips
                  int tx0, wr, s0, s1;
                  // order != nullptr: block L marches the tile in slot order_slot(j / order_run, L % 8, j % order_run), j = L / 8, of a table that
                  // rad_kernel's extra block writes (see there): runs of order_run x-adjacent tiles, sorted by the time their rays spend in the cube and dealt
                  // to the XCDs so that all of them carry the same load and end on their lightest runs (speed only).
                  const uint32_t *order; int order_run; };

#define VV_GRID __host__ __device__ __forceinline__

// ---- pixels ----
// strip -> its first pixel row (strips of a sharded frame lie in bands of strips_per_band, band_stride_px apart)
VV_GRID int strip_row(const StripMap &M, int strip)
{
    return M.y0 + (strip / M.strips_per_band) * M.band_stride_px + (strip % M.strips_per_band) * (256 >> M.blk_log2w);
}
// (strip, tile column, thread of the block) -> pixel.  A wave's tile is 2^tw x 2^(6-tw) pixels; the 4 waves of a block tile its 2^bl x (256 >> bl) rectangle
VV_GRID void tile_pixel(const StripMap &M, int strip, int tile_x, int thread, int &x, int &y)
{
    const int lane = thread & 63, wave = thread >> 6;
    const int bl = M.blk_log2w, tw = M.tile_log2w, th = 6 - tw;
    const int wx = wave & (((1 << bl) >> tw) - 1), wy = wave >> (bl - tw);
    x = (tile_x << bl) + (wx << tw) + (lane & ((1 << tw) - 1));
    y = strip_row(M, strip) + (wy << th) + (lane >> tw);
}

// ---- the order table ----
// The launch's tiles are numbered in raster order, t = row * wr + column.  Units = runs of order_run x-adjacent tiles of a strip (the last run of a strip
// may be shorter), order_units_per_row of them per strip, numbered in raster order too.  rad_kernel's extra block ranks the units and deals them to the 8 XCDs
// in rounds; slot order_slot(r, xcd, i) holds tile i of the r-th unit of that XCD, or ~0 (a unit shorter than a run, the last round).
VV_GRID int order_units_per_row(const StripMap &M) { return (M.wr + M.order_run - 1) / M.order_run; }
VV_GRID int order_units(const StripMap &M) { return (M.s1 - M.s0) * order_units_per_row(M); }
VV_GRID int order_words(const StripMap &M) { return (order_units(M) + 7) / 8 * 8 * M.order_run; }          // whole rounds of 8 units
VV_GRID int order_slot(const StripMap &M, int r, int xcd, int i) { return (r * 8 + xcd) * M.order_run + i; }

// ---- blocks ----
// block -> (strip, tile column); false: the block has nothing to do (an empty slot of the table).  The band order rounds the grid up to 8 whole bands:
// its last blocks come back with strip >= s1, which the kernels test after forming the pixel.
VV_GRID bool block_tile(const StripMap &M, uint32_t block, int &strip, int &tile_x)
{
    const int ntx = M.wr;                                             // the launch covers ntx tile columns from tx0 on
    if (M.order) {
        // block L runs on XCD L % 8 and reads slot order_slot(j / order_run, L % 8, j % order_run), j = L / 8: runs of order_run consecutive tiles of the list
        // go to one XCD, so x-neighbours share an L2 as in the strip order below.  The grid is exactly the table.
        const int L = (int)block, xcd = L & 7, j = L >> 3;
        const uint32_t t = M.order[order_slot(M, j / M.order_run, xcd, j % M.order_run)];
        if (t == ~0u) return false;
        strip = M.s0 + (int)t / ntx; tile_x = M.tx0 + (int)t % ntx;
    } else if (M.xcd_band > 0) {
        // XCD-aware order (speed only): linear block L runs on XCD L % 8 (round-robin dispatch);
        // XCD k walks bands k, k+8, ... of xcd_band strips so that neighbouring tiles share an L2
        const int L = (int)block, per_band = ntx * M.xcd_band;
        const int xcd = L & 7, j = L >> 3;
        const int band = (j / per_band) * 8 + xcd, w = j % per_band;
        strip = M.s0 + band * M.xcd_band + w / ntx; tile_x = M.tx0 + w % ntx;
    } else { strip = M.s0 + block / ntx; tile_x = M.tx0 + block % ntx; }
    return true;
}
// the number of blocks a launch has (0: nothing to launch)
VV_GRID unsigned grid_blocks(const StripMap &M)
{
    const int ntx = M.wr, ns = M.s1 - M.s0;
    if (ntx <= 0 || ns <= 0) return 0;
    if (M.order) return (unsigned)order_words(M);
    if (M.xcd_band > 0) {
        const int nbands = (ns + M.xcd_band - 1) / M.xcd_band;
        return (unsigned)(((nbands + 7) / 8) * 8 * M.xcd_band * ntx);
    }
    return (unsigned)(ns * ntx);
}

#undef VV_GRID

} // namespace vv
