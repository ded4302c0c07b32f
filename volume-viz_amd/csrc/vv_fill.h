// vv_fill.h -- the fill blocks of march_kernel: which pixels the blocks appended behind the marching blocks of a composite unshaded frame set to 0
// (internal; included from vv_kernels.h).
//
// The pixels of such a frame that lie beside the screen rectangle of the volume hold 0: their rays miss it.  Nobody reads them and nothing orders them
// against the march, so they are written by blocks of the march launch itself instead of by the pre-pass in front of it.  The rule for a pixel is
// rad_kernel's: x <= W-2, y <= H-2, the row is owned (vv_device.h: row_owned), and the pixel is not inside the rectangle.  What is enumerated is the
// frame's written area minus the rectangle, cut into at most four pixel regions (above, below, left of and right of the rectangle); a fill block
// takes kFillBlockPixels consecutive pixels of one region in row-major order.  Fill pixels and marching pixels are disjoint by construction: no block
// waits for another.  Everything here compiles for the host as well: host/fill_grid_check.cpp walks whole frames on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vv {

constexpr int kFillBlockPixels = 4096;          // per block: 256 threads x 16 pixels, a thread's pixels 256 apart (C3: 316 fill blocks for 5.1 MB of zeros)
constexpr int kFillSlab = 14;                   // = kSlab (vv_device.h): row ownership is decided per slab row

struct FillRegion { int x, y, w, h; };          // pixels [x, x + w) x [y, y + h)
struct FillMap {
    uint32_t first;                             // the launch's first fill block (= the number of marching blocks); no fill blocks: ~0u
    int W, H;                                   // the frame (pixel pitch W; column W-1 and row H-1 are never written)
    int x0, x1, y0, y1;                         // the rectangle the marching blocks cover (PixelRect)
    int rb, re, band, count, index;             // row ownership (FrameParams)
    FillRegion reg[4];
    int end[4];                                 // blocks of regions 0 .. r together (end[3] = all fill blocks)
};

#define VV_FILL __host__ __device__ __forceinline__

// Does a fill block write pixel (x, y) of the frame?
VV_FILL bool fill_writes(const FillMap &F, int x, int y)
{
    const int r = y / kFillSlab;
    const bool owned = r >= F.rb && r < F.re && (F.count <= 1 || ((r / F.band) % F.count) == F.index);
    return x <= F.W - 2 && y <= F.H - 2 && owned && !(x >= F.x0 && x < F.x1 && y >= F.y0 && y < F.y1);
}

// The regions of a frame and their blocks.  [ya, yb): the pixel rows from the first owned one to the last (a row range: exactly the owned ones; a
// shard: fill_writes sorts out the other ranks' bands between them).  Returns the number of fill blocks (0: every owned pixel lies inside the rectangle).
// (BP: the pixels of a block, a multiple of 256 -- kFillBlockPixels everywhere but in host/fill_grid_check.cpp, whose frames are small)
template <int BP = kFillBlockPixels>
VV_FILL int fill_map(FillMap &F, int W, int H, int x0, int x1, int y0, int y1, int rb, int re, int band, int count, int index)
{
    F.first = ~0u; F.W = W; F.H = H; F.x0 = x0; F.x1 = x1; F.y0 = y0; F.y1 = y1;
    F.rb = rb; F.re = re; F.band = band; F.count = count; F.index = index;
    const int xe = W - 1;
    // from the first owned pixel row to behind the last one (host only: a walk over the frame's slab rows)
    int ya = 0, yb = 0;
    {
        const int nrows = H >= 2 ? (H - 2) / kFillSlab + 1 : 0;           // slab rows that hold written pixel rows
        int r_first = -1, r_last = -1;
        for (int r = rb > 0 ? rb : 0; r < re && r < nrows; ++r)
            if (count <= 1 || ((r / band) % count) == index) { if (r_first < 0) r_first = r; r_last = r; }
        if (r_first >= 0) { ya = r_first * kFillSlab; yb = (r_last + 1) * kFillSlab < H - 1 ? (r_last + 1) * kFillSlab : H - 1; }
    }
    // the rectangle clamped to [0, xe) x [ya, yb)
    const int cx0 = x0 < 0 ? 0 : (x0 > xe ? xe : x0), cx1 = x1 < cx0 ? cx0 : (x1 > xe ? xe : x1);
    const int cy0 = y0 < ya ? ya : (y0 > yb ? yb : y0), cy1 = y1 < cy0 ? cy0 : (y1 > yb ? yb : y1);
    const bool empty = cx1 == cx0 || cy1 == cy0;            // (nothing of the rectangle in the written area: one region takes it all)
    const FillRegion above = {0, ya, xe, (empty ? yb : cy0) - ya}, below = {0, cy1, xe, empty ? 0 : yb - cy1};
    const FillRegion left = {0, cy0, cx0, empty ? 0 : cy1 - cy0}, right = {cx1, cy0, xe - cx1, empty ? 0 : cy1 - cy0};
    F.reg[0] = above; F.reg[1] = below; F.reg[2] = left; F.reg[3] = right;
    int n = 0;
    for (int r = 0; r < 4; ++r) {
        const long long px = F.reg[r].w > 0 && F.reg[r].h > 0 ? (long long)F.reg[r].w * F.reg[r].h : 0;
        n += (int)((px + BP - 1) / BP);
        F.end[r] = n;
    }
    return n;
}

// Pixel k (0 .. BP / 256 - 1) of thread `thread` of fill block `b` (0 .. end[3] - 1); false: beyond the end of the block's region.
template <int BP = kFillBlockPixels>
VV_FILL bool fill_pixel(const FillMap &F, int b, int thread, int k, int &x, int &y)
{
    const int r = (b >= F.end[0] ? 1 : 0) + (b >= F.end[1] ? 1 : 0) + (b >= F.end[2] ? 1 : 0);
    const int start = r == 0 ? 0 : (r == 1 ? F.end[0] : (r == 2 ? F.end[1] : F.end[2]));
    const int rx = r == 0 ? F.reg[0].x : (r == 1 ? F.reg[1].x : (r == 2 ? F.reg[2].x : F.reg[3].x));
    const int ry = r == 0 ? F.reg[0].y : (r == 1 ? F.reg[1].y : (r == 2 ? F.reg[2].y : F.reg[3].y));
    const int rw = r == 0 ? F.reg[0].w : (r == 1 ? F.reg[1].w : (r == 2 ? F.reg[2].w : F.reg[3].w));
    const int rh = r == 0 ? F.reg[0].h : (r == 1 ? F.reg[1].h : (r == 2 ? F.reg[2].h : F.reg[3].h));
    const uint32_t i = (uint32_t)(b - start) * (uint32_t)BP + (uint32_t)k * 256u + (uint32_t)thread;       // (a region holds fewer than 2^31 pixels: W * H of a frame does)
    if (i >= (uint32_t)rw * (uint32_t)rh) return false;
    x = rx + (int)(i % (uint32_t)rw); y = ry + (int)(i / (uint32_t)rw);
    return true;
}

#undef VV_FILL

} // namespace vv
