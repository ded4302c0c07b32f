// fill_grid_check -- walks the fill blocks of march_kernel (csrc/vv_fill.h) on the CPU, with the functions the kernel and render_frame use.  For small
// frames, every block and wave-tile shape the launch policy reaches, rectangles of every kind and every way a frame can be owned: each owned pixel
// outside the rectangle is written by exactly one fill block and no other pixel is written at all.  The expectation is restated here from rad_kernel's
// rule (the pixels rad_kernel writes when there are no fill blocks), not taken from the header.  No HIP call.  Exit status 0 / 1.
#include <cstdio>
#include <vector>
#include "../csrc/vv_fill.h"

using namespace vv;

static long failures = 0, frames = 0, blocks_walked = 0;
struct Own { int rb, re, band, count, index; };

static void fail(const char *what, int W, int H, const int r[4], const Own &o, long a, long b)
{
    if (++failures <= 40)
        printf("FAIL %s (%ld, %ld): frame %d x %d rect [%d, %d) x [%d, %d) rows [%d, %d) band %d rank %d of %d\n", what, a, b, W, H, r[0], r[1], r[2], r[3],
               o.rb, o.re, o.band, o.index, o.count);
}

// rad_kernel's rule, restated: column W-1 and row H-1 are never written; a row belongs to its slab row of 14; slab rows [rb, re) of a row range, the
// bands of `band` slab rows dealt to the ranks in turn
static bool expected(int W, int H, const int r[4], const Own &o, int x, int y)
{
    if (x > W - 2 || y > H - 2) return false;
    const int slab_row = y / 14;
    if (slab_row < o.rb || slab_row >= o.re) return false;
    if ((slab_row / o.band) % o.count != o.index) return false;
    return !(x >= r[0] && x < r[1] && y >= r[2] && y < r[3]);
}

template <int BP>
static void check_bp(int W, int H, const int r[4], const Own &o)
{
    FillMap F;
    const int n = fill_map<BP>(F, W, H, r[0], r[1], r[2], r[3], o.rb, o.re, o.band, o.count, o.index);
    ++frames;
    if (n < 0 || n != F.end[3]) { fail("block count", W, H, r, o, n, F.end[3]); return; }
    std::vector<int> written((size_t)W * H, 0);
    for (int b = 0; b < n; ++b, ++blocks_walked)
        for (int t = 0; t < 256; ++t)
            for (int k = 0; k < BP / 256; ++k) {
                int x = -1, y = -1;
                if (!fill_pixel<BP>(F, b, t, k, x, y) || !fill_writes(F, x, y)) continue;
                if (x < 0 || x >= W || y < 0 || y >= H) { fail("store outside the frame", W, H, r, o, x, y); continue; }
                ++written[(size_t)y * W + x];
            }
    long want = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const bool e = expected(W, H, r, o, x, y);
            want += e;
            if (written[(size_t)y * W + x] != (e ? 1 : 0)) fail(e ? "owned pixel outside the rectangle not written once" : "pixel written that is not the fill's", W, H, r, o, x, y);
        }
    if ((n != 0) != (want != 0)) fail("fill blocks / pixels to fill", W, H, r, o, n, want);
}

// the product's block size (one block per region in frames this small) and two small ones (many blocks per region, the last one partly beyond its end)
static void check(int W, int H, const int r[4], const Own &o)
{
    check_bp<kFillBlockPixels>(W, H, r, o); check_bp<256>(W, H, r, o); check_bp<768>(W, H, r, o);
}

int main()
{
    // every block shape choose_launch reaches (2^bl x (256 >> bl) pixels; the wave-tile shapes 8 x 8, 16 x 4 and 32 x 2 tile them and do not change the
    // rectangle): the rectangle is made of whole blocks, tiles_under_rect's way
    const int frame_w[] = {2, 3, 15, 16, 29, 33, 70}, frame_h[] = {2, 3, 15, 16, 29, 43, 45};
    for (int W : frame_w) for (int H : frame_h)
        for (int tw = 3; tw <= 5; ++tw) for (int bl = 3; bl <= 7; ++bl) {
            if (bl != 5 && !(bl >= tw && (256 >> bl) >= (64 >> tw))) continue;
            const int bw = 1 << bl, bh = 256 >> bl, nby = (H + 13) / 14;
            const int ntx = (W + bw - 1) / bw;
            // ownership: the whole frame, row ranges, shards of 2 and 3 ranks (bands of 4 slab rows, the smallest the API takes)
            std::vector<Own> owns = {{0, nby, 4, 1, 0}};
            if (nby >= 2) { owns.push_back({1, nby, 4, 1, 0}); owns.push_back({0, nby - 1, 4, 1, 0}); }
            if (nby >= 3) owns.push_back({1, 2, 4, 1, 0});
            for (int count = 2; count <= 3; ++count) for (int index = 0; index < count; ++index) owns.push_back({0, nby, 4, count, index});
            for (const Own &o : owns) {
                const int ya = o.count > 1 ? 0 : o.rb * 14;                       // StripMap::y0 of the launch
                const int nst = o.count > 1 ? (H + bh - 1) / bh : ((o.re * 14 < H - 1 ? o.re * 14 : H - 1) - ya + bh - 1) / bh;
                // tile columns [c0, c1) x strips [s0, s1): inside, touching each edge, covering the frame, and empty
                const int cols[][2] = {{0, ntx}, {0, 1}, {ntx - 1, ntx}, {ntx / 2, ntx / 2 + 1}, {1, ntx > 2 ? ntx - 1 : ntx}, {0, 0}};
                const int rows[][2] = {{0, nst}, {0, 1}, {nst - 1, nst}, {nst / 2, nst / 2 + 1}, {1, nst > 2 ? nst - 1 : nst}, {0, 0}};
                for (const auto &c : cols) for (const auto &s : rows) {
                    if (c[0] < 0 || c[1] < c[0] || s[0] < 0 || s[1] < s[0]) continue;
                    int r[4] = {c[0] * bw, c[1] * bw, ya + s[0] * bh, ya + s[1] * bh};
                    if (o.count > 1) { r[2] = 0; r[3] = 0x7fffffff; }                 // a shard's rectangle limits columns only
                    if (c[1] == c[0] || s[1] == s[0]) r[0] = r[1] = r[2] = r[3] = 0;   // the cube is off the screen
                    check(W, H, r, o);
                }
            }
        }
    // no rectangle at all (x1 = y1 = INT_MAX): nothing to fill
    { const int r[4] = {0, 0x7fffffff, 0, 0x7fffffff}; check(70, 45, r, {0, 4, 4, 1, 0}); }
    printf("%ld frames, %ld fill blocks walked, %ld failures\n", frames, blocks_walked, failures);
    return failures ? 1 : 0;
}
