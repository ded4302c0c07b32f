// tile_grid_check -- walks the tile grid of march_kernel / mip_kernel (csrc/vv_tiles.h) on the CPU, with the functions the kernels, their launchers and
// rad_kernel's table writer use.  For a set of small launches: every (strip, tile column) of the launch comes up in exactly one block, no block reads
// beyond the order table, and the 256 threads of a block own 256 distinct pixels of the block's rectangle.  No HIP call.  Exit status 0 / 1.
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>
#include "../csrc/vv_tiles.h"

using namespace vv;

static int failures = 0;
static void fail(const StripMap &M, const char *what, long a = 0, long b = 0)
{
    ++failures;
    printf("FAIL %s (%ld, %ld): wr %d strips [%d, %d) run %d (table %s) xcd_band %d tile_log2w %d blk_log2w %d strips_per_band %d\n", what, a, b,
           M.wr, M.s0, M.s1, M.order_run, M.order ? "yes" : "no", M.xcd_band, M.tile_log2w, M.blk_log2w, M.strips_per_band);
}

// the table a launch reads: order_words words, written through order_slot from a shuffled ranking of the units (rank k: the (k / 8)-th unit of XCD k % 8).
// Units and their tiles are restated here (runs of order_run tiles of a row, the last one of a row shorter), not taken from the header.
static std::vector<uint32_t> make_order(const StripMap &M, std::mt19937 &rng)
{
    std::vector<uint32_t> table((size_t)order_words(M), ~0u);
    const int run = M.order_run, nseg = (M.wr + run - 1) / run;
    std::vector<int> rank((size_t)((M.s1 - M.s0) * nseg));
    if ((int)rank.size() != order_units(M)) fail(M, "order_units", order_units(M), (long)rank.size());
    for (size_t u = 0; u < rank.size(); ++u) rank[u] = (int)u;
    std::shuffle(rank.begin(), rank.end(), rng);
    for (size_t u = 0; u < rank.size(); ++u) {
        const int col0 = ((int)u % nseg) * run, t0 = ((int)u / nseg) * M.wr + col0, count = std::min(run, M.wr - col0);
        for (int i = 0; i < count; ++i) {
            const int slot = order_slot(M, rank[u] >> 3, rank[u] & 7, i);
            if (slot < 0 || slot >= (int)table.size() || table[(size_t)slot] != ~0u) { fail(M, "slot written twice or outside the table", slot, (long)table.size()); continue; }
            table[(size_t)slot] = (uint32_t)(t0 + i);
        }
    }
    return table;
}

static void check(StripMap M, std::mt19937 &rng)
{
    std::vector<uint32_t> table;
    if (M.order_run > 0) { table = make_order(M, rng); M.order = table.data(); } else { M.order = nullptr; M.order_run = 1; }
    std::set<std::pair<int, int>> seen;
    const unsigned nblocks = grid_blocks(M);
    for (unsigned L = 0; L < nblocks; ++L) {
        if (M.order) {                                                 // the slot block_tile is about to read, against the storage there is
            const long slot = order_slot(M, (int)(L >> 3) / M.order_run, (int)(L & 7), (int)(L >> 3) % M.order_run);
            if (slot < 0 || slot >= (long)table.size()) { fail(M, "block reads beyond the table", L, slot); continue; }
        }
        int strip, tile_x;
        if (!block_tile(M, L, strip, tile_x) || strip >= M.s1) continue;
        if (strip < M.s0 || tile_x < M.tx0 || tile_x >= M.tx0 + M.wr) fail(M, "tile outside the launch", strip, tile_x);
        if (!seen.insert({strip, tile_x}).second) fail(M, "tile marched twice", strip, tile_x);
        const int bw = 1 << M.blk_log2w, bh = 256 >> M.blk_log2w, x0 = tile_x * bw, y0 = strip_row(M, strip);
        std::set<std::pair<int, int>> px;
        for (int t = 0; t < 256; ++t) {
            int x, y;
            tile_pixel(M, strip, tile_x, t, x, y);
            if (x < x0 || x >= x0 + bw || y < y0 || y >= y0 + bh) fail(M, "pixel outside its block", x, y);
            px.insert({x, y});
        }
        if (px.size() != 256) fail(M, "threads of a block share pixels", L, (long)px.size());
    }
    if ((long)seen.size() != (long)M.wr * (M.s1 - M.s0)) fail(M, "tiles marched / tiles of the launch", (long)seen.size(), (long)M.wr * (M.s1 - M.s0));
}

int main()
{
    std::mt19937 rng(20251018);
    int maps = 0;
    for (int tw = 3; tw <= 5; ++tw)
        for (int bl = 3; bl <= 7; ++bl) {
            if (bl != 5 && !(bl >= tw && (256 >> bl) >= (64 >> tw))) continue;      // choose_launch: a block is at least one wave tile wide and high
            for (int wr : {1, 5, 7, 17}) for (int ns : {1, 3, 9}) for (int banded = 0; banded < 2; ++banded)
                for (int order : {0, 1, 5, 64}) for (int xb : {0, 1, 3}) {
                    if (order && xb) continue;                                      // (a launch with a table does not look at xcd_band)
                    StripMap M = {};
                    M.tile_log2w = tw; M.blk_log2w = bl; M.tx0 = 3; M.wr = wr; M.s0 = 2; M.s1 = 2 + ns; M.n_strips = 2 + ns + 1;
                    M.y0 = banded ? 28 : 5; M.strips_per_band = banded ? 7 : 1 << 28; M.band_stride_px = banded ? 3 * 7 * (256 >> bl) : 0;
                    M.xcd_band = xb; M.order_run = order;
                    check(M, rng); ++maps;
                }
        }
    printf("%d launches walked, %d failures\n", maps, failures);
    return failures ? 1 : 0;
}
