// vv_distance.hip -- the exact squared Euclidean distance transform of a box of the loaded volume for gfx950 (no reference counterpart; the contract
// is the comment on vv_distance_volume in include/volviz.h).
//
//   distance_x_kernel<SRC>        every row of the box: out = (spacing_x * distance to the nearest seed of the row)^2, or the no-seed marker
//   distance_line_kernel<NCAP>    every line along y (second launch) or z (third launch): out[u] = min over j of g[j] + (w (u - j))^2, in place;
//                                 the third launch also applies VV_DIST_WITHIN's threshold
//
// Representation.  i = ((z - lo_z) b_y + (y - lo_y)) b_x + (x - lo_x) numbers the box's voxels, x fastest.  Between the launches out[i] is the squared
// distance to the nearest seed among the voxels that share the coordinates not yet swept, or kDtNone = 0xFFFFFFFF where there is none.  The caller
// vouches that sum_a (spacing_a (b_a - 1))^2 <= 0xFFFFFFFE, so no distance reaches the marker; the marker is compared, never added to: a line
// element that holds it contributes no parabola.  Distances live in uint32 and meet only unsigned or 64-bit arithmetic (one above 2^31 never sees
// a signed int); the intersection of two parabolas is formed in int64 / uint64.
//
// x pass.  A wave takes a row (4 rows per block of 256 threads; VV_DISTANCE_BLOCKS caps every grid, the loops then take blockIdx.x, + gridDim.x, ...).
// It reads the row in chunks of 64 consecutive voxels, one per lane; the seeds of a chunk are one ballot, which lane c keeps for chunk c (a row has
// at most 2048 / 64 = 32 chunks).  A forward wave scan (maximum) gives every chunk the last seed before it, a backward one (minimum) the first seed
// behind it; inside the chunk the nearest seed on either side is a bit scan of the ballot.  Then the row is written.  Everything a row's words
// depend on is in registers before its first store, so out == labels is safe: a row has one reader and writer, the wave.
//
// y and z pass.  The lower envelope of the parabolas g[j] + (w (u - j))^2 along a line (Felzenszwalb and Huttenlocher's two scans, on integer
// positions).  A block takes a tile of COLS lines adjacent in x (times one y-z coordinate): all 256 threads copy it to LDS with x-contiguous reads,
// the block synchronises, and lane c < COLS sweeps line c: scan 1 builds the stack of the parabolas that own a part of the line (V: their positions,
// Z: the first position each owns; 16 bits each), scan 2 walks the line and the stack once and stores the minima (lanes of adjacent x store adjacent
// words).  Since stores go to global memory and G, the LDS copy, is read only, a block never reads what it wrote.  LDS per element: 4 (G) + 2 (V)
// + 2 (Z) bytes; COLS * NCAP * 8 = 64 KiB for lines up to 1024 (32, 16 or 8 lines per tile), 128 KiB for lines up to 2048 (8 lines).
//   Z[k] is the least integer u at which V[k] is not above V[k - 1]: for parabolas at p < q, f_q - f_p falls linearly in u, so f_q <= f_p iff
//   u >= s = (g_q - g_p + w^2 (q^2 - p^2)) / (2 w^2 (q - p)), and the least such integer is max(0, ceil(s)).  A new parabola whose first position is
//   not behind Z[top] leaves the top nothing and pops it (ceil(s) <= Z[top] iff num <= Z[top] * den: no division); one whose first position is
//   behind the line's end is never pushed.  Where two parabolas are equal either serves: only the value is written.  The one division per pushed
//   parabola is a binary64 quotient of integers below 2^35, truncated and then corrected by an integer multiplication, so it is exact whatever
//   the rounding.  The top of the stack in scan 1 and the owning parabola in scan 2 are kept in registers: an element that neither pops nor
//   advances costs no dependent LDS read.
//
// Ownership.  In each launch every word of `out` belongs to one row or one line, and that to one wave or block: no block reads a word another
// block writes in the same launch.  No atomics, no spin, no grid barrier, no cooperative launch; launch boundaries order the passes.
// Termination (every loop that is not a counted loop over rows, items or elements): the pop loop of scan 1 lowers `top` by one per trip and stops
// at 0 -- over a line it pops at most what was pushed, one parabola per element; the advance loop of scan 2 raises k by one per trip and stops at
// top - 1, where the next first position is the line's length.  Both are bounded by the line length whatever the data, and the work per line is linear in it.
// Addresses.  Source: voxel (x, y, z) < b of the box, as in vv_label.hip.  labels / out: row * b_x + x with x < b_x, row < b_y b_z, or
// other * other_stride + j * stride + x0 + c with c < b_x - x0 and j < n: below b_x b_y b_z.  LDS: j * COLS + c with j < n <= NCAP, and a stack
// slot k < pushes <= n.  No scalar-memory stores, no inline assembly, no xnack.
#include "vv_device.h"
#include "vv_kernels.h"

namespace vv {

constexpr int kDtThreads = 256, kDtWave = 64, kDtRows = kDtThreads / kDtWave;   // tests/test_distance.py names kDtThreads THREADS
constexpr int kDtMaxLine = VV_DISTANCE_MAX_EXTENT;
constexpr uint32_t kDtNone = 0xFFFFFFFFu;                  // no seed (between the launches, and VV_DIST_SQUARED's output)
constexpr int kDtFar = 1 << 30;                            // x pass: "no seed on this side", above every position
constexpr int kDtSrcLabels = 2;                            // distance_x_kernel's SRC besides VV_VOXEL_U8 / VV_VOXEL_F32
// lines per tile of distance_line_kernel<NCAP> (tests/test_distance.py: COLS)
constexpr int dt_cols(int ncap) { return ncap <= 256 ? 32 : ncap <= 512 ? 16 : 8; }

static_assert(kDtMaxLine / kDtWave <= kDtWave, "a lane per chunk of a row");
static_assert(dt_cols(2048) * 2048 * 8 <= 160 * 1024, "a tile of the longest lines fits a CU's LDS");

template <int SRC>
__global__ __launch_bounds__(kDtThreads) void distance_x_kernel(DistanceArgs A, uint64_t rows)
{
    const uint32_t lane = threadIdx.x % kDtWave, wave = threadIdx.x / kDtWave;
    const uint32_t bx = A.b[0], by = A.b[1], chunks = (bx + kDtWave - 1) / kDtWave;
    for (uint64_t row = (uint64_t)blockIdx.x * kDtRows + wave; row < rows; row += (uint64_t)gridDim.x * kDtRows) {
        const uint32_t y = (uint32_t)(row % by), z = (uint32_t)(row / by);
        const char *src = (const char *)A.src0 + ((uint64_t)z * A.slice_pitch + (uint64_t)y * A.row_pitch);
        const uint64_t i0 = row * bx;
        unsigned long long mine = 0;                                           // lane c: the seeds of chunk c
        for (uint32_t c = 0; c < chunks; ++c) {
            const uint32_t x = c * kDtWave + lane;
            bool seed = false;
            if (x < bx) {
                bool test;
                if constexpr (SRC == kDtSrcLabels) {
                    const uint32_t v = A.labels[i0 + x];
                    test = A.seed == VV_SEED_LABEL ? v == A.label : v != 0;
                } else {
                    uint32_t bin;
                    if constexpr (SRC == VV_VOXEL_F32) bin = index_of<VV_VOXEL_F32>(*(const float *)(src + (uint64_t)x * 4));
                    else bin = (uint32_t)*(const uint8_t *)(src + x);
                    test = bin >= A.bin_lo && bin <= A.bin_hi;
                }
                seed = test != (A.invert != 0);
            }
            const unsigned long long m = __ballot(seed);
            if (lane == c) mine = m;
        }
        // the last seed before chunk `lane` (-1: none), the first seed behind it (kDtFar: none)
        const int last = mine ? (int)(lane * kDtWave) + 63 - __clzll((long long)mine) : -1;
        const int first = mine ? (int)(lane * kDtWave) + __ffsll((long long)mine) - 1 : kDtFar;
        int before = __shfl_up(last, 1), behind = __shfl_down(first, 1);
        if (lane == 0) before = -1;
        if (lane == kDtWave - 1) behind = kDtFar;
#pragma unroll
        for (int d = 1; d < kDtWave; d <<= 1) {
            const int p = __shfl_up(before, d), q = __shfl_down(behind, d);
            if ((int)lane >= d) before = max(before, p);
            if ((int)lane + d < kDtWave) behind = min(behind, q);
        }
        const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
        for (uint32_t c = 0; c < chunks; ++c) {
            const unsigned long long m = (unsigned long long)(uint32_t)__shfl((int)lo, (int)c) | ((unsigned long long)(uint32_t)__shfl((int)hi, (int)c) << 32);
            const int left_far = __shfl(before, (int)c), right_far = __shfl(behind, (int)c);
            const int x = (int)(c * kDtWave + lane);
            if ((uint32_t)x >= bx) continue;                                   // (the shuffles above are executed by every lane)
            const unsigned long long ml = m & (~0ull >> (63 - lane)), mr = m >> lane;
            const int left = ml ? (int)(c * kDtWave) + 63 - __clzll((long long)ml) : left_far;
            const int right = mr ? x + __ffsll((long long)mr) - 1 : right_far;
            int d = kDtFar;
            if (left >= 0) d = x - left;
            if (right < kDtFar) d = min(d, right - x);
            const uint64_t wd = (uint64_t)A.spacing[0] * (uint32_t)d;          // (d < 2048, spacing_x * (b_x - 1) < 2^16)
            A.out[i0 + x] = d == kDtFar ? kDtNone : (uint32_t)(wd * wd);
        }
    }
}

struct DistanceLineArgs {
    uint32_t *out;
    uint32_t bx, n, tiles_x;                // the row length, the line length, tiles per row
    uint64_t stride, other_stride, items;   // words between a line's elements, between the tiles of one x0; tiles in all
    uint32_t w;                             // the spacing along the line
    int within; uint32_t r2;                // the last launch: 0 = keep the distances, 1 = VV_DIST_WITHIN's threshold
};

template <int NCAP>
__global__ __launch_bounds__(kDtThreads) void distance_line_kernel(DistanceLineArgs L)
{
    constexpr int COLS = dt_cols(NCAP);
    __shared__ uint32_t G[COLS * NCAP];
    __shared__ uint16_t V[COLS * NCAP], Z[COLS * NCAP];
    const uint32_t n = L.n;
    const uint64_t w2 = (uint64_t)L.w * L.w;
    // Tiles adjacent in x share cache lines (a tile's row is COLS * 4 bytes).  Blocks are dealt to the XCDs in turn, each with an L2 of its own: walk
    // index i takes tile (i % 8) * per + i / 8, so that neighbouring tiles meet in one L2 (speed only: any bijection gives the same words).
    const uint64_t per = (L.items + 7) / 8;
    for (uint64_t i = blockIdx.x; i < per * 8; i += gridDim.x) {
        const uint64_t item = (i % 8) * per + i / 8;
        if (item >= L.items) continue;                                         // (the same for the whole block)
        const uint64_t other = item / L.tiles_x;
        const uint32_t x0 = (uint32_t)(item - other * L.tiles_x) * COLS, ncols = min((uint32_t)COLS, L.bx - x0);
        uint32_t *line0 = L.out + (other * L.other_stride + x0);
        for (uint32_t e = threadIdx.x; e < n * COLS; e += kDtThreads) {
            const uint32_t c = e % COLS, j = e / COLS;
            if (c < ncols) G[e] = line0[(uint64_t)j * L.stride + c];
        }
        __syncthreads();
        if (threadIdx.x < ncols) {
            const uint32_t c = threadIdx.x;
            // scan 1: the lower envelope.  The top of the stack (position tp, value tg, first owned position tz) stays in registers.
            uint32_t top = 0, tp = 0, tg = 0, tz = 0;
            uint32_t gnext = G[c];
            for (uint32_t q = 0; q < n; ++q) {
                const uint32_t gq = gnext;
                if (q + 1 < n) gnext = G[(q + 1) * COLS + c];
                if (gq == kDtNone) continue;
                uint32_t s = 0;
                while (top > 0) {
                    const long long num = (long long)gq - (long long)tg + (long long)(w2 * ((uint64_t)(q - tp) * (q + tp)));
                    const unsigned long long den = 2ull * w2 * (q - tp);
                    if (num > (long long)(tz * den)) {                         // max(0, ceil(num / den)) > tz: the top keeps [tz, s)
                        if ((unsigned long long)num >= n * den) s = n;
                        else {                                                 // the quotient is below n <= 2048; the division's result is corrected in integers
                            unsigned long long t = (unsigned long long)((double)num / (double)den);
                            if (t * den < (unsigned long long)num) ++t;
                            s = (uint32_t)t;
                        }
                        break;
                    }
                    --top;
                    if (top > 0) { tp = V[(top - 1) * COLS + c]; tz = Z[(top - 1) * COLS + c]; tg = G[tp * COLS + c]; }
                }
                if (top == 0) s = 0;
                if (s < n) { V[top * COLS + c] = (uint16_t)q; Z[top * COLS + c] = (uint16_t)s; ++top; tp = q; tg = gq; tz = s; }
            }
            // scan 2: the minima.  The parabola that owns u (position cp, value cg) and the next one's first position nz stay in registers.
            uint32_t k = 0, cp = 0, cg = 0, nz = n;
            if (top > 0) { cp = V[c]; cg = G[cp * COLS + c]; nz = top > 1 ? Z[COLS + c] : n; }
            uint32_t *at = line0 + c;
            for (uint32_t u = 0; u < n; ++u, at += L.stride) {
                uint32_t v = kDtNone;
                if (top > 0) {
                    while (u >= nz) {                                          // (nz = n behind the last parabola: k stays below top)
                        ++k;
                        cp = V[k * COLS + c]; cg = G[cp * COLS + c];
                        nz = k + 1 < top ? Z[(k + 1) * COLS + c] : n;
                    }
                    const uint64_t du = u > cp ? u - cp : cp - u;
                    v = (uint32_t)((uint64_t)cg + w2 * du * du);               // (at most 0xFFFFFFFE: the caller's bound)
                }
                if (L.within) v = v != kDtNone && v <= L.r2 ? 1u : 0u;
                *at = v;
            }
        }
        __syncthreads();                                                       // (the next tile reuses G, V and Z)
    }
}

static unsigned distance_grid(uint64_t items, int max_blocks)
{
    uint64_t grid = items ? items : 1;
    if (max_blocks > 0 && grid > (uint64_t)max_blocks) grid = (uint64_t)max_blocks;
    if (grid > 0x7FFFFFFFull) grid = 0x7FFFFFFFull;
    return (unsigned)grid;
}

static void launch_distance_lines(DistanceLineArgs L, uint32_t others, int max_blocks, hipStream_t s)
{
    const int cols = dt_cols((int)L.n);
    L.tiles_x = (L.bx + cols - 1) / cols;
    L.items = (uint64_t)L.tiles_x * others;
    const dim3 grid(distance_grid(L.items, max_blocks)), block(kDtThreads);
    if (L.n <= 256)       hipLaunchKernelGGL(distance_line_kernel<256>, grid, block, 0, s, L);
    else if (L.n <= 512)  hipLaunchKernelGGL(distance_line_kernel<512>, grid, block, 0, s, L);
    else if (L.n <= 1024) hipLaunchKernelGGL(distance_line_kernel<1024>, grid, block, 0, s, L);
    else                  hipLaunchKernelGGL(distance_line_kernel<2048>, grid, block, 0, s, L);
}

void launch_distance(const DistanceArgs &a, int n_cu, int max_blocks, int phases, hipStream_t s)
{
    (void)n_cu;
    const uint64_t rows = (uint64_t)a.b[1] * a.b[2];
    const dim3 grid(distance_grid((rows + kDtRows - 1) / kDtRows, max_blocks)), block(kDtThreads);
    if (a.seed != VV_SEED_BINS)            hipLaunchKernelGGL(distance_x_kernel<kDtSrcLabels>, grid, block, 0, s, a, rows);
    else if (a.src_type == VV_VOXEL_F32)   hipLaunchKernelGGL(distance_x_kernel<VV_VOXEL_F32>, grid, block, 0, s, a, rows);
    else                                   hipLaunchKernelGGL(distance_x_kernel<VV_VOXEL_U8>, grid, block, 0, s, a, rows);
    if (phases == 1) return;
    DistanceLineArgs L;
    L.out = a.out; L.bx = a.b[0]; L.tiles_x = 0; L.items = 0;
    L.within = 0; L.r2 = 0;
    L.n = a.b[1]; L.stride = a.b[0]; L.other_stride = (uint64_t)a.b[0] * a.b[1]; L.w = a.spacing[1];
    launch_distance_lines(L, a.b[2], max_blocks, s);
    if (phases == 2) return;
    L.n = a.b[2]; L.stride = (uint64_t)a.b[0] * a.b[1]; L.other_stride = a.b[0]; L.w = a.spacing[2];
    L.within = a.mode == VV_DIST_WITHIN; L.r2 = a.within_r2;
    launch_distance_lines(L, a.b[1], max_blocks, s);
}

} // namespace vv
