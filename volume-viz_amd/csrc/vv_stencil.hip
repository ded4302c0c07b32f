// vv_stencil.hip -- neighbourhood filters on the loaded volume for gfx950: a separable convolution of up to 9 taps per axis, the 3x3x3 median and the
// gradient magnitude of a box, written as a dense volume (no reference counterpart; the contract is the comment on vv_stencil_volume in
// include/volviz.h).
//
//   stencil_sep_kernel<SRC, OUT>          VV_STENCIL_SEPARABLE: the x, y and z passes in one launch, no volume-sized intermediate
//   stencil_nb_kernel<SRC, OUT, KIND>     VV_STENCIL_MEDIAN / VV_STENCIL_GRADMAG: the 3x3x3 neighbourhood
//
// Work.  The box is cut into tiles of 32 x 16 (separable) or 32 x 8 (3x3x3) output voxels in (x, y) and its z range into segments; a block of 32 x 8
// threads takes one (tile, segment) item at a time (blockIdx.x, then + gridDim.x) and marches it in z: thread (lx, ly) owns the output column
// (x0 + lx, y0 + ly), in the separable kernel also (x0 + lx, y0 + ly + 8).
// Every source plane of the tile, with its halo in x and y, is loaded once per item: the halo is paid in two dimensions, the third is the march.
// stencil_sep_kernel, per source plane: the (32 + 2 R_x) x (16 + 2 R_y) voxels go to LDS as binary32 (S); the x pass makes 32 x (16 + 2 R_y) values
// (Px) of them; the y pass makes the thread's two values of that plane, which go into the thread's slots of a ring of 2 R_z + 1 planes (LDS,
// indexed by the step: a register ring would need the radius at compile time); the z pass reads the ring and the output stage stores two voxels.
// A plane that the clamp repeats at the volume's ends is not computed again.  The loads of the next plane are issued before the passes of this one.
// stencil_nb_kernel: a ring of four planes of 34 x 10 raw values (bytes, binary32 patterns; the median of an f32 volume: hist_key of the
// pattern); three of them are read while the fourth is written, one barrier per plane.
// Edges.  Every coordinate is clamped to the volume (not to the box), per axis, where the address of the load is made: the value a pass finds
// at a clamped coordinate is the value of the clamped voxel, so each pass clamps on its own axis as the contract says.  Addresses come from the
// box, the clamped coordinates and the pitches alone, in 64 bits; padding is never addressed.  Each output voxel has one writer: no atomics.
// Arithmetic: binary32 in the contract's order under contract(off); a pass of radius 0 copies.  The median is a fixed selection network of
// integer minima and maxima: no floating-point comparison, no data-dependent branch.
#include "vv_device.h"
#include "vv_kernels.h"

namespace vv {

constexpr int kStTX = 32, kStTY = 8;                                     // the threads of a block in x and y; the 3x3x3 kernels' tile
constexpr int kStThreads = kStTX * kStTY;
constexpr int kSepRows = 2, kSepTY = kStTY * kSepRows;                   // the separable kernel: output rows per thread (ly, ly + 8), rows per tile
constexpr int kStR = VV_STENCIL_MAX_RADIUS;
constexpr int kStSW = kStTX + 2 * kStR, kStSH = kSepTY + 2 * kStR;       // S: row stride and rows of the separable kernel
constexpr int kStLoads = (kStSW * kStSH + kStThreads - 1) / kStThreads;  // source voxels per thread and plane, at most
constexpr int kStXRounds = kStSH * kStTX / kStThreads;                   // x-pass values per thread and plane, at most
constexpr int kNbSW = kStTX + 2, kNbSH = kStTY + 2;                      // the 3x3x3 kernels' planes
constexpr int kNbLoads = (kNbSW * kNbSH + kStThreads - 1) / kStThreads;
constexpr uint32_t kStMinSegment = 32;                                   // planes of a z segment, at least (each segment primes 2 R_z planes)
static_assert(kStSH * kStTX % kStThreads == 0 && kStTX == 32, "the passes' index arithmetic");

struct StencilKernelArgs {
    StencilArgs S;
    uint32_t ntx, tiles;            // tiles per row of tiles, tiles per segment
    uint32_t seg_len;               // planes per z segment
    uint64_t items;                 // tiles * segments
};

template <bool F32> __device__ __forceinline__ uint32_t stencil_load(const char *p)
{
    if constexpr (F32) return *(const uint32_t *)p; else return (uint32_t)*(const uint8_t *)p;
}
template <bool F32> __device__ __forceinline__ float stencil_value(uint32_t raw) { return F32 ? __uint_as_float(raw) : (float)raw; }

// one pass: acc = t[0] * c, then acc = acc + t[k] * (v(-k) + v(+k)) for k = 1..R; R = 0: c itself (t: the axis' taps in registers, R uniform)
__device__ __forceinline__ float stencil_pass(const float *centre, int stride, int R, const float (&t)[kStR + 1])
{
#pragma clang fp contract(off)
    const float c = centre[0];
    if (R == 0) return c;
    float acc = t[0] * c;
#pragma unroll
    for (int k = 1; k <= kStR; ++k)
        if (k <= R) acc = acc + t[k] * (centre[-k * stride] + centre[k * stride]);
    return acc;
}

// what the kernels share: the item's tile and z range
struct StencilItem { int x0, y0, zb, ze; uint32_t ox, oy; bool owns; uint64_t first, plane; };   // first / plane: the column's first output voxel, voxels per output plane
template <int TILE_Y> __device__ __forceinline__ StencilItem stencil_item(const StencilKernelArgs &A, uint64_t item, uint32_t lx, uint32_t ly)
{
    const StencilArgs &D = A.S;
    const uint32_t seg = (uint32_t)(item / A.tiles), t = (uint32_t)(item % A.tiles), ty = t / A.ntx, tx = t % A.ntx;
    StencilItem I;
    I.ox = tx * kStTX + lx; I.oy = ty * TILE_Y + ly;                 // the thread's (first) output column, in the box
    I.owns = I.ox < D.b[0] && I.oy < D.b[1];
    I.x0 = D.lo[0] + (int)(tx * kStTX); I.y0 = D.lo[1] + (int)(ty * TILE_Y);
    const uint32_t zs = seg * A.seg_len;
    I.zb = D.lo[2] + (int)zs; I.ze = D.lo[2] + (int)min(zs + A.seg_len, D.b[2]);
    I.plane = (uint64_t)D.b[0] * D.b[1];
    I.first = zs * I.plane + (uint64_t)I.oy * D.b[0] + I.ox;
    return I;
}
__device__ __forceinline__ int stencil_clamp(int v, int n) { return max(0, min(v, n - 1)); }

template <int SRC, int OUT>
__global__ __launch_bounds__(kStThreads) void stencil_sep_kernel(StencilKernelArgs A)
{
#pragma clang fp contract(off)
    constexpr bool F32 = SRC == VV_VOXEL_F32, OF32 = OUT == VV_VOXEL_F32;
    constexpr int SIZE = F32 ? 4 : 1, OSIZE = OF32 ? 4 : 1;
    __shared__ float S[kStSH * kStSW];
    __shared__ float Px[kStSH * kStTX];
    __shared__ float ring[(2 * kStR + 1) * kSepRows * kStThreads];
    const StencilArgs &D = A.S;
    const int Rx = D.radius[0], Ry = D.radius[1], Rz = D.radius[2];
    const uint32_t tid = threadIdx.x, lx = tid & (kStTX - 1), ly = tid / kStTX;
    const int W = kStTX + 2 * Rx, H = kSepTY + 2 * Ry, NE = W * H, NZ = 2 * Rz + 1;
    float tx[kStR + 1], ty[kStR + 1], tz[kStR + 1];
#pragma unroll
    for (int k = 0; k <= kStR; ++k) { tx[k] = D.taps[0][k]; ty[k] = D.taps[1][k]; tz[k] = D.taps[2][k]; }

    for (uint64_t item = blockIdx.x; item < A.items; item += gridDim.x) {
        const StencilItem I = stencil_item<kSepTY>(A, item, lx, ly);
        // this thread's voxels of a source plane: where they lie in the plane (clamped to the volume) and in S
        uint64_t off[kStLoads]; int at[kStLoads];
#pragma unroll
        for (int r = 0; r < kStLoads; ++r) {
            const int e = (int)tid + r * kStThreads;
            at[r] = -1; off[r] = 0;
            if (e < NE) {
                const int row = e / W, col = e - row * W;
                const int xc = stencil_clamp(I.x0 - Rx + col, D.n[0]), yc = stencil_clamp(I.y0 - Ry + row, D.n[1]);
                off[r] = (uint64_t)yc * D.row_pitch + (uint64_t)xc * SIZE;
                at[r] = row * kStSW + col;
            }
        }
        const int zfirst = stencil_clamp(I.zb - Rz, D.n[2]), zlast = stencil_clamp(I.ze - 1 + Rz, D.n[2]);
        uint32_t raw[kStLoads];
#pragma unroll
        for (int r = 0; r < kStLoads; ++r)
            raw[r] = at[r] >= 0 ? stencil_load<F32>((const char *)D.vol + (uint64_t)zfirst * D.slice_pitch + off[r]) : 0u;
        int have = -1, slot = 0;
        float py[kSepRows];
        bool owns[kSepRows];
#pragma unroll
        for (int q = 0; q < kSepRows; ++q) { py[q] = 0.f; owns[q] = I.ox < D.b[0] && I.oy + q * kStTY < D.b[1]; }
        char *op = (char *)D.out + I.first * OSIZE;                       // the first column's next output voxel (dereferenced by owners only)
        const uint64_t qstep = (uint64_t)kStTY * D.b[0] * OSIZE;         // from one of the thread's columns to the next
        for (int j = I.zb - Rz; j < I.ze + Rz; ++j) {
            const int zc = stencil_clamp(j, D.n[2]);
            if (zc != have) {                                            // (the same for the whole block)
#pragma unroll
                for (int r = 0; r < kStLoads; ++r)
                    if (at[r] >= 0) S[at[r]] = stencil_value<F32>(raw[r]);
                if (zc < zlast) {                                        // the next plane's loads, in flight during the passes
#pragma unroll
                    for (int r = 0; r < kStLoads; ++r)
                        if (at[r] >= 0) raw[r] = stencil_load<F32>((const char *)D.vol + (uint64_t)(zc + 1) * D.slice_pitch + off[r]);
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < kStXRounds; ++r) {
                    const int idx = (int)tid + r * kStThreads, row = idx / kStTX, x = idx & (kStTX - 1);
                    if (row < H) Px[idx] = stencil_pass(&S[row * kStSW + x + Rx], 1, Rx, tx);
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < kSepRows; ++q)
                    py[q] = stencil_pass(&Px[((int)ly + q * kStTY + Ry) * kStTX + (int)lx], kStTX, Ry, ty);
                have = zc;
            }
            float r[kSepRows];
#pragma unroll
            for (int q = 0; q < kSepRows; ++q) r[q] = py[q];
            if (Rz > 0) {
                // the thread's own rings: the plane of this step into `slot`; the output plane j - R_z has its centre R_z steps back
#pragma unroll
                for (int q = 0; q < kSepRows; ++q) ring[(slot * kSepRows + q) * kStThreads + (int)tid] = py[q];
                if (j - Rz >= I.zb) {
                    int c = slot - Rz; if (c < 0) c += NZ;
#pragma unroll
                    for (int q = 0; q < kSepRows; ++q) r[q] = tz[0] * ring[(c * kSepRows + q) * kStThreads + (int)tid];
#pragma unroll
                    for (int k = 1; k <= kStR; ++k)
                        if (k <= Rz) {
                            int lo = c - k, hi = c + k;
                            if (lo < 0) lo += NZ;
                            if (hi >= NZ) hi -= NZ;
#pragma unroll
                            for (int q = 0; q < kSepRows; ++q)
                                r[q] = r[q] + tz[k] * (ring[(lo * kSepRows + q) * kStThreads + (int)tid] + ring[(hi * kSepRows + q) * kStThreads + (int)tid]);
                        }
                }
                if (++slot == NZ) slot = 0;
            }
            if (j - Rz >= I.zb) {                                         // output plane j - R_z
#pragma unroll
                for (int q = 0; q < kSepRows; ++q)
                    if (owns[q]) voxel_store<OF32>(op + q * qstep, voxel_out<F32, OF32>(r[q]));
                op += I.plane * OSIZE;
            }
        }
        __syncthreads();                                                 // the next item's planes overwrite S and Px
    }
}

// ---- the median of 27: forgetful selection.  Of N values of which the wanted one is the middle of those still in play, the least and the greatest
// cannot be it: minmax<N> moves them to the ends, the greatest is dropped, the least is replaced by the next value not yet looked at.  15 values
// to start with, 12 to take in, 3 at the end.
__device__ __forceinline__ void stencil_cx(uint32_t &a, uint32_t &b) { const uint32_t lo = min(a, b), hi = max(a, b); a = lo; b = hi; }
template <int N> __device__ __forceinline__ void stencil_minmax(uint32_t *v)
{
#pragma unroll
    for (int i = 0; i < N / 2; ++i) stencil_cx(v[i], v[N - 1 - i]);                      // the least is now in v[0 .. N/2], the greatest in v[N/2 .. N-1]
#pragma unroll
    for (int i = 1; i < (N + 1) / 2; ++i) stencil_cx(v[0], v[i]);
#pragma unroll
    for (int i = N / 2; i < N - 1; ++i) stencil_cx(v[i], v[N - 1]);
}
template <int N> __device__ __forceinline__ uint32_t stencil_select(uint32_t *w, const uint32_t *rest)
{
    stencil_minmax<N>(w);
    if constexpr (N == 3) return w[1];
    else { w[0] = rest[0]; return stencil_select<N - 1>(w, rest + 1); }
}

template <int SRC, int OUT, int KIND>
__global__ __launch_bounds__(kStThreads) void stencil_nb_kernel(StencilKernelArgs A)
{
#pragma clang fp contract(off)
    constexpr bool F32 = SRC == VV_VOXEL_F32, OF32 = OUT == VV_VOXEL_F32, MEDIAN = KIND == VV_STENCIL_MEDIAN;
    constexpr int SIZE = F32 ? 4 : 1, OSIZE = OF32 ? 4 : 1, NE = kNbSW * kNbSH;
    __shared__ uint32_t S[4][NE];
    const StencilArgs &D = A.S;
    const uint32_t tid = threadIdx.x, lx = tid & (kStTX - 1), ly = tid / kStTX;
    const int ci = ((int)ly + 1) * kNbSW + (int)lx + 1;                  // the thread's own voxel in a plane of S

    for (uint64_t item = blockIdx.x; item < A.items; item += gridDim.x) {
        const StencilItem I = stencil_item<kStTY>(A, item, lx, ly);
        uint64_t off[kNbLoads]; int at[kNbLoads];
#pragma unroll
        for (int r = 0; r < kNbLoads; ++r) {
            const int e = (int)tid + r * kStThreads;
            at[r] = -1; off[r] = 0;
            if (e < NE) {
                const int row = e / kNbSW, col = e - row * kNbSW;
                const int xc = stencil_clamp(I.x0 - 1 + col, D.n[0]), yc = stencil_clamp(I.y0 - 1 + row, D.n[1]);
                off[r] = (uint64_t)yc * D.row_pitch + (uint64_t)xc * SIZE;
                at[r] = e;
            }
        }
        uint32_t raw[kNbLoads];
#pragma unroll
        for (int r = 0; r < kNbLoads; ++r)
            raw[r] = at[r] >= 0 ? stencil_load<F32>((const char *)D.vol + (uint64_t)stencil_clamp(I.zb - 1, D.n[2]) * D.slice_pitch + off[r]) : 0u;
        int s = 0;
        char *op = (char *)D.out + I.first * OSIZE;                       // the column's next output voxel (dereferenced by owners only)
        for (int j = I.zb - 1; j <= I.ze; ++j, ++s) {                    // step s brings plane j; from s = 2 on it completes output plane j - 1
#pragma unroll
            for (int r = 0; r < kNbLoads; ++r)
                if (at[r] >= 0) S[s & 3][at[r]] = (MEDIAN && F32) ? hist_key(raw[r]) : raw[r];
            if (j < I.ze) {
                const uint64_t zoff = (uint64_t)stencil_clamp(j + 1, D.n[2]) * D.slice_pitch;
#pragma unroll
                for (int r = 0; r < kNbLoads; ++r)
                    if (at[r] >= 0) raw[r] = stencil_load<F32>((const char *)D.vol + zoff + off[r]);
            }
            __syncthreads();                                             // (the plane written at step s + 1 is the one no thread reads at step s)
            if (s < 2) continue;
            const uint32_t *pa = S[(s - 2) & 3], *pb = S[(s - 1) & 3], *pc = S[s & 3];
            uint32_t v;
            if constexpr (MEDIAN) {
                uint32_t w[27];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int q = ci + (dy - 1) * kNbSW + dx - 1;
                        w[dy * 3 + dx] = pa[q]; w[9 + dy * 3 + dx] = pb[q]; w[18 + dy * 3 + dx] = pc[q];
                    }
                const uint32_t m = stencil_select<15>(w, w + 15);
                v = voxel_out_copy<F32, OF32>(F32 ? hist_key_inverse(m) : m);
            } else {
                const float gx = stencil_value<F32>(pb[ci + 1]) - stencil_value<F32>(pb[ci - 1]);
                const float gy = stencil_value<F32>(pb[ci + kNbSW]) - stencil_value<F32>(pb[ci - kNbSW]);
                const float gz = stencil_value<F32>(pc[ci]) - stencil_value<F32>(pa[ci]);
                const float Gx = gx * D.gscale[0], Gy = gy * D.gscale[1], Gz = gz * D.gscale[2];
                v = voxel_out<F32, OF32>(sqrtf((Gx * Gx + Gy * Gy) + Gz * Gz));
            }
            if (I.owns) voxel_store<OF32>(op, v);
            op += I.plane * OSIZE;
        }
        __syncthreads();                                                 // the next item starts over at plane 0 of S
    }
}

template <int SRC, int OUT>
static void launch_stencil_kind(const StencilKernelArgs &a, int grid, hipStream_t s)
{
    const dim3 g(grid), b(kStThreads);
    switch (a.S.kind) {
        case VV_STENCIL_SEPARABLE: hipLaunchKernelGGL((stencil_sep_kernel<SRC, OUT>), g, b, 0, s, a); break;
        case VV_STENCIL_MEDIAN:    hipLaunchKernelGGL((stencil_nb_kernel<SRC, OUT, VV_STENCIL_MEDIAN>), g, b, 0, s, a); break;
        default:                   hipLaunchKernelGGL((stencil_nb_kernel<SRC, OUT, VV_STENCIL_GRADMAG>), g, b, 0, s, a); break;
    }
}

void launch_stencil(const StencilArgs &d, int n_cu, int max_blocks, hipStream_t s)
{
    StencilKernelArgs a;
    a.S = d;
    a.ntx = (d.b[0] + kStTX - 1) / kStTX;
    const uint32_t tile_y = d.kind == VV_STENCIL_SEPARABLE ? kSepTY : kStTY;
    const uint64_t tiles = (uint64_t)a.ntx * ((d.b[1] + tile_y - 1) / tile_y);         // (below 2^32: a tile holds 256 columns or more of an allocation)
    a.tiles = (uint32_t)tiles;
    // z segments: enough items to fill the part several times over where the (x, y) extent alone does not, none shorter than kStMinSegment planes
    const uint64_t want = (uint64_t)(n_cu > 0 ? n_cu : 256) * 32;
    uint64_t nseg = (want + tiles - 1) / tiles;
    const uint64_t most = (d.b[2] + kStMinSegment - 1) / kStMinSegment;
    if (nseg > most) nseg = most;
    a.seg_len = (uint32_t)((d.b[2] + nseg - 1) / nseg);
    nseg = (d.b[2] + a.seg_len - 1) / a.seg_len;
    a.items = tiles * nseg;
    uint64_t grid = a.items;
    const uint64_t cap = max_blocks > 0 ? (uint64_t)max_blocks : 0x7FFFFFFFull;
    if (grid > cap) grid = cap;
    const bool sf = d.src_type == VV_VOXEL_F32, of = d.out_type == VV_VOXEL_F32;
    if (sf && of)       launch_stencil_kind<VV_VOXEL_F32, VV_VOXEL_F32>(a, (int)grid, s);
    else if (sf)        launch_stencil_kind<VV_VOXEL_F32, VV_VOXEL_U8>(a, (int)grid, s);
    else if (of)        launch_stencil_kind<VV_VOXEL_U8, VV_VOXEL_F32>(a, (int)grid, s);
    else                launch_stencil_kind<VV_VOXEL_U8, VV_VOXEL_U8>(a, (int)grid, s);
}

} // namespace vv
