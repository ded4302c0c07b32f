// vv_derive.hip -- derived volumes for gfx950: a box of the loaded volume cropped, reduced by whole factors, windowed and converted into a dense volume
// (no reference counterpart; the contract is the comment on vv_derive_volume in include/volviz.h).
//
//   derive_kernel<SRC, OUT, FX>   FX = 1, 2, 4, 8: that factor along x with vector loads; FX = 0: any factor, one voxel per load
//
// Work.  An output row (Y, Z) is cut into chunks of 64 * OPL output voxels, a chunk is one trip of one wave: lane l owns the OPL consecutive output
// voxels from (chunk * 64 + l) * OPL on, and walks their cells by itself: source slice by source slice, row by row, x fastest -- the contract's
// order, so the f32 sum needs no cross-lane step.  For every source row of the cells the lane loads its OPL * f_x consecutive voxels: the wave reads
// one contiguous span of 64 * OPL * f_x voxels.  OPL is 4 (u8 outputs are stored as dwords, f32 outputs as 16 bytes), fewer where an f32 source
// with f32 output already has 16 bytes per lane and row with fewer, more where 4 outputs of a u8 source stored as u8 have less than 16 bytes (derive_opl).
// The (row, chunk) pairs are dealt to the grid's waves round-robin and stepped through in mixed radix (chunk, Y, Z), as hist_kernel's: no division
// in the loop.
// Loads.  FX > 0: the lane's OPL * FX voxels of a source row as aligned vectors of up to 16 bytes.  launch_derive takes this path only where every
// lane's span starts on a vector boundary (the box's first voxel and both pitches) and where a vector that starts inside the box ends inside the
// allocation; voxels of a vector beyond the box's high x are loaded and not looked at.  FX = 0: every voxel of the cell by its own load.
// Addresses come from the box, the factors and the pitches alone, in 64 bits.  Every output voxel has one writer: no atomics.
// Arithmetic.  All three reductions are carried along (u8: sum, max, min; f32: the ordered sum and the two integer keys of vv_hist.hip) and the
// mode picks one at the end: the pass is bound by memory, the mode is then no template parameter.  The f32 sum starts as -0.0f, the one binary32 value
// x + which is x for every x (so "starts as the cell's first voxel" holds bit for bit, -0.0 and denormals included); a cell of one voxel is copied as
// bits.  Stage 2 (window, unit scale, output type) runs once per output voxel under contract(off).
#include "vv_device.h"
#include "vv_kernels.h"

namespace vv {

constexpr int kDeriveWaves = 4;               // waves per block
constexpr int kDeriveBlocksPerCU = 32 / kDeriveWaves;

// output voxels per lane and trip
constexpr int derive_opl(int src, int out, int fx)
{
    return out == VV_VOXEL_F32 ? (src == VV_VOXEL_U8 ? 4 : fx == 1 ? 4 : fx == 2 ? 2 : 1)      // f32 output: 16 bytes per lane and store, no more
         : src == VV_VOXEL_U8 ? (fx == 1 ? 16 : fx == 2 ? 8 : 4) : 4;                          // u8 -> u8: 16 bytes per lane and row where 4 outputs have fewer
}

struct DeriveKernelArgs {
    DeriveArgs D;
    uint32_t cpr;                   // chunks per output row
    uint32_t dk, dry, drz;          // the grid's stride (gridDim.x * kDeriveWaves pairs) as digits: chunks, output rows (with the chunks' carry), output slices
};

// the reductions of one output voxel
template <bool F32> struct DeriveCell;
template <> struct DeriveCell<false> {
    uint32_t sum, hi, lo;
    __device__ __forceinline__ void init() { sum = 0; hi = 0; lo = 255; }
    __device__ __forceinline__ void add(uint32_t v, bool) { sum += v; hi = max(hi, v); lo = min(lo, v); }
};
template <> struct DeriveCell<true> {
    float acc; uint32_t first, kmax, knmin;       // kmax / knmin: largest key, largest complemented key of the non-NaN voxels (0: none yet)
    __device__ __forceinline__ void init() { acc = -0.0f; first = 0; kmax = 0; knmin = 0; }
    __device__ __forceinline__ void add(uint32_t u, bool is_first)
    {
#pragma clang fp contract(off)
        acc = acc + __uint_as_float(u);
        if (is_first) first = u;
        const uint32_t key = hist_key(u);
        if ((u & 0x7FFFFFFFu) <= 0x7F800000u) { kmax = max(kmax, key); knmin = max(knmin, ~key); }
    }
};

template <int W> __device__ __forceinline__ void derive_load(const char *p, uint32_t *w);
template <> __device__ __forceinline__ void derive_load<4>(const char *p, uint32_t *w) { w[0] = *(const uint32_t *)p; }
template <> __device__ __forceinline__ void derive_load<8>(const char *p, uint32_t *w) { const uint2 q = *(const uint2 *)p; w[0] = q.x; w[1] = q.y; }
template <> __device__ __forceinline__ void derive_load<16>(const char *p, uint32_t *w) { const uint4 q = *(const uint4 *)p; w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; }

// stage 1's result r of a cell of n voxels -> the output voxel: a byte, or a binary32 bit pattern
// (n_full: the voxels of a whole cell of this trip, the same for every lane: where it is 1 no lane divides)
template <bool F32, bool OF32>
__device__ __forceinline__ uint32_t derive_finish(const DeriveCell<F32> &c, uint32_t n, uint32_t n_full, int mode, int window, float win_lo, float win_hi)
{
#pragma clang fp contract(off)
    uint32_t rbits;                       // F32: r's pattern; u8: r
    float u;                              // r in storage units
    if constexpr (F32) {
        if (mode == VV_REDUCE_MEAN) { if (n_full == 1) rbits = c.first; else rbits = n == 1 ? c.first : __float_as_uint(c.acc / (float)n); }
        else if (c.kmax == 0) rbits = 0x7FC00000u;
        else rbits = hist_key_inverse(mode == VV_REDUCE_MAX ? c.kmax : ~c.knmin);
        u = __uint_as_float(rbits);
    } else {
        // (2 s + n) / (2 n) in integers as one binary32 division: numerator < 2^18 and denominator <= 1024 are exact, a quotient that is no integer
        // lies 1 / 1024 or more off the next one, the division's error is below 2^-16: truncation gives the integer quotient
        if (mode == VV_REDUCE_MEAN) { if (n_full == 1) rbits = c.sum; else rbits = (uint32_t)((float)(2u * c.sum + n) / (float)(2u * n)); }
        else rbits = mode == VV_REDUCE_MAX ? c.hi : c.lo;
        u = (float)rbits;
    }
    if (window) {
        const float w = (u - win_lo) / (win_hi - win_lo);
        return OF32 ? __float_as_uint(w) : index_of<VV_VOXEL_F32>(w);
    }
    return voxel_out_copy<F32, OF32>(rbits);
}

template <int SRC, int OUT, int FX>
__global__ __launch_bounds__(64 * kDeriveWaves) void derive_kernel(DeriveKernelArgs A)
{
    constexpr bool F32 = SRC == VV_VOXEL_F32, OF32 = OUT == VV_VOXEL_F32;
    constexpr int SIZE = F32 ? 4 : 1, OSIZE = OF32 ? 4 : 1;
    constexpr int OPL = derive_opl(SRC, OUT, FX);
    const DeriveArgs &D = A.D;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t fx = FX ? (uint32_t)FX : D.f[0];

    const uint32_t first = blockIdx.x * kDeriveWaves + wave;
    uint32_t k = first % A.cpr, ry = (first / A.cpr) % D.m[1], rz = (first / A.cpr) / D.m[1];
    while (rz < D.m[2]) {
        const uint32_t X0 = (k * 64u + lane) * OPL;                        // the lane's first output voxel of the row
        if (X0 < D.m[0]) {
            const uint32_t sy0 = ry * D.f[1], sz0 = rz * D.f[2], x0 = X0 * fx;          // the cells' first source voxel, in the box
            const uint32_t cy = min(D.f[1], D.b[1] - sy0), cz = min(D.f[2], D.b[2] - sz0);   // source rows and slices of the cells (partial at the high end)
            const uint32_t rem = D.b[0] - x0;                              // source voxels of the box's rows from x0 on (>= 1)
            DeriveCell<F32> cell[OPL];
#pragma unroll
            for (int o = 0; o < OPL; ++o) cell[o].init();
            const char *pz = (const char *)D.src0 + (uint64_t)sz0 * D.slice_pitch + (uint64_t)sy0 * D.row_pitch + (uint64_t)x0 * SIZE;
            for (uint32_t dz = 0; dz < cz; ++dz, pz += D.slice_pitch) {
                const char *p = pz;
                for (uint32_t dy = 0; dy < cy; ++dy, p += D.row_pitch) {
                    const bool row0 = (dz | dy) == 0;
                    if constexpr (FX > 0) {
                        constexpr int NVOX = OPL * FX, B = NVOX * SIZE, W = B < 16 ? B : 16;
                        uint32_t w[B / 4];
#pragma unroll
                        for (int j = 0; j < B / W; ++j) derive_load<W>(p + j * W, w + j * (W / 4));
#pragma unroll
                        for (int e = 0; e < NVOX; ++e) {
                            uint32_t v;
                            if constexpr (F32) v = w[e]; else v = (w[e >> 2] >> (8 * (e & 3))) & 255u;
                            if ((uint32_t)e < rem) cell[e / FX].add(v, row0 && e % FX == 0);
                        }
                    } else {
#pragma unroll
                        for (int o = 0; o < OPL; ++o) {
                            const uint32_t at = (uint32_t)o * fx;
                            const uint32_t cnt = at < rem ? min(fx, rem - at) : 0u;
                            for (uint32_t e = 0; e < cnt; ++e) {
                                const char *q = p + (size_t)(at + e) * SIZE;
                                const uint32_t v = F32 ? *(const uint32_t *)q : (uint32_t)*(const uint8_t *)q;
                                cell[o].add(v, row0 && e == 0);
                            }
                        }
                    }
                }
            }
            // stage 2 and the stores: whole groups at aligned addresses as one store, the row's tail (and rows that start off a boundary) voxel by voxel
            uint32_t r[OPL];
#pragma unroll
            for (int o = 0; o < OPL; ++o) {
                const uint32_t at = (uint32_t)o * fx;
                const uint32_t cx = at < rem ? min(fx, rem - at) : 1u;     // (no such output voxel: computed, not stored)
                r[o] = derive_finish<F32, OF32>(cell[o], cx * cy * cz, fx * cy * cz, D.mode, D.window, D.win_lo, D.win_hi);
            }
            char *dst = (char *)D.out + (((uint64_t)rz * D.m[1] + ry) * D.m[0] + X0) * OSIZE;
            const uint32_t n_out = min((uint32_t)OPL, D.m[0] - X0);
            if (n_out == OPL && ((uintptr_t)dst & (OF32 && OPL >= 4 ? 15 : 3)) == 0) {
                if constexpr (!OF32) {
#pragma unroll
                    for (int g = 0; g < OPL / 4; ++g) ((uint32_t *)dst)[g] = r[4 * g] | r[4 * g + 1] << 8 | r[4 * g + 2] << 16 | r[4 * g + 3] << 24;
                } else if constexpr (OPL >= 4) {
#pragma unroll
                    for (int g = 0; g < OPL / 4; ++g) ((uint4 *)dst)[g] = make_uint4(r[4 * g], r[4 * g + 1], r[4 * g + 2], r[4 * g + 3]);
                } else {
#pragma unroll
                    for (int o = 0; o < OPL; ++o) ((uint32_t *)dst)[o] = r[o];
                }
            } else {
#pragma unroll
                for (int o = 0; o < OPL; ++o)
                    if ((uint32_t)o < n_out) voxel_store<OF32>(dst + o * OSIZE, r[o]);
            }
        }
        k += A.dk;
        uint32_t carry = k >= A.cpr;
        if (carry) k -= A.cpr;
        ry += A.dry + carry;
        carry = ry >= D.m[1];
        if (carry) ry -= D.m[1];
        rz += A.drz + carry;
    }
}

template <int SRC, int OUT>
static void launch_derive_fx(const DeriveKernelArgs &a, int fx /* 0: generic */, int grid, hipStream_t s)
{
    const dim3 g(grid), b(64 * kDeriveWaves);
    switch (fx) {
        case 1:  hipLaunchKernelGGL((derive_kernel<SRC, OUT, 1>), g, b, 0, s, a); break;
        case 2:  hipLaunchKernelGGL((derive_kernel<SRC, OUT, 2>), g, b, 0, s, a); break;
        case 4:  hipLaunchKernelGGL((derive_kernel<SRC, OUT, 4>), g, b, 0, s, a); break;
        case 8:  hipLaunchKernelGGL((derive_kernel<SRC, OUT, 8>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((derive_kernel<SRC, OUT, 0>), g, b, 0, s, a); break;
    }
}

void launch_derive(const DeriveArgs &d, int n_cu, int max_blocks, hipStream_t s)
{
    DeriveKernelArgs a;
    a.D = d;
    const uint32_t size = d.src_type == VV_VOXEL_F32 ? 4 : 1;
    // vector loads: a specialised factor, every lane's span of every source row on a vector boundary, and the last vector inside the allocation
    int fx = (d.f[0] == 1 || d.f[0] == 2 || d.f[0] == 4 || d.f[0] == 8) ? (int)d.f[0] : 0;
    if (fx) {
        const uint32_t span = (uint32_t)derive_opl(d.src_type, d.out_type, fx) * fx * size, vec = span < 16 ? span : 16;
        const bool one_row = (uint64_t)d.b[1] * d.b[2] == 1;
        const bool aligned = (uintptr_t)d.src0 % vec == 0 && (one_row || (d.row_pitch % vec == 0 && d.slice_pitch % vec == 0));
        if (!aligned || d.slack < span) fx = 0;
    }
    const uint32_t per_chunk = 64u * derive_opl(d.src_type, d.out_type, fx);
    a.cpr = (d.m[0] + per_chunk - 1) / per_chunk;
    const uint64_t pairs = (uint64_t)a.cpr * d.m[1] * d.m[2];
    uint64_t grid = (pairs + kDeriveWaves - 1) / kDeriveWaves;
    const uint64_t cap = max_blocks > 0 ? (uint64_t)max_blocks : (uint64_t)(n_cu > 0 ? n_cu : 256) * kDeriveBlocksPerCU;
    if (grid > cap) grid = cap;
    const uint64_t stride = grid * kDeriveWaves, dq = stride / a.cpr;
    a.dk = (uint32_t)(stride % a.cpr); a.dry = (uint32_t)(dq % d.m[1]); a.drz = (uint32_t)(dq / d.m[1]);
    const bool sf = d.src_type == VV_VOXEL_F32, of = d.out_type == VV_VOXEL_F32;
    if (sf && of)       launch_derive_fx<VV_VOXEL_F32, VV_VOXEL_F32>(a, fx, (int)grid, s);
    else if (sf)        launch_derive_fx<VV_VOXEL_F32, VV_VOXEL_U8>(a, fx, (int)grid, s);
    else if (of)        launch_derive_fx<VV_VOXEL_U8, VV_VOXEL_F32>(a, fx, (int)grid, s);
    else                launch_derive_fx<VV_VOXEL_U8, VV_VOXEL_U8>(a, fx, (int)grid, s);
}

} // namespace vv
