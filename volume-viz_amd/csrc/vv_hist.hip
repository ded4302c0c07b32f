// vv_hist.hip -- histograms of the loaded volume and of index images for gfx950: voxels per classification index, NaN count and value range
// (no reference counterpart; the contract is the comment on vv_volume_histogram in include/volviz.h).
//
//   hist_kernel<VOXEL, VEC>   counts the voxels of a set of equally long contiguous RUNS (HistRuns, vv_kernels.h) into the global accumulator
//   hist_finish_kernel        accumulator -> vv_histogram (or the 256 counts alone)
//
// Work.  A run is cut into chunks of 1024 voxels, a chunk is one trip of one wave: 16 voxels per lane.  The (run, chunk) pairs are numbered run by
// run and dealt to the grid's waves round-robin; a wave steps through its pairs by adding the grid's stride in mixed radix (chunk, row, slice),
// whose digits the launcher works out, so the loop has no division.
// Loads.  VEC: 16 bytes per lane (one for u8, four for f32, each wave-wide load 1 KiB of consecutive bytes) at 16-byte aligned addresses; a run that
// starts `head` voxels into a vector and ends inside one has the lanes of those two vectors masked.  A vector with one voxel of the volume in it lies
// inside the volume's allocation, because the allocation starts 16-byte aligned and ends with more than 16 bytes of padding; for an index image
// (`tight`: a caller's buffer) the voxels of a partial vector are loaded one by one instead.  Lanes without a voxel do not load.  !VEC: one voxel
// per load, 16 wave-wide loads of 64 consecutive voxels, for runs whose starts share no alignment.
// Counting.  Each wave owns VV_HIST_COPIES interleaved 256-bin uint32 sub-histograms in LDS (lane l adds to copy l % COPIES, word bin * COPIES +
// copy).  A lane merges runs of equal bins among its 16 voxels into one ds_add: a volume that is mostly one value (medical data, the brain
// phantom) would otherwise have 64 lanes adding to one word 16 times a trip.  The bin is the only data-dependent index and index_of clamps it.
// f32 voxels also keep, per lane, the largest key and the largest complemented key of the non-NaN voxels (pin 2: integer keys, total order of the
// bit patterns, nothing is flushed) and the number of NaNs.  A block's share is at most 2^31 voxels (launch_hist), so no uint32 counter wraps.
// Flush.  Per block: one 64-bit atomicAdd per non-zero bin, one for the NaN count, one atomicMax per key.  Integer adds and maxima: the result does
// not depend on the order of arrival.
#include "vv_device.h"
#include "vv_kernels.h"

#ifndef VV_HIST_COPIES
#define VV_HIST_COPIES 4          // sub-histograms per wave (profiles/hist_c3.txt)
#endif
#ifndef VV_HIST_MERGE
#define VV_HIST_MERGE 1           // 1: a lane adds a run of equal bins among its 16 voxels at once; 0: every voxel by itself (A/B only)
#endif
#ifndef VV_HIST_WAVES
#define VV_HIST_WAVES 8           // waves per block; the grid is 32 / VV_HIST_WAVES blocks per CU: fewer, larger blocks flush fewer atomics (profiles/hist_c3.txt)
#endif
static_assert(VV_HIST_WAVES == 4 || VV_HIST_WAVES == 8 || VV_HIST_WAVES == 16, "VV_HIST_WAVES: 4, 8 or 16 (the flush wants 256 threads at least)");
static_assert(VV_HIST_COPIES >= 1 && VV_HIST_COPIES <= 16 && (VV_HIST_COPIES & (VV_HIST_COPIES - 1)) == 0, "VV_HIST_COPIES: a power of two up to 16");

namespace vv {

constexpr int kHistWaves = VV_HIST_WAVES;     // waves per block
constexpr int kHistChunk = 1024;              // voxels per trip of a wave: 16 per lane
constexpr int kHistBlocksPerCU = 32 / kHistWaves;     // default grid: this many blocks per CU (32 waves: a CU's full complement)

struct HistKernelArgs {
    HistRuns R;
    uint32_t head;                  // VEC: voxels between the 16-byte boundary at or below a run's first voxel and that voxel (the same for every run)
    uint32_t cpr;                   // chunks per run
    uint32_t dk, dry, drz;          // the grid's stride (gridDim.x * kHistWaves pairs) as digits: chunks, rows (with the carry of the chunks), slices
    unsigned long long *acc;
};

// (hist_key / hist_key_inverse, the total-order keys of binary32 bit patterns: vv_device.h)
template <int VOXEL, bool VEC>
__global__ __launch_bounds__(64 * kHistWaves) void hist_kernel(HistKernelArgs A)
{
    constexpr int C = VV_HIST_COPIES;
    constexpr bool F32 = VOXEL == VV_VOXEL_F32;
    constexpr int SIZE = F32 ? 4 : 1, VPV = 16 / SIZE, NV = 16 / VPV;      // voxel bytes, voxels per vector, vectors per lane and trip
    __shared__ uint32_t sub[kHistWaves * 256 * C];
    __shared__ uint32_t red[kHistWaves][3];
    for (int i = threadIdx.x; i < kHistWaves * 256 * C; i += 64 * kHistWaves) sub[i] = 0;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *mine = sub + wave * (256 * C) + (lane & (C - 1));
    uint32_t kmax = 0, knmin = 0, nans = 0;            // f32: max key, max ~key (0: no voxel yet; no key of a non-NaN voxel is 0 or ~0), NaN voxels

    // this wave's first pair, then the grid's stride digit by digit
    const uint32_t first = blockIdx.x * kHistWaves + wave;
    uint32_t k = first % A.cpr, ry = (first / A.cpr) % A.R.rps, rz = (first / A.cpr) / A.R.rps;
    const uint64_t end = (uint64_t)A.head + A.R.run_voxels;                // positions count voxels from the run's vector boundary
    while (rz < A.R.n_slices) {
        const char *run = (const char *)A.R.data0 + (uint64_t)rz * A.R.slice_step + (uint64_t)ry * A.R.row_step - (size_t)A.head * SIZE;
        const uint64_t p_chunk = (uint64_t)k * kHistChunk;
        uint32_t v[16];                                                    // the lane's voxels: bytes, or binary32 bit patterns
        uint32_t mask = 0;                                                 // bit e: v[e] is a voxel of the run
        if (VEC) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const uint64_t p0 = p_chunk + (uint32_t)(j * 64 * VPV) + lane * VPV;
                // the vector's voxels [lo, hi) belong to the run
                const int64_t to_head = (int64_t)A.head - (int64_t)p0, to_end = (int64_t)end - (int64_t)p0;
                const int lo = (int)(to_head < 0 ? 0 : (to_head > VPV ? VPV : to_head)), hi = (int)(to_end < 0 ? 0 : (to_end > VPV ? VPV : to_end));
                const uint32_t m = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
                const char *src = run + p0 * SIZE;
                uint4 q = make_uint4(0, 0, 0, 0);
                if (m == (1u << VPV) - 1u || (m && !A.R.tight)) q = *(const uint4 *)src;
                else if (m) {                                              // a caller's buffer: only its own bytes
                    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int e = 0; e < VPV; ++e)
                        if ((m >> e) & 1u) { if (F32) w[e] = ((const uint32_t *)src)[e]; else w[e >> 2] |= (uint32_t)((const uint8_t *)src)[e] << (8 * (e & 3)); }
                    q = make_uint4(w[0], w[1], w[2], w[3]);
                }
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < VPV; ++e) v[j * VPV + e] = F32 ? w[e] : (w[e >> 2] >> (8 * (e & 3))) & 255u;
                mask |= m << (j * VPV);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint64_t p = p_chunk + (uint32_t)(e * 64) + lane;
                const bool in = p < end;                                   // (head = 0)
                v[e] = 0;
                if (in) v[e] = F32 ? ((const uint32_t *)run)[p] : (uint32_t)((const uint8_t *)run)[p];
                mask |= (uint32_t)in << e;
            }
        }
        // bins, with runs of equal bins merged into one add
        uint32_t cur = 0, cnt = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const bool in = (mask >> e) & 1u;
            const uint32_t b = F32 ? index_of<VV_VOXEL_F32>(__uint_as_float(v[e])) : index_of<VV_VOXEL_U8>((float)v[e]);
            if (in && (b != cur || !VV_HIST_MERGE) && cnt) { atomicAdd(mine + cur * C, cnt); cnt = 0; }
            if (in) { cur = b; ++cnt; }
            if (F32) {
                const bool nan = (v[e] & 0x7FFFFFFFu) > 0x7F800000u;
                const uint32_t key = hist_key(v[e]);
                if (in && nan) ++nans;
                if (in && !nan) { kmax = max(kmax, key); knmin = max(knmin, ~key); }
            }
        }
        if (cnt) atomicAdd(mine + cur * C, cnt);

        k += A.dk;
        uint32_t carry = k >= A.cpr;
        if (carry) k -= A.cpr;
        ry += A.dry + carry;
        carry = ry >= A.R.rps;
        if (carry) ry -= A.R.rps;
        rz += A.drz + carry;
    }

    // flush: keys and NaN count wave, block, grid; bins block, grid
    if (F32) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
            knmin = max(knmin, (uint32_t)__shfl_xor((int)knmin, o));
            nans += (uint32_t)__shfl_xor((int)nans, o);
        }
        if (lane == 0) { red[wave][0] = kmax; red[wave][1] = knmin; red[wave][2] = nans; }
    }
    __syncthreads();
    if (F32 && threadIdx.x == 0) {
        uint32_t a = 0, b = 0, n = 0;
        for (int w = 0; w < kHistWaves; ++w) { a = max(a, red[w][0]); b = max(b, red[w][1]); n += red[w][2]; }
        uint32_t *keys = (uint32_t *)(A.acc + kHistAccKeys);
        if (a) { atomicMax(keys, a); atomicMax(keys + 1, b); }
        if (n) atomicAdd(A.acc + kHistAccNan, (unsigned long long)n);
    }
    if (threadIdx.x < 256) {
        const uint32_t bin = threadIdx.x;                                  // one thread per bin
        uint32_t sum = 0;
        for (int w = 0; w < kHistWaves; ++w)
#pragma unroll
            for (int c = 0; c < C; ++c) sum += sub[w * (256 * C) + bin * C + c];
        if (sum) atomicAdd(A.acc + bin, (unsigned long long)sum);
    }
}

// accumulator -> vv_histogram at `out`, or the counts alone at `counts` (out = null).  One block of 256 threads.
__global__ __launch_bounds__(256) void hist_finish_kernel(const unsigned long long *acc, int vtype, unsigned long long voxels, vv_histogram *out,
                                                          unsigned long long *counts)
{
    __shared__ uint32_t lo, hi;
    const uint32_t t = threadIdx.x;
    const unsigned long long n = acc[t];
    (out ? out->counts : counts)[t] = n;
    if (!out) return;
    if (t == 0) { lo = 0xFFFFFFFFu; hi = 0; }
    __syncthreads();
    if (n) { atomicMin(&lo, t); atomicMax(&hi, t); }                       // u8 volumes: the range is the lowest and the highest bin in use
    __syncthreads();
    if (t != 0) return;
    uint32_t bmin = 0x7F800000u, bmax = 0xFF800000u;                       // no non-NaN voxel: +Inf, -Inf
    if (vtype == VV_VOXEL_F32) {
        const uint32_t *keys = (const uint32_t *)(acc + kHistAccKeys);
        if (keys[0]) { bmax = hist_key_inverse(keys[0]); bmin = hist_key_inverse(~keys[1]); }
    } else if (lo <= hi) {
        bmin = __float_as_uint((float)lo); bmax = __float_as_uint((float)hi);
    }
    out->voxels = voxels;
    out->nan_voxels = acc[kHistAccNan];
    *(uint32_t *)&out->vmin = bmin;                                        // bit patterns: stored as integers, whatever the unit's denormal mode
    *(uint32_t *)&out->vmax = bmax;
}

template <int VOXEL>
static void launch_hist_vec(const HistKernelArgs &a, bool vec, int grid, hipStream_t s)
{
    if (vec) hipLaunchKernelGGL((hist_kernel<VOXEL, true>),  dim3(grid), dim3(64 * kHistWaves), 0, s, a);
    else     hipLaunchKernelGGL((hist_kernel<VOXEL, false>), dim3(grid), dim3(64 * kHistWaves), 0, s, a);
}

void launch_hist(const HistRuns &r, int n_cu, int max_blocks, unsigned long long *acc, hipStream_t s)
{
    HistKernelArgs a;
    a.R = r; a.acc = acc;
    const uint32_t size = r.vtype == VV_VOXEL_F32 ? 4 : 1;
    // 16-byte loads: every run starts at the same offset from a 16-byte boundary
    const bool vec = (uint64_t)r.rps * r.n_slices == 1 || (r.row_step % 16 == 0 && r.slice_step % 16 == 0);
    a.head = vec ? (uint32_t)(((uintptr_t)r.data0 & 15u) / size) : 0u;
    a.cpr = (uint32_t)((a.head + r.run_voxels + kHistChunk - 1) / kHistChunk);
    const uint64_t pairs = (uint64_t)a.cpr * r.rps * r.n_slices;
    // one wave per pair up to the cap; never so few blocks that one of them counts 2^31 voxels (2^20 pairs and a trip per wave)
    uint64_t grid = (pairs + kHistWaves - 1) / kHistWaves;
    const uint64_t cap = max_blocks > 0 ? (uint64_t)max_blocks : (uint64_t)(n_cu > 0 ? n_cu : 256) * kHistBlocksPerCU;
    if (grid > cap) grid = cap;
    const uint64_t least = (pairs + (1ull << 20) - 1) >> 20;
    if (grid < least) grid = least;
    const uint64_t stride = grid * kHistWaves, dq = stride / a.cpr;
    a.dk = (uint32_t)(stride % a.cpr); a.dry = (uint32_t)(dq % r.rps); a.drz = (uint32_t)(dq / r.rps);
    if (r.vtype == VV_VOXEL_F32) launch_hist_vec<VV_VOXEL_F32>(a, vec, (int)grid, s);
    else                         launch_hist_vec<VV_VOXEL_U8>(a, vec, (int)grid, s);
}

void launch_hist_finish(const unsigned long long *acc, int vtype, unsigned long long voxels, vv_histogram *out, unsigned long long *counts, hipStream_t s)
{
    hipLaunchKernelGGL(hist_finish_kernel, dim3(1), dim3(256), 0, s, acc, vtype, voxels, out, counts);
}

} // namespace vv
