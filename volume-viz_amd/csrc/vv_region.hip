// vv_region.hip -- region measurements for gfx950: the regions of a label volume ranked device-wide, relabelled 1..K and measured into one table row each
// (no reference counterpart; the contract is the comment on vv_region_table in include/volviz.h).
//
//   region_count_kernel      launch 1: the roots of every chunk counted (ballot + popcount), one partial per chunk; the non-zero labels counted
//   region_scan_kernel       launch 2: one block turns the partials into exclusive offsets and writes K
//   region_rank_kernel       launch 3: every root gets compact[r] = rank + 1 and, below max_regions, initialises its row
//   region_measure_kernel    launch 4: every voxel finds its row, writes its own compact word and adds itself to the row, combined per wave
//   region_finish_kernel     launch 5: keys back to floats, the aux slot unpacked, hi made exclusive, the summary
//
// Representation.  i numbers the box's voxels, x fastest (vv_label_volume's rule 4).  VV_REGION_LABELS: voxel r is a ROOT iff labels[r] == r + 1; voxel i
// is OWNED by root r iff labels[i] != 0, r = labels[i] - 1 < voxels and labels[r] == r + 1; any other non-zero label is a STRAY.  VV_REGION_NONZERO: the one
// root is the least i with labels[i] != 0 and owns every non-zero voxel.  The rank of a root is the number of roots below it.
//
// Chunks.  The box's indices are cut into `nchunks` runs of chunk_len = max(kRegionMinChunk, ceil(voxels / cap)) voxels, rounded up to the wave size; cap is
// kRegionMaxChunks, or VV_REGION_CHUNKS where that is lower.  A chunk is walked by ONE wave, 64 consecutive voxels a step, front to back: the roots it has
// met so far are a wave-uniform number, so a root's rank is the chunk's offset + that number + the ballot's prefix, with no barrier.  A block of
// kRgWaves waves takes kRgWaves consecutive chunks (a contiguous span); VV_REGION_BLOCKS caps every grid, the loop then takes blockIdx.x, + gridDim.x, ...
//
// Phases.  Launch boundaries are the only synchronisation between blocks: no kernel waits for another block or wave, there is no spin, no look-back, no
// grid barrier and no cooperative launch; the launches are five for any data (VV_REGION_PHASES cuts them short for timing).  No host read-back.
//
// Ownership of every word, and why each cross-block read is safe:
//  labels, aux, the volume    read-only in all five launches: a plain load sees what the caller put there, whatever block reads it.  The ownership test of
//                             launch 4 (labels[labels[i] - 1] == labels[i]) and the six face neighbours read only these.
//  partials[c]                written by the wave of chunk c in launch 1; read and rewritten (as offsets) by the one block of launch 2; read by the wave of
//                             chunk c in launch 3.  hdr (foreground, stray, first, K): atomics of launches 1 and 4, written in 2, read in 3, 4, 5 only behind
//                             the launch that completed them (first: 1 -> 2, 3, 4; K: 2 -> 5; foreground: 1 -> 5; stray: 4 -> 5).
//  compact[r], r a root       written in launch 3 by r's own thread, and in no other launch.  Launch 4 reads compact[] ONLY at an index r that it has just
//                             proved a root from `labels`, so every word it reads was completed by launch 3 and nobody writes it meanwhile.
//  compact[i], i no root      written in launch 4 by i's own thread (0 for background and strays), read by nobody in this call.  A label that points at a
//                             non-root (caller data) therefore never makes a thread read a word another thread of the same launch writes: such a voxel
//                             fails the test on `labels` and is a stray before compact is touched.  Launch 3 need not define these words.
//  table rows < written       initialised in launch 3 by the root's thread; in launch 4 only atomics (64-bit adds, 32-bit min / max, one 64-bit max: integers,
//                             so the arrival order does not matter); in launch 5 each row is rewritten by one thread.
// Addresses.  labels[r], compact[r] are indexed only behind r < voxels; a row only behind rank < max_regions, rank read from a root's compact word, which
// launch 3 wrote below K; a face neighbour only inside the box.  No label makes an address unchecked.
//
// Combining (launch 4).  A wave keeps, in registers, the partial sums of TWO regions cur0 and cur1, lane by lane: a lane whose voxel belongs to one of
// them adds to its own registers and nothing leaves the lane.  The voxels of a step that belong to other regions are taken region by region (the first
// such lane's rank, a ballot of the lanes that share it).  A region with kRgKeep voxels or more in the step takes a slot that is empty, or else the slot
// whose region is absent from this step (of two absent ones the one idle longest): the old region is reduced across the wave and leaves as one set of
// atomics.  One or two voxels, and (rarely) the voxels of a third region while both slots are busy in the step, add themselves.  Both slots
// are flushed when the wave is done.  A giant component, whatever share of a step's lanes it holds, so costs a wave one set of atomics, not one per
// voxel or per step; two structures that alternate along a row (nested shells) do not evict each other.  (The first form kept one region and took a
// new one only when it held more than half of a step: a component of density 0.31 never did.  profiles/regions_c3.txt, part 3.)
//
// Termination.  Every loop is counted (chunks, steps, rows, scan strides) except the loop over the distinct ranks of a step, which clears at least the
// leader's bit of a 64-bit mask on every trip.
// No scalar-memory stores, no inline assembly, no xnack.
#include "vv_device.h"
#include "vv_kernels.h"
#include <algorithm>

namespace vv {

constexpr int kRgWaves = 4, kRgThreads = 64 * kRgWaves;
constexpr int kRgScanThreads = 1024, kRgScanPer = kRegionMaxChunks / kRgScanThreads;
constexpr uint32_t kRgNone = 0xFFFFFFFFu;
constexpr int kRgKeep = 3;                                  // launch 4: a region with at least this many voxels in a step may take a register slot
static_assert(kRegionMaxChunks % kRgScanThreads == 0, "the scan block takes a whole number of partials per thread");

struct RegionKernelArgs {
    RegionArgs A;
    uint64_t voxels, chunk_len;
    uint32_t nchunks;
};

__global__ __launch_bounds__(kRgThreads) void region_count_kernel(RegionKernelArgs K)
{
    __shared__ unsigned long long fg_s[kRgWaves];
    const RegionArgs &A = K.A;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool nonzero = A.source == VV_REGION_NONZERO;
    unsigned long long fg = 0;                                               // wave-uniform
    uint32_t first = 0;                                                      // NONZERO: 0xFFFFFFFF - the least non-zero index this wave met (0: none)
    for (uint32_t g = blockIdx.x; g * kRgWaves < K.nchunks; g += gridDim.x) {
        const uint32_t chunk = g * kRgWaves + wave;
        if (chunk >= K.nchunks) continue;
        const uint64_t begin = (uint64_t)chunk * K.chunk_len, end = min(begin + K.chunk_len, K.voxels);
        uint32_t roots = 0;
        for (uint64_t i0 = begin; i0 < end; i0 += 64) {
            const uint64_t i = i0 + lane;
            const bool in = i < end;
            const uint32_t lab = in ? A.labels[i] : 0u;
            const unsigned long long nz = __ballot(lab != 0);
            fg += (unsigned long long)__popcll(nz);
            if (nonzero) {
                if (nz && !first) first = kRgNone - (uint32_t)(i0 + (uint32_t)(__ffsll(nz) - 1));      // (chunks and steps ascend: the first hit is the least)
            } else roots += (uint32_t)__popcll(__ballot(in && lab == (uint32_t)i + 1u));
        }
        if (lane == 0) A.partials[chunk] = roots;
    }
    if (lane == 0) {
        fg_s[wave] = fg;
        if (first) atomicMax((uint32_t *)(A.hdr + kRegionFirst), first);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < kRgWaves; ++w) sum += fg_s[w];
        if (sum) atomicAdd(A.hdr + kRegionForeground, sum);
    }
}

__global__ __launch_bounds__(kRgScanThreads) void region_scan_kernel(RegionKernelArgs K)
{
    __shared__ uint32_t s[kRgScanThreads];
    const RegionArgs &A = K.A;
    const uint32_t t = threadIdx.x;
    uint32_t v[kRgScanPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kRgScanPer; ++k) {
        const uint32_t idx = t * kRgScanPer + k;
        v[k] = idx < K.nchunks ? A.partials[idx] : 0u;
        sum += v[k];                                                         // (all roots together are at most the box's voxels: below 2^32)
    }
    s[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kRgScanThreads; off <<= 1) {
        const uint32_t x = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    uint32_t excl = s[t] - sum;
#pragma unroll
    for (int k = 0; k < kRgScanPer; ++k) {
        const uint32_t idx = t * kRgScanPer + k;
        if (idx < K.nchunks) A.partials[idx] = excl;
        excl += v[k];
    }
    if (t == kRgScanThreads - 1)
        A.hdr[kRegionCount] = A.source == VV_REGION_NONZERO ? (unsigned long long)(*(const uint32_t *)(A.hdr + kRegionFirst) != 0) : (unsigned long long)s[t];
}

// the row of a region before launch 4: the label, the identities of the minima and maxima (hi holds the largest coordinate, vmin / vmax the keys, the
// aux slot the packed key until launch 5), zeros
__device__ __forceinline__ void region_row_init(vv_region *r, uint32_t label)
{
    r->label = label; r->reserved = 0; r->voxels = 0;
    for (int a = 0; a < 3; ++a) { r->lo[a] = 0x7FFFFFFF; r->hi[a] = 0; r->sum[a] = 0; r->faces[a] = 0; }
    for (int a = 0; a < 6; ++a) r->sum2[a] = 0;
    r->bin_min = kRgNone; r->bin_max = 0; r->bin_sum = 0; r->bin_sum2 = 0;
    *(uint32_t *)&r->vmin = kRgNone; *(uint32_t *)&r->vmax = 0;
    r->aux_sum = 0; r->aux_argmax = 0; r->aux_max = 0;
}

__global__ __launch_bounds__(kRgThreads) void region_rank_kernel(RegionKernelArgs K)
{
    const RegionArgs &A = K.A;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (A.source == VV_REGION_NONZERO) {                                      // one root at most: the least non-zero voxel
        const uint32_t first = *(const uint32_t *)(A.hdr + kRegionFirst);
        if (blockIdx.x == 0 && threadIdx.x == 0 && first) {
            const uint32_t r = kRgNone - first;
            A.compact[r] = 1u;
            if (A.max_regions) region_row_init(A.table, r + 1u);
        }
        return;
    }
    for (uint32_t g = blockIdx.x; g * kRgWaves < K.nchunks; g += gridDim.x) {
        const uint32_t chunk = g * kRgWaves + wave;
        if (chunk >= K.nchunks) continue;
        const uint64_t begin = (uint64_t)chunk * K.chunk_len, end = min(begin + K.chunk_len, K.voxels);
        uint32_t base = A.partials[chunk];                                    // roots below this chunk, then below this step: wave-uniform
        for (uint64_t i0 = begin; i0 < end; i0 += 64) {
            const uint64_t i = i0 + lane;
            const bool root = i < end && A.labels[i] == (uint32_t)i + 1u;
            const unsigned long long m = __ballot(root);
            if (root) {
                const uint32_t rank = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                A.compact[i] = rank + 1u;
                if (rank < A.max_regions) region_row_init(A.table + rank, (uint32_t)i + 1u);
            }
            base += (uint32_t)__popcll(m);
        }
    }
}

// What one voxel, one lane over many steps or one wave adds to a row.  s: voxels, sum x y z, sum2 xx yy zz xy xz yz, bin_sum, bin_sum2, faces x y z, aux_sum.
// mn / mx: x, y, z, bin, value key (mx[4] == 0: no value that is not a NaN).  key: aux_max << 32 | (0xFFFFFFFF - i), 0 without aux.
struct RegionPart {
    unsigned long long s[16];
    uint32_t mn[5], mx[5];
    unsigned long long key;
};
__device__ __forceinline__ void part_clear(RegionPart &p)
{
#pragma unroll
    for (int k = 0; k < 16; ++k) p.s[k] = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { p.mn[k] = kRgNone; p.mx[k] = 0; }
    p.key = 0;
}
// one voxel of a region as launch 4 holds it before it is added anywhere: volume coordinates, bin, value key (0: a NaN), faces per axis, aux, box index
struct RegionVoxel {
    uint32_t X, Y, Z, bin, key, f[3], av, i;
};
__device__ __forceinline__ void part_add_voxel(RegionPart &p, const RegionVoxel &v, bool has_aux)
{
    const unsigned long long X = v.X, Y = v.Y, Z = v.Z;
    p.s[0] += 1;
    p.s[1] += X; p.s[2] += Y; p.s[3] += Z;
    p.s[4] += X * X; p.s[5] += Y * Y; p.s[6] += Z * Z; p.s[7] += X * Y; p.s[8] += X * Z; p.s[9] += Y * Z;
    p.s[10] += v.bin; p.s[11] += (unsigned long long)(v.bin * v.bin);
#pragma unroll
    for (int a = 0; a < 3; ++a) p.s[12 + a] += v.f[a];
    p.mn[0] = min(p.mn[0], v.X); p.mn[1] = min(p.mn[1], v.Y); p.mn[2] = min(p.mn[2], v.Z); p.mn[3] = min(p.mn[3], v.bin);
    p.mx[0] = max(p.mx[0], v.X); p.mx[1] = max(p.mx[1], v.Y); p.mx[2] = max(p.mx[2], v.Z); p.mx[3] = max(p.mx[3], v.bin);
    if (v.key) { p.mn[4] = min(p.mn[4], v.key); p.mx[4] = max(p.mx[4], v.key); }      // (no key of a value that is not a NaN is 0 or ~0)
    if (has_aux) {
        p.s[15] += v.av;
        p.key = max(p.key, ((unsigned long long)v.av << 32) | (unsigned long long)(kRgNone - v.i));
    }
}
// every lane's part combined: all 64 lanes hold the result
__device__ __forceinline__ void part_wave_reduce(RegionPart &p)
{
#pragma unroll 1
    for (int o = 32; o >= 1; o >>= 1) {                                       // (a loop, not six copies: the reduction is rare and its copies cost the kernel registers)
#pragma unroll
        for (int k = 0; k < 16; ++k) p.s[k] += __shfl_xor(p.s[k], o);
#pragma unroll
        for (int k = 0; k < 5; ++k) { p.mn[k] = min(p.mn[k], (uint32_t)__shfl_xor((int)p.mn[k], o)); p.mx[k] = max(p.mx[k], (uint32_t)__shfl_xor((int)p.mx[k], o)); }
        p.key = max(p.key, __shfl_xor(p.key, o));
    }
}
// one set of atomics (a part with no voxel is not emitted by the callers)
__device__ __forceinline__ void part_emit(vv_region *r, const RegionPart &p, bool has_aux)
{
    atomicAdd(&r->voxels, p.s[0]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (p.s[1 + a]) atomicAdd(&r->sum[a], p.s[1 + a]);
        if (p.s[12 + a]) atomicAdd(&r->faces[a], p.s[12 + a]);
        atomicMin((uint32_t *)&r->lo[a], p.mn[a]);                            // (coordinates are not negative: the unsigned order is the signed one)
        atomicMax((uint32_t *)&r->hi[a], p.mx[a]);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
        if (p.s[4 + a]) atomicAdd(&r->sum2[a], p.s[4 + a]);
    if (p.s[10]) { atomicAdd(&r->bin_sum, p.s[10]); atomicAdd(&r->bin_sum2, p.s[11]); }
    atomicMin(&r->bin_min, p.mn[3]);
    atomicMax(&r->bin_max, p.mx[3]);
    if (p.mx[4]) { atomicMin((uint32_t *)&r->vmin, p.mn[4]); atomicMax((uint32_t *)&r->vmax, p.mx[4]); }
    if (has_aux) {
        if (p.s[15]) atomicAdd(&r->aux_sum, p.s[15]);
        atomicMax((unsigned long long *)&r->aux_argmax, p.key);               // (aux_argmax and aux_max: one 8-byte aligned slot, low word first)
    }
}

// one voxel by itself: the same set of atomics from its own values
__device__ __forceinline__ void voxel_emit(vv_region *r, const RegionVoxel &v, bool has_aux)
{
    const unsigned long long c[3] = {v.X, v.Y, v.Z};
    atomicAdd(&r->voxels, 1ull);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (c[a]) { atomicAdd(&r->sum[a], c[a]); atomicAdd(&r->sum2[a], c[a] * c[a]); }
        if (v.f[a]) atomicAdd(&r->faces[a], (unsigned long long)v.f[a]);
        atomicMin((uint32_t *)&r->lo[a], (uint32_t)c[a]);
        atomicMax((uint32_t *)&r->hi[a], (uint32_t)c[a]);
    }
    if (c[0] * c[1]) atomicAdd(&r->sum2[3], c[0] * c[1]);
    if (c[0] * c[2]) atomicAdd(&r->sum2[4], c[0] * c[2]);
    if (c[1] * c[2]) atomicAdd(&r->sum2[5], c[1] * c[2]);
    if (v.bin) { atomicAdd(&r->bin_sum, (unsigned long long)v.bin); atomicAdd(&r->bin_sum2, (unsigned long long)(v.bin * v.bin)); }
    atomicMin(&r->bin_min, v.bin);
    atomicMax(&r->bin_max, v.bin);
    if (v.key) { atomicMin((uint32_t *)&r->vmin, v.key); atomicMax((uint32_t *)&r->vmax, v.key); }
    if (has_aux) {
        if (v.av) atomicAdd(&r->aux_sum, (unsigned long long)v.av);
        atomicMax((unsigned long long *)&r->aux_argmax, ((unsigned long long)v.av << 32) | (unsigned long long)(kRgNone - v.i));
    }
}

// the sums a wave kept for rank `cur` leave it as one set of atomics, and the slot is empty again (all lanes call it; cur is wave-uniform)
__device__ __forceinline__ void region_flush(vv_region *table, uint32_t cur, RegionPart &acc, uint32_t lane, bool has_aux)
{
    if (cur == kRgNone) return;
    part_wave_reduce(acc);
    if (lane == 0 && acc.s[0]) part_emit(table + cur, acc, has_aux);
    part_clear(acc);
}

template <int SRC>
__global__ __launch_bounds__(kRgThreads) void region_measure_kernel(RegionKernelArgs K)
{
    constexpr bool F32 = SRC == VV_VOXEL_F32;
    constexpr int SIZE = F32 ? 4 : 1;
    __shared__ unsigned long long stray_s[kRgWaves];
    const RegionArgs &A = K.A;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool nonzero = A.source == VV_REGION_NONZERO, has_aux = A.aux != nullptr;
    const uint32_t first = nonzero ? *(const uint32_t *)(A.hdr + kRegionFirst) : 0u;
    const uint64_t plane = (uint64_t)A.b[0] * A.b[1];
    unsigned long long stray = 0;                                            // wave-uniform
    uint32_t cur0 = kRgNone, cur1 = kRgNone;                                 // wave-uniform: the two ranks whose sums this wave keeps in acc0 / acc1
    uint32_t seen0 = 0, seen1 = 0, now = 0;                                  // wave-uniform: the step that last held a voxel of cur0 / cur1; the step's number
    RegionPart acc0, acc1;
    part_clear(acc0);
    part_clear(acc1);
    for (uint32_t g = blockIdx.x; g * kRgWaves < K.nchunks; g += gridDim.x) {
        const uint32_t chunk = g * kRgWaves + wave;
        if (chunk >= K.nchunks) continue;
        const uint64_t begin = (uint64_t)chunk * K.chunk_len, end = min(begin + K.chunk_len, K.voxels);
        uint32_t lab_next = begin + lane < end ? A.labels[begin + lane] : 0u;
        for (uint64_t i0 = begin; i0 < end; i0 += 64) {
            const uint64_t i = i0 + lane;
            const bool in = i < end;
            const uint32_t lab = lab_next;
            lab_next = i + 64 < end ? A.labels[i + 64] : 0u;                  // the next step's label is on its way while this step is worked on
            ++now;
            bool owned = false, root = false;
            uint32_t rank = 0;
            if (nonzero) {
                owned = lab != 0;
                root = owned && kRgNone - (uint32_t)i == first;
            } else if (lab != 0) {
                const uint32_t r = lab - 1u;
                if ((uint64_t)r < K.voxels && (r == (uint32_t)i || A.labels[r] == lab)) {     // rule 1, on `labels` alone
                    owned = true;
                    root = r == (uint32_t)i;
                    rank = A.compact[r] - 1u;                                // a root's word: launch 3 wrote it, nobody writes it now
                }
            }
            stray += (unsigned long long)__popcll(__ballot(lab != 0 && !owned));
            if (in && !root) A.compact[i] = owned ? rank + 1u : 0u;
            const bool tracked = owned && rank < A.max_regions;
            unsigned long long act = __ballot(tracked);
            if (!act) continue;
            RegionVoxel v = {};
            if (tracked) {
                const uint32_t q = (uint32_t)(i / A.b[0]), x = (uint32_t)(i - (uint64_t)q * A.b[0]), z = q / A.b[1], y = q - z * A.b[1];
                v.X = (uint32_t)(A.lo[0] + (int32_t)x); v.Y = (uint32_t)(A.lo[1] + (int32_t)y); v.Z = (uint32_t)(A.lo[2] + (int32_t)z); v.i = (uint32_t)i;
                const char *at = (const char *)A.src0 + ((uint64_t)z * A.slice_pitch + (uint64_t)y * A.row_pitch + (uint64_t)x * SIZE);
                uint32_t bin, raw;
                if constexpr (F32) { raw = *(const uint32_t *)at; bin = index_of<VV_VOXEL_F32>(__uint_as_float(raw)); }
                else { bin = (uint32_t)*(const uint8_t *)at; raw = __float_as_uint((float)bin); }
                v.bin = bin;
                v.key = (raw & 0x7FFFFFFFu) <= 0x7F800000u ? hist_key(raw) : 0u;
                // faces: a neighbour outside the box or not owned by the same root (same root <=> the same label, given this voxel is owned)
                const uint32_t pos[3] = {x, y, z};
                const uint64_t step[3] = {1ull, (uint64_t)A.b[0], plane};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    uint32_t n = 0;
                    if (pos[a] == 0) ++n;
                    else { const uint32_t nl = A.labels[i - step[a]]; n += nonzero ? nl == 0 : nl != lab; }
                    if (pos[a] + 1u == A.b[a]) ++n;
                    else { const uint32_t nl = A.labels[i + step[a]]; n += nonzero ? nl == 0 : nl != lab; }
                    v.f[a] = n;
                }
                if (has_aux) v.av = A.aux[i];
            }
            bool here0 = false, here1 = false;                                // wave-uniform: this step holds a voxel of cur0 / cur1
            if (cur0 != kRgNone) {
                const bool mine = tracked && rank == cur0;
                const unsigned long long m = __ballot(mine);
                if (mine) part_add_voxel(acc0, v, has_aux);
                if (m) { here0 = true; seen0 = now; act &= ~m; }
            }
            if (cur1 != kRgNone) {
                const bool mine = tracked && rank == cur1;
                const unsigned long long m = __ballot(mine);
                if (mine) part_add_voxel(acc1, v, has_aux);
                if (m) { here1 = true; seen1 = now; act &= ~m; }
            }
            while (act) {
                const int leader = __ffsll(act) - 1;
                const uint32_t rk = (uint32_t)__shfl((int)rank, leader);
                const bool mine = tracked && rank == rk;
                const unsigned long long m = __ballot(mine);
                const int n = __popcll(m);
                if (n >= kRgKeep && !(here0 && here1)) {                      // kept in registers from here on, in the slot that is free or was idle longest
                    const bool slot0 = cur0 == kRgNone ? true : cur1 == kRgNone ? false : here0 ? false : here1 ? true : seen0 <= seen1;
                    if (slot0) {
                        region_flush(A.table, cur0, acc0, lane, has_aux);
                        cur0 = rk; here0 = true; seen0 = now;
                        if (mine) part_add_voxel(acc0, v, has_aux);
                    } else {
                        region_flush(A.table, cur1, acc1, lane, has_aux);
                        cur1 = rk; here1 = true; seen1 = now;
                        if (mine) part_add_voxel(acc1, v, has_aux);
                    }
                } else if (mine) voxel_emit(A.table + rk, v, has_aux);       // one or two voxels, or both slots busy in this step: each voxel adds itself
                act &= ~m;
            }
        }
    }
    region_flush(A.table, cur0, acc0, lane, has_aux);
    region_flush(A.table, cur1, acc1, lane, has_aux);
    if (lane == 0) stray_s[wave] = stray;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int w = 0; w < kRgWaves; ++w) sum += stray_s[w];
        if (sum) atomicAdd(A.hdr + kRegionStray, sum);
    }
}

__global__ __launch_bounds__(kRgThreads) void region_finish_kernel(RegionKernelArgs K)
{
    const RegionArgs &A = K.A;
    const unsigned long long regions = A.hdr[kRegionCount], written = regions < A.max_regions ? regions : (unsigned long long)A.max_regions;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kRgThreads + threadIdx.x; k < written; k += (unsigned long long)gridDim.x * kRgThreads) {
        vv_region *r = A.table + k;
        for (int a = 0; a < 3; ++a) r->hi[a] += 1;
        const uint32_t kmin = *(const uint32_t *)&r->vmin, kmax = *(const uint32_t *)&r->vmax;
        *(uint32_t *)&r->vmin = kmax ? hist_key_inverse(kmin) : 0x7F800000u;   // no value that is not a NaN: +Inf, -Inf (bit patterns, stored as integers)
        *(uint32_t *)&r->vmax = kmax ? hist_key_inverse(kmax) : 0xFF800000u;
        if (A.aux) r->aux_argmax = kRgNone - r->aux_argmax;
    }
    if (A.summary && blockIdx.x == 0 && threadIdx.x == 0) {
        vv_region_summary s;
        s.regions = regions; s.written = written;
        s.foreground = A.hdr[kRegionForeground]; s.stray = A.hdr[kRegionStray];
        *A.summary = s;
    }
}

void launch_region(const RegionArgs &a, int max_blocks, int max_chunks, int phases, hipStream_t s)
{
    RegionKernelArgs k;
    k.A = a;
    k.voxels = (uint64_t)a.b[0] * a.b[1] * a.b[2];
    const uint64_t cap = max_chunks > 0 && max_chunks < kRegionMaxChunks ? (uint64_t)max_chunks : (uint64_t)kRegionMaxChunks;
    const uint64_t per = (k.voxels + cap - 1) / cap, len = per > (uint64_t)kRegionMinChunk ? per : (uint64_t)kRegionMinChunk;
    k.chunk_len = (len + 63) / 64 * 64;
    k.nchunks = (uint32_t)((k.voxels + k.chunk_len - 1) / k.chunk_len);      // at most cap: rounding chunk_len up only lowers it
    uint32_t grid = (k.nchunks + kRgWaves - 1) / kRgWaves;
    if (max_blocks > 0 && grid > (uint32_t)max_blocks) grid = (uint32_t)max_blocks;
    if (grid < 1) grid = 1;
    const dim3 block(kRgThreads);
    hipLaunchKernelGGL(region_count_kernel, dim3(grid), block, 0, s, k);
    if (phases == 1) return;
    hipLaunchKernelGGL(region_scan_kernel, dim3(1), dim3(kRgScanThreads), 0, s, k);
    if (phases == 2) return;
    hipLaunchKernelGGL(region_rank_kernel, dim3(grid), block, 0, s, k);
    if (phases == 3) return;
    if (a.src_type == VV_VOXEL_F32) hipLaunchKernelGGL(region_measure_kernel<VV_VOXEL_F32>, dim3(grid), block, 0, s, k);
    else                            hipLaunchKernelGGL(region_measure_kernel<VV_VOXEL_U8>, dim3(grid), block, 0, s, k);
    if (phases == 4) return;
    uint32_t fgrid = (uint32_t)((std::min<uint64_t>(a.max_regions, k.voxels) + kRgThreads - 1) / kRgThreads);
    if (fgrid > 1024) fgrid = 1024;
    if (max_blocks > 0 && fgrid > (uint32_t)max_blocks) fgrid = (uint32_t)max_blocks;
    if (fgrid < 1) fgrid = 1;
    hipLaunchKernelGGL(region_finish_kernel, dim3(fgrid), block, 0, s, k);
}

} // namespace vv
