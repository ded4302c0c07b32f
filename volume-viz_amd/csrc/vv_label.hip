// vv_label.hip -- segmentation for gfx950: the connected components of a box of the loaded volume as canonical labels, and the loaded volume masked by
// a test on such labels (no reference counterpart; the contracts are the comments on vv_label_volume and vv_mask_volume in include/volviz.h,
// DESIGN.md section 4n).
//
//   label_local_kernel<SRC>     a tile of the box labelled in LDS; labels[i] = 1 + the tile-local root's index, 0 for background
//   label_merge_kernel          the components of neighbouring tiles joined across the tile faces: union-find on `labels` through global atomics
//   label_flatten_kernel        every voxel set to its root; tile counts added up at the roots; foreground and component counters
//   label_stats_kernel          the largest component: one 64-bit atomicMax per block over `sizes`
//   label_stats_finish_kernel   the counters turned into a vv_label_stats
//   mask_kernel<SRC, OUT>       elementwise: the source voxel where the label test holds, `fill` elsewhere
//
// Representation.  i = ((z - lo_z) b_y + (y - lo_y)) b_x + (x - lo_x) numbers the box's voxels, x fastest.  From label_local_kernel's first store on,
// labels[i] is 0 for a background voxel and p + 1 for a foreground one, p <= i the index of its parent in a forest whose roots have p == i: a slot
// never changes between "background" and "parent" and a parent only ever decreases.  Every link puts the larger root below a smaller index of the
// other tree, so a tree's root is its least voxel, and the forest at the end of label_merge_kernel has one tree per component: the label 1 + i_min
// is a property of the input, whatever the order the blocks ran in and the atomics arrived in.
//
// Tiles.  The box is cut into tiles of kLbTX x kLbTY x kLbTZ = 16 x 8 x 8 voxels, numbered x fastest; a block of 256 threads takes a tile, a thread
// the four voxels l = t, t + 256, t + 512, t + 768 of the tile's local numbering l = (lz * 8 + ly) * 16 + lx (the same lexicographic order as i, so
// the least local index of a set is its least global one).  Three kernels walk the tiles (VV_LABEL_BLOCKS caps every grid; the loop then takes
// blockIdx.x, + gridDim.x, ...).
//
// Phases.  Launch boundaries are the only synchronisation between blocks: no kernel waits for another block or wave, there is no spin, no grid
// barrier and no cooperative launch, and the number of launches depends on the arguments (sizes, stats) and never on the data.
//  local:   the foreground of the tile is formed from the voxels (the bin of vv_volume_histogram's rule 1 inside [bin_lo, bin_hi]), an LDS union-find
//           joins each foreground voxel with the foreground voxels of its backward half neighbourhood (3, 9 or 13 offsets) inside the tile, every voxel
//           reads its root, the roots count their voxels in LDS.  Stores: labels (every voxel of the box) and, with sizes, the tile count at the
//           tile-local root and 0 everywhere else.
//  merge:   every foreground voxel on a tile's surface joins the foreground voxels of its backward half neighbourhood that lie in another tile.
//           `labels` is only read by agent-scope atomic loads and only written by atomicMin here.  Per-XCD L2s are not coherent and a plain load may
//           return what the word held earlier in the launch; the algorithm is right under exactly that weakness: a parent that a find reads late is an
//           earlier parent of the same voxel, so still an ancestor-to-be in the same component, and whether a link happens is decided by the value the
//           atomicMin returns, which is exact.  The atomic loads keep the compiler from caching a word in a register and bypass the CU's L1.
//  flatten: a tile's parents go to LDS; the voxels whose parent lies outside the tile or is the voxel itself (former tile roots: the only slots merge
//           has written) find their root in global memory, every other voxel follows its parents inside LDS to such a voxel.  A concurrent block may
//           meanwhile replace a parent by its root: either value leads to the same root.  With sizes, a former tile root that is no root moves its
//           count to the root by one atomicAdd; no other thread reads or writes its slot.
//
// Termination (every loop of this file that is not a counted loop over tiles, items or offsets):
//  lds_find / lds_union     a hop goes from x to P[x] < x and stops at P[x] == x; a failed union trip continues with the value the atomicMin
//                           returned, which is below the index it was applied to, so the larger of the two indices falls with every trip.  Both loops
//                           also carry the explicit trip bound kLbTile (the tile's voxel count), which a chain of decreasing local indices cannot reach.
//                           (An in-tile propagation of labels by sweeps would need about kLbTile trips on a serpentine; the union-find needs none.)
//  global_find              stops at the first parent that is not below the index (`p >= x`, which a root and -- were one ever met -- a background slot
//                           satisfy); every hop otherwise goes to a strictly smaller index >= 0.
//  global_union             returns when both finds meet, or when the atomicMin returns nothing below the index it was applied to (the root was
//                           linked); otherwise continues with that returned smaller index: the larger index falls with every trip.
//  flatten's walk in LDS    an unresolved voxel's parent is a smaller local index; bounded by kLbTile as well.
// Addresses.  Every index that addresses `labels` or `sizes` is a voxel's own index or was reached from one by decreasing hops: never above the box's
// last voxel.  mask_kernel takes labels from the caller: it compares them and, for VV_KEEP_MIN_SIZE, indexes `sizes` only behind label - 1 < voxels.
// No scalar-memory stores, no inline assembly, no xnack.
#include "vv_device.h"
#include "vv_kernels.h"

namespace vv {

constexpr int kLbTX = 16, kLbTY = 8, kLbTZ = 8;             // the tile (tests/test_label.py names it TILE)
constexpr int kLbTile = kLbTX * kLbTY * kLbTZ;             // 1024 voxels
constexpr int kLbThreads = 256, kLbVpt = kLbTile / kLbThreads;
constexpr uint32_t kLbNone = 0xFFFFFFFFu;                  // LDS: a background voxel's parent
constexpr int kLbBlocksPerCU = 8;                          // the elementwise kernels: a CU's full complement of waves

struct LabelKernelArgs {
    LabelArgs A;
    uint32_t ntx, plane;            // tiles per row of tiles, per plane of tiles
    uint64_t tiles, voxels;
    int reach;                      // coordinates a neighbour may differ in: 1, 2 or 3 (connectivity 6, 18, 26)
};

__device__ __forceinline__ uint32_t lds_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t agent_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of local voxel x as far as it is known now (P[x] <= x; concurrent unions only lower parents)
__device__ __forceinline__ uint32_t lds_find(const uint32_t *P, uint32_t x)
{
    for (int trip = 0; trip < kLbTile; ++trip) {
        const uint32_t p = lds_load(P + x);
        if (p >= x) break;
        x = p;
    }
    return x;
}
__device__ __forceinline__ void lds_union(uint32_t *P, uint32_t a, uint32_t b)
{
    for (int trip = 0; trip < kLbTile; ++trip) {
        a = lds_find(P, a); b = lds_find(P, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(P + a, b);
        if (old >= a) return;                                  // a was a root and hangs below b now
        a = old;                                               // someone linked a first: its old parent and b remain to be joined
    }
}

// labels: 0 = background, p + 1 = parent p.  x: a foreground voxel.
__device__ __forceinline__ uint32_t global_find(const uint32_t *labels, uint32_t x)
{
    for (;;) {
        const uint32_t p = agent_load(labels + x) - 1u;
        if (p >= x) break;
        x = p;
    }
    return x;
}
__device__ __forceinline__ void global_union(uint32_t *labels, uint32_t a, uint32_t b)
{
    for (;;) {
        a = global_find(labels, a); b = global_find(labels, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(labels + a, b + 1u) - 1u;
        if (old >= a) return;
        a = old;
    }
}

// tile `tile` -> its origin in the box
__device__ __forceinline__ void tile_origin(const LabelKernelArgs &K, uint64_t tile, uint32_t &ox, uint32_t &oy, uint32_t &oz)
{
    const uint32_t tz = (uint32_t)(tile / K.plane), rem = (uint32_t)(tile - (uint64_t)tz * K.plane), ty = rem / K.ntx, tx = rem - ty * K.ntx;
    ox = tx * kLbTX; oy = ty * kLbTY; oz = tz * kLbTZ;
}
__device__ __forceinline__ void local_coords(uint32_t l, uint32_t &lx, uint32_t &ly, uint32_t &lz)
{
    lx = l % kLbTX; ly = (l / kLbTX) % kLbTY; lz = l / (kLbTX * kLbTY);
}
__device__ __forceinline__ uint32_t box_index(const LabelArgs &A, uint32_t x, uint32_t y, uint32_t z)
{
    return (uint32_t)(((uint64_t)z * A.b[1] + y) * A.b[0] + x);          // (the box holds at most 2^32 - 2 voxels)
}
// offset (dx, dy, dz) of the backward half neighbourhood number o = 0..12: the 13 offsets whose local (and global) index is smaller
__device__ __forceinline__ void half_offset(int o, int &dx, int &dy, int &dz)
{
    dx = o % 3 - 1; dy = (o / 3) % 3 - 1; dz = o / 9 - 1;                 // o = 0..8: dz = -1; 9..11: dz = 0, dy = -1; 12: (-1, 0, 0)
}

template <int SRC>
__global__ __launch_bounds__(kLbThreads) void label_local_kernel(LabelKernelArgs K)
{
    constexpr bool F32 = SRC == VV_VOXEL_F32;
    constexpr int SIZE = F32 ? 4 : 1;
    __shared__ uint32_t P[kLbTile], cnt[kLbTile];
    const LabelArgs &A = K.A;
    for (uint64_t tile = blockIdx.x; tile < K.tiles; tile += gridDim.x) {
        uint32_t ox, oy, oz;
        tile_origin(K, tile, ox, oy, oz);
        bool in[kLbVpt], fg[kLbVpt];
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            const uint32_t l = threadIdx.x + k * kLbThreads;
            uint32_t lx, ly, lz;
            local_coords(l, lx, ly, lz);
            const uint32_t x = ox + lx, y = oy + ly, z = oz + lz;
            in[k] = x < A.b[0] && y < A.b[1] && z < A.b[2];
            fg[k] = false;
            if (in[k]) {
                const char *at = (const char *)A.src0 + ((uint64_t)z * A.slice_pitch + (uint64_t)y * A.row_pitch + (uint64_t)x * SIZE);
                uint32_t bin;
                if constexpr (F32) bin = index_of<VV_VOXEL_F32>(*(const float *)at); else bin = (uint32_t)*(const uint8_t *)at;
                fg[k] = bin >= A.bin_lo && bin <= A.bin_hi;
            }
            P[l] = fg[k] ? l : kLbNone;
            cnt[l] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            if (!fg[k]) continue;
            const uint32_t l = threadIdx.x + k * kLbThreads;
            uint32_t lx, ly, lz;
            local_coords(l, lx, ly, lz);
            for (int o = 0; o < 13; ++o) {
                int dx, dy, dz;
                half_offset(o, dx, dy, dz);
                if ((dx != 0) + (dy != 0) + (dz != 0) > K.reach) continue;
                const uint32_t mx = lx + dx, my = ly + dy, mz = lz + dz;       // (a coordinate below 0 wraps above the tile)
                if (mx >= kLbTX || my >= kLbTY || mz >= kLbTZ) continue;
                const uint32_t m = (mz * kLbTY + my) * kLbTX + mx;
                if (lds_load(P + m) != kLbNone) lds_union(P, l, m);           // (a tile voxel outside the box is background)
            }
        }
        __syncthreads();
        uint32_t root[kLbVpt];
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            root[k] = 0;
            if (!fg[k]) continue;
            root[k] = lds_find(P, threadIdx.x + k * kLbThreads);               // (no union runs any more: the root is final)
            if (A.sizes) atomicAdd(cnt + root[k], 1u);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            if (!in[k]) continue;
            const uint32_t l = threadIdx.x + k * kLbThreads;
            uint32_t lx, ly, lz, rx, ry, rz;
            local_coords(l, lx, ly, lz);
            local_coords(root[k], rx, ry, rz);
            const uint32_t i = box_index(A, ox + lx, oy + ly, oz + lz);
            A.labels[i] = fg[k] ? box_index(A, ox + rx, oy + ry, oz + rz) + 1u : 0u;
            if (A.sizes) A.sizes[i] = cnt[l];
        }
        __syncthreads();                                                       // (the next tile reuses P and cnt)
    }
}

__global__ __launch_bounds__(kLbThreads) void label_merge_kernel(LabelKernelArgs K)
{
    const LabelArgs &A = K.A;
    for (uint64_t tile = blockIdx.x; tile < K.tiles; tile += gridDim.x) {
        uint32_t ox, oy, oz;
        tile_origin(K, tile, ox, oy, oz);
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            const uint32_t l = threadIdx.x + k * kLbThreads;
            uint32_t lx, ly, lz;
            local_coords(l, lx, ly, lz);
            // a backward neighbour lies in another tile only for voxels on these five faces (no backward offset has dz = +1)
            if (!(lx == 0 || lx == kLbTX - 1 || ly == 0 || ly == kLbTY - 1 || lz == 0)) continue;
            const uint32_t x = ox + lx, y = oy + ly, z = oz + lz;
            if (x >= A.b[0] || y >= A.b[1] || z >= A.b[2]) continue;
            const uint32_t i = box_index(A, x, y, z);
            if (agent_load(A.labels + i) == 0) continue;
            for (int o = 0; o < 13; ++o) {
                int dx, dy, dz;
                half_offset(o, dx, dy, dz);
                if ((dx != 0) + (dy != 0) + (dz != 0) > K.reach) continue;
                const uint32_t mx = lx + dx, my = ly + dy, mz = lz + dz;
                if (mx < kLbTX && my < kLbTY && mz < kLbTZ) continue;          // the same tile: joined in LDS
                const uint32_t nx = x + dx, ny = y + dy, nz = z + dz;          // (below 0 wraps above the box)
                if (nx >= A.b[0] || ny >= A.b[1] || nz >= A.b[2]) continue;   // voxels outside the box do not exist
                const uint32_t n = box_index(A, nx, ny, nz);
                if (agent_load(A.labels + n) == 0) continue;
                global_union(A.labels, i, n);
            }
        }
    }
}

// sums a and b over the block and adds them to the two counters (all threads call it)
__device__ __forceinline__ void block_add2(uint32_t a, uint32_t b, unsigned long long *ca, unsigned long long *cb)
{
    __shared__ uint32_t ra[kLbThreads], rb[kLbThreads];
    ra[threadIdx.x] = a; rb[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sa = 0, sb = 0;
        for (int t = 0; t < kLbThreads; ++t) { sa += ra[t]; sb += rb[t]; }
        if (sa) atomicAdd(ca, sa);
        if (sb) atomicAdd(cb, sb);
    }
}

__global__ __launch_bounds__(kLbThreads) void label_flatten_kernel(LabelKernelArgs K)
{
    // state: 0 = background or outside the box; 1 = resolved, Q holds the root's index; 2 = unresolved, Q holds the parent's local index (below the voxel's own)
    __shared__ uint32_t Q[kLbTile];
    __shared__ uint8_t state[kLbTile];
    const LabelArgs &A = K.A;
    uint32_t n_fg = 0, n_roots = 0;                                            // (a thread meets at most 2^32 / 256 voxels)
    for (uint64_t tile = blockIdx.x; tile < K.tiles; tile += gridDim.x) {
        uint32_t ox, oy, oz;
        tile_origin(K, tile, ox, oy, oz);
        uint32_t idx[kLbVpt];
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            const uint32_t l = threadIdx.x + k * kLbThreads;
            uint32_t lx, ly, lz;
            local_coords(l, lx, ly, lz);
            const uint32_t x = ox + lx, y = oy + ly, z = oz + lz;
            idx[k] = kLbNone;
            uint8_t s = 0;
            uint32_t q = 0;
            if (x < A.b[0] && y < A.b[1] && z < A.b[2]) {
                const uint32_t i = box_index(A, x, y, z);
                const uint32_t v = agent_load(A.labels + i);
                if (v != 0) {
                    idx[k] = i;
                    const uint32_t p = v - 1u;
                    const uint32_t px = p % A.b[0], pq = p / A.b[0], py = pq % A.b[1], pz = pq / A.b[1];
                    const uint32_t mx = px - ox, my = py - oy, mz = pz - oz;
                    if (p < i && mx < kLbTX && my < kLbTY && mz < kLbTZ) { s = 2; q = (mz * kLbTY + my) * kLbTX + mx; }
                    else { s = 1; q = global_find(A.labels, p <= i ? p : i); }
                }
            }
            Q[l] = q; state[l] = s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLbVpt; ++k) {
            if (idx[k] == kLbNone) continue;
            uint32_t m = threadIdx.x + k * kLbThreads;
            for (int trip = 0; trip < kLbTile && state[m] == 2; ++trip) m = Q[m];
            const uint32_t i = idx[k], r = state[m] == 1 ? Q[m] : i;
            A.labels[i] = r + 1u;
            ++n_fg;
            if (r == i) ++n_roots;
            else if (A.sizes) {
                const uint32_t c = A.sizes[i];                                // nonzero at a former tile root: the count of its tile component
                if (c) { A.sizes[i] = 0; atomicAdd(A.sizes + r, c); }
            }
        }
        __syncthreads();                                                       // (the next tile reuses Q and state)
    }
    block_add2(n_fg, n_roots, A.counters + kLabelForeground, A.counters + kLabelComponents);
}

// key of the component at i: size << 32 | (0xFFFFFFFF - label): the largest key is the largest size and, among equals, the smallest label
__global__ __launch_bounds__(kLbThreads) void label_stats_kernel(const uint32_t *sizes, uint64_t voxels, unsigned long long *counters)
{
    __shared__ unsigned long long red[kLbThreads];
    unsigned long long best = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x; i < voxels; i += (uint64_t)gridDim.x * kLbThreads) {
        const uint32_t s = sizes[i];
        if (s) {
            const unsigned long long key = ((unsigned long long)s << 32) | (unsigned long long)(0xFFFFFFFFu - ((uint32_t)i + 1u));
            best = key > best ? key : best;
        }
    }
    red[threadIdx.x] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < kLbThreads; ++t) best = red[t] > best ? red[t] : best;
        if (best) atomicMax(counters + kLabelLargest, best);
    }
}

__global__ void label_stats_finish_kernel(const unsigned long long *counters, int with_sizes, vv_label_stats *out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long key = with_sizes ? counters[kLabelLargest] : 0ull;
    vv_label_stats s;
    s.foreground = counters[kLabelForeground];
    s.components = counters[kLabelComponents];
    s.largest_size = key >> 32;
    s.largest_label = key ? 0xFFFFFFFFu - (uint32_t)key : 0u;
    s.reserved = 0;
    *out = s;
}

static unsigned label_grid(uint64_t items, int max_blocks)
{
    uint64_t grid = items ? items : 1;
    if (max_blocks > 0 && grid > (uint64_t)max_blocks) grid = (uint64_t)max_blocks;
    if (grid > 0x7FFFFFFFull) grid = 0x7FFFFFFFull;
    return (unsigned)grid;
}
// the grid of an elementwise kernel over `items` threads' worth of work
static unsigned label_flat_grid(uint64_t items, int n_cu, int max_blocks)
{
    const uint64_t blocks = (items + kLbThreads - 1) / kLbThreads, cap = (uint64_t)(n_cu > 0 ? n_cu : 256) * kLbBlocksPerCU;
    return label_grid(blocks < cap ? blocks : cap, max_blocks);
}

void launch_label(const LabelArgs &a, int n_cu, int max_blocks, int phases, hipStream_t s)
{
    LabelKernelArgs k;
    k.A = a;
    k.ntx = (a.b[0] + kLbTX - 1) / kLbTX;
    k.plane = k.ntx * ((a.b[1] + kLbTY - 1) / kLbTY);
    k.tiles = (uint64_t)k.plane * ((a.b[2] + kLbTZ - 1) / kLbTZ);
    k.voxels = (uint64_t)a.b[0] * a.b[1] * a.b[2];
    k.reach = a.connectivity == 6 ? 1 : a.connectivity == 18 ? 2 : 3;
    const dim3 grid(label_grid(k.tiles, max_blocks)), block(kLbThreads);
    if (a.src_type == VV_VOXEL_F32) hipLaunchKernelGGL(label_local_kernel<VV_VOXEL_F32>, grid, block, 0, s, k);
    else                            hipLaunchKernelGGL(label_local_kernel<VV_VOXEL_U8>, grid, block, 0, s, k);
    if (phases == 1) return;
    hipLaunchKernelGGL(label_merge_kernel, grid, block, 0, s, k);
    if (phases == 2) return;
    hipLaunchKernelGGL(label_flatten_kernel, grid, block, 0, s, k);
    if (phases == 3) return;
    if (a.stats) {
        if (a.sizes) hipLaunchKernelGGL(label_stats_kernel, dim3(label_flat_grid(k.voxels, n_cu, max_blocks)), block, 0, s, (const uint32_t *)a.sizes, k.voxels, a.counters);
        hipLaunchKernelGGL(label_stats_finish_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long *)a.counters, a.sizes ? 1 : 0, a.stats);
    }
}

// ---- vv_mask_volume ----------------------------------------------------------------------------------------------------------------------------
// Work.  A row of the box is cut into chunks of four voxels consecutive in x; a thread takes a chunk (grid-stride over rows x chunks).  The four
// labels are one 16-byte load where they are aligned, the four source bytes of a u8 volume one dword likewise; whole aligned chunks are stored at
// once, the row's tail and unaligned starts voxel by voxel.  Every output voxel has one writer.
template <int SRC, int OUT>
__global__ __launch_bounds__(kLbThreads) void mask_kernel(MaskArgs M, uint32_t cpr, uint64_t items)
{
#pragma clang fp contract(off)
    constexpr bool F32 = SRC == VV_VOXEL_F32, OF32 = OUT == VV_VOXEL_F32;
    constexpr int SIZE = F32 ? 4 : 1, OSIZE = OF32 ? 4 : 1;
    const uint32_t fill_out = voxel_out<F32, OF32>(M.fill);
    const uint64_t voxels = (uint64_t)M.b[0] * M.b[1] * M.b[2];
    for (uint64_t it = (uint64_t)blockIdx.x * kLbThreads + threadIdx.x; it < items; it += (uint64_t)gridDim.x * kLbThreads) {
        const uint64_t row = it / cpr;
        const uint32_t x0 = (uint32_t)(it - row * cpr) * 4u, y = (uint32_t)(row % M.b[1]), z = (uint32_t)(row / M.b[1]);
        const uint32_t n = min(4u, M.b[0] - x0);
        const uint64_t i0 = row * M.b[0] + x0;
        const char *src = (const char *)M.src0 + ((uint64_t)z * M.slice_pitch + (uint64_t)y * M.row_pitch + (uint64_t)x0 * SIZE);
        const uint32_t *lp = M.labels + i0;
        uint32_t lab[4] = {0, 0, 0, 0}, raw[4] = {0, 0, 0, 0}, v[4];
        if (n == 4 && ((uintptr_t)lp & 15) == 0) {
            const uint4 q = *(const uint4 *)lp;
            lab[0] = q.x; lab[1] = q.y; lab[2] = q.z; lab[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)k < n) lab[k] = lp[k];
        }
        if (!F32 && n == 4 && ((uintptr_t)src & 3) == 0) {
            const uint32_t w = *(const uint32_t *)src;
#pragma unroll
            for (int k = 0; k < 4; ++k) raw[k] = (w >> (8 * k)) & 255u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)k < n) { if constexpr (F32) raw[k] = *(const uint32_t *)(src + k * 4); else raw[k] = (uint32_t)*(const uint8_t *)(src + k); }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool test;
            if (M.keep == VV_KEEP_LABEL) test = lab[k] == M.label;
            else if (M.keep == VV_KEEP_FOREGROUND) test = lab[k] != 0;
            else {
                test = false;
                if ((uint32_t)k < n && lab[k] != 0 && (uint64_t)(lab[k] - 1u) < voxels) test = M.sizes[lab[k] - 1u] >= M.min_size;   // the bound check is the contract's
            }
            v[k] = test != (M.invert != 0) ? voxel_out_copy<F32, OF32>(raw[k]) : fill_out;
        }
        char *at = (char *)M.out + i0 * OSIZE;
        if (n == 4 && ((uintptr_t)at & (uintptr_t)(4 * OSIZE - 1)) == 0) {
            if constexpr (OF32) *(uint4 *)at = make_uint4(v[0], v[1], v[2], v[3]);
            else *(uint32_t *)at = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((uint32_t)k < n) voxel_store<OF32>(at + k * OSIZE, v[k]);
        }
    }
}

void launch_mask(const MaskArgs &m, int n_cu, int max_blocks, hipStream_t s)
{
    const uint32_t cpr = (m.b[0] + 3) / 4;
    const uint64_t items = (uint64_t)cpr * m.b[1] * m.b[2];
    const dim3 grid(label_flat_grid(items, n_cu, max_blocks)), block(kLbThreads);
    const bool sf = m.src_type == VV_VOXEL_F32, of = m.out_type == VV_VOXEL_F32;
    if (sf && of)       hipLaunchKernelGGL((mask_kernel<VV_VOXEL_F32, VV_VOXEL_F32>), grid, block, 0, s, m, cpr, items);
    else if (sf)        hipLaunchKernelGGL((mask_kernel<VV_VOXEL_F32, VV_VOXEL_U8>), grid, block, 0, s, m, cpr, items);
    else if (of)        hipLaunchKernelGGL((mask_kernel<VV_VOXEL_U8, VV_VOXEL_F32>), grid, block, 0, s, m, cpr, items);
    else                hipLaunchKernelGGL((mask_kernel<VV_VOXEL_U8, VV_VOXEL_U8>), grid, block, 0, s, m, cpr, items);
}

} // namespace vv
