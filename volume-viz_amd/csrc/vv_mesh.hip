// vv_mesh.hip -- surface meshes for gfx950: the naive surface-nets mesh of a level of the loaded volume or of a segmentation, ranked device-wide into an
// indexed list of vertices and quads (no reference counterpart; the contract is the comment on vv_surface_mesh in include/volviz.h).
//
//   mesh_count_kernel        launch 1: the active sites and the emitting edges of every chunk counted (ballots + popcounts), one partial per chunk
//   mesh_scan_kernel         launch 2: one block turns the partials into exclusive offsets, writes V and Q and the summary
//   mesh_vertices_kernel     launch 3: every site gets its index word; an active site of rank < max_vertices its vertex (and normal) record
//   mesh_quads_kernel        launch 4: every emitting owned edge of rank < max_quads gets its quad record from four index words
//
// Representation.  j numbers the sites of the m_x x m_y x m_z grid, x fastest (rule 2); site s is the cell of the box voxels s - cap + {0, 1}^3.  A corner
// value is g (rule 1) of a real voxel and 0 of a virtual one: the address of a virtual voxel is clamped into the box and the loaded value replaced
// by a select, so no load ever leaves the box.  Lanes hold consecutive j: a lane loads its four corners at x offset 0 (the rows (y, z), (y + 1, z),
// (y, z + 1), (y + 1, z + 1): coalesced) and takes the four at offset 1 from the next lane, whose offset-0 corners they are; only the last site of a row
// of sites and the last lane of a step load them themselves.  A row of sites may end anywhere inside a step: every lane carries its own (s_x, s_y, s_z).
//
// Chunks (as vv_region.hip).  The sites are cut into `nchunks` runs of chunk_len = max(kMeshMinChunk, ceil(sites / cap)) sites, rounded up to the wave
// size; cap is kMeshMaxChunks, or VV_MESH_CHUNKS where that is lower.  A chunk is walked by ONE wave, 64 consecutive sites a step, front to back: what
// it has met so far is a wave-uniform number, so a rank is the chunk's offset + that number + the ballot's prefix, with no barrier.  A block of kMsWaves
// waves takes kMsWaves consecutive chunks; VV_MESH_BLOCKS caps every grid, the loop then takes blockIdx.x, + gridDim.x, ...  A wave can issue the loads
// of kMsAhead steps before it works on the first of them; with 4 the count launch took 10.3 ms at 1024^3 against 7.4 ms with 1 (74 VGPRs, six waves per
// SIMD): the walk is bound by the instructions per site, not by the latency of a step's loads (profiles/mesh_c3.txt).
//
// Phases.  Launch boundaries are the only synchronisation between blocks: no kernel waits for another block or wave, there is no spin, no look-back, no
// grid barrier, no cooperative launch and no atomic; the launches are four for any data, two for a count-only call (VV_MESH_PHASES cuts them short for
// timing).  No host read-back.  Launches 3 and 4 derive the corner values from the volume again: nothing is parked in `index` between launches.
//
// Ownership of every word, and why each cross-block read is safe:
//  the volume, labels         read-only in every launch: a plain load sees what the caller put there, whatever block reads it.
//  partials[c]                written by the wave of chunk c in launch 1; read and rewritten (as offsets) by the one block of launch 2; read by the wave of
//                             chunk c in launches 3 and 4.  hdr (V, Q) and the summary: written by the last thread of launch 2, read by nobody here.
//  index[j]                   written in launch 3 by j's own lane, every word of it, and in no other launch; launch 4 only reads it (the site's own word
//                             and those of three neighbour sites, which other blocks wrote): every word it reads was completed by launch 3.
//  vertices, normals [rank]   written in launch 3 by the one lane that holds that rank; quads [rank] in launch 4 likewise.  Read by nobody.
// Addresses.  index[j] only behind j < sites; a neighbour site only behind s_b + 1 < m_b and s_c + 1 < m_c; a record only behind rank < max_vertices /
// max_quads, rank formed from the partials and the ballots.  No loaded word is ever an address: a vertex number read from `index` is stored, not followed.
//
// Termination.  Every loop is counted (chunks, steps, edges, scan strides).
// No scalar-memory stores, no inline assembly, no xnack.
#include "vv_device.h"
#include "vv_kernels.h"
#include <algorithm>

namespace vv {

constexpr int kMsWaves = 4, kMsThreads = 64 * kMsWaves;
constexpr int kMsAhead = 1;                                 // steps of a chunk whose loads are issued together: 4 was slower (profiles/mesh_c3.txt, part 2)
constexpr int kMsScanThreads = 1024, kMsScanPer = kMeshMaxChunks / kMsScanThreads;
static_assert(kMeshMaxChunks % kMsScanThreads == 0, "the scan block takes a whole number of partials per thread");
static_assert(sizeof(MeshPartial) == 16 && sizeof(vv_mesh_vertex) == 16 && sizeof(vv_mesh_normal) == 16, "16-byte records: one store each");
enum { MS_U8 = 0, MS_F32 = 1, MS_LABELS = 2 };              // what a corner is loaded from

struct MeshKernelArgs {
    MeshArgs A;
    uint64_t sites, chunk_len;
    uint32_t nchunks;
};

// g of the real voxel x of a row (rule 1).  row: the row's byte offset from src0, or (labels) the index of its first word
template <int SRC>
__device__ __forceinline__ uint32_t mesh_g(const MeshArgs &A, uint64_t row, uint32_t x)
{
    if constexpr (SRC == MS_LABELS) {
        const uint32_t w = A.labels[row + x];
        return A.source == VV_MESH_LABEL ? (uint32_t)(w == A.label) : (uint32_t)(w != 0u);
    } else {
        uint32_t bin;
        if constexpr (SRC == MS_F32) bin = index_of<VV_VOXEL_F32>(*(const float *)((const char *)A.src0 + row + 4ull * x));
        else bin = (uint32_t)*((const uint8_t *)A.src0 + row + x);
        return A.source == VV_MESH_BINS ? (uint32_t)(A.bin_lo <= bin && bin <= A.bin_hi) : bin;
    }
}

// a box coordinate that may be virtual (-1 or b): whether it is real, and clamped into 0..b-1
__device__ __forceinline__ uint32_t mesh_clamp(int32_t v, uint32_t b, bool &real)
{
    real = (uint32_t)v < b;
    return v < 0 ? 0u : min((uint32_t)v, b - 1u);
}

// What a lane loads of its site s: the four corner values at x offset 0 (v0[dy + 2 dz]) and, where the lane cannot take them from the next lane (the site
// ends its row of sites, or the lane ends the step: `own`), the four at offset 1.  `in`: the lane has a site.  The loads of kMsAhead steps are issued
// before the first of them is used.
struct MeshFetch { uint32_t v0[4], v1[4]; bool own; };
template <int SRC>
__device__ __forceinline__ void mesh_fetch(const MeshArgs &A, bool in, uint32_t lane, const uint32_t s[3], MeshFetch &f)
{
    bool rx0, rx1;
    const int32_t x0 = (int32_t)s[0] - A.cap;
    const uint32_t cx0 = mesh_clamp(x0, A.b[0], rx0), cx1 = mesh_clamp(x0 + 1, A.b[0], rx1);
    f.own = in && (lane == 63u || s[0] + 1u == A.m[0]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bool ry, rz;
        const uint32_t cy = mesh_clamp((int32_t)s[1] - A.cap + (r & 1), A.b[1], ry), cz = mesh_clamp((int32_t)s[2] - A.cap + (r >> 1), A.b[2], rz);
        const uint64_t row = SRC == MS_LABELS ? ((uint64_t)cz * A.b[1] + cy) * A.b[0] : (uint64_t)cz * A.slice_pitch + (uint64_t)cy * A.row_pitch;
        f.v0[r] = 0; f.v1[r] = 0;
        if (in) { const uint32_t v = mesh_g<SRC>(A, row, cx0); f.v0[r] = rx0 && ry && rz ? v : 0u; }
        if (f.own) { const uint32_t v = mesh_g<SRC>(A, row, cx1); f.v1[r] = rx1 && ry && rz ? v : 0u; }
    }
}
// The eight corner values of the lane's site, g[dx + 2 dy + 4 dz].  Called by all lanes of the wave together (the x + 1 corners of a lane are the next
// lane's x corners unless it loaded them itself).
__device__ __forceinline__ void mesh_corners(const MeshFetch &f, uint32_t g[8])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t next = __shfl_down(f.v0[r], 1);
        g[2 * r] = f.v0[r]; g[2 * r + 1] = f.own ? f.v1[r] : next;
    }
}

// what the corners say of a site: the 8-bit mask of the corners inside, and the 3-bit mask of the owned edges (axis a: the edge along a that ends at
// corner (1, 1, 1)) that emit a quad (rule 6)
__device__ __forceinline__ uint32_t mesh_inside(const MeshArgs &A, const uint32_t g[8])
{
    uint32_t in8 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) in8 |= (uint32_t)(g[k] >= A.level) << k;
    return in8;
}
__device__ __forceinline__ uint32_t mesh_emit(const MeshArgs &A, bool in, uint32_t in8, const uint32_t s[3])
{
    uint32_t emit = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const bool act = (((in8 >> (7 ^ (1 << a))) ^ (in8 >> 7)) & 1u) != 0u;
        emit |= (uint32_t)(in && act && s[b] + 1u < A.m[b] && s[c] + 1u < A.m[c]) << a;
    }
    return emit;
}

// the lane's site as a chunk is walked: set at the chunk's first step, moved on by 64 sites a step (a division only where a row of sites ends)
__device__ __forceinline__ void mesh_walk_begin(const MeshArgs &A, uint64_t j, uint32_t s[3])
{
    const uint64_t q = j / A.m[0];
    s[0] = (uint32_t)(j - q * A.m[0]); s[1] = (uint32_t)(q % A.m[1]); s[2] = (uint32_t)(q / A.m[1]);
}
__device__ __forceinline__ void mesh_walk_step(const MeshArgs &A, uint32_t s[3])
{
    s[0] += 64u;
    if (A.m[0] >= 64u) {                                                      // (wave-uniform) a step ends at most one row of sites
        const bool wrap = s[0] >= A.m[0];
        s[0] -= wrap ? A.m[0] : 0u; s[1] += wrap ? 1u : 0u;
        const bool wrap2 = s[1] >= A.m[1];
        s[1] -= wrap2 ? A.m[1] : 0u; s[2] += wrap2 ? 1u : 0u;
    } else if (s[0] >= A.m[0]) {
        const uint32_t q = s[0] / A.m[0];
        s[0] -= q * A.m[0]; s[1] += q;
        if (s[1] >= A.m[1]) { const uint32_t q2 = s[1] / A.m[1]; s[1] -= q2 * A.m[1]; s[2] += q2; }
    }
}
// the fetches of the next kMsAhead steps of a chunk, from step i0 on: the lane's sites st[u], whether it has one (in[u]), what it loaded (f[u]); s moves on
template <int SRC>
__device__ __forceinline__ void mesh_fetch_ahead(const MeshArgs &A, uint64_t i0, uint64_t end, uint32_t lane, uint32_t s[3], uint32_t st[][3], bool in[], MeshFetch f[])
{
#pragma unroll
    for (int u = 0; u < kMsAhead; ++u) {
        st[u][0] = s[0]; st[u][1] = s[1]; st[u][2] = s[2];
        in[u] = i0 + 64ull * u + lane < end;
        mesh_fetch<SRC>(A, in[u], lane, s, f[u]);
        mesh_walk_step(A, s);
    }
}

template <int SRC>
__global__ __launch_bounds__(kMsThreads) void mesh_count_kernel(MeshKernelArgs K)
{
    const MeshArgs &A = K.A;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk * kMsWaves < K.nchunks; blk += gridDim.x) {
        const uint32_t chunk = blk * kMsWaves + wave;
        if (chunk >= K.nchunks) continue;
        const uint64_t begin = (uint64_t)chunk * K.chunk_len, end = min(begin + K.chunk_len, K.sites);
        uint32_t s[3];
        mesh_walk_begin(A, begin + lane, s);
        unsigned long long nv = 0, nq = 0;                                    // wave-uniform
        for (uint64_t i0 = begin; i0 < end; i0 += 64 * kMsAhead) {
            uint32_t st[kMsAhead][3];
            bool inu[kMsAhead];
            MeshFetch f[kMsAhead];
            mesh_fetch_ahead<SRC>(A, i0, end, lane, s, st, inu, f);
#pragma unroll
            for (int u = 0; u < kMsAhead; ++u) {                              // (a step behind the chunk's end holds no site: it counts nothing)
                const bool in = inu[u];
                uint32_t g[8];
                mesh_corners(f[u], g);
                const uint32_t in8 = mesh_inside(A, g), emit = mesh_emit(A, in, in8, st[u]);
                nv += (unsigned long long)__popcll(__ballot(in && in8 != 0u && in8 != 0xFFu));
#pragma unroll
                for (int a = 0; a < 3; ++a) nq += (unsigned long long)__popcll(__ballot((emit >> a) & 1u));
            }
        }
        if (lane == 0) { MeshPartial p; p.vertices = nv; p.quads = nq; A.partials[chunk] = p; }
    }
}

__global__ __launch_bounds__(kMsScanThreads) void mesh_scan_kernel(MeshKernelArgs K)
{
    __shared__ unsigned long long sv[kMsScanThreads], sq[kMsScanThreads];
    const MeshArgs &A = K.A;
    const uint32_t t = threadIdx.x;
    MeshPartial v[kMsScanPer];
    unsigned long long sumv = 0, sumq = 0;
#pragma unroll
    for (int k = 0; k < kMsScanPer; ++k) {
        const uint32_t idx = t * kMsScanPer + k;
        if (idx < K.nchunks) v[k] = A.partials[idx]; else { v[k].vertices = 0; v[k].quads = 0; }
        sumv += v[k].vertices; sumq += v[k].quads;                            // (at most the sites and three times the sites: below 2^34)
    }
    sv[t] = sumv; sq[t] = sumq;
    __syncthreads();
    for (uint32_t off = 1; off < kMsScanThreads; off <<= 1) {
        const unsigned long long xv = t >= off ? sv[t - off] : 0ull, xq = t >= off ? sq[t - off] : 0ull;
        __syncthreads();
        sv[t] += xv; sq[t] += xq;
        __syncthreads();
    }
    MeshPartial excl;
    excl.vertices = sv[t] - sumv; excl.quads = sq[t] - sumq;
#pragma unroll
    for (int k = 0; k < kMsScanPer; ++k) {
        const uint32_t idx = t * kMsScanPer + k;
        if (idx < K.nchunks) A.partials[idx] = excl;
        excl.vertices += v[k].vertices; excl.quads += v[k].quads;
    }
    if (t == kMsScanThreads - 1) {
        A.hdr[kMeshVertices] = sv[t]; A.hdr[kMeshQuads] = sq[t];
        if (A.summary) {
            vv_mesh_summary r;
            r.vertices = sv[t]; r.quads = sq[t];
            r.written_vertices = min(sv[t], (unsigned long long)A.max_vertices); r.written_quads = min(sq[t], (unsigned long long)A.max_quads);
            *A.summary = r;
        }
    }
}

// the vertex and normal records of an active site (rules 3 and 4): no multiplication anywhere, one division per crossing and one per coordinate
__device__ __forceinline__ void mesh_vertex(const MeshArgs &A, const uint32_t g[8], uint32_t in8, const uint32_t s[3], uint32_t j, uint32_t rank)
{
    float S[3] = {0.0f, 0.0f, 0.0f};
    uint32_t n = 0, mask = 0;
    const int32_t level = (int32_t)A.level;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int a = e >> 2, db = e & 1, dc = (e >> 1) & 1, b = (a + 1) % 3, c = (a + 2) % 3;
        const int p = (db << b) | (dc << c), q = p | (1 << a);
        if ((((in8 >> p) ^ (in8 >> q)) & 1u) != 0u) {
            const int32_t gp = (int32_t)g[p], gq = (int32_t)g[q];
            S[a] += (float)(2 * level - 1 - 2 * gp) / (float)(2 * (gq - gp));
            if (db) S[b] += 1.0f;                                             // (an offset of 0.0f leaves the sum as it is)
            if (dc) S[c] += 1.0f;
            ++n; mask |= 1u << e;
        }
    }
    const float fn = (float)n;
    uint4 rec;
    rec.x = __float_as_uint((float)(A.lo[0] + (int32_t)s[0] - A.cap) + S[0] / fn);
    rec.y = __float_as_uint((float)(A.lo[1] + (int32_t)s[1] - A.cap) + S[1] / fn);
    rec.z = __float_as_uint((float)(A.lo[2] + (int32_t)s[2] - A.cap) + S[2] / fn);
    rec.w = j;
    *(uint4 *)(A.vertices + rank) = rec;
    if (A.normals) {
        int32_t d[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) d[ax] += ((k >> ax) & 1) ? -(int32_t)g[k] : (int32_t)g[k];
        uint4 nr;
        nr.x = (uint32_t)d[0]; nr.y = (uint32_t)d[1]; nr.z = (uint32_t)d[2]; nr.w = mask;
        *(uint4 *)(A.normals + rank) = nr;
    }
}

template <int SRC>
__global__ __launch_bounds__(kMsThreads) void mesh_vertices_kernel(MeshKernelArgs K)
{
    const MeshArgs &A = K.A;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t blk = blockIdx.x; blk * kMsWaves < K.nchunks; blk += gridDim.x) {
        const uint32_t chunk = blk * kMsWaves + wave;
        if (chunk >= K.nchunks) continue;
        const uint64_t begin = (uint64_t)chunk * K.chunk_len, end = min(begin + K.chunk_len, K.sites);
        uint32_t s[3];
        mesh_walk_begin(A, begin + lane, s);
        uint32_t base = (uint32_t)A.partials[chunk].vertices;                 // active sites below this chunk, then below this step: wave-uniform (below 2^32)
        for (uint64_t i0 = begin; i0 < end; i0 += 64 * kMsAhead) {
            uint32_t st[kMsAhead][3];
            bool inu[kMsAhead];
            MeshFetch f[kMsAhead];
            mesh_fetch_ahead<SRC>(A, i0, end, lane, s, st, inu, f);
#pragma unroll
            for (int u = 0; u < kMsAhead; ++u) {
                const uint64_t j = i0 + 64ull * u + lane;
                const bool in = inu[u];
                uint32_t g[8];
                mesh_corners(f[u], g);
                const uint32_t in8 = mesh_inside(A, g);
                const bool active = in && in8 != 0u && in8 != 0xFFu;
                const unsigned long long m = __ballot(active);
                if (in) {
                    const uint32_t rank = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    A.index[j] = active ? rank + 1u : 0u;
                    if (active && rank < A.max_vertices) mesh_vertex(A, g, in8, st[u], (uint32_t)j, rank);
                }
                base += (uint32_t)__popcll(m);
            }
        }
    }
}

template <int SRC>
__global__ __launch_bounds__(kMsThreads) void mesh_quads_kernel(MeshKernelArgs K)
{
    const MeshArgs &A = K.A;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t stride[3] = {1ull, (uint64_t)A.m[0], (uint64_t)A.m[0] * A.m[1]};
    for (uint32_t blk = blockIdx.x; blk * kMsWaves < K.nchunks; blk += gridDim.x) {
        const uint32_t chunk = blk * kMsWaves + wave;
        if (chunk >= K.nchunks) continue;
        const uint64_t begin = (uint64_t)chunk * K.chunk_len, end = min(begin + K.chunk_len, K.sites);
        uint32_t s[3];
        mesh_walk_begin(A, begin + lane, s);
        unsigned long long base = A.partials[chunk].quads;                    // quads below this chunk, then below this step: wave-uniform
        for (uint64_t i0 = begin; i0 < end; i0 += 64 * kMsAhead) {
            uint32_t st[kMsAhead][3];
            bool inu[kMsAhead];
            MeshFetch f[kMsAhead];
            mesh_fetch_ahead<SRC>(A, i0, end, lane, s, st, inu, f);
#pragma unroll
            for (int u = 0; u < kMsAhead; ++u) {
                const uint64_t j = i0 + 64ull * u + lane;
                uint32_t g[8];
                mesh_corners(f[u], g);
                const uint32_t in8 = mesh_inside(A, g), emit = mesh_emit(A, inu[u], in8, st[u]);
                const unsigned long long below = (1ull << lane) - 1ull;
                unsigned long long rank = base;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const unsigned long long m = __ballot((emit >> a) & 1u);
                    rank += (unsigned long long)__popcll(m & below);
                    base += (unsigned long long)__popcll(m);
                }
                if (emit && rank < A.max_quads) {
                    const uint32_t c0 = A.index[j] - 1u;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        if (!((emit >> a) & 1u)) continue;
                        if (rank < A.max_quads) {
                            const uint64_t sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];
                            const uint32_t c1 = A.index[j + sb] - 1u, c2 = A.index[j + sb + sc] - 1u, c3 = A.index[j + sc] - 1u;
                            const bool p_in = ((in8 >> (7 ^ (1 << a))) & 1u) != 0u;
                            uint4 rec;
                            rec.x = c0; rec.y = p_in ? c1 : c3; rec.z = c2; rec.w = p_in ? c3 : c1;
                            A.quads[rank] = rec;
                        }
                        ++rank;
                    }
                }
            }
        }
    }
}

template <int SRC>
static void launch_mesh_src(const MeshKernelArgs &k, uint32_t grid, int phases, hipStream_t s)
{
    const dim3 block(kMsThreads);
    hipLaunchKernelGGL(mesh_count_kernel<SRC>, dim3(grid), block, 0, s, k);
    if (phases == 1) return;
    hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kMsScanThreads), 0, s, k);
    if (phases == 2 || !k.A.index) return;
    hipLaunchKernelGGL(mesh_vertices_kernel<SRC>, dim3(grid), block, 0, s, k);
    if (phases == 3) return;
    hipLaunchKernelGGL(mesh_quads_kernel<SRC>, dim3(grid), block, 0, s, k);
}

void launch_mesh(const MeshArgs &a, int max_blocks, int max_chunks, int phases, hipStream_t s)
{
    MeshKernelArgs k;
    k.A = a;
    k.sites = (uint64_t)a.m[0] * a.m[1] * a.m[2];
    const uint64_t cap = max_chunks > 0 && max_chunks < kMeshMaxChunks ? (uint64_t)max_chunks : (uint64_t)kMeshMaxChunks;
    const uint64_t per = (k.sites + cap - 1) / cap, len = per > (uint64_t)kMeshMinChunk ? per : (uint64_t)kMeshMinChunk;
    k.chunk_len = (len + 63) / 64 * 64;
    k.nchunks = (uint32_t)((k.sites + k.chunk_len - 1) / k.chunk_len);        // at most cap: rounding chunk_len up only lowers it; 0 for an empty grid
    uint32_t grid = (k.nchunks + kMsWaves - 1) / kMsWaves;
    if (max_blocks > 0 && grid > (uint32_t)max_blocks) grid = (uint32_t)max_blocks;
    if (grid < 1) grid = 1;
    const bool labels = a.source == VV_MESH_LABEL || a.source == VV_MESH_NONZERO;
    if (labels)                          launch_mesh_src<MS_LABELS>(k, grid, phases, s);
    else if (a.src_type == VV_VOXEL_F32) launch_mesh_src<MS_F32>(k, grid, phases, s);
    else                                 launch_mesh_src<MS_U8>(k, grid, phases, s);
}

} // namespace vv
