// vv_mip.hip -- maximum-intensity projection kernels for gfx950 (MI355X).  No reference counterpart: the reference composites only.
//
// A MIP frame marches the rays of an unshaded vv_render frame -- same end points, same per-slab sphere radius (rad_kernel), same
// setup_ray with its cut plane, same 30-sample chunks, same (pos - .5) / scale + .5 mapping, same filter, same 8-bit classification
// index -- and keeps, per pixel, the largest index M over the samples it executes (0 when it executes none).  No table look-up, no
// blend, no early-termination state: the ray state and the U samples in flight live in registers, the per-sample work behind the
// trilinear reconstruction is one v_max_u32, and the transfer table is read once per pixel, in the epilogue.
//   * mip_kernel           the march: trip structure of march_kernel (vv_raymarch.hip), on the tile grid both share (vv_tiles.h: block order, wave tiles, launch size);
//   * fill_outside_kernel  the pixels beside the volume's screen rectangle, which the tiles of mip_kernel, iso_kernel and proj_kernel do not cover: no
//                          sample, so index 0, no hit, n = 0 (one kernel for the three kinds; linear build only);
//   * mip_classify_kernel  index image -> RGBA through a table (vv_classify_indices).
// Like vv_raymarch.hip this file is compiled once per volume layout (vv_layout.h; the Makefile passes the layout's macros); each unit defines
// launch_frame<FRAME_MIP, kBuild>.
#include "vv_device.h"
#include "vv_kernels.h"
#include "vv_layout.h"

namespace vv {
namespace VV_BIG_NS {

// channel c of an RGBA pixel = sat_u8(clamp(tf[M][c], 0, 1) * 255): pack_rgba's conversion of a table entry
__device__ __forceinline__ uint32_t classify_entry(const float4 e) { return pack_rgba(e.x, e.y, e.z, e.w); }

// blockDim = 256 = 4 waves; block -> (strip, tile) and wave -> pixels through vv_tiles.h, as in march_kernel.  `pixels` and `index`
// may each be null (vv_render_mip wants at least one).  Uninstrumented frames drop a ray once its maximum is 255 (nothing can raise
// it); instrumented frames march every ray to its end so that the count is the full executed count.
template <int VOXEL, bool TEX8, bool INSTR, int U>
__global__ __launch_bounds__(256) void mip_kernel(FrameParams P, VolumeView V,
                                                  const float4 *__restrict__ tf,
                                                  const float *__restrict__ rad,
                                                  uint32_t *__restrict__ pixels,
                                                  uint8_t *__restrict__ index,
                                                  unsigned long long *__restrict__ counter,
                                                  InstrArgs I, StripMap M)
{
    int strip, tile_x, x, y;
    if (!block_tile(M, blockIdx.x, strip, tile_x)) return;
    tile_pixel(M, strip, tile_x, threadIdx.x, x, y);
    if (strip >= M.s1) return;

    // pixels no frame writes: column W-1 / row H-1 (W,H >= 2), rows of other shards
    const int xmax = P.W >= 2 ? P.W - 2 : 0, ymax = P.H >= 2 ? P.H - 2 : 0;
    const bool in_frame = x <= xmax && y <= ymax && row_owned(P, y);

    uint32_t m = 0;
    unsigned long long executed = 0, slots = 0;

    Ray r;
    int alive = 0;
    if (in_frame) {
        f3 front, back;
        ray_endpoints(P, x, y, front, back);
        float length = vlen3(back.x - front.x, back.y - front.y, back.z - front.z);
        if (!(length < 0.001f)) {                                    // (a zero-length ray executes nothing: M = 0)
            float rd;
            if (P.W < 2 || P.H < 2) {
                rd = vlen3(front.x - P.cam_pos[0], front.y - P.cam_pos[1], front.z - P.cam_pos[2]);
            } else {
                int ox = owner_slab(x, P.W, P.nbx, P.conflict_x), oy = owner_slab(y, P.H, P.nby, P.conflict_y);
                rd = rad[oy * P.nbx + ox];
            }
            setup_ray(P, front, back, rd, r);
            alive = r.cut_return ? 0 : 1;
        }
    }
    if (!alive) { r.upper = -1.f; r.dist0 = 0.f; r.sstep = 1.f; r.origin = mk3(0, 0, 0); r.dir = r.origin; r.sdir = r.origin; }

    float dist = r.dist0;
    for (int chunk = 0; chunk < P.max_chunks && __any(dist < r.upper); ++chunk) {
        const int n = chunk_count(dist, r.upper, r.sstep);
        float px, py, pz;
        {
#pragma clang fp contract(off)
            px = r.origin.x + r.dir.x * dist;
            py = r.origin.y + r.dir.y * dist;
            pz = r.origin.z + r.dir.z * dist;
        }
        // wave-uniform trip count (5 ballots: n <= 30); lanes with fewer samples are predicated, not branched
        int nmax = 0;
#pragma unroll
        for (int bit = 16; bit > 0; bit >>= 1)
            if (__any(n >= (nmax | bit))) nmax |= bit;
        if (INSTR) slots += (unsigned long long)((nmax + U - 1) / U * U) * 64ull;
        for (int i0 = 1; i0 <= nmax; i0 += U) {
            float tx[U], ty[U], tz[U];
            typename CornerSel<VOXEL>::type C[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                px += r.sdir.x; py += r.sdir.y; pz += r.sdir.z;
                tx[u] = __builtin_fmaf(px - 0.5f, P.inv_scale[0], 0.5f);
                ty[u] = __builtin_fmaf(py - 0.5f, P.inv_scale[1], 0.5f);
                tz[u] = __builtin_fmaf(pz - 0.5f, P.inv_scale[2], 0.5f);
                fetch_any<VOXEL, TEX8>(V, tx[u], ty[u], tz[u], C[u]);
            }
            __builtin_amdgcn_sched_barrier(0);           // all gathers of the trip are issued before the first is consumed
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = i0 + u <= n;
                const uint32_t k = classify_index<VOXEL>(C[u], tx[u], ty[u], tz[u]);
                m = max(m, live ? k : 0u);
                if (INSTR) instrument_sample<VOXEL, TEX8>(I, V, tx[u], ty[u], tz[u], live, executed);
            }
        }
        if (!INSTR && m == 255u) r.upper = -1.f;
        {
#pragma clang fp contract(off)
            dist += r.sstep * kChunkSteps;
        }
    }

    if (in_frame) {
        const size_t p = (size_t)y * P.W + x;
        if (index) index[p] = (uint8_t)m;
        if (pixels) pixels[p] = classify_entry(tf[m]);
    }
    if (INSTR) flush_counters(counter, executed, slots);
}

static void launch_mip_impl(const MarchArgs &a, hipStream_t s)
{
    const unsigned nblocks = grid_blocks(a.strips);
    if (!nblocks) return;
    for_variant(a, [&](auto VOXEL, auto TEX8, auto INSTR, auto U) {
        hipLaunchKernelGGL((mip_kernel<VOXEL(), TEX8(), INSTR(), U()>), dim3(nblocks), dim3(256), reducer_lds(a), s,
                           a.P, a.V, a.tf, a.rad, a.pixels, a.index, a.counter, a.I, a.strips);
    });
}

#ifdef VV_BUILD_LINEAR       // (once: the build for the linear layout)
// The owned pixels outside the rectangle that the tiles of a MIP, isosurface or projection frame cover: their rays miss the volume (vv_render: screen_rect),
// so they execute no sample -- index 0, the RGBA of the table's entry 0 (MIP and projection frames; `tf` null: 0, the isosurface frame's "no hit") and
// all-zero records, each written in one store: `stat` the projection frame's {0, 0}, `hit` the isosurface frame's (0, 0, 0, 0).  Every image may be null.
// One thread per pixel of the frame; threads inside the rectangle, in column W-1 / row H-1 or in another shard's rows leave at once.
__global__ __launch_bounds__(256) void fill_outside_kernel(FrameParams P, PixelRect R, const float4 *__restrict__ tf, uint32_t *__restrict__ pixels,
                                                           uint8_t *__restrict__ index, uint2 *__restrict__ stat, float4 *__restrict__ hit)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x > P.W - 2 || y > P.H - 2 || !row_owned(P, y)) return;
    if (x >= R.x0 && x < R.x1 && y >= R.y0 && y < R.y1) return;
    const size_t p = (size_t)y * P.W + x;
    if (index) index[p] = 0;
    if (stat) stat[p] = make_uint2(0u, 0u);
    if (hit) hit[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pixels) pixels[p] = tf ? classify_entry(tf[0]) : 0u;
}

__global__ __launch_bounds__(256) void mip_classify_kernel(const uint8_t *__restrict__ index, size_t n, const float4 *__restrict__ tf,
                                                           uint32_t *__restrict__ pixels)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        pixels[i] = classify_entry(tf[index[i]]);
}
#endif

} // namespace VV_BIG_NS

template <> void launch_frame<FRAME_MIP, kBuild>(const MarchArgs &a, hipStream_t s) { VV_BIG_NS::launch_mip_impl(a, s); }
#ifdef VV_BUILD_LINEAR
void launch_fill(const MarchArgs &a, const PixelRect &rect, hipStream_t s)
{
    if (a.P.W < 2 || a.P.H < 2) return;
    dim3 grid((unsigned)((a.P.W - 1 + 63) / 64), (unsigned)((a.P.H - 1 + 3) / 4));
    hipLaunchKernelGGL(small::fill_outside_kernel, grid, dim3(256), 0, s, a.P, rect, a.fill_tf, a.pixels, a.index, a.stat, a.hit);
}
void launch_mip_classify(const uint8_t *index, size_t n, const float4 *tf, uint32_t *pixels, hipStream_t s)
{
    if (!n) return;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(small::mip_classify_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, index, n, tf, pixels);
}
#endif

} // namespace vv
