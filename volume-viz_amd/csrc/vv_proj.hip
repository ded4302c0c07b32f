// vv_proj.hip -- projection kernels for gfx950 (MI355X): maximum, minimum and mean intensity, with the extremum's place along the ray.
// No reference counterpart: the reference composites only.
//
// A projection frame marches the rays and executed samples of a MIP frame (vv_mip.hip) -- same end points, per-slab radius (rad_kernel), setup_ray with its
// cut plane, 30-sample chunks, (pos - .5) / scale + .5 mapping, filter and 8-bit classification index k -- but reduces only the samples that lie in the
// volume: an executed sample is *counted* iff its texture coordinates pass bounds_check.  (mip_kernel gives the others index 0, which never wins a maximum;
// it would win every minimum and bias every mean.)  Per pixel, in integers:
//   MAX / MIN   v = the extremum of k over the counted samples, ord = the 1-based ordinal among the ray's executed samples of the first counted sample
//               that attains it, n = the counted samples;
//   MEAN        s = the sum of k over the counted samples, v = (2 s + n) / (2 n);
//   n == 0      v = 0, ord = 0, s = 0.
// Up to three images: RGBA (mip_kernel's conversion of tf[v]), index (v) and a record of two uint32 ({ord, n} or {s, n}), written in one 8-byte store.
//   * proj_kernel       the march: mip_kernel's tile grid, block order, trip structure, fetch and scheduling barrier.  The ray state, the U samples in
//                       flight and the two or three words of reduction state live in registers; no LDS; the table is read once per pixel, in the epilogue.
//                       Per sample behind the reconstruction: the bounds test (made once: classify_raw, not classify_index), and one compare and two selects
//                       (MAX / MIN) or one predicated add (MEAN), plus the count of counted samples;
//   * proj_fill_kernel  the pixels beside the volume's screen rectangle (n = 0), which proj_kernel's tiles do not cover.
// Like vv_mip.hip this file is compiled once per volume layout (vv_layout.h), through the vv_proj_*.hip wrappers; each unit defines launch_proj<kBuild>.
#include "vv_device.h"
#include "vv_kernels.h"
#include "vv_layout.h"

namespace vv {
namespace VV_BIG_NS {

// blockDim = 256 = 4 waves; block -> (strip, tile) and wave -> pixels through vv_tiles.h, as in mip_kernel.  `pixels`, `index` and `stat` may each be
// null (vv_render_projection wants at least one).  A MAX / MIN frame without a stat image drops a ray once a counted sample has reached 255 / 0: nothing
// can change v, and ord and n are not asked for.  Every other frame, and every instrumented frame, marches each ray to its end.
template <int VOXEL, bool TEX8, bool INSTR, int U, int MODE>
__global__ __launch_bounds__(256) void proj_kernel(FrameParams P, VolumeView V,
                                                   const float4 *__restrict__ tf,
                                                   const float *__restrict__ rad,
                                                   uint32_t *__restrict__ pixels,
                                                   uint8_t *__restrict__ index,
                                                   uint2 *__restrict__ stat,
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

    unsigned long long executed = 0, slots = 0;

    Ray r;
    int alive = 0;
    if (in_frame) {
        f3 front, back;
        ray_endpoints(P, x, y, front, back);
        float length = vlen3(back.x - front.x, back.y - front.y, back.z - front.z);
        if (!(length < 0.001f)) {                                    // (a zero-length ray executes nothing: n = 0)
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

    // MAX / MIN: the extremum so far, one beyond the range until a sample is counted (so that the first counted sample always replaces it, and a later
    // one only when strictly greater / less), and its ordinal.  MEAN: acc is the sum.  `before` = executed samples of the chunks already marched.
    int ext = MODE == VV_PROJ_MIN ? 256 : -1;
    uint32_t acc = 0, cnt = 0;
    int before = 0;
    const bool drop = !INSTR && MODE != VV_PROJ_MEAN && stat == nullptr;

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
                const bool counted = live && bounds_check(tx[u], ty[u], tz[u]);
                const int k = (int)classify_raw<VOXEL>(C[u]);
                if (MODE == VV_PROJ_MEAN) {
                    acc += counted ? (uint32_t)k : 0u;
                } else {
                    const bool better = counted && (MODE == VV_PROJ_MIN ? k < ext : k > ext);
                    ext = better ? k : ext;
                    acc = better ? (uint32_t)(before + i0 + u) : acc;
                }
                cnt += counted ? 1u : 0u;
                if (INSTR) instrument_sample<VOXEL, TEX8>(I, V, tx[u], ty[u], tz[u], live, executed);
            }
        }
        before += n;
        if (drop && ext == (MODE == VV_PROJ_MIN ? 0 : 255)) r.upper = -1.f;
        {
#pragma clang fp contract(off)
            dist += r.sstep * kChunkSteps;
        }
    }

    if (in_frame) {
        uint32_t v;
        if (MODE == VV_PROJ_MEAN) {
            // the mean rounded half up, in 64 bits as the contract writes it (s <= 255 n and n < 2^24: 2 s + n can pass 2^32); once per pixel
            const unsigned long long num = 2ull * acc + cnt;
            v = cnt ? (uint32_t)(num / (2ull * cnt)) : 0u;
        } else {
            v = cnt ? (uint32_t)ext : 0u;
        }
        const size_t p = (size_t)y * P.W + x;
        if (index) index[p] = (uint8_t)v;
        if (stat) stat[p] = make_uint2(cnt ? acc : 0u, cnt);                  // one 8-byte store: {ord, n} or {s, n}
        if (pixels) { const float4 e = tf[v]; pixels[p] = pack_rgba(e.x, e.y, e.z, e.w); }
    }
    if (INSTR) flush_counters(counter, executed, slots);
}

template <int VOXEL, bool TEX8, bool INSTR, int MODE>
static void launch_proj_m(const MarchArgs &a, hipStream_t s)
{
    const unsigned nblocks = grid_blocks(a.strips);
    if (!nblocks) return;
    // Blocks per CU: as launch_mip_t.  proj_kernel has no LDS of its own either, so march_kernel's 4 KB table is added to the reserve: the same
    // number of resident blocks per CU as the march and MIP frames of the same view.
    const size_t lds = (size_t)a.lds_reserve + kMipTableBytes;
    dim3 grid(nblocks);
    if (a.unroll == 3)
        hipLaunchKernelGGL((proj_kernel<VOXEL, TEX8, INSTR, 3, MODE>), grid, dim3(256), lds, s,
                           a.P, a.V, a.tf, a.rad, a.pixels, a.index, a.stat, a.counter, a.I, a.strips);
    else
        hipLaunchKernelGGL((proj_kernel<VOXEL, TEX8, INSTR, 2, MODE>), grid, dim3(256), lds, s,
                           a.P, a.V, a.tf, a.rad, a.pixels, a.index, a.stat, a.counter, a.I, a.strips);
}

template <int VOXEL, bool TEX8, bool INSTR>
static void launch_proj_t(const MarchArgs &a, hipStream_t s)
{
    if (a.proj_mode == VV_PROJ_MIN) launch_proj_m<VOXEL, TEX8, INSTR, VV_PROJ_MIN>(a, s);
    else if (a.proj_mode == VV_PROJ_MEAN) launch_proj_m<VOXEL, TEX8, INSTR, VV_PROJ_MEAN>(a, s);
    else launch_proj_m<VOXEL, TEX8, INSTR, VV_PROJ_MAX>(a, s);
}

static void launch_proj_impl(const MarchArgs &a, hipStream_t s)
{
    const bool f32 = a.V_type == VV_VOXEL_F32;
    if (a.instr) {
        if (f32) { if (a.tex8) launch_proj_t<VV_VOXEL_F32, true, true>(a, s); else launch_proj_t<VV_VOXEL_F32, false, true>(a, s); }
        else     { if (a.tex8) launch_proj_t<VV_VOXEL_U8,  true, true>(a, s); else launch_proj_t<VV_VOXEL_U8,  false, true>(a, s); }
    } else {
        if (f32) { if (a.tex8) launch_proj_t<VV_VOXEL_F32, true, false>(a, s); else launch_proj_t<VV_VOXEL_F32, false, false>(a, s); }
        else     { if (a.tex8) launch_proj_t<VV_VOXEL_U8,  true, false>(a, s); else launch_proj_t<VV_VOXEL_U8,  false, false>(a, s); }
    }
}

#ifdef VV_BUILD_LINEAR       // (once: the build for the linear layout)
// The owned pixels outside the rectangle proj_kernel's tiles cover: their rays miss the volume (vv_render: screen_rect), so n = 0 in every mode.
// One thread per pixel of the frame; threads inside the rectangle, in column W-1 / row H-1 or in another shard's rows leave at once.
__global__ __launch_bounds__(256) void proj_fill_kernel(FrameParams P, PixelRect R, const float4 *__restrict__ tf,
                                                        uint32_t *__restrict__ pixels, uint8_t *__restrict__ index, uint2 *__restrict__ stat)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x > P.W - 2 || y > P.H - 2 || !row_owned(P, y)) return;
    if (x >= R.x0 && x < R.x1 && y >= R.y0 && y < R.y1) return;
    const size_t p = (size_t)y * P.W + x;
    if (index) index[p] = 0;
    if (stat) stat[p] = make_uint2(0u, 0u);
    if (pixels) { const float4 e = tf[0]; pixels[p] = pack_rgba(e.x, e.y, e.z, e.w); }
}
#endif

} // namespace VV_BIG_NS

template <> void launch_proj<kBuild>(const MarchArgs &a, hipStream_t s) { VV_BIG_NS::launch_proj_impl(a, s); }
#ifdef VV_BUILD_LINEAR
void launch_proj_fill(const MarchArgs &a, const PixelRect &rect, hipStream_t s)
{
    if (a.P.W < 2 || a.P.H < 2) return;
    dim3 grid((unsigned)((a.P.W - 1 + 63) / 64), (unsigned)((a.P.H - 1 + 3) / 4));
    hipLaunchKernelGGL(small::proj_fill_kernel, grid, dim3(256), 0, s, a.P, rect, a.tf, a.pixels, a.index, a.stat);
}
#endif

} // namespace vv
