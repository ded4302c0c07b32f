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
//                       (MAX / MIN) or one predicated add (MEAN), plus the count of counted samples.
// The pixels beside the volume's screen rectangle, which proj_kernel's tiles do not cover, are fill_outside_kernel's (vv_mip.hip; n = 0: v = 0, tf[0], {0, 0}).
// Like vv_mip.hip this file is compiled once per volume layout (vv_layout.h); each unit defines launch_frame<FRAME_PROJ, kBuild>.
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

static void launch_proj_impl(const MarchArgs &a, hipStream_t s)
{
    const unsigned nblocks = grid_blocks(a.strips);
    if (!nblocks) return;
    for_sampler(a, [&](auto VOXEL, auto TEX8, auto INSTR) {
        auto launch = [&](auto MODE) {
            for_unroll(a, [&](auto U) {
                hipLaunchKernelGGL((proj_kernel<VOXEL(), TEX8(), INSTR(), U(), MODE()>), dim3(nblocks), dim3(256), reducer_lds(a), s,
                                   a.P, a.V, a.tf, a.rad, a.pixels, a.index, a.stat, a.counter, a.I, a.strips);
            });
        };
        switch (a.proj_mode) {                  // (the mode sits between the sampler and U: see for_sampler on the order of the instantiations)
        case VV_PROJ_MIN:  launch(int_c<VV_PROJ_MIN>{}); break;
        case VV_PROJ_MEAN: launch(int_c<VV_PROJ_MEAN>{}); break;
        default:           launch(int_c<VV_PROJ_MAX>{}); break;
        }
    });
}

} // namespace VV_BIG_NS

template <> void launch_frame<FRAME_PROJ, kBuild>(const MarchArgs &a, hipStream_t s) { VV_BIG_NS::launch_proj_impl(a, s); }

} // namespace vv
