// vv_iso.hip -- isosurface (first-hit) kernels for gfx950 (MI355X).  No reference counterpart: the reference composites only.
//
// An isosurface frame marches the rays and samples of a MIP frame (vv_mip.hip) -- same end points, per-slab radius (rad_kernel), setup_ray with its
// cut plane, 30-sample chunks, (pos - .5) / scale + .5 mapping, filter and 8-bit classification index k -- and stops each ray at its first executed sample
// with k >= level: the hit.  Per pixel it keeps the hit's k, its ordinal (samples executed up to and including it) and the march's own accumulated
// position; the epilogue takes six more samples around the hit (central differences of k), shades the table's entry k by a headlight and writes up to three
// images: RGBA, index, and a 16-byte record (x, y, z, ordinal).  Per sample the work behind the trilinear reconstruction is one compare and a few selects.
//   * iso_kernel        the march: mip_kernel's tile grid, block order, trip structure, fetch and scheduling barrier; a lane with a hit stops contributing and
//                       a wave leaves both loops as soon as none of its lanes has samples left (one ballot per trip) -- the early exit is what makes the frame cheap;
// The pixels beside the volume's screen rectangle, which iso_kernel's tiles do not cover, are fill_outside_kernel's (vv_mip.hip; no hit: zeros in all three images).
// Like vv_mip.hip this file is compiled once per volume layout (vv_layout.h); each unit defines launch_frame<FRAME_ISO, kBuild>.
#include "vv_device.h"
#include "vv_kernels.h"
#include "vv_layout.h"

namespace vv {
namespace VV_BIG_NS {

// the 8-bit index at texture coordinates t, through the fetch, filter, classification and bounds test of the march (0 outside [0,1)^3)
template <int VOXEL, bool TEX8>
__device__ __forceinline__ int iso_index_at(const VolumeView &V, float tx, float ty, float tz)
{
    typename CornerSel<VOXEL>::type C;
    fetch_any<VOXEL, TEX8>(V, tx, ty, tz, C);
    return (int)classify_index<VOXEL>(C, tx, ty, tz);
}

// Headlight shade of a hit: central differences of k at t +- h along each axis, scaled to cube space (up to the common factor 1/2), against the ray.
// Strict binary32 in the order written; IEEE sqrtf and / (once per pixel: the gated cores of the Phong kernel are not needed).
__device__ __forceinline__ float iso_shade(const FrameParams &P, const IsoParams &Q, const int g[3], const f3 dir)
{
#pragma clang fp contract(off)
    const f3 G = mk3(((float)g[0] * P.inv_scale[0]) * Q.n[0], ((float)g[1] * P.inv_scale[1]) * Q.n[1], ((float)g[2] * P.inv_scale[2]) * Q.n[2]);
    const float dp = dot3s(G, dir);
    const float len = sqrtf(dot3s(G, G));
    const float diffuse = len > 0.f ? fminf(fabsf(dp) / len, 1.0f) : 0.0f;
    return 0.3f + 0.7f * diffuse;
}

// blockDim = 256 = 4 waves; block -> (strip, tile) and wave -> pixels through vv_tiles.h, as in mip_kernel.  `pixels`, `index` and `hit` may each be
// null (vv_render_iso wants at least one).  Instrumented and uninstrumented frames execute the same samples.
template <int VOXEL, bool TEX8, bool INSTR, int U>
__global__ __launch_bounds__(256) void iso_kernel(FrameParams P, VolumeView V, IsoParams Q,
                                                  const float4 *__restrict__ tf,
                                                  const float *__restrict__ rad,
                                                  uint32_t *__restrict__ pixels,
                                                  uint8_t *__restrict__ index,
                                                  float4 *__restrict__ hit,
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
        if (!(length < 0.001f)) {                                    // (a zero-length ray executes nothing: no hit)
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

    const uint32_t level = (uint32_t)Q.level;
    bool found = false;
    uint32_t hk = 0;                      // the hit: its index,
    int hord = 0, before = 0;             // its ordinal (`before` = samples of the chunks already marched),
    float hx = 0.f, hy = 0.f, hz = 0.f;   // and the march's position at it

    float dist = r.dist0;
    for (int chunk = 0; chunk < P.max_chunks && __any(dist < r.upper); ++chunk) {
        int n = chunk_count(dist, r.upper, r.sstep);
        float px, py, pz;
        {
#pragma clang fp contract(off)
            px = r.origin.x + r.dir.x * dist;
            py = r.origin.y + r.dir.y * dist;
            pz = r.origin.z + r.dir.z * dist;
        }
        // a trip while any lane has samples left in this chunk (a lane's n drops to 0 at its hit); lanes with fewer samples are predicated, not branched
        for (int i0 = 1; __any(i0 <= n); i0 += U) {
            float sx[U], sy[U], sz[U], tx[U], ty[U], tz[U];
            typename CornerSel<VOXEL>::type C[U];
            if (INSTR) slots += (unsigned long long)U * 64ull;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                px += r.sdir.x; py += r.sdir.y; pz += r.sdir.z;
                sx[u] = px; sy[u] = py; sz[u] = pz;
                // a lane without this sample -- past its ray's end, or past its hit (n = 0) -- gathers texel 0 with the others of its kind instead of marching on
                // through the volume: one line for all of them, so the bytes a frame moves fall with the samples it executes (three selects per sample)
                const bool on = i0 + u <= n;
                tx[u] = on ? __builtin_fmaf(px - 0.5f, P.inv_scale[0], 0.5f) : 0.f;
                ty[u] = on ? __builtin_fmaf(py - 0.5f, P.inv_scale[1], 0.5f) : 0.f;
                tz[u] = on ? __builtin_fmaf(pz - 0.5f, P.inv_scale[2], 0.5f) : 0.f;
                fetch_any<VOXEL, TEX8>(V, tx[u], ty[u], tz[u], C[u]);
            }
            __builtin_amdgcn_sched_barrier(0);           // all gathers of the trip are issued before the first is consumed
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool live = i0 + u <= n && !found;
                const uint32_t k = classify_index<VOXEL>(C[u], tx[u], ty[u], tz[u]);
                if (INSTR) instrument_sample<VOXEL, TEX8>(I, V, tx[u], ty[u], tz[u], live, executed);
                const bool h = live && k >= level;
                hk = h ? k : hk; hord = h ? before + i0 + u : hord;
                hx = h ? sx[u] : hx; hy = h ? sy[u] : hy; hz = h ? sz[u] : hz;
                found = found || h;
            }
            if (found) n = 0;
        }
        before += n;
        if (found) r.upper = -1.f;
        {
#pragma clang fp contract(off)
            dist += r.sstep * kChunkSteps;
        }
    }

    uint32_t rgba = 0;
    if (pixels) {                         // (the shade is all the gradient is for: a frame without an RGBA image issues no gather for it)
        if (found) {
            // the hit's texture coordinates, from its position by the march's own expression: the same bits
            const float tx = __builtin_fmaf(hx - 0.5f, P.inv_scale[0], 0.5f);
            const float ty = __builtin_fmaf(hy - 0.5f, P.inv_scale[1], 0.5f);
            const float tz = __builtin_fmaf(hz - 0.5f, P.inv_scale[2], 0.5f);
            const float gx[6] = {tx + Q.h[0], tx - Q.h[0], tx, tx, tx, tx};
            const float gy[6] = {ty, ty, ty + Q.h[1], ty - Q.h[1], ty, ty};
            const float gz[6] = {tz, tz, tz, tz, tz + Q.h[2], tz - Q.h[2]};
            int k6[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                k6[j] = iso_index_at<VOXEL, TEX8>(V, gx[j], gy[j], gz[j]);
                if (INSTR && (I.lines || I.pairs) && I.lines_all) mark_sample_lines<VOXEL, TEX8>(I, V, gx[j], gy[j], gz[j]);
            }
            const int g[3] = {k6[0] - k6[1], k6[2] - k6[3], k6[4] - k6[5]};
            const float shade = iso_shade(P, Q, g, r.dir);
            const float4 e = tf[hk];
            {
#pragma clang fp contract(off)
                rgba = pack_rgba(e.x * shade, e.y * shade, e.z * shade, 1.0f);
            }
        }
    }

    if (in_frame) {
        const size_t p = (size_t)y * P.W + x;
        if (index) index[p] = (uint8_t)hk;
        if (hit) hit[p] = found ? make_float4(hx, hy, hz, (float)hord) : make_float4(0.f, 0.f, 0.f, 0.f);      // one 16-byte store
        if (pixels) pixels[p] = rgba;
    }
    if (INSTR) flush_counters(counter, executed, slots);
}

static void launch_iso_impl(const MarchArgs &a, hipStream_t s)
{
    const unsigned nblocks = grid_blocks(a.strips);
    if (!nblocks) return;
    for_variant(a, [&](auto VOXEL, auto TEX8, auto INSTR, auto U) {
        hipLaunchKernelGGL((iso_kernel<VOXEL(), TEX8(), INSTR(), U()>), dim3(nblocks), dim3(256), reducer_lds(a), s,
                           a.P, a.V, a.iso, a.tf, a.rad, a.pixels, a.index, a.hit, a.counter, a.I, a.strips);
    });
}

} // namespace VV_BIG_NS

template <> void launch_frame<FRAME_ISO, kBuild>(const MarchArgs &a, hipStream_t s) { VV_BIG_NS::launch_iso_impl(a, s); }

} // namespace vv
