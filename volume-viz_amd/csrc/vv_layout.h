// vv_layout.h -- the volume layout a march translation unit is compiled for (internal; included once per unit, after vv_device.h).
//
// The four kernel files (vv_raymarch.hip, vv_mip.hip, vv_iso.hip, vv_proj.hip) are each compiled seven times: as they are, and with the layout macros
// the Makefile's LAYOUT_FLAGS table gives (VV_BIG_VOLUME / VV_BRICKED (+ VV_BRICKED_CACHED) / VV_ZPAIR / VV_ZFAST / VV_ZPAIR + VV_XPAIR).  This header turns
// those macros -- here and nowhere else -- into the unit's namespace (VV_BIG_NS), its build (kBuild: the launcher specialisation it defines), its layout
// constant (kLayout; two builds share the bricked layout), its corner registers and fetch, the instrumentation of instrumented frames, and the host-side
// choice of a kernel instantiation (for_variant).  The unit for the linear layout, which also holds the kernels that exist once (rad_kernel,
// fill_outside_kernel, mip_classify_kernel), sees VV_BUILD_LINEAR.
//
// The builds, in the order of the chain below:
//   xpair         the z-pair build on the x-pair copy (the z-pair copy with x and z in each other's roles: records {v(x,y,z), v(x+1,y,z)}, z fastest; handed
//                 over in VolumeView::zpair): side views of the volumes whose front views take the z-pair copy, two gathers per sample instead of four;
//   zpair         the z-pair copy (VolumeView::zpair: records {v(x,y,z), v(x,y,z+1)}): views along the memory axis, two 16-byte gathers per sample
//                 instead of four 8-byte ones;
//   brick_cached  the bricked build once more for volumes that live in the caches (up to 1 GiB): the same kernels in namespace brickc, compiled without
//                 the SLP vectoriser (Makefile: NOSLP_LAYOUTS);
//   brick         the bricked copy (VolumeView::bricks: 4x4x4-voxel bricks with an x halo): views that are not aligned with the memory axis, where the
//                 linear layout costs one cache line per lane and gather;
//   zfast         the z-fastest copy (VolumeView::zfast): views whose screen x runs along the volume's z axis (side views) -- the lanes of a 32 x 2 wave
//                 tile read consecutive z, the rays march along x;
//   big           the linear layout above 4 GiB (64-bit slice base per sample; tex3d_raw in vv_device.h);
//   (none)        the linear layout up to 4 GiB.
#pragma once
#include <type_traits>
#include "vv_device.h"
#include "vv_kernels.h"

#if defined(VV_ZPAIR) && defined(VV_XPAIR)
#define VV_BIG_NS xpair
constexpr vv::MarchBuild kBuild = vv::MB_XPAIR;
constexpr int kLayout = vv::LAYOUT_ZPAIR;
#elif defined(VV_ZPAIR)
#define VV_BIG_NS zpair
constexpr vv::MarchBuild kBuild = vv::MB_ZPAIR;
constexpr int kLayout = vv::LAYOUT_ZPAIR;
#elif defined(VV_BRICKED) && defined(VV_BRICKED_CACHED)
#define VV_BIG_NS brickc
constexpr vv::MarchBuild kBuild = vv::MB_BRICKED_CACHED;
constexpr int kLayout = vv::LAYOUT_BRICKED;
#elif defined(VV_BRICKED)
#define VV_BIG_NS brick
constexpr vv::MarchBuild kBuild = vv::MB_BRICKED;
constexpr int kLayout = vv::LAYOUT_BRICKED;
#elif defined(VV_ZFAST)
#define VV_BIG_NS zfast
constexpr vv::MarchBuild kBuild = vv::MB_ZFAST;
constexpr int kLayout = vv::LAYOUT_ZFAST;
#elif defined(VV_BIG_VOLUME)
#define VV_BIG_NS big
constexpr vv::MarchBuild kBuild = vv::MB_LINEAR_BIG;
constexpr int kLayout = vv::LAYOUT_LINEAR_BIG;
#else
#define VV_BIG_NS small
#define VV_BUILD_LINEAR
constexpr vv::MarchBuild kBuild = vv::MB_LINEAR;
constexpr int kLayout = vv::LAYOUT_LINEAR;
#endif

// march_kernel, per build: what the trip loop does with sample slots no lane needs (vv_raymarch.hip).  kParkIdle: a lane that has no sample left when a
// trip begins gathers texel 0, as iso_kernel's lanes do, instead of marching on along its ray with only its blend predicated.  kLeaveEarly: the wave leaves
// a chunk's trip loop once no lane has a sample left in it.  Both are on in the builds whose bench workloads gained in the A/B against the parent commit
// (profiles/idle_lanes_ab.txt): big (C3), brick (C3 rotated), zfast (C3 from the side).  They are off, and the kernels instruction for instruction what they
// were, in the others: the builds for cache-resident volumes pay for the selects (C2 and C1 +5 % with parking; VALU-bound), and no bench workload runs
// the linear, the brick_cached or the x-pair build.  (The macros exist for A/B builds: make variant VFLAGS="-DVV_PARK_IDLE=0 -DVV_LEAVE_EARLY=1".)
#if defined(VV_BIG_VOLUME) || (defined(VV_BRICKED) && !defined(VV_BRICKED_CACHED)) || defined(VV_ZFAST)
#define VV_IDLE_LANES_DEFAULT 1
#else
#define VV_IDLE_LANES_DEFAULT 0
#endif
#ifndef VV_PARK_IDLE
#define VV_PARK_IDLE VV_IDLE_LANES_DEFAULT
#endif
#ifndef VV_LEAVE_EARLY
#define VV_LEAVE_EARLY VV_IDLE_LANES_DEFAULT
#endif
constexpr bool kParkIdle = VV_PARK_IDLE != 0;
constexpr bool kLeaveEarly = VV_LEAVE_EARLY != 0;

namespace vv {
namespace VV_BIG_NS {

// corner registers and fetch of the layout this translation unit is compiled for
template <int VOXEL> struct CornerSel { using type = Corners<VOXEL>; };
#ifdef VV_ZPAIR
template <> struct CornerSel<VV_VOXEL_F32> { using type = CornersZ; };
template <> struct CornerSel<VV_VOXEL_U8>  { using type = CornersZ8; };
#endif
template <int VOXEL, bool TEX8, class CT>
__device__ __forceinline__ void fetch_any(const VolumeView &V, float px, float py, float pz, CT &C)
{
#ifdef VV_ZPAIR
    fetch_corners_zpair<TEX8>(V, px, py, pz, C);
#else
    fetch_corners<VOXEL, TEX8, kLayout>(V, px, py, pz, C);
#endif
}

// Instrumented frames only: the 128-byte lines (offsets from the sampled layout's base) the gathers of one sample touch -- the address
// arithmetic of fetch_any() for this translation unit's layout, restated (InstrArgs::lines).
template <int VOXEL, bool TEX8>
__device__ __noinline__ void mark_sample_lines(const InstrArgs &I, const VolumeView &V, float px, float py, float pz)
{
    uint32_t ix, iy, iz;
    (void)axis_coord<TEX8>(px, (float)V.nx, (float)(V.nx - 1), ix);
    (void)axis_coord<TEX8>(py, (float)V.ny, (float)(V.ny - 1), iy);
    (void)axis_coord<TEX8>(pz, (float)V.nz, (float)(V.nz - 1), iz);
    constexpr bool F = VOXEL == VV_VOXEL_F32;
#if defined(VV_ZPAIR)
    const uint32_t rec = F ? 8u : 2u, bytes = F ? 16u : 4u;
#ifdef VV_XPAIR
    const uint64_t off = (uint64_t)ix * V.zp_slab_bytes + (uint64_t)iy * V.zp_row_bytes + (uint64_t)iz * rec;
#else
    const uint64_t off = (uint64_t)iz * V.zp_slab_bytes + (uint64_t)iy * V.zp_row_bytes + (uint64_t)ix * rec;
#endif
    mark_line_range(I, off, bytes); mark_line_range(I, off + V.zp_row_bytes, bytes);
#else
    if constexpr (kLayout == LAYOUT_LINEAR || kLayout == LAYOUT_LINEAR_BIG) {
        const uint64_t o = (uint64_t)iz * V.slice_bytes + (uint64_t)iy * V.row_bytes + (F ? ix * 4u : (ix & ~3u));
        mark_line_range(I, o, 8); mark_line_range(I, o + V.row_bytes, 8);
        mark_line_range(I, o + V.slice_bytes, 8); mark_line_range(I, o + V.slice_bytes + V.row_bytes, 8);
    } else if constexpr (kLayout == LAYOUT_ZFAST) {
        const uint64_t o = (uint64_t)ix * V.zf_slice_bytes + (uint64_t)iy * V.zf_row_bytes + (F ? iz * 4u : (iz & ~3u));
        mark_line_range(I, o, 8); mark_line_range(I, o + V.zf_row_bytes, 8);
        mark_line_range(I, o + V.zf_slice_bytes, 8); mark_line_range(I, o + V.zf_slice_bytes + V.zf_row_bytes, 8);
    } else {
        using G = BrickGeom<VOXEL>;
        uint64_t a[4];
        brick_offsets<VOXEL>(V, ix, iy, iz, a);
        if constexpr (F && G::halo == 0) {
            const uint32_t dx = (ix & (G::bx - 1u)) == G::bx - 1u ? G::brick - (G::bx - 1u) * 4u : 4u;
            for (int k = 0; k < 4; ++k) { mark_line_range(I, a[k], 4); mark_line_range(I, a[k] + dx, 4); }
        } else {
            for (int k = 0; k < 4; ++k) mark_line_range(I, a[k], 8);
        }
    }
#endif
}

// Instrumented frames only: one sample of march_kernel / mip_kernel / iso_kernel / proj_kernel, `live` when its lane executes it.  Counts it, marks its 8^3 bricks when it lies in
// the volume, and the lines its gathers touch (InstrArgs::lines_all: those of idle lanes and out-of-volume samples too).  The rule: bricks and, under lines_all = 0,
// lines are marked for `live && inv` samples and for no others -- an executed sample outside [0, 1)^3 is counted but marks nothing (it classifies to 0 whatever it
// loads), a lane that is predicated off marks nothing although its gathers are issued.  march_phong_kernel has its own rule (`need`, vv_raymarch.hip; InstrArgs).
template <int VOXEL, bool TEX8>
__device__ __forceinline__ void instrument_sample(const InstrArgs &I, const VolumeView &V, float tx, float ty, float tz, bool live, unsigned long long &executed)
{
    const bool inv = bounds_check(tx, ty, tz);
    if (live) {
        executed++;
        if (I.bricks && inv) mark_bricks(I.bricks, V, tx, ty, tz);
    }
    if ((I.lines || I.pairs) && (I.lines_all || (live && inv))) mark_sample_lines<VOXEL, TEX8>(I, V, tx, ty, tz);
}

// Instrumented frames only, at the end of a kernel: counter[0] += the wave's executed samples, counter[1] += its lane slots (developer statistic: lane
// utilisation; march_phong_kernel has none), counter[2] / counter[3] += 1 per wave that sampled the bricked / the z-pair copy.
__device__ __forceinline__ void flush_counters(unsigned long long *__restrict__ counter, unsigned long long executed, unsigned long long slots)
{
    const bool first = (threadIdx.x & 63) == 0;
    for (int o = 32; o > 0; o >>= 1) executed += __shfl_down(executed, o);
    if (first && executed) atomicAdd(counter, executed);
    if (first && slots) atomicAdd(counter + 1, slots);
    if (kLayout == LAYOUT_BRICKED && first && executed) atomicAdd(counter + 2, 1ull);
    if (kLayout == LAYOUT_ZPAIR && first && executed) atomicAdd(counter + 3, 1ull);
}

// Host: the kernel instantiation of a frame.  with_bool hands a run-time bool to the generic lambda f as std::true_type / std::false_type; for_sampler
// hands it a.V_type, a.tex8 and a.instr as the integral constants VOXEL, TEX8 and INSTR; for_variant adds a.unroll as U (2 or 3), so that f launches
// kernel<VOXEL(), TEX8(), INSTR(), U()>.  (The nesting is the order in which the compiler emits the instantiations into the code object: instrumented
// first, then f32 before u8, the 8-bit filter before the exact one, U = 3 before 2 -- the order of the hand-written ladders these replace.)
template <int N> using int_c = std::integral_constant<int, N>;
template <class F> static void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F> static void for_sampler(const MarchArgs &a, F &&f)
{
    with_bool(a.instr, [&](auto instr) { with_bool(a.V_type == VV_VOXEL_F32, [&](auto f32) { with_bool(a.tex8, [&](auto tex8) {
        f(int_c<decltype(f32)::value ? VV_VOXEL_F32 : VV_VOXEL_U8>{}, tex8, instr);
    }); }); });
}
template <class F> static void for_unroll(const MarchArgs &a, F &&f) { if (a.unroll == 3) f(int_c<3>{}); else f(int_c<2>{}); }
template <class F> static void for_variant(const MarchArgs &a, F &&f)
{
    for_sampler(a, [&](auto VOXEL, auto TEX8, auto INSTR) { for_unroll(a, [&](auto U) { f(VOXEL, TEX8, INSTR, U); }); });
}

// Dynamic LDS of a reducer kernel's launch (mip_kernel, iso_kernel, proj_kernel).  Blocks per CU: the launch policy's lds_reserve values were measured on
// march_kernel, whose blocks hold a 4 KB table in LDS besides the reserve.  The reducers have no LDS of their own, so the table's 4 KB are added to the
// reserve here: the same LDS per block, the same number of resident blocks per CU (and waves on its L1) as the march frame of the same view.
static inline size_t reducer_lds(const MarchArgs &a) { return (size_t)a.lds_reserve + kMipTableBytes; }

} // namespace VV_BIG_NS
} // namespace vv
