// vv_slab.hip -- thick-slab slice views for gfx950: the maximum, minimum or mean over K samples of the slice sampler along the slab's axis
// (no reference counterpart; the contract is the comment on vv_slice_slab in include/volviz.h).
//
//   slab_kernel<VOXEL, TEX8, BIG, MODE>   one lane per output pixel; K samples in groups of VV_SLAB_U
//
// Every sample is slice_kernel's own (vv_aux.hip): the same position arithmetic with the slab offset added to one operand, the same bounds test, the
// same filtered value.  What the kernel adds is the order of the work: the gathers of a whole group are issued before the first of them is consumed
// (fetch_corners / finish_corners, vv_device.h), which a loop around slice_kernel's one sample per thread cannot do.
#include "vv_device.h"
#include "vv_kernels.h"

#ifndef VV_SLAB_U
#define VV_SLAB_U 4           // samples per group: their gathers are in flight together (profiles/slab_c3.txt)
#endif
#ifndef VV_SLAB_BW
#define VV_SLAB_BW 16         // thread block: VV_SLAB_BW x VV_SLAB_BH pixels, 256 threads (16 x 16 as slice_kernel, or 64 x 4: a wave is one row of 64)
#endif
#ifndef VV_SLAB_BH
#define VV_SLAB_BH 16
#endif
static_assert(VV_SLAB_U >= 1 && VV_SLAB_U <= 16, "VV_SLAB_U: the group's corners live in registers");
static_assert(VV_SLAB_BW * VV_SLAB_BH == 256 && VV_SLAB_BW % 16 == 0, "slab_kernel blocks are 256 threads, whole waves per pixel-row segment");

namespace vv {

template <int VOXEL, bool TEX8, bool BIG, int MODE>
__global__ __launch_bounds__(256) void slab_kernel(SlabArgs A)
{
#pragma clang fp contract(off)
    constexpr int U = VV_SLAB_U;
    const size_t i = threadIdx.x + (size_t)blockIdx.x * VV_SLAB_BW;
    const size_t j = threadIdx.y + (size_t)blockIdx.y * VV_SLAB_BH;
    // storage: slice_kernel's three tests, in its order
    if (!(j < A.height && i < A.width)) return;
    const size_t offset = j * A.height + i;
    if (offset >= A.height * A.width) return;
    if (i >= A.height && j + 1 < A.height) return;
    const float u = ((float)i) / ((float)A.width), w = ((float)j) / ((float)A.height);
    const float ix = 1.0f / A.scale[0], iy = 1.0f / A.scale[1], iz = 1.0f / A.scale[2];

    // what does not depend on the sample.  Advanced: the first two products of each row (the sum runs left to right).  Canonical: the texture
    // coordinates of the two axes the slab does not run along, and the slab axis' displacement and reciprocal scale.
    const int axis = A.orientation == VV_SAGITTAL ? 2 : A.orientation == VV_HORIZONTAL ? 1 : 0;
    float qx, qy, qz, d_a = 0.f, i_a = 0.f;
    if (A.advanced) {
        qx = A.trans[0] * u + A.trans[1] * w;
        qy = A.trans[4] * u + A.trans[5] * w;
        qz = A.trans[8] * u + A.trans[9] * w;
    } else {
        float px = 0.f, py = 0.f, pz = 0.f;
        switch (A.orientation) {                                  // slice_kernel's switch
            case VV_SAGITTAL:   pz += 0.f; py += w;   px += u;   break;
            case VV_HORIZONTAL: pz += u;   py += 0.f; px += w;   break;
            default:            pz += u;   py += w;   px += 0.f; break;      // VV_CORONAL (the API admits no other)
        }
        px += A.dx; py += A.dy; pz += A.dz;
        qx = __builtin_fmaf(px - 0.5f, ix, 0.5f);
        qy = __builtin_fmaf(py - 0.5f, iy, 0.5f);
        qz = __builtin_fmaf(pz - 0.5f, iz, 0.5f);
        d_a = axis == 0 ? A.dx : axis == 1 ? A.dy : A.dz;
        i_a = axis == 0 ? ix : axis == 1 ? iy : iz;
    }
    const int K = A.samples;
    const float spacing = A.thickness / (float)K;
    const float half = 0.5f * (float)(K - 1);

    float best = 0.f;            // MAX / MIN: the extremum so far; MEAN: the running sum
    int arg = -1, n = 0;         // MAX / MIN: its sample; n: executed samples
    for (int k0 = 0; k0 < K; k0 += U) {
        // 1. positions and bounds tests of the group (samples beyond K - 1 are masked: the remainder group is this code too)
        float px[U], py[U], pz[U];
        bool in[U], any = false;
#pragma unroll
        for (int g = 0; g < U; ++g) {
            const int k = k0 + g;
            const float o = ((float)k - half) * spacing;
            if (A.advanced) {
                const float rz = 0.5f + o, rw = 1.f;
                float x = qx + A.trans[2]  * rz + A.trans[3]  * rw;
                float y = qy + A.trans[6]  * rz + A.trans[7]  * rw;
                float z = qz + A.trans[10] * rz + A.trans[11] * rw;
                x *= ix; y *= iy; z *= iz;
                px[g] = __builtin_fmaf(x - 0.5f, ix, 0.5f);
                py[g] = __builtin_fmaf(y - 0.5f, iy, 0.5f);
                pz[g] = __builtin_fmaf(z - 0.5f, iz, 0.5f);
            } else {
                const float d = d_a + o;                          // the one add, made before anything else
                float p = 0.f; p += 0.f; p += d;                  // the axis the switch leaves at 0
                p = __builtin_fmaf(p - 0.5f, i_a, 0.5f);
                px[g] = axis == 0 ? p : qx; py[g] = axis == 1 ? p : qy; pz[g] = axis == 2 ? p : qz;
            }
            in[g] = k < K && px[g] < 1.0f && px[g] >= 0.0f && py[g] < 1.0f && py[g] >= 0.0f && pz[g] < 1.0f && pz[g] >= 0.0f;
            any = any || in[g];
        }
        // 2. nothing to do for the whole wave: no gather is issued (a canonical slab leaves the volume for every pixel at once)
        if (__ballot(any) == 0) continue;
        // 3. every gather of the group, back to back.  A lane whose sample is outside still issues its own: axis_coord clamps the index, so the
        //    address lies inside the allocation, and the value is dropped below
        Corners<VOXEL> C[U];
#pragma unroll
        for (int g = 0; g < U; ++g)
            fetch_corners<VOXEL, TEX8, BIG ? LAYOUT_LINEAR_BIG : LAYOUT_LINEAR>(A.V, px[g], py[g], pz[g], C[g]);
        // 4. lerps and the reduction, in sample order
#pragma unroll
        for (int g = 0; g < U; ++g) {
            const float L = finish_corners<VOXEL>(C[g]);
            const float s = (VOXEL == VV_VOXEL_U8) ? L / 255.0f : L;      // what slice_kernel stores
            if (in[g]) {
                if (MODE == VV_SLAB_MEAN) best = n == 0 ? s : best + s;
                else if (n == 0 || (MODE == VV_SLAB_MAX ? s > best : s < best)) { best = s; arg = k0 + g; }
                ++n;
            }
        }
    }
    if (MODE == VV_SLAB_MEAN) { best = n ? best / (float)n : 0.f; arg = n; }
    A.buffer[offset] = best;
    if (A.aux) A.aux[offset] = arg;
}

template <int VOXEL, bool TEX8, bool BIG>
static void launch_slab_mode(const SlabArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    switch (a.mode) {
        case VV_SLAB_MAX: hipLaunchKernelGGL((slab_kernel<VOXEL, TEX8, BIG, VV_SLAB_MAX>),  grid, block, 0, s, a); break;
        case VV_SLAB_MIN: hipLaunchKernelGGL((slab_kernel<VOXEL, TEX8, BIG, VV_SLAB_MIN>),  grid, block, 0, s, a); break;
        default:          hipLaunchKernelGGL((slab_kernel<VOXEL, TEX8, BIG, VV_SLAB_MEAN>), grid, block, 0, s, a); break;
    }
}
template <int VOXEL, bool TEX8>
static void launch_slab_big(const SlabArgs &a, dim3 grid, dim3 block, hipStream_t s)
{
    if (a.V.big) launch_slab_mode<VOXEL, TEX8, true>(a, grid, block, s);
    else         launch_slab_mode<VOXEL, TEX8, false>(a, grid, block, s);
}

void launch_slab(const SlabArgs &a, hipStream_t s)
{
    dim3 block(VV_SLAB_BW, VV_SLAB_BH), grid((unsigned)((a.width + VV_SLAB_BW - 1) / VV_SLAB_BW), (unsigned)((a.height + VV_SLAB_BH - 1) / VV_SLAB_BH));
    if (a.V_type == VV_VOXEL_F32) {
        if (a.tex8) launch_slab_big<VV_VOXEL_F32, true>(a, grid, block, s);
        else        launch_slab_big<VV_VOXEL_F32, false>(a, grid, block, s);
    } else {
        if (a.tex8) launch_slab_big<VV_VOXEL_U8, true>(a, grid, block, s);
        else        launch_slab_big<VV_VOXEL_U8, false>(a, grid, block, s);
    }
}

} // namespace vv
