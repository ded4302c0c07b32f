// device_math_check -- exhaustive sweeps of the kernels' arithmetic helpers (csrc/vv_device.h) on the GPU, against plain definitions written here
// in binary64 or integers.  An 8-bit frame cannot hold these pieces: a wrong last bit in a gradient quotient, a texture weight or a chunk count
// almost never moves a pixel.  The helpers are the __device__ __forceinline__ functions the kernels inline, compiled with the library's flags.
//
//   device_math_check --list                      the sweeps' names
//   device_math_check [--self-test] [name ...]    run the named sweeps (default: all); one JSON line each:
//       visited      inputs the sweep ran           mismatches   inputs on which helper and definition differ
//       first        the operands of the first (up to eight) mismatches recorded, as bit patterns
//       self_test_mismatches (--self-test)          the same sweep over a deliberately wrong twin of the helper: must be > 0
//   exit status 0: every sweep clean (`bounds`: exactly the pattern of -0.0 in each coordinate) and, with --self-test, every twin caught.
//
// No sweep compares a helper with another call of product code.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../csrc/vv_device.h"
#include "../csrc/vv_gate.h"

using namespace vv;

#define HIP_OK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "device_math_check: %s: %s\n", #e, hipGetErrorString(e_)); exit(2); } } while (0)

struct Record {
    unsigned long long mismatches;
    unsigned int noted, pad;
    unsigned int ops[8][4];
};
// the operands of a mismatch (the first eight that arrive; the count itself is added once per thread)
__device__ __forceinline__ void note(Record *R, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    if (*(volatile unsigned int *)&R->noted < 8u) {
        const unsigned int s = atomicAdd(&R->noted, 1u);
        if (s < 8u) { R->ops[s][0] = a; R->ops[s][1] = b; R->ops[s][2] = c; R->ops[s][3] = d; }
    }
}
__device__ __forceinline__ void tally(Record *R, unsigned long long bad) { if (bad) atomicAdd(&R->mismatches, bad); }
// A binary64 value the optimiser cannot see through: without it the compiler is entitled to narrow (float)((double)n / (double)d) to a binary32 division
// (the results are equal, which is the very theorem the definitions rest on) and the definition would run on the instructions under test.
__device__ __forceinline__ double wide(float v) { double w = (double)v; asm volatile("" : "+v"(w)); return w; }
__device__ __forceinline__ unsigned long long thread_index() { return (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; }

// ---------------------------------------------------------------------------------------------------------------------
// div: ph_div_core(n, d) against (float)((double)n / (double)d).  The binary64 quotient of two binary32 numbers, narrowed, is the correctly
// rounded binary32 quotient: 53 >= 2 * 24 + 2 (Figueroa, "When is double rounding innocuous?", 1995); the same holds for the square root.
// ---------------------------------------------------------------------------------------------------------------------
struct DenSpec { int lo, hi; };                                   // every mantissa of every binade lo .. hi (positive: the denominators are tangents and steps)
__host__ __device__ inline unsigned long long den_count(const DenSpec &S) { return (unsigned long long)(S.hi - S.lo + 1) << 23; }
__device__ __forceinline__ float den_of(const DenSpec &S, unsigned long long idx) { return __uint_as_float((uint32_t)(((unsigned long long)(127 + S.lo) << 23) + idx)); }
// wrong twins.  1: the core without its residual steps (the product by the refined reciprocal).  2: the core without its LAST residual step only -- a
// measurement, not a twin: one correction by an exact residual already lands within about 2^-24 ulp of the quotient, which misrounds only where a
// quotient lies that close to a midpoint, and over these operands none does (profiles/device_math_sensitivity.txt)
template <int TWIN>
__device__ __forceinline__ float twin_div(float n, float d)
{
    const float y0 = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, y0, 1.0f);
    const float y = __builtin_fmaf(e, y0, y0);
    const float q0 = n * y;
    if (TWIN == 1) return q0;
    const float r0 = __builtin_fmaf(-d, q0, n);
    return __builtin_fmaf(r0, y, q0);
}
template <int TWIN>
__global__ __launch_bounds__(256) void div_kernel(const float *__restrict__ nums, int n_nums, DenSpec S, Record *R)
{
    const unsigned long long idx = thread_index();
    if (idx >= den_count(S)) return;
    const float d = den_of(S, idx);
    const double dd = wide(d);
    unsigned long long bad = 0;
    for (int j = 0; j < n_nums; ++j) {
        const float n = nums[j];
        const float got = TWIN ? twin_div<TWIN>(n, d) : ph_div_core(n, d);
        const float want = (float)(wide(n) / dd);
        if (__float_as_uint(got) != __float_as_uint(want)) { ++bad; note(R, __float_as_uint(n), __float_as_uint(d), __float_as_uint(got), __float_as_uint(want)); }
    }
    tally(R, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// sqrt: ph_sqrt_core(x) against (float)sqrt((double)x) for every binary32 of the range, and ph_div_core(1, s) for every root s that comes out
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kSqrtLo = -52, kSqrtHi = 86;                        // binades swept: x in [2^-52, 2^87)
constexpr unsigned long long kSqrtCount = (unsigned long long)(kSqrtHi - kSqrtLo + 1) << 23;
template <int TWIN> __device__ __forceinline__ float twin_sqrt(float x)       // 1: without the test of the float above; 2: without the test of the float below
{
    const float s0 = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s0) - 1u), sp = __uint_as_float(__float_as_uint(s0) + 1u);
    float s = s0;
    if (TWIN != 2) { const float t1 = __builtin_fmaf(-sm, s0, x); s = (0.f >= t1) ? sm : s0; }
    if (TWIN != 1) { const float t2 = __builtin_fmaf(-sp, s0, x); s = (0.f < t2) ? sp : s; }
    return s;
}
template <int TWIN>
__global__ __launch_bounds__(256) void sqrt_kernel(Record *R, Record *Rinv)
{
    unsigned long long bad = 0, bad_inv = 0;
    for (unsigned long long idx = thread_index(); idx < kSqrtCount; idx += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((uint32_t)(((unsigned long long)(127 + kSqrtLo) << 23) + idx));
        const float s = TWIN ? twin_sqrt<TWIN>(x) : ph_sqrt_core(x);
        const float want = (float)sqrt(wide(x));
        if (__float_as_uint(s) != __float_as_uint(want)) { ++bad; note(R, __float_as_uint(x), 0u, __float_as_uint(s), __float_as_uint(want)); }
        if (!TWIN) {
            const float inv = ph_div_core(1.0f, s), want_inv = (float)(1.0 / wide(s));
            if (__float_as_uint(inv) != __float_as_uint(want_inv)) { ++bad_inv; note(Rinv, __float_as_uint(1.0f), __float_as_uint(s), __float_as_uint(inv), __float_as_uint(want_inv)); }
        }
    }
    tally(R, bad); if (!TWIN) tally(Rinv, bad_inv);
}

// ---------------------------------------------------------------------------------------------------------------------
// axis: axis_coord<TEX8>(x, n, n - 1) -> (texel index, weight).  Definition in binary64: x * n is exact (24 x 24 bits); p - 0.5 is exact
// unless x is so small that the difference spans more than 53 bits, and then the binary64 sum is rounded to odd, which makes the one narrowing to
// binary32 the correctly rounded x * n - 0.5 in every case (fmaf's value); clamp to [0, n - 1] (NaN -> 0); floor; an exact subtraction; TEX8:
// rint(a * 256) / 256, ties to even.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kAxisSizes = 12;
__constant__ uint32_t c_axis_sizes[kAxisSizes] = {1u, 2u, 3u, 5u, 7u, 16u, 255u, 256u, 257u, 1024u, 2048u, (1u << 24) - 1u};
constexpr uint32_t kUnitPatterns = 0x3F800000u;                   // every bit pattern of [0, 1)
constexpr int kAxisExtras = 22;
__constant__ uint32_t c_axis_extras[kAxisExtras] = {
    0x80000000u, 0x80000001u, 0x807FFFFFu, 0x80800000u,           // -0, the negative denormals' ends, -FLT_MIN
    0x8DA24260u, 0xBE800000u, 0xBF000000u, 0xBF800000u, 0xF149F2CAu, 0xFF7FFFFFu,      // -1e-30, -0.25, -0.5, -1, -1e30, -FLT_MAX
    0x3F800000u, 0x3F800001u, 0x3FC00000u, 0x40000000u, 0x4B800000u, 0x7149F2CAu, 0x7F7FFFFFu,      // 1, its successor, 1.5, 2, 2^24, 1e30, FLT_MAX
    0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00000u, 0x7F800001u };             // +-Inf, quiet NaNs of both signs, a signalling NaN
// (positive denormals are part of [0, 1))
__device__ __forceinline__ void ref_axis(float x, uint32_t n, bool tex8, uint32_t &i, float &a)
{
#pragma clang fp contract(off)
    if (x != x) { i = 0u; a = 0.f; return; }
    const double p = wide(x) * (double)n;
    double s = p - 0.5;
    if (p - p == 0.0) {                                            // finite: TwoSum(p, -0.5) gives the rounding error of s exactly
        const double bb = s - p, err = (p - (s - bb)) + (-0.5 - bb);
        unsigned long long sb = (unsigned long long)__double_as_longlong(s);
        if (err != 0.0 && !(sb & 1ull)) {                          // inexact and even: the neighbour on the side of the exact value is odd
            const bool away = (err > 0.0) == (s > 0.0);
            sb = away ? sb + 1ull : sb - 1ull;
            s = __longlong_as_double((long long)sb);
        }
    }
    float xb = (float)s;
    const float nm1 = (float)(n - 1u);
    if (!(xb > 0.f)) xb = 0.f; else if (xb > nm1) xb = nm1;
    const double fl = floor((double)xb);
    i = (uint32_t)fl;
    a = (float)((double)xb - fl);
    if (tex8) a = (float)(rint((double)a * 256.0) / 256.0);
}
// wrong twin: TEX8 weights truncated instead of rounded
template <bool TEX8>
__device__ __forceinline__ float twin_axis(float x, float n, float nm1, uint32_t &i)
{
    float xb = __builtin_fmaf(x, n, -0.5f);
    xb = __builtin_amdgcn_fmed3f(xb, 0.0f, nm1);
    i = (uint32_t)xb;
    float a = __builtin_amdgcn_fractf(xb);
    if (TEX8) a = floorf(a * 256.0f) * (1.0f / 256.0f);
    return a;
}
template <int TWIN>
__global__ __launch_bounds__(256) void axis_kernel(Record *R)
{
    const unsigned long long idx = thread_index();
    if (idx >= (unsigned long long)kUnitPatterns + kAxisExtras) return;
    const float x = __uint_as_float(idx < kUnitPatterns ? (uint32_t)idx : c_axis_extras[idx - kUnitPatterns]);
    unsigned long long bad = 0;
    for (int k = 0; k < kAxisSizes; ++k) {
        const uint32_t n = c_axis_sizes[k];
        const float fn = (float)n, fnm1 = (float)(n - 1u);
        uint32_t i0, i1, r0, r1;
        const float a0 = TWIN ? twin_axis<false>(x, fn, fnm1, i0) : axis_coord<false>(x, fn, fnm1, i0);
        const float a1 = TWIN ? twin_axis<true>(x, fn, fnm1, i1) : axis_coord<true>(x, fn, fnm1, i1);
        float w0, w1;
        ref_axis(x, n, false, r0, w0); ref_axis(x, n, true, r1, w1);
        if (i0 != r0 || !(a0 == w0)) { ++bad; note(R, __float_as_uint(x), n, i0, __float_as_uint(a0)); }
        if (i1 != r1 || !(a1 == w1)) { ++bad; note(R, __float_as_uint(x), n | 0x80000000u, i1, __float_as_uint(a1)); }      // (top bit of the size: TEX8)
    }
    tally(R, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// bounds: bounds_check against x >= 0 && x < 1, all 2^32 patterns in each coordinate in turn, the others at 0.5
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool twin_bounds(float x, float y, float z)          // wrong twin: admits 1.0
{
    uint32_t m = max(max(__float_as_uint(x), __float_as_uint(y)), __float_as_uint(z));
    return m <= 0x3F800000u;
}
template <int TWIN>
__global__ __launch_bounds__(256) void bounds_kernel(Record *R)
{
    unsigned long long bad = 0;
    for (unsigned long long idx = thread_index(); idx < (1ull << 32); idx += (unsigned long long)gridDim.x * blockDim.x) {
        const float v = __uint_as_float((uint32_t)idx);
        const bool want = v >= 0.0f && v < 1.0f;
        for (int c = 0; c < 3; ++c) {
            const float x = c == 0 ? v : 0.5f, y = c == 1 ? v : 0.5f, z = c == 2 ? v : 0.5f;
            const bool got = TWIN ? twin_bounds(x, y, z) : bounds_check(x, y, z);
            if (got != want) { ++bad; note(R, (uint32_t)idx, (uint32_t)c, got, want); }
        }
    }
    tally(R, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// convert: the index conversion of classify_raw / classify_index (index_of: u8 and f32 scaling) and one channel of pack_rgba, all 2^32 patterns.
// Definition of the conversion: NaN -> 0, negative -> 0, truncate, saturate at 255.  pack_rgba clamps to [0, 1] in front of it with fminf / fmaxf,
// which send a NaN to 1 (so does the reference's clamp), then scales by 255 in binary32.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ref_convert(float s)
{
    if (s != s) return 0u;
    if (s < 0.0f) return 0u;
    if (s >= 255.0f) return 255u;
    return (uint32_t)(int)truncf(s);
}
__device__ __forceinline__ float ref_times255(float v) { return (float)(wide(v) * 255.0); }       // (24 x 8 bits: the binary64 product is exact)
template <int VOXEL> __device__ __forceinline__ uint32_t twin_index_of(float L)                     // wrong twin: rounds instead of truncating
{
    float s = (VOXEL == VV_VOXEL_F32) ? L * 255.0f : L;
    return min((uint32_t)(s + 0.5f), 255u);
}
template <int TWIN>
__global__ __launch_bounds__(256) void convert_kernel(Record *R)
{
    unsigned long long bad = 0;
    for (unsigned long long idx = thread_index(); idx < (1ull << 32); idx += (unsigned long long)gridDim.x * blockDim.x) {
        const float v = __uint_as_float((uint32_t)idx);
        const uint32_t g8 = TWIN ? twin_index_of<VV_VOXEL_U8>(v) : index_of<VV_VOXEL_U8>(v), w8 = ref_convert(v);
        const uint32_t gf = TWIN ? twin_index_of<VV_VOXEL_F32>(v) : index_of<VV_VOXEL_F32>(v), wf = ref_convert(ref_times255(v));
        const float c = (v != v) ? 1.0f : (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v));
        const uint32_t gp = pack_rgba(v, 0.f, 0.f, 0.f), wp = ref_convert(ref_times255(c));
        if (g8 != w8) { ++bad; note(R, (uint32_t)idx, 0u, g8, w8); }
        if (gf != wf) { ++bad; note(R, (uint32_t)idx, 1u, gf, wf); }
        if (gp != wp) { ++bad; note(R, (uint32_t)idx, 2u, gp, wp); }
    }
    tally(R, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// chunks: chunk_count(dist, upper, sstep) against the loop of the reference itself (kernel.cu:248-257): under dist < upper, i = 1 .. 30 run until
// (float)i * sstep + dist > upper, uncontracted.  For ordered operands that counts the i with (float)i * sstep + dist <= upper; a NaN step never
// compares greater, so all 30 run.
// ---------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long kChunkRandom = 1ull << 28, kChunkPairs = 1ull << 20, kChunkPerPair = 32 * 5, kChunkNan = 1024, kChunkBehind = 1024;
constexpr unsigned long long kChunkCount = kChunkRandom + kChunkPairs * kChunkPerPair + kChunkNan + kChunkBehind;
struct ChunkSpec { float sstep_lo, sstep_hi, log2_lo, log2_hi; };
__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
__device__ __forceinline__ float ulp_move(float f, int by)         // by steps along the ordered binary32 line (through zero)
{
    const uint32_t b = __float_as_uint(f);
    long long o = (b & 0x80000000u) ? -(long long)(b & 0x7FFFFFFFu) : (long long)b;
    o += by;
    return __uint_as_float(o < 0 ? (0x80000000u | (uint32_t)(-o)) : (uint32_t)o);
}
__device__ __forceinline__ int ref_chunks(float dist, float upper, float sstep)
{
#pragma clang fp contract(off)
    if (!(dist < upper)) return 0;
    int n = 0;
    for (int i = 1; i <= 30; ++i) {
        const float vd = (float)i * sstep + dist;
        if (vd > upper) break;
        ++n;
    }
    return n;
}
__device__ __forceinline__ int twin_chunks(float dist, float upper, float sstep)      // wrong twin: a sample AT the end of the ray is not counted
{
#pragma clang fp contract(off)
    if (!(dist < upper)) return 0;
    float est = (upper - dist) / sstep;
    int n = est >= 30.f ? 30 : (est > 0.f ? (int)est : 0);
    while (n < 30 && !((float)(n + 1) * sstep + dist >= upper)) ++n;
    while (n > 0 && ((float)n * sstep + dist >= upper)) --n;
    if (sstep != sstep) n = 30;
    return n;
}
template <int TWIN>
__global__ __launch_bounds__(256) void chunks_kernel(ChunkSpec S, Record *R)
{
#pragma clang fp contract(off)
    unsigned long long bad = 0;
    for (unsigned long long idx = thread_index(); idx < kChunkCount; idx += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long j = idx, key;
        int kind;
        if (j < kChunkRandom) { kind = 0; key = j; }
        else if ((j -= kChunkRandom) < kChunkPairs * kChunkPerPair) { kind = 1; key = (1ull << 40) + j / kChunkPerPair; }
        else if ((j -= kChunkPairs * kChunkPerPair) < kChunkNan) { kind = 2; key = (2ull << 40) + j; }
        else { j -= kChunkNan; kind = 3; key = (3ull << 40) + j; }
        const unsigned long long h0 = mix64(key ^ 0x20251018ull), h1 = mix64(h0);
        const float u0 = (float)(h0 & 0xFFFFFFu) * 0x1p-24f, u1 = (float)((h0 >> 24) & 0xFFFFFFu) * 0x1p-24f, u2 = (float)(h1 & 0xFFFFFFu) * 0x1p-24f;
        float sstep = fminf(S.sstep_hi, fmaxf(S.sstep_lo, exp2f(S.log2_lo + u0 * (S.log2_hi - S.log2_lo))));      // log-uniform over the gate's steps
        float dist = u1 * kSqrt3, upper;
        if (kind == 0) upper = (h1 >> 63) ? u2 * kSqrt3 : dist + u2 * 32.f * sstep;        // anywhere in the cube, or within 32 steps of dist
        else if (kind == 1) { const int r = (int)(j % kChunkPerPair); upper = ulp_move((float)(r / 5) * sstep + dist, r % 5 - 2); }
        else if (kind == 2) { upper = u2 * kSqrt3 * 1.5f; sstep = __uint_as_float((j & 1) ? 0x7FC00000u : 0xFFC00001u); }
        else { upper = dist * u2; if (!(upper < dist)) upper = dist - 1.0f; }
        const int got = TWIN ? twin_chunks(dist, upper, sstep) : chunk_count(dist, upper, sstep), want = ref_chunks(dist, upper, sstep);
        if (got != want) { ++bad; note(R, __float_as_uint(dist), __float_as_uint(upper), __float_as_uint(sstep), ((uint32_t)got << 8) | (uint32_t)want); }
    }
    tally(R, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
static const char *kNames[] = {"div", "sqrt", "axis", "bounds", "convert", "chunks"};
constexpr int kSweeps = 6;

struct Result { unsigned long long visited = 0; Record rec = {}; float seconds = 0.f; };

struct Timer {
    hipEvent_t a, b;
    Timer() { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); HIP_OK(hipEventRecord(a, 0)); }
    float stop() { float ms = 0.f; HIP_OK(hipEventRecord(b, 0)); HIP_OK(hipEventSynchronize(b)); HIP_OK(hipEventElapsedTime(&ms, a, b)); (void)hipEventDestroy(a); (void)hipEventDestroy(b); return ms * 1e-3f; }
};
static Record *new_record() { Record *r; HIP_OK(hipMalloc(&r, sizeof(Record))); HIP_OK(hipMemset(r, 0, sizeof(Record))); return r; }
static Record take(Record *d) { Record h; HIP_OK(hipDeviceSynchronize()); HIP_OK(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost)); HIP_OK(hipFree(d)); return h; }
static unsigned blocks_for(unsigned long long n) { return (unsigned)((n + 255) / 256); }
constexpr unsigned kStrideBlocks = 1u << 16;                       // grid-stride sweeps: 2^24 threads

// the gradient's operand ranges, from the gate's named limits (vv_gate.h) and the march: sstep = |unit ray * step| lies within a few ulps of
// [min step, max step]; vd = i * sstep + dist lies in [sstep, kSqrt3 + 30 * sstep]; denominators are tan_fov * vd and sstep * 2
struct Ranges { double sstep_lo, sstep_hi, den_lo, den_hi; int derived_lo, derived_hi, lo, hi; double nmin; };
static std::vector<float> numerators()
{
    // every value q255[i] - q255[j], formed in binary32 as the kernel forms rr - l (q255[q] = (float)q / 255.f by IEEE division), each value once
    float q[256];
    for (int i = 0; i < 256; ++i) q[i] = (float)i / 255.f;
    std::vector<uint32_t> bits;
    for (int i = 0; i < 256; ++i) for (int j = 0; j < 256; ++j) { volatile float n = q[i] - q[j]; float v = n; uint32_t b; memcpy(&b, &v, 4); bits.push_back(b); }
    std::sort(bits.begin(), bits.end()); bits.erase(std::unique(bits.begin(), bits.end()), bits.end());
    std::vector<float> out(bits.size());
    for (size_t k = 0; k < bits.size(); ++k) memcpy(&out[k], &bits[k], 4);
    return out;
}
static Ranges ranges(const std::vector<float> &nums)
{
    Ranges r;
    const double few = 0x1p-20;                                    // 8 ulps
    r.sstep_lo = (double)kStepMin * (1.0 - few); r.sstep_hi = (double)kSafeDivStepMax * (1.0 + few);
    const double vd_lo = r.sstep_lo, vd_hi = (double)kSqrt3 + 30.0 * r.sstep_hi;
    r.den_lo = std::min((double)kSafeDivTanLo * vd_lo, 2.0 * r.sstep_lo);
    r.den_hi = std::max((double)kSafeDivTanHi * vd_hi, 2.0 * r.sstep_hi);
    r.derived_lo = ilogb(r.den_lo); r.derived_hi = ilogb(r.den_hi);
    r.nmin = 1.0;
    for (float n : nums) if (n != 0.f) r.nmin = std::min(r.nmin, (double)fabsf(n));
    // the kernel's comment states quotients in [2^-26, 2^42] (a superset of what the limits give): sweep the denominators of that range as well
    r.lo = std::min(r.derived_lo, ilogb(1.0 / 0x1p42)); r.hi = std::max(r.derived_hi, ilogb(r.nmin / 0x1p-26));
    return r;
}
static void guard(bool ok, const char *what) { if (!ok) { fprintf(stderr, "device_math_check: range guard failed: %s\n", what); exit(3); } }

template <int TWIN> static Result run_div()
{
    const std::vector<float> nums = numerators();
    const Ranges g = ranges(nums);
    guard(g.lo <= g.derived_lo && g.hi >= g.derived_hi, "swept binades contain the derived ones");
    guard(1.0 / ldexp(1.0, g.lo) >= 0x1p42 && g.nmin / ldexp(1.0, g.hi + 1) <= 0x1p-26, "swept quotients contain [2^-26, 2^42]");
    DenSpec S = {g.lo, g.hi};
    float *d_nums; HIP_OK(hipMalloc(&d_nums, nums.size() * 4)); HIP_OK(hipMemcpy(d_nums, nums.data(), nums.size() * 4, hipMemcpyHostToDevice));
    Record *R = new_record();
    Result out; Timer t;
    div_kernel<TWIN><<<blocks_for(den_count(S)), 256>>>(d_nums, (int)nums.size(), S, R);
    HIP_OK(hipGetLastError());
    out.seconds = t.stop(); out.rec = take(R); out.visited = den_count(S) * nums.size();
    HIP_OK(hipFree(d_nums));
    return out;
}
template <int TWIN> static Result run_sqrt(Result *inv)
{
    const std::vector<float> nums = numerators();
    const Ranges g = ranges(nums);
    const double qmin = g.nmin / g.den_hi, qmax = 1.0 / g.den_lo;   // the quotients the limits give; three of them, squared, are summed
    guard(qmin * qmin >= ldexp(1.0, kSqrtLo) && 3.0 * qmax * qmax * (1.0 + 0x1p-20) < ldexp(1.0, kSqrtHi + 1), "swept radicands contain the derived ones");
    guard(kSqrtLo <= -52 && kSqrtHi >= 86, "swept radicands contain [2^-52, 2^86]");
    Record *R = new_record(), *Ri = new_record();
    Result out; Timer t;
    sqrt_kernel<TWIN><<<kStrideBlocks, 256>>>(R, Ri);
    HIP_OK(hipGetLastError());
    out.seconds = t.stop(); out.rec = take(R); out.visited = kSqrtCount;
    Record ri = take(Ri);
    if (inv) { inv->rec = ri; inv->visited = kSqrtCount; }
    return out;
}
template <int TWIN> static Result run_axis()
{
    Record *R = new_record(); Result out; Timer t;
    const unsigned long long n = (unsigned long long)kUnitPatterns + kAxisExtras;
    axis_kernel<TWIN><<<blocks_for(n), 256>>>(R);
    HIP_OK(hipGetLastError());
    out.seconds = t.stop(); out.rec = take(R); out.visited = n * kAxisSizes * 2;
    return out;
}
template <int TWIN> static Result run_bounds()
{
    Record *R = new_record(); Result out; Timer t;
    bounds_kernel<TWIN><<<kStrideBlocks, 256>>>(R);
    HIP_OK(hipGetLastError());
    out.seconds = t.stop(); out.rec = take(R); out.visited = 3ull << 32;
    return out;
}
template <int TWIN> static Result run_convert()
{
    Record *R = new_record(); Result out; Timer t;
    convert_kernel<TWIN><<<kStrideBlocks, 256>>>(R);
    HIP_OK(hipGetLastError());
    out.seconds = t.stop(); out.rec = take(R); out.visited = 3ull << 32;
    return out;
}
template <int TWIN> static Result run_chunks()
{
    const Ranges g = ranges(numerators());
    ChunkSpec S = {(float)g.sstep_lo, (float)g.sstep_hi, (float)log2(g.sstep_lo), (float)log2(g.sstep_hi)};
    Record *R = new_record(); Result out; Timer t;
    chunks_kernel<TWIN><<<kStrideBlocks, 256>>>(S, R);
    HIP_OK(hipGetLastError());
    out.seconds = t.stop(); out.rec = take(R); out.visited = kChunkCount;
    return out;
}

static std::string first_json(const Record &r)
{
    std::string s = "[";
    const unsigned n = r.noted < 8u ? r.noted : 8u;
    char buf[96];
    for (unsigned k = 0; k < n; ++k) {
        snprintf(buf, sizeof buf, "%s[\"0x%08x\", \"0x%08x\", \"0x%08x\", \"0x%08x\"]", k ? ", " : "", r.ops[k][0], r.ops[k][1], r.ops[k][2], r.ops[k][3]);
        s += buf;
    }
    return s + "]";
}

int main(int argc, char **argv)
{
    bool self_test = false, want[kSweeps] = {}, any = false;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--list")) { for (const char *n : kNames) printf("%s\n", n); return 0; }
        if (!strcmp(argv[a], "--self-test")) { self_test = true; continue; }
        int k = 0;
        while (k < kSweeps && strcmp(argv[a], kNames[k])) ++k;
        if (k == kSweeps) { fprintf(stderr, "usage: device_math_check [--list] [--self-test] [div|sqrt|axis|bounds|convert|chunks ...]\n"); return 2; }
        want[k] = any = true;
    }
    int rc = 0;
    for (int k = 0; k < kSweeps; ++k) {
        if (any && !want[k]) continue;
        Result r, inv, twin, twin2;
        std::string extra;
        char buf[256];
        bool clean;
        switch (k) {
        case 0: {
            r = run_div<0>(); if (self_test) { twin = run_div<1>(); twin2 = run_div<2>(); }
            const std::vector<float> nums = numerators(); const Ranges g = ranges(nums);
            snprintf(buf, sizeof buf, ", \"numerators\": %zu, \"binade_lo\": %d, \"binade_hi\": %d, \"derived_lo\": %d, \"derived_hi\": %d, \"mantissas_per_binade\": %d",
                     nums.size(), g.lo, g.hi, g.derived_lo, g.derived_hi, 1 << 23);
            extra = buf;
            if (self_test) { snprintf(buf, sizeof buf, ", \"self_test_without_last_step\": %llu", twin2.rec.mismatches); extra += buf; }
            clean = r.rec.mismatches == 0; break; }
        case 1:
            r = run_sqrt<0>(&inv); if (self_test) { twin = run_sqrt<1>(nullptr); twin2 = run_sqrt<2>(nullptr); }
            snprintf(buf, sizeof buf, ", \"binade_lo\": %d, \"binade_hi\": %d, \"root_mismatches\": %llu, \"reciprocal_mismatches\": %llu, \"first_reciprocal\": ", kSqrtLo, kSqrtHi,
                     r.rec.mismatches, inv.rec.mismatches);
            extra = buf + first_json(inv.rec);
            if (self_test) { snprintf(buf, sizeof buf, ", \"self_test_without_lower_test\": %llu", twin2.rec.mismatches); extra += buf; }
            r.rec.mismatches += inv.rec.mismatches;
            clean = r.rec.mismatches == 0; break;
        case 2: r = run_axis<0>(); if (self_test) twin = run_axis<1>(); clean = r.rec.mismatches == 0; break;
        case 3: {
            r = run_bounds<0>(); if (self_test) twin = run_bounds<1>();
            // the set of disagreeing patterns must be exactly {0x80000000} (-0.0), once per coordinate
            bool seen[3] = {};
            clean = r.rec.mismatches == 3 && r.rec.noted == 3;
            for (unsigned m = 0; clean && m < 3; ++m) {
                if (r.rec.ops[m][0] != 0x80000000u || r.rec.ops[m][1] > 2u || seen[r.rec.ops[m][1]]) clean = false; else seen[r.rec.ops[m][1]] = true;
            }
            std::string set = "[";
            std::vector<uint32_t> pats;
            for (unsigned m = 0; m < std::min(r.rec.noted, 8u); ++m) pats.push_back(r.rec.ops[m][0]);
            std::sort(pats.begin(), pats.end()); pats.erase(std::unique(pats.begin(), pats.end()), pats.end());
            for (size_t m = 0; m < pats.size(); ++m) { snprintf(buf, sizeof buf, "%s\"0x%08x\"", m ? ", " : "", pats[m]); set += buf; }
            extra = ", \"disagreeing_patterns\": " + set + "]";
            break; }
        case 4: r = run_convert<0>(); if (self_test) twin = run_convert<1>(); clean = r.rec.mismatches == 0; break;
        default: r = run_chunks<0>(); if (self_test) twin = run_chunks<1>(); clean = r.rec.mismatches == 0; break;
        }
        if (!clean) rc = 1;
        std::string st;
        if (self_test) {
            snprintf(buf, sizeof buf, ", \"self_test_mismatches\": %llu, \"self_test_seconds\": %.3f", twin.rec.mismatches, twin.seconds);
            st = buf;
            if (twin.rec.mismatches == 0) rc = 1;                  // a sweep that cannot tell its wrong twin apart is a failing sweep
        }
        printf("{\"sweep\": \"%s\", \"visited\": %llu, \"mismatches\": %llu, \"first\": %s, \"seconds\": %.3f%s%s}\n", kNames[k], r.visited, r.rec.mismatches,
               first_json(r.rec).c_str(), r.seconds, extra.c_str(), st.c_str());
        fflush(stdout);
    }
    return rc;
}
