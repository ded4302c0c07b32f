// vv_kernels.h -- host-visible launch interface of the HIP kernels (internal).
#pragma once
#include <hip/hip_runtime.h>
#include "vv_device.h"
#include "vv_tiles.h"       // StripMap and the tile grid of the march kernels
#include "vv_fill.h"        // FillMap and the fill blocks of march_kernel

namespace vv {

static_assert(kFillSlab == kSlab, "vv_fill.h decides row ownership per slab row of vv_device.h (fill_writes restates row_owned)");

// the rectangle of a StripMap / SlabMap launch in pixels: [x0, x1) x [y0, y1).  Every owned pixel outside it is a pixel whose ray misses the volume: rad_kernel writes its 0,
// and computes no radius for slabs that do not meet the rectangle (march_kernel, which reads them, is not launched there).  No rectangle: x1 = y1 = INT_MAX.
struct PixelRect { int x0, x1, y0, y1; };

// blockIdx.x -> slab of a shard (march_phong_kernel)
struct SlabMap  { int r0, band, band_stride, n_regular;
                  // march_phong_kernel launches slab columns [gx0, gx0 + wg) of the grid rows [gs0, gs1) and the extra row n_regular (pin 10): the slabs under the
                  // volume's screen rectangle, or all of them (gx0 = 0, wg = nbx, gs0 = 0, gs1 = n_regular)
                  int gx0, wg, gs0, gs1; };

// the build of the march kernels a frame runs: vv_raymarch.hip, vv_mip.hip, vv_iso.hip and vv_proj.hip are each compiled once per build (vv_layout.h: kBuild)
// (the list generates the enum and the launcher table below, so their orders cannot part: MB_LINEAR_BIG volumes above 4 GiB, MB_BRICKED on VolumeView::bricks,
//  MB_BRICKED_CACHED the same for volumes up to 1 GiB, MB_ZPAIR on VolumeView::zpair, MB_ZFAST on VolumeView::zfast, MB_XPAIR on the x-pair copy, handed over in VolumeView::zpair)
#define VV_FOR_EACH_BUILD(X, K) X(K, MB_LINEAR) X(K, MB_LINEAR_BIG) X(K, MB_BRICKED) X(K, MB_BRICKED_CACHED) X(K, MB_ZPAIR) X(K, MB_ZFAST) X(K, MB_XPAIR)
#define VV_X(K, B) B,
enum MarchBuild : uint8_t { VV_FOR_EACH_BUILD(VV_X, ) MB_COUNT };
#undef VV_X

// what a frame keeps of its samples: their composite (vv_render), their maximum (vv_render_mip), the first at or above a level (vv_render_iso) or the
// maximum / minimum / mean of those inside the volume (vv_render_projection).  One kernel file per kind (vv_raymarch.hip, vv_mip.hip, vv_iso.hip, vv_proj.hip).
// The values are vv_debug_last_launch's kernel family of the three unshaded-only kinds (composite frames report 0 or 1 with the shading); the list
// generates the rows of the launcher table, which frame_row() finds.
enum FrameKind { FRAME_COMPOSITE = 0, FRAME_MIP = 2, FRAME_ISO = 3, FRAME_PROJ = 4 };
#define VV_FOR_EACH_KIND(X) X(FRAME_COMPOSITE) X(FRAME_MIP) X(FRAME_ISO) X(FRAME_PROJ)
#define VV_X(K) K,
constexpr FrameKind kFrameKinds[] = { VV_FOR_EACH_KIND(VV_X) };
#undef VV_X
constexpr int kFrameKindCount = sizeof(kFrameKinds) / sizeof(kFrameKinds[0]);
constexpr int frame_row(FrameKind k) { int r = 0; while (r < kFrameKindCount - 1 && kFrameKinds[r] != k) ++r; return r; }

// what an isosurface frame knows beyond FrameParams / VolumeView (iso_kernel): the level, and the gradient's offsets h[a] = 1 / n_a in texture
// coordinates with n[a] = (float)n_a, the volume's dimensions
struct IsoParams { int level; float h[3]; float n[3]; };

struct MarchArgs {
    FrameParams P;
    VolumeView  V;
    int V_type;                 // vv_voxel_type
    bool tex8, gray, phong, instr;
    MarchBuild build;           // vv_render's choice (MB_XPAIR: VolumeView::zpair holds the x-pair copy)
    int lds_reserve;            // march_kernel: dynamic LDS bytes reserved only to cap blocks per CU
    int unroll;                 // march_kernel: samples per loop trip (2 or 3)
    int lds_reserve_phong;      // march_phong_kernel: same occupancy cap (its own LDS is 14 KB)
    StripMap strips;                   // march_kernel: strips of 8 pixel rows (n_strips of them)
    PixelRect rect;                    // rad_kernel + march kernels: the pixels the march kernel's tiles / slabs cover
    bool fill_outside;                 // Phong frames: rad_kernel is launched (without radii) to write the pixels outside `rect`
    uint32_t *order_out;               // rad_kernel: where its extra block writes StripMap::order (nullptr: no such block)
    SlabMap slabs;                     // march_phong_kernel grid.y = n_regular + 1
    const float4 *tf;           // device, 256 entries
    const float *rad;           // device, nbx*nby (read by march_kernel)
    float *rad_out;             // same buffer (written by rad_kernel)
    const float4 *fill_tf;      // fill_outside_kernel: the table whose entry 0 is the RGBA of the pixels beside the rectangle, or null for RGBA 0 (isosurface frames)
    uint32_t *pixels;           // device RGBA8 frame (MIP frames: may be null)
    uint32_t *rad_pixels;       // rad_kernel: `pixels` where it writes the zeros beside `rect`, null where it has none to write or march_kernel's fill blocks write them
    FillMap fill;               // march_kernel: the fill blocks behind its marching blocks (vv_fill.h; `first` is the launcher's to set)
    int fill_blocks;            // how many of them (0: none)
    uint8_t *index;             // MIP frames: device image of the per-pixel maxima, W * H bytes, or null (isosurface frames: of the hits' indices)
    float4 *hit;                // isosurface frames: device image of the hit records (x, y, z, ordinal), W * H * 16 bytes, or null
    IsoParams iso;              // isosurface frames
    uint2 *stat;                // projection frames: device image of the records {ord, n} / {s, n}, W * H * 8 bytes, or null
    int proj_mode;              // projection frames: vv_proj_mode
    unsigned long long *counter;
    InstrArgs I;                // bitmaps of an instrumented frame (vv_render_options::touched_bricks / touched_lines)
};

// The launchers: one explicit specialisation per frame kind and build, each defined by the kind's kernel file compiled for that build;
// kLaunch[frame_row(k)][b] is the launcher of FrameKind k and MarchBuild b.  The kernels that exist once live in the linear build's units: rad_kernel
// (the pre-pass of all four kinds) in vv_raymarch.hip, fill_outside_kernel and mip_classify_kernel in vv_mip.hip.
template <int KIND, MarchBuild B> void launch_frame(const MarchArgs &a, hipStream_t s);
#define VV_X(K, B) template <> void launch_frame<K, B>(const MarchArgs &, hipStream_t);
#define VV_ROW(K) VV_FOR_EACH_BUILD(VV_X, K)
VV_FOR_EACH_KIND(VV_ROW)
#undef VV_ROW
#undef VV_X
using MarchLauncher = void (*)(const MarchArgs &, hipStream_t);
#define VV_X(K, B) launch_frame<K, B>,
#define VV_ROW(K) { VV_FOR_EACH_BUILD(VV_X, K) },
constexpr MarchLauncher kLaunch[][MB_COUNT] = { VV_FOR_EACH_KIND(VV_ROW) };
#undef VV_ROW
#undef VV_X
static_assert(sizeof(kLaunch) == sizeof(MarchLauncher) * kFrameKindCount * MB_COUNT, "one launcher per frame kind and build");
void launch_rad(const MarchArgs &a, hipStream_t s);
constexpr int kMipTableBytes = 4096;      // march_kernel's LDS table, which the reducer kernels (mip, iso, proj) do not have (vv_layout.h: reducer_lds)
// the owned pixels outside `rect` of a MIP, isosurface or projection frame, whose rays miss the volume: index 0, RGBA of MarchArgs::fill_tf, zero records
void launch_fill(const MarchArgs &a, const PixelRect &rect, hipStream_t s);
void launch_mip_classify(const uint8_t *index, size_t n, const float4 *tf, uint32_t *pixels, hipStream_t s);   // pixels[i] = RGBA8 of tf[index[i]]
void launch_build_xpair(int vtype, const void *zfast, uint32_t zf_row_bytes, uint64_t zf_slice_bytes, void *xpair, int nx, int ny, int nz, hipStream_t s);
void launch_build_zfast(int vtype, const void *vol, uint32_t row_pitch, uint64_t slice_pitch, void *out, uint32_t zf_row_bytes, uint64_t zf_slice_bytes, int nx, int ny, int nz, hipStream_t s);
size_t zpair_copy_bytes(int vtype, int nx, int ny, int nz, uint32_t *row_bytes, uint32_t *slab_bytes);
void launch_build_zpair(int vtype, const void *linear, size_t row_pitch, size_t slice_pitch, void *zpair, int nx, int ny, int nz, hipStream_t s);
void launch_repitch(const void *dense, void *pitched, size_t row_bytes /* multiple of 16 */, size_t ny, size_t nz,
                    size_t row_pitch, size_t slice_pitch, hipStream_t s);
size_t brick_copy_bytes(int vtype, int nx, int ny, int nz, uint32_t *sy, uint32_t *sz64);
void launch_build_bricks(int vtype, const void *linear, size_t row_pitch, size_t slice_pitch, void *bricks, int nx, int ny, int nz, hipStream_t s);
struct SliceArgs {
    VolumeView V; int V_type; bool tex8;
    float *buffer; size_t height, width;
    float dx, dy, dz; int orientation; int legacy;
    float scale[3];
    float trans[16]; int advanced;
};
void launch_slice(const SliceArgs &a, hipStream_t s);
// thick-slab slices (vv_slab.hip): SliceArgs' view, image and position fields without the legacy form, the slab (vv_slab of include/volviz.h) and the
// second image: aux[offset] = the extremum's sample (MAX / MIN) or the number of executed samples (MEAN), or null
struct SlabArgs {
    VolumeView V; int V_type; bool tex8;
    float *buffer; int32_t *aux; size_t height, width;
    float dx, dy, dz; int orientation;
    float scale[3];
    float trans[16]; int advanced;
    int mode, samples; float thickness;
};
void launch_slab(const SlabArgs &a, hipStream_t s);
// histograms (vv_hist.hip).  What is counted is a set of equally long contiguous runs of voxels: run (ry, rz), 0 <= ry < rps, 0 <= rz < n_slices, starts at
// data0 + rz * slice_step + ry * row_step bytes and holds run_voxels voxels (a box of the volume: its rows, or whole slices / the whole box where the
// rows are dense; an index image: one run of u8).  The caller vouches that every run lies inside one allocation that starts 16-byte aligned and, unless
// `tight`, extends 16 bytes beyond the last run; with `tight` no byte outside the runs is read.
struct HistRuns {
    const void *data0; int vtype; int tight;
    uint64_t run_voxels, row_step, slice_step;
    uint32_t rps, n_slices;
};
// the accumulator: 256 counts, the NaN count, and two uint32 in one word: the largest key and the largest complemented key of the non-NaN f32 voxels.
// All zeros before launch_hist (zero keys = no voxel yet).
constexpr int kHistAccNan = 256, kHistAccKeys = 257, kHistAccWords = 258;
void launch_hist(const HistRuns &r, int n_cu, int max_blocks /* <= 0: kHistBlocksPerCU per CU */, unsigned long long *acc, hipStream_t s);
void launch_hist_finish(const unsigned long long *acc, int vtype, unsigned long long voxels, vv_histogram *out, unsigned long long *counts /* used when out is null */,
                        hipStream_t s);
// derived volumes (vv_derive.hip): a box of the linear volume reduced cell by cell into a dense volume at `out` (vv_derive of include/volviz.h, checked by
// the caller).  src0: the box's first voxel; b / f / m: the box's extents, the factors (1..8) and the output's extents in voxels (x, y, z),
// m = ceil(b / f).  The caller vouches that the box lies inside one allocation that extends `slack` bytes beyond the box's last voxel (vector loads
// are taken only where they are aligned and stay inside it), and that `out` holds m[0] * m[1] * m[2] voxels of out_type.
struct DeriveArgs {
    const void *src0; void *out;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    uint32_t b[3], f[3], m[3];
    int src_type, out_type, mode, window;   // vv_voxel_type (2 x), vv_reduce_mode, 0 / 1
    float win_lo, win_hi;
    uint64_t slack;
};
void launch_derive(const DeriveArgs &a, int n_cu, int max_blocks /* <= 0: a CU's full complement of waves per CU */, hipStream_t s);
// neighbourhood filters (vv_stencil.hip): a box of the linear volume filtered into a dense volume of the box's extents at `out` (vv_stencil of
// include/volviz.h, checked by the caller: radii 0..VV_STENCIL_MAX_RADIUS, gscale resolved).  vol: the volume's first voxel; n: its extents;
// lo / b: the box's low corner and extents in voxels (x, y, z).  Every voxel a stencil reaches is addressed by coordinates clamped to n: the
// caller vouches that the n[0] x n[1] x n[2] voxels at the two pitches lie inside one allocation and that `out` holds b[0] * b[1] * b[2] voxels of
// out_type outside it.
struct StencilArgs {
    const void *vol; void *out;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    int32_t n[3], lo[3];
    uint32_t b[3];
    int src_type, out_type, kind;           // vv_voxel_type (2 x), vv_stencil_kind
    int radius[3];
    float taps[3][5];
    float gscale[3];
};
void launch_stencil(const StencilArgs &a, int n_cu, int max_blocks /* <= 0: one block per (tile, z segment) */, hipStream_t s);
// resampled volumes (vv_resample.hip): the box lo / b (voxels, x, y, z) of an output grid sampled from the linear volume V into a dense volume of
// the box's extents at `out` (vv_resample of include/volviz.h, checked by the caller).  inv[a] = 1.0f / (float)dims[a] of the grid; m, fill,
// filter: the descriptor's.  The caller vouches that V is the linear layout as slice_kernel takes it (its padding behind the last slice
// included) and that `out` holds b[0] * b[1] * b[2] voxels of out_type outside it.
struct ResampleArgs {
    VolumeView V; void *out;
    int src_type, out_type, filter;         // vv_voxel_type (2 x), vv_resample_filter
    int32_t lo[3];
    uint32_t b[3];
    float inv[3], m[12], fill;
};
void launch_resample(const ResampleArgs &a, int n_cu, int max_blocks /* <= 0: one block per tile */, hipStream_t s);
// segmentation (vv_label.hip).  launch_label: the connected components of the box of b[0] x b[1] x b[2] voxels whose first voxel is src0 (vv_label of
// include/volviz.h, checked by the caller) as labels, x fastest, at `labels`; with `sizes` the components' voxel counts at their least voxels; with
// `stats` a vv_label_stats.  counters: kLabelCounters words, all zero before the launch (the kernels' accumulators).  The caller vouches that the box
// lies inside one allocation (f32: src0 and both pitches 4-byte aligned), that it holds at most 2^32 - 2 voxels and that labels / sizes hold as many
// words outside it and outside each other.  Three launches, and one or two more with `stats`.
constexpr int kLabelForeground = 0, kLabelComponents = 1, kLabelLargest = 2, kLabelCounters = 4;
struct LabelArgs {
    const void *src0; uint32_t *labels, *sizes; vv_label_stats *stats;
    unsigned long long *counters;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    uint32_t b[3];
    uint32_t bin_lo, bin_hi;
    int src_type, connectivity;             // vv_voxel_type; 6, 18 or 26
};
void launch_label(const LabelArgs &a, int n_cu, int max_blocks /* <= 0: one block per tile, a CU's complement of waves for the elementwise kernels */,
                  int phases /* 1..3: stop behind that launch (timing aid); anything else: all */, hipStream_t s);
// launch_mask: out[i] = the box's voxel i through the copy stage where the test on labels[i] holds (vv_mask of include/volviz.h, checked by the
// caller), `fill` through the arithmetic output stage elsewhere.  labels / sizes: b[0] * b[1] * b[2] words each (sizes may be null unless keep is
// VV_KEEP_MIN_SIZE), whatever they hold.
struct MaskArgs {
    const void *src0; const uint32_t *labels, *sizes; void *out;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    uint32_t b[3];
    int src_type, out_type, keep, invert;   // vv_voxel_type (2 x), vv_keep, 0 / 1
    uint32_t label, min_size;
    float fill;
};
void launch_mask(const MaskArgs &a, int n_cu, int max_blocks, hipStream_t s);
// distance transform (vv_distance.hip).  launch_distance: the squared Euclidean distance of every voxel of the box of b[0] x b[1] x b[2] voxels to the
// nearest seed (vv_distance of include/volviz.h, checked by the caller), x fastest, at `out`; three launches, in place on `out`.  The caller vouches
// for what launch_label's caller does, that every extent is at most VV_DISTANCE_MAX_EXTENT, that sum_a (spacing[a] (b[a] - 1))^2 <= 0xFFFFFFFE, and
// that `labels` (the labels sources) holds b[0] * b[1] * b[2] words and is `out` itself or lies outside it.
struct DistanceArgs {
    const void *src0; const uint32_t *labels; uint32_t *out;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    uint32_t b[3], spacing[3];
    uint32_t bin_lo, bin_hi, label, within_r2;
    int src_type, seed, invert, mode;       // vv_voxel_type, vv_seed, 0 / 1, vv_dist_out
};
void launch_distance(const DistanceArgs &a, int n_cu, int max_blocks /* <= 0: a block per four rows / per tile of lines */,
                     int phases /* 1, 2: stop behind that launch (timing aid); anything else: all three */, hipStream_t s);
// region measurements (vv_region.hip).  launch_region: the regions of `labels` (vv_regions of include/volviz.h, checked by the caller) ranked, relabelled
// 1..K at `compact` and measured into `table` (max_regions rows; null with 0), with `summary` a vv_region_summary.  hdr: kRegionHeader words, all zero
// before the launch; partials: kRegionMaxChunks words, whatever they hold.  The caller vouches for what launch_mask's caller does, that labels, aux (or
// null) and compact hold b[0] * b[1] * b[2] words each, compact outside everything else, and that table and summary are 8-byte aligned.  Five launches.
constexpr int kRegionForeground = 0, kRegionStray = 1, kRegionCount = 2, kRegionFirst = 3, kRegionHeader = 4;
constexpr int kRegionMaxChunks = 8192;      // the cap on the chunks of a call: the partials of scratch entry SC_REGION
constexpr int kRegionMinChunk = 1024;       // voxels; tests/test_regions.py names it CHUNK
struct RegionArgs {
    const void *src0; const uint32_t *labels, *aux; uint32_t *compact; vv_region *table; vv_region_summary *summary;
    unsigned long long *hdr; uint32_t *partials;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    uint32_t b[3]; int32_t lo[3];           // the box's extents and its origin in the volume
    uint32_t max_regions;
    int src_type, source;                   // vv_voxel_type, vv_region_source
};
void launch_region(const RegionArgs &a, int max_blocks /* <= 0: a block per kRgWaves chunks */, int max_chunks /* <= 0: kRegionMaxChunks */,
                   int phases /* 1..4: stop behind that launch (timing aid); anything else: all five */, hipStream_t s);
// surface meshes (vv_mesh.hip).  launch_mesh: the surface-nets mesh of the box of b[0] x b[1] x b[2] voxels whose first voxel is src0 (vv_mesh of
// include/volviz.h, checked by the caller): `index` (one word per site of the m[0] x m[1] x m[2] grid, m[a] = b[a] - 1 + 2 cap), the vertex and
// normal records of rank < max_vertices, the quad records of rank < max_quads, with `summary` a vv_mesh_summary.  index == nullptr: a count-only call
// (both maxima 0), two launches; else four.  hdr: kMeshHeader words and partials: kMeshMaxChunks pairs, whatever they hold.  The caller vouches for what
// launch_mask's caller does, that the site grid holds at most 2^32 - 2 sites, that `labels` (the labels sources) holds b[0] * b[1] * b[2] words, that
// index holds a word per site, vertices / normals max_vertices and quads max_quads 16-byte aligned records, all outside each other and the inputs.
constexpr int kMeshVertices = 0, kMeshQuads = 1, kMeshHeader = 4;
constexpr int kMeshMaxChunks = 8192;        // the cap on the chunks of a call: the partials of scratch entry SC_MESH
constexpr int kMeshMinChunk = 1024;         // sites; tests/test_mesh.py names it CHUNK
struct MeshPartial { unsigned long long vertices, quads; };      // of a chunk (launch 1); of all chunks below it (behind launch 2)
struct MeshArgs {
    const void *src0; const uint32_t *labels; uint32_t *index; vv_mesh_vertex *vertices; vv_mesh_normal *normals; uint4 *quads; vv_mesh_summary *summary;
    unsigned long long *hdr; MeshPartial *partials;
    uint64_t row_pitch, slice_pitch;        // of the source, bytes
    uint32_t b[3], m[3]; int32_t lo[3];     // the box's extents, the site grid's, the box's origin in the volume
    uint32_t level, bin_lo, bin_hi, label;  // level: 1 for the three binary sources
    uint32_t max_vertices, max_quads;
    int src_type, source, cap;              // vv_voxel_type, vv_mesh_source, 0 / 1
};
void launch_mesh(const MeshArgs &a, int max_blocks /* <= 0: a block per kMeshWaves chunks */, int max_chunks /* <= 0: kMeshMaxChunks */,
                 int phases /* 1..3: stop behind that launch (timing aid); anything else: all */, hipStream_t s);
void launch_first_pass(const FrameParams &P, uint32_t *front, uint32_t *back, hipStream_t s);

size_t generate_scratch_floats(int nx, int ny, int nz, int n);
void launch_generate_ellipsoids(uint8_t *out, int nx, int ny, int nz, int n,
                                const float *centers, const float *axes, const uint8_t *colors,
                                int in_place, float *scratch /* generate_scratch_floats() device floats */, hipStream_t s);
void launch_promote_u8_f32(const uint8_t *in, float *out, size_t n, hipStream_t s);
void launch_noise_u8(uint8_t *out, int nx, int ny, int nz, uint32_t seed, hipStream_t s);

constexpr int kMaxEllipsoids = 64;

} // namespace vv
