/*
 * volviz.h -- C-ABI boundary of the MI355X-native volume ray-marcher.
 *
 * This header is what a host application (the reference's glwidget.cpp /
 * slicewidget.cpp, or any FFI) binds instead of the reference's kernel.cuh.
 * Every entry point cites the reference interface it replaces.  All types are
 * plain C: pointers, sizes, PODs.  No torch / HIP types appear in signatures
 * (a stream is passed as an opaque void* that is a hipStream_t; NULL = the
 * default stream).
 *
 * Conventions
 *   - every function returns VV_OK (0) or a negative vv_status; it never calls
 *     exit() (the reference's checkCudaErrors does: include/helper_cuda.h:763-777);
 *     vv_last_error() returns the text for the last failure on the context.
 *   - calls are synchronous from the caller's view unless a stream is passed
 *     AND the output buffer is device memory, in which case the work is only
 *     enqueued on that stream (reference contract: kernel.cu:452,517 fence each call).
 *   - a context owns one volume, one transfer function, scratch buffers
 *     (reference: file-static globals, kernel.cu:35-51).  Not re-entrant.
 *   - volume layout: u8 or f32, x fastest, then y, then z (kernel.cu:477,
 *     volumegenerator.cpp:41).
 *   - output image: RGBA u8, row-major, row 0 = bottom (GL), W*H*4 bytes
 *     (glwidget.cpp:365-369, kernel.cu:365).
 */
#ifndef VOLVIZ_H
#define VOLVIZ_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference PODs, byte-identical to kernel.cuh:18-40 ------------------- */
#ifndef SLICE_NONE
#define SLICE_NONE      -1   /* kernel.cuh:18 */
#define SLICE_PLANE      0   /* kernel.cuh:19 */
#define SLICE_PLANE_CUT  1   /* kernel.cuh:20 */
#endif
#ifndef TRANSFER_PRESET_DEFAULT
#define TRANSFER_PRESET_DEFAULT -1  /* kernel.cuh:22 */
#define TRANSFER_PRESET_ENGINE   0  /* kernel.cuh:23 */
#define TRANSFER_PRESET_MRI      1  /* kernel.cuh:24 */
#endif

struct slice_params {        /* kernel.cuh:26-29 */
    int   type;              /* SLICE_NONE / SLICE_PLANE / SLICE_PLANE_CUT */
    float params[6];         /* plane point xyz, plane normal xyz (cube space) */
};

struct camera_params {       /* kernel.cuh:31-35 */
    float origin[3];         /* world-space eye (glwidget.cpp:271-273) */
    float fovX, fovY;        /* degrees; fovX = fovY*aspect (glwidget.cpp:340-341) */
    float scale[3];          /* object scale (glwidget.cpp:267-269) */
};

struct shading_params {      /* kernel.cuh:37-40 */
    int  transferPreset;     /* carried, never read by the kernel (as in the reference) */
    bool phongShading;
};

/* params.h:46 canonicalOrientation, same enumerator values */
typedef enum {
    VV_HORIZONTAL = 0, VV_SAGITTAL = 1, VV_CORONAL = 2,
    VV_N_CANONICAL_ORIENTATIONS = 3, VV_FREE_FORM = 4
} vv_orientation;

/* ---- status ----------------------------------------------------------------- */
typedef enum {
    VV_OK = 0,
    VV_ERR_INVALID = -1,     /* bad argument */
    VV_ERR_NO_VOLUME = -2,   /* render/slice before a volume was loaded */
    VV_ERR_DEVICE = -3,      /* HIP runtime error */
    VV_ERR_NOMEM = -4,
    VV_ERR_IO = -5
} vv_status;

typedef struct vv_context vv_context;

/* The `stream` argument of the entry points below is a hipStream_t passed as void*:
 *   NULL                     the context's own stream; the call returns when the work is complete (the reference's
 *                            synchronous contract, kernel.cu:452,517);
 *   VV_STREAM_DEFAULT_ASYNC  the device's default (null) stream, enqueue only;
 *   any other handle         that stream, enqueue only: the caller synchronises.                                  */
#define VV_STREAM_DEFAULT_ASYNC ((void *)1)

typedef enum { VV_VOXEL_U8 = 0, VV_VOXEL_F32 = 1 } vv_voxel_type;

/* Trilinear reconstruction model (what tex3D does in kernel.cu:102,589,628).
 *   VV_FILTER_TEX8  : CUDA texture-unit model -- interpolation weights rounded
 *                     to 8 fractional bits (1.8 fixed point).  Default.
 *   VV_FILTER_EXACT : full float weights.                                     */
typedef enum { VV_FILTER_TEX8 = 0, VV_FILTER_EXACT = 1 } vv_filter;

/* Early-ray termination.
 *   VV_ERT_REFERENCE : the reference's behaviour -- `break` leaves only the
 *                      30-sample inner loop (kernel.cu:272-274); every later
 *                      chunk still composites its first sample.  Default.
 *   VV_ERT_TRUE      : the ray stops for good once alpha > threshold.          */
typedef enum { VV_ERT_REFERENCE = 0, VV_ERT_TRUE = 1 } vv_ert_mode;

/* Where front/back ray end points come from (first-pass contract,
 * firstpass.vert:6, glwidget.cpp:198-228).                                    */
typedef enum {
    VV_RAYS_IMAGES = 0,   /* two RGBA8 images = the reference's FBO0/FBO1        */
    VV_RAYS_ANALYTIC = 1  /* ray/box intersection computed from the camera       */
} vv_ray_mode;

typedef struct vv_ray_source {
    int            mode;             /* vv_ray_mode */
    /* VV_RAYS_IMAGES: RGBA8, row 0 = bottom, sampled at (x/W, y/H) with point
     * filtering exactly like tex2D(inTexture0, ..) in kernel.cu:317-318.      */
    const uint8_t *front;            /* img_w*img_h*4 bytes */
    const uint8_t *back;
    int            img_w, img_h;     /* FBO size (reference: widget size = 3x the render size) */
    int            images_on_device; /* 0 = host pointers, 1 = device pointers */
    /* VV_RAYS_ANALYTIC: camera basis (camera.cpp:78-91); eye = camera_params.origin,
     * projection = perspective(fovY, aspect) as glwidget.cpp:338.
     * VV_RAYS_IMAGES: optional HINT (speed only, pixels never depend on it): the camera that drew the
     * images, if the host knows it (glwidget.cpp:188-228 draws them from `camera`).  With a hint vv_render
     * chooses wave tiles, volume layout and occupancy as for analytic rays; without one it estimates the
     * view from the images' centre row (host images; device images only in synchronous calls, which may
     * read them back) and otherwise launches conservatively.  Leave look / up zero for "no hint": ZERO-INITIALISE this struct -- stale
     * values in look / up of an image source are read as a camera and pick tile shape, layout (possibly building a copy of the volume)
     * and occupancy from it; a non-finite or degenerate hint is ignored.  Device images must be 4-byte aligned (VV_ERR_INVALID otherwise). */
    float          look[3];
    float          up[3];
    float          aspect;           /* <= 0 : use W/H */
    int            quantize8;        /* 1 = round end points to RGBA8 like the FBO does */
} vv_ray_source;

typedef struct vv_render_options {
    float    step[3];        /* per-axis step; all 0 => 1/dims (kernel.cu:415)   */
    float    ert_threshold;  /* 0 => .95f (kernel.cu:272)                        */
    int      filter;         /* vv_filter                                        */
    int      ert_mode;       /* vv_ert_mode                                      */
    /* Screen-tile sharding (multi-GPU).  A pixel row y belongs to slab row r = y/14 of the
     * global 14x14 slab grid (kernel.cu:418); this call renders the rows whose r satisfies
     *   begin <= r < end   (0,0 => all)   and   (r / shard_band) % shard_count == shard_index
     * Other rows are left untouched.  shard_count <= 1 disables the interleave;
     * shard_band must be a multiple of 4 slab rows when shard_count > 1.              */
    int      slab_row_begin;
    int      slab_row_end;
    int      shard_band;     /* slab rows per interleave band (e.g. 4 = 56 pixel rows)  */
    int      shard_count;    /* number of shards (ranks)                                */
    int      shard_index;    /* this shard                                               */
    int      count_samples;  /* 1 => count executed samples (vv_last_sample_count)*/
    uint32_t *touched_bricks;/* device bitmap, 1 bit per 8^3 brick, or NULL:     */
                             /* instrumentation for the roofline's byte model    */
    /* The same at the granularity the memory system fetches at: 1 bit per 128-byte line of the LAYOUT THE FRAME SAMPLES (bit = byte offset
     * from that layout's base / 128; vv_device_bytes() bounds the size: the largest resident layout), or NULL.  touched_lines_all = 0 marks
     * the lines of executed in-volume samples (what must be fetched at least once), 1 the lines of every gather the kernel issues.      */
    uint32_t *touched_lines;
    unsigned long long touched_line_bits;   /* size of touched_lines in bits */
    int      touched_lines_all;
    /* ... and per block: a zero-initialised device hash set of 2^log2 64-bit words that receives one entry per (thread block, line) pair
     * under the same rule (count the non-zero words afterwards): the bytes the frame fetches if blocks share nothing.  Size it at
     * >= 2 x the pairs expected.  NULL = off. */
    unsigned long long *touched_block_lines;
    int      touched_block_lines_log2;
} vv_render_options;

/* ---- lifecycle ---------------------------------------------------------------- */
/* replaces initCuda() (kernel.cuh:44, kernel.cu:369-373).  device < 0 => current device. */
int  vv_init(int device, vv_context **out_ctx);
int  vv_shutdown(vv_context *ctx);
const char *vv_last_error(const vv_context *ctx);   /* ctx may be NULL (global error) */

/* ---- volume + transfer function: replaces cudaLoadVolume (kernel.cuh:53, kernel.cu:456-498).
 * texels: host pointer, nx*ny*nz voxels, x fastest.  tf: 256 RGBA float entries.
 * Reloading frees the previous volume (the reference leaks it).
 *
 * Value domain of f32 voxels (every call below that takes or produces VV_VOXEL_F32 data: vv_load_volume_f32,
 * vv_load_volume_device, the vv_load_volume_stream_* calls, vv_load_volume_t3d): finite, |v| <= 2^126.  Inside it every
 * difference the trilinear lerps form is finite, so the weight-0 corner the kernels fetch beside an edge texel contributes
 * exactly nothing and results do not depend on the layout (bit-exact, tests/test_witness.py).  The library does not scan
 * the volume.  An out-of-domain voxel (Inf, NaN, |v| > 2^126) makes unspecified the samples that lie within one voxel of
 * it and, on the linear layouts, the samples in the outer half-voxel shell of the row or slice that ends just before it in
 * memory; no other sample is affected, and no access leaves the allocation: addresses come from coordinates, never
 * from voxel values.                                                            */
int  vv_load_volume_u8 (vv_context *ctx, const uint8_t *texels, size_t size,
                        int nx, int ny, int nz, const float tf[1024]);
int  vv_load_volume_f32(vv_context *ctx, const float *texels, size_t size,
                        int nx, int ny, int nz, const float tf[1024]);
/* Same, from a buffer already resident in HBM (e.g. written by vv_generate_*); f32 voxels: the value domain above. */
int  vv_load_volume_device(vv_context *ctx, const void *dev_texels, int voxel_type,
                           int nx, int ny, int nz, const float tf[1024], void *stream);
int  vv_set_transfer_function(vv_context *ctx, const float tf[1024]);

/* Streamed upload for volumes that should not sit in host memory whole (config C5: 2048^3
 * streamed from pinned host memory).  begin allocates the device volume; each slices call
 * enqueues slices [z0, z0+n) on an internal copy stream (directly if `src` is pinned host
 * memory, through a pinned double buffer otherwise) and returns; src_type may be VV_VOXEL_U8
 * while the volume is VV_VOXEL_F32, in which case the slices are promoted (v/255) on the
 * device.  end waits for the copies.  Slices may arrive in any order.  A slices call returns once the source
 * buffer has been read (pinned sources are copied from directly), so the caller may refill it at once.
 * f32 slices: the value domain above (promoted u8 slices are inside it by construction).                            */
int  vv_load_volume_stream_begin(vv_context *ctx, int voxel_type, int nx, int ny, int nz,
                                 const float tf[1024]);
int  vv_load_volume_stream_slices(vv_context *ctx, const void *src, int src_type, int z0, int nslices);
/* The same in two halves, for a host that feeds several contexts from one pinned buffer (volviz_mgpu) or wants to
 * overlap its own work with the transfer: _async only enqueues (H2D copy, then the promotion kernel on a second
 * stream), _wait_source returns when the copy engine has read every pinned source handed over so far -- the buffer may
 * then be refilled; promotion kernels may still be running (stream_end waits for them).
 * vv_load_volume_stream_slices == _async followed by _wait_source. */
int  vv_load_volume_stream_slices_async(vv_context *ctx, const void *src, int src_type, int z0, int nslices);
int  vv_load_volume_stream_wait_source(vv_context *ctx);
int  vv_load_volume_stream_end(vv_context *ctx);
/* .t3d file -> device volume in chunks (never holds the file in memory); voxel_type F32 promotes (v/255: inside the
 * f32 value domain above). */
int  vv_load_volume_t3d(vv_context *ctx, const char *path, int header, int voxel_type,
                        const float tf[1024]);

/* ---- ray march: replaces runCuda (kernel.cuh:46-51, kernel.cu:388-453) ----------
 * rgba_out: W*H*4 bytes; out_on_device selects host or device pointer.
 * Pixels the reference never writes (column W-1, row H-1) are left untouched.   */
int  vv_render(vv_context *ctx, int width, int height,
               const struct slice_params *slice,
               const struct camera_params *camera,
               const struct shading_params *shading,
               const vv_ray_source *rays,
               const vv_render_options *opts,     /* NULL => reference defaults */
               uint8_t *rgba_out, int out_on_device, void *stream);

/* ---- maximum-intensity projection (no reference counterpart: the reference only composites) ----------------------------------
 * A MIP frame marches exactly the rays and samples of an unshaded vv_render frame in which no ray ever crosses the early-termination
 * threshold: same end points, per-slab radius, cut plane (SLICE_PLANE_CUT; SLICE_PLANE marches as SLICE_NONE: its highlight is a
 * compositing effect), 30-sample chunks, step, object scale, filter and 8-bit classification index.  opts->ert_threshold and
 * opts->ert_mode are ignored.  Per pixel, M = the largest index over the executed samples, 0 when none is executed (a ray that misses
 * the volume, the cut plane's early return).
 *   index_out : W*H bytes, row 0 = bottom, holding M                                       (or NULL)
 *   rgba_out  : W*H*4 bytes; channel c = (uint8)(clamp(tf[M][c], 0, 1) * 255), the conversion vv_render applies to its sums, for every
 *               pixel the frame writes, M = 0 included                                      (or NULL; at least one of the two)
 * Column W-1, row H-1 and the rows of other shards (slab_row_begin / _end, shard_*) stay untouched in both images; count_samples and the
 * touched_* instruments work as in vv_render, as do `stream`, out_on_device (both images), the layout policy of vv_set_layout_policy,
 * vv_last_frame_ms, vv_last_sample_count and vv_debug_last_launch.  The context's state (volume, table, copies) is not changed.   */
int  vv_render_mip(vv_context *ctx, int width, int height,
                   const struct slice_params *slice,
                   const struct camera_params *camera,
                   const vv_ray_source *rays,
                   const vv_render_options *opts,     /* NULL => defaults */
                   uint8_t *rgba_out, uint8_t *index_out, int out_on_device, void *stream);
/* The same conversion over an index image of n bytes (one vv_render_mip wrote, or any other): rgba_out[i] = RGBA8 of tf[index[i]].
 * tf: 256 RGBA float entries in host memory, finite, or NULL = the context's table.  index and rgba_out (n*4 bytes, 4-byte aligned) are
 * both host or both device pointers (on_device).  Needs no volume: after a table edit a 2-megapixel look-up replaces a march of the
 * volume.  An enqueue-only call with an explicit table copies it through one buffer of the context: keep such calls on one stream.  */
int  vv_classify_indices(vv_context *ctx, const uint8_t *index, size_t n, const float tf[1024],
                         uint8_t *rgba_out, int on_device, void *stream);

/* ---- isosurface frames: the first sample at or above a level (no reference counterpart) -----------------------------------------
 * An isosurface frame marches exactly the rays and samples of a vv_render_mip frame: same end points, per-slab radius, setup with the cut
 * plane (SLICE_PLANE_CUT; SLICE_PLANE marches as SLICE_NONE), 30-sample chunks, step, object scale, filter and 8-bit classification index k;
 * opts->ert_threshold and opts->ert_mode are ignored.  level: an integer in 1..255.  Per pixel, the HIT is the first executed sample, in
 * march order, with k >= level; the ray executes nothing after it.  A pixel therefore has a hit iff vv_render_mip's M >= level.
 * Each output may be NULL, at least one must be given; row 0 is the bottom row:
 *   index_out : W*H bytes: k of the hit, 0 where there is none.
 *   hit_out   : W*H records of four binary32 (16 bytes; a device pointer must be 16-byte aligned, else VV_ERR_INVALID).  xyz = the hit sample's
 *               position in cube space -- the coordinates of slice_params planes and of the first-pass images, before the object-scale
 *               mapping -- bit for bit the march's own accumulated position: origin + dir * dist of the sample's chunk (no contraction), then
 *               += sdir once per sample.  w = the number of samples the ray executed up to and including the hit, as a float (exact: a ray
 *               has fewer than 2^24 samples at the minimum step).  Depth along the ray: |xyz - ray origin|, or w * |sdir|.  No hit: (0, 0, 0, 0).
 *   rgba_out  : W*H*4 bytes: the hit shaded by a headlight, (0,0,0,0) where there is no hit.  With t the hit's texture coordinates,
 *               n_a the volume's dimensions and h_a = 1.0f / (float)n_a:
 *                 g_a = (int)k(t + h_a e_a) - (int)k(t - h_a e_a), a = x, y, z: six more samples through the march's fetch, filter,
 *                       classification and bounds test (index 0 outside [0,1)^3), issued once per pixel (and only when rgba_out is given);
 *                 G_a = ((float)g_a * (1.0f / scale[a])) * (float)n_a          (the gradient in cube space, up to the common factor 1/2)
 *                 dp = G . dir,  len = sqrtf(G . G),  diffuse = len > 0 ? fminf(fabsf(dp) / len, 1.0f) : 0.0f,  shade = 0.3f + 0.7f * diffuse
 *                 channel c of RGB = tf[k][c] * shade, alpha = 1, all four through vv_render's clamp-and-truncate conversion
 *               in binary32, evaluated in the order written without contraction (dot products x, y, z left to right), IEEE sqrtf and /.
 * Column W-1, row H-1 and the rows of other shards (slab_row_begin / _end, shard_*) stay untouched in all three images.  With count_samples,
 * vv_last_sample_count is the sum over the written rays of the samples executed up to and including the hit (all of them where there is none);
 * the touched_* instruments mark the same samples, and the six gradient gathers only under touched_lines_all = 1.  An instrumented frame
 * holds the same three images.  `stream`, out_on_device (all three images), the layout policy, vv_last_frame_ms and vv_debug_last_launch
 * (kernel family 3) work as for vv_render_mip.  The context's state is not changed.
 * Errors: level outside 1..255, all three outputs NULL, NULL slice / camera / rays: VV_ERR_INVALID; no volume: VV_ERR_NO_VOLUME.   */
int  vv_render_iso(vv_context *ctx, int width, int height,
                   const struct slice_params *slice,
                   const struct camera_params *camera,
                   const vv_ray_source *rays,
                   const vv_render_options *opts,     /* NULL => defaults */
                   int level,
                   uint8_t *rgba_out, uint8_t *index_out, float *hit_out, int out_on_device, void *stream);

/* ---- projection frames: maximum, minimum and mean intensity, with the extremum's place along the ray (no reference counterpart) ----
 * A projection frame marches exactly the rays and executed samples of a vv_render_mip frame: same end points, per-slab radius, setup with the
 * cut plane (SLICE_PLANE_CUT, its clipping and early return; SLICE_PLANE marches as SLICE_NONE), 30-sample chunks (sample i of a chunk runs
 * iff i * sstep + dist <= upper), step, object scale and filter; opts->ert_threshold and opts->ert_mode are ignored.
 * An executed sample is COUNTED iff its texture coordinates pass the march's bounds test, all three in [0,1); its k is the 8-bit
 * classification index the march gives it.  Executed samples outside the volume are not counted: they are no zeros.  (The per-slab sphere
 * starts rays in front of the cube, so most rays execute some.)  n = the counted samples of the ray, e = its executed samples, outside
 * ones included.  Per pixel, in integer arithmetic:
 *   VV_PROJ_MAX  : v = the largest k over the counted samples; ord = the 1-based ordinal, among the ray's executed samples in march order,
 *                  of the first counted sample with k == v (a later sample replaces an earlier one only if strictly greater).
 *   VV_PROJ_MIN  : the same with the smallest k and strictly less.
 *   VV_PROJ_MEAN : s = the sum of k over the counted samples (it fits 32 bits: a ray has fewer than 2^24 samples);
 *                  v = (2 * s + n) / (2 * n), evaluated in 64 bits, truncating: the mean rounded half up.
 *   n == 0       : v = 0, ord = 0, s = 0 (a ray that misses the volume, a zero-length ray, the cut plane's early return, a ray whose
 *                  samples all lie outside).
 * Each output may be NULL, at least one must be given; row 0 is the bottom row:
 *   index_out : W*H bytes holding v.
 *   rgba_out  : W*H*4 bytes: vv_render_mip's conversion of tf[v], for every pixel the frame writes, n == 0 included.
 *   stat_out  : W*H records of two uint32 (8 bytes; a device pointer must be 8-byte aligned, else VV_ERR_INVALID): {ord, n} for
 *               VV_PROJ_MAX / VV_PROJ_MIN, {s, n} for VV_PROJ_MEAN.  Depth of the extremum along the ray: ord * |sdir|, the meaning
 *               vv_render_iso gives to its w.
 * In VV_PROJ_MAX, index_out and rgba_out equal vv_render_mip's byte for byte for the same arguments (there an outside sample contributes 0
 * to the maximum, and n == 0 gives 0).
 * Column W-1, row H-1 and the rows of other shards (slab_row_begin / _end, shard_*) stay untouched in all three images.  With count_samples,
 * vv_last_sample_count is the sum of e over the written rays -- vv_render_mip's count; the touched_* instruments mark what they mark in a MIP
 * frame.  An instrumented frame holds the same three images.  `stream`, out_on_device (all three images), the layout policy, vv_last_frame_ms
 * and vv_debug_last_launch (kernel family 4) work as for vv_render_mip.  The context's state is not changed.  No result depends on the layout
 * sampled, the launch geometry or the samples per loop trip.
 * Errors: NULL ctx / slice / camera / rays, a mode outside 0..2, all three outputs NULL, a misaligned device stat_out: VV_ERR_INVALID; no
 * volume: VV_ERR_NO_VOLUME.  A failed call leaves the context usable.   */
typedef enum { VV_PROJ_MAX = 0, VV_PROJ_MIN = 1, VV_PROJ_MEAN = 2 } vv_proj_mode;
int  vv_render_projection(vv_context *ctx, int width, int height,
                          const struct slice_params *slice,
                          const struct camera_params *camera,
                          const vv_ray_source *rays,
                          const vv_render_options *opts,     /* NULL => defaults */
                          int mode,
                          uint8_t *rgba_out, uint8_t *index_out, uint32_t *stat_out, int out_on_device, void *stream);

/* ---- slice view: replaces invoke_slice_kernel (kernel.cuh:59, kernel.cu:506-519)
 * and invoke_advanced_slice_kernel (kernel.cuh:61, kernel.cu:522-541).
 * buffer: height*width floats; element (j,i) is stored at j*height+i exactly as
 * the reference does (kernel.cu:550,604).  legacy != 0 selects the 4-argument
 * slicekernel.cu:51-82 semantics (sagittal only, no scale, no bounds check).   */
int  vv_slice(vv_context *ctx, float *buffer, size_t height, size_t width,
              float dx, float dy, float dz, int orientation,
              const float scale[3], int legacy, int filter,
              int out_on_device, void *stream);
int  vv_slice_advanced(vv_context *ctx, float *buffer, size_t height, size_t width,
                       const float trans[16] /* row-major, CS123Algebra.h:278-281 */,
                       const float scale[3], int filter,
                       int out_on_device, void *stream);

/* ---- thick-slab slices: the maximum, minimum or mean over K samples around the slice plane (no reference counterpart) ------------
 * A slab call takes K = slab->samples (1..VV_SLAB_MAX_SAMPLES) samples of vv_slice / vv_slice_advanced per pixel and keeps one number.
 * Everything is binary32, evaluated in the order written, without contraction.
 *   spacing = thickness / (float)K;   sample k (0 <= k < K) has offset  o_k = ((float)k - 0.5f * (float)(K - 1)) * spacing.
 * Position of sample k:
 *   vv_slice_slab          : the slab runs along the coordinate the slice kernel's orientation switch leaves at 0 -- VV_SAGITTAL: z,
 *                            VV_HORIZONTAL: y, VV_CORONAL: x.  The position is vv_slice's own arithmetic with that axis' displacement d_a
 *                            replaced by d_a + o_k (one add, made before anything else).  thickness is in the units of dx, dy, dz.
 *   vv_slice_advanced_slab : vv_slice_advanced's arithmetic with rz = 0.5f + o_k in the place of 0.5f.  thickness is in the units of the
 *                            transform's third input coordinate.
 * A sample is EXECUTED iff its texture coordinates pass the slice kernel's bounds test (all three in [0, 1)); its value s_k is what the
 * slice kernel would store there (the filtered value, / 255 for u8 volumes).  Samples outside the volume are not executed: they do not
 * count as 0.  Per pixel, with n the number of executed samples:
 *   VV_SLAB_MAX  : the largest s_k;  aux = the smallest k that attains it (a later sample replaces the current one only if strictly greater)
 *   VV_SLAB_MIN  : the smallest s_k; aux = the smallest k that attains it (... only if strictly less)
 *   VV_SLAB_MEAN : acc / (float)n, IEEE division; acc starts as the first executed sample's value, every later executed sample is added
 *                  in order of k, one add each; aux = n
 *   n = 0        : the value is 0.0f; aux = -1 (MAX, MIN) or 0 (MEAN)
 * Storage is vv_slice's: the element of pixel (j, i) goes to offset j*height + i of `buffer` and, where given, of `aux` (height*width
 * int32 each); offsets at or beyond height*width are skipped, and so are pixels with i >= height && j + 1 < height.  Elements that are
 * not written keep the caller's bytes in both buffers.  vv_slice_to_bgra works on `buffer` unchanged.
 * With samples == 1, `buffer` equals what vv_slice / vv_slice_advanced write for the same arguments, bit for bit, in every mode and for
 * any thickness.
 * `stream` and out_on_device work as for vv_slice and apply to both buffers; a device `aux` must be 4-byte aligned.  The kernel samples
 * the linear volume (volumes above 4 GiB included); the optional layout copies and the context's state are not touched.  f32 voxels: the
 * value domain of vv_load_volume_f32; a mean whose running sum leaves the binary32 range is +-Inf as IEEE addition says, and no NaN
 * arises from in-domain voxels.
 * Errors: NULL ctx, buffer, scale, trans or slab, a mode outside vv_slab_mode, samples outside 1..VV_SLAB_MAX_SAMPLES, a thickness that is
 * negative or not finite, an orientation other than the three canonical ones, sizes vv_slice rejects, a misaligned device aux:
 * VV_ERR_INVALID; no volume: VV_ERR_NO_VOLUME.  There is no legacy form.  A failed call leaves the context usable.                  */
typedef enum { VV_SLAB_MAX = 0, VV_SLAB_MIN = 1, VV_SLAB_MEAN = 2 } vv_slab_mode;
#define VV_SLAB_MAX_SAMPLES 1024
typedef struct vv_slab { int mode; int samples; float thickness; } vv_slab;
int  vv_slice_slab(vv_context *ctx, float *buffer, int32_t *aux /* or NULL */, size_t height, size_t width,
                   float dx, float dy, float dz, int orientation, const float scale[3], int filter,
                   const vv_slab *slab, int out_on_device, void *stream);
int  vv_slice_advanced_slab(vv_context *ctx, float *buffer, int32_t *aux /* or NULL */, size_t height, size_t width,
                            const float trans[16], const float scale[3], int filter,
                            const vv_slab *slab, int out_on_device, void *stream);

/* ---- histograms: how the loaded volume, or an index image, is distributed over the 256 classification indices (no reference counterpart) ----
 * vv_volume_histogram counts the voxels of a box of the loaded volume where it lies, in HBM, whatever put it there (host upload, device buffer,
 * streamed upload with or without promotion, re-pitching after the upload).
 *  1. BIN of a voxel v: the 8-bit classification index the march, MIP and isosurface kernels give a sample that falls exactly on the voxel's
 *     centre (the kernels' own conversion, index_of in csrc/vv_device.h).  u8: the byte itself.  f32: s = v * 255.0f in binary32, one rounding;
 *     the bin is 0 if s is NaN or s < 1, 255 if s >= 255 (+Inf included), otherwise s truncated toward zero.  counts[k] therefore answers "how
 *     much of the volume does table entry k colour".
 *  2. RANGE: vmin / vmax are bit-for-bit copies of a voxel of the box: the least and the greatest of its non-NaN voxels under the total order of
 *     binary32 bit patterns (-0.0 below +0.0; +-Inf take part; denormals are not flushed: integer keys are compared, no floating-point minimum
 *     or maximum is taken, and the denormal mode of the library's units does not show).  No non-NaN voxel: vmin = +Inf, vmax = -Inf.  u8 volumes:
 *     the smallest and the largest byte, as float.  NaN voxels are counted in nan_voxels and, by rule 1, in counts[0].
 *  3. BOX: box_lo inclusive, box_hi exclusive, in voxels (x, y, z), 0 <= lo[a] < hi[a] <= dims[a]; both NULL = the whole volume.  Only voxels of
 *     the box are read as data; the padding of a re-pitched volume (32 bytes per row, an extra row per slice) is never counted.
 *  4. EXACT: every field is exact and the same from run to run (integer adds and maxima do not depend on the order of arrival); nothing depends
 *     on what `out` held, on the volume's layout in HBM, on the launch geometry or on how the volume was loaded.
 *  5. vv_histogram_indices: counts[k] = the number of bytes of index[0..n) equal to k; n = 0 gives 256 zeros.  index and counts are both host or
 *     both device pointers (on_device); device counts must be 8-byte aligned.  Needs no volume, as vv_classify_indices: the distribution of a MIP
 *     or isosurface index image, for auto-windowing.  No byte outside index[0..n) is read.
 *  6. `stream` / out_on_device / on_device as for vv_classify_indices: NULL = the context's stream, the call returns when the work is complete; any
 *     other handle with device output only enqueues.  The accumulators live in scratch of the context: keep enqueue-only histogram calls of one
 *     context on one stream.  The context's volume, table, layout copies and residency state are not touched; vv_last_frame_ms keeps its value.
 *  7. Errors: NULL ctx or out / counts, a box with one bound NULL, a box outside rule 3, a misaligned device out / counts, NULL index with
 *     n > 0: VV_ERR_INVALID; vv_volume_histogram before a volume is loaded: VV_ERR_NO_VOLUME.  A failed call leaves the context usable.
 * A device vv_histogram must be 8-byte aligned.                                                                                              */
typedef struct vv_histogram {
    unsigned long long counts[256];  /* voxels per classification index */
    unsigned long long voxels;       /* voxels in the box = sum of counts */
    unsigned long long nan_voxels;   /* f32 volumes: NaN voxels (also counted in counts[0]); u8: 0 */
    float vmin, vmax;                /* storage units: u8 0..255 as float, f32 the voxel itself */
} vv_histogram;                      /* 2072 bytes */
int  vv_volume_histogram(vv_context *ctx, const int box_lo[3], const int box_hi[3],   /* both NULL = whole volume */
                         vv_histogram *out, int out_on_device, void *stream);
int  vv_histogram_indices(vv_context *ctx, const uint8_t *index, size_t n,
                          unsigned long long counts[256], int on_device, void *stream);

/* ---- derived volumes: a box of the loaded volume cropped, reduced by whole factors, windowed and converted (no reference counterpart) ----
 * vv_derive_volume makes another volume out of the loaded one where it lies, in HBM, whatever put it there: `out` receives a dense volume, x
 * fastest, of m_x * m_y * m_z voxels of out_type, m_a = ceil((hi_a - lo_a) / f_a) (vv_derive_dims), ready for vv_load_volume_device /
 * vv_load_volume_* on this or another context.
 *  1. CELL: output voxel (X, Y, Z) covers the source voxels with lo_a + X_a f_a <= x_a < min(lo_a + (X_a + 1) f_a, hi_a); n is their number
 *     (n >= 1).  Cells at the high end of the box are partial: the voxels they lack are not zeros, they do not count.
 *  2. REDUCTION, in storage units, giving r.
 *     u8 source, MEAN: r = (2 s + n) / (2 n) in integers, s the cell's sum: the mean rounded half up (the rule of VV_PROJ_MEAN).
 *     u8 source, MAX / MIN: the largest / smallest byte.
 *     f32 source, MEAN: acc starts as the cell's first voxel (lowest z, then lowest y, then lowest x); every other voxel is added in memory order
 *     (x fastest, then y, then z), one binary32 add each, no contraction; r = acc / (float)n, IEEE division.  n == 1: r is the voxel bit for
 *     bit.  Sums that leave the binary32 range are +-Inf as IEEE addition says; a NaN in the cell gives a NaN (which one is not specified).
 *     f32 source, MAX / MIN: a bit-for-bit copy of the greatest / least non-NaN voxel of the cell under the total order of bit patterns of
 *     vv_volume_histogram's rule 2 (-0.0 below +0.0, +-Inf take part, denormals are values like any other: integer keys are compared).  A cell
 *     of NaNs only: r = 0x7FC00000.
 *  3. UNIT SCALE, WINDOW, OUTPUT TYPE: binary32, in the order written, no contraction.
 *     window = 0:  u8 -> u8: out = r.  u8 -> f32: out = r / 255, correctly rounded (the promotion of vv_promote_u8_to_f32 and of the streamed
 *     upload).  f32 -> f32: out = r.  f32 -> u8: out = the classification index of r, vv_volume_histogram's rule 1.
 *     window = 1:  u = r (f32 source) or (float)r (u8 source); w = (u - win_lo) / (win_hi - win_lo): two subtractions and one IEEE division, so
 *     w is exactly 0 at win_lo and exactly 1 at win_hi.  f32 out: out = w, not clamped (the classification saturates; a NaN stays a NaN).
 *     u8 out: out = the classification index of w.  win_lo / win_hi are in storage units, those of vv_histogram.vmin / vmax (u8: 0..255).
 *  4. What follows: (a) factor (1, 1, 1), no window, out_type = the volume's type: `out` is the box of the volume as it was loaded, byte for
 *     byte -- the read-back (MAX / MIN write a NaN voxel as 0x7FC00000).  (b) factor 1, f32 -> u8, no window: the byte at a voxel is that
 *     voxel's histogram bin, so vv_volume_histogram of the derived volume, once loaded, has the counts of the source box.  (c) Nothing depends on
 *     the pitch of the source in HBM, on the launch geometry, on how the volume was loaded or on what `out` held.  (d) No byte outside the box
 *     is read as data (the padding of a re-pitched volume never shows); no byte beyond m_x m_y m_z voxels of `out` is written.
 *  5. BOX: box_lo inclusive, box_hi exclusive, in voxels (x, y, z), 0 <= lo < hi <= dims on every axis; all six values 0 = the whole volume.
 *     factor: source voxels per output voxel and axis, 1..8; 0 is read as 1.
 *  6. `stream` / out_on_device as for vv_volume_histogram: NULL = the context's stream, the call returns when the work is complete; any other
 *     handle with a device `out` only enqueues.  A host `out` is staged through a device buffer of the call's own, allocated at the output's
 *     size and released before the call returns (not kept in the context: the 2x reduction of a 2048^3 f32 volume is 4 GiB).  The context's
 *     volume, table, layout copies and residency state are not touched; vv_last_frame_ms keeps its value.
 *  7. Errors, in this order.  VV_ERR_INVALID: NULL ctx / d / out / out_dims.  VV_ERR_NO_VOLUME: no volume loaded (vv_derive_dims too: the box is
 *     measured against the volume).  VV_ERR_INVALID: a box outside rule 5; a factor outside 0..8; a mode or out_type outside its enum; window
 *     not 0 or 1; a window whose win_lo, win_hi or win_hi - win_lo (binary32) is not finite or whose difference is not > 0; capacity (bytes)
 *     below the output's bytes; a device f32 `out` that is not 4-byte aligned.  VV_ERR_NOMEM: the staging buffer of a host `out` could not be
 *     allocated.  A failed call leaves the context usable and `out` untouched.                                                              */
typedef enum { VV_REDUCE_MEAN = 0, VV_REDUCE_MAX = 1, VV_REDUCE_MIN = 2 } vv_reduce_mode;
typedef struct vv_derive {
    int   box_lo[3], box_hi[3];  /* voxels (x, y, z), lo inclusive, hi exclusive, 0 <= lo < hi <= dims; all six 0 = the whole volume */
    int   factor[3];             /* source voxels per output voxel and axis, 1..8; 0 is read as 1 */
    int   mode;                  /* vv_reduce_mode */
    int   out_type;              /* VV_VOXEL_U8 or VV_VOXEL_F32, whatever the loaded volume's type */
    int   window;                /* 0 = none; 1 = map [win_lo, win_hi] onto [0, 1] */
    float win_lo, win_hi;        /* storage units, those of vv_histogram.vmin / vmax (u8 volumes: 0..255) */
} vv_derive;                     /* 56 bytes */
int  vv_derive_dims(const vv_context *ctx, const vv_derive *d, int out_dims[3]);   /* host only; m_a = ceil((hi_a - lo_a) / f_a) */
int  vv_derive_volume(vv_context *ctx, const vv_derive *d, void *out, size_t capacity,
                      int out_on_device, void *stream);

/* ---- neighbourhood filters ("stencils"): a box of the loaded volume smoothed, median-filtered or turned into its gradient magnitude (no
 * reference counterpart; vv_filter is the trilinear model, these calls look at a voxel's neighbours) ----
 * vv_stencil_volume filters the loaded volume where it lies, in HBM: `out` receives a dense volume, x fastest, of the box's extents hi - lo (no
 * reduction) in out_type, ready for vv_load_volume_device / vv_load_volume_* on this or another context.
 *  1. SOURCE VALUE AND EDGES: u(x, y, z) is the voxel in storage units as binary32: an f32 voxel itself, (float)byte for u8.  Every coordinate a
 *     stencil reaches is clamped to [0, n_a - 1] of the VOLUME, not of the box (edge replication): a box inside the volume sees its true
 *     neighbours outside the box, and the result for a box is the crop of the result for the whole volume, bit for bit.
 *  2. ARITHMETIC: binary32, in the order written, one rounding per operation, no contraction, denormals kept (vv_derive_volume's stage 3).
 *  3. VV_STENCIL_SEPARABLE: three passes, x then y then z: P_x = conv_x(u), P_y = conv_y(P_x), r = conv_z(P_y).  Each intermediate is a binary32
 *     value defined at every voxel of the volume; the clamp of rule 1 applies to the axis of the pass.  One pass with radius R and taps t:
 *     acc = t[0] * c, then for k = 1..R in order acc = acc + t[k] * (v(-k) + v(+k)): the pair's sum, then the product, then the add.  R = 0: the
 *     pass is the identity, bit for bit (no multiplication by t[0]).  taps[a][k] with k > radius[a] are ignored.
 *  4. VV_STENCIL_MEDIAN: the 27 values of the clamped 3x3x3 neighbourhood (at an edge values repeat), ordered as bytes (u8) or by the total order
 *     of binary32 bit patterns of vv_volume_histogram's rule 2 (f32: a NaN takes part by its pattern, positive-sign NaNs above +Inf, negative-sign
 *     ones below -Inf); r is a bit-for-bit copy of the 14th smallest.  No floating-point comparison is made.
 *  5. VV_STENCIL_GRADMAG: g_a = u(+e_a) - u(-e_a) with clamped coordinates (at a face a one-sided difference, unscaled); G_a = g_a * gscale[a];
 *     r = sqrtf((G_x * G_x + G_y * G_y) + G_z * G_z), IEEE sqrtf.  gscale (0, 0, 0) is read as (1, 1, 1).
 *  6. OUTPUT: f32 -> f32: out = r.  f32 -> u8: out = the classification index of r (vv_volume_histogram's rule 1; a NaN gives 0).  u8 -> f32:
 *     out = r / 255.0f, IEEE division (MEDIAN: the promotion of vv_promote_u8_to_f32).  u8 -> u8, MEDIAN: out = r.  u8 -> u8, SEPARABLE and
 *     GRADMAG: 0 if r is NaN or r < 0.5f; 255 if r >= 254.5f; otherwise (int)(r + 0.5f): one binary32 add, then truncation (this sequence of
 *     operations is the rule, not "round half up" as mathematics).
 *  7. What follows: (a) the crop identity of rule 1.  (b) SEPARABLE with radius (0, 0, 0) equals vv_derive_volume at factor 1, MEAN, no window,
 *     the same box and out_type, byte for byte, for all four type pairs.  (c) Nothing depends on the pitch of the source in HBM, on the 64-bit
 *     addressing build, on the launch geometry, on how the volume was loaded or on what `out` held.  (d) No byte beyond the output's voxels is
 *     written, no byte outside the volume's allocation is read, and the padding of a re-pitched volume is never read as data: clamping is by
 *     coordinates.  (e) Results are the same from run to run.
 *  8. `stream` / out_on_device as for vv_derive_volume.  A host `out` is staged through a device buffer of the call's own, sized to the output
 *     and released before the call returns.  A device-`out` call allocates no device memory and uses no volume-sized temporary: the three passes
 *     are one launch (a 1024^3 f32 intermediate would be 4 GiB beside a volume and its copies, which are under a budget).  The context's volume,
 *     table, layout copies and residency state are not touched; vv_last_frame_ms keeps its value.
 *  9. Errors, in this order.  VV_ERR_INVALID: NULL ctx / s / out.  VV_ERR_NO_VOLUME: no volume loaded.  VV_ERR_INVALID, each in turn: a box
 *     outside vv_derive's rule 5; a kind or out_type outside its enum; SEPARABLE: a radius outside 0..VV_STENCIL_MAX_RADIUS, or a tap with index
 *     <= its radius that is not finite; GRADMAG: a gscale that is not finite; capacity (bytes) below the output's bytes; a device f32 `out` that
 *     is not 4-byte aligned; a device `out` whose byte range overlaps the context's linear volume allocation (the pass is not in place).
 *     VV_ERR_NOMEM: the staging buffer of a host `out` could not be allocated.  A failed call writes nothing and leaves the context usable.
 * vv_stencil_taps fills taps[0..radius] (the rest with 0) for one axis; host only.  VV_TAPS_BOX: every tap 1.0f / (2 R + 1).  VV_TAPS_BINOMIAL:
 * tap k = C(2 R, R + k) / 4^R, exact dyadics.  VV_TAPS_GAUSS: w_k = exp(-k^2 / (2 sigma^2)) in binary64, normalised by w_0 + 2 w_1 + ... + 2 w_R
 * (summed in that order), rounded once to binary32; sigma must be finite and > 0 (the other shapes ignore it).  VV_ERR_INVALID: a shape outside
 * the enum, a radius outside 0..VV_STENCIL_MAX_RADIUS, a bad sigma, NULL taps.                                                              */
typedef enum { VV_STENCIL_SEPARABLE = 0, VV_STENCIL_MEDIAN = 1, VV_STENCIL_GRADMAG = 2 } vv_stencil_kind;
#define VV_STENCIL_MAX_RADIUS 4
typedef struct vv_stencil {
    int   box_lo[3], box_hi[3];  /* as vv_derive: lo inclusive, hi exclusive, all six 0 = the whole volume */
    int   kind;                  /* vv_stencil_kind */
    int   out_type;              /* VV_VOXEL_U8 or VV_VOXEL_F32, whatever the loaded volume's type */
    int   radius[3];             /* SEPARABLE: taps per side on x, y, z, 0..VV_STENCIL_MAX_RADIUS; 0 = that axis is not filtered */
    float taps[3][5];            /* SEPARABLE: taps[a][0] the centre, taps[a][k] at distance k on both sides */
    float gscale[3];             /* GRADMAG: per-axis multiplier; all three 0 = (1, 1, 1) */
} vv_stencil;                    /* 116 bytes */
int  vv_stencil_volume(vv_context *ctx, const vv_stencil *s, void *out, size_t capacity,
                       int out_on_device, void *stream);
typedef enum { VV_TAPS_BOX = 0, VV_TAPS_BINOMIAL = 1, VV_TAPS_GAUSS = 2 } vv_taps_shape;
int  vv_stencil_taps(int shape, int radius, float sigma, float taps[5]);   /* host only, no context */

/* ---- resampled volumes: the loaded volume on another grid (no reference counterpart) ----
 * vv_resample_volume samples the loaded volume where it lies, in HBM: every voxel of an output grid of dims m_x x m_y x m_z is the sample of the
 * volume at an affinely mapped position -- an anisotropic scan made isotropic, a reoriented or zoomed volume, a level of detail that is no whole
 * factor.  `out` receives a dense volume, x fastest, of the box's extents in out_type, ready for vv_load_volume_device / vv_load_volume_*.
 * Everything below is binary32, in the order written, one rounding per operation, no contraction, denormals kept.
 *  1. POSITION: inv_a = 1.0f / (float)m_a, one IEEE division made once.  Output voxel (X, Y, Z) of the GRID (not of the box):
 *     q_a = ((float)X_a + 0.5f) * inv_a;  p_r = ((m[4r] * q_x + m[4r+1] * q_y) + m[4r+2] * q_z) + m[4r+3], r = 0, 1, 2.  p is in the texture
 *     coordinates of vv_slice: [0, 1) spans the volume on each axis.
 *  2. INSIDE: vv_slice's test: p_r >= 0.0f && p_r < 1.0f for all three r (a NaN is outside; -0.0f is inside and samples as 0.0f).  Outside: r = fill.
 *  3. VALUE: VV_RESAMPLE_TEX8 / VV_RESAMPLE_EXACT: r = the trilinear value of the texture model at p under that vv_filter, in storage units
 *     (0..255 for u8): what vv_slice filters before its / 255 -- x, then y, then z, each fma(w, b - a, a).  VV_RESAMPLE_NEAREST:
 *     i_a = min((uint32_t)(p_a * (float)n_a), n_a - 1); r = that voxel as binary32 ((float)byte for u8); no arithmetic touches it afterwards.
 *  4. OUTPUT (vv_stencil_volume's rule 6 for arithmetic results): f32 -> f32: r (NEAREST: the voxel's pattern, bit for bit).  f32 -> u8: the
 *     classification index of r.  u8 -> f32: r / 255.0f, IEEE.  u8 -> u8: 0 if r is NaN or r < 0.5f; 255 if r >= 254.5f; otherwise
 *     (int)(r + 0.5f) (NEAREST: the byte).  fill goes through the same stage.
 *  5. LAYOUT: `out` is dense, x fastest, with the box's extents hi - lo.
 *  6. What follows: (a) the result for a box is the crop of the whole grid's result, bit for bit.  (b) The identity m with dims = the volume's,
 *     NEAREST and the volume's own type is the volume read back, byte for byte, for any dims up to VV_RESAMPLE_MAX_DIM ((uint32_t)(q * n) == X
 *     and q < 1 for every X < n); so it is with TEX8 on u8 volumes (|fma(q, n, -0.5) - X| <= 2^-13: the weight rounds to 0, or to 1 on the voxel
 *     below), and with TEX8 / EXACT on f32 volumes whose dims are powers of two (fma(q, n, -0.5) == X).  (c) Nothing depends on the pitch of the
 *     source, on the 64-bit addressing build, on the launch geometry, on how the volume was loaded or on what `out` held.  (d) No byte beyond the
 *     output's voxels is written, no byte outside the volume's allocation is read, padding is never data: addresses come from coordinates clamped
 *     as the texture model clamps them, never from voxel values.  (e) Results are the same from run to run.
 *  7. VALUE DOMAIN of f32 voxels: that of vv_load_volume_f32 under TEX8 / EXACT; NEAREST copies any pattern.
 *  8. `stream` / out_on_device / staging as for vv_stencil_volume: a host `out` goes through a device buffer of the call's own, a device-`out`
 *     call allocates nothing.  The linear volume is sampled (above 4 GiB with 64-bit slice bases, as vv_slice); volume, table, copies,
 *     residency state and vv_last_frame_ms are not touched.
 *  9. Errors, in this order.  VV_ERR_INVALID: NULL ctx / r / out.  VV_ERR_NO_VOLUME: no volume loaded.  VV_ERR_INVALID, each in turn: dims
 *     outside 1..VV_RESAMPLE_MAX_DIM; a box that is not all zeros and not 0 <= lo < hi <= dims; a filter or out_type outside its enum; any of
 *     m[0..11] or fill not finite; capacity (bytes) below the output's bytes (computed in 64 bits); a device f32 `out` that is not 4-byte
 *     aligned; a device `out` whose byte range overlaps the context's linear volume allocation.  VV_ERR_NOMEM: the staging buffer of a host
 *     `out` could not be allocated.  A refused call writes nothing and leaves the context usable.
 * vv_resample_matrix (host only, binary64): R = Rz(euler[2]) * Ry(euler[1]) * Rx(euler[0]), angles in radians; A_rc = R_rc * (s_c / s_r) / zoom
 * with s = scale (NULL or all zeros = (1, 1, 1)); t = centre - A * (0.5, 0.5, 0.5); m = [A | t], each entry rounded once to binary32.  Zero
 * angles, zoom 1 and centre (0.5, 0.5, 0.5) give the identity exactly for any scale; zoom 2 gives diag 0.5 and t = 0.25.  VV_ERR_INVALID: NULL
 * euler / centre / m, an input that is not finite, zoom not > 0, a scale component not > 0 when not all are zero.                          */
typedef enum { VV_RESAMPLE_TEX8 = 0, VV_RESAMPLE_EXACT = 1, VV_RESAMPLE_NEAREST = 2 } vv_resample_filter;  /* 0, 1 = the values of vv_filter */
#define VV_RESAMPLE_MAX_DIM 16384
typedef struct vv_resample {
    int   dims[3];               /* output grid m_x, m_y, m_z, each 1..VV_RESAMPLE_MAX_DIM */
    int   box_lo[3], box_hi[3];  /* the part of the OUTPUT grid to compute, lo inclusive, hi exclusive; all six 0 = the whole grid */
    int   filter;                /* vv_resample_filter */
    int   out_type;              /* VV_VOXEL_U8 or VV_VOXEL_F32, whatever the loaded volume's type */
    float m[12];                 /* row-major 3 x 4: output coordinates q -> texture coordinates p of the loaded volume */
    float fill;                  /* r of a sample outside the volume, storage units of the source */
} vv_resample;                   /* 96 bytes; offsets 0, 12, 24, 36, 40, 44, 92 */
int  vv_resample_volume(vv_context *ctx, const vv_resample *r, void *out, size_t capacity,
                        int out_on_device, void *stream);
int  vv_resample_matrix(const float euler[3], float zoom, const float centre[3], const float scale[3] /* or NULL */,
                        float m[12]);   /* host only, no context */

/* ---- segmentation: connected-component labels of a box of the loaded volume, and the volume masked by them (no reference counterpart) ----
 * vv_label_volume labels the loaded volume where it lies, in HBM: the voxels of a box whose classification index lies in a range are the
 * foreground, and every foreground voxel receives the label of its connected component.  vv_mask_volume then writes the volume where a test
 * on the labels holds and `fill` elsewhere: thresholding by the table entries that colour a structure, keeping the region under a seed (or the
 * largest region, or everything above a size), and rendering only that, without the volume leaving the device.
 *  1. FOREGROUND: a voxel of the box is foreground iff bin_lo <= bin <= bin_hi, bin the classification index of vv_volume_histogram's rule 1 (the
 *     byte of a u8 voxel).  A NaN has bin 0, +Inf has bin 255.
 *  2. NEIGHBOURS: two voxels of the box are neighbours iff their coordinates differ by at most 1 on every axis and differ on exactly one axis
 *     (connectivity 6), on at most two (18) or on up to three (26).  Voxels outside the box do not exist: a structure that the box cuts in two
 *     becomes two components.  Unlike vv_derive_volume, vv_stencil_volume and vv_resample_volume, the result for a box is therefore NOT the crop
 *     of the whole volume's result.
 *  3. COMPONENT: the classes of the transitive closure of "neighbours and both foreground".
 *  4. LABEL: a background voxel gets 0; a foreground voxel gets 1 + i_min, where i = ((z - lo_z) b_y + (y - lo_y)) b_x + (x - lo_x) numbers the
 *     box's voxels (b = hi - lo) and i_min is the least i of the voxel's component.  The label is a property of the input alone: every output is
 *     exact and the same from run to run.  The box may hold at most 2^32 - 2 voxels (0xFFFFFFFF is never a label).  `labels` is dense, x fastest,
 *     with the box's extents: labels[i] is the label of voxel i.
 *  5. SIZES (optional): sizes[i] = the number of voxels of the component whose least voxel is i, and 0 at every other i: sizes[label - 1] is the
 *     size of a labelled voxel's component.
 *  6. STATS (optional): foreground = the box's foreground voxels, components = their components; with `sizes`, largest_size = the largest
 *     component's voxels and largest_label = the smallest label among the components of that size; without `sizes` (or without foreground) both
 *     are 0.  reserved is written as 0.
 *  7. What follows: (a) bin_lo = 0, bin_hi = 255: every voxel has label 1.  (b) The components under 6 refine those under 18, which refine those
 *     under 26.  (c) Nothing depends on the pitch of the source, on the 64-bit addressing build, on the launch geometry, on how the volume was
 *     loaded or on what the outputs held.  (d) No byte outside the box is read as data; no byte beyond 4 b_x b_y b_z of labels / sizes and
 *     sizeof(vv_label_stats) of stats is written.
 *  8. STREAM AND MEMORY: labels, sizes and stats are all host pointers or all device pointers (out_on_device).  Device labels and sizes must be
 *     4-byte aligned, device stats 8-byte aligned.  A device-output call allocates no device memory: `labels` is its only volume-sized working
 *     array, the counters live in scratch the context holds from vv_init on (keep enqueue-only calls of one context on one stream).  The call is
 *     a fixed number of kernel launches for given arguments, with no host read-back between them: `stream` NULL = the context's stream, the call
 *     returns when the work is complete; any other handle with device outputs only enqueues (as vv_stencil_volume).  Host outputs are staged
 *     through device buffers of the call's own, released before it returns.  The context's volume, table, layout copies and residency state are
 *     not touched; vv_last_frame_ms keeps its value.
 *  9. Errors, in this order.  VV_ERR_INVALID: NULL ctx / d / labels.  VV_ERR_NO_VOLUME: no volume loaded.  VV_ERR_INVALID, each in turn: a box
 *     outside vv_derive's rule 5; more than 2^32 - 2 voxels in the box; bins outside 0 <= bin_lo <= bin_hi <= 255; a connectivity other than 6, 18
 *     or 26; capacity (bytes, of labels and of sizes each) below 4 b_x b_y b_z; a misaligned device pointer; a device labels or sizes whose byte
 *     range overlaps the context's linear volume allocation or the other buffer.  VV_ERR_NOMEM: a staging buffer of a host output could not be
 *     allocated.  A refused call writes nothing and leaves the context usable.
 * vv_mask_volume: `out` receives a dense volume, x fastest, of the box's extents in out_type, ready for vv_load_volume_device / vv_load_volume_*.
 *  M1. Output voxel i is KEPT iff test(i) != invert.  VV_KEEP_LABEL: labels[i] == label.  VV_KEEP_FOREGROUND: labels[i] != 0.  VV_KEEP_MIN_SIZE:
 *      labels[i] != 0 && labels[i] - 1 < voxels && sizes[labels[i] - 1] >= min_size (voxels = b_x b_y b_z; the bound is part of the rule:
 *      `labels` is caller data and never makes an address unchecked).
 *  M2. A kept voxel is the source voxel through the copy stage: vv_derive_volume at factor 1 without a window (rule 3 there).  Any other voxel
 *      is `fill` (storage units of the source) through the arithmetic output stage: vv_resample_volume's rule 4.
 *  M3. What follows: with the labels of bins 0..255 and VV_KEEP_FOREGROUND, `out` equals vv_derive_volume at factor 1, same box and out_type,
 *      byte for byte.  Rule 7 (c), (d) hold here too.
 *  M4. labels, sizes and out are all host or all device pointers (on_device); device labels / sizes must be 4-byte aligned, a device f32 out
 *      too.  Host buffers are staged through device buffers of the call's own; a device call allocates nothing.  `stream` as in rule 8.
 *  M5. Errors, in this order.  VV_ERR_INVALID: NULL ctx / m / labels / out.  VV_ERR_NO_VOLUME: no volume loaded.  VV_ERR_INVALID, each in turn:
 *      a box outside vv_derive's rule 5 or above 2^32 - 2 voxels; an out_type or keep outside its enum; invert not 0 or 1; a fill that is not
 *      finite; VV_KEEP_MIN_SIZE with sizes == NULL; capacity (bytes) below the output's bytes; a misaligned device pointer; a device out whose
 *      byte range overlaps the context's linear volume allocation, labels or sizes.  VV_ERR_NOMEM: a staging buffer could not be allocated.  A
 *      refused call writes nothing and leaves the context usable.                                                                            */
typedef struct vv_label {
    int box_lo[3], box_hi[3];   /* as vv_derive: lo inclusive, hi exclusive, all six 0 = the whole volume */
    int bin_lo, bin_hi;         /* foreground: bin_lo <= bin <= bin_hi, both in 0..255, bin_lo <= bin_hi */
    int connectivity;           /* 6, 18 or 26 */
} vv_label;                     /* 36 bytes */
typedef struct vv_label_stats {
    unsigned long long foreground;    /* foreground voxels of the box */
    unsigned long long components;
    unsigned long long largest_size;  /* 0 when `sizes` is NULL */
    uint32_t largest_label;           /* smallest label among the components of that size; 0 when `sizes` is NULL or there is no foreground */
    uint32_t reserved;                /* written as 0 */
} vv_label_stats;                     /* 32 bytes */
int  vv_label_volume(vv_context *ctx, const vv_label *d, uint32_t *labels, size_t capacity,
                     uint32_t *sizes /* or NULL; same extents and capacity */, vv_label_stats *stats /* or NULL */,
                     int out_on_device, void *stream);
typedef enum { VV_KEEP_LABEL = 0, VV_KEEP_FOREGROUND = 1, VV_KEEP_MIN_SIZE = 2 } vv_keep;
typedef struct vv_mask {
    int      box_lo[3], box_hi[3];  /* the box the labels were made for */
    int      out_type;              /* VV_VOXEL_U8 or VV_VOXEL_F32 */
    int      keep;                  /* vv_keep */
    int      invert;                /* 0 / 1 */
    uint32_t label;                 /* VV_KEEP_LABEL */
    uint32_t min_size;              /* VV_KEEP_MIN_SIZE (needs sizes) */
    float    fill;                  /* storage units of the source, finite */
} vv_mask;                          /* 48 bytes */
int  vv_mask_volume(vv_context *ctx, const vv_mask *m, const uint32_t *labels, const uint32_t *sizes /* or NULL */,
                    void *out, size_t capacity, int on_device, void *stream);

/* ---- distance transform: the exact squared Euclidean distance of every voxel of a box to a voxel set (no reference counterpart) ----
 * vv_distance_volume writes, for a box of the loaded volume, how far each voxel lies from the nearest SEED: a voxel chosen by its classification
 * index or by a test on labels that vv_label_volume (or this call) wrote for the box.  With integer voxel pitches the squared distance is an
 * integer and a property of the input alone.  Growing a margin, and opening or closing a segmentation with a ball, are this call composed with
 * itself on the device (Context.morphology of the Python binding).
 *  1. SEEDS: a voxel of the box is a seed iff test != invert.  VV_SEED_BINS: bin_lo <= bin <= bin_hi, bin the classification index of
 *     vv_label_volume's rule 1 read from the loaded volume (a NaN has bin 0, +Inf has bin 255).  VV_SEED_LABEL: labels[i] == label.
 *     VV_SEED_NONZERO: labels[i] != 0.
 *  2. LABELS: `labels` is dense, x fastest, with the box's extents (i as in vv_label_volume's rule 4): what vv_label_volume or a VV_DIST_WITHIN
 *     call wrote for that box.  NULL for VV_SEED_BINS.
 *  3. BOX: voxels outside the box do not exist (vv_label_volume's rule 2): a seed one voxel outside the box is not seen, and the complement of
 *     a set ends at the box's faces (an erosion does not eat in from them).  The result for a box is NOT the crop of the whole volume's.
 *  4. DISTANCE: D(i) = min over the seeds s of sum_a (spacing_a (i_a - s_a))^2, an integer.  VV_DIST_SQUARED writes D(i) as uint32; 0xFFFFFFFF
 *     at every voxel if the box has no seed.  VV_DIST_WITHIN writes 1 where D(i) <= within_r2 and 0 elsewhere (everywhere without a seed).
 *  5. COMPOSITION: a VV_DIST_WITHIN result is a valid `labels` for vv_mask_volume (VV_KEEP_FOREGROUND) and for another vv_distance_volume.
 *  6. EXACTNESS: every output word is exact and the same from run to run.  Nothing depends on the pitch of the source, on the 64-bit addressing
 *     build, on the launch geometry, on how the volume was loaded or on what `out` held.  No byte outside the box is read as data; no byte
 *     beyond 4 b_x b_y b_z of `out` is written.
 *  7. LIMITS: every extent of the box is at most 2048 (a line and its working arrays live in one block's LDS); the box holds at most 2^32 - 2
 *     voxels; sum_a (spacing_a (b_a - 1))^2, formed in 64 bits, is at most 0xFFFFFFFE, so every D(i) is below the no-seed marker.
 *  8. ALIASING: out == labels, the identical pointer, is allowed for host and for device buffers (a line is read completely by the one block
 *     that owns it before that block writes it).  Any other overlap of a device `out` with `labels` or with the context's linear volume
 *     allocation is refused.
 *  9. STREAM AND MEMORY (vv_label_volume's rule 8): labels and out are both host or both device pointers (on_device); device pointers must be
 *     4-byte aligned.  A device call allocates nothing: `out` is the only volume-sized working array and the call takes no scratch.  The call is
 *     three kernel launches, with no host read-back: `stream` NULL = the context's stream, the call returns when the work is complete; any other
 *     handle with device buffers only enqueues.  Host buffers are staged through device buffers of the call's own (out == labels: one buffer,
 *     uploaded and downloaded), released before it returns.  The context's volume, table, layout copies and residency state are not touched;
 *     vv_last_frame_ms keeps its value.
 * 10. Errors, in this order.  VV_ERR_INVALID: NULL ctx / d / out.  VV_ERR_NO_VOLUME: no volume loaded (for the labels sources too: the box is
 *     measured against the volume).  VV_ERR_INVALID, each in turn: a box outside vv_derive's rule 5; more than 2^32 - 2 voxels in the box; an
 *     extent above 2048; a seed outside its enum; VV_SEED_BINS with bins outside 0 <= bin_lo <= bin_hi <= 255; labels == NULL for a labels
 *     source or labels != NULL for VV_SEED_BINS; invert not 0 or 1; a spacing below 1; the distance bound of rule 7; an `out` mode outside its
 *     enum; capacity (bytes) below 4 b_x b_y b_z; a misaligned device pointer; an overlap that rule 8 refuses.  VV_ERR_NOMEM: a staging buffer
 *     could not be allocated.  A refused call writes nothing and leaves the context usable.                                                  */
#define VV_DISTANCE_MAX_EXTENT 2048
typedef enum { VV_SEED_BINS = 0, VV_SEED_LABEL = 1, VV_SEED_NONZERO = 2 } vv_seed;
typedef enum { VV_DIST_SQUARED = 0, VV_DIST_WITHIN = 1 } vv_dist_out;
typedef struct vv_distance {
    int      box_lo[3], box_hi[3];   /* as vv_label */
    int      seed;                   /* vv_seed */
    int      bin_lo, bin_hi;         /* VV_SEED_BINS: vv_label's rule 1 */
    uint32_t label;                  /* VV_SEED_LABEL */
    int      invert;                 /* 0 / 1: the seeds are the voxels where the test FAILS */
    int      spacing[3];             /* x, y, z voxel pitch as positive integers (1,1,1 = isotropic) */
    int      out;                    /* vv_dist_out */
    uint32_t within_r2;              /* VV_DIST_WITHIN */
} vv_distance;                       /* 64 bytes */
int  vv_distance_volume(vv_context *ctx, const vv_distance *d, const uint32_t *labels /* NULL for VV_SEED_BINS */,
                        uint32_t *out, size_t capacity, int on_device, void *stream);

/* ---- region measurements: one table row per region of a label volume, and consecutive labels 1..K (no reference counterpart) ----
 * vv_region_table measures what vv_label_volume, vv_mask_volume and vv_distance_volume segmented, where it lies, in HBM: every region's voxel count,
 * bounding box, coordinate moments, intensity range, surface faces and, with `aux` (e.g. the squared distances vv_distance_volume wrote), its thickness;
 * and it rewrites the sparse canonical labels (1 + least voxel index) as consecutive ones.  i, b, lo, hi are those of vv_label_volume's rule 4.
 *  1. REGIONS, VV_REGION_LABELS: voxel r is a ROOT iff labels[r] == r + 1.  Voxel i is OWNED by root r iff labels[i] != 0, r = labels[i] - 1 < voxels
 *     (voxels = b_x b_y b_z) and r is a root.  A voxel with labels[i] != 0 that is not owned is a STRAY.  The rule is total on any caller data, and no
 *     label ever makes an address unchecked; on what vv_label_volume wrote there are no strays.  K = the number of roots; the RANK of a root is the
 *     number of roots with a smaller index: rows are in ascending label order.
 *  2. VV_REGION_NONZERO: all voxels with labels[i] != 0 form one region whose label is 1 + the least such i; K is 1 or 0; there are no strays.  (How a
 *     VV_DIST_WITHIN or morphology result is measured.)
 *  3. COMPACT: compact[i] = rank + 1 of the owning root, 0 for background and strays.  Every word is written, whatever max_regions is.  A device
 *     `compact` may not overlap labels, aux, table or the context's linear volume allocation.
 *  4. TABLE: row k < min(K, max_regions) describes the region of rank k; rows at and beyond that are not written.  Every field is an integer or a
 *     bit-for-bit copy of a voxel: exact, and the same from run to run.  label: the region's label.  voxels: its voxel count.  lo, hi: its bounding box
 *     in VOLUME coordinates (box_lo + the box's coordinate), hi exclusive.  sum: the sums of x, y, z in volume coordinates (centroid = sum / voxels on
 *     the host).  sum2: the sums of xx, yy, zz, xy, xz, yz.  bin_min, bin_max, bin_sum, bin_sum2: over the classification index of
 *     vv_volume_histogram's rule 1.  vmin, vmax: as vv_histogram's rule 2 (integer keys compared, NaN excluded, +Inf / -Inf when there is none; u8:
 *     (float)byte).  faces[a]: the number of voxel faces of the region perpendicular to axis a whose neighbour across the face lies outside the box or
 *     is not owned by the same root (NONZERO: is 0), both directions counted; surface area = sum_a faces[a] pitch_b pitch_c on the host.  aux_sum,
 *     aux_max: the sum and the maximum of aux over the region; aux_argmax: the least box index i among the maxima; all three 0 without aux.  reserved: 0.
 *     OVERFLOW BOUNDS: with every volume coordinate of the box below 2^14 and fewer than 2^32 voxels in the box, sum < 2^46 and sum2 < 2^60: exact.
 *     (A volume with a longer axis is not refused: its sums are then taken modulo 2^64.)  aux_sum < 2^64 always: fewer than 2^32 words below 2^32.
 *  5. SUMMARY (optional): regions = K; written = min(K, max_regions); foreground = the number of non-zero labels; stray = the number of strays.
 *  6. What follows: (a) with labels from vv_label_volume, table[k].voxels == sizes[table[k].label - 1] and summary.regions == vv_label_stats.components.
 *     (b) The sum of voxels over a complete table is foreground - stray.  (c) Nothing depends on the pitch of the source, on the 64-bit addressing
 *     build, on the layout copies, on the launch geometry, on how the volume was loaded or on what the outputs held.  (d) No byte outside the box is read
 *     as data; no byte beyond 4 b_x b_y b_z of compact, sizeof(vv_region) * min(K, max_regions) of table and sizeof(vv_region_summary) of summary is written.
 *  7. STREAM AND MEMORY (vv_label_volume's rule 8): labels, aux, compact, table and summary are all host pointers or all device pointers (on_device).
 *     Device labels, aux and compact must be 4-byte aligned, device table and summary 8-byte aligned.  A device call allocates nothing: the chunk
 *     counters live in scratch the context holds from vv_init on (keep enqueue-only calls of one context on one stream).  The call is five kernel
 *     launches whatever the data, with no host read-back: `stream` NULL = the context's stream, the call returns when the work is complete; any other
 *     handle with device buffers only enqueues.  Host buffers are staged through device buffers of the call's own (labels and aux as inputs; a host
 *     table is uploaded first, so the rows that are not written keep the caller's bytes), released before it returns.  The context's volume, table,
 *     layout copies and residency state are not touched; vv_last_frame_ms keeps its value.
 *  8. Errors, in this order.  VV_ERR_INVALID: NULL ctx / d / labels / compact.  VV_ERR_NO_VOLUME: no volume loaded (the box is measured against the
 *     volume, and the intensity fields read it).  VV_ERR_INVALID, each in turn: a box outside vv_derive's rule 5 or above 2^32 - 2 voxels; a source
 *     outside its enum; table == NULL with max_regions != 0; compact_capacity (bytes) below 4 b_x b_y b_z; table_capacity (bytes) below
 *     sizeof(vv_region) * max_regions, formed in 64 bits; a misaligned device pointer; a device compact whose byte range overlaps labels, aux, table or
 *     the context's linear volume allocation, or a device table that overlaps labels, aux or that allocation.  VV_ERR_NOMEM: a staging buffer could
 *     not be allocated.  A refused call writes nothing and leaves the context usable.                                                          */
typedef enum { VV_REGION_LABELS = 0, VV_REGION_NONZERO = 1 } vv_region_source;
typedef struct vv_regions {
    int      box_lo[3], box_hi[3];   /* the box the labels were made for (as vv_label) */
    int      source;                 /* vv_region_source */
    uint32_t max_regions;            /* rows of `table` */
} vv_regions;                        /* 32 bytes */
typedef struct vv_region {
    uint32_t label;                     /*   0 */
    uint32_t reserved;                  /*   4: written as 0 */
    unsigned long long voxels;          /*   8 */
    int      lo[3], hi[3];              /*  16, 28: volume coordinates, hi exclusive */
    unsigned long long sum[3];          /*  40: x, y, z */
    unsigned long long sum2[6];         /*  64: xx, yy, zz, xy, xz, yz */
    uint32_t bin_min, bin_max;          /* 112, 116 */
    unsigned long long bin_sum, bin_sum2;   /* 120, 128 */
    float    vmin, vmax;                /* 136, 140 */
    unsigned long long faces[3];        /* 144: faces perpendicular to x, y, z */
    unsigned long long aux_sum;         /* 168 */
    uint32_t aux_argmax;                /* 176: with aux_max one 8-byte slot (the kernels keep aux_max << 32 | (0xFFFFFFFF - i) there and take its maximum) */
    uint32_t aux_max;                   /* 180 */
} vv_region;                            /* 184 bytes, 8-byte aligned */
typedef struct vv_region_summary {
    unsigned long long regions, written, foreground, stray;
} vv_region_summary;                    /* 32 bytes */
int  vv_region_table(vv_context *ctx, const vv_regions *d, const uint32_t *labels, const uint32_t *aux /* or NULL */,
                     uint32_t *compact, size_t compact_capacity, vv_region *table /* or NULL with max_regions == 0 */, size_t table_capacity,
                     vv_region_summary *summary /* or NULL */, int on_device, void *stream);

/* ---- surface meshes: the surface-nets quads of a level or of a segmentation, indexed, in HBM (no reference counterpart) ----
 * vv_surface_mesh gives the surface that vv_render_iso shows, or the boundary of what vv_label_volume, vv_distance_volume or vv_region_table
 * segmented, as geometry: one vertex per grid cell the surface crosses, one quad per grid edge it crosses (naive surface nets).  Vertices are shared
 * by construction and both outputs have a canonical order, so every output word, floats included, is a property of the input alone.  b, lo, hi and i
 * are those of vv_label_volume's rule 4.
 *  1. FIELD: every voxel of the box has an integer g in 0..255, the call a level in 1..255; a voxel is INSIDE iff g >= level.  VV_MESH_INDEX: g is the
 *     classification index of vv_volume_histogram's rule 1 (the byte of a u8 voxel; a NaN gives 0, +Inf 255), level the descriptor's.  VV_MESH_BINS:
 *     g = 1 iff bin_lo <= bin <= bin_hi, else 0.  VV_MESH_LABEL: g = (labels[i] == label).  VV_MESH_NONZERO: g = (labels[i] != 0).  The three binary
 *     sources have level 1 and ignore the descriptor's.  `labels` is what vv_label_volume, vv_distance_volume (VV_DIST_WITHIN) or vv_region_table
 *     (compact) wrote for the box; NULL for the first two sources.
 *  2. BOX AND CAP: voxels outside the box do not exist.  cap = 1 surrounds the box with one layer of virtual voxels with g = 0, which are never loaded
 *     from anywhere: the surface closes at the box's faces.  cap = 0 leaves it open there.  The SITE grid has extents m_a = b_a - 1 + 2 cap, which may
 *     be 0 (vv_mesh_dims); site s = (s_x, s_y, s_z) has the number j = (s_z m_y + s_y) m_x + s_x and is the cell whose eight corner voxels are the box
 *     voxels s - cap + (dx, dy, dz), d in {0, 1}^3.
 *  3. EDGES of a cell: e = 4 a + db + 2 dc for the axis a in (x, y, z) = (0, 1, 2) with (a, b, c) cyclic: the edge along a from corner p (offset 0 on
 *     a, db on b, dc on c) to corner q = p + e_a.  It is ACTIVE iff exactly one of p, q is inside.  Its crossing lies at
 *     t = (float)(2 level - 1 - 2 g_p) / (float)(2 (g_q - g_p)) from p: one IEEE binary32 division of two exactly represented integers of equal sign.
 *     0 < t < 1 always, t = 0.5 for the binary sources: the surface is at level - 1/2, no crossing sits on a voxel.
 *  4. VERTICES: a site is ACTIVE iff its corners are not all inside and not all outside (iff it has an active edge).  The active sites in ascending j
 *     are the vertices 0..V-1.  S_k = the binary32 sum over the active edges, in the order e = 0..11, of the crossing's offset on axis k (t on the
 *     edge's own axis, else its db or dc as 0.0f / 1.0f); n = the number of active edges; the coordinate is (float)(lo_k + s_k - cap) + S_k / (float)n
 *     (one division, one addition; no expression holds a multiplication), in volume voxel coordinates.  vv_mesh_vertex: x, y, z, site = j.  The
 *     optional vv_mesh_normal at the same rank: g[k] = the sum of g over the four corners at offset 0 on axis k minus the sum over the four at offset
 *     1 (an exact integer, unnormalised, pointing out of the inside); edges = the 12-bit mask of the active edges.
 *  5. INDEX: index[j] = vertex number + 1 at active sites, 0 elsewhere.  Every word (4 m_x m_y m_z bytes) is written whatever the maxima are.  index
 *     == NULL is allowed only with max_vertices == 0 && max_quads == 0: a COUNT-ONLY call, which writes the summary alone.
 *  6. QUADS: for each axis a, site s OWNS the edge along a that ends at its corner (1, 1, 1).  The owned edge EMITS iff it is active and s_b + 1 < m_b
 *     and s_c + 1 < m_c (the four sites around it exist; with cap = 1 every active edge of the padded grid emits exactly once).  The quads in
 *     ascending (j, a) are the quads 0..Q-1.  With c0 = s, c1 = s + e_b, c2 = s + e_b + e_c, c3 = s + e_c the record is the vertex numbers of
 *     (c0, c1, c2, c3) if the edge's lower end p is inside, else of (c0, c3, c2, c1): four uint32, 0-based, counter-clockwise seen from outside.
 *  7. CAPACITIES: the vertex and normal records of rank < max_vertices and the quad records of rank < max_quads are written, nothing beyond them
 *     (`normals` holds as many records as `vertices`).  A written quad may name a vertex of rank >= max_vertices.  vv_mesh_summary (optional):
 *     vertices = V, quads = Q, written_vertices = min(V, max_vertices), written_quads = min(Q, max_quads).  Intended use: a count-only call, an
 *     allocation, the full call.
 *  8. What follows: (a) with cap = 1 every directed edge (u, v) of the quads occurs as often as (v, u): the mesh is closed and consistently oriented;
 *     no undirected edge is used more than 4 times.  (b) With cap = 1 and a binary source, Q = the number of voxel faces between an inside voxel and
 *     an outside or non-existent one (VV_MESH_NONZERO: faces[0] + faces[1] + faces[2] of vv_region_table's VV_REGION_NONZERO row).  (c) The cap = 0
 *     mesh is the sub-mesh of the cap = 1 mesh on the sites whose eight corners are real, with the same coordinates.  (d) A box entirely inside gives
 *     V = prod(b_a + 1) - prod(b_a - 1), Q = 2 (b_x b_y + b_y b_z + b_x b_z) with cap = 1 and nothing with cap = 0.  (e) Nothing depends on the pitch,
 *     the 64-bit addressing build, the layout copies, the launch geometry, the load path or what the outputs held.  (f) No byte outside the box is
 *     read as data.
 *  9. LIMITS: the box holds at most 2^32 - 2 voxels, the site grid at most 2^32 - 2 sites; quad ranks and the summary are formed in 64 bits.
 * 10. STREAM AND MEMORY (vv_region_table's rule 7): all buffers are host pointers or all device pointers (on_device).  Device labels and index must be
 *     4-byte aligned, vertices, normals and quads 16-byte aligned, summary 8-byte aligned.  A device call allocates nothing: the chunk partials live
 *     in scratch the context holds from vv_init on.  The call is four kernel launches (count, scan, vertices, quads), two for a count-only call,
 *     whatever the data, with no host read-back.  Host buffers are staged through device buffers of the call's own; the tables go up before they come
 *     down, so the records that are not written keep the caller's bytes.  The context's volume, table, layout copies and residency state are not
 *     touched; vv_last_frame_ms keeps its value.
 * 11. Errors, in this order.  VV_ERR_INVALID: NULL ctx / d.  VV_ERR_NO_VOLUME: no volume loaded.  VV_ERR_INVALID, each in turn: a box outside
 *     vv_derive's rule 5 or above 2^32 - 2 voxels; more than 2^32 - 2 sites; a source outside its enum; VV_MESH_INDEX with a level outside 1..255;
 *     VV_MESH_BINS with bins outside 0 <= bin_lo <= bin_hi <= 255; labels == NULL for a labels source or != NULL for the other two; cap not 0 or 1;
 *     index == NULL with a non-zero maximum; vertices == NULL with max_vertices != 0; quads == NULL with max_quads != 0; a capacity (bytes, formed in
 *     64 bits: 4 per site of a given index, 16 per record) below what it must hold; a misaligned device pointer; a device output that overlaps
 *     another buffer of the call or the context's linear volume allocation.  VV_ERR_NOMEM: a staging buffer could not be allocated.  A refused call
 *     writes nothing and leaves the context usable.                                                                                              */
typedef enum { VV_MESH_INDEX = 0, VV_MESH_BINS = 1, VV_MESH_LABEL = 2, VV_MESH_NONZERO = 3 } vv_mesh_source;
typedef struct vv_mesh {
    int      box_lo[3], box_hi[3];   /* as vv_label */
    int      source;                 /* vv_mesh_source */
    int      level;                  /* VV_MESH_INDEX: 1..255 */
    int      bin_lo, bin_hi;         /* VV_MESH_BINS: vv_label's rule 1 */
    uint32_t label;                  /* VV_MESH_LABEL */
    int      cap;                    /* 0 / 1 */
    uint32_t max_vertices, max_quads;    /* records of `vertices` (and `normals`) / of `quads` */
} vv_mesh;                           /* 56 bytes */
typedef struct vv_mesh_vertex { float x, y, z; uint32_t site; } vv_mesh_vertex;      /* 16 bytes */
typedef struct vv_mesh_normal { int32_t g[3]; uint32_t edges; } vv_mesh_normal;      /* 16 bytes */
typedef struct vv_mesh_summary {
    unsigned long long vertices, quads, written_vertices, written_quads;
} vv_mesh_summary;                   /* 32 bytes */
int  vv_mesh_dims(const vv_context *ctx, const vv_mesh *d, int dims[3]);   /* host only; m_a = b_a - 1 + 2 cap (the box, the cap) */
int  vv_surface_mesh(vv_context *ctx, const vv_mesh *d, const uint32_t *labels /* NULL for VV_MESH_INDEX / VV_MESH_BINS */,
                     uint32_t *index /* or NULL: count only */, size_t index_capacity,
                     vv_mesh_vertex *vertices, size_t vertices_capacity, vv_mesh_normal *normals /* or NULL */,
                     uint32_t *quads, size_t quads_capacity, vv_mesh_summary *summary /* or NULL */, int on_device, void *stream);

/* The first pass on its own (firstpass.vert:6, firstpass.frag:4, glwidget.cpp:198-228): the
 * RGBA8 images the reference's two FBOs would hold for this camera -- cube-space entry (front
 * faces) and exit (back faces) positions, UNORM8-rounded, alpha 255 where a face is visible and
 * the clear colour (0,0,0,0) elsewhere.  A host without GL can feed them to VV_RAYS_IMAGES.
 * rays must be VV_RAYS_ANALYTIC.  Images are img_w x img_h x 4 bytes, row 0 = bottom.        */
int  vv_first_pass(vv_context *ctx, int img_w, int img_h, const struct camera_params *camera,
                   const vv_ray_source *rays, uint8_t *front_rgba, uint8_t *back_rgba,
                   int out_on_device, void *stream);

/* Cutting plane of the canonical slice views (GLWidget::setSliceCanonical, glwidget.cpp:743-788)
 * and the orientation rule applied before the plane goes into slice_params (glwidget.cpp:243-258:
 * the normal is negated when flip_cross_section && n.y < -1e-6, or !flip && n.y > 1e-6).       */
int  vv_cut_plane_canonical(int orientation, float displace, float point[3], float normal[3]);
/* Cutting plane of the free-form ("pro") slice view: Window::renderSlice's PRO_SLICING branch (window.cpp:425-443), which hands
 * GLWidget::setSlicePro (glwidget.cpp:743-755)  point = (dx, dy, dz) + .5  and  normal = T(.5) Rx(theta) Ry(phi) Rz(psi) T(-.5) (0,0,1,0),
 * binary32 with the operation order of cs123math (bit-identical to the compiled reference: tests/golden/cut_planes_pro.json).  Host-only. */
int  vv_cut_plane_from_euler(float dx, float dy, float dz, float theta, float phi, float psi, float point[3], float normal[3]);
int  vv_cut_plane_to_slice_params(int slice_type, const float point[3], const float normal[3],
                                  int flip_cross_section, struct slice_params *out);

/* Camera / cutting-plane controls of the 3D view (host-only arithmetic, no device work).
 * The reference does these with Qt 4 value types (float-stored QVector3D read back as qreal,
 * double QMatrix4x4) inside its mouse handlers; Qt is not available to pin them bit for bit, so
 * they are restated in double precision on float inputs/outputs and tested to 1e-5.
 *   vv_camera_orbit_drag    right-button drag (glwidget.cpp:432-446): spherical orbit about the
 *                           origin, theta clamped to [0.1, pi-0.1], look re-aimed at the origin
 *   vv_camera_zoom          wheel (glwidget.cpp:607-620): position += look * delta/200
 *   vv_cut_plane_from_drag  left-button drag released (glwidget.cpp:482-535): the plane through the
 *                           eye ray of the release point and the near-plane point of the press
 *                           point; window coordinates are fractions of the widget (y down);
 *                           point comes back in cube space [0,1]^3, normal un-normalised as in
 *                           the reference; perspective(45 deg, aspect, 0.1, 100) (glwidget.cpp:338)
 *   vv_cut_plane_drag       middle-button drag of such a plane (glwidget.cpp:447-452)          */
int  vv_camera_orbit_drag(const float position[3], int dx, int dy, float out_position[3], float out_look[3]);
int  vv_camera_zoom(const float position[3], const float look[3], int delta, float out_position[3]);
int  vv_cut_plane_from_drag(const float position[3], const float look[3], const float up[3], float aspect,
                            const float press[2], const float release[2],
                            float point[3], float normal[3], float plane_up[3], float plane_right[3]);
int  vv_cut_plane_drag(float point[3], const float plane_up[3], const float plane_right[3],
                       int dx, int dy, int width, int height);

/* Slice buffer -> the BGRA image SliceWidget shows (slicewidget.cpp:108-121): grey value
 * (unsigned)(f*255), alpha 255, written mirrored at bits[size - offset] with offset = j*height+i;
 * bits[0] and elements whose index falls outside stay untouched.  bgra: width*height*4 bytes. */
int  vv_slice_to_bgra(const float *slice, size_t height, size_t width, uint8_t *bgra);

/* Slice transform of the free-form slice view: SliceWidget::getTransformationMatrix
 * (slicewidget.cpp:147-165) = T(+.5) T(dx,dy,dz) Rx(theta) Ry(phi) Rz(psi) T(-.5),
 * binary32, row-major, multiplied left to right (cs123math/CS123Matrix.cpp:27-62).
 * Angles must lie in [-3.2, 3.2) (the reference asserts this).  Host-only.       */
int  vv_slice_matrix(float dx, float dy, float dz, float theta, float phi, float psi,
                     float out[16]);

/* ---- procedural generator: replaces VolumeGenerator::drawEllipsoid / drawDefaultBrain
 * (volumegenerator.cpp:31-119).  One fused pass applies the n ellipsoids in order
 * to a zero-filled volume, bit-identical to n successive drawEllipsoid calls.
 * out: nx*ny*nz bytes (host or device).                                          */
int  vv_generate_ellipsoids(vv_context *ctx, uint8_t *out, int out_on_device,
                            int nx, int ny, int nz, int n,
                            const float *centers /* n*3 */, const float *axes /* n*3 */,
                            const uint8_t *colors /* n */, void *stream);
/* One drawEllipsoid call (volumegenerator.cpp:31-97) applied IN PLACE to an existing volume:
 * voxels outside the ellipsoid keep their value, the marker slab fi >= 0.99 is set to 4. */
int  vv_draw_ellipsoid(vv_context *ctx, uint8_t *vol, int vol_on_device,
                       int nx, int ny, int nz, const float center[3], const float axes[3],
                       uint8_t color, void *stream);
int  vv_generate_default_brain(vv_context *ctx, uint8_t *out, int out_on_device,
                               int nx, int ny, int nz, void *stream);
/* u8 -> f32 promotion v/255 on the device (build extension for f32 configs). */
int  vv_promote_u8_to_f32(vv_context *ctx, const uint8_t *dev_in, float *dev_out,
                          size_t n, void *stream);
/* Synthetic "noise" volume V2 of the measurement plan: smooth hash field. */
int  vv_generate_noise_u8(vv_context *ctx, uint8_t *dev_out, int nx, int ny, int nz,
                          uint32_t seed, void *stream);

/* ---- transfer-function presets: transfer_functions.h:4-9 as closed forms -------- */
typedef enum { VV_TF_ENGINE = 0, VV_TF_HEAD = 1, VV_TF_MRI = 2 } vv_tf_preset;
int  vv_transfer_preset(int preset, float tf_out[1024]);

/* ---- dataset presets: the rule of GLWidget::loadVolume (glwidget.cpp:678-689) ----
 * The reference picks the transfer table and the object scale from the file name's ending:
 *     "engine.t3d"  -> g_transferEngine, scale (1, 1, 1)        "head.t3d" -> g_transferEngine, scale (1, 1, 0.8)
 *     "VisMale.t3d" -> g_transferHead,   scale (1.57, 1, 1)
 * Returns 1 and fills *tf_preset (a vv_tf_preset) and scale[3] when a rule matches; returns 0 and leaves both
 * untouched otherwise (the reference then reads an uninitialised table pointer and keeps the previous scale: the
 * caller's current table and scale are this library's reading of that); VV_ERR_INVALID (< 0) for NULL arguments.
 * Case-sensitive suffix match, as QString::endsWith. */
int  vv_dataset_preset(const char *path, int *tf_preset, float scale[3]);

/* ---- .t3d container (volumegenerator.cpp:147-220): 3 x u64 LE header + bytes ---- */
int  vv_t3d_read_header(const char *path, int header, int *nx, int *ny, int *nz);
int  vv_t3d_read (const char *path, int header, uint8_t *dst, size_t capacity);
int  vv_t3d_write(const char *path, int header, const uint8_t *src, int nx, int ny, int nz);

/* ---- optional second layouts of the loaded volume (no reference counterpart: cudaArray hides its layout) -----------------------
 * Which copy a frame samples is a launch-policy decision; results never depend on it.
 *   VV_LAYOUT_BRICKED  4x4x4-voxel bricks with an x halo (1.25x an f32 volume, 2x a u8 volume): frames whose screen x direction is more
 *                      than ~14 degrees off the volume's x and z axes; volumes of 2 M voxels and more
 *   VV_LAYOUT_ZFAST    rows along z (1x the volume, both voxel types): side views (screen x within ~14 degrees of the volume's z axis).
 *                      Preparing it also builds the x-pair copy (2x) where the policy would sample it (unshaded side views of u8 volumes
 *                      and of f32 volumes up to 512 MiB)
 *   VV_LAYOUT_ZPAIR    {v(z), v(z+1)} records (2x the volume): unshaded frames along the x axis, f32 up to 512 MiB, u8 up to 2 GiB
 *   VV_LAYOUT_POLICY   every copy of the above that vv_render's policy can pick for the loaded volume
 * RESIDENCY.  All copies together stay within a budget: by default the larger of 8 GiB and 2.5 x the linear volume (C3's 4.3 GB volume: the
 * bricked + z-fastest copies, 9.7 GB; C5's 32 GiB volume: 72 GiB), vv_set_layout_policy changes it.  A copy that does not fit evicts the
 * copies sampled least recently; if that is not enough it is not built and frames take the next layout of the policy (at worst the linear
 * volume).  By default vv_render builds a missing copy on the first frame that wants it: a kernel over the volume (1024^3 f32: bricked 4.2 ms,
 * z-fastest 2.5 ms; x 8 at 2048^3), a hipMalloc and a stream synchronisation -- also inside an enqueue-only call.  A host that must not
 * stall in its paint loop calls vv_prepare_layouts(VV_LAYOUT_POLICY) after loading (the mirror's cudaLoadVolume and PaintLoop::loadVolume
 * do) and may switch building in vv_render off (build_in_render = 0): frames then sample what is resident.
 * All copies are dropped when another volume is loaded.
 * vv_prepare_layouts returns the bit mask of the requested layouts that are resident afterwards, or a negative vv_status.               */
enum { VV_LAYOUT_BRICKED = 1, VV_LAYOUT_ZPAIR = 2, VV_LAYOUT_ZFAST = 4, VV_LAYOUT_POLICY = 256 };
int  vv_prepare_layouts(vv_context *ctx, int which, void *stream);
int  vv_set_layout_policy(vv_context *ctx, unsigned long long budget_bytes /* 0 = default */, int build_in_render /* default 1 */);
/* out = { linear volume, bricked, z-pair, z-fastest, x-pair copy (bytes; 0 = not resident), budget for the copies, copies built inside
 *         vv_render since the volume was loaded, build_in_render } */
int  vv_layout_state(const vv_context *ctx, unsigned long long out[8]);
/* Device memory held by the context: out[0] linear volume, [1] bricked copy, [2] z-pair + z-fastest + x-pair copies,
 * [3] tables and scratch (bytes). */
int  vv_device_bytes(const vv_context *ctx, unsigned long long out[4]);

/* ---- metrics (the reference only has a clock() overlay) ---------------- */
float              vv_last_frame_ms(const vv_context *ctx);      /* hipEvent time of the last vv_render / vv_render_mip / vv_render_iso / vv_render_projection (-1: not timed) */
/* Every vv_render brackets its kernels with two hipEventRecord (what vv_last_frame_ms reads): two more packets the stream has to retire per
 * frame, ~2-4 us each back to back.  A host that times whole runs itself (bench.py) or does not time at all switches them off (on = 0);
 * vv_last_frame_ms then returns -1.  Default: on, the reference's lastRenderTime overlay (glwidget.cpp:288-293) wants it. */
int                vv_set_frame_timing(vv_context *ctx, int on);
unsigned long long vv_last_sample_count(vv_context *ctx);        /* executed samples, if count_samples */
int                vv_debug_last_launch(vv_context *ctx, int out[8]);  /* what the launch policy chose for the last vv_render (developer aid): wave tile log2 width,
                                                                       * block log2 width, samples per trip, LDS reserve, layout (0 linear, 1 linear/64-bit, 2 bricked,
                                                                       * 3 z-pair, 4 z-fastest, 5 x-pair), view known to the policy (0 / 1), density x 1000, kernel family (0 unshaded, 1 Phong, 2 MIP: vv_render_mip, 3 isosurface: vv_render_iso, 4 projection: vv_render_projection) */
/* A resident layout as it lies in HBM (developer aid; what tests/test_footprint.py holds the copy builders and the touched_lines instrument to).
 * `layout`: the codes of vv_debug_last_launch (0 and 1 name the same allocation).  geom = {allocation bytes, the zeroed bytes behind the layout
 * included, or 0 when the layout is not resident; row stride; slice stride; nx; ny; nz; voxel type; 0}, the strides being the fields the kernels
 * address with: row_bytes / slice_bytes of the linear layout, bytes per row of bricks / bytes per layer of bricks in 64-byte units, bytes per row /
 * per slab of records of a pair copy, bytes per row / per slice of the z-fastest copy.  The allocation is then copied to host_dst (`capacity` bytes),
 * synchronously on the context's stream; host_dst NULL with capacity 0 asks for the geometry alone.  Builds nothing and changes no state.
 * Errors: NULL ctx / geom, a layout outside 0..5, a capacity below geom[0]: VV_ERR_INVALID; no volume: VV_ERR_NO_VOLUME.   */
int                vv_debug_read_layout(vv_context *ctx, int layout, unsigned long long geom[8], void *host_dst, size_t capacity);
/* The rectangle of pixel coordinates (x_min, x_max, y_min, y_max, margin included) outside of which vv_render lets its pre-pass write (0,0,0,0) instead of
 * marching (analytic ray sources): returns 1 and fills out[4], or 0 when this camera gets no rectangle (a cube corner at or behind the eye's plane, a
 * margin wider than the frame).  Needs no device and no context: tests/test_host.py checks it against the oracle's ray-box test pixel by pixel. */
int                vv_debug_screen_rect(int width, int height, const struct camera_params *cam, const vv_ray_source *rays, double out[4]);
int                vv_debug_counters(vv_context *ctx, unsigned long long out[16]);  /* developer statistics of the last instrumented frame: [0] executed samples,
                                                                                     * [1] lane slots spent, [2] / [3] waves that sampled the bricked / a pair copy */
/* The radius pre-pass of unshaded frames (vv_render without Phong shading, vv_render_mip, vv_render_iso, vv_render_projection).  Its results -- one
 * radius per 14 x 14 pixel slab and, where the launch policy asks for one, the tile order table -- are a pure function of the arguments it is launched
 * with: the frame's parameters (camera, frame size, steps, slice plane, shard, row range, ...), the screen rectangle, the tile grid, the two buffers,
 * the stream and the device.  The context keeps those arguments as bytes.  A frame with an analytic ray source whose arguments are byte-identical to
 * those of the last pre-pass launches none: a host that keeps the view and changes the transfer function, or redraws on a timer, pays for the march
 * alone.  Frames with an image ray source always launch (the images may change under the same pointers), and so does the first frame after a volume
 * load, vv_reread_env, a failed frame, a frame on another stream, and a frame that made the context's radius / order buffers grow.  Phong frames have
 * no such pre-pass and neither use nor disturb it.  The (0,0,0,0) pixels beside the volume's screen rectangle of a composite unshaded frame are
 * written by blocks appended to the march launch, which fill the slots its last marching blocks leave empty.  No pixel depends on either.
 * The reuse relies on the stream's order: the earlier pre-pass has run, on that stream, before the later march.  A frame issued while its stream
 * is being captured into a graph therefore always records its own pre-pass and leaves nothing to reuse; a host that REPLAYS captured frames between
 * live ones (a replay rewrites the radii at a time the library does not see), or that destroys a stream and goes on with a new one, calls
 * vv_reread_env in between or runs with VV_RAD_REUSE=0.
 *   VV_RAD_REUSE=0   the pre-pass is launched on every frame
 *   VV_TAIL_FILL=0   the pre-pass writes those pixels, as it does for frames in which nothing marches; it then runs on every frame that has any
 * out = { pre-passes launched since the context was created, frames that reused the last one's results, whether the last frame did (0 / 1),
 *         the fill blocks of the last frame's march launch }  (developer aid; tests/test_prepass.py) */
int                vv_debug_prepass_state(vv_context *ctx, int out[4]);
/* The VV_* developer knobs of the environment are read when a context is created and at every volume load, never
 * per frame; this reads them again (tests that flip a knob between two frames of one volume). */
int                vv_reread_env(vv_context *ctx);
int                vv_volume_dims(const vv_context *ctx, int dims[3], int *voxel_type);

#ifdef __cplusplus
}
#endif
#endif /* VOLVIZ_H */
