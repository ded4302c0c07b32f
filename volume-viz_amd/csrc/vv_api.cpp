// vv_api.cpp -- the C-ABI of include/volviz.h over the HIP kernels.
//
// Replaces the host half of kernel.cu (initCuda/registerCudaResources/runCuda/
// cudaLoadVolume, kernel.cu:369-498; invoke_*_slice_kernel, kernel.cu:506-541).
// There is no CPU fallback: every entry point that computes needs a HIP device and
// fails with VV_ERR_DEVICE otherwise.
#include "../../include/volviz.h"
#include "vv_kernels.h"
#include "vv_gate.h"

#include <cassert>
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

using namespace vv;

// Developer / experiment knobs (VV_* environment variables).  Read when the context is created and again at every
// volume load -- never on the per-frame path.
struct vv_knobs {
    int tile_log2w = -1, xcd_band = -1, unroll = -1, lds_reserve = -1, lds_reserve_phong = -1;
    int bricked = -1, zpair = -1, zfast = -1, force_big = 0;
    int block_w = -1, tail = -1, rect = -1, lpt = -1, lpt_run = -1, phong_bricks = -1;
    int rad_reuse = -1;                     // VV_RAD_REUSE=0: the radius pre-pass is launched on every frame (issue_prepass)
    int tail_fill = -1;                     // VV_TAIL_FILL=0: the zeros beside the rectangle stay with rad_kernel (no fill blocks in the march launch)
    int hist_blocks = -1;                   // VV_HIST_BLOCKS: cap on hist_kernel's grid (tests drive its grid-stride loop with it)
    int derive_blocks = -1;                 // VV_DERIVE_BLOCKS: the same for derive_kernel
    int stencil_blocks = -1;                // VV_STENCIL_BLOCKS: the same for the stencil kernels (their loop over (tile, z segment) items)
    int resample_blocks = -1;               // VV_RESAMPLE_BLOCKS: the same for resample_kernel (its loop over tiles)
    int label_blocks = -1;                  // VV_LABEL_BLOCKS: the same for the label kernels and mask_kernel (tests vary the block order with it)
    int label_phases = -1;                  // VV_LABEL_PHASES = 1 / 2 / 3: vv_label_volume stops behind its local / merge / flatten launch (tools/time_label.py times the
                                            // launches by difference; the outputs are then unfinished)
    int distance_blocks = -1;               // VV_DISTANCE_BLOCKS: cap on the grids of the distance kernels (tests vary the block order with it)
    int distance_phases = -1;               // VV_DISTANCE_PHASES = 1 / 2: vv_distance_volume stops behind its x / y launch (tools/time_distance.py, as VV_LABEL_PHASES)
    int region_blocks = -1;                 // VV_REGION_BLOCKS: cap on the grids of the region kernels (tests vary the block order with it)
    int region_chunks = -1;                 // VV_REGION_CHUNKS: lowers the cap on the chunks of a call (small test boxes reach the long-chunk path with it)
    int region_phases = -1;                 // VV_REGION_PHASES = 1..4: vv_region_table stops behind that launch (tools/time_regions.py, as VV_LABEL_PHASES)
    int mesh_blocks = -1;                   // VV_MESH_BLOCKS: cap on the grids of the mesh kernels (tests vary the block order with it)
    int mesh_chunks = -1;                   // VV_MESH_CHUNKS: lowers the cap on the chunks of a call (small test boxes reach the long-chunk path with it)
    int mesh_phases = -1;                   // VV_MESH_PHASES = 1..3: vv_surface_mesh stops behind that launch (tools/time_mesh.py, as VV_LABEL_PHASES)
    // finalize_layout: VV_PITCH_PAD = bytes of row padding (0 or anything that is no number: rows stay dense; not a multiple of 16 in 16..4096: the default),
    // VV_PITCH_FORCE (set: any row length is padded), VV_PITCH_ROWS = extra rows per slice (0..64, anything else: the default)
    int pitch_pad = 32, pitch_rows = -1; bool pitch_force = false;
    static int geti(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
    void read()
    {
        tile_log2w = geti("VV_TILE_LOG2W", -1); xcd_band = geti("VV_XCD_BAND", -1); unroll = geti("VV_UNROLL", -1);
        lds_reserve = geti("VV_LDS_RESERVE", -1); lds_reserve_phong = geti("VV_LDS_RESERVE_PHONG", -1);
        bricked = geti("VV_BRICKED", -1); zpair = geti("VV_ZPAIR", -1);
        block_w = geti("VV_BLOCK_W", -1); tail = geti("VV_TAIL", -1);
        zfast = geti("VV_ZFAST", -1); force_big = getenv("VV_FORCE_BIG") != nullptr;
        rect = geti("VV_RECT", -1); lpt = geti("VV_LPT", -1); lpt_run = geti("VV_LPT_RUN", -1); phong_bricks = geti("VV_PHONG_BRICKS", -1);
        rad_reuse = geti("VV_RAD_REUSE", -1); tail_fill = geti("VV_TAIL_FILL", -1);
        hist_blocks = geti("VV_HIST_BLOCKS", -1); derive_blocks = geti("VV_DERIVE_BLOCKS", -1);
        stencil_blocks = geti("VV_STENCIL_BLOCKS", -1); resample_blocks = geti("VV_RESAMPLE_BLOCKS", -1);
        label_blocks = geti("VV_LABEL_BLOCKS", -1); label_phases = geti("VV_LABEL_PHASES", -1);
        distance_blocks = geti("VV_DISTANCE_BLOCKS", -1); distance_phases = geti("VV_DISTANCE_PHASES", -1);
        region_blocks = geti("VV_REGION_BLOCKS", -1); region_chunks = geti("VV_REGION_CHUNKS", -1); region_phases = geti("VV_REGION_PHASES", -1);
        mesh_blocks = geti("VV_MESH_BLOCKS", -1); mesh_chunks = geti("VV_MESH_CHUNKS", -1); mesh_phases = geti("VV_MESH_PHASES", -1);
        const int pad = geti("VV_PITCH_PAD", 32);
        pitch_pad = pad <= 0 ? 0 : ((pad >= 16 && pad <= 4096 && pad % 16 == 0) ? pad : 32);
        pitch_force = getenv("VV_PITCH_FORCE") != nullptr; pitch_rows = geti("VV_PITCH_ROWS", -1);
    }
};

// The optional copies of the loaded volume, built on first use and dropped on reload: bricked (views off the memory axis),
// z-pair (views along the memory axis), z-fastest (side views) and x-pair (side views of small / u8 volumes; built from the z-fastest copy).
enum { CP_BRICKS = 0, CP_ZPAIR = 1, CP_ZFAST = 2, CP_XPAIR = 3, CP_N = 4 };
struct layout_copy {
    void *ptr = nullptr; size_t bytes = 0;
    size_t alloc = 0;                       // bytes + the zeroed bytes behind them (vv_debug_read_layout)
    bool valid = false, failed = false;     // failed: not tried again until the next volume load (or an explicit vv_prepare_layouts)
    unsigned long long last_used = 0;       // when a frame last sampled it (the least recently used copy is evicted first)
    // what the sampler needs (VolumeView): bytes per row and per slab (pair copies), per row and per slice (z-fastest), per brick row and per brick layer / 64
    uint32_t row = 0; uint64_t slab = 0;
};

// The context's scratch buffers: device memory that a call grows to what it needs and the next call reuses.
enum {
    SC_RAD,         // frames: one radius per slab (rad_kernel -> march kernels)
    SC_ORDER,       // frames: StripMap::order of the frame in flight
    SC_FRAME,       // RGBA image of a host-buffer frame / of vv_classify_indices
    SC_INDEX,       // index image of a host-buffer MIP / iso / projection frame, of vv_classify_indices and of vv_histogram_indices
    SC_HIT,         // iso: hit records of a host-buffer frame
    SC_STAT,        // projection: stat records of a host-buffer frame
    SC_IMG,         // the two first-pass images: of a host image ray source, of a host-buffer vv_first_pass
    SC_SLICE,       // the image of a host-buffer slice, both images of a slab slice
    SC_GEN,         // per-axis tables of the ellipsoid generator
    SC_TF_ARG,      // vv_classify_indices: the caller's table
    SC_LABEL,       // vv_label_volume: the kernels' counters, then the vv_label_stats of a host-output call (kLabelScratchBytes, held from vv_init on)
    SC_REGION,      // vv_region_table: the header counters, the chunk partials, then the vv_region_summary of a host call (kRegionScratchBytes, held from vv_init on)
    SC_MESH,        // vv_surface_mesh: the header, the chunk partials, then the vv_mesh_summary of a host call (kMeshScratchBytes, held from vv_init on)
    SC_N
};
struct scratch_buf { void *p = nullptr; size_t cap = 0; };

// Everything the last radius pre-pass of an unshaded frame was launched with (issue_prepass): the radii in SC_RAD and the order table in SC_ORDER are a pure
// function of it.  Compared as bytes: zeroed before it is filled, so the padding compares equal.
struct prepass_key {
    FrameParams P; PixelRect rect; StripMap strips;
    int want_order;                         // a table was asked for (MarchArgs::order_out)
    float *rad; uint32_t *order;            // SC_RAD / SC_ORDER as the launch saw them ...
    unsigned long long gen;                 // ... and the allocation generation of the two (ensure may hand back the same address with other contents)
    hipStream_t stream; int device;
};

struct vv_context {
    int device = 0;
    vv_knobs knobs;
    hipStream_t stream = nullptr;          // used when the caller passes no stream
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_count = nullptr;               // recorded behind the last kernel of every instrumented frame: what the counter read-backs wait on
    bool timed = false, time_frames = true;      // vv_set_frame_timing
    // volume
    void *d_vol = nullptr; size_t vol_bytes = 0; int vtype = VV_VOXEL_U8; int nx = 0, ny = 0, nz = 0;
    size_t row_pitch = 0, slice_pitch = 0, alloc_bytes = 0;   // linear layout in HBM (bytes); vol_bytes stays nx*ny*nz*voxel
    layout_copy copies[CP_N];
    // residency policy of the optional copies (vv_set_layout_policy): HBM budget for all of them together (0 = default, layout_budget())
    // and whether vv_render may build a missing copy by itself
    size_t layout_budget_bytes = 0; bool build_in_render = true;
    unsigned long long frame_no = 0;                                          // the clock of layout_copy::last_used
    unsigned long long builds_in_render = 0;                                  // copies built inside vv_render since the volume was loaded
    float last_density = 1e9f;                                                // what the launch policy took the last frame's sampling density to be
    // transfer function
    float4 *d_tf = nullptr; bool tf_gray = false; bool have_tf = false;
    bool tf_alpha_unit = false;          // every opacity of the table lies in [0, 1]: accumulated opacity never decreases
    scratch_buf scratch[SC_N];                              // grown on demand (ensure), freed and counted in loops over the table
    // launch-policy estimate taken from device-resident first-pass images (vv_render, synchronous calls), kept while the view stays
    struct view_key_t { float cam[8]; const void *front, *back; int img_w, img_h, W, H; } view_key;
    bool view_key_valid = false, view_est_ok = false; float view_side[3] = {0, 0, 0}, view_px_cube = 0.f;
    std::vector<uint8_t> row_buf;
    int last_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // vv_debug_last_launch
    // the radius pre-pass of unshaded frames (issue_prepass): what SC_RAD / SC_ORDER hold, and vv_debug_prepass_state's counts
    prepass_key prepass; bool prepass_valid = false;
    unsigned long long prepass_gen = 0;              // bumped whenever SC_RAD or SC_ORDER is allocated anew or freed
    int prepass_launched = 0, prepass_reused = 0, last_reused = 0, last_fill_blocks = 0;
    unsigned long long *d_counter = nullptr;
    unsigned long long *d_hist = nullptr;       // histogram calls: the accumulator (kHistAccWords), then a vv_histogram for host-output calls
    int n_cu = 0;                               // compute units of the device (hist_kernel's grid)
    bool counter_valid = false;          // counters of the last instrumented frame
    // streamed upload
    hipStream_t copy_stream = nullptr, promo_stream = nullptr;   // H2D copies / u8 -> f32 promotion kernels
    void *pin[2] = {nullptr, nullptr}; hipEvent_t pin_ev[2] = {nullptr, nullptr}; int pin_next = 0;   // pin_ev[b]: staging buffers b free again
    hipEvent_t src_ev[2] = {nullptr, nullptr}; int src_last = -1;       // src_ev[b]: the copy engine has read piece b's source
    uint8_t *d_stage[2] = {nullptr, nullptr};     // u8 slices awaiting promotion
    bool streaming = false;
    std::string err;
};

static std::string g_err;

// vv_context::d_hist: the accumulator, then (8-byte aligned) the vv_histogram a host-output call copies back
static const size_t kHistResultOffset = kHistAccWords * sizeof(unsigned long long);
static const size_t kHistScratchBytes = kHistResultOffset + sizeof(vv_histogram);
static_assert(sizeof(vv_histogram) == 2072 && sizeof(unsigned long long) == 8, "vv_histogram layout (include/volviz.h)");
// scratch entry SC_LABEL: the counters of the label kernels, then (8-byte aligned) the vv_label_stats a host-output call copies back
static const size_t kLabelStatsOffset = kLabelCounters * sizeof(unsigned long long);
static const size_t kLabelScratchBytes = kLabelStatsOffset + sizeof(vv_label_stats);
static_assert(sizeof(vv_label) == 36 && sizeof(vv_label_stats) == 32 && sizeof(vv_mask) == 48, "vv_label / vv_label_stats / vv_mask layout (include/volviz.h)");
static_assert(sizeof(vv_distance) == 64, "vv_distance layout (include/volviz.h)");
// scratch entry SC_REGION: the header counters, the chunk partials, then (8-byte aligned) the vv_region_summary a host call copies back
static const size_t kRegionPartialsOffset = kRegionHeader * sizeof(unsigned long long);
static const size_t kRegionSummaryOffset = kRegionPartialsOffset + kRegionMaxChunks * sizeof(uint32_t);
static const size_t kRegionScratchBytes = kRegionSummaryOffset + sizeof(vv_region_summary);
static_assert(sizeof(vv_regions) == 32 && sizeof(vv_region) == 184 && alignof(vv_region) == 8 && sizeof(vv_region_summary) == 32, "vv_regions / vv_region / vv_region_summary layout (include/volviz.h)");
static_assert(offsetof(vv_region, voxels) == 8 && offsetof(vv_region, lo) == 16 && offsetof(vv_region, hi) == 28 && offsetof(vv_region, sum) == 40 &&
              offsetof(vv_region, sum2) == 64 && offsetof(vv_region, bin_min) == 112 && offsetof(vv_region, bin_sum) == 120 && offsetof(vv_region, vmin) == 136 &&
              offsetof(vv_region, faces) == 144 && offsetof(vv_region, aux_sum) == 168 && offsetof(vv_region, aux_argmax) == 176 && offsetof(vv_region, aux_max) == 180,
              "vv_region offsets (include/volviz.h)");
// scratch entry SC_MESH: the header (V, Q), the chunk partials, then (8-byte aligned) the vv_mesh_summary a host call copies back
static const size_t kMeshPartialsOffset = kMeshHeader * sizeof(unsigned long long);
static const size_t kMeshSummaryOffset = kMeshPartialsOffset + kMeshMaxChunks * sizeof(MeshPartial);
static const size_t kMeshScratchBytes = kMeshSummaryOffset + sizeof(vv_mesh_summary);
static_assert(sizeof(vv_mesh) == 56 && sizeof(vv_mesh_vertex) == 16 && sizeof(vv_mesh_normal) == 16 && sizeof(vv_mesh_summary) == 32 && sizeof(MeshPartial) == 16,
              "vv_mesh / vv_mesh_vertex / vv_mesh_normal / vv_mesh_summary layout (include/volviz.h)");
static_assert(offsetof(vv_mesh, box_hi) == 12 && offsetof(vv_mesh, source) == 24 && offsetof(vv_mesh, level) == 28 && offsetof(vv_mesh, bin_lo) == 32 &&
              offsetof(vv_mesh, bin_hi) == 36 && offsetof(vv_mesh, label) == 40 && offsetof(vv_mesh, cap) == 44 && offsetof(vv_mesh, max_vertices) == 48 &&
              offsetof(vv_mesh, max_quads) == 52 && offsetof(vv_mesh_vertex, site) == 12 && offsetof(vv_mesh_normal, edges) == 12 &&
              offsetof(vv_mesh_summary, written_vertices) == 16, "vv_mesh offsets (include/volviz.h)");
static const size_t kStageBytes = 64u << 20;      // streamed upload: pinned / device staging buffers (vv_context::pin, d_stage)

static int fail(vv_context *c, int code, const std::string &msg)
{
    // (a failed call of the context, a HIP error in a frame among them: what SC_RAD / SC_ORDER hold is no longer vouched for, issue_prepass)
    if (c) { c->err = msg; c->prepass_valid = false; } else g_err = msg;
    return code;
}
#define HIPCHK(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail((c), VV_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// `stream` of the C-ABI: NULL = the context's own stream, the call returns when the work is done;
// VV_STREAM_DEFAULT_ASYNC = the device's default (null) stream, enqueue only; anything else = that stream, enqueue only.
static inline hipStream_t pick_stream(const vv_context *c, void *stream)
{
    if (!stream) return c->stream;
    if (stream == VV_STREAM_DEFAULT_ASYNC) return (hipStream_t)0;
    return (hipStream_t)stream;
}

static void drop_copies(vv_context *c)
{
    for (layout_copy &cp : c->copies) {
        if (cp.ptr) (void)hipFree(cp.ptr);
        cp = layout_copy();
    }
    c->builds_in_render = 0;
    c->view_key_valid = false;             // (a new volume: the launch-policy estimate taken from first-pass images is re-taken)
    c->prepass_valid = false;              // (and the next unshaded frame computes its radii)
}

static size_t voxel_bytes(int vtype) { return vtype == VV_VOXEL_F32 ? 4 : 1; }

// ---- the linear volume: checked, given up and allocated in one place each (the loaders, the streamed upload, vv_shutdown) -------------------
// `who`: the caller's message prefix; bad_dims / bad_type: its texts for those two findings
static int check_volume(vv_context *c, const char *who, const char *bad_dims, const char *bad_type, int vtype, int nx, int ny, int nz)
{
    const std::string w(who);
    if (nx < 1 || ny < 1 || nz < 1) return fail(c, VV_ERR_INVALID, w + bad_dims);
    if (vtype != VV_VOXEL_U8 && vtype != VV_VOXEL_F32) return fail(c, VV_ERR_INVALID, w + bad_type);
    const size_t vsz = voxel_bytes(vtype);
    if ((size_t)nx * ny * vsz > 0xFFFFFFF0ull) return fail(c, VV_ERR_INVALID, w + "one slice must stay below 4 GiB");
    if ((size_t)nx * vsz >= (1u << 24) || ny >= (1 << 24) || nz >= (1 << 24))
        return fail(c, VV_ERR_INVALID, w + "a volume row must be below 16 MiB and each dimension below 2^24");
    return VV_OK;
}

// Gives up the loaded volume and its copies: later calls report VV_ERR_NO_VOLUME until the next load.  (The reference leaks its old volume.)
static int release_volume(vv_context *c)
{
    drop_copies(c);
    void *old = c->d_vol;
    c->d_vol = nullptr; c->nx = c->ny = c->nz = 0; c->vol_bytes = 0;
    if (old) HIPCHK(c, hipFree(old));
    return VV_OK;
}

// Allocates the (dense) linear volume and sets its geometry.  Behind the voxels lie one slice + two rows + 4096 bytes, zeroed on `st`: weight-0
// corner fetches of edge samples land there instead of needing index clamps (see vv_device.h VolumeView).
static int alloc_volume(vv_context *c, int vtype, int nx, int ny, int nz, hipStream_t st)
{
    const size_t vsz = voxel_bytes(vtype);
    const size_t bytes = (size_t)nx * ny * nz * vsz, pad = (size_t)nx * ny * vsz + 2 * (size_t)nx * vsz + 4096;
    HIPCHK(c, hipMalloc(&c->d_vol, bytes + pad));
    HIPCHK(c, hipMemsetAsync((char *)c->d_vol + bytes, 0, pad, st));
    c->vol_bytes = bytes; c->vtype = vtype; c->nx = nx; c->ny = ny; c->nz = nz;
    c->prepass_valid = false;
    c->row_pitch = (size_t)nx * vsz; c->slice_pitch = c->row_pitch * ny; c->alloc_bytes = bytes + pad;
    return VV_OK;
}

static int ensure(vv_context *c, int id, size_t need)
{
    scratch_buf &s = c->scratch[id];
    if (s.cap >= need && s.p) return VV_OK;
    if (id == SC_RAD || id == SC_ORDER) { ++c->prepass_gen; c->prepass_valid = false; }      // (the radii / the order table go with their buffer)
    if (s.p) { HIPCHK(c, hipFree(s.p)); s.p = nullptr; s.cap = 0; }
    HIPCHK(c, hipMalloc(&s.p, need));
    s.cap = need;
    return VV_OK;
}

// ---- host-or-device buffers of the calls that are not frames --------------------------------------------------------------------------------
// One buffer of a call: the caller's pointer and size, and where it lives.  A device buffer is used where it is.  A host buffer gets a place on
// the device -- `home` if the call has a fixed one, else the next bytes of scratch entry `scratch` (the host buffers of a call that name the
// same entry lie one after another in list order) -- which the caller's bytes are copied into before the kernels (`in`: data the kernel reads,
// or an output whose skipped elements must keep the caller's bytes) and / or copied back from behind them (`out`).  Zero-byte buffers are not staged.
struct CallBuf {
    void *user; size_t bytes;
    bool host, in, out;
    int scratch; void *home;
    void *dev;                          // stage_call: where the kernels read / write
};

// Before the kernels: sets the device, picks the stream (*st), gives every host buffer its place and enqueues the uploads in list order.
static int stage_call(vv_context *c, void *stream, hipStream_t *st, CallBuf *b, int n)
{
    HIPCHK(c, hipSetDevice(c->device));
    *st = pick_stream(c, stream);
    size_t need[SC_N] = {}, off[8];
    bool staged = false;
    assert(n <= 8);
    for (int i = 0; i < n; ++i) {
        b[i].dev = b[i].user;
        if (!b[i].host || !b[i].bytes) continue;
        staged = true;
        if (!b[i].home) { off[i] = need[b[i].scratch]; need[b[i].scratch] += b[i].bytes; }
    }
    if (!staged) return VV_OK;                  // every buffer is on the device or empty: used where it is
    for (int id = 0; id < SC_N; ++id)
        if (need[id]) { int rc = ensure(c, id, need[id]); if (rc) return rc; }
    for (int i = 0; i < n; ++i) {
        if (!b[i].host || !b[i].bytes) continue;
        b[i].dev = b[i].home ? b[i].home : (char *)c->scratch[b[i].scratch].p + off[i];
        if (b[i].in) HIPCHK(c, hipMemcpyAsync(b[i].dev, b[i].user, b[i].bytes, hipMemcpyHostToDevice, *st));
    }
    return VV_OK;
}

// Behind the kernels: their launch errors, the downloads in list order, and the one rule of who waits: a call with a host output returns when the
// caller's buffer is filled; a call whose outputs stay on the device waits only when `stream` is NULL (with a stream it has only enqueued).
static int finish_call(vv_context *c, void *stream, hipStream_t st, const CallBuf *b, int n)
{
    HIPCHK(c, hipGetLastError());
    bool host_out = false;
    for (int i = 0; i < n; ++i) {
        if (!b[i].host || !b[i].out) continue;
        host_out = true;
        if (b[i].bytes) HIPCHK(c, hipMemcpyAsync(b[i].user, b[i].dev, b[i].bytes, hipMemcpyDeviceToHost, st));
    }
    if (host_out || !stream) HIPCHK(c, hipStreamSynchronize(st));
    return VV_OK;
}

// ---- what the calls that read the loaded volume's boxes and write a dense volume share -----------------------------------
// Source addressing: the byte offset of voxel (x, y, z) in the linear volume, and the end of the last voxel of the box below `hi`.
static size_t voxel_offset(const vv_context *c, int x, int y, int z)
{
    return (size_t)z * c->slice_pitch + (size_t)y * c->row_pitch + (size_t)x * voxel_bytes(c->vtype);
}
static size_t box_end(const vv_context *c, const int hi[3]) { return voxel_offset(c, hi[0], hi[1] - 1, hi[2] - 1); }

static bool box_in_range(const int lo[3], const int hi[3], const int ext[3])
{
    for (int a = 0; a < 3; ++a)
        if (!(0 <= lo[a] && lo[a] < hi[a] && hi[a] <= ext[a])) return false;
    return true;
}
// The box of a descriptor, measured against `ext`: six zeros mean all of it.  (err_to: vv_derive_dims has a const context.)
static int check_box(vv_context *err_to, const char *who, const int box_lo[3], const int box_hi[3], const int ext[3], int lo[3], int hi[3])
{
    bool whole = true;
    for (int a = 0; a < 3; ++a) whole = whole && box_lo[a] == 0 && box_hi[a] == 0;
    for (int a = 0; a < 3; ++a) { lo[a] = whole ? 0 : box_lo[a]; hi[a] = whole ? ext[a] : box_hi[a]; }
    if (!box_in_range(lo, hi, ext)) return fail(err_to, VV_ERR_INVALID, std::string(who) + ": the box must satisfy 0 <= lo < hi <= dims on every axis (or be all zeros)");
    return VV_OK;
}
static int check_out_type(vv_context *err_to, const char *who, int out_type)
{
    if (out_type != VV_VOXEL_U8 && out_type != VV_VOXEL_F32) return fail(err_to, VV_ERR_INVALID, std::string(who) + ": out_type must be VV_VOXEL_U8 or VV_VOXEL_F32");
    return VV_OK;
}
// The caller's buffer for a dense volume of m[0] x m[1] x m[2] voxels of `out_type`: its bytes (*bytes), its capacity (`whence`: the message's
// word on where the extents come from, or ""), a device f32 buffer's alignment and, for the calls that promise it, no overlap with the loaded volume.
static int check_out_volume(vv_context *c, const char *who, const char *whence, const void *out, size_t capacity, int out_on_device, int out_type,
                            const int m[3], bool refuse_overlap, size_t *bytes)
{
    const std::string w(who);
    *bytes = (size_t)m[0] * (size_t)m[1] * (size_t)m[2] * voxel_bytes(out_type);
    if (capacity < *bytes) return fail(c, VV_ERR_INVALID, w + ": capacity is below the output's bytes" + whence);
    if (out_on_device && out_type == VV_VOXEL_F32 && ((uintptr_t)out & 3) != 0) return fail(c, VV_ERR_INVALID, w + ": a device f32 out must be 4-byte aligned");
    if (refuse_overlap && out_on_device && (uintptr_t)out < (uintptr_t)c->d_vol + c->alloc_bytes && (uintptr_t)c->d_vol < (uintptr_t)out + *bytes)
        return fail(c, VV_ERR_INVALID, w + ": out overlaps the loaded volume (the pass is not in place)");
    return VV_OK;
}

// Runs a call that fills a volume of `bytes` at `out`, behind its checks.  A host volume goes through a device buffer of the call's own, not through
// the scratch table: a volume-sized buffer must not stay resident in the context.  stage_call finds it as the buffer's fixed home (and uploads the
// caller's bytes into it where the call works `in_place`); it is freed on every path.  `body(dev, st)` launches on the device volume and returns
// VV_OK, or fails before it launches; the download and the wait are finish_call's.
// run_out_volumes is the same for a short list of buffers (a call with several volume-sized arguments, inputs among them): every host buffer of the
// list that has no home gets a device buffer of the call's own; `body(b, st)` finds the device addresses in b[i].dev.
template <class Body>
static int run_out_volumes(vv_context *c, const char *who, CallBuf *b, int n, void *stream, Body body)
{
    HIPCHK(c, hipSetDevice(c->device));
    void *tmp[8] = {};
    assert(n <= 8);
    int rc = VV_OK;
    for (int i = 0; i < n && rc == VV_OK; ++i) {
        if (!b[i].host || !b[i].bytes || b[i].home) continue;
        if (hipMalloc(&tmp[i], b[i].bytes) != hipSuccess) {
            (void)hipGetLastError();
            tmp[i] = nullptr;
            rc = fail(c, VV_ERR_NOMEM, std::string(who) + ": no device memory for the staging buffer of a host out");
        } else b[i].home = tmp[i];
    }
    hipStream_t st;
    if (rc == VV_OK) rc = stage_call(c, stream, &st, b, n);
    if (rc == VV_OK) rc = body(b, st);
    if (rc == VV_OK) rc = finish_call(c, stream, st, b, n);
    for (void *t : tmp)
        if (t) (void)hipFree(t);
    return rc;
}
// The roles a buffer of such a list can have.  `p` may be NULL (an optional argument): the buffer is then empty, whatever `bytes` says.
//   buf_in      data the kernels read
//   buf_out     an output the kernels write whole
//   buf_inout   an output whose unwritten part keeps the caller's bytes (a table with rows to spare; a volume worked on in place)
//   buf_out_at  an output with a fixed home on the device (the stats / summary structs, which live in the call's scratch)
static CallBuf buf_role(const void *p, size_t bytes, bool host, bool in, bool out, void *home)
{
    return {(void *)p, p ? bytes : 0, host, in, out, 0, home, nullptr};
}
static CallBuf buf_in(const void *p, size_t bytes, bool host) { return buf_role(p, bytes, host, true, false, nullptr); }
static CallBuf buf_out(void *p, size_t bytes, bool host) { return buf_role(p, bytes, host, false, true, nullptr); }
static CallBuf buf_inout(void *p, size_t bytes, bool host) { return buf_role(p, bytes, host, true, true, nullptr); }
static CallBuf buf_out_at(void *p, size_t bytes, bool host, void *home) { return buf_role(p, bytes, host, false, true, home); }

template <class Body>
static int run_out_volume(vv_context *c, const char *who, void *out, size_t bytes, int out_on_device, bool in_place, void *stream, Body body)
{
    CallBuf b = in_place ? buf_inout(out, bytes, !out_on_device) : buf_out(out, bytes, !out_on_device);
    return run_out_volumes(c, who, &b, 1, stream, [&](CallBuf *bb, hipStream_t st) { return body(bb[0].dev, st); });
}

// ---- the calls that take or produce word-per-voxel arrays over a box of the loaded volume: label, mask, distance, region table, mesh ----------
// Their opening, in the order every one of them refuses in: the context, the descriptor and the other arguments that must not be NULL
// (`args_given`), the loaded volume, the descriptor's box, its voxel count (at most 2^32 - 2).  Then A is zeroed and told the source: the
// box's first voxel, the pitches, the voxel type, the extents b and -- where the kernels want it -- the origin lo.  Yields lo, hi and voxels.
// (err_to: vv_mesh_dims has a const context.)
struct CallBox { int lo[3], hi[3]; unsigned long long voxels; };
template <class Args> static auto tell_origin(Args &A, const int lo[3], int) -> decltype((void)A.lo[0]) { for (int a = 0; a < 3; ++a) A.lo[a] = lo[a]; }
template <class Args> static void tell_origin(Args &, const int *, long) {}

template <class Desc, class Args>
static int open_box_call(const vv_context *c, vv_context *err_to, const char *who, const Desc *d, bool args_given, Args &A, CallBox &B)
{
    const std::string w(who);
    if (!c) return fail(nullptr, VV_ERR_INVALID, w + ": NULL context");
    if (!d || !args_given) return fail(err_to, VV_ERR_INVALID, w + ": NULL argument");
    if (!c->d_vol) return fail(err_to, VV_ERR_NO_VOLUME, w + ": no volume loaded");
    const int dims[3] = {c->nx, c->ny, c->nz};
    const int rc = check_box(err_to, who, d->box_lo, d->box_hi, dims, B.lo, B.hi);
    if (rc) return rc;
    memset(&A, 0, sizeof A);
    for (int a = 0; a < 3; ++a) A.b[a] = (uint32_t)(B.hi[a] - B.lo[a]);
    B.voxels = (unsigned long long)A.b[0] * A.b[1] * A.b[2];        // (each below 2^24: the product fits)
    if (B.voxels > 0xFFFFFFFEull) return fail(err_to, VV_ERR_INVALID, w + ": the box may hold at most 2^32 - 2 voxels");
    A.src0 = (const char *)c->d_vol + voxel_offset(c, B.lo[0], B.lo[1], B.lo[2]);
    A.row_pitch = c->row_pitch; A.slice_pitch = c->slice_pitch;
    A.src_type = c->vtype;
    tell_origin(A, B.lo, 0);
    return VV_OK;
}
// what these kernels' source addressing is promised: the box's last voxel lies inside the allocation, f32 voxels are aligned.  (A step of its own:
// every call refuses it behind its argument checks.)
static bool label_source_ok(const vv_context *c, const int hi[3])
{
    return box_end(c, hi) <= c->alloc_bytes && !(c->vtype == VV_VOXEL_F32 && (((uintptr_t)c->d_vol | c->row_pitch | c->slice_pitch) & 3) != 0);
}
static int check_bins(vv_context *c, const char *who, int bin_lo, int bin_hi)
{
    if (!(0 <= bin_lo && bin_lo <= bin_hi && bin_hi <= 255)) return fail(c, VV_ERR_INVALID, std::string(who) + ": bins must satisfy 0 <= bin_lo <= bin_hi <= 255");
    return VV_OK;
}

// Overlap of device buffers.  A NULL range overlaps nothing; an empty one inside another still does (nonempty() makes it NULL where a call
// lets it pass).  first_overlap: of a list whose first `outs` spans are outputs, the name of the first output that overlaps a span behind it
// in the list -- a later output, an input, the loaded volume -- or null.
static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    return a && b && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
struct Span { const void *p; size_t n; const char *name; };
static Span nonempty(const void *p, size_t n, const char *name) { return {n ? p : nullptr, n, name}; }
static const char *first_overlap(const Span *s, int outs, int n)
{
    for (int i = 0; i < outs; ++i)
        for (int k = i + 1; k < n; ++k)
            if (ranges_overlap(s[i].p, s[i].n, s[k].p, s[k].n)) return s[i].name;
    return nullptr;
}

static int finalize_layout(vv_context *c, hipStream_t st);
static int camera_basis(vv_context *c, FrameParams &P, const camera_params *cam, const vv_ray_source *rays, int W, int H);
typedef vv_context::view_key_t vv_view_key;

// ---- launch policy for image ray sources (speed only; the pixels never depend on it) ----
// An image source may carry the camera that drew it in the fields analytic sources use (look, up, aspect): a hint.
static bool image_source_has_hint(const vv_ray_source *r)
{
    if (r->mode != VV_RAYS_IMAGES) return false;
    const float l2 = r->look[0] * r->look[0] + r->look[1] * r->look[1] + r->look[2] * r->look[2];
    const float cx = r->look[1] * r->up[2] - r->look[2] * r->up[1], cy = r->look[2] * r->up[0] - r->look[0] * r->up[2], cz = r->look[0] * r->up[1] - r->look[1] * r->up[0];
    return std::isfinite(l2) && l2 > 0.f && std::isfinite(cx + cy + cz) && (cx * cx + cy * cy + cz * cz) > 0.f;
}
static int clamp_row(long long t, int n) { return (int)(t < 0 ? 0 : (t > n - 1 ? n - 1 : t)); }
static vv_view_key view_key_of(const camera_params *cam, const vv_ray_source *r, int W, int H)
{
    vv_view_key k;
    memset(&k, 0, sizeof k);
    memcpy(k.cam, cam, sizeof(float) * 8);
    k.front = r->front; k.back = r->back; k.img_w = r->img_w; k.img_h = r->img_h; k.W = W; k.H = H;
    return k;
}
// The centre pixel row of the frame, looked up in the images exactly as the kernels do (kernel.cu:317-321): where it enters and
// leaves the cube's silhouette, and how the rays' mid-depth points move through cube space between those pixels.  side = that
// direction (unit), px_cube = its length per pixel.  False when the row misses the cube.
static bool estimate_view_from_images(const uint8_t *front, const uint8_t *back, int img_w, int img_h, int W, int H, float side[3], float *px_cube)
{
    if (!front || !back || img_w < 1 || img_h < 1 || W < 8 || H < 1) return false;
    const int y = H / 2;
    const int ty = clamp_row((long long)floorf((float)y / (float)H * (float)img_h), img_h);
    const uint8_t *fr = front + (size_t)ty * img_w * 4, *br = back + (size_t)ty * img_w * 4;
    auto texel = [&](int x) { return clamp_row((long long)floorf((float)x / (float)W * (float)img_w), img_w); };
    auto hit = [&](int x) { const int t = texel(x) * 4; return fr[t] != br[t] || fr[t + 1] != br[t + 1] || fr[t + 2] != br[t + 2]; };
    int xl = -1, xr = -1;
    for (int x = 0; x <= W - 2; ++x) if (hit(x)) { xl = x; break; }
    if (xl < 0) return false;
    for (int x = W - 2; x >= xl; --x) if (hit(x)) { xr = x; break; }
    if (xr - xl < 8) return false;
    const int a = (xl + xr) / 2 - (xr - xl) / 8, b = (xl + xr) / 2 + (xr - xl) / 8;   // the middle quarter: rays that cross the cube front to back
    float d[3], len2 = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int ta = texel(a) * 4 + k, tb = texel(b) * 4 + k;
        d[k] = (((float)fr[tb] + (float)br[tb]) - ((float)fr[ta] + (float)br[ta])) / (2.f * 255.f);
        len2 += d[k] * d[k];
    }
    if (!(len2 > 0.f)) return false;
    const float len = sqrtf(len2);
    side[0] = d[0] / len; side[1] = d[1] / len; side[2] = d[2] / len;
    *px_cube = len / (float)(b - a);
    return true;
}

// ---- residency of the optional copies -----------------------------------------------------------------------------------------
// All copies of a volume together stay within a budget (default: the larger of 8 GiB and 2.5 x the linear volume -- room for the bricked and the
// z-fastest copy of an f32 volume, C3: 9.7 GB of copies beside the 4.3 GB volume, C5: 72 GiB beside 32 GiB; every copy of a u8 volume up to 1 GiB).
// A copy that would not fit evicts copies no frame has sampled more recently (least recently used first); if that is not enough it is not built
// and the frame takes the next layout of the policy.  Results never depend on any of this.
static size_t layout_budget(const vv_context *c)
{
    if (c->layout_budget_bytes) return c->layout_budget_bytes;
    return std::max<size_t>((size_t)8 << 30, c->alloc_bytes / 2 * 5);
}
static size_t copy_bytes(const vv_context *c, int k) { return c->copies[k].valid ? c->copies[k].bytes : 0; }
static void copy_drop(vv_context *c, int k)
{
    layout_copy &cp = c->copies[k];
    if (cp.ptr) (void)hipFree(cp.ptr);               // (hipFree waits for the device: frames still in flight on a caller's stream have finished with it)
    cp.ptr = nullptr; cp.valid = false; cp.bytes = 0; cp.alloc = 0;
}
// Room for `need` more bytes of copies?  `keep`: bit mask of copies that must stay (the ones the frame being set up samples or builds from).
static bool make_room(vv_context *c, size_t need, unsigned keep)
{
    const size_t budget = layout_budget(c);
    if (need > budget) return false;
    for (;;) {
        size_t used = 0;
        for (int k = 0; k < CP_N; ++k) used += copy_bytes(c, k);
        if (used + need <= budget) return true;
        int victim = -1;
        for (int k = 0; k < CP_N; ++k)
            if (c->copies[k].valid && !(keep & (1u << k)) && (victim < 0 || c->copies[k].last_used < c->copies[victim].last_used)) victim = k;
        if (victim < 0) return false;
        copy_drop(c, victim);
    }
}

// Copy k could not be built.  Remembered until the next volume load, except for the z-pair copy, which is tried again at every request.
static bool copy_refused(vv_context *c, int k)
{
    if (k != CP_ZPAIR) c->copies[k].failed = true;
    return false;
}

// Builds copy k: `bytes` of it (what the budget counts) and `pad` more bytes of allocation, [zero_from, bytes + pad) zeroed, then `build(ptr)`,
// provided it fits the budget (evicting copies not in `keep`) and leaves 512 MiB of HBM free.  Waits for the build: later frames may come on
// another stream.  (The build kernels write [0, bytes) only: the zeros may go first.)
template <class Build>
static bool build_copy(vv_context *c, int k, size_t bytes, size_t pad, size_t zero_from, unsigned keep, hipStream_t st, Build build)
{
    layout_copy &cp = c->copies[k];
    size_t free_b = 0, total_b = 0;
    if (make_room(c, bytes, keep | (1u << k)) && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= bytes + (512ull << 20) &&
        hipMalloc(&cp.ptr, bytes + pad) == hipSuccess) {
        if (hipMemsetAsync((char *)cp.ptr + zero_from, 0, bytes + pad - zero_from, st) == hipSuccess) {
            build(cp.ptr);
            if (hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess) { cp.bytes = bytes; cp.alloc = bytes + pad; cp.valid = true; return true; }
        }
        (void)hipFree(cp.ptr);
    }
    (void)hipGetLastError();
    cp.ptr = nullptr;
    return copy_refused(c, k);
}

// The copies' sizes, geometry, addressing limits and build kernels.  Each returns true when its copy is usable afterwards; a copy the limits rule
// out is refused before anything is evicted for it, and the frame takes the next layout of the policy.  
static bool ensure_bricks(vv_context *c, hipStream_t st)
{
    layout_copy &cp = c->copies[CP_BRICKS];
    if (cp.valid || cp.failed) return cp.valid;
    uint32_t sy = 0, sz64 = 0;
    const size_t bytes = brick_copy_bytes(c->vtype, c->nx, c->ny, c->nz, &sy, &sz64);
    if (sz64 >= (1u << 24) || sy >= (1u << 24)) return copy_refused(c, CP_BRICKS);          // (the sampler multiplies b_sy and b_sz64 as 24-bit values)
    cp.row = sy; cp.slab = sz64;
    return build_copy(c, CP_BRICKS, bytes, 16, bytes, 0, st, [&](void *p) {
        launch_build_bricks(c->vtype, c->d_vol, c->row_pitch, c->slice_pitch, p, c->nx, c->ny, c->nz, st); });
}

// The launch policy's two questions about the loaded volume (choose_launch, where the measurements behind them are, and vv_prepare_layouts):
// may unshaded frames take the pair copies (u8, or f32 up to 512 MiB), and is the volume big enough for the bricked / z-fastest copy to pay?
static bool pair_copies_allowed(const vv_context *c) { return c->vtype == VV_VOXEL_U8 || c->vol_bytes <= (512ull << 20); }
static bool big_enough_for_copies(const vv_context *c) { return (size_t)c->nx * c->ny * c->nz >= (1ull << 21); }

// The addressing limits of a pair copy of `bytes` whose rows run along a dimension of n_fast voxels (z-pair: nx, x-pair: nz)
static bool pair_copy_addressable(const vv_context *c, int n_fast, size_t bytes)
{
    return (size_t)(c->ny + 1) * ((size_t)n_fast + 1) * 8 < (1ull << 32) && ((size_t)n_fast + 1) * 8 < (1u << 24) &&
           !(c->vtype == VV_VOXEL_U8 && bytes >= (1ull << 32));                // u8 sampler: 32-bit offsets
}

static bool ensure_zpair(vv_context *c, hipStream_t st)
{
    layout_copy &cp = c->copies[CP_ZPAIR];
    if (cp.valid) return true;
    uint32_t rb = 0, sb = 0;
    const size_t bytes = zpair_copy_bytes(c->vtype, c->nx, c->ny, c->nz, &rb, &sb);
    if (!pair_copy_addressable(c, c->nx, bytes)) return copy_refused(c, CP_ZPAIR);
    cp.row = rb; cp.slab = sb;
    return build_copy(c, CP_ZPAIR, bytes, 32, bytes, 0, st, [&](void *p) {
        launch_build_zpair(c->vtype, c->d_vol, c->row_pitch, c->slice_pitch, p, c->nx, c->ny, c->nz, st); });
}

// The z-fastest copy of the volume (VolumeView::zfast): rows of nz voxels padded like the linear layout's rows (finalize_layout),
// ny rows per slice, nx slices + one slice, one row and 16 bytes of zeros behind them (the weight-0 corners of edge samples).
static bool ensure_zfast(vv_context *c, hipStream_t st)
{
    layout_copy &cp = c->copies[CP_ZFAST];
    if (cp.valid || cp.failed) return cp.valid;
    const size_t vsz = voxel_bytes(c->vtype);
    size_t row = (size_t)c->nz * vsz;
    if (row % 1024 == 0) row += 32;
    else if (vsz == 1) row = (row + 3) & ~(size_t)3;                       // (u8 rows are read as aligned dwords)
    size_t rows = (size_t)c->ny;
    if (row % 1024 == 32 && (rows * row) % 4096 == 0) rows += 1;
    const size_t slice = rows * row, bytes = slice * ((size_t)c->nx + 1) + row + 16;
    if (c->ny > 65535 || (c->nz + 31) / 32 > 65535 || row >= (1u << 24) || slice >= (1ull << 32))     // (launch_build_zfast: one grid layer per row)
        return copy_refused(c, CP_ZFAST);                                   // the bricked copy serves the view
    cp.row = (uint32_t)row; cp.slab = slice;
    return build_copy(c, CP_ZFAST, bytes, 0, 0, 0, st, [&](void *p) {     // (zeroed whole: the padding of every row too)
        launch_build_zfast(c->vtype, c->d_vol, (uint32_t)c->row_pitch, (uint64_t)c->slice_pitch, p, (uint32_t)row, (uint64_t)slice, c->nx, c->ny, c->nz, st); });
}

// The x-pair copy (the z-pair copy with x and z exchanged; built from the z-fastest copy).
static bool ensure_xpair(vv_context *c, hipStream_t st)
{
    layout_copy &cp = c->copies[CP_XPAIR];
    if (cp.valid || cp.failed) return cp.valid;
    if (!ensure_zfast(c, st)) return false;
    uint32_t rb = 0, sb = 0;
    const size_t bytes = zpair_copy_bytes(c->vtype, c->nz, c->ny, c->nx, &rb, &sb);
    if (!pair_copy_addressable(c, c->nz, bytes)) return copy_refused(c, CP_XPAIR);
    cp.row = rb; cp.slab = sb;
    const layout_copy &zf = c->copies[CP_ZFAST];
    return build_copy(c, CP_XPAIR, bytes, 32, bytes, 1u << CP_ZFAST, st, [&](void *p) {
        launch_build_xpair(c->vtype, zf.ptr, zf.row, zf.slab, p, c->nx, c->ny, c->nz, st); });
}

static bool (*const ensure_copy[CP_N])(vv_context *, hipStream_t) = {ensure_bricks, ensure_zpair, ensure_zfast, ensure_xpair};   // indexed by CP_*

// Can the frame being set up (c->frame_no) sample copy k?  Resident, or built now if vv_render may build copies.  If so it counts as used by the frame.
static bool take_copy(vv_context *c, int k, hipStream_t st)
{
    if (!(c->build_in_render ? ensure_copy[k](c, st) : c->copies[k].valid)) return false;
    c->copies[k].last_used = c->frame_no;
    return true;
}

extern "C" {

const char *vv_last_error(const vv_context *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// ---- lifecycle: initCuda, kernel.cu:369-373 ------------------------------------
int vv_init(int device, vv_context **out)
{
    if (!out) return fail(nullptr, VV_ERR_INVALID, "vv_init: out_ctx is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, VV_ERR_DEVICE, "vv_init: no HIP device available (this library has no CPU path)");
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= count) return fail(nullptr, VV_ERR_INVALID, "vv_init: device index out of range");
    vv_context *c = new vv_context();
    c->device = device;
    c->knobs.read();
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess || hipEventCreateWithFlags(&c->ev_count, hipEventDisableTiming) != hipSuccess ||
        hipMalloc((void **)&c->d_counter, 16 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void **)&c->d_hist, kHistScratchBytes) != hipSuccess ||
        hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        hipMalloc((void **)&c->d_tf, 256 * sizeof(float4)) != hipSuccess ||
        ensure(c, SC_LABEL, kLabelScratchBytes) != VV_OK ||               // (held from here on: a label call allocates nothing)
        ensure(c, SC_REGION, kRegionScratchBytes) != VV_OK ||             // (nor does a region call)
        ensure(c, SC_MESH, kMeshScratchBytes) != VV_OK) {                 // (nor a mesh call)
        vv_shutdown(c);                           // (gives back whatever was created before the failure)
        return fail(nullptr, VV_ERR_DEVICE, "vv_init: device set-up failed");
    }
    *out = c;
    return VV_OK;
}

int vv_shutdown(vv_context *c)
{
    if (!c) return VV_OK;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    c->prepass_valid = false; ++c->prepass_gen;
    (void)release_volume(c);
    if (c->d_tf) hipFree(c->d_tf);
    for (scratch_buf &s : c->scratch)
        if (s.p) hipFree(s.p);
    if (c->d_counter) hipFree(c->d_counter);
    if (c->d_hist) hipFree(c->d_hist);
    for (int i = 0; i < 2; ++i) {
        if (c->pin[i]) hipHostFree(c->pin[i]);
        if (c->pin_ev[i]) hipEventDestroy(c->pin_ev[i]);
        if (c->src_ev[i]) hipEventDestroy(c->src_ev[i]);
        if (c->d_stage[i]) hipFree(c->d_stage[i]);
    }
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    if (c->promo_stream) hipStreamDestroy(c->promo_stream);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->ev_count) hipEventDestroy(c->ev_count);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return VV_OK;
}

// ---- volume + TF: cudaLoadVolume, kernel.cu:456-498 ------------------------------
int vv_set_transfer_function(vv_context *c, const float tf[1024])
{
    if (!c || !tf) return fail(c, VV_ERR_INVALID, "vv_set_transfer_function: NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < 1024; ++i)
        if (!std::isfinite(tf[i])) return fail(c, VV_ERR_INVALID, "vv_set_transfer_function: table entries must be finite");
    bool gray = true, unit = true;
    for (int i = 0; i < 256; ++i)
        if (!(tf[4*i] == tf[4*i+1] && tf[4*i] == tf[4*i+2])) { gray = false; break; }
    for (int i = 0; i < 256; ++i)
        if (!(tf[4*i+3] >= 0.f && tf[4*i+3] <= 1.f)) { unit = false; break; }
    // pageable host memory: the copy is staged before hipMemcpy returns      kernel.cu:495-496
    HIPCHK(c, hipMemcpy(c->d_tf, tf, 1024 * sizeof(float), hipMemcpyHostToDevice));
    c->tf_gray = gray; c->tf_alpha_unit = unit; c->have_tf = true;
    return VV_OK;
}

static int install_volume(vv_context *c, const void *src, bool src_on_device, int vtype,
                          int nx, int ny, int nz, const float tf[1024], hipStream_t s)
{
    if (!c || !src) return fail(c, VV_ERR_INVALID, "load_volume: NULL argument");
    int rc = check_volume(c, "load_volume: ", "dims must be >= 1", "bad voxel type", vtype, nx, ny, nz);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->knobs.read();
    hipStream_t st = pick_stream(c, s);
    if ((rc = release_volume(c)) != VV_OK || (rc = alloc_volume(c, vtype, nx, ny, nz, st)) != VV_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_vol, src, c->vol_bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    if ((rc = finalize_layout(c, st)) != VV_OK) return rc;
    if (!src_on_device || !s) HIPCHK(c, hipStreamSynchronize(st));
    if (tf) return vv_set_transfer_function(c, tf);
    return VV_OK;
}

int vv_load_volume_u8(vv_context *c, const uint8_t *texels, size_t size, int nx, int ny, int nz, const float tf[1024])
{
    if (size != (size_t)nx * ny * nz) return fail(c, VV_ERR_INVALID, "vv_load_volume_u8: size != nx*ny*nz");
    return install_volume(c, texels, false, VV_VOXEL_U8, nx, ny, nz, tf, nullptr);
}
int vv_load_volume_f32(vv_context *c, const float *texels, size_t size, int nx, int ny, int nz, const float tf[1024])
{
    if (size != (size_t)nx * ny * nz * 4) return fail(c, VV_ERR_INVALID, "vv_load_volume_f32: size != nx*ny*nz*4 bytes");
    return install_volume(c, texels, false, VV_VOXEL_F32, nx, ny, nz, tf, nullptr);
}
int vv_load_volume_device(vv_context *c, const void *dev, int vtype, int nx, int ny, int nz, const float tf[1024], void *stream)
{
    return install_volume(c, dev, true, vtype, nx, ny, nz, tf, (hipStream_t)stream);
}

int vv_prepare_layouts(vv_context *c, int which, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_prepare_layouts: NULL context");
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_prepare_layouts: no volume loaded");
    if (which & ~(VV_LAYOUT_BRICKED | VV_LAYOUT_ZPAIR | VV_LAYOUT_ZFAST | VV_LAYOUT_POLICY)) return fail(c, VV_ERR_INVALID, "vv_prepare_layouts: unknown layout bit");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, stream);
    const bool pair_ok = pair_copies_allowed(c);          // (the z-pair / x-pair conditions of vv_render)
    if (which & VV_LAYOUT_POLICY) {
        // every copy vv_render's policy can pick for this volume, in the order of what an orbit needs most: oblique views, side views, the pair copies
        if (big_enough_for_copies(c)) which |= VV_LAYOUT_BRICKED | VV_LAYOUT_ZFAST;
        if (pair_ok) which |= VV_LAYOUT_ZPAIR;
    }
    int built = 0;
    if (which & VV_LAYOUT_BRICKED) c->copies[CP_BRICKS].failed = false;       // an explicit request retries after an earlier shortage of HBM
    if (which & VV_LAYOUT_ZFAST) c->copies[CP_ZFAST].failed = c->copies[CP_XPAIR].failed = false;
    // (a copy built here counts as just used: the next one must not evict it to make room for itself)
    auto prepare = [&](int k) {
        if (!ensure_copy[k](c, st)) return false;
        c->copies[k].last_used = ++c->frame_no;
        return true;
    };
    if ((which & VV_LAYOUT_BRICKED) && prepare(CP_BRICKS)) built |= VV_LAYOUT_BRICKED;
    if ((which & VV_LAYOUT_ZFAST) && prepare(CP_ZFAST)) {
        built |= VV_LAYOUT_ZFAST;
        // side views of unshaded frames take the x-pair copy where front views take the z-pair copy: built with the z-fastest copy it is made from
        if (pair_ok) prepare(CP_XPAIR);
    }
    if ((which & VV_LAYOUT_ZPAIR) && prepare(CP_ZPAIR)) built |= VV_LAYOUT_ZPAIR;
    return built;
}

int vv_reread_env(vv_context *c)
{
    if (!c) return VV_ERR_INVALID;
    c->knobs.read();
    c->prepass_valid = false;
    return VV_OK;
}

int vv_set_layout_policy(vv_context *c, unsigned long long budget_bytes, int build_in_render)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_set_layout_policy: NULL context");
    c->layout_budget_bytes = (size_t)budget_bytes;
    c->build_in_render = build_in_render != 0;
    return VV_OK;
}

int vv_layout_state(const vv_context *c, unsigned long long out[8])
{
    if (!c || !out) return VV_ERR_INVALID;
    out[0] = c->d_vol ? c->alloc_bytes : 0;
    for (int k = 0; k < CP_N; ++k) out[1 + k] = copy_bytes(c, k);
    out[5] = c->d_vol ? layout_budget(c) : c->layout_budget_bytes;
    out[6] = c->builds_in_render;
    out[7] = c->build_in_render ? 1 : 0;
    return VV_OK;
}

int vv_device_bytes(const vv_context *c, unsigned long long out[4])
{
    if (!c || !out) return VV_ERR_INVALID;
    out[0] = c->d_vol ? c->alloc_bytes : 0;
    out[1] = copy_bytes(c, CP_BRICKS);
    out[2] = copy_bytes(c, CP_ZPAIR) + copy_bytes(c, CP_ZFAST) + copy_bytes(c, CP_XPAIR);
    // tables and scratch: the fixed allocations of vv_init (transfer function, counters, histogram scratch), the scratch table, the streamed upload's staging
    out[3] = 256 * sizeof(float4) + 16 * sizeof(unsigned long long) + kHistScratchBytes;
    for (const scratch_buf &s : c->scratch) out[3] += s.cap;
    for (const uint8_t *stage : c->d_stage) out[3] += stage ? kStageBytes : 0;
    return VV_OK;
}

// developer statistics of the last instrumented launch (staged kernel): [0] executed samples,
// [1] stages, [2] samples served from global memory, [3] bytes staged into LDS, [4] wave compute trips
int vv_debug_counters(vv_context *c, unsigned long long out[16])
{
    if (!c || !out || !c->counter_valid) return VV_ERR_INVALID;
    if (hipEventSynchronize(c->ev_count) != hipSuccess) return VV_ERR_DEVICE;
    if (hipMemcpy(out, c->d_counter, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return VV_ERR_DEVICE;
    return VV_OK;
}

// ---- streamed upload ---------------------------------------------------------------------
int vv_load_volume_stream_begin(vv_context *c, int vtype, int nx, int ny, int nz, const float tf[1024])
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "stream_begin: NULL context");
    int rc = check_volume(c, "stream_begin: ", "bad dims / voxel type", "bad dims / voxel type", vtype, nx, ny, nz);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    c->knobs.read();
    if (!c->copy_stream) HIPCHK(c, hipStreamCreate(&c->copy_stream));
    if (!c->promo_stream) HIPCHK(c, hipStreamCreate(&c->promo_stream));
    if ((rc = release_volume(c)) != VV_OK || (rc = alloc_volume(c, vtype, nx, ny, nz, c->copy_stream)) != VV_OK) return rc;
    c->src_last = -1;
    c->streaming = true;
    if (tf) return vv_set_transfer_function(c, tf);
    return VV_OK;
}

// Enqueue only.  H2D copies run on copy_stream, promotion kernels on promo_stream behind the copy's event, so the copy of
// the next piece overlaps the promotion of this one.  Two events per staging slot: src_ev (the copy engine has read the
// source: what a caller that refills a pinned buffer has to wait for) and pin_ev (copy AND promotion done: the slot's
// staging buffers may be reused).
int vv_load_volume_stream_slices_async(vv_context *c, const void *src, int src_type, int z0, int nslices)
{
    if (!c || !c->streaming) return fail(c, VV_ERR_INVALID, "stream_slices: no stream_begin");
    if (!src || z0 < 0 || nslices < 1 || z0 + nslices > c->nz) return fail(c, VV_ERR_INVALID, "stream_slices: bad slice range");
    if (src_type != c->vtype && !(src_type == VV_VOXEL_U8 && c->vtype == VV_VOXEL_F32))
        return fail(c, VV_ERR_INVALID, "stream_slices: source type must match the volume (or be u8 for an f32 volume)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t ssz = voxel_bytes(src_type), dsz = voxel_bytes(c->vtype);
    const size_t slice_vox = (size_t)c->nx * c->ny;
    const bool promote = src_type != c->vtype;
    hipPointerAttribute_t attr;
    bool pinned = hipPointerGetAttributes(&attr, src) == hipSuccess && attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();                       // an unregistered pointer is not an error for us
    // work in pieces of at most kStageBytes of source data
    size_t total_vox = slice_vox * (size_t)nslices, done = 0;
    const size_t piece_vox_max = ((kStageBytes / ssz) / 16) * 16;
    while (done < total_vox) {
        const size_t nv = std::min(piece_vox_max, total_vox - done);
        const int b = c->pin_next; c->pin_next ^= 1;
        if (!c->pin_ev[b]) HIPCHK(c, hipEventCreate(&c->pin_ev[b]));
        if (!c->src_ev[b]) HIPCHK(c, hipEventCreate(&c->src_ev[b]));
        HIPCHK(c, hipEventSynchronize(c->pin_ev[b]));          // staging slot b free again
        const char *hsrc = (const char *)src + done * ssz;
        if (!pinned) {
            if (!c->pin[b]) HIPCHK(c, hipHostMalloc(&c->pin[b], kStageBytes, hipHostMallocDefault));
            memcpy(c->pin[b], hsrc, nv * ssz);
            hsrc = (const char *)c->pin[b];
        }
        char *dst = (char *)c->d_vol + ((size_t)z0 * slice_vox + done) * dsz;
        if (!promote) {
            HIPCHK(c, hipMemcpyAsync(dst, hsrc, nv * ssz, hipMemcpyHostToDevice, c->copy_stream));
            HIPCHK(c, hipEventRecord(c->src_ev[b], c->copy_stream));
            HIPCHK(c, hipEventRecord(c->pin_ev[b], c->copy_stream));
        } else {
            if (!c->d_stage[b]) HIPCHK(c, hipMalloc((void **)&c->d_stage[b], kStageBytes));
            HIPCHK(c, hipMemcpyAsync(c->d_stage[b], hsrc, nv, hipMemcpyHostToDevice, c->copy_stream));
            HIPCHK(c, hipEventRecord(c->src_ev[b], c->copy_stream));
            HIPCHK(c, hipStreamWaitEvent(c->promo_stream, c->src_ev[b], 0));
            launch_promote_u8_f32(c->d_stage[b], (float *)dst, nv, c->promo_stream);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventRecord(c->pin_ev[b], c->promo_stream));
        }
        // (pageable sources were copied into our own staging buffer above.)  An outstanding pinned source stays outstanding when a
        // pageable piece follows: copies are ordered on copy_stream, so this piece's event covers the earlier ones.
        if (pinned || c->src_last >= 0) c->src_last = b;
        done += nv;
    }
    return VV_OK;
}

// Returns when the copy engine has read every pinned source buffer handed to ..._slices_async so far (copies are in
// order on one stream: the last one's event covers the earlier ones).  Does not wait for promotion kernels.
int vv_load_volume_stream_wait_source(vv_context *c)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "stream_wait_source: NULL context");
    if (c->src_last < 0) return VV_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->src_ev[c->src_last]));
    c->src_last = -1;
    return VV_OK;
}

// A pinned source is read by the copy engine straight from the caller's buffer: do not return before that read is over, or
// a producer that refills the buffer would race it.  (The transfer of a pageable source keeps overlapping the caller's
// next fill; the promotion of a pinned piece overlaps it too.)
int vv_load_volume_stream_slices(vv_context *c, const void *src, int src_type, int z0, int nslices)
{
    int rc = vv_load_volume_stream_slices_async(c, src, src_type, z0, nslices);
    if (rc) return rc;
    return vv_load_volume_stream_wait_source(c);
}

int vv_load_volume_stream_end(vv_context *c)
{
    if (!c || !c->streaming) return fail(c, VV_ERR_INVALID, "stream_end: no stream_begin");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->promo_stream));
    c->streaming = false; c->src_last = -1;
    c->knobs.read();                      // (the pitch knobs are taken as they stand when the volume is complete, as before they moved into vv_knobs)
    { int rc = finalize_layout(c, c->copy_stream); if (rc) return rc; }
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    return VV_OK;
}

int vv_load_volume_t3d(vv_context *c, const char *path, int header, int vtype, const float tf[1024])
{
    if (!c || !path) return fail(c, VV_ERR_INVALID, "vv_load_volume_t3d: NULL argument");
    int nx, ny, nz;
    int rc = vv_t3d_read_header(path, header, &nx, &ny, &nz);
    if (rc) return fail(c, rc, "vv_load_volume_t3d: cannot read the header");
    FILE *f = fopen(path, "rb");                 // before the old volume is given up
    if (!f) return fail(c, VV_ERR_IO, "vv_load_volume_t3d: cannot open file");
    if (header && fseek(f, 24, SEEK_SET) != 0) { fclose(f); return fail(c, VV_ERR_IO, "vv_load_volume_t3d: seek failed"); }
    rc = vv_load_volume_stream_begin(c, vtype, nx, ny, nz, tf);
    if (rc) { fclose(f); return rc; }
    const size_t slice = (size_t)nx * ny;
    int per = (int)std::max<size_t>(1, (32u << 20) / slice);
    std::string buf;
    buf.resize(slice * (size_t)per);
    rc = VV_OK;
    for (int z = 0; z < nz && rc == VV_OK; z += per) {
        const int n = std::min(per, nz - z);
        size_t got = fread(&buf[0], 1, slice * n, f);
        if (got != slice * n) memset(&buf[got], 0, slice * n - got);      // short file: zero tail (reported below)
        int r2 = vv_load_volume_stream_slices(c, buf.data(), VV_VOXEL_U8, z, n);
        if (r2) rc = r2;
        else if (got != slice * n) rc = VV_ERR_IO;
        // the staging copy has consumed buf when the call returns (unpinned source)
    }
    fclose(f);
    int r3 = vv_load_volume_stream_end(c);
    if (rc || r3) {
        // a partly filled volume must not be rendered: drop it, later calls report VV_ERR_NO_VOLUME
        (void)release_volume(c);
        c->streaming = false;
        if (rc == VV_ERR_IO) return fail(c, VV_ERR_IO, "vv_load_volume_t3d: file shorter than its header says");
        return rc ? rc : r3;
    }
    return VV_OK;
}

int vv_volume_dims(const vv_context *c, int dims[3], int *vtype)
{
    if (!c || !c->d_vol) return VV_ERR_NO_VOLUME;
    if (dims) { dims[0] = c->nx; dims[1] = c->ny; dims[2] = c->nz; }
    if (vtype) *vtype = c->vtype;
    return VV_OK;
}

// Pitch of the linear layout.  A row pitch that is a multiple of 1 KiB (1024^3 f32: 4 KiB) puts the four
// rows a sample gathers from (y, y+1, z, z+1) on the same cache channels: the same frame takes 9 % longer
// on a 1024^3 volume than on 1016^3 or 1032^3 (tools/ab_size.sh).  Such volumes are re-pitched on the
// device after the upload: rows get 32 bytes of padding (swept 16...2048: 32, 48 and 96 are best, 128 is
// 4 % behind) and, if a slice would still be a multiple of 4 KiB, one extra row.  Needs the old and the new buffer side by side for a moment; if that does not
// fit, the dense layout stays.  Measured on C3 (A/B on one box): 1.19 -> 1.08 ms although the padded
// 1024^3 volume is 4.4 GB and so takes the 64-bit slice addressing (+3 % by itself); nothing on the Phong
// (+3 % by itself); C3 + Phong 2.52 -> 2.46 ms; 512^3 0.71 -> 0.66 ms and C2 0.245 -> 0.224 ms on the linear path;
// u8 1024^3 0.88 -> 0.77 ms on the linear path (= its z-pair copy), u8 + Phong -1 %; other edge lengths gain 1 %
// (not re-pitched).
// VV_PITCH_PAD=0 disables, VV_PITCH_PAD=<bytes> sets the padding, VV_PITCH_FORCE=1 pads any row length (vv_knobs, read by the caller just before).
static int finalize_layout(vv_context *c, hipStream_t st)
{
    const vv_knobs &K = c->knobs;
    c->prepass_valid = false;              // (every volume load ends here)
    if (K.pitch_pad == 0) return VV_OK;
    const size_t pad_bytes = (size_t)K.pitch_pad;
    const size_t dense_row = c->row_pitch;
    if (dense_row % 1024 != 0 && !K.pitch_force) return VV_OK;
    if (dense_row % 16 != 0) return VV_OK;
    const size_t row = dense_row + pad_bytes;
    size_t rows = (size_t)c->ny;
    if ((rows * row) % 4096 == 0) rows += 1;
    if (K.pitch_rows >= 0 && K.pitch_rows <= 64) rows = (size_t)c->ny + (size_t)K.pitch_rows;
    const size_t slice = rows * row;
    if (slice > 0xFFFFFFF0ull || row >= (1u << 24)) return VV_OK;
    const size_t bytes = slice * (size_t)c->nz, pad = slice + 2 * row + 4096;
    size_t free_b = 0, total_b = 0;
    void *nv = nullptr;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + pad + (512ull << 20) ||
        hipMalloc(&nv, bytes + pad) != hipSuccess) { (void)hipGetLastError(); return VV_OK; }
    HIPCHK(c, hipMemsetAsync(nv, 0, bytes + pad, st));           // padding must be finite (weight-0 corners); so must the data: include/volviz.h, value domain of f32 voxels
    launch_repitch(c->d_vol, nv, dense_row, (size_t)c->ny, (size_t)c->nz, row, slice, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipFree(c->d_vol));
    c->d_vol = nv; c->row_pitch = row; c->slice_pitch = slice; c->alloc_bytes = bytes + pad;
    return VV_OK;
}

// The volume as the kernels of build `b` see it: the linear layout and the copy that build samples (an x-pair frame carries the z-fastest copy
// as well, and the x-pair copy in the z-pair fields).
static VolumeView view_of(const vv_context *c, MarchBuild b)
{
    VolumeView V = {};
    V.data = c->d_vol; V.nx = c->nx; V.ny = c->ny; V.nz = c->nz;
    V.row_bytes = (uint32_t)c->row_pitch;
    V.slice_bytes = (uint32_t)c->slice_pitch;
    V.big = c->slice_pitch * (size_t)c->nz > (1ull << 32) || V.slice_bytes >= (1u << 24) || c->knobs.force_big;
    const layout_copy *cp = c->copies;
    if (b == MB_BRICKED || b == MB_BRICKED_CACHED) { V.bricks = cp[CP_BRICKS].ptr; V.b_sy = cp[CP_BRICKS].row; V.b_sz64 = (uint32_t)cp[CP_BRICKS].slab; }
    if (b == MB_ZFAST || b == MB_XPAIR) { V.zfast = cp[CP_ZFAST].ptr; V.zf_row_bytes = cp[CP_ZFAST].row; V.zf_slice_bytes = cp[CP_ZFAST].slab; }
    const layout_copy &pc = cp[b == MB_XPAIR ? CP_XPAIR : CP_ZPAIR];
    if (b == MB_ZPAIR || b == MB_XPAIR) { V.zpair = pc.ptr; V.zp_row_bytes = pc.row; V.zp_slab_bytes = (uint32_t)pc.slab; }
    return V;
}

// ---- ray march: runCuda, kernel.cu:388-453 ----------------------------------------
static inline float vlen_h(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }

// camera basis of the analytic ray source (shared by vv_render and vv_first_pass)
static int camera_basis(vv_context *c, FrameParams &P, const camera_params *cam, const vv_ray_source *rays, int W, int H)
{
    // camera.cpp:78-91 look-at basis, float
    float lx = rays->look[0], ly = rays->look[1], lz = rays->look[2];
    float ll = vlen_h(lx, ly, lz);
    if (!(ll > 0.f)) return fail(c, VV_ERR_INVALID, "vv_render: look vector is zero");
    lx /= ll; ly /= ll; lz /= ll;
    float ux = rays->up[0], uy = rays->up[1], uz = rays->up[2];
    float sx = ly * uz - lz * uy, sy = lz * ux - lx * uz, sz = lx * uy - ly * ux;
    float sl = vlen_h(sx, sy, sz);
    if (!(sl > 0.f)) return fail(c, VV_ERR_INVALID, "vv_render: up vector is parallel to look");
    sx /= sl; sy /= sl; sz /= sl;
    float vx = sy * lz - sz * ly, vy = sz * lx - sx * lz, vz = sx * ly - sy * lx;
    float vl = vlen_h(vx, vy, vz);
    vx /= vl; vy /= vl; vz /= vl;
    P.look[0] = lx; P.look[1] = ly; P.look[2] = lz;
    P.side[0] = sx; P.side[1] = sy; P.side[2] = sz;
    P.up[0] = vx; P.up[1] = vy; P.up[2] = vz;
    float aspect = rays->aspect > 0.f ? rays->aspect : (float)W / (float)H;
    float th = (float)tan((double)cam->fovY * M_PI / 360.0);
    P.tan_half_x = th * aspect; P.tan_half_y = th;
    return VV_OK;
}


} // extern "C"

// ---- launch policy of vv_render (speed only: the pixels never depend on anything decided here) -----------------------------------------------
// From what is known about the view (`have_basis`: P.side holds the screen x direction in volume space; `density`: voxels of volume per sample, 1e9 =
// unknown) it picks the layout the frame samples (building a missing copy when the context allows it), the wave tile and block shape, the samples in
// flight per lane and the blocks per CU, and fills MarchArgs accordingly.  Every threshold below carries the measurement it comes from; the VV_* knobs
// override single decisions for A/Bs.  Sets MarchArgs::build, the kernel build the frame runs.  Returns whether the volume is beyond the caches.
static bool choose_launch(vv_context *c, MarchArgs &A, const camera_params *cam, const vv_ray_source *rays, const shading_params *shading,
                          bool have_basis, float density, int H, hipStream_t st)
{
    FrameParams &P = A.P;
    A.V_type = c->vtype;
    // Wave tile shape (speed only): memory is contiguous along the volume's x axis.  When the
    // screen x direction maps (almost) onto it, a 32x2 tile lets the 32 lanes of a row read one
    // or two cache lines (measured C3, view along z: 1.6 ms vs 2.1 ms for 8x8); otherwise the
    // compact 8x8 tile touches the fewest lines.  VV_TILE_LOG2W overrides (3, 4 or 5).
    A.strips.tile_log2w = 3;
    if (have_basis) {
        const float ax = fabsf(P.side[0]) , ay = fabsf(P.side[1]), az = fabsf(P.side[2]);
        if (ax >= 0.97f * sqrtf(ax * ax + ay * ay + az * az)) A.strips.tile_log2w = 5;
    }
    const vv_knobs &K = c->knobs;
    // Sampling density: voxels of volume per sample = (voxels per step) x (voxels per pixel)^2 at the
    // cube centre.  Sparse rays (C3 at 1080p: 4.9) reuse little of a cache line and want few waves on a CU's
    // L1; the denser frames of the multi-GPU configurations (2716x1528: 2.5, 3840x2160: 1.2, and 0.6 at
    // step 1/1024) want more: the whole 3840x2160 / 1024-step frame takes 3.51 ms with 2 blocks per CU and
    // 2.71 ms with 4 (tools/sweep.sh --frame-of 8; bricked copy 4.71 -> 3.34 ms, Phong 9.0 -> 7.9 ms).
    if ((rays->mode == VV_RAYS_ANALYTIC || image_source_has_hint(rays)) && have_basis && H > 0) {
        const float dist = vlen_h(cam->origin[0], cam->origin[1], cam->origin[2]);
        const float vpw = cbrtf(((float)c->nx / (2.f * P.scale[0])) * ((float)c->ny / (2.f * P.scale[1])) * ((float)c->nz / (2.f * P.scale[2])));
        const float px_vox = 2.f * P.tan_half_y * dist / (float)H * vpw;
        const float step_vox = fmaxf(P.step[0] * c->nx, fmaxf(P.step[1] * c->ny, P.step[2] * c->nz));
        if (std::isfinite(px_vox) && std::isfinite(step_vox) && px_vox > 0.f && step_vox > 0.f) density = step_vox * px_vox * px_vox;
    }
    // z-fastest copy (speed only): when the screen x direction maps onto the volume's z axis (side views) the same 32 x 2 tile reads whole
    // lines of a copy whose rows run along z -- the front view's kernel instead of the bricked copy's (C3 1.33 -> 1.0 ms, C2 0.223 -> 0.186,
    // profiles/r04_side_view.txt).  Both voxel types, both kernels, every volume the bricked copy would serve; built on first use if HBM has
    // room (one more copy of the volume).  VV_ZFAST=0/1 overrides.
    bool use_zfast = false;
    if (have_basis && A.strips.tile_log2w == 3) {
        const float ax = fabsf(P.side[0]) , ay = fabsf(P.side[1]), az = fabsf(P.side[2]);
        use_zfast = az >= 0.97f * sqrtf(ax * ax + ay * ay + az * az) && big_enough_for_copies(c);
        if (K.zfast >= 0) use_zfast = K.zfast != 0;
    }
    // Phong frames of f32 volumes beyond the caches sample the bricked copy from every direction: march_phong_kernel's blocks are 16 pixels wide whatever the
    // view, and 16 pixels of a row use 0.8 of the 1.8 lines they touch in a linear layout, while a 4 x 4 x 4 brick is used whole.  Measured:
    // C3 + Phong along z 1.750 -> 1.650 ms (-5.5 %), from the side (z-fastest copy) 1.758 -> 1.666; volumes in the caches lose 20 % (VALU-bound): not for those.
    // The 32 GiB volume of C5 (a pixel every 3.2 voxels: a brick serves 1.5 pixels a side) loses 9 %, the dense frame of the 8-GPU configuration 15 %, 768^3
    // (1.8 GiB, 2.2 voxels per sample) 12 %: for sparse frames (3.5 ... 8 voxels per sample) of volumes between 2 and 8 GiB.  VV_PHONG_BRICKS=0/1 overrides.
    const bool phong_bricks_fit = K.phong_bricks > 0 || (density > 3.5f && density <= 8.f && c->vol_bytes > (2ull << 30) && c->vol_bytes <= (8ull << 30));
    const bool phong_bricks = phong_bricks_fit && shading->phongShading && c->vol_bytes > (1ull << 30) && c->vtype == VV_VOXEL_F32 && K.bricked != 0 && K.phong_bricks != 0 &&
                              (c->copies[CP_BRICKS].valid || (c->build_in_render && !c->copies[CP_BRICKS].failed));
    if (phong_bricks && K.zfast < 0) use_zfast = false;
    ++c->frame_no;
    auto copies_valid = [c] { int n = 0; for (const layout_copy &cp : c->copies) n += cp.valid; return n; };
    const int valid_before = copies_valid();
    if (use_zfast) use_zfast = take_copy(c, CP_ZFAST, st);
    if (use_zfast) A.strips.tile_log2w = 5;
    if (K.tile_log2w >= 3 && K.tile_log2w <= 5 && !use_zfast) A.strips.tile_log2w = K.tile_log2w;
    // Occupancy cap + gathers in flight (speed only; measured on MI355X, profiles/EXPERIMENTS.md part B section 4):
    //   volume beyond the caches (> 1 GiB), aligned view : 2 blocks per CU, 3 samples per trip
    //   volume beyond the caches, rotated, linear layout : 1 block  per CU, 3 samples per trip
    //   smaller volumes                                  : 4 blocks per CU, 3 (aligned) / 2 samples per trip
    //   bricked copy (below)                             : 2 / 4 blocks per CU, 2 samples per trip
    // LDS per block = 4 KB table + reserve; 160 KB per CU.  VV_LDS_RESERVE / VV_UNROLL override.
    // XCD-aware block order: XCD k renders strips k, k+8, ... (each a full-width row of tiles), so
    // the tiles that share volume cache lines share an L2 (measured: -4 % on every workload)
    A.strips.xcd_band = 1;
    if (K.xcd_band >= 0 && K.xcd_band <= 64) A.strips.xcd_band = K.xcd_band;
    const bool beyond_caches = c->vol_bytes > (1ull << 30);
    const int big_reserve = density > 3.5f ? 76000 : (density > 1.8f ? 49000 : 36000);   // 2 / 3 / 4 blocks per CU
    // 3 samples per trip along the memory axis (A/B with repeats on MI355X: C3 -1.6 %, C2 -5.7 %, 512^3 -10 %,
    // u8 1024^3 -6.5 %; 4 per trip is no better), 2 on the bricked copy (3 there: +3.5 %)
    A.unroll = (A.strips.tile_log2w == 5 || beyond_caches) ? 3 : 2;
    // (re-swept with tools/ab_reserve.sh at the end of round 1: 4 blocks per CU for volumes up to 1 GiB)
    A.lds_reserve = !beyond_caches ? 36000 : (A.strips.tile_log2w == 5 ? big_reserve : 155000);
    // Block shape (speed only).  32 x 2 wave tiles: stacked (32 x 8 pixels), 2 x 2 (64 x 4) or side by side (128 x 2): the partial lines two x-adjacent wave
    // tiles share are then fetched within one block; strips get lower.  8 x 8 wave tiles: side by side (32 x 8), 2 x 2 (16 x 16) or stacked (8 x 32).  VV_BLOCK_W=8...128.
    //   measured (tools/ab_env.sh, profiles/r03_block_shape.txt): 64 x 4: C3 -2.4 % (EA bytes 1.474 -> 1.364 x algorithmic), u8 1024^3 -1.3 %, tilted views -1.7 %, but
    //   +4.5 % on C2, +1 % on C1 / 512^3 and +0.5 % on the dense frames of the multi-GPU configurations: used for sparse frames of volumes beyond the caches.
    //   16 x 16: a strip 16 pixels high re-reads fewer brick layers of its neighbours (which run on other XCDs): rotated C3 -2 % (EA bytes 2.00 -> 1.81 x), C2 -5.5 %,
    //   C1 -6.5 %, other orbits -2 ... -4 %, 512^3 and the 3840 x 2160 frame -0.5 %: used for every frame with 8 x 8 tiles.
    A.strips.blk_log2w = 5;
    A.strips.tail_batch = K.tail == 0 ? 0 : 1;
    const int rows_px_8 = A.strips.n_strips * 8;              // (the shard's pixel rows as strips of 8)
    int block_w = A.strips.tile_log2w == 3 ? 16 : ((A.strips.tile_log2w == 5 && c->vol_bytes >= (1ull << 30) && density > 3.5f) ? 64 : 32);      // (>=: u8 1024^3 -2 %, tools/policy_sweep.sh)
    if (K.block_w >= 8 && K.block_w <= 128 && (K.block_w & (K.block_w - 1)) == 0) block_w = K.block_w;
    {
        int lw = 3; while ((1 << lw) < block_w) ++lw;
        const int h = 256 >> lw;                               // strip height in pixels
        if (lw != 5 && lw >= A.strips.tile_log2w && h >= (64 >> A.strips.tile_log2w)) {     // (a block is at least one wave tile wide and high)
            A.strips.blk_log2w = lw;
            // rows past the end of a band or of the range belong to nobody or to another rank: not owned (row_owned), their lanes stay idle
            if (A.strips.strips_per_band < (1 << 26)) {
                const int band_px = A.strips.strips_per_band * 8, spb = (band_px + h - 1) / h;
                A.strips.n_strips = (rows_px_8 / band_px) * spb; A.strips.strips_per_band = spb;
            } else A.strips.n_strips = (rows_px_8 + h - 1) / h;
        }
    }
    const bool k_unroll = K.unroll >= 1 && K.unroll <= 3, k_reserve = K.lds_reserve >= 0 && K.lds_reserve <= 155 * 1024;
    if (k_unroll) A.unroll = K.unroll;
    if (k_reserve) A.lds_reserve = K.lds_reserve;
    // Bricked copy (speed only): off the memory axis the linear layout costs one cache line per lane
    // and gather; 4x4x4 bricks keep a wave's footprint in a few dozen lines.  both voxel types, both kernels;
    // built on first use if HBM has room (1.25x an f32 volume, 2x a u8 volume).  VV_BRICKED=0/1 overrides the policy.
    // Measured: 1024^3 rotated 3.85 -> 1.65 ms (f32), 3.17 -> 0.99 ms (u8); C2 (256^3) -19 %, C1 (128^3) -9 %;
    // only volumes far below the frame's sampling density lose (64^3 at 1080p, step 1/512: +10 %).
    bool use_bricks = (A.strips.tile_log2w == 3 || phong_bricks) && big_enough_for_copies(c);
    if (K.bricked >= 0) use_bricks = K.bricked != 0;
    if (use_zfast) use_bricks = false;
    if (use_bricks) use_bricks = take_copy(c, CP_BRICKS, st);
    if (use_bricks) {
        // measured (C3 rotated, 1024^3): 2 blocks per CU and 2 samples per trip: 3.64 -> 1.60 ms
        if (!k_unroll) A.unroll = 2;
        if (!k_reserve) A.lds_reserve = beyond_caches ? big_reserve : 36000;
    }
    // z-pair copy (speed only): along the memory axis the four corners (x..x+1, z..z+1) of a row come
    // from one gather (16 bytes for f32, 4 for u8), so a sample costs 2 gathers instead of 4 (f32) or 8
    // aligned dwords (u8).  2x the volume in HBM.  Measured on MI355X, unshaded frames:
    //   f32: -7 % on C1/C2, -10 % on 256^3 at C3's frame, -3 % on 512^3, but +6 % on 768^3 and +20 % on
    //        1024^3 (rays of different z phase stop sharing slices in L2): used up to 512 MiB;
    //   u8 : -8 % (256^3), -12 % (512^3), -4 % (1024^3): used whenever the copy stays below 4 GiB;
    //   Phong path: 0...-3 %: not used.                                  VV_ZPAIR=0/1 overrides.
    bool use_zpair = !use_bricks && A.strips.tile_log2w == 5 && !shading->phongShading && pair_copies_allowed(c);
    if (K.zpair >= 0) use_zpair = K.zpair != 0 && !use_bricks;
    if (use_zfast) use_zpair = false;
    if (use_zpair) use_zpair = take_copy(c, CP_ZPAIR, st);
    // x-pair copy (speed only): the same two-gather form for side views -- the z-pair copy with x and z exchanged, handed to the kernel in the
    // z-pair fields of the view -- under the z-pair copy's conditions (unshaded, u8 or f32 up to 512 MiB).  Follows VV_ZPAIR=0.
    const bool use_xpair = use_zfast && !shading->phongShading && K.zpair != 0 && pair_copies_allowed(c) && take_copy(c, CP_XPAIR, st);
    const int valid_after = copies_valid();
    if (valid_after > valid_before) c->builds_in_render += valid_after - valid_before;
    // The kernel build.  Linear volumes beyond the caches take the 64-bit-addressing build in Phong frames even below 4 GiB: the other one is compiled
    // for 5 waves per SIMD, which only cache-resident volumes want (1000^3 f32: 1.884 -> 1.817 ms, tools/ab_env.sh VV_FORCE_BIG=1).
    A.build = use_xpair ? MB_XPAIR : use_zfast ? MB_ZFAST : use_bricks ? (beyond_caches ? MB_BRICKED : MB_BRICKED_CACHED) : use_zpair ? MB_ZPAIR :
              (view_of(c, MB_LINEAR).big || (shading->phongShading && beyond_caches)) ? MB_LINEAR_BIG : MB_LINEAR;
    A.V = view_of(c, A.build);
    // Phong kernel: 14.3 KB of LDS per block + this reserve.  Measured (tools/ab_phong.sh): volumes up to
    // 1 GiB like 5 blocks per CU (C2 0.54 -> 0.47 ms against no cap, u8 1024^3 1.88 -> 1.78), the 4 GiB
    // volume of C3 3 blocks (2.77 ms with 2, 2.48 with 3, 2.54 with 4), the 32 GiB volume of C5 2 (18.2 vs 20.2 ms)
    // (re-swept with the depth-limited refresh, tools/ab_phong_reserve.sh: C3 1.97 ms with 3, 4 or 5 blocks, 2.22 with 2; the
    // bricked copy likes 5: rotated C3 + Phong 2.25 -> 2.13 ms; C5 5.95 ms with 2, 6.25 with 3, 6.55 with 5)
    A.lds_reserve_phong = c->vol_bytes > (8ull << 30) ? 40000 : ((beyond_caches && density > 3.5f && !use_bricks) ? 30000 : 13000);
    if (K.lds_reserve_phong >= 0 && K.lds_reserve_phong <= 146 * 1024) A.lds_reserve_phong = K.lds_reserve_phong;
    c->last_density = density;
    return beyond_caches;
}

// The volume's screen rectangle (speed only in intent, but the frame relies on it: see below).  Analytic rays only.  Of C3's 8100 tiles 5150 lie beside the
// cube: blocks that set up 256 rays, find none alive and leave -- 2 us each, plus the ~4 us a slot stands empty between two blocks (per-block time stamps,
// tools/timeline.py): together 6 % of the frame's slot time.  march_kernel is therefore launched over the tiles under the cube's bounding rectangle only, and
// rad_kernel, which visits every slab anyway, writes the 0 of the pixels outside it and skips the radii nobody reads.
// The rectangle must contain every pixel whose ray meets the cube.  A ray that meets the cube passes through a point of it, so its pixel lies in the convex hull
// of the eight projected corners -- in exact arithmetic.  ray_endpoints decides in binary32: its direction carries an error of a few ulps (|d| ~ 1) and its slab
// test errors of a few ulps of (|o| + s) / |d_a|; a ray can be taken for a hit only if it passes the cube within ~1e-6 (|o| + s).  Seen from the eye that is an
// angle of at most 1e-6 (|o| + s) / depth_min, which the margin below covers a hundred times over, expressed in pixels (+ 1); a corner at or behind the eye's plane
// (depth <= 1e-3 (|o| + s)), a margin wider than the frame or anything non-finite: no rectangle, the whole frame is launched as before.
static bool screen_rect(const MarchArgs &A, int W, int H, double *xmin, double *xmax, double *ymin, double *ymax)
{
    const FrameParams &P = A.P;
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY}, dmin = INFINITY, ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, (double)fabsf(P.cam_pos[a]) + (double)P.scale[a]);
    for (int k = 0; k < 8; ++k) {
        const double v[3] = {((k & 1) ? P.scale[0] : -P.scale[0]) - (double)P.cam_pos[0], ((k & 2) ? P.scale[1] : -P.scale[1]) - (double)P.cam_pos[1],
                             ((k & 4) ? P.scale[2] : -P.scale[2]) - (double)P.cam_pos[2]};
        const double depth = v[0] * P.look[0] + v[1] * P.look[1] + v[2] * P.look[2];
        if (!(depth > 1e-3 * ext)) return false;
        dmin = std::min(dmin, depth);
        const double sx = (v[0] * P.side[0] + v[1] * P.side[1] + v[2] * P.side[2]) / depth, sy = (v[0] * P.up[0] + v[1] * P.up[1] + v[2] * P.up[2]) / depth;
        const double px = (sx / P.tan_half_x + 1.0) * 0.5 * W - 0.5, py = (sy / P.tan_half_y + 1.0) * 0.5 * H - 0.5;     // (ray_endpoints' pixel centres)
        lo[0] = std::min(lo[0], px); hi[0] = std::max(hi[0], px); lo[1] = std::min(lo[1], py); hi[1] = std::max(hi[1], py);
    }
    const double ang = 1e-4 * ext / dmin;                                                       // (100 x the bound above)
    const double mx = 1.0 + ang / (2.0 * P.tan_half_x / W), my = 1.0 + ang / (2.0 * P.tan_half_y / H);
    if (!std::isfinite(lo[0] + hi[0] + lo[1] + hi[1] + mx + my) || mx > W || my > H) return false;
    *xmin = lo[0] - mx; *xmax = hi[0] + mx; *ymin = lo[1] - my; *ymax = hi[1] + my;
    return true;
}

static void launch_build(FrameKind kind, const MarchArgs &A, hipStream_t st) { assert(A.build < MB_COUNT); kLaunch[frame_row(kind)][A.build](A, st); }

// One output image of a frame.  render_frame describes the four once (rgba, index, hit, stat: the order of every enqueued copy) and stages, checks and
// reads them back in loops over that table.
struct FrameImage {
    void *host;                         // the caller's buffer (on the device when out_on_device), or null: not asked for
    size_t px_bytes;                    // bytes per pixel
    int scratch;                        // the context's staging buffer of a host-buffer frame (SC_*)
    unsigned align;                     // of the device pointer the kernels write through (a record is written in one store)
    const char *misaligned;             // vv_last_error text of a misaligned device pointer
    uint8_t *dev;                       // where the kernels write: `host` itself, or the scratch entry
};

// What the stages of render_frame hand on to each other.
struct Frame {
    MarchArgs A;
    FrameKind kind; int W, H; hipStream_t st;
    bool have_basis; float density;     // what the launch policy knows about the view: P.side is filled in; voxels of volume per sample (unknown ray source: sparse)
    bool beyond_caches;                 // choose_launch's verdict
    bool rect_limits; PixelRect fill_rect;      // unshaded frames: the screen rectangle limits the launch; the pixels the tiles cover (what launch_fill leaves alone)
    bool whole;                         // the frame writes the whole (W-1) x (H-1) rectangle: no shards, no row limits
    FrameImage img[4];
};

// stage 1: the arguments every frame kind checks before it touches the device
static int check_frame_args(vv_context *c, int W, int H, const slice_params *slice, const camera_params *cam, const vv_ray_source *rays)
{
    if (W < 1 || H < 1) return fail(c, VV_ERR_INVALID, "vv_render: width/height must be >= 1");
    if (!c->d_vol || !c->have_tf) return fail(c, VV_ERR_NO_VOLUME, "vv_render: no volume / transfer function loaded");
    if (slice->type != SLICE_NONE && slice->type != SLICE_PLANE && slice->type != SLICE_PLANE_CUT)
        return fail(c, VV_ERR_INVALID, "vv_render: slice type must be SLICE_NONE/PLANE/PLANE_CUT");
    if (rays->mode == VV_RAYS_IMAGES && (!rays->front || !rays->back || rays->img_w < 1 || rays->img_h < 1))
        return fail(c, VV_ERR_INVALID, "vv_render: image ray source needs front/back images");
    if (rays->mode != VV_RAYS_IMAGES && rays->mode != VV_RAYS_ANALYTIC)
        return fail(c, VV_ERR_INVALID, "vv_render: bad ray source mode");
    for (int a = 0; a < 3; ++a)
        if (!(cam->scale[a] > 0.f) || !std::isfinite(cam->scale[a]))
            return fail(c, VV_ERR_INVALID, "vv_render: camera scale must be finite and > 0");
    return VV_OK;
}

// stage 2: options and camera -> FrameParams, and the grid maps of the shard / slab rows this call launches
static int frame_params(vv_context *c, Frame &F, const slice_params *slice, const camera_params *cam, const vv_ray_source *rays, const vv_render_options *opts)
{
    MarchArgs &A = F.A;
    FrameParams &P = A.P;
    const int W = F.W, H = F.H;
    const bool reducer = F.kind != FRAME_COMPOSITE;
    P.W = W; P.H = H;
    P.nbx = W / kSlab + ((W % kSlab) ? 1 : 0);                         // kernel.cu:418-425
    P.nby = H / kSlab + ((H % kSlab) ? 1 : 0);
    P.conflict_x = (W >= 2 && W - 1 == (P.nbx - 1) * kSlab);
    P.conflict_y = (H >= 2 && H - 1 == (P.nby - 1) * kSlab);
    int rb = 0, re = P.nby;
    int s_count = 1, s_index = 0, s_band = 4;
    P.step[0] = 1.f / (float)c->nx; P.step[1] = 1.f / (float)c->ny; P.step[2] = 1.f / (float)c->nz;   // :415
    P.ert_thr = .95f; P.ert_true = 0; P.alpha_unit = c->tf_alpha_unit;
    A.tex8 = true; A.instr = false;
    if (opts) {
        if (opts->step[0] > 0.f || opts->step[1] > 0.f || opts->step[2] > 0.f) {
            P.step[0] = opts->step[0]; P.step[1] = opts->step[1]; P.step[2] = opts->step[2];
        }
        if (opts->ert_threshold > 0.f) P.ert_thr = opts->ert_threshold;
        P.ert_true = opts->ert_mode == VV_ERT_TRUE;
        A.tex8 = opts->filter != VV_FILTER_EXACT;
        if (!(opts->slab_row_begin == 0 && opts->slab_row_end == 0)) { rb = opts->slab_row_begin; re = opts->slab_row_end; }
        if (opts->shard_count > 1) { s_count = opts->shard_count; s_index = opts->shard_index; s_band = opts->shard_band; }
        A.instr = opts->count_samples != 0 || opts->touched_bricks != nullptr || opts->touched_lines != nullptr || opts->touched_block_lines != nullptr;
        if (opts->touched_block_lines && (opts->touched_block_lines_log2 < 10 || opts->touched_block_lines_log2 > 34))
            return fail(c, VV_ERR_INVALID, "vv_render: touched_block_lines_log2 must lie in [10, 34]");
        A.I.pairs = opts->touched_block_lines; A.I.pairs_log2 = (uint32_t)opts->touched_block_lines_log2;
        A.I.bricks = opts->touched_bricks;
        A.I.lines = opts->touched_lines; A.I.line_bits = opts->touched_lines ? opts->touched_line_bits : 0; A.I.lines_all = opts->touched_lines_all;
    }
    float min_step = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (!(P.step[a] >= kStepMin) || !std::isfinite(P.step[a]))
            return fail(c, VV_ERR_INVALID, "vv_render: step must be finite and >= 1e-5 per axis");
        min_step = fminf(min_step, P.step[a]);
    }
    if (rb < 0 || re > P.nby || rb > re) return fail(c, VV_ERR_INVALID, "vv_render: slab row range out of bounds");
    // chunks needed for the longest possible ray (upper <= sqrt 3, kernel.cu:350) + slack
    P.max_chunks = (int)(kSqrt3 / (min_step * kChunkSteps)) + 4;
    if (s_count > 1 && (s_band < 4 || s_band % 4 != 0 || s_index < 0 || s_index >= s_count))
        return fail(c, VV_ERR_INVALID, "vv_render: shard_band must be a positive multiple of 4, 0 <= shard_index < shard_count");
    P.rb = rb; P.re = re; P.band = s_band; P.count = s_count; P.index = s_index;
    // grid maps (see vv_kernels.h): which strips / slab rows this call launches
    const int last_written = H >= 2 ? H - 2 : 0;
    const int geo_rows = last_written / kSlab + 1;            // slab rows that own pixel rows geometrically
    if (s_count > 1) {
        const int nbands = (geo_rows + s_band - 1) / s_band;
        const int own = s_index < nbands ? (nbands - s_index + s_count - 1) / s_count : 0;
        A.strips.y0 = s_index * s_band * kSlab; A.strips.strips_per_band = s_band * kSlab / 8;
        A.strips.band_stride_px = s_count * s_band * kSlab;
        A.strips.n_strips = own * A.strips.strips_per_band;
        A.slabs.r0 = s_index * s_band; A.slabs.band = s_band; A.slabs.band_stride = s_count * s_band;
        A.slabs.n_regular = own * s_band;
    } else {
        const int r_lo = rb, r_hi = re < geo_rows ? re : geo_rows;
        const int y_lo = r_lo * kSlab, y_hi = (r_hi * kSlab < last_written + 1) ? r_hi * kSlab : last_written + 1;
        A.strips.y0 = y_lo; A.strips.strips_per_band = 1 << 28; A.strips.band_stride_px = 0;
        A.strips.n_strips = y_hi > y_lo ? (y_hi - y_lo + 7) / 8 : 0;
        A.slabs.r0 = r_lo; A.slabs.band = 1 << 28; A.slabs.band_stride = 0;
        A.slabs.n_regular = r_hi > r_lo ? r_hi - r_lo : 0;
    }
    P.slice_type = (reducer && slice->type == SLICE_PLANE) ? SLICE_NONE : slice->type;      // (a MIP / iso / projection frame has no highlight to draw: SLICE_PLANE marches as SLICE_NONE)
    for (int a = 0; a < 3; ++a) {
        P.slice_point[a] = slice->params[a]; P.slice_normal[a] = slice->params[3 + a];   // kernel.cu:224-225
        P.cam_pos[a] = cam->origin[a]; P.scale[a] = cam->scale[a];
        P.inv_scale[a] = 1.0f / cam->scale[a];
    }
    // kernel.cu:221-222: float * double / float -> double; tan in double; narrowed
    P.tan_fov_x = (float)tan((double)cam->fovX * M_PI / (double)(180.f * (float)(unsigned)W));
    P.tan_fov_y = (float)tan((double)cam->fovY * M_PI / (double)(180.f * (float)(unsigned)H));
    {
        const float lo = kSafeDivTanLo, hi = kSafeDivTanHi;                                 // (vv_gate.h: host/device_math_check.hip sweeps the cores over these ranges)
        P.safe_div = P.tan_fov_x >= lo && P.tan_fov_x <= hi && P.tan_fov_y >= lo && P.tan_fov_y <= hi &&
                     P.step[0] <= kSafeDivStepMax && P.step[1] <= kSafeDivStepMax && P.step[2] <= kSafeDivStepMax;          // (>= kStepMin and finite: checked above)
    }
    P.ray_mode = rays->mode; P.quantize8 = rays->quantize8;
    return VV_OK;
}

// stage 3: what the launch policy knows about the view (speed only): the camera basis -- given (analytic rays), hinted (an image
// source whose look / up fields are filled in: the host that drew the first pass knows its camera) or estimated from the images.
// Host images of an image ray source are uploaded here.
static int view_knowledge(vv_context *c, Frame &F, const camera_params *cam, const vv_ray_source *rays, void *stream)
{
    FrameParams &P = F.A.P;
    const int W = F.W, H = F.H;
    hipStream_t st = F.st;
    bool &have_basis = F.have_basis;
    float &density = F.density;
    have_basis = false;
    density = 1e9f;                                 // voxels of volume per sample; unknown ray source: treat as sparse
    if (rays->mode == VV_RAYS_ANALYTIC) {
        int brc = camera_basis(c, P, cam, rays, W, H);
        if (brc) return brc;
        have_basis = true;
    } else {
        if (image_source_has_hint(rays)) have_basis = camera_basis(nullptr, P, cam, rays, W, H) == VV_OK;
        const size_t ib = (size_t)rays->img_w * rays->img_h * 4;
        P.img_w = rays->img_w; P.img_h = rays->img_h;
        if (rays->images_on_device) {
            if (((uintptr_t)rays->front & 3) || ((uintptr_t)rays->back & 3)) return fail(c, VV_ERR_INVALID, "vv_render: device images must be 4-byte aligned");
            P.front_img = rays->front; P.back_img = rays->back;
        }
        else {
            int rc = ensure(c, SC_IMG, 2 * ib);
            if (rc) return rc;
            uint8_t *d_img = (uint8_t *)c->scratch[SC_IMG].p;
            HIPCHK(c, hipMemcpyAsync(d_img, rays->front, ib, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_img + ib, rays->back, ib, hipMemcpyHostToDevice, st));
            P.front_img = d_img; P.back_img = d_img + ib;
        }
        // no hint: the images themselves say how screen x runs through the volume and how dense the rays are.  Host images are
        // read in place; device images only by a synchronous call (an enqueue-only call must not wait for the stream), and the
        // estimate is kept while camera and image geometry stay the same.
        if (!have_basis) {
            bool est = false;
            float side[3] = {0, 0, 0}, px_cube = 0.f;
            if (!rays->images_on_device) est = estimate_view_from_images(rays->front, rays->back, rays->img_w, rays->img_h, W, H, side, &px_cube);
            else if (!stream) {
                const vv_view_key key = view_key_of(cam, rays, W, H);
                if (c->view_key_valid && memcmp(&c->view_key, &key, sizeof key) == 0) { est = c->view_est_ok; memcpy(side, c->view_side, sizeof side); px_cube = c->view_px_cube; }
                else {
                    const int yt = clamp_row((H / 2) * (long long)rays->img_h / H, rays->img_h);
                    const size_t rowb = (size_t)rays->img_w * 4;
                    c->row_buf.resize(2 * rowb);
                    HIPCHK(c, hipStreamSynchronize(st));
                    HIPCHK(c, hipMemcpy(c->row_buf.data(), rays->front + (size_t)yt * rowb, rowb, hipMemcpyDeviceToHost));
                    HIPCHK(c, hipMemcpy(c->row_buf.data() + rowb, rays->back + (size_t)yt * rowb, rowb, hipMemcpyDeviceToHost));
                    // (the centre row alone, presented as a one-row image pair)
                    est = estimate_view_from_images(c->row_buf.data(), c->row_buf.data() + rowb, rays->img_w, 1, W, 1, side, &px_cube);
                    c->view_key = key; c->view_key_valid = true; c->view_est_ok = est; memcpy(c->view_side, side, sizeof side); c->view_px_cube = px_cube;
                }
            }
            if (est) {
                P.side[0] = side[0]; P.side[1] = side[1]; P.side[2] = side[2];
                have_basis = true;
                // px_cube = cube-space distance between horizontally neighbouring pixels' rays at mid depth
                const float vpw = cbrtf((float)c->nx * (float)c->ny * (float)c->nz);
                const float px_vox = px_cube * vpw;
                const float step_vox = fmaxf(P.step[0] * c->nx, fmaxf(P.step[1] * c->ny, P.step[2] * c->nz));
                if (std::isfinite(px_vox) && px_vox > 0.f && step_vox > 0.f) density = step_vox * px_vox * px_vox;
            }
        }
    }
    return VV_OK;
}

// stage 4: the unshaded kernels' tiles / march_phong_kernel's slabs: those under the volume's screen rectangle (screen_rect), or all of them
static void tiles_under_rect(const vv_context *c, Frame &F, const vv_ray_source *rays)
{
    MarchArgs &A = F.A;
    const FrameParams &P = A.P;
    const int W = F.W, H = F.H, s_count = P.count;
    bool &rect_limits = F.rect_limits;
    rect_limits = false;
    StripMap &M = A.strips;
    const int bw = 1 << M.blk_log2w, bh = 256 >> M.blk_log2w;
    M.tx0 = 0; M.wr = (W + bw - 1) >> M.blk_log2w; M.s0 = 0; M.s1 = M.n_strips;
    A.rect.x0 = 0; A.rect.y0 = 0; A.rect.x1 = INT_MAX; A.rect.y1 = INT_MAX;
    double xmin, xmax, ymin, ymax;
    SlabMap &S = A.slabs;
    S.gx0 = 0; S.wg = P.nbx; S.gs0 = 0; S.gs1 = S.n_regular;
    A.fill_outside = false;
    const bool have_rect = c->knobs.rect != 0 && rays->mode == VV_RAYS_ANALYTIC && W >= 2 && H >= 2 && screen_rect(A, W, H, &xmin, &xmax, &ymin, &ymax);
    if (have_rect && A.phong && S.n_regular > 0) {
        // march_phong_kernel: the slabs whose own 14 x 14 pixels meet the rectangle.  A pixel is written by the slab that owns it (pin 10): when W == 1 (mod 14)
        // pixel column W-2 lies in slab column nbx-2 and belongs to nbx-1, which therefore comes along; the extra slab row is always launched.
        auto slab_of = [](double v, int lo, int hi) { const double t = floor(v / kSlab); return t < lo ? lo : (t > hi ? hi : (int)t); };
        int gx0 = slab_of(xmin, 0, P.nbx), gx1 = slab_of(xmax, -1, P.nbx - 1) + 1;
        if (P.conflict_x && gx1 == P.nbx - 1) gx1 = P.nbx;
        if (gx1 < gx0) gx1 = gx0;
        S.gx0 = gx0; S.wg = gx1 - gx0;
        A.rect.x0 = gx0 * kSlab; A.rect.x1 = gx1 >= P.nbx ? INT_MAX : gx1 * kSlab;
        if (s_count <= 1) {
            S.gs0 = slab_of(ymin, S.r0, S.r0 + S.n_regular) - S.r0; S.gs1 = slab_of(ymax, S.r0 - 1, S.r0 + S.n_regular - 1) + 1 - S.r0;
            if (S.gs1 < S.gs0) S.gs1 = S.gs0;
            A.rect.y0 = (S.r0 + S.gs0) * kSlab; A.rect.y1 = (S.r0 + S.gs1) * kSlab;
        }
        if (S.wg == 0 || S.gs1 == S.gs0) { S.wg = 0; A.rect.x0 = A.rect.x1 = A.rect.y0 = A.rect.y1 = 0; }
        A.fill_outside = true;
    }
    if (have_rect && !A.phong && M.n_strips > 0) {
        auto tile_of = [](double v, int unit, int lo, int hi) { const double t = floor(v / unit); return t < lo ? lo : (t > hi ? hi : (int)t); };
        const int ntx = M.wr;
        M.tx0 = tile_of(xmin, bw, 0, ntx); M.wr = tile_of(xmax, bw, -1, ntx - 1) + 1 - M.tx0;
        if (s_count <= 1) { M.s0 = tile_of(ymin - M.y0, bh, 0, M.n_strips); M.s1 = tile_of(ymax - M.y0, bh, -1, M.n_strips - 1) + 1; }
        if (M.wr < 0) M.wr = 0;
        if (M.s1 < M.s0) M.s1 = M.s0;
        A.rect.x0 = M.tx0 * bw; A.rect.x1 = (M.tx0 + M.wr) * bw;
        if (s_count <= 1) { A.rect.y0 = M.y0 + M.s0 * bh; A.rect.y1 = M.y0 + M.s1 * bh; }
        if (M.wr == 0 || M.s1 == M.s0) { A.rect.x0 = A.rect.x1 = A.rect.y0 = A.rect.y1 = 0; }       // (the cube is off the screen: every pixel is rad_kernel's)
        rect_limits = true;
    }
    // The pixels beside the rectangle of a MIP, isosurface or projection frame are not rad_kernel's (0,0,0,0): they hold the table's entry 0 or no RGBA
    // image at all, and there are the other images.  fill_outside_kernel writes them, and rad_kernel gets no rectangle (it then writes no pixel and computes
    // every slab's radius).
    F.fill_rect = A.rect;
    if (F.kind != FRAME_COMPOSITE) { A.rect.x0 = 0; A.rect.y0 = 0; A.rect.x1 = INT_MAX; A.rect.y1 = INT_MAX; }
}

// stage 5: balanced, heaviest-first tile order (StripMap::order, built by rad_kernel's extra block): analytic rays (the weights are the centre rays' chords),
// 8 ... 1024 units of at most 16 x-adjacent tiles.  VV_LPT=0 switches it off, VV_LPT_RUN sets the unit length.
// (units, their number and the table's size: vv_tiles.h)
static int tile_order(vv_context *c, Frame &F, const vv_ray_source *rays)
{
    MarchArgs &A = F.A;
    const int W = F.W, H = F.H;
    const bool beyond_caches = F.beyond_caches;
    A.strips.order = nullptr; A.order_out = nullptr;
    const int wr = A.strips.wr, ns = A.strips.s1 - A.strips.s0;
    A.strips.order_run = wr > 0 ? (wr + (wr + 15) / 16 - 1) / ((wr + 15) / 16) : 1;                  // the strip in ceil(wr / 16) equal runs
    if (c->knobs.lpt_run > 0 && c->knobs.lpt_run <= 256) A.strips.order_run = c->knobs.lpt_run;
    const int units = wr > 0 ? order_units(A.strips) : 0;
    // Measured (tools/ab_rep.sh, profiles/EXPERIMENTS.md part A5): aligned views of volumes up to 1 GiB gain 4 % (C2, 512^3, u8 1024^3); volumes beyond the
    // caches lose 1-6 % (the heaviest tiles marching together move more bytes), oblique views gain or lose up to 15 % with the camera: there the strips stay.
    const bool want = c->knobs.lpt > 0 ? true : (A.strips.tile_log2w == 5 && !beyond_caches && (long long)wr * ns >= 1024);      // (C1's 576 tiles: +2 %, the sort outlasts the rad pre-pass)
    if (c->knobs.lpt != 0 && want && !A.phong && rays->mode == VV_RAYS_ANALYTIC && W >= 2 && H >= 2 && units >= 8 && units <= 1024 && (long long)(wr + 1) * (ns + 1) <= 24576) {     // (rad_kernel: kMaxUnits, kMaxPoints)
        const int rc = ensure(c, SC_ORDER, std::max((size_t)order_words(A.strips), (size_t)65536) * sizeof(uint32_t));
        if (rc) return rc;
        A.strips.order = A.order_out = (uint32_t *)c->scratch[SC_ORDER].p;
    } else A.strips.order_run = 1;
    return VV_OK;
}

// stage 6: where the kernels write.  Pixels the frame does not write (column W-1, row H-1, rows of other shards) must keep the caller's bytes.  A whole
// frame is read back as the (W-1) x (H-1) rectangle it writes; a sharded / row-limited frame goes through a staged copy of the caller's buffer (rare path).
static int stage_images(vv_context *c, Frame &F, int out_on_device)
{
    const size_t npx = (size_t)F.W * F.H;
    for (FrameImage &im : F.img) {
        im.dev = (uint8_t *)im.host;
        if (out_on_device || !im.host) continue;
        int rc = ensure(c, im.scratch, npx * im.px_bytes);
        if (rc) return rc;
        im.dev = (uint8_t *)c->scratch[im.scratch].p;
        if (!F.whole) HIPCHK(c, hipMemcpyAsync(im.dev, im.host, npx * im.px_bytes, hipMemcpyHostToDevice, F.st));
    }
    for (const FrameImage &im : F.img)
        if (((uintptr_t)im.dev & (im.align - 1)) != 0) return fail(c, VV_ERR_INVALID, im.misaligned);
    return VV_OK;
}

// The radius pre-pass of an unshaded frame (composite, MIP, isosurface, projection): rad_kernel writes the radii into SC_RAD and, where the frame asked for
// one, the order table into SC_ORDER -- both a pure function of the launch's arguments.  The context keeps a byte image of the arguments of the last
// pre-pass (prepass_key: the whole argument block, not the fields the radii happen to depend on -- a spurious miss costs one short launch, a false hit
// a wrong frame).  A frame whose key is byte-identical launches nothing: the radii and the table stand in the buffers from the earlier launch on the
// same stream.  Never reused: image ray sources (the images' contents may change under the same pointers) and frames whose pre-pass also writes
// pixels (`rad_pixels`: the zeros beside the rectangle, when the march launch has no fill blocks for them).  The key is dropped when SC_RAD or
// SC_ORDER is allocated anew (ensure; the generation counts those, the address alone may come back), by every volume load, by vv_reread_env, by a
// failed call (fail(): every error return of render_frame passes through it) and with the context.  A frame issued while its stream is being
// captured into a graph neither reuses nor records: its pre-pass has not run when the call returns, and a replay runs at a time of the caller's
// choosing.  VV_RAD_REUSE=0: every frame launches.
static void issue_prepass(vv_context *c, Frame &F)
{
    MarchArgs &A = F.A;
    prepass_key key;
    memset(&key, 0, sizeof key);
    key.P = A.P; key.rect = A.rect; key.strips = A.strips; key.want_order = A.order_out != nullptr;
    key.rad = A.rad_out; key.order = A.order_out; key.gen = c->prepass_gen; key.stream = F.st; key.device = c->device;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    const bool live = hipStreamIsCapturing(F.st, &capture) == hipSuccess && capture == hipStreamCaptureStatusNone;
    if (!live) { (void)hipGetLastError(); c->prepass_valid = false; }       // (a captured pre-pass overwrites SC_RAD whenever the graph is replayed)
    const bool reusable = live && c->knobs.rad_reuse != 0 && A.P.ray_mode == VV_RAYS_ANALYTIC;
    if (reusable && !A.rad_pixels && c->prepass_valid && memcmp(&key, &c->prepass, sizeof key) == 0) {
        ++c->prepass_reused; c->last_reused = 1;
        return;
    }
    launch_rad(A, F.st);
    ++c->prepass_launched;
    memcpy(&c->prepass, &key, sizeof key); c->prepass_valid = reusable;
}

// stage 7: the kernels.  Unshaded frames: the rad pre-pass (unless its results stand from an earlier frame), the fill beside the rectangle (composite
// frames: fill blocks of the march launch, vv_fill.h, or rad_kernel with VV_TAIL_FILL=0 and where nothing marches), the march.
static void launch_kernels(vv_context *c, Frame &F)
{
    MarchArgs &A = F.A;
    hipStream_t st = F.st;
    c->last_reused = 0; c->last_fill_blocks = 0;
    A.rad_pixels = A.pixels; A.fill_blocks = 0;
    if (A.phong) {
        if (A.fill_outside) { A.rad_out = nullptr; launch_rad(A, st); }          // the pixels beside the volume's screen rectangle (rad_kernel writes them; no radii here)
        launch_build(F.kind, A, st);
    } else if (A.strips.n_strips > 0) {
        const bool rect_given = A.rect.x1 != INT_MAX || A.rect.y1 != INT_MAX;    // (else rad_kernel has no pixel to write: tiles_under_rect)
        if (!rect_given) A.rad_pixels = nullptr;
        else if (F.kind == FRAME_COMPOSITE && c->knobs.tail_fill != 0 && grid_blocks(A.strips) > 0 && (long long)F.W * F.H < (1ll << 31)) {
            const FrameParams &P = A.P;
            A.fill_blocks = fill_map(A.fill, F.W, F.H, A.rect.x0, A.rect.x1, A.rect.y0, A.rect.y1, P.rb, P.re, P.band, P.count, P.index);
            A.rad_pixels = nullptr;
            c->last_fill_blocks = A.fill_blocks;
        }
        if (F.W >= 2 && F.H >= 2) issue_prepass(c, F);
        if (F.kind != FRAME_COMPOSITE && F.rect_limits) launch_fill(A, F.fill_rect, st);
        launch_build(F.kind, A, st);
    }
}

// stage 8: host-buffer frames: the images back to the caller, and the wait; device-buffer frames wait only when the call is synchronous
static int read_back(vv_context *c, const Frame &F, int out_on_device, void *stream)
{
    const size_t W = (size_t)F.W, H = (size_t)F.H;
    if (!out_on_device) {
        for (const FrameImage &im : F.img) {
            if (!im.host) continue;
            const size_t pitch = W * im.px_bytes;
            if (F.whole) HIPCHK(c, hipMemcpy2DAsync(im.host, pitch, im.dev, pitch, (W - 1) * im.px_bytes, H - 1, hipMemcpyDeviceToHost, F.st));
            else HIPCHK(c, hipMemcpyAsync(im.host, im.dev, pitch * H, hipMemcpyDeviceToHost, F.st));
        }
        HIPCHK(c, hipStreamSynchronize(F.st));
    } else if (!stream) {
        HIPCHK(c, hipStreamSynchronize(F.st));
    }
    return VV_OK;
}

// One frame: vv_render (FRAME_COMPOSITE: rgba_out, shading), vv_render_mip (FRAME_MIP: rgba_out and / or index_out), vv_render_iso (FRAME_ISO: any of
// rgba_out, index_out, hit_out; `level`) and vv_render_projection (FRAME_PROJ: any of rgba_out, index_out, stat_out; `level` holds the vv_proj_mode); the
// last three never Phong.  All share the stages above; only the kernels (kLaunch's row) and the images differ.
static int render_frame(vv_context *c, int W, int H, const slice_params *slice, const camera_params *cam,
                        const shading_params *shading, const vv_ray_source *rays, const vv_render_options *opts,
                        uint8_t *rgba_out, uint8_t *index_out, float *hit_out, uint32_t *stat_out, FrameKind kind, int level, int out_on_device, void *stream)
{
    int rc = check_frame_args(c, W, H, slice, cam, rays);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Frame F;
    memset(&F, 0, sizeof F);
    F.kind = kind; F.W = W; F.H = H; F.st = pick_stream(c, stream);
    MarchArgs &A = F.A;
    const FrameParams &P = A.P;
    hipStream_t st = F.st;
    if ((rc = frame_params(c, F, slice, cam, rays, opts)) != VV_OK) return rc;
    if ((rc = view_knowledge(c, F, cam, rays, stream)) != VV_OK) return rc;
    F.beyond_caches = choose_launch(c, A, cam, rays, shading, F.have_basis, F.density, H, st);
    F.density = c->last_density;
    A.gray = c->tf_gray; A.phong = shading->phongShading;
    tiles_under_rect(c, F, rays);
    A.tf = c->d_tf; A.fill_tf = kind == FRAME_ISO ? nullptr : A.tf;
    if ((rc = ensure(c, SC_RAD, (size_t)P.nbx * P.nby * sizeof(float))) != VV_OK) return rc;
    if ((rc = tile_order(c, F, rays)) != VV_OK) return rc;
    A.rad = A.rad_out = (float *)c->scratch[SC_RAD].p;
    A.counter = c->d_counter;

    F.whole = P.count <= 1 && P.rb == 0 && P.re == P.nby && W >= 2 && H >= 2;
    const FrameImage images[4] = {
        {rgba_out,  4,  SC_FRAME, 4,  "vv_render: output buffer must be 4-byte aligned", nullptr},
        {index_out, 1,  SC_INDEX, 1,  "", nullptr},
        {hit_out,   16, SC_HIT,   16, "vv_render_iso: a device hit_out must be 16-byte aligned", nullptr},                  // (iso_kernel writes a record in one store)
        {stat_out,  8,  SC_STAT,  8,  "vv_render_projection: a device stat_out must be 8-byte aligned", nullptr},          // (proj_kernel likewise)
    };
    memcpy(F.img, images, sizeof images);
    if ((rc = stage_images(c, F, out_on_device)) != VV_OK) return rc;
    A.pixels = (uint32_t *)F.img[0].dev; A.index = F.img[1].dev; A.hit = (float4 *)F.img[2].dev; A.stat = (uint2 *)F.img[3].dev;
    A.proj_mode = kind == FRAME_PROJ ? level : 0;
    if (kind == FRAME_ISO) {
        A.iso.level = level;
        const int dims[3] = {c->nx, c->ny, c->nz};
        for (int a = 0; a < 3; ++a) { A.iso.n[a] = (float)dims[a]; A.iso.h[a] = 1.0f / (float)dims[a]; }
    }

    if (A.instr) HIPCHK(c, hipMemsetAsync(c->d_counter, 0, 16 * sizeof(unsigned long long), st));
#ifdef VV_TIMELINE
    { const char *e = getenv("VV_TIMELINE_PTR"); A.I.timeline = e ? (unsigned long long *)strtoull(e, nullptr, 0) : nullptr; }
#endif
    c->counter_valid = A.instr;
    {
        static const int layout_code[] = {0, 1, 2, 2, 3, 4, 5};        // MarchBuild -> the layout code of vv_debug_last_launch
        const int v[8] = {A.strips.tile_log2w, A.strips.blk_log2w, A.unroll, A.phong ? A.lds_reserve_phong : A.lds_reserve, layout_code[A.build],
                          F.have_basis ? 1 : 0, (int)fminf(F.density * 1000.f, 2e9f), kind != FRAME_COMPOSITE ? (int)kind : (A.phong ? 1 : 0)};
        memcpy(c->last_launch, v, sizeof v);
    }
    if (c->time_frames) HIPCHK(c, hipEventRecord(c->ev0, st));
    launch_kernels(c, F);
    if (c->time_frames) HIPCHK(c, hipEventRecord(c->ev1, st));
    if (A.instr) HIPCHK(c, hipEventRecord(c->ev_count, st));      // frame timing may be off, and the read-back's null-stream copy does not order behind a non-blocking stream
    HIPCHK(c, hipGetLastError());
    c->timed = c->time_frames;
    return read_back(c, F, out_on_device, stream);
}

// the shading of the frame kinds that have none (MIP, isosurface, projection)
static shading_params unshaded()
{
    shading_params s;
    memset(&s, 0, sizeof s);
    s.transferPreset = -1; s.phongShading = false;
    return s;
}

extern "C" {

int vv_render(vv_context *c, int W, int H, const slice_params *slice, const camera_params *cam,
              const shading_params *shading, const vv_ray_source *rays, const vv_render_options *opts,
              uint8_t *rgba_out, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_render: NULL context");
    if (!slice || !cam || !shading || !rays || !rgba_out) return fail(c, VV_ERR_INVALID, "vv_render: NULL argument");
    return render_frame(c, W, H, slice, cam, shading, rays, opts, rgba_out, nullptr, nullptr, nullptr, FRAME_COMPOSITE, 0, out_on_device, stream);
}

// ---- maximum-intensity projection (no reference counterpart) ---------------------------------
int vv_render_mip(vv_context *c, int W, int H, const slice_params *slice, const camera_params *cam,
                  const vv_ray_source *rays, const vv_render_options *opts,
                  uint8_t *rgba_out, uint8_t *index_out, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_render_mip: NULL context");
    if (!slice || !cam || !rays) return fail(c, VV_ERR_INVALID, "vv_render_mip: NULL argument");
    if (!rgba_out && !index_out) return fail(c, VV_ERR_INVALID, "vv_render_mip: rgba_out and index_out are both NULL");
    const shading_params none = unshaded();
    return render_frame(c, W, H, slice, cam, &none, rays, opts, rgba_out, index_out, nullptr, nullptr, FRAME_MIP, 0, out_on_device, stream);
}

// ---- isosurface frames: the first sample at or above a level (no reference counterpart) --------
int vv_render_iso(vv_context *c, int W, int H, const slice_params *slice, const camera_params *cam,
                  const vv_ray_source *rays, const vv_render_options *opts, int level,
                  uint8_t *rgba_out, uint8_t *index_out, float *hit_out, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_render_iso: NULL context");
    if (!slice || !cam || !rays) return fail(c, VV_ERR_INVALID, "vv_render_iso: NULL argument");
    if (!rgba_out && !index_out && !hit_out) return fail(c, VV_ERR_INVALID, "vv_render_iso: rgba_out, index_out and hit_out are all NULL");
    if (level < 1 || level > 255) return fail(c, VV_ERR_INVALID, "vv_render_iso: level must lie in 1..255");
    const shading_params none = unshaded();
    return render_frame(c, W, H, slice, cam, &none, rays, opts, rgba_out, index_out, hit_out, nullptr, FRAME_ISO, level, out_on_device, stream);
}

// ---- projection frames: maximum / minimum / mean over the samples inside the volume (no reference counterpart) --------
int vv_render_projection(vv_context *c, int W, int H, const slice_params *slice, const camera_params *cam,
                         const vv_ray_source *rays, const vv_render_options *opts, int mode,
                         uint8_t *rgba_out, uint8_t *index_out, uint32_t *stat_out, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_render_projection: NULL context");
    if (!slice || !cam || !rays) return fail(c, VV_ERR_INVALID, "vv_render_projection: NULL argument");
    if (mode != VV_PROJ_MAX && mode != VV_PROJ_MIN && mode != VV_PROJ_MEAN) return fail(c, VV_ERR_INVALID, "vv_render_projection: mode must be VV_PROJ_MAX, VV_PROJ_MIN or VV_PROJ_MEAN");
    if (!rgba_out && !index_out && !stat_out) return fail(c, VV_ERR_INVALID, "vv_render_projection: rgba_out, index_out and stat_out are all NULL");
    if (out_on_device && ((uintptr_t)stat_out & 7) != 0) return fail(c, VV_ERR_INVALID, "vv_render_projection: a device stat_out must be 8-byte aligned");
    const shading_params none = unshaded();
    return render_frame(c, W, H, slice, cam, &none, rays, opts, rgba_out, index_out, nullptr, stat_out, FRAME_PROJ, mode, out_on_device, stream);
}

int vv_classify_indices(vv_context *c, const uint8_t *index, size_t n, const float tf[1024], uint8_t *rgba_out, int on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_classify_indices: NULL context");
    if (!index || !rgba_out) return fail(c, VV_ERR_INVALID, "vv_classify_indices: NULL argument");
    if (!tf && !c->have_tf) return fail(c, VV_ERR_NO_VOLUME, "vv_classify_indices: no transfer function loaded");
    if (tf) for (int i = 0; i < 1024; ++i) if (!std::isfinite(tf[i])) return fail(c, VV_ERR_INVALID, "vv_classify_indices: transfer function must be finite");
    hipStream_t st;
    CallBuf b[3] = {
        {(void *)tf,    tf ? 1024 * sizeof(float) : 0, true, true, false, SC_TF_ARG, nullptr, nullptr},     // (the caller's table is on the host whatever on_device says)
        {(void *)index, n,     !on_device, true,  false, SC_INDEX, nullptr, nullptr},
        {rgba_out,      n * 4, !on_device, false, true,  SC_FRAME, nullptr, nullptr},
    };
    int rc = stage_call(c, stream, &st, b, 3);
    if (rc) return rc;
    if (((uintptr_t)b[2].dev & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_classify_indices: output buffer must be 4-byte aligned");
    launch_mip_classify((const uint8_t *)b[1].dev, n, tf ? (const float4 *)b[0].dev : c->d_tf, (uint32_t *)b[2].dev, st);
    return finish_call(c, stream, st, b, 3);
}

// ---- first pass images ------------------------------------------------------------------
int vv_first_pass(vv_context *c, int W, int H, const camera_params *cam, const vv_ray_source *rays,
                  uint8_t *front, uint8_t *back, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_first_pass: NULL context");
    if (!cam || !rays || !front || !back || W < 1 || H < 1) return fail(c, VV_ERR_INVALID, "vv_first_pass: bad argument");
    if (rays->mode != VV_RAYS_ANALYTIC) return fail(c, VV_ERR_INVALID, "vv_first_pass: needs an analytic ray source");
    for (int a = 0; a < 3; ++a)
        if (!(cam->scale[a] > 0.f) || !std::isfinite(cam->scale[a])) return fail(c, VV_ERR_INVALID, "vv_first_pass: camera scale must be finite and > 0");
    FrameParams P;
    memset(&P, 0, sizeof P);
    P.W = W; P.H = H;
    for (int a = 0; a < 3; ++a) { P.cam_pos[a] = cam->origin[a]; P.scale[a] = cam->scale[a]; }
    int rc = camera_basis(c, P, cam, rays, W, H);
    if (rc) return rc;
    const size_t ib = (size_t)W * H * 4;
    hipStream_t st;
    CallBuf b[2] = {{front, ib, !out_on_device, false, true, SC_IMG, nullptr, nullptr}, {back, ib, !out_on_device, false, true, SC_IMG, nullptr, nullptr}};
    if ((rc = stage_call(c, stream, &st, b, 2)) != VV_OK) return rc;
    if (((uintptr_t)b[0].dev & 3) || ((uintptr_t)b[1].dev & 3)) return fail(c, VV_ERR_INVALID, "vv_first_pass: images must be 4-byte aligned");
    launch_first_pass(P, (uint32_t *)b[0].dev, (uint32_t *)b[1].dev, st);
    return finish_call(c, stream, st, b, 2);
}

int vv_debug_screen_rect(int W, int H, const camera_params *cam, const vv_ray_source *rays, double out[4])
{
    if (!cam || !rays || !out || W < 1 || H < 1) return fail(nullptr, VV_ERR_INVALID, "vv_debug_screen_rect: bad argument");
    if (rays->mode != VV_RAYS_ANALYTIC) return 0;
    MarchArgs A;
    memset(&A, 0, sizeof A);
    for (int a = 0; a < 3; ++a) { A.P.cam_pos[a] = cam->origin[a]; A.P.scale[a] = cam->scale[a]; }
    int rc = camera_basis(nullptr, A.P, cam, rays, W, H);
    if (rc) return rc;
    return screen_rect(A, W, H, &out[0], &out[1], &out[2], &out[3]) ? 1 : 0;
}

// the radius pre-pass (issue_prepass; developer aid, tests): {pre-passes launched since the context was created, frames that reused the last one's
// results, whether the last frame did, the fill blocks of the last frame's march launch}
int vv_debug_prepass_state(vv_context *c, int out[4])
{
    if (!c || !out) return VV_ERR_INVALID;
    out[0] = c->prepass_launched; out[1] = c->prepass_reused; out[2] = c->last_reused; out[3] = c->last_fill_blocks;
    return VV_OK;
}

// what vv_render chose for its last frame (developer aid, tests): {wave tile log2 width, block log2 width, samples per trip, LDS reserve, layout (0 linear,
// 1 linear with 64-bit addressing, 2 bricked, 3 z-pair, 4 z-fastest, 5 x-pair), 1 if the view was known to the policy, density x 1000, Phong}
int vv_debug_last_launch(vv_context *c, int out[8])
{
    if (!c || !out) return VV_ERR_INVALID;
    memcpy(out, c->last_launch, sizeof c->last_launch);
    return VV_OK;
}

// A resident layout as it lies in HBM (developer aid, tests/test_footprint.py): geom = {allocation bytes (the zeroed bytes behind the copy included;
// 0: not resident, nothing is copied), the layout's two VolumeView strides -- row_bytes / slice_bytes, b_sy / b_sz64 (64-byte units), zp_row_bytes /
// zp_slab_bytes, zf_row_bytes / zf_slice_bytes --, nx, ny, nz, voxel type, 0}; then the allocation is copied to host_dst on the context's stream and
// waited for (host_dst NULL with capacity 0: the geometry alone).  `layout`: the codes of vv_debug_last_launch (0 and 1 are the same allocation).  Builds nothing, changes no state.
int vv_debug_read_layout(vv_context *c, int layout, unsigned long long geom[8], void *host_dst, size_t capacity)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_debug_read_layout: NULL context");
    if (!geom) return fail(c, VV_ERR_INVALID, "vv_debug_read_layout: NULL geom");
    if (layout < 0 || layout > 5) return fail(c, VV_ERR_INVALID, "vv_debug_read_layout: unknown layout");
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_debug_read_layout: no volume loaded");
    static const int copy_of[] = {-1, -1, CP_BRICKS, CP_ZPAIR, CP_ZFAST, CP_XPAIR};
    const void *src = c->d_vol;
    unsigned long long g[8] = {c->alloc_bytes, c->row_pitch, c->slice_pitch, (unsigned long long)c->nx, (unsigned long long)c->ny, (unsigned long long)c->nz,
                               (unsigned long long)c->vtype, 0};
    if (copy_of[layout] >= 0) {
        const layout_copy &cp = c->copies[copy_of[layout]];
        src = cp.ptr; g[0] = cp.valid ? cp.alloc : 0; g[1] = cp.valid ? cp.row : 0; g[2] = cp.valid ? cp.slab : 0;
    }
    memcpy(geom, g, sizeof g);
    if (g[0] == 0 || (!host_dst && capacity == 0)) return VV_OK;           // (NULL, 0: the geometry alone)
    if (!host_dst || capacity < g[0]) return fail(c, VV_ERR_INVALID, "vv_debug_read_layout: host_dst is NULL or smaller than the allocation (geom[0])");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_dst, src, g[0], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VV_OK;
}

int vv_set_frame_timing(vv_context *c, int on)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_set_frame_timing: NULL context");
    c->time_frames = on != 0;
    if (!on) c->timed = false;
    return VV_OK;
}

float vv_last_frame_ms(const vv_context *c)
{
    if (!c || !c->timed) return -1.f;
    float ms = -1.f;
    if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.f;
    return ms;
}

unsigned long long vv_last_sample_count(vv_context *c)
{
    if (!c || !c->counter_valid) return 0;
    unsigned long long v = 0;
    hipSetDevice(c->device);
    if (hipEventSynchronize(c->ev_count) != hipSuccess) return 0;
    if (hipMemcpy(&v, c->d_counter, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return v;
}

// ---- slice view: invoke_slice_kernel / invoke_advanced_slice_kernel, kernel.cu:506-541 ----
extern "C++" {
// SliceArgs and SlabArgs name the image, the position and the filter alike: the fields of either that the four entry points share.  `trans`: the matrix of the
// free-form views, or null for a canonical view at (dx, dy, dz) in `orientation`.
template <class Args>
static Args slice_args(size_t height, size_t width, float dx, float dy, float dz, int orientation, const float *trans, const float scale[3], int filter)
{
    Args S; memset(&S, 0, sizeof S);
    S.height = height; S.width = width; S.dx = dx; S.dy = dy; S.dz = dz;
    S.orientation = orientation; S.advanced = trans != nullptr;
    S.tex8 = filter != VV_FILTER_EXACT;
    for (int a = 0; a < 3; ++a) S.scale[a] = scale[a];
    if (trans) memcpy(S.trans, trans, 16 * sizeof(float));
    return S;
}
static bool slice_size_ok(size_t height, size_t width) { return height >= 1 && width >= 1 && height <= 65535u * 16 && width <= 65535u * 16; }

// Runs slice_kernel or slab_kernel (`launch`: gets the device images and the stream) on the loaded volume: one image, or image + aux.  Host images go
// through the slice scratch (instead of the reference's cudaMalloc / cudaFree per call, kernel.cu:508-518), one after the other, and are uploaded
// first: elements the kernel skips keep the caller's bytes.
template <class Args, class Launch>
static int run_planar(vv_context *c, Args &S, float *buffer, int32_t *aux, int out_on_device, void *stream, Launch launch)
{
    const size_t bytes = S.height * S.width * sizeof(float);        // of either image
    S.V = view_of(c, MB_LINEAR); S.V_type = c->vtype;
    hipStream_t st;
    CallBuf b[2] = {{buffer, bytes, !out_on_device, true, true, SC_SLICE, nullptr, nullptr}, {aux, aux ? bytes : 0, !out_on_device, true, true, SC_SLICE, nullptr, nullptr}};
    int rc = stage_call(c, stream, &st, b, 2);
    if (rc) return rc;
    launch((float *)b[0].dev, (int32_t *)b[1].dev, st);
    return finish_call(c, stream, st, b, 2);
}
} // extern "C++"

static int run_slice(vv_context *c, SliceArgs &S, float *buffer, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_slice: NULL context");
    if (!buffer) return fail(c, VV_ERR_INVALID, "vv_slice: NULL buffer");
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_slice: no volume loaded");
    if (!slice_size_ok(S.height, S.width)) return fail(c, VV_ERR_INVALID, "vv_slice: bad buffer size");
    return run_planar(c, S, buffer, nullptr, out_on_device, stream, [&S](float *d, int32_t *, hipStream_t st) { S.buffer = d; launch_slice(S, st); });
}

int vv_slice(vv_context *c, float *buffer, size_t height, size_t width, float dx, float dy, float dz,
             int orientation, const float scale[3], int legacy, int filter, int out_on_device, void *stream)
{
    if (!scale) return fail(c, VV_ERR_INVALID, "vv_slice: NULL scale");
    SliceArgs S = slice_args<SliceArgs>(height, width, dx, dy, dz, orientation, nullptr, scale, filter);
    S.legacy = legacy;
    return run_slice(c, S, buffer, out_on_device, stream);
}

int vv_slice_advanced(vv_context *c, float *buffer, size_t height, size_t width, const float trans[16],
                      const float scale[3], int filter, int out_on_device, void *stream)
{
    if (!scale || !trans) return fail(c, VV_ERR_INVALID, "vv_slice_advanced: NULL argument");
    SliceArgs S = slice_args<SliceArgs>(height, width, 0.f, 0.f, 0.f, 0, trans, scale, filter);
    return run_slice(c, S, buffer, out_on_device, stream);
}

// ---- thick-slab slices (include/volviz.h: vv_slice_slab) ------------------------------------
static int run_slab(vv_context *c, SlabArgs &S, float *buffer, int32_t *aux, const vv_slab *slab, int out_on_device, void *stream)
{
    if (!buffer) return fail(c, VV_ERR_INVALID, "vv_slice_slab: NULL buffer");
    if (slab->mode != VV_SLAB_MAX && slab->mode != VV_SLAB_MIN && slab->mode != VV_SLAB_MEAN)
        return fail(c, VV_ERR_INVALID, "vv_slice_slab: mode must be VV_SLAB_MAX, VV_SLAB_MIN or VV_SLAB_MEAN");
    if (slab->samples < 1 || slab->samples > VV_SLAB_MAX_SAMPLES) return fail(c, VV_ERR_INVALID, "vv_slice_slab: samples must lie in 1..1024");
    if (!(slab->thickness >= 0.f) || !std::isfinite(slab->thickness)) return fail(c, VV_ERR_INVALID, "vv_slice_slab: thickness must be finite and >= 0");
    if (!slice_size_ok(S.height, S.width)) return fail(c, VV_ERR_INVALID, "vv_slice_slab: bad buffer size");
    if (out_on_device && ((uintptr_t)aux & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_slice_slab: a device aux must be 4-byte aligned");
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_slice_slab: no volume loaded");
    S.mode = slab->mode; S.samples = slab->samples; S.thickness = slab->thickness;
    return run_planar(c, S, buffer, aux, out_on_device, stream, [&S](float *d, int32_t *da, hipStream_t st) { S.buffer = d; S.aux = da; launch_slab(S, st); });
}

int vv_slice_slab(vv_context *c, float *buffer, int32_t *aux, size_t height, size_t width, float dx, float dy, float dz,
                  int orientation, const float scale[3], int filter, const vv_slab *slab, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_slice_slab: NULL context");
    if (!scale || !slab) return fail(c, VV_ERR_INVALID, "vv_slice_slab: NULL argument");
    if (orientation != VV_SAGITTAL && orientation != VV_HORIZONTAL && orientation != VV_CORONAL)
        return fail(c, VV_ERR_INVALID, "vv_slice_slab: orientation must be VV_SAGITTAL, VV_HORIZONTAL or VV_CORONAL");
    SlabArgs S = slice_args<SlabArgs>(height, width, dx, dy, dz, orientation, nullptr, scale, filter);
    return run_slab(c, S, buffer, aux, slab, out_on_device, stream);
}

int vv_slice_advanced_slab(vv_context *c, float *buffer, int32_t *aux, size_t height, size_t width, const float trans[16],
                           const float scale[3], int filter, const vv_slab *slab, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_slice_advanced_slab: NULL context");
    if (!scale || !trans || !slab) return fail(c, VV_ERR_INVALID, "vv_slice_advanced_slab: NULL argument");
    SlabArgs S = slice_args<SlabArgs>(height, width, 0.f, 0.f, 0.f, VV_SAGITTAL, trans, scale, filter);
    return run_slab(c, S, buffer, aux, slab, out_on_device, stream);
}

// ---- histograms (include/volviz.h: vv_volume_histogram) ------------------------------------
// accumulator zeroed, counted (unless there is nothing to count), turned into `out` / `counts`: all on `st` (finish_call checks the launches)
static int run_hist(vv_context *c, const HistRuns *runs, int vtype, unsigned long long voxels, vv_histogram *d_out, unsigned long long *d_counts, hipStream_t st)
{
    HIPCHK(c, hipMemsetAsync(c->d_hist, 0, kHistAccWords * sizeof(unsigned long long), st));
    if (runs) launch_hist(*runs, c->n_cu, c->knobs.hist_blocks, c->d_hist, st);
    launch_hist_finish(c->d_hist, vtype, voxels, d_out, d_counts, st);
    return VV_OK;
}

int vv_volume_histogram(vv_context *c, const int box_lo[3], const int box_hi[3], vv_histogram *out, int out_on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_volume_histogram: NULL context");
    if (!out) return fail(c, VV_ERR_INVALID, "vv_volume_histogram: NULL out");
    if ((box_lo == nullptr) != (box_hi == nullptr)) return fail(c, VV_ERR_INVALID, "vv_volume_histogram: box_lo and box_hi must both be given or both be NULL");
    if (out_on_device && ((uintptr_t)out & 7) != 0) return fail(c, VV_ERR_INVALID, "vv_volume_histogram: a device out must be 8-byte aligned");
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_volume_histogram: no volume loaded");
    const int dims[3] = {c->nx, c->ny, c->nz};
    int lo[3] = {0, 0, 0}, hi[3] = {c->nx, c->ny, c->nz};
    if (box_lo) {
        for (int a = 0; a < 3; ++a) { lo[a] = box_lo[a]; hi[a] = box_hi[a]; }
        if (!box_in_range(lo, hi, dims)) return fail(c, VV_ERR_INVALID, "vv_volume_histogram: the box must satisfy 0 <= lo < hi <= dims on every axis");
    }
    hipStream_t st;
    CallBuf b = {out, sizeof(vv_histogram), !out_on_device, false, true, 0, (char *)c->d_hist + kHistResultOffset, nullptr};
    int rc = stage_call(c, stream, &st, &b, 1);
    if (rc) return rc;
    // the box as runs of the linear layout: its rows; whole slices of it where the rows are dense and taken whole; the whole box where the slices are too
    const size_t size = voxel_bytes(c->vtype);
    const size_t bx = (size_t)(hi[0] - lo[0]), by = (size_t)(hi[1] - lo[1]), bz = (size_t)(hi[2] - lo[2]);
    const bool rows_dense = bx == (size_t)c->nx && c->row_pitch == (size_t)c->nx * size;
    const bool slices_dense = rows_dense && by == (size_t)c->ny && c->slice_pitch == (size_t)c->ny * c->row_pitch;
    HistRuns R;
    memset(&R, 0, sizeof R);
    R.vtype = c->vtype; R.tight = 0;
    R.data0 = (const char *)c->d_vol + voxel_offset(c, lo[0], lo[1], lo[2]);
    R.row_step = c->row_pitch; R.slice_step = c->slice_pitch;
    if (slices_dense)    { R.run_voxels = bx * by * bz; R.rps = 1; R.n_slices = 1; }
    else if (rows_dense) { R.run_voxels = bx * by; R.rps = 1; R.n_slices = (uint32_t)bz; }
    else                 { R.run_voxels = bx; R.rps = (uint32_t)by; R.n_slices = (uint32_t)bz; }
    // what launch_hist is promised: the last voxel of the box lies inside the volume, which ends more than 16 bytes before its allocation does
    if (((uintptr_t)c->d_vol & 15) != 0 || box_end(c, hi) + 16 > c->alloc_bytes) return fail(c, VV_ERR_DEVICE, "vv_volume_histogram: volume allocation is not what the kernel expects");
    if ((rc = run_hist(c, &R, c->vtype, (unsigned long long)(bx * by * bz), (vv_histogram *)b.dev, nullptr, st)) != VV_OK) return rc;
    return finish_call(c, stream, st, &b, 1);
}

int vv_histogram_indices(vv_context *c, const uint8_t *index, size_t n, unsigned long long counts[256], int on_device, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_histogram_indices: NULL context");
    if (!counts || (!index && n)) return fail(c, VV_ERR_INVALID, "vv_histogram_indices: NULL argument");
    if (on_device && ((uintptr_t)counts & 7) != 0) return fail(c, VV_ERR_INVALID, "vv_histogram_indices: device counts must be 8-byte aligned");
    hipStream_t st;
    CallBuf b[2] = {
        {(void *)index, n, !on_device, true, false, SC_INDEX, nullptr, nullptr},
        {counts, 256 * sizeof(unsigned long long), !on_device, false, true, 0, (char *)c->d_hist + kHistResultOffset, nullptr},
    };
    int rc = stage_call(c, stream, &st, b, 2);
    if (rc) return rc;
    HistRuns R;
    memset(&R, 0, sizeof R);
    R.data0 = b[0].dev; R.vtype = VV_VOXEL_U8; R.tight = 1;          // one run of n bytes in a buffer whose surroundings are not ours to read
    R.run_voxels = n; R.rps = 1; R.n_slices = 1;
    if ((rc = run_hist(c, n ? &R : nullptr, VV_VOXEL_U8, n, nullptr, (unsigned long long *)b[1].dev, st)) != VV_OK) return rc;
    return finish_call(c, stream, st, b, 2);
}

// ---- derived volumes (include/volviz.h: vv_derive_volume) ----------------------------------
// The checks vv_derive_dims and vv_derive_volume share, in the order of the header's rule 7 (behind the NULL checks): the box (lo, hi), the
// factors (f, 0 read as 1) and the output's extents (m).
static int derive_check(const vv_context *c, vv_context *err_to, const char *who, const vv_derive *d, int lo[3], int hi[3], int f[3], int m[3])
{
    const std::string w(who);
    if (!c->d_vol) return fail(err_to, VV_ERR_NO_VOLUME, w + ": no volume loaded");
    const int dims[3] = {c->nx, c->ny, c->nz};
    int rc = check_box(err_to, who, d->box_lo, d->box_hi, dims, lo, hi);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) {
        if (d->factor[a] < 0 || d->factor[a] > 8) return fail(err_to, VV_ERR_INVALID, w + ": factors must lie in 1..8 (0 is read as 1)");
        f[a] = d->factor[a] ? d->factor[a] : 1;
        m[a] = (hi[a] - lo[a] + f[a] - 1) / f[a];
    }
    if (d->mode != VV_REDUCE_MEAN && d->mode != VV_REDUCE_MAX && d->mode != VV_REDUCE_MIN)
        return fail(err_to, VV_ERR_INVALID, w + ": mode must be VV_REDUCE_MEAN, VV_REDUCE_MAX or VV_REDUCE_MIN");
    if ((rc = check_out_type(err_to, who, d->out_type)) != VV_OK) return rc;
    if (d->window != 0 && d->window != 1) return fail(err_to, VV_ERR_INVALID, w + ": window must be 0 or 1");
    if (d->window) {
        const volatile float span = d->win_hi - d->win_lo;            // binary32, as the kernel takes it
        if (!std::isfinite(d->win_lo) || !std::isfinite(d->win_hi) || !std::isfinite((float)span) || !(span > 0.f))
            return fail(err_to, VV_ERR_INVALID, w + ": win_lo and win_hi must be finite with a finite win_hi - win_lo > 0");
    }
    return VV_OK;
}

int vv_derive_dims(const vv_context *c, const vv_derive *d, int out_dims[3])
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_derive_dims: NULL context");
    vv_context *e = const_cast<vv_context *>(c);                    // (the message alone)
    if (!d || !out_dims) return fail(e, VV_ERR_INVALID, "vv_derive_dims: NULL argument");
    int lo[3], hi[3], f[3], m[3];
    const int rc = derive_check(c, e, "vv_derive_dims", d, lo, hi, f, m);
    if (rc) return rc;
    for (int a = 0; a < 3; ++a) out_dims[a] = m[a];
    return VV_OK;
}

int vv_derive_volume(vv_context *c, const vv_derive *d, void *out, size_t capacity, int out_on_device, void *stream)
{
    static const char who[] = "vv_derive_volume";
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_derive_volume: NULL context");
    if (!d || !out) return fail(c, VV_ERR_INVALID, "vv_derive_volume: NULL argument");
    int lo[3], hi[3], f[3], m[3];
    size_t bytes;
    int rc = derive_check(c, c, who, d, lo, hi, f, m);
    if (!rc) rc = check_out_volume(c, who, " (vv_derive_dims)", out, capacity, out_on_device, d->out_type, m, false, &bytes);
    if (rc) return rc;
    DeriveArgs A;
    memset(&A, 0, sizeof A);
    A.src0 = (const char *)c->d_vol + voxel_offset(c, lo[0], lo[1], lo[2]);
    A.row_pitch = c->row_pitch; A.slice_pitch = c->slice_pitch;
    for (int a = 0; a < 3; ++a) { A.b[a] = (uint32_t)(hi[a] - lo[a]); A.f[a] = (uint32_t)f[a]; A.m[a] = (uint32_t)m[a]; }
    A.src_type = c->vtype; A.out_type = d->out_type; A.mode = d->mode; A.window = d->window;
    A.win_lo = d->win_lo; A.win_hi = d->win_hi;
    // what launch_derive is promised: the allocation starts 16-byte aligned and holds the box's last voxel; what lies behind that voxel is its to read
    const size_t last = box_end(c, hi);
    if (((uintptr_t)c->d_vol & 15) != 0 || last > c->alloc_bytes) return fail(c, VV_ERR_DEVICE, "vv_derive_volume: volume allocation is not what the kernel expects");
    A.slack = c->alloc_bytes - last;
    return run_out_volume(c, who, out, bytes, out_on_device, false, stream, [&](void *dev, hipStream_t st) {
        A.out = dev;
        launch_derive(A, c->n_cu, c->knobs.derive_blocks, st);
        return VV_OK;
    });
}

// ---- neighbourhood filters (include/volviz.h: vv_stencil_volume) ---------------------------
int vv_stencil_volume(vv_context *c, const vv_stencil *d, void *out, size_t capacity, int out_on_device, void *stream)
{
    static const char who[] = "vv_stencil_volume";
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_stencil_volume: NULL context");
    if (!d || !out) return fail(c, VV_ERR_INVALID, "vv_stencil_volume: NULL argument");
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_stencil_volume: no volume loaded");
    // the header's rule 9, in its order
    const int dims[3] = {c->nx, c->ny, c->nz};
    int lo[3], hi[3];
    int rc = check_box(c, who, d->box_lo, d->box_hi, dims, lo, hi);
    if (rc) return rc;
    if (d->kind != VV_STENCIL_SEPARABLE && d->kind != VV_STENCIL_MEDIAN && d->kind != VV_STENCIL_GRADMAG)
        return fail(c, VV_ERR_INVALID, "vv_stencil_volume: kind must be VV_STENCIL_SEPARABLE, VV_STENCIL_MEDIAN or VV_STENCIL_GRADMAG");
    if ((rc = check_out_type(c, who, d->out_type)) != VV_OK) return rc;
    StencilArgs A;
    memset(&A, 0, sizeof A);
    if (d->kind == VV_STENCIL_SEPARABLE)
        for (int a = 0; a < 3; ++a) {
            if (d->radius[a] < 0 || d->radius[a] > VV_STENCIL_MAX_RADIUS) return fail(c, VV_ERR_INVALID, "vv_stencil_volume: radii must lie in 0..4");
            A.radius[a] = d->radius[a];
            for (int k = 0; k <= d->radius[a]; ++k) {
                if (!std::isfinite(d->taps[a][k])) return fail(c, VV_ERR_INVALID, "vv_stencil_volume: the taps up to the radius must be finite");
                A.taps[a][k] = d->taps[a][k];
            }
        }
    if (d->kind == VV_STENCIL_GRADMAG) {
        const bool unset = d->gscale[0] == 0.f && d->gscale[1] == 0.f && d->gscale[2] == 0.f;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(d->gscale[a])) return fail(c, VV_ERR_INVALID, "vv_stencil_volume: gscale must be finite");
            A.gscale[a] = unset ? 1.f : d->gscale[a];
        }
    }
    const int b[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    size_t bytes;
    if ((rc = check_out_volume(c, who, "", out, capacity, out_on_device, d->out_type, b, true, &bytes)) != VV_OK) return rc;
    A.vol = c->d_vol;
    A.row_pitch = c->row_pitch; A.slice_pitch = c->slice_pitch;
    for (int a = 0; a < 3; ++a) { A.n[a] = dims[a]; A.lo[a] = lo[a]; A.b[a] = (uint32_t)b[a]; }
    A.src_type = c->vtype; A.out_type = d->out_type; A.kind = d->kind;
    // what launch_stencil is promised: the volume's last voxel lies inside the allocation
    if (box_end(c, dims) > c->alloc_bytes || (c->vtype == VV_VOXEL_F32 && (((uintptr_t)c->d_vol | c->row_pitch | c->slice_pitch) & 3) != 0))
        return fail(c, VV_ERR_DEVICE, "vv_stencil_volume: volume allocation is not what the kernel expects");
    return run_out_volume(c, who, out, bytes, out_on_device, false, stream, [&](void *dev, hipStream_t st) {
        A.out = dev;
        launch_stencil(A, c->n_cu, c->knobs.stencil_blocks, st);
        return VV_OK;
    });
}

// ---- resampled volumes (include/volviz.h: vv_resample_volume) -------------------------------
// The header's rule 9 behind the NULL checks, in its order; fills the box (lo, hi) and the output's bytes.
static int resample_check(vv_context *c, const char *who, const vv_resample *r, const void *out, size_t capacity, int out_on_device, int lo[3], int hi[3], size_t *bytes)
{
    if (!c->d_vol) return fail(c, VV_ERR_NO_VOLUME, "vv_resample_volume: no volume loaded");
    for (int a = 0; a < 3; ++a)
        if (r->dims[a] < 1 || r->dims[a] > VV_RESAMPLE_MAX_DIM) return fail(c, VV_ERR_INVALID, "vv_resample_volume: dims must lie in 1..16384");
    int rc = check_box(c, who, r->box_lo, r->box_hi, r->dims, lo, hi);
    if (rc) return rc;
    if (r->filter != VV_RESAMPLE_TEX8 && r->filter != VV_RESAMPLE_EXACT && r->filter != VV_RESAMPLE_NEAREST)
        return fail(c, VV_ERR_INVALID, "vv_resample_volume: filter must be VV_RESAMPLE_TEX8, VV_RESAMPLE_EXACT or VV_RESAMPLE_NEAREST");
    if ((rc = check_out_type(c, who, r->out_type)) != VV_OK) return rc;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(r->m[k])) return fail(c, VV_ERR_INVALID, "vv_resample_volume: the matrix must be finite");
    if (!std::isfinite(r->fill)) return fail(c, VV_ERR_INVALID, "vv_resample_volume: fill must be finite");
    const int b[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    return check_out_volume(c, who, "", out, capacity, out_on_device, r->out_type, b, true, bytes);
}

int vv_resample_volume(vv_context *c, const vv_resample *r, void *out, size_t capacity, int out_on_device, void *stream)
{
    static const char who[] = "vv_resample_volume";
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_resample_volume: NULL context");
    if (!r || !out) return fail(c, VV_ERR_INVALID, "vv_resample_volume: NULL argument");
    int lo[3], hi[3];
    size_t bytes = 0;
    const int rc = resample_check(c, who, r, out, capacity, out_on_device, lo, hi, &bytes);
    if (rc) return rc;
    ResampleArgs A;
    memset(&A, 0, sizeof A);
    A.V = view_of(c, MB_LINEAR);
    A.src_type = c->vtype; A.out_type = r->out_type; A.filter = r->filter;
    for (int a = 0; a < 3; ++a) {
        A.lo[a] = lo[a]; A.b[a] = (uint32_t)(hi[a] - lo[a]);
        const volatile float inv = 1.0f / (float)r->dims[a];        // one IEEE binary32 division
        A.inv[a] = inv;
    }
    memcpy(A.m, r->m, sizeof A.m); A.fill = r->fill;
    // what launch_resample is promised: the weight-0 corners of the last voxel's sample (one slice and one row on, two dwords) lie inside the allocation
    const size_t reach = voxel_offset(c, c->nx, 0, c->nz + 1) + 8;
    if (reach > c->alloc_bytes || (c->vtype == VV_VOXEL_F32 && (((uintptr_t)c->d_vol | c->row_pitch | c->slice_pitch) & 3) != 0))
        return fail(c, VV_ERR_DEVICE, "vv_resample_volume: volume allocation is not what the kernel expects");
    return run_out_volume(c, who, out, bytes, out_on_device, false, stream, [&](void *dev, hipStream_t st) {
        A.out = dev;
        launch_resample(A, c->n_cu, c->knobs.resample_blocks, st);
        return VV_OK;
    });
}

// ---- segmentation (include/volviz.h: vv_label_volume, vv_mask_volume) ------------------------
int vv_label_volume(vv_context *c, const vv_label *d, uint32_t *labels, size_t capacity, uint32_t *sizes, vv_label_stats *stats, int out_on_device, void *stream)
{
    static const char who[] = "vv_label_volume";
    LabelArgs A;
    CallBox B;
    int rc = open_box_call(c, c, who, d, labels != nullptr, A, B);
    if (rc) return rc;
    // the header's rule 9, in its order
    if ((rc = check_bins(c, who, d->bin_lo, d->bin_hi)) != VV_OK) return rc;
    if (d->connectivity != 6 && d->connectivity != 18 && d->connectivity != 26) return fail(c, VV_ERR_INVALID, "vv_label_volume: connectivity must be 6, 18 or 26");
    const size_t bytes = (size_t)B.voxels * sizeof(uint32_t);
    if (capacity < bytes) return fail(c, VV_ERR_INVALID, "vv_label_volume: capacity is below 4 bytes per voxel of the box");
    if (out_on_device) {
        if ((((uintptr_t)labels | (uintptr_t)sizes) & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_label_volume: device labels and sizes must be 4-byte aligned");
        if (((uintptr_t)stats & 7) != 0) return fail(c, VV_ERR_INVALID, "vv_label_volume: a device stats must be 8-byte aligned");
        // (by hand: the message names the pair, and the volume's comes first)
        if (ranges_overlap(labels, bytes, c->d_vol, c->alloc_bytes) || ranges_overlap(sizes, bytes, c->d_vol, c->alloc_bytes))
            return fail(c, VV_ERR_INVALID, "vv_label_volume: labels / sizes overlap the loaded volume");
        if (ranges_overlap(labels, bytes, sizes, bytes)) return fail(c, VV_ERR_INVALID, "vv_label_volume: labels and sizes overlap");
    }
    if (((uintptr_t)c->d_vol & 15) != 0 || !label_source_ok(c, B.hi) || !c->scratch[SC_LABEL].p)
        return fail(c, VV_ERR_DEVICE, "vv_label_volume: volume allocation is not what the kernel expects");
    A.bin_lo = (uint32_t)d->bin_lo; A.bin_hi = (uint32_t)d->bin_hi; A.connectivity = d->connectivity;
    A.counters = (unsigned long long *)c->scratch[SC_LABEL].p;
    const bool host = !out_on_device;
    CallBuf b[3] = {
        buf_out(labels, bytes, host),
        buf_out(sizes, bytes, host),
        buf_out_at(stats, sizeof(vv_label_stats), host, (char *)c->scratch[SC_LABEL].p + kLabelStatsOffset),
    };
    return run_out_volumes(c, who, b, 3, stream, [&](CallBuf *bb, hipStream_t st) {
        A.labels = (uint32_t *)bb[0].dev; A.sizes = (uint32_t *)bb[1].dev; A.stats = (vv_label_stats *)bb[2].dev;
        HIPCHK(c, hipMemsetAsync(A.counters, 0, kLabelCounters * sizeof(unsigned long long), st));
        launch_label(A, c->n_cu, c->knobs.label_blocks, c->knobs.label_phases, st);
        return (int)VV_OK;
    });
}

int vv_mask_volume(vv_context *c, const vv_mask *m, const uint32_t *labels, const uint32_t *sizes, void *out, size_t capacity, int on_device, void *stream)
{
    static const char who[] = "vv_mask_volume";
    MaskArgs A;
    CallBox B;
    int rc = open_box_call(c, c, who, m, labels && out, A, B);
    if (rc) return rc;
    // the header's rule M5, in its order
    if ((rc = check_out_type(c, who, m->out_type)) != VV_OK) return rc;
    if (m->keep != VV_KEEP_LABEL && m->keep != VV_KEEP_FOREGROUND && m->keep != VV_KEEP_MIN_SIZE)
        return fail(c, VV_ERR_INVALID, "vv_mask_volume: keep must be VV_KEEP_LABEL, VV_KEEP_FOREGROUND or VV_KEEP_MIN_SIZE");
    if (m->invert != 0 && m->invert != 1) return fail(c, VV_ERR_INVALID, "vv_mask_volume: invert must be 0 or 1");
    if (!std::isfinite(m->fill)) return fail(c, VV_ERR_INVALID, "vv_mask_volume: fill must be finite");
    if (m->keep == VV_KEEP_MIN_SIZE && !sizes) return fail(c, VV_ERR_INVALID, "vv_mask_volume: VV_KEEP_MIN_SIZE needs sizes");
    const int ext[3] = {(int)A.b[0], (int)A.b[1], (int)A.b[2]};
    size_t bytes;
    if ((rc = check_out_volume(c, who, "", out, capacity, on_device, m->out_type, ext, true, &bytes)) != VV_OK) return rc;
    const size_t lbytes = (size_t)B.voxels * sizeof(uint32_t);
    if (on_device) {
        if ((((uintptr_t)labels | (uintptr_t)sizes) & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_mask_volume: device labels and sizes must be 4-byte aligned");
        const Span s[3] = {{out, bytes, "out"}, {labels, lbytes, "labels"}, {sizes, lbytes, "sizes"}};
        if (first_overlap(s, 1, 3)) return fail(c, VV_ERR_INVALID, "vv_mask_volume: out overlaps labels or sizes (the pass is not in place)");
    }
    if (!label_source_ok(c, B.hi)) return fail(c, VV_ERR_DEVICE, "vv_mask_volume: volume allocation is not what the kernel expects");
    A.out_type = m->out_type; A.keep = m->keep; A.invert = m->invert;
    A.label = m->label; A.min_size = m->min_size; A.fill = m->fill;
    const bool host = !on_device;
    CallBuf b[3] = {
        buf_in(labels, lbytes, host),
        buf_in(sizes, m->keep == VV_KEEP_MIN_SIZE ? lbytes : 0, host),         // (read under VV_KEEP_MIN_SIZE only)
        buf_out(out, bytes, host),
    };
    return run_out_volumes(c, who, b, 3, stream, [&](CallBuf *bb, hipStream_t st) {
        A.labels = (const uint32_t *)bb[0].dev; A.sizes = (const uint32_t *)bb[1].dev; A.out = bb[2].dev;
        launch_mask(A, c->n_cu, c->knobs.label_blocks, st);
        return (int)VV_OK;
    });
}

// ---- distance transform (include/volviz.h: vv_distance_volume) ------------------------
int vv_distance_volume(vv_context *c, const vv_distance *d, const uint32_t *labels, uint32_t *out, size_t capacity, int on_device, void *stream)
{
    static const char who[] = "vv_distance_volume";
    DistanceArgs A;
    CallBox B;
    int rc = open_box_call(c, c, who, d, out != nullptr, A, B);
    if (rc) return rc;
    // the header's rule 10, in its order
    for (int a = 0; a < 3; ++a)
        if (A.b[a] > (uint32_t)VV_DISTANCE_MAX_EXTENT) return fail(c, VV_ERR_INVALID, "vv_distance_volume: every extent of the box must be at most 2048");
    if (d->seed != VV_SEED_BINS && d->seed != VV_SEED_LABEL && d->seed != VV_SEED_NONZERO)
        return fail(c, VV_ERR_INVALID, "vv_distance_volume: seed must be VV_SEED_BINS, VV_SEED_LABEL or VV_SEED_NONZERO");
    const bool bins = d->seed == VV_SEED_BINS;
    if (bins && (rc = check_bins(c, who, d->bin_lo, d->bin_hi)) != VV_OK) return rc;
    if (bins ? labels != nullptr : labels == nullptr) return fail(c, VV_ERR_INVALID, "vv_distance_volume: labels must be NULL for VV_SEED_BINS and given for the labels sources");
    if (d->invert != 0 && d->invert != 1) return fail(c, VV_ERR_INVALID, "vv_distance_volume: invert must be 0 or 1");
    for (int a = 0; a < 3; ++a)
        if (d->spacing[a] < 1) return fail(c, VV_ERR_INVALID, "vv_distance_volume: every spacing must be at least 1");
    unsigned long long bound = 0;
    for (int a = 0; a < 3; ++a) {                                           // (a term alone may pass 2^64: stop at the first one above the bound)
        const unsigned long long far = (unsigned long long)d->spacing[a] * (A.b[a] - 1);
        if (far > 0xFFFFull || (bound += far * far) > 0xFFFFFFFEull)
            return fail(c, VV_ERR_INVALID, "vv_distance_volume: the largest squared distance of the box, sum of (spacing (extent - 1))^2, must be at most 0xFFFFFFFE");
    }
    if (d->out != VV_DIST_SQUARED && d->out != VV_DIST_WITHIN) return fail(c, VV_ERR_INVALID, "vv_distance_volume: out must be VV_DIST_SQUARED or VV_DIST_WITHIN");
    const size_t bytes = (size_t)B.voxels * sizeof(uint32_t);
    if (capacity < bytes) return fail(c, VV_ERR_INVALID, "vv_distance_volume: capacity is below 4 bytes per voxel of the box");
    const bool aliased = labels == out;
    if (on_device) {
        if ((((uintptr_t)labels | (uintptr_t)out) & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_distance_volume: device labels and out must be 4-byte aligned");
        // (by hand: out == labels is the one overlap that is allowed)
        if (ranges_overlap(out, bytes, c->d_vol, c->alloc_bytes)) return fail(c, VV_ERR_INVALID, "vv_distance_volume: out overlaps the loaded volume");
        if (!aliased && ranges_overlap(out, bytes, labels, bytes))
            return fail(c, VV_ERR_INVALID, "vv_distance_volume: out overlaps labels without being the same pointer");
    }
    if (!label_source_ok(c, B.hi)) return fail(c, VV_ERR_DEVICE, "vv_distance_volume: volume allocation is not what the kernel expects");
    for (int a = 0; a < 3; ++a) A.spacing[a] = (uint32_t)d->spacing[a];
    A.bin_lo = (uint32_t)d->bin_lo; A.bin_hi = (uint32_t)d->bin_hi; A.label = d->label; A.within_r2 = d->within_r2;
    A.seed = d->seed; A.invert = d->invert; A.mode = d->out;
    const bool host = !on_device;
    // out == labels: one buffer, uploaded and downloaded; else the labels (if any) are an input and out an output
    CallBuf b[2] = {
        aliased ? buf_inout(out, bytes, host) : buf_out(out, bytes, host),
        buf_in(labels, aliased ? 0 : bytes, host),
    };
    return run_out_volumes(c, who, b, 2, stream, [&](CallBuf *bb, hipStream_t st) {
        A.out = (uint32_t *)bb[0].dev;
        A.labels = bins ? nullptr : aliased ? (const uint32_t *)bb[0].dev : (const uint32_t *)bb[1].dev;
        launch_distance(A, c->n_cu, c->knobs.distance_blocks, c->knobs.distance_phases, st);
        return (int)VV_OK;
    });
}

// ---- region measurements (include/volviz.h: vv_region_table) ------------------------
int vv_region_table(vv_context *c, const vv_regions *d, const uint32_t *labels, const uint32_t *aux, uint32_t *compact, size_t compact_capacity,
                    vv_region *table, size_t table_capacity, vv_region_summary *summary, int on_device, void *stream)
{
    static const char who[] = "vv_region_table";
    RegionArgs A;
    CallBox B;
    const int rc = open_box_call(c, c, who, d, labels && compact, A, B);
    if (rc) return rc;
    // the header's rule 8, in its order
    if (d->source != VV_REGION_LABELS && d->source != VV_REGION_NONZERO) return fail(c, VV_ERR_INVALID, "vv_region_table: source must be VV_REGION_LABELS or VV_REGION_NONZERO");
    if (!table && d->max_regions != 0) return fail(c, VV_ERR_INVALID, "vv_region_table: table is NULL with max_regions != 0");
    const size_t bytes = (size_t)B.voxels * sizeof(uint32_t);
    const unsigned long long tbytes = (unsigned long long)sizeof(vv_region) * d->max_regions;      // (below 2^40)
    if (compact_capacity < bytes) return fail(c, VV_ERR_INVALID, "vv_region_table: compact capacity is below 4 bytes per voxel of the box");
    if ((unsigned long long)table_capacity < tbytes) return fail(c, VV_ERR_INVALID, "vv_region_table: table capacity is below sizeof(vv_region) * max_regions");
    if (on_device) {
        if ((((uintptr_t)labels | (uintptr_t)aux | (uintptr_t)compact) & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_region_table: device labels, aux and compact must be 4-byte aligned");
        if ((((uintptr_t)table | (uintptr_t)summary) & 7) != 0) return fail(c, VV_ERR_INVALID, "vv_region_table: a device table and summary must be 8-byte aligned");
        // (the summary is not checked; a table without rows inside another buffer is refused like any other)
        const Span s[5] = {{compact, bytes, "compact"}, {table, (size_t)tbytes, "table"}, {labels, bytes, nullptr}, {aux, bytes, nullptr}, {c->d_vol, c->alloc_bytes, nullptr}};
        const char *name = first_overlap(s, 2, 5);
        if (name) return fail(c, VV_ERR_INVALID, std::string("vv_region_table: ") + name + (name == s[0].name ? " overlaps labels, aux, table or the loaded volume" : " overlaps labels, aux or the loaded volume"));
    }
    if (!label_source_ok(c, B.hi) || !c->scratch[SC_REGION].p) return fail(c, VV_ERR_DEVICE, "vv_region_table: volume allocation is not what the kernel expects");
    A.max_regions = d->max_regions; A.source = d->source;
    char *sc = (char *)c->scratch[SC_REGION].p;
    A.hdr = (unsigned long long *)sc; A.partials = (uint32_t *)(sc + kRegionPartialsOffset);
    const bool host = !on_device;
    // (a host table goes up before it comes down: the rows the kernels do not write keep the caller's bytes)
    CallBuf b[5] = {
        buf_in(labels, bytes, host),
        buf_in(aux, bytes, host),
        buf_out(compact, bytes, host),
        buf_inout(table, (size_t)tbytes, host),
        buf_out_at(summary, sizeof(vv_region_summary), host, sc + kRegionSummaryOffset),
    };
    return run_out_volumes(c, who, b, 5, stream, [&](CallBuf *bb, hipStream_t st) {
        A.labels = (const uint32_t *)bb[0].dev; A.aux = aux ? (const uint32_t *)bb[1].dev : nullptr; A.compact = (uint32_t *)bb[2].dev;
        A.table = d->max_regions ? (vv_region *)bb[3].dev : nullptr; A.summary = (vv_region_summary *)bb[4].dev;
        HIPCHK(c, hipMemsetAsync(A.hdr, 0, kRegionHeader * sizeof(unsigned long long), st));
        launch_region(A, c->knobs.region_blocks, c->knobs.region_chunks, c->knobs.region_phases, st);
        return (int)VV_OK;
    });
}

// ---- surface meshes (include/volviz.h: vv_mesh_dims, vv_surface_mesh) ------------------------
// What both calls share, rule 11 up to the site grid: the family's opening and the site grid's extents A.m.  A cap outside 0 / 1 is refused
// further down (rule 11's order); the grid is measured with it as it stands only where it is 0 or 1.
static int mesh_box(const vv_context *c, vv_context *err_to, const char *who, const vv_mesh *d, bool args_given, MeshArgs &A, CallBox &B)
{
    const int rc = open_box_call(c, err_to, who, d, args_given, A, B);
    if (rc) return rc;
    const uint32_t pad = d->cap == 1 ? 2u : 0u;
    for (int a = 0; a < 3; ++a) A.m[a] = A.b[a] - 1u + pad;
    // (each extent is below 2^24 + 2: the product of two fits 64 bits, and the third is applied only to a product below 2^32)
    const unsigned long long two = (unsigned long long)A.m[0] * A.m[1];
    if (two > 0xFFFFFFFEull || two * A.m[2] > 0xFFFFFFFEull) return fail(err_to, VV_ERR_INVALID, std::string(who) + ": the site grid may hold at most 2^32 - 2 sites");
    return VV_OK;
}

int vv_mesh_dims(const vv_context *c, const vv_mesh *d, int out_dims[3])
{
    vv_context *e = const_cast<vv_context *>(c);                    // (the message alone)
    MeshArgs A;
    CallBox B;
    const int rc = mesh_box(c, e, "vv_mesh_dims", d, out_dims != nullptr, A, B);
    if (rc) return rc;
    if (d->cap != 0 && d->cap != 1) return fail(e, VV_ERR_INVALID, "vv_mesh_dims: cap must be 0 or 1");
    for (int a = 0; a < 3; ++a) out_dims[a] = (int)A.m[a];
    return VV_OK;
}

int vv_surface_mesh(vv_context *c, const vv_mesh *d, const uint32_t *labels, uint32_t *index, size_t index_capacity,
                    vv_mesh_vertex *vertices, size_t vertices_capacity, vv_mesh_normal *normals, uint32_t *quads, size_t quads_capacity,
                    vv_mesh_summary *summary, int on_device, void *stream)
{
    static const char who[] = "vv_surface_mesh";
    MeshArgs A;
    CallBox B;
    int rc = mesh_box(c, c, who, d, true, A, B);
    if (rc) return rc;
    // the header's rule 11, in its order
    if (d->source != VV_MESH_INDEX && d->source != VV_MESH_BINS && d->source != VV_MESH_LABEL && d->source != VV_MESH_NONZERO)
        return fail(c, VV_ERR_INVALID, "vv_surface_mesh: source must be VV_MESH_INDEX, VV_MESH_BINS, VV_MESH_LABEL or VV_MESH_NONZERO");
    if (d->source == VV_MESH_INDEX && !(1 <= d->level && d->level <= 255)) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: level must lie in 1..255");
    if (d->source == VV_MESH_BINS && (rc = check_bins(c, who, d->bin_lo, d->bin_hi)) != VV_OK) return rc;
    const bool from_labels = d->source == VV_MESH_LABEL || d->source == VV_MESH_NONZERO;
    if (from_labels ? labels == nullptr : labels != nullptr)
        return fail(c, VV_ERR_INVALID, "vv_surface_mesh: labels must be given for the labels sources and NULL for VV_MESH_INDEX and VV_MESH_BINS");
    if (d->cap != 0 && d->cap != 1) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: cap must be 0 or 1");
    if (!index && (d->max_vertices != 0 || d->max_quads != 0)) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: index is NULL with a non-zero maximum");
    if (!vertices && d->max_vertices != 0) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: vertices is NULL with max_vertices != 0");
    if (!quads && d->max_quads != 0) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: quads is NULL with max_quads != 0");
    const unsigned long long sites = (unsigned long long)A.m[0] * A.m[1] * A.m[2];                 // (at most 2^32 - 2: mesh_box)
    const unsigned long long ibytes = index ? 4ull * sites : 0ull, vbytes = 16ull * d->max_vertices, qbytes = 16ull * d->max_quads;
    if ((unsigned long long)index_capacity < ibytes) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: index capacity is below 4 bytes per site (vv_mesh_dims)");
    if ((unsigned long long)vertices_capacity < vbytes) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: vertices capacity is below 16 bytes * max_vertices");
    if ((unsigned long long)quads_capacity < qbytes) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: quads capacity is below 16 bytes * max_quads");
    const size_t lbytes = (size_t)B.voxels * sizeof(uint32_t);        // (labels are NULL unless the source reads them)
    if (on_device) {
        if ((((uintptr_t)labels | (uintptr_t)index) & 3) != 0) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: device labels and index must be 4-byte aligned");
        if ((((uintptr_t)vertices | (uintptr_t)normals | (uintptr_t)quads) & 15) != 0)
            return fail(c, VV_ERR_INVALID, "vv_surface_mesh: device vertices, normals and quads must be 16-byte aligned");
        if (((uintptr_t)summary & 7) != 0) return fail(c, VV_ERR_INVALID, "vv_surface_mesh: a device summary must be 8-byte aligned");
        // every output against the input, the volume and the outputs behind it in the list; a buffer without a record overlaps nothing
        const Span s[7] = {nonempty(index, (size_t)ibytes, "index"), nonempty(vertices, (size_t)vbytes, "vertices"), nonempty(normals, (size_t)vbytes, "normals"),
                           nonempty(quads, (size_t)qbytes, "quads"), {summary, sizeof(vv_mesh_summary), "summary"}, {labels, lbytes, nullptr}, {c->d_vol, c->alloc_bytes, nullptr}};
        const char *name = first_overlap(s, 5, 7);
        if (name) return fail(c, VV_ERR_INVALID, std::string("vv_surface_mesh: ") + name + " overlaps another buffer of the call or the loaded volume");
    }
    // what the kernels may read of [d_vol, d_vol + alloc_bytes): the box's voxels at the two pitches and nothing else (virtual voxels are clamped into
    // the box before they are addressed); f32 voxels are loaded as aligned words
    if (!label_source_ok(c, B.hi) || !c->scratch[SC_MESH].p) return fail(c, VV_ERR_DEVICE, "vv_surface_mesh: volume allocation is not what the kernel expects");
    A.level = d->source == VV_MESH_INDEX ? (uint32_t)d->level : 1u;
    A.bin_lo = (uint32_t)d->bin_lo; A.bin_hi = (uint32_t)d->bin_hi; A.label = d->label;
    A.max_vertices = d->max_vertices; A.max_quads = d->max_quads;
    A.source = d->source; A.cap = d->cap;
    char *sc = (char *)c->scratch[SC_MESH].p;
    A.hdr = (unsigned long long *)sc; A.partials = (MeshPartial *)(sc + kMeshPartialsOffset);
    const bool host = !on_device;
    // (host tables go up before they come down: the records the kernels do not write keep the caller's bytes)
    CallBuf b[6] = {
        buf_in(labels, lbytes, host),
        buf_out(index, (size_t)ibytes, host),
        buf_inout(vertices, (size_t)vbytes, host),
        buf_inout(normals, (size_t)vbytes, host),
        buf_inout(quads, (size_t)qbytes, host),
        buf_out_at(summary, sizeof(vv_mesh_summary), host, sc + kMeshSummaryOffset),
    };
    return run_out_volumes(c, who, b, 6, stream, [&](CallBuf *bb, hipStream_t st) {
        A.labels = from_labels ? (const uint32_t *)bb[0].dev : nullptr; A.index = index ? (uint32_t *)bb[1].dev : nullptr;
        A.vertices = d->max_vertices ? (vv_mesh_vertex *)bb[2].dev : nullptr; A.normals = d->max_vertices && normals ? (vv_mesh_normal *)bb[3].dev : nullptr;
        A.quads = d->max_quads ? (uint4 *)bb[4].dev : nullptr; A.summary = (vv_mesh_summary *)bb[5].dev;
        launch_mesh(A, c->knobs.mesh_blocks, c->knobs.mesh_chunks, c->knobs.mesh_phases, st);
        return (int)VV_OK;
    });
}

// ---- generator: VolumeGenerator::drawEllipsoid / drawDefaultBrain ------------------------
static int generate_impl(vv_context *c, uint8_t *out, int out_on_device, int nx, int ny, int nz, int n,
                         const float *centers, const float *axes, const uint8_t *colors, int in_place, void *stream)
{
    if (!c) return fail(nullptr, VV_ERR_INVALID, "vv_generate_ellipsoids: NULL context");
    if (!out || nx < 1 || ny < 1 || nz < 1 || n < 0 || n > kMaxEllipsoids || (n > 0 && (!centers || !axes || !colors)))
        return fail(c, VV_ERR_INVALID, "vv_generate_ellipsoids: bad argument (n <= 64)");
    if ((((unsigned long long)nx + 15ull) / 16ull) * (unsigned long long)ny >= (1ull << 31))
        return fail(c, VV_ERR_INVALID, "vv_generate_ellipsoids: a slice must have fewer than 2^31 16-voxel chunks");
    if (out_on_device && ((uintptr_t)out & 15) != 0) return fail(c, VV_ERR_INVALID, "vv_generate_ellipsoids: device buffer must be 16-byte aligned");     // (a staging buffer is)
    return run_out_volume(c, "vv_generate_ellipsoids", out, (size_t)nx * ny * nz, out_on_device, in_place != 0, stream, [&](void *dev, hipStream_t st) {
        const int rc = ensure(c, SC_GEN, generate_scratch_floats(nx, ny, nz, n) * sizeof(float));
        if (rc) return rc;
        launch_generate_ellipsoids((uint8_t *)dev, nx, ny, nz, n, centers, axes, colors, in_place, (float *)c->scratch[SC_GEN].p, st);
        return (int)VV_OK;
    });
}

int vv_generate_ellipsoids(vv_context *c, uint8_t *out, int out_on_device, int nx, int ny, int nz, int n,
                           const float *centers, const float *axes, const uint8_t *colors, void *stream)
{
    return generate_impl(c, out, out_on_device, nx, ny, nz, n, centers, axes, colors, 0, stream);
}

int vv_draw_ellipsoid(vv_context *c, uint8_t *vol, int vol_on_device, int nx, int ny, int nz,
                      const float center[3], const float axes[3], uint8_t color, void *stream)
{
    return generate_impl(c, vol, vol_on_device, nx, ny, nz, 1, center, axes, &color, 1, stream);
}

int vv_generate_default_brain(vv_context *c, uint8_t *out, int out_on_device, int nx, int ny, int nz, void *stream)
{
    // volumegenerator.cpp:100-119: centre-major, layer-minor; later ellipsoids overwrite earlier
    static const float centers2[2][3] = { {0.25f, 0.50f, 0.50f}, {0.75f, 0.50f, 0.50f} };
    static const float layers4[4][3]  = { {0.23f, 0.30f, 0.45f}, {0.18f, 0.27f, 0.40f},
                                          {0.10f, 0.23f, 0.30f}, {0.03f, 0.20f, 0.20f} };
    static const uint8_t shades4[4] = { 60, 80, 100, 120 };
    float centers[8 * 3], axes[8 * 3]; uint8_t colors[8];
    int e = 0;
    for (int ci = 0; ci < 2; ++ci) for (int li = 0; li < 4; ++li, ++e) {
        for (int a = 0; a < 3; ++a) { centers[3*e+a] = centers2[ci][a]; axes[3*e+a] = layers4[li][a]; }
        colors[e] = shades4[li];
    }
    return vv_generate_ellipsoids(c, out, out_on_device, nx, ny, nz, 8, centers, axes, colors, stream);
}

int vv_promote_u8_to_f32(vv_context *c, const uint8_t *dev_in, float *dev_out, size_t n, void *stream)
{
    if (!c || !dev_in || !dev_out) return fail(c, VV_ERR_INVALID, "vv_promote_u8_to_f32: NULL argument");
    if (((uintptr_t)dev_in & 15) || ((uintptr_t)dev_out & 15)) return fail(c, VV_ERR_INVALID, "vv_promote_u8_to_f32: buffers must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, stream);
    launch_promote_u8_f32(dev_in, dev_out, n, st);
    return finish_call(c, stream, st, nullptr, 0);
}

int vv_generate_noise_u8(vv_context *c, uint8_t *dev_out, int nx, int ny, int nz, uint32_t seed, void *stream)
{
    if (!c || !dev_out || nx < 1 || ny < 1 || nz < 1) return fail(c, VV_ERR_INVALID, "vv_generate_noise_u8: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, stream);
    launch_noise_u8(dev_out, nx, ny, nz, seed, st);
    return finish_call(c, stream, st, nullptr, 0);
}

} // extern "C"
