"""ctypes binding of the C-ABI in include/volviz.h (libvolviz_hip.so).

This is the host-side mirror used by tests/, bench.py and __graft_entry__.py.  It is a
thin 1:1 wrapper: every method names the C entry point it calls, which in turn cites
the reference interface it replaces (kernel.cuh / volumegenerator.h).  There is no
Python or CPU implementation of any kernel here -- if the shared library or a HIP
device is missing, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.normpath(os.path.join(_HERE, "..", ".."))          # volume-viz_amd/
REPO_ROOT = os.path.normpath(os.path.join(PKG_ROOT, ".."))
LIB_PATH = os.environ.get("VV_LIB", os.path.join(PKG_ROOT, "lib", "libvolviz_hip.so"))

# kernel.cuh:18-20
SLICE_NONE, SLICE_PLANE, SLICE_PLANE_CUT = -1, 0, 1
# params.h:46
HORIZONTAL, SAGITTAL, CORONAL, FREE_FORM = 0, 1, 2, 4
VOXEL_U8, VOXEL_F32 = 0, 1
LAYOUT_BRICKED, LAYOUT_ZPAIR, LAYOUT_ZFAST, LAYOUT_POLICY = 1, 2, 4, 256
FILTER_TEX8, FILTER_EXACT = 0, 1
ERT_REFERENCE, ERT_TRUE = 0, 1
SLAB_MAX, SLAB_MIN, SLAB_MEAN = 0, 1, 2          # vv_slab_mode
SLAB_MAX_SAMPLES = 1024
PROJ_MAX, PROJ_MIN, PROJ_MEAN = 0, 1, 2          # vv_proj_mode
REDUCE_MEAN, REDUCE_MAX, REDUCE_MIN = 0, 1, 2    # vv_reduce_mode
STENCIL_SEPARABLE, STENCIL_MEDIAN, STENCIL_GRADMAG = 0, 1, 2     # vv_stencil_kind
STENCIL_MAX_RADIUS = 4
TAPS_BOX, TAPS_BINOMIAL, TAPS_GAUSS = 0, 1, 2    # vv_taps_shape
RESAMPLE_TEX8, RESAMPLE_EXACT, RESAMPLE_NEAREST = 0, 1, 2        # vv_resample_filter
RESAMPLE_MAX_DIM = 16384
KEEP_LABEL, KEEP_FOREGROUND, KEEP_MIN_SIZE = 0, 1, 2             # vv_keep
SEED_BINS, SEED_LABEL, SEED_NONZERO = 0, 1, 2                    # vv_seed
DIST_SQUARED, DIST_WITHIN = 0, 1                                 # vv_dist_out
DISTANCE_MAX_EXTENT = 2048
DISTANCE_NONE = 0xFFFFFFFF                                       # DIST_SQUARED of a box without a seed
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3  # Context.morphology
REGION_LABELS, REGION_NONZERO = 0, 1                             # vv_region_source
MESH_INDEX, MESH_BINS, MESH_LABEL, MESH_NONZERO = 0, 1, 2, 3     # vv_mesh_source
RAYS_IMAGES, RAYS_ANALYTIC = 0, 1
TF_ENGINE, TF_HEAD, TF_MRI = 0, 1, 2
# `stream` arguments: 0/None = the context's own stream, synchronous; STREAM_DEFAULT_ASYNC = the device's default (null)
# stream, enqueue only (include/volviz.h VV_STREAM_DEFAULT_ASYNC); any other hipStream_t handle = that stream, enqueue only
STREAM_DEFAULT_ASYNC = 1


def stream_handle(torch_stream) -> int:
    """hipStream_t of a torch.cuda.Stream for the `stream` arguments (torch's default stream has handle 0, which the
    C-ABI reads as 'no stream': it maps to STREAM_DEFAULT_ASYNC)."""
    h = int(torch_stream.cuda_stream)
    return h if h != 0 else STREAM_DEFAULT_ASYNC


class slice_params(C.Structure):          # kernel.cuh:26-29
    _fields_ = [("type", C.c_int), ("params", C.c_float * 6)]


class camera_params(C.Structure):         # kernel.cuh:31-35
    _fields_ = [("origin", C.c_float * 3), ("fovX", C.c_float), ("fovY", C.c_float),
                ("scale", C.c_float * 3)]


class shading_params(C.Structure):        # kernel.cuh:37-40
    _fields_ = [("transferPreset", C.c_int), ("phongShading", C.c_bool)]


class vv_ray_source(C.Structure):
    _fields_ = [("mode", C.c_int), ("front", C.c_void_p), ("back", C.c_void_p),
                ("img_w", C.c_int), ("img_h", C.c_int), ("images_on_device", C.c_int),
                ("look", C.c_float * 3), ("up", C.c_float * 3), ("aspect", C.c_float),
                ("quantize8", C.c_int)]


class vv_render_options(C.Structure):
    _fields_ = [("step", C.c_float * 3), ("ert_threshold", C.c_float), ("filter", C.c_int),
                ("ert_mode", C.c_int), ("slab_row_begin", C.c_int), ("slab_row_end", C.c_int),
                ("shard_band", C.c_int), ("shard_count", C.c_int), ("shard_index", C.c_int),
                ("count_samples", C.c_int), ("touched_bricks", C.c_void_p),
                ("touched_lines", C.c_void_p), ("touched_line_bits", C.c_ulonglong), ("touched_lines_all", C.c_int),
                ("touched_block_lines", C.c_void_p), ("touched_block_lines_log2", C.c_int)]


class vv_slab(C.Structure):
    _fields_ = [("mode", C.c_int), ("samples", C.c_int), ("thickness", C.c_float)]


class vv_histogram(C.Structure):          # 2072 bytes
    _fields_ = [("counts", C.c_ulonglong * 256), ("voxels", C.c_ulonglong), ("nan_voxels", C.c_ulonglong),
                ("vmin", C.c_float), ("vmax", C.c_float)]


class vv_derive(C.Structure):             # 56 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("factor", C.c_int * 3), ("mode", C.c_int),
                ("out_type", C.c_int), ("window", C.c_int), ("win_lo", C.c_float), ("win_hi", C.c_float)]


class vv_stencil(C.Structure):            # 116 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("kind", C.c_int), ("out_type", C.c_int), ("radius", C.c_int * 3),
                ("taps", (C.c_float * 5) * 3), ("gscale", C.c_float * 3)]


class vv_resample(C.Structure):           # 96 bytes
    _fields_ = [("dims", C.c_int * 3), ("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("filter", C.c_int), ("out_type", C.c_int),
                ("m", C.c_float * 12), ("fill", C.c_float)]


class vv_label(C.Structure):              # 36 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("bin_lo", C.c_int), ("bin_hi", C.c_int), ("connectivity", C.c_int)]


class vv_label_stats(C.Structure):        # 32 bytes
    _fields_ = [("foreground", C.c_ulonglong), ("components", C.c_ulonglong), ("largest_size", C.c_ulonglong),
                ("largest_label", C.c_uint32), ("reserved", C.c_uint32)]


class vv_mask(C.Structure):               # 48 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("out_type", C.c_int), ("keep", C.c_int), ("invert", C.c_int),
                ("label", C.c_uint32), ("min_size", C.c_uint32), ("fill", C.c_float)]


class vv_distance(C.Structure):           # 64 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("seed", C.c_int), ("bin_lo", C.c_int), ("bin_hi", C.c_int),
                ("label", C.c_uint32), ("invert", C.c_int), ("spacing", C.c_int * 3), ("out", C.c_int), ("within_r2", C.c_uint32)]


class vv_regions(C.Structure):            # 32 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("source", C.c_int), ("max_regions", C.c_uint32)]


class vv_region(C.Structure):             # 184 bytes, 8-byte aligned
    _fields_ = [("label", C.c_uint32), ("reserved", C.c_uint32), ("voxels", C.c_ulonglong), ("lo", C.c_int * 3), ("hi", C.c_int * 3),
                ("sum", C.c_ulonglong * 3), ("sum2", C.c_ulonglong * 6), ("bin_min", C.c_uint32), ("bin_max", C.c_uint32),
                ("bin_sum", C.c_ulonglong), ("bin_sum2", C.c_ulonglong), ("vmin", C.c_float), ("vmax", C.c_float),
                ("faces", C.c_ulonglong * 3), ("aux_sum", C.c_ulonglong), ("aux_argmax", C.c_uint32), ("aux_max", C.c_uint32)]


class vv_region_summary(C.Structure):     # 32 bytes
    _fields_ = [("regions", C.c_ulonglong), ("written", C.c_ulonglong), ("foreground", C.c_ulonglong), ("stray", C.c_ulonglong)]


# vv_region as a numpy structured dtype: a table is np.ndarray[max_regions] of it (vmin / vmax: compare them as uint32 patterns)
REGION_DTYPE = np.dtype({
    "names": ["label", "reserved", "voxels", "lo", "hi", "sum", "sum2", "bin_min", "bin_max", "bin_sum", "bin_sum2", "vmin", "vmax",
              "faces", "aux_sum", "aux_argmax", "aux_max"],
    "formats": ["<u4", "<u4", "<u8", ("<i4", 3), ("<i4", 3), ("<u8", 3), ("<u8", 6), "<u4", "<u4", "<u8", "<u8", "<f4", "<f4",
                ("<u8", 3), "<u8", "<u4", "<u4"],
    "offsets": [0, 4, 8, 16, 28, 40, 64, 112, 116, 120, 128, 136, 140, 144, 168, 176, 180],
    "itemsize": 184})
assert C.sizeof(vv_regions) == 32 and C.sizeof(vv_region) == 184 and C.alignment(vv_region) == 8 and C.sizeof(vv_region_summary) == 32
assert all(getattr(vv_region, n).offset == REGION_DTYPE.fields[n][1] for n in REGION_DTYPE.names), "vv_region layout (include/volviz.h)"


class vv_mesh(C.Structure):               # 56 bytes
    _fields_ = [("box_lo", C.c_int * 3), ("box_hi", C.c_int * 3), ("source", C.c_int), ("level", C.c_int), ("bin_lo", C.c_int), ("bin_hi", C.c_int),
                ("label", C.c_uint32), ("cap", C.c_int), ("max_vertices", C.c_uint32), ("max_quads", C.c_uint32)]


class vv_mesh_vertex(C.Structure):        # 16 bytes
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("site", C.c_uint32)]


class vv_mesh_normal(C.Structure):        # 16 bytes
    _fields_ = [("g", C.c_int32 * 3), ("edges", C.c_uint32)]


class vv_mesh_summary(C.Structure):       # 32 bytes
    _fields_ = [("vertices", C.c_ulonglong), ("quads", C.c_ulonglong), ("written_vertices", C.c_ulonglong), ("written_quads", C.c_ulonglong)]


# vv_mesh_vertex / vv_mesh_normal as numpy structured dtypes (compare x, y, z as uint32 patterns)
MESH_VERTEX_DTYPE = np.dtype({"names": ["x", "y", "z", "site"], "formats": ["<f4", "<f4", "<f4", "<u4"], "offsets": [0, 4, 8, 12], "itemsize": 16})
MESH_NORMAL_DTYPE = np.dtype({"names": ["g", "edges"], "formats": [("<i4", 3), "<u4"], "offsets": [0, 12], "itemsize": 16})
assert C.sizeof(vv_mesh) == 56 and C.sizeof(vv_mesh_vertex) == 16 and C.sizeof(vv_mesh_normal) == 16 and C.sizeof(vv_mesh_summary) == 32
assert all(getattr(vv_mesh_vertex, n).offset == MESH_VERTEX_DTYPE.fields[n][1] for n in MESH_VERTEX_DTYPE.names), "vv_mesh_vertex layout (include/volviz.h)"
assert all(getattr(vv_mesh_normal, n).offset == MESH_NORMAL_DTYPE.fields[n][1] for n in MESH_NORMAL_DTYPE.names), "vv_mesh_normal layout (include/volviz.h)"


@dataclass
class MeshSummary:
    """vv_mesh_summary as Python ints."""
    vertices: int
    quads: int
    written_vertices: int
    written_quads: int

    @staticmethod
    def from_bytes(raw) -> "MeshSummary":
        """From the 32 bytes of a vv_mesh_summary (e.g. read back from a device buffer)."""
        q = np.frombuffer(bytes(raw), np.uint8, C.sizeof(vv_mesh_summary)).view(np.uint64)
        return MeshSummary(int(q[0]), int(q[1]), int(q[2]), int(q[3]))


@dataclass
class Mesh:
    """What Context.surface returns: vertices float32 [V, 3] in volume voxel coordinates, sites uint32 [V] (the cell each vertex lies in), quads uint32
    [Q, 4] (0-based, counter-clockwise seen from outside), normals (MESH_NORMAL_DTYPE [V]) or None, index uint32 [m_z, m_y, m_x] or None."""
    vertices: np.ndarray
    sites: np.ndarray
    quads: np.ndarray
    normals: Optional[np.ndarray] = None
    index: Optional[np.ndarray] = None


def mesh_triangles(quads) -> np.ndarray:
    """Every quad (a, b, c, d) split along (0, 2) into (a, b, c) and (a, c, d): uint32 [2 Q, 3], same winding (host only)."""
    q = np.asarray(quads, np.uint32).reshape(-1, 4)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


def mesh_area_volume(mesh, spacing=(1.0, 1.0, 1.0)):
    """(area, signed volume) of the triangles of mesh_triangles, in binary64, with the voxel pitch `spacing` (x, y, z).  The volume is that of a
    closed mesh (cap=True) and positive for the library's winding (host only)."""
    v = np.asarray(mesh.vertices, np.float64).reshape(-1, 3) * np.asarray(spacing, np.float64).reshape(3)
    t = mesh_triangles(mesh.quads).astype(np.int64)
    if not len(t):
        return 0.0, 0.0
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    cross = np.cross(b - a, c - a)
    return float(np.sqrt((cross * cross).sum(axis=1)).sum() / 2.0), float((a * np.cross(b, c)).sum() / 6.0)


def write_obj(path, mesh, spacing=(1.0, 1.0, 1.0)) -> None:
    """Wavefront OBJ of a Mesh: `v` lines (coordinates times `spacing`), `vn` lines from the normalised integer normals when the mesh has them (a zero
    normal is written as 0 0 1), `f` lines with the quads, 1-based (host only)."""
    sp = np.asarray(spacing, np.float64).reshape(3)
    v = np.asarray(mesh.vertices, np.float64).reshape(-1, 3) * sp
    with open(path, "w") as f:
        f.write(f"# {len(v)} vertices, {len(mesh.quads)} quads\n")
        for x, y, z in v:
            f.write(f"v {x:.9g} {y:.9g} {z:.9g}\n")
        if mesh.normals is not None:
            n = mesh.normals["g"].astype(np.float64) / sp                # (a gradient: it scales with the inverse pitch)
            length = np.sqrt((n * n).sum(axis=1))
            n = np.where(length[:, None] > 0, n / np.maximum(length, 1e-300)[:, None], np.array([0.0, 0.0, 1.0]))
            for x, y, z in n:
                f.write(f"vn {x:.9g} {y:.9g} {z:.9g}\n")
        for q in np.asarray(mesh.quads, np.int64).reshape(-1, 4) + 1:
            f.write("f " + " ".join(f"{k}//{k}" if mesh.normals is not None else f"{k}" for k in q) + "\n")


@dataclass
class RegionSummary:
    """vv_region_summary as Python ints."""
    regions: int
    written: int
    foreground: int
    stray: int

    @staticmethod
    def from_bytes(raw) -> "RegionSummary":
        """From the 32 bytes of a vv_region_summary (e.g. read back from a device buffer)."""
        q = np.frombuffer(bytes(raw), np.uint8, C.sizeof(vv_region_summary)).view(np.uint64)
        return RegionSummary(int(q[0]), int(q[1]), int(q[2]), int(q[3]))


def region_properties(table, spacing=(1.0, 1.0, 1.0)) -> dict:
    """What a vv_region table says in physical units, in binary64 (host only).  spacing = the voxel pitch (x, y, z).  Per row: voxels, volume,
    centroid [n, 3] (voxel-centre coordinates times the pitch), surface_area (faces[a] times the product of the other two pitches), covariance
    [n, 3, 3] of the coordinates (population covariance: E[pq] - E[p]E[q], scaled by the pitches), bbox_lo / bbox_hi [n, 3] in voxels, mean_bin,
    and inscribed_radius = sqrt(aux_max) (the unit of aux: with the squared distances of vv_distance_volume to the complement, the radius of the
    largest ball centred on a voxel of the region that stays inside it)."""
    t = np.atleast_1d(np.asarray(table))
    sp = np.asarray(spacing, np.float64).reshape(3)
    n = t["voxels"].astype(np.float64)
    mean = t["sum"].astype(np.float64) / n[:, None]
    s2 = t["sum2"].astype(np.float64) / n[:, None]
    cov = np.empty((len(t), 3, 3), np.float64)
    for (p, q), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}.items():
        cov[:, p, q] = cov[:, q, p] = (s2[:, k] - mean[:, p] * mean[:, q]) * sp[p] * sp[q]
    faces = t["faces"].astype(np.float64)
    area = faces[:, 0] * sp[1] * sp[2] + faces[:, 1] * sp[0] * sp[2] + faces[:, 2] * sp[0] * sp[1]
    return dict(label=t["label"].copy(), voxels=t["voxels"].copy(), volume=n * sp.prod(), centroid=mean * sp, surface_area=area, covariance=cov,
                bbox_lo=t["lo"].copy(), bbox_hi=t["hi"].copy(), mean_bin=t["bin_sum"].astype(np.float64) / n,
                inscribed_radius=np.sqrt(t["aux_max"].astype(np.float64)))


@dataclass
class LabelStats:
    """vv_label_stats as Python ints."""
    foreground: int
    components: int
    largest_size: int
    largest_label: int
    reserved: int = 0

    @staticmethod
    def from_bytes(raw) -> "LabelStats":
        """From the 32 bytes of a vv_label_stats (e.g. read back from a device buffer)."""
        raw = np.frombuffer(bytes(raw), np.uint8, C.sizeof(vv_label_stats))
        q, w = raw[:24].view(np.uint64), raw[24:].view(np.uint32)
        return LabelStats(int(q[0]), int(q[1]), int(q[2]), int(w[0]), int(w[1]))


@dataclass
class Histogram:
    """vv_histogram as numpy values: counts uint64[256], voxels, nan_voxels, vmin / vmax as np.float32 (bit for bit what the library wrote)."""
    counts: np.ndarray
    voxels: int
    nan_voxels: int
    vmin: np.float32
    vmax: np.float32

    @staticmethod
    def from_bytes(raw) -> "Histogram":
        """From the 2072 bytes of a vv_histogram (e.g. read back from a device buffer)."""
        raw = np.frombuffer(bytes(raw), np.uint8, C.sizeof(vv_histogram))
        q = raw[:258 * 8].view(np.uint64)
        f = raw[258 * 8:].view(np.float32)
        return Histogram(q[:256].copy(), int(q[256]), int(q[257]), f[0], f[1])


EXPORTS = [
    "vv_init", "vv_shutdown", "vv_last_error", "vv_load_volume_u8", "vv_load_volume_f32",
    "vv_load_volume_device", "vv_set_transfer_function", "vv_render", "vv_slice",
    "vv_slice_advanced", "vv_generate_ellipsoids", "vv_generate_default_brain",
    "vv_promote_u8_to_f32", "vv_generate_noise_u8", "vv_transfer_preset",
    "vv_t3d_read_header", "vv_t3d_read", "vv_t3d_write", "vv_last_frame_ms",
    "vv_last_sample_count", "vv_volume_dims", "vv_slice_matrix", "vv_draw_ellipsoid", "vv_debug_counters",
    "vv_first_pass", "vv_cut_plane_canonical", "vv_cut_plane_from_euler", "vv_cut_plane_to_slice_params", "vv_slice_to_bgra",
    "vv_camera_orbit_drag", "vv_camera_zoom", "vv_cut_plane_from_drag", "vv_cut_plane_drag",
    "vv_prepare_layouts", "vv_set_layout_policy", "vv_layout_state", "vv_device_bytes", "vv_reread_env",
    "vv_load_volume_stream_begin", "vv_load_volume_stream_slices", "vv_load_volume_stream_end", "vv_load_volume_t3d",
    "vv_load_volume_stream_slices_async", "vv_load_volume_stream_wait_source", "vv_dataset_preset", "vv_debug_last_launch", "vv_set_frame_timing", "vv_debug_screen_rect",
    "vv_render_mip", "vv_classify_indices", "vv_render_iso", "vv_slice_slab", "vv_slice_advanced_slab",
    "vv_volume_histogram", "vv_histogram_indices", "vv_render_projection", "vv_debug_read_layout",
    "vv_derive_dims", "vv_derive_volume", "vv_stencil_volume", "vv_stencil_taps", "vv_resample_volume", "vv_resample_matrix",
    "vv_label_volume", "vv_mask_volume", "vv_distance_volume", "vv_debug_prepass_state", "vv_region_table",
    "vv_mesh_dims", "vv_surface_mesh",
]
# entry points a variant library built from an earlier tree (A/B tools, load_library(path)) may lack
_NEWER_EXPORTS = ("vv_render_mip", "vv_classify_indices", "vv_render_iso", "vv_slice_slab", "vv_slice_advanced_slab",
                  "vv_volume_histogram", "vv_histogram_indices", "vv_render_projection", "vv_debug_read_layout",
                  "vv_derive_dims", "vv_derive_volume", "vv_stencil_volume", "vv_stencil_taps", "vv_resample_volume", "vv_resample_matrix",
                  "vv_label_volume", "vv_mask_volume", "vv_distance_volume", "vv_debug_prepass_state", "vv_region_table",
                  "vv_mesh_dims", "vv_surface_mesh")

_lib = None
_libs = {}


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libvolviz_hip.so and declare the prototypes.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is not None and path in _libs:
        return _libs[path]
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not found: build it with `make -C {PKG_ROOT}` "
                           "(python __graft_entry__.py does). There is no fallback path.")
    lib = C.CDLL(p)
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    lib.vv_init.argtypes = [i, C.POINTER(vp)]
    lib.vv_shutdown.argtypes = [vp]
    lib.vv_last_error.argtypes = [vp]; lib.vv_last_error.restype = C.c_char_p
    lib.vv_load_volume_u8.argtypes = [vp, vp, sz, i, i, i, vp]
    lib.vv_load_volume_f32.argtypes = [vp, vp, sz, i, i, i, vp]
    lib.vv_load_volume_device.argtypes = [vp, vp, i, i, i, i, vp, vp]
    lib.vv_set_transfer_function.argtypes = [vp, vp]
    lib.vv_load_volume_stream_begin.argtypes = [vp, i, i, i, i, vp]
    lib.vv_load_volume_stream_slices.argtypes = [vp, vp, i, i, i]
    lib.vv_load_volume_stream_slices_async.argtypes = [vp, vp, i, i, i]
    lib.vv_load_volume_stream_wait_source.argtypes = [vp]
    lib.vv_load_volume_stream_end.argtypes = [vp]
    lib.vv_load_volume_t3d.argtypes = [vp, C.c_char_p, i, i, vp]
    lib.vv_render.argtypes = [vp, i, i, C.POINTER(slice_params), C.POINTER(camera_params),
                              C.POINTER(shading_params), C.POINTER(vv_ray_source),
                              C.POINTER(vv_render_options), vp, i, vp]
    if hasattr(lib, "vv_render_mip"):
        lib.vv_render_mip.argtypes = [vp, i, i, C.POINTER(slice_params), C.POINTER(camera_params), C.POINTER(vv_ray_source),
                                      C.POINTER(vv_render_options), vp, vp, i, vp]
        lib.vv_classify_indices.argtypes = [vp, vp, sz, vp, vp, i, vp]
    if hasattr(lib, "vv_render_iso"):
        lib.vv_render_iso.argtypes = [vp, i, i, C.POINTER(slice_params), C.POINTER(camera_params), C.POINTER(vv_ray_source),
                                      C.POINTER(vv_render_options), i, vp, vp, vp, i, vp]
    if hasattr(lib, "vv_render_projection"):
        lib.vv_render_projection.argtypes = [vp, i, i, C.POINTER(slice_params), C.POINTER(camera_params), C.POINTER(vv_ray_source),
                                             C.POINTER(vv_render_options), i, vp, vp, vp, i, vp]
    lib.vv_slice.argtypes = [vp, vp, sz, sz, f, f, f, i, C.POINTER(f * 3), i, i, i, vp]
    lib.vv_slice_advanced.argtypes = [vp, vp, sz, sz, C.POINTER(f * 16), C.POINTER(f * 3), i, i, vp]
    if hasattr(lib, "vv_slice_slab"):
        lib.vv_slice_slab.argtypes = [vp, vp, vp, sz, sz, f, f, f, i, C.POINTER(f * 3), i, C.POINTER(vv_slab), i, vp]
        lib.vv_slice_advanced_slab.argtypes = [vp, vp, vp, sz, sz, C.POINTER(f * 16), C.POINTER(f * 3), i, C.POINTER(vv_slab), i, vp]
    if hasattr(lib, "vv_volume_histogram"):
        lib.vv_volume_histogram.argtypes = [vp, C.POINTER(i * 3), C.POINTER(i * 3), vp, i, vp]
        lib.vv_histogram_indices.argtypes = [vp, vp, sz, vp, i, vp]
    if hasattr(lib, "vv_derive_volume"):
        lib.vv_derive_dims.argtypes = [vp, C.POINTER(vv_derive), C.POINTER(i * 3)]
        lib.vv_derive_volume.argtypes = [vp, C.POINTER(vv_derive), vp, sz, i, vp]
    if hasattr(lib, "vv_stencil_volume"):
        lib.vv_stencil_volume.argtypes = [vp, C.POINTER(vv_stencil), vp, sz, i, vp]
        lib.vv_stencil_taps.argtypes = [i, i, f, C.POINTER(f * 5)]
    if hasattr(lib, "vv_resample_volume"):
        lib.vv_resample_volume.argtypes = [vp, C.POINTER(vv_resample), vp, sz, i, vp]
        lib.vv_resample_matrix.argtypes = [C.POINTER(f * 3), f, C.POINTER(f * 3), C.POINTER(f * 3), C.POINTER(f * 12)]
    if hasattr(lib, "vv_label_volume"):
        lib.vv_label_volume.argtypes = [vp, C.POINTER(vv_label), vp, sz, vp, vp, i, vp]
        lib.vv_mask_volume.argtypes = [vp, C.POINTER(vv_mask), vp, vp, vp, sz, i, vp]
    if hasattr(lib, "vv_distance_volume"):
        lib.vv_distance_volume.argtypes = [vp, C.POINTER(vv_distance), vp, vp, sz, i, vp]
    if hasattr(lib, "vv_region_table"):
        lib.vv_region_table.argtypes = [vp, C.POINTER(vv_regions), vp, vp, vp, sz, vp, sz, vp, i, vp]
    if hasattr(lib, "vv_surface_mesh"):
        lib.vv_mesh_dims.argtypes = [vp, C.POINTER(vv_mesh), C.POINTER(i * 3)]
        lib.vv_surface_mesh.argtypes = [vp, C.POINTER(vv_mesh), vp, vp, sz, vp, sz, vp, vp, sz, vp, i, vp]
    lib.vv_generate_ellipsoids.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp, vp]
    lib.vv_generate_default_brain.argtypes = [vp, vp, i, i, i, i, vp]
    lib.vv_draw_ellipsoid.argtypes = [vp, vp, i, i, i, i, vp, vp, C.c_uint8, vp]
    lib.vv_promote_u8_to_f32.argtypes = [vp, vp, vp, sz, vp]
    lib.vv_generate_noise_u8.argtypes = [vp, vp, i, i, i, C.c_uint32, vp]
    lib.vv_transfer_preset.argtypes = [i, vp]
    lib.vv_dataset_preset.argtypes = [C.c_char_p, vp, vp]
    lib.vv_t3d_read_header.argtypes = [C.c_char_p, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.vv_t3d_read.argtypes = [C.c_char_p, i, vp, sz]
    lib.vv_t3d_write.argtypes = [C.c_char_p, i, vp, i, i, i]
    lib.vv_last_frame_ms.argtypes = [vp]; lib.vv_last_frame_ms.restype = f
    lib.vv_last_sample_count.argtypes = [vp]; lib.vv_last_sample_count.restype = C.c_ulonglong
    lib.vv_slice_matrix.argtypes = [f, f, f, f, f, f, vp]
    lib.vv_first_pass.argtypes = [vp, i, i, C.POINTER(camera_params), C.POINTER(vv_ray_source), vp, vp, i, vp]
    lib.vv_cut_plane_canonical.argtypes = [i, f, vp, vp]
    lib.vv_cut_plane_from_euler.argtypes = [f, f, f, f, f, f, vp, vp]
    lib.vv_cut_plane_to_slice_params.argtypes = [i, vp, vp, i, C.POINTER(slice_params)]
    lib.vv_slice_to_bgra.argtypes = [vp, sz, sz, vp]
    lib.vv_camera_orbit_drag.argtypes = [vp, i, i, vp, vp]
    lib.vv_camera_zoom.argtypes = [vp, vp, i, vp]
    lib.vv_cut_plane_from_drag.argtypes = [vp, vp, vp, f, vp, vp, vp, vp, vp, vp]
    lib.vv_cut_plane_drag.argtypes = [vp, vp, vp, i, i, i, i]
    lib.vv_debug_counters.argtypes = [vp, vp]
    lib.vv_debug_last_launch.argtypes = [vp, vp]
    if hasattr(lib, "vv_debug_prepass_state"):
        lib.vv_debug_prepass_state.argtypes = [vp, vp]
    if hasattr(lib, "vv_debug_read_layout"):
        lib.vv_debug_read_layout.argtypes = [vp, i, vp, vp, sz]
    lib.vv_set_frame_timing.argtypes = [vp, i]
    lib.vv_debug_screen_rect.argtypes = [i, i, C.POINTER(camera_params), C.POINTER(vv_ray_source), C.POINTER(C.c_double * 4)]
    lib.vv_reread_env.argtypes = [vp]
    lib.vv_prepare_layouts.argtypes = [vp, i, vp]
    lib.vv_device_bytes.argtypes = [vp, vp]
    lib.vv_set_layout_policy.argtypes = [vp, C.c_ulonglong, i]
    lib.vv_layout_state.argtypes = [vp, vp]
    lib.vv_volume_dims.argtypes = [vp, C.POINTER(i * 3), C.POINTER(i)]
    # (the HIP runtime the library links: the working buffers of the composed calls, _DeviceBuffers)
    lib.hipMalloc.argtypes, lib.hipFree.argtypes, lib.hipMemcpy.argtypes = [C.POINTER(vp), sz], [vp], [vp, vp, sz, i]
    for name in EXPORTS:
        if path is not None and name in _NEWER_EXPORTS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        if name not in ("vv_last_error", "vv_last_frame_ms", "vv_last_sample_count"):
            fn.restype = i
    if path is None:
        _lib = lib
    else:
        _libs[path] = lib
    return lib


class VolvizError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"volviz error {code}: {msg}")
        self.code = code


# ---- what the methods of the box-of-the-volume calls share ----
def _set_box(d, box):
    """box = ((x0, y0, z0), (x1, y1, z1)) or None = all of it (the descriptor's six zeros)."""
    if box is not None:
        d.box_lo[:] = [int(v) for v in box[0]]
        d.box_hi[:] = [int(v) for v in box[1]]
    return d


def _set_bins(d, bins):
    """bins = (bin_lo, bin_hi), both inclusive, or one bin."""
    d.bin_lo, d.bin_hi = (int(bins), int(bins)) if np.isscalar(bins) else (int(bins[0]), int(bins[1]))


def _words_like(a, shape, what):
    """`a` as a contiguous uint32 array of the box's `shape` (None stays None); `what`: how the ValueError begins ("labels have")."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.uint32)
    if a.shape != tuple(shape):
        raise ValueError(f"{what} shape {a.shape}, the box has {tuple(shape)}")
    return a


def _prefill(byte, *objs):
    """Every byte of the numpy arrays and ctypes structures `objs` becomes `byte`; a None byte or object is skipped."""
    for o in objs if byte is not None else ():
        if isinstance(o, np.ndarray):
            o.view(np.uint8)[...] = byte
        elif o is not None:
            C.memset(C.byref(o), byte, C.sizeof(o))


def _one_or_tuple(out):
    return out[0] if len(out) == 1 else tuple(out)


class _DeviceBuffers:
    """The working buffers of a composed call (`who`, for the messages), as a context manager: alloc() on demand, upload() and download()
    between them and host arrays, all of them freed on every way out.  VolvizError -4: no memory; -3: a copy failed."""

    def __init__(self, lib, who):
        self.lib, self.who, self.bufs = lib, who, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bufs:
            self.lib.hipFree(p)

    def alloc(self, nbytes, what="a working buffer") -> int:
        p = C.c_void_p()
        if self.lib.hipMalloc(C.byref(p), max(int(nbytes), 8)) != 0 or not p.value:
            raise VolvizError(-4, f"{self.who}: no device memory for {what}")
        self.bufs.append(p)
        return p.value

    def upload(self, dev_ptr, a, what):
        if self.lib.hipMemcpy(dev_ptr, a.ctypes.data, a.nbytes, 1) != 0:
            raise VolvizError(-3, f"{self.who}: the upload of {what} failed")

    def download(self, a, dev_ptr, what):
        if a.nbytes and self.lib.hipMemcpy(a.ctypes.data, dev_ptr, a.nbytes, 2) != 0:
            raise VolvizError(-3, f"{self.who}: the download of {what} failed")
        return a


def transfer_preset(preset: int) -> np.ndarray:
    """vv_transfer_preset: transfer_functions.h:4-9 tables as float32[1024]."""
    tf = np.zeros(1024, np.float32)
    rc = load_library().vv_transfer_preset(preset, tf.ctypes.data)
    if rc:
        raise VolvizError(rc, "bad preset")
    return tf


def dataset_preset(path: str):
    """vv_dataset_preset: (tf_preset, (sx, sy, sz)) by the file name's ending (glwidget.cpp:678-689), or None."""
    tfp = C.c_int(-1)
    sc = (C.c_float * 3)(0, 0, 0)
    rc = load_library().vv_dataset_preset(path.encode(), C.byref(tfp), sc)
    if rc < 0:
        raise VolvizError(rc, "bad argument")
    return (tfp.value, (sc[0], sc[1], sc[2])) if rc == 1 else None


@dataclass
class Camera:
    """The camera surface of glwidget.cpp:113-114,262-276,338-341 + camera.cpp."""
    origin: Sequence[float] = (0.0, 0.0, -4.0)
    look_at: Sequence[float] = (0.0, 0.0, 0.0)
    up: Sequence[float] = (0.0, 1.0, 0.0)
    fov_y: float = 45.0
    scale: Sequence[float] = (1.0, 1.0, 1.0)

    def params(self, width: int, height: int) -> camera_params:
        aspect = np.float32(width) / np.float32(height)
        cp = camera_params()
        cp.origin[:] = [float(v) for v in self.origin]
        cp.fovY = float(self.fov_y)
        cp.fovX = float(np.float32(self.fov_y) * aspect)        # glwidget.cpp:341
        cp.scale[:] = [float(v) for v in self.scale]
        return cp

    def look(self):
        return [float(np.float32(t) - np.float32(o)) for t, o in zip(self.look_at, self.origin)]

    @staticmethod
    def orbit(r: float, theta: float, phi: float, **kw) -> "Camera":
        """glwidget.cpp:435-445 orbit position."""
        return Camera(origin=(r * np.sin(theta) * np.cos(phi), r * np.cos(theta),
                              r * np.sin(theta) * np.sin(phi)), **kw)


def screen_rect(cam: "Camera", width: int, height: int):
    """vv_debug_screen_rect: (x_min, x_max, y_min, y_max) in pixel coordinates, or None when this camera gets no rectangle.  No device needed."""
    out = (C.c_double * 4)()
    cp = cam.params(width, height); rs = analytic_rays(cam)
    rc = load_library().vv_debug_screen_rect(width, height, C.byref(cp), C.byref(rs), C.byref(out))
    if rc < 0:
        raise VolvizError(rc, "vv_debug_screen_rect")
    return tuple(out) if rc == 1 else None


def analytic_rays(cam: Camera, quantize8: bool = False, aspect: float = 0.0) -> vv_ray_source:
    rs = vv_ray_source()
    rs.mode = RAYS_ANALYTIC
    rs.look[:] = cam.look()
    rs.up[:] = [float(v) for v in cam.up]
    rs.aspect = aspect
    rs.quantize8 = int(quantize8)
    return rs


def _hint(rs: vv_ray_source, cam: Optional["Camera"], aspect: float) -> vv_ray_source:
    if cam is not None:                     # the camera that drew the images: a launch-policy hint (include/volviz.h)
        rs.look[:] = cam.look()
        rs.up[:] = [float(v) for v in cam.up]
        rs.aspect = aspect
    return rs


def image_rays(front: np.ndarray, back: np.ndarray, hint: Optional["Camera"] = None, aspect: float = 0.0) -> vv_ray_source:
    """front/back: uint8 [H_fbo, W_fbo, 4] host arrays (kept alive by the caller)."""
    assert front.dtype == np.uint8 and back.dtype == np.uint8 and front.shape == back.shape
    rs = vv_ray_source()
    rs.mode = RAYS_IMAGES
    rs.front = front.ctypes.data
    rs.back = back.ctypes.data
    rs.img_h, rs.img_w = front.shape[0], front.shape[1]
    rs.images_on_device = 0
    return _hint(rs, hint, aspect)


def device_image_rays(front_ptr: int, back_ptr: int, img_w: int, img_h: int, hint: Optional["Camera"] = None, aspect: float = 0.0) -> vv_ray_source:
    """Two device-resident RGBA8 images (e.g. written by Context.first_pass_device)."""
    rs = vv_ray_source()
    rs.mode = RAYS_IMAGES
    rs.front = front_ptr
    rs.back = back_ptr
    rs.img_h, rs.img_w = img_h, img_w
    rs.images_on_device = 1
    return _hint(rs, hint, aspect)


def make_slice_params(slice_type: int = SLICE_NONE, point=(0.5, 0.5, 0.5), normal=(0.0, 0.0, 1.0)) -> slice_params:
    sp = slice_params()
    sp.type = slice_type
    sp.params[:] = [float(v) for v in (*point, *normal)]
    return sp


def make_options(step=None, ert_threshold=0.0, filter=FILTER_TEX8, ert_mode=ERT_REFERENCE,
                 slab_rows=(0, 0), shard=None, count_samples=False, touched_bricks=0, touched_lines=0, touched_line_bits=0,
                 touched_lines_all=False, touched_block_lines=0, touched_block_lines_log2=0) -> vv_render_options:
    o = vv_render_options()
    if step is not None:
        s = [step] * 3 if np.isscalar(step) else list(step)
        o.step[:] = [float(v) for v in s]
    o.ert_threshold = ert_threshold
    o.filter = filter
    o.ert_mode = ert_mode
    o.slab_row_begin, o.slab_row_end = slab_rows
    if shard is not None:                       # (band, count, index)
        o.shard_band, o.shard_count, o.shard_index = shard
    o.count_samples = int(count_samples)
    o.touched_bricks = touched_bricks
    o.touched_lines = touched_lines
    o.touched_line_bits = touched_line_bits
    o.touched_lines_all = int(touched_lines_all)
    o.touched_block_lines = touched_block_lines
    o.touched_block_lines_log2 = touched_block_lines_log2
    return o


class Context:
    """One vv_context: one device, one volume, one transfer function (kernel.cu:35-51)."""

    def __init__(self, device: int = -1, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.vv_init(device, C.byref(h))
        if rc:
            raise VolvizError(rc, (self.lib.vv_last_error(None) or b"").decode())
        self.h = h

    def _chk(self, rc: int):
        if rc:
            raise VolvizError(rc, (self.lib.vv_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.vv_shutdown(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # cudaLoadVolume (kernel.cu:456-498)
    def load_volume(self, vol: np.ndarray, tf: np.ndarray):
        """vol: [nz, ny, nx] uint8 or float32 (x fastest); tf: float32[1024]."""
        assert vol.ndim == 3 and vol.flags.c_contiguous
        tf = np.ascontiguousarray(tf, np.float32).reshape(1024)
        nz, ny, nx = vol.shape
        if vol.dtype == np.uint8:
            self._chk(self.lib.vv_load_volume_u8(self.h, vol.ctypes.data, vol.nbytes, nx, ny, nz, tf.ctypes.data))
        elif vol.dtype == np.float32:
            self._chk(self.lib.vv_load_volume_f32(self.h, vol.ctypes.data, vol.nbytes, nx, ny, nz, tf.ctypes.data))
        else:
            raise TypeError("volume must be uint8 or float32")

    def load_volume_device(self, dev_ptr: int, voxel_type: int, nx: int, ny: int, nz: int, tf: np.ndarray, stream: int = 0):
        tf = np.ascontiguousarray(tf, np.float32).reshape(1024)
        self._chk(self.lib.vv_load_volume_device(self.h, dev_ptr, voxel_type, nx, ny, nz, tf.ctypes.data, stream))

    def load_volume_streamed(self, slabs, voxel_type: int, nx: int, ny: int, nz: int, tf: np.ndarray):
        """vv_load_volume_stream_*: `slabs` yields (z0, array[nslices, ny, nx]) in any order; u8 slabs
        into an f32 volume are promoted on the device."""
        tf = np.ascontiguousarray(tf, np.float32).reshape(1024)
        self._chk(self.lib.vv_load_volume_stream_begin(self.h, voxel_type, nx, ny, nz, tf.ctypes.data))
        for z0, arr in slabs:
            arr = np.ascontiguousarray(arr)
            st = VOXEL_U8 if arr.dtype == np.uint8 else VOXEL_F32
            self._chk(self.lib.vv_load_volume_stream_slices(self.h, arr.ctypes.data, st, z0, arr.shape[0]))
        self._chk(self.lib.vv_load_volume_stream_end(self.h))

    def load_volume_t3d(self, path: str, header: bool, voxel_type: int, tf: np.ndarray):
        tf = np.ascontiguousarray(tf, np.float32).reshape(1024)
        self._chk(self.lib.vv_load_volume_t3d(self.h, path.encode(), int(header), voxel_type, tf.ctypes.data))

    def set_transfer_function(self, tf: np.ndarray):
        tf = np.ascontiguousarray(tf, np.float32).reshape(1024)
        self._chk(self.lib.vv_set_transfer_function(self.h, tf.ctypes.data))

    @staticmethod
    def _frame_args(width, height, cam, slice, rays, options, shading=None):
        """The leading arguments of a vv_render* call after (context, W, H): slice, camera, [shading,] ray source, options."""
        sp = slice if slice is not None else make_slice_params()
        rs = rays if rays is not None else analytic_rays(cam)
        return ((C.byref(sp), C.byref(cam.params(width, height))) + ((C.byref(shading),) if shading is not None else ()) +
                (C.byref(rs), C.byref(options) if options is not None else None))

    @staticmethod
    def _host_images(width, height, fill, *extra):
        """The host images of a frame, every byte `fill`: rgba uint8 [H, W, 4] and one per (wanted, bytes of a pixel as a shape, dtype) of `extra`.
        Returns their addresses (None where not wanted) and what the render method returns: the rgba image, or a tuple with the wanted others behind it."""
        imgs = [np.full((height, width, 4), fill, np.uint8)]
        imgs += [np.full((height, width) + px, fill, np.uint8).view(dtype) if wanted else None for wanted, px, dtype in extra]
        res = tuple(i for i in imgs if i is not None)
        return [None if i is None else i.ctypes.data for i in imgs], res if len(res) > 1 else res[0]

    # runCuda (kernel.cu:388-453)
    def render(self, width: int, height: int, cam: Camera, *, slice: Optional[slice_params] = None,
               phong: bool = False, rays: Optional[vv_ray_source] = None,
               options: Optional[vv_render_options] = None, out: Optional[np.ndarray] = None,
               fill: int = 0) -> np.ndarray:
        """Host-buffer render; returns uint8 [H, W, 4] (row 0 = bottom)."""
        if out is None:
            _, out = self._host_images(width, height, fill)
        args = self._frame_args(width, height, cam, slice, rays, options, shading_params(-1, phong))
        self._chk(self.lib.vv_render(self.h, width, height, *args, out.ctypes.data, 0, None))
        return out

    def render_device(self, width: int, height: int, cam: Camera, out_ptr: int, *, slice=None, phong=False,
                      rays=None, options=None, stream: int = 0):
        """Device-buffer render enqueued on `stream` (a hipStream_t as int)."""
        args = self._frame_args(width, height, cam, slice, rays, options, shading_params(-1, phong))
        self._chk(self.lib.vv_render(self.h, width, height, *args, out_ptr, 1, stream))

    # vv_render_mip / vv_classify_indices (no reference counterpart)
    def render_mip(self, width: int, height: int, cam: Camera, *, slice: Optional[slice_params] = None,
                   rays: Optional[vv_ray_source] = None, options: Optional[vv_render_options] = None,
                   fill: int = 0, return_index: bool = False):
        """Host-buffer maximum-intensity projection; returns rgba uint8 [H, W, 4] (row 0 = bottom), or (rgba, index uint8 [H, W])
        with return_index.  Pixels the frame does not write keep `fill` in both images."""
        ptrs, res = self._host_images(width, height, fill, (return_index, (), np.uint8))
        self._chk(self.lib.vv_render_mip(self.h, width, height, *self._frame_args(width, height, cam, slice, rays, options), *ptrs, 0, None))
        return res

    def render_mip_device(self, width: int, height: int, cam: Camera, rgba_ptr: int = 0, index_ptr: int = 0, *, slice=None,
                          rays=None, options=None, stream: int = 0):
        """Device-buffer MIP frame enqueued on `stream` (a hipStream_t as int): rgba_ptr (W*H*4 bytes) and / or index_ptr (W*H bytes), 0 = not wanted."""
        self._chk(self.lib.vv_render_mip(self.h, width, height, *self._frame_args(width, height, cam, slice, rays, options),
                                         rgba_ptr or None, index_ptr or None, 1, stream))

    # vv_render_iso (no reference counterpart)
    def render_iso(self, width: int, height: int, cam: Camera, level: int, *, slice: Optional[slice_params] = None,
                   rays: Optional[vv_ray_source] = None, options: Optional[vv_render_options] = None,
                   fill: int = 0, return_index: bool = False, return_hit: bool = False):
        """Host-buffer isosurface frame at `level` (1..255); returns rgba uint8 [H, W, 4] (row 0 = bottom), or a tuple with index uint8 [H, W]
        (return_index) and hit float32 [H, W, 4] = (x, y, z, ordinal) (return_hit) behind it.  Pixels the frame does not write keep `fill` in
        every byte of all images (the float image's bytes too)."""
        ptrs, res = self._host_images(width, height, fill, (return_index, (), np.uint8), (return_hit, (16,), np.float32))
        self._chk(self.lib.vv_render_iso(self.h, width, height, *self._frame_args(width, height, cam, slice, rays, options), int(level), *ptrs, 0, None))
        return res

    def render_iso_device(self, width: int, height: int, cam: Camera, level: int, rgba_ptr: int = 0, index_ptr: int = 0, hit_ptr: int = 0, *,
                          slice=None, rays=None, options=None, stream: int = 0):
        """Device-buffer isosurface frame enqueued on `stream` (a hipStream_t as int): rgba_ptr (W*H*4 bytes), index_ptr (W*H bytes) and / or
        hit_ptr (W*H*16 bytes, 16-byte aligned), 0 = not wanted."""
        self._chk(self.lib.vv_render_iso(self.h, width, height, *self._frame_args(width, height, cam, slice, rays, options), int(level),
                                         rgba_ptr or None, index_ptr or None, hit_ptr or None, 1, stream))

    # vv_render_projection (no reference counterpart)
    def render_projection(self, width: int, height: int, cam: Camera, mode: int, *, slice: Optional[slice_params] = None,
                          rays: Optional[vv_ray_source] = None, options: Optional[vv_render_options] = None,
                          fill: int = 0, return_index: bool = False, return_stat: bool = False):
        """Host-buffer projection frame, mode PROJ_MAX / PROJ_MIN / PROJ_MEAN over the samples inside the volume; returns rgba uint8 [H, W, 4]
        (row 0 = bottom), or a tuple with index uint8 [H, W] (return_index) and stat uint32 [H, W, 2] (return_stat) behind it: (ordinal of the
        extremum among the ray's executed samples, counted samples) for PROJ_MAX / PROJ_MIN, (sum, counted samples) for PROJ_MEAN.  Pixels the
        frame does not write keep `fill` in every byte of all images."""
        ptrs, res = self._host_images(width, height, fill, (return_index, (), np.uint8), (return_stat, (8,), np.uint32))
        self._chk(self.lib.vv_render_projection(self.h, width, height, *self._frame_args(width, height, cam, slice, rays, options), int(mode), *ptrs, 0, None))
        return res

    def render_projection_device(self, width: int, height: int, cam: Camera, mode: int, rgba_ptr: int = 0, index_ptr: int = 0, stat_ptr: int = 0, *,
                                 slice=None, rays=None, options=None, stream: int = 0):
        """Device-buffer projection frame enqueued on `stream` (a hipStream_t as int): rgba_ptr (W*H*4 bytes), index_ptr (W*H bytes) and / or
        stat_ptr (W*H*8 bytes, 8-byte aligned), 0 = not wanted."""
        self._chk(self.lib.vv_render_projection(self.h, width, height, *self._frame_args(width, height, cam, slice, rays, options), int(mode),
                                                rgba_ptr or None, index_ptr or None, stat_ptr or None, 1, stream))

    def classify_indices(self, index: np.ndarray, tf: Optional[np.ndarray] = None) -> np.ndarray:
        """vv_classify_indices on a host index image (uint8, any shape): uint8 [..., 4] through `tf` (float32[1024]) or the context's table."""
        index = np.ascontiguousarray(index, np.uint8)
        out = np.zeros(index.shape + (4,), np.uint8)
        t = None if tf is None else np.ascontiguousarray(tf, np.float32).reshape(1024)
        self._chk(self.lib.vv_classify_indices(self.h, index.ctypes.data, index.size, None if t is None else t.ctypes.data,
                                               out.ctypes.data, 0, None))
        return out

    def classify_indices_device(self, index_ptr: int, n: int, rgba_ptr: int, tf: Optional[np.ndarray] = None, stream: int = 0):
        """vv_classify_indices on device buffers (n index bytes -> n * 4 RGBA bytes), enqueued on `stream`."""
        t = None if tf is None else np.ascontiguousarray(tf, np.float32).reshape(1024)
        self._chk(self.lib.vv_classify_indices(self.h, index_ptr, n, None if t is None else t.ctypes.data, rgba_ptr, 1, stream))

    def first_pass(self, img_w: int, img_h: int, cam: Camera):
        """vv_first_pass: the two RGBA8 FBO images of glwidget.cpp:200-228 for this camera."""
        front = np.zeros((img_h, img_w, 4), np.uint8); back = np.zeros((img_h, img_w, 4), np.uint8)
        cp = cam.params(img_w, img_h); rs = analytic_rays(cam)
        self._chk(self.lib.vv_first_pass(self.h, img_w, img_h, C.byref(cp), C.byref(rs), front.ctypes.data, back.ctypes.data, 0, None))
        return front, back

    def first_pass_device(self, img_w: int, img_h: int, cam: Camera, front_ptr: int, back_ptr: int, stream: int = 0):
        """vv_first_pass into two device buffers of img_w * img_h * 4 bytes, enqueued on `stream`."""
        cp = cam.params(img_w, img_h); rs = analytic_rays(cam)
        self._chk(self.lib.vv_first_pass(self.h, img_w, img_h, C.byref(cp), C.byref(rs), front_ptr, back_ptr, 1, stream))

    def last_frame_ms(self) -> float:
        return float(self.lib.vv_last_frame_ms(self.h))

    def set_frame_timing(self, on: bool) -> None:
        """vv_set_frame_timing: the two hipEventRecord per vv_render behind last_frame_ms(), on (default) or off."""
        self._chk(self.lib.vv_set_frame_timing(self.h, int(bool(on))))

    def debug_counters(self):
        out = np.zeros(16, np.uint64)
        self._chk(self.lib.vv_debug_counters(self.h, out.ctypes.data))
        return out

    def last_launch(self) -> dict:
        """vv_debug_last_launch: what the launch policy chose for the last render."""
        out = (C.c_int * 8)()
        self._chk(self.lib.vv_debug_last_launch(self.h, out))
        k = ("tile_log2w", "blk_log2w", "unroll", "lds_reserve", "layout", "view_known", "density_x1000", "phong")     # phong: 0 unshaded, 1 Phong, 2 MIP, 3 isosurface, 4 projection
        return dict(zip(k, list(out)))

    def prepass_state(self) -> tuple:
        """vv_debug_prepass_state: (radius pre-passes launched since the context was created, frames that reused the last one's results, whether the
        last frame did, the fill blocks of the last frame's march launch)."""
        out = (C.c_int * 4)()
        self._chk(self.lib.vv_debug_prepass_state(self.h, out))
        return tuple(out)

    def read_layout(self, code: int):
        """vv_debug_read_layout: the resident layout `code` (last_launch()["layout"]'s codes) as it lies in HBM: (uint8 array of the whole allocation,
        the zeroed bytes behind the layout included; dict of its geometry).  The array is empty and alloc_bytes 0 when the layout is not resident."""
        geom = np.zeros(8, np.uint64)
        self._chk(self.lib.vv_debug_read_layout(self.h, int(code), geom.ctypes.data, None, 0))
        raw = np.zeros(int(geom[0]), np.uint8)
        if raw.size:
            self._chk(self.lib.vv_debug_read_layout(self.h, int(code), geom.ctypes.data, raw.ctypes.data, raw.size))
        k = ("alloc_bytes", "row", "slice", "nx", "ny", "nz", "voxel_type")   # row / slice: the layout's two VolumeView strides (bricked: slice in 64-byte units)
        return raw, dict(zip(k, (int(v) for v in geom)))

    def reread_env(self):
        """vv_reread_env: pick up VV_* knobs changed since the last volume load."""
        self._chk(self.lib.vv_reread_env(self.h))

    def last_sample_count(self) -> int:
        return int(self.lib.vv_last_sample_count(self.h))

    def prepare_layouts(self, which: int = 3, stream=None) -> int:
        """vv_prepare_layouts: build the bricked (1) / z-pair (2) / z-fastest (4, with the x-pair copy) copies now, or LAYOUT_POLICY = every copy
        the launch policy can pick for the loaded volume; returns the resident mask."""
        rc = self.lib.vv_prepare_layouts(self.h, which, stream)
        if rc < 0:
            self._chk(rc)
        return rc

    def set_layout_policy(self, budget_bytes: int = 0, build_in_render: bool = True):
        """vv_set_layout_policy: HBM budget of the optional copies (0 = default) and whether vv_render may build a missing one."""
        self._chk(self.lib.vv_set_layout_policy(self.h, int(budget_bytes), int(build_in_render)))

    def layout_state(self) -> dict:
        """vv_layout_state: resident bytes per layout, the budget, copies built inside vv_render since the load."""
        out = np.zeros(8, np.uint64)
        self._chk(self.lib.vv_layout_state(self.h, out.ctypes.data))
        k = ("linear", "bricked", "zpair", "zfast", "xpair", "budget", "builds_in_render", "build_in_render")
        return dict(zip(k, (int(v) for v in out)))

    def device_bytes(self):
        """vv_device_bytes: [linear volume, bricked copy, z-pair + z-fastest copies, tables + scratch]."""
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.vv_device_bytes(self.h, out.ctypes.data))
        return [int(v) for v in out]

    # invoke_slice_kernel (kernel.cu:506-519) / slicekernel.cu legacy
    def slice(self, height: int, width: int, dx=0.0, dy=0.0, dz=0.0, orientation=SAGITTAL,
              scale=(1.0, 1.0, 1.0), legacy=False, filter=FILTER_TEX8, fill=0.0) -> np.ndarray:
        buf = np.full(height * width, fill, np.float32)
        sc = (C.c_float * 3)(*[float(v) for v in scale])
        self._chk(self.lib.vv_slice(self.h, buf.ctypes.data, height, width, dx, dy, dz, orientation,
                                    C.byref(sc), int(legacy), filter, 0, None))
        return buf

    # invoke_advanced_slice_kernel (kernel.cu:522-541)
    def slice_advanced(self, height: int, width: int, trans: np.ndarray, scale=(1.0, 1.0, 1.0),
                       filter=FILTER_TEX8, fill=0.0) -> np.ndarray:
        buf = np.full(height * width, fill, np.float32)
        t = (C.c_float * 16)(*[float(v) for v in np.asarray(trans, np.float32).reshape(16)])
        sc = (C.c_float * 3)(*[float(v) for v in scale])
        self._chk(self.lib.vv_slice_advanced(self.h, buf.ctypes.data, height, width, C.byref(t), C.byref(sc),
                                             filter, 0, None))
        return buf

    # vv_slice_slab / vv_slice_advanced_slab: the maximum, minimum or mean over `samples` slices across `thickness`
    def slice_slab(self, height: int, width: int, dx=0.0, dy=0.0, dz=0.0, orientation=SAGITTAL, *, mode=SLAB_MAX, samples=1,
                   thickness=0.0, scale=(1.0, 1.0, 1.0), filter=FILTER_TEX8, fill=0.0, return_aux=False, aux_fill=-7):
        """The float32 buffer, or (buffer, aux int32): aux = the extremum's sample (MAX, MIN; -1: none) or the number of
        executed samples (MEAN).  Elements the kernel does not write hold `fill` / `aux_fill`."""
        buf = np.full(height * width, fill, np.float32)
        aux = np.full(height * width, aux_fill, np.int32) if return_aux else None
        self.slice_slab_device(height, width, dx, dy, dz, orientation, buf.ctypes.data, aux.ctypes.data if return_aux else 0,
                               mode=mode, samples=samples, thickness=thickness, scale=scale, filter=filter, stream=None, on_device=False)
        return (buf, aux) if return_aux else buf

    def slice_advanced_slab(self, height: int, width: int, trans: np.ndarray, *, mode=SLAB_MAX, samples=1, thickness=0.0,
                            scale=(1.0, 1.0, 1.0), filter=FILTER_TEX8, fill=0.0, return_aux=False, aux_fill=-7):
        buf = np.full(height * width, fill, np.float32)
        aux = np.full(height * width, aux_fill, np.int32) if return_aux else None
        self.slice_advanced_slab_device(height, width, trans, buf.ctypes.data, aux.ctypes.data if return_aux else 0,
                                        mode=mode, samples=samples, thickness=thickness, scale=scale, filter=filter, stream=None, on_device=False)
        return (buf, aux) if return_aux else buf

    def slice_slab_device(self, height: int, width: int, dx, dy, dz, orientation, buffer_ptr: int, aux_ptr: int = 0, *, mode=SLAB_MAX,
                          samples=1, thickness=0.0, scale=(1.0, 1.0, 1.0), filter=FILTER_TEX8, stream=0, on_device=True):
        """Device pointers (height * width float32, and int32 or 0); with a stream the call only enqueues."""
        sc = (C.c_float * 3)(*[float(v) for v in scale])
        sl = vv_slab(int(mode), int(samples), float(thickness))
        self._chk(self.lib.vv_slice_slab(self.h, buffer_ptr or None, aux_ptr or None, height, width, dx, dy, dz, orientation, C.byref(sc),
                                         filter, C.byref(sl), int(on_device), stream or None))

    def slice_advanced_slab_device(self, height: int, width: int, trans, buffer_ptr: int, aux_ptr: int = 0, *, mode=SLAB_MAX, samples=1,
                                   thickness=0.0, scale=(1.0, 1.0, 1.0), filter=FILTER_TEX8, stream=0, on_device=True):
        t = (C.c_float * 16)(*[float(v) for v in np.asarray(trans, np.float32).reshape(16)])
        sc = (C.c_float * 3)(*[float(v) for v in scale])
        sl = vv_slab(int(mode), int(samples), float(thickness))
        self._chk(self.lib.vv_slice_advanced_slab(self.h, buffer_ptr or None, aux_ptr or None, height, width, C.byref(t), C.byref(sc),
                                                  filter, C.byref(sl), int(on_device), stream or None))

    # vv_volume_histogram / vv_histogram_indices (no reference counterpart)
    @staticmethod
    def _box(box):
        if box is None:
            return None, None
        (x0, y0, z0), (x1, y1, z1) = box
        return C.byref((C.c_int * 3)(int(x0), int(y0), int(z0))), C.byref((C.c_int * 3)(int(x1), int(y1), int(z1)))

    def histogram(self, box=None, prefill: int = 0) -> Histogram:
        """vv_volume_histogram of the loaded volume, or of box = ((x0, y0, z0), (x1, y1, z1)), lo inclusive, hi exclusive, in voxels.
        `prefill`: the byte the output structure holds before the call (the result does not depend on it)."""
        out = vv_histogram()
        _prefill(prefill, out)
        lo, hi = self._box(box)
        self._chk(self.lib.vv_volume_histogram(self.h, lo, hi, C.addressof(out), 0, None))
        return Histogram.from_bytes(out)

    def histogram_device(self, out_ptr: int, box=None, stream: int = 0):
        """vv_volume_histogram into a device vv_histogram (2072 bytes, 8-byte aligned), enqueued on `stream`."""
        lo, hi = self._box(box)
        self._chk(self.lib.vv_volume_histogram(self.h, lo, hi, out_ptr or None, 1, stream or None))

    def histogram_indices(self, index: np.ndarray) -> np.ndarray:
        """vv_histogram_indices of a host index image (uint8, any shape): uint64[256]."""
        index = np.ascontiguousarray(index, np.uint8)
        counts = np.full(256, 0xA5A5A5A5A5A5A5A5, np.uint64)
        self._chk(self.lib.vv_histogram_indices(self.h, index.ctypes.data if index.size else None, index.size, counts.ctypes.data, 0, None))
        return counts

    def histogram_indices_device(self, index_ptr: int, n: int, counts_ptr: int, stream: int = 0):
        """vv_histogram_indices on device buffers (n index bytes -> 256 uint64, 8-byte aligned), enqueued on `stream`."""
        self._chk(self.lib.vv_histogram_indices(self.h, index_ptr or None, n, counts_ptr or None, 1, stream or None))

    # vv_derive_dims / vv_derive_volume (no reference counterpart)
    def volume_type(self) -> int:
        """The loaded volume's voxel type (vv_volume_dims)."""
        dims, vt = (C.c_int * 3)(), C.c_int()
        self._chk(self.lib.vv_volume_dims(self.h, C.byref(dims), C.byref(vt)))
        return int(vt.value)

    # what the volume-to-volume calls share: the descriptor's box and output type, the output's extents, the host and the device call
    def _box_and_type(self, d, box, out_type):
        """box = ((x0, y0, z0), (x1, y1, z1)) or None = all of it (six zeros); out_type None = the volume's type."""
        _set_box(d, box)
        d.out_type = self.volume_type() if out_type is None else int(out_type)
        return d

    def _out_dims(self, d, whole=None):
        """(bx, by, bz) of the descriptor's box; `whole`: what six zeros stand for (None: the loaded volume's extents)."""
        if any(d.box_lo) or any(d.box_hi):
            return tuple(max(int(h) - int(l), 0) for l, h in zip(d.box_lo, d.box_hi))
        if whole is None:
            whole = (C.c_int * 3)()
            self._chk(self.lib.vv_volume_dims(self.h, C.byref(whole), None))
        return int(whole[0]), int(whole[1]), int(whole[2])

    def _volume_to_host(self, call, d, dims, prefill) -> np.ndarray:
        """`call` (a vv_*_volume) into a new host array [bz, by, bx] of the descriptor's out_type, prefilled with the byte `prefill` unless None."""
        out = np.empty(tuple(dims)[::-1], np.float32 if d.out_type == VOXEL_F32 else np.uint8)
        _prefill(prefill, out)
        self._chk(call(self.h, C.byref(d), out.ctypes.data if out.size else None, out.nbytes, 0, None))
        return out

    def _volume_to_device(self, call, d, out_ptr, capacity, stream):
        self._chk(call(self.h, C.byref(d), out_ptr or None, int(capacity), 1, stream or None))

    def _derive(self, box, factor, mode, out_type, window) -> vv_derive:
        """box and out_type as _box_and_type; factor: an int or (fx, fy, fz); window = (win_lo, win_hi) or None."""
        d = self._box_and_type(vv_derive(), box, out_type)
        d.factor[:] = [int(factor)] * 3 if np.isscalar(factor) else [int(v) for v in factor]
        d.mode = int(mode)
        if window is not None:
            d.window, d.win_lo, d.win_hi = 1, float(window[0]), float(window[1])
        return d

    def derive_dims(self, box=None, factor=1):
        """vv_derive_dims: (mx, my, mz) of the volume derive() makes of this box and factor."""
        return self._derive_dims(self._derive(box, factor, REDUCE_MEAN, VOXEL_U8, None))

    def _derive_dims(self, d: vv_derive):
        m = (C.c_int * 3)()
        self._chk(self.lib.vv_derive_dims(self.h, C.byref(d), C.byref(m)))
        return int(m[0]), int(m[1]), int(m[2])

    def derive(self, box=None, factor=1, mode=REDUCE_MEAN, out_type=None, window=None, prefill=None) -> np.ndarray:
        """vv_derive_volume into a host array [mz, my, mx] of uint8 or float32.  `prefill`: the byte the buffer holds before the call (the
        result does not depend on it)."""
        d = self._derive(box, factor, mode, out_type, window)
        return self._volume_to_host(self.lib.vv_derive_volume, d, self._derive_dims(d), prefill)

    def derive_device(self, out_ptr: int, capacity: int, box=None, factor=1, mode=REDUCE_MEAN, out_type=None, window=None, stream: int = 0):
        """vv_derive_volume into a device buffer of `capacity` bytes, enqueued on `stream`; returns (mx, my, mz)."""
        d = self._derive(box, factor, mode, out_type, window)
        m = self._derive_dims(d)
        self._volume_to_device(self.lib.vv_derive_volume, d, out_ptr, capacity, stream)
        return m

    # vv_stencil_volume (no reference counterpart)
    def _stencil(self, kind, box, out_type, radius, taps, gscale) -> vv_stencil:
        """box and out_type as _box_and_type; radius: an int or (rx, ry, rz); taps: None, one row of up to 5 taps for all three axes, or three rows
        (x, y, z), taps[a][0] the centre; gscale: None (= (1, 1, 1)) or three multipliers."""
        d = self._box_and_type(vv_stencil(), box, out_type)
        d.kind = int(kind)
        d.radius[:] = [int(radius)] * 3 if np.isscalar(radius) else [int(v) for v in radius]
        if taps is not None:
            t = np.asarray(taps, np.float32)
            rows = [t, t, t] if t.ndim == 1 else list(t)
            for a in range(3):
                for k, v in enumerate(np.asarray(rows[a], np.float32)[:5]):
                    d.taps[a][k] = float(v)
        if gscale is not None:
            d.gscale[:] = [float(v) for v in gscale]
        return d

    def stencil(self, kind, box=None, out_type=None, radius=(0, 0, 0), taps=None, gscale=None, prefill=None) -> np.ndarray:
        """vv_stencil_volume into a host array [bz, by, bx] of uint8 or float32 (the box's extents).  `prefill`: the byte the buffer holds before
        the call (the result does not depend on it)."""
        d = self._stencil(kind, box, out_type, radius, taps, gscale)
        return self._volume_to_host(self.lib.vv_stencil_volume, d, self._out_dims(d), prefill)

    def stencil_device(self, out_ptr: int, capacity: int, kind, box=None, out_type=None, radius=(0, 0, 0), taps=None, gscale=None, stream: int = 0):
        """vv_stencil_volume into a device buffer of `capacity` bytes, enqueued on `stream`; returns the output's (bx, by, bz)."""
        d = self._stencil(kind, box, out_type, radius, taps, gscale)
        self._volume_to_device(self.lib.vv_stencil_volume, d, out_ptr, capacity, stream)
        return self._out_dims(d)

    def smooth(self, radius=1, shape=TAPS_BINOMIAL, sigma=0.0, box=None, out_type=None) -> np.ndarray:
        """The volume (or a box of it) smoothed with stencil_taps(shape, r, sigma) on every axis; radius: an int or (rx, ry, rz)."""
        r = [int(radius)] * 3 if np.isscalar(radius) else [int(v) for v in radius]
        return self.stencil(STENCIL_SEPARABLE, box, out_type, r, [stencil_taps(shape, v, sigma) for v in r])

    def median(self, box=None, out_type=None) -> np.ndarray:
        """The 3x3x3 median of the volume (or of a box of it)."""
        return self.stencil(STENCIL_MEDIAN, box, out_type)

    def gradient_magnitude(self, gscale=None, box=None, out_type=None) -> np.ndarray:
        """The magnitude of the central-difference gradient, each axis multiplied by gscale[a] first."""
        return self.stencil(STENCIL_GRADMAG, box, out_type, gscale=gscale)

    # vv_resample_volume (no reference counterpart)
    def _resample(self, dims, matrix, filter, fill, out_type, box) -> vv_resample:
        """dims = (mx, my, mz) of the output grid; matrix: 12 floats (row-major 3 x 4) or None = the identity; box = ((x0, y0, z0), (x1, y1, z1))
        of the output grid or None = the whole grid; out_type None = the volume's type."""
        d = vv_resample()
        d.dims[:] = [int(v) for v in dims]
        self._box_and_type(d, box, out_type)
        d.filter = int(filter)
        m = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0) if matrix is None else np.asarray(matrix, np.float32).reshape(12)
        d.m[:] = [float(v) for v in m]
        d.fill = float(fill)
        return d

    def resample(self, dims, matrix=None, filter=RESAMPLE_TEX8, fill=0.0, out_type=None, box=None, prefill=None) -> np.ndarray:
        """vv_resample_volume into a host array [bz, by, bx] of uint8 or float32 (the box's extents).  `prefill`: the byte the buffer holds before
        the call (the result does not depend on it)."""
        d = self._resample(dims, matrix, filter, fill, out_type, box)
        return self._volume_to_host(self.lib.vv_resample_volume, d, self._out_dims(d, d.dims), prefill)

    def resample_device(self, out_ptr: int, capacity: int, dims, matrix=None, filter=RESAMPLE_TEX8, fill=0.0, out_type=None, box=None, stream: int = 0):
        """vv_resample_volume into a device buffer of `capacity` bytes, enqueued on `stream`; returns the output's (bx, by, bz)."""
        d = self._resample(dims, matrix, filter, fill, out_type, box)
        self._volume_to_device(self.lib.vv_resample_volume, d, out_ptr, capacity, stream)
        return self._out_dims(d, d.dims)

    # vv_label_volume / vv_mask_volume (no reference counterpart)
    def _label(self, bins, connectivity, box) -> vv_label:
        """bins = (bin_lo, bin_hi), both inclusive, or one bin; box = ((x0, y0, z0), (x1, y1, z1)) or None = the whole volume."""
        d = _set_box(vv_label(), box)
        _set_bins(d, bins)
        d.connectivity = int(connectivity)
        return d

    def label(self, bins, connectivity=6, box=None, sizes=False, stats=False, prefill=None):
        """vv_label_volume into host arrays: labels [bz, by, bx] uint32; with `sizes` also the sizes array of the same shape; with `stats` also
        a LabelStats (in that order, as a tuple).  `prefill`: the byte the outputs hold before the call (the result does not depend on it)."""
        d = self._label(bins, connectivity, box)
        shape = self._out_dims(d)[::-1]
        labels = np.empty(shape, np.uint32)
        size_arr = np.empty(shape, np.uint32) if sizes else None
        st = vv_label_stats() if stats else None
        _prefill(prefill, labels, size_arr, st)
        self._chk(self.lib.vv_label_volume(self.h, C.byref(d), labels.ctypes.data if labels.size else None, labels.nbytes,
                                           size_arr.ctypes.data if sizes else None, C.addressof(st) if stats else None, 0, None))
        return _one_or_tuple([labels] + ([size_arr] if sizes else []) + ([LabelStats.from_bytes(st)] if stats else []))

    def label_device(self, labels_ptr: int, capacity: int, bins, connectivity=6, box=None, sizes_ptr: int = 0, stats_ptr: int = 0, stream: int = 0):
        """vv_label_volume into device buffers (labels and sizes: `capacity` bytes each, 4-byte aligned; stats: 32 bytes, 8-byte aligned),
        enqueued on `stream`; returns the box's (bx, by, bz)."""
        d = self._label(bins, connectivity, box)
        self._chk(self.lib.vv_label_volume(self.h, C.byref(d), labels_ptr or None, int(capacity), sizes_ptr or None, stats_ptr or None, 1, stream or None))
        return self._out_dims(d)

    def _mask(self, keep, label, min_size, invert, fill, box, out_type) -> vv_mask:
        d = self._box_and_type(vv_mask(), box, out_type)
        d.keep, d.invert, d.label, d.min_size, d.fill = int(keep), int(bool(invert)), int(label), int(min_size), float(fill)
        return d

    def mask(self, labels: np.ndarray, keep=KEEP_FOREGROUND, label=0, min_size=0, sizes=None, invert=False, fill=0.0, box=None, out_type=None,
             prefill=None) -> np.ndarray:
        """vv_mask_volume with host labels (and sizes) [bz, by, bx] uint32 into a host array of the same shape, uint8 or float32: the volume's
        voxels where the test on the labels holds, `fill` elsewhere."""
        d = self._mask(keep, label, min_size, invert, fill, box, out_type)
        shape = self._out_dims(d)[::-1]
        labels = _words_like(labels, shape, "labels have")
        sizes = _words_like(sizes, shape, "sizes have")
        out = np.empty(shape, np.float32 if d.out_type == VOXEL_F32 else np.uint8)
        _prefill(prefill, out)
        self._chk(self.lib.vv_mask_volume(self.h, C.byref(d), labels.ctypes.data, sizes.ctypes.data if sizes is not None else None,
                                          out.ctypes.data, out.nbytes, 0, None))
        return out

    def mask_device(self, out_ptr: int, capacity: int, labels_ptr: int, keep=KEEP_FOREGROUND, label=0, min_size=0, sizes_ptr: int = 0, invert=False,
                    fill=0.0, box=None, out_type=None, stream: int = 0):
        """vv_mask_volume on device buffers, enqueued on `stream`; returns the box's (bx, by, bz)."""
        d = self._mask(keep, label, min_size, invert, fill, box, out_type)
        self._chk(self.lib.vv_mask_volume(self.h, C.byref(d), labels_ptr or None, sizes_ptr or None, out_ptr or None, int(capacity), 1, stream or None))
        return self._out_dims(d)

    def keep_component(self, seed, bins, connectivity=6, invert=False, fill=0.0, box=None, out_type=None) -> np.ndarray:
        """The seeded region grow, composed of the two calls: label(bins, connectivity, box), then mask(KEEP_LABEL) with the label under
        seed = (x, y, z) in volume coordinates.  ValueError if the seed lies outside the box or on background."""
        labels = self.label(bins, connectivity, box)
        lo = (0, 0, 0) if box is None else tuple(int(v) for v in box[0])
        x, y, z = (int(s) - l for s, l in zip(seed, lo))
        bz, by, bx = labels.shape
        if not (0 <= x < bx and 0 <= y < by and 0 <= z < bz):
            raise ValueError(f"seed {tuple(seed)} lies outside the box")
        lab = int(labels[z, y, x])
        if lab == 0:
            raise ValueError(f"seed {tuple(seed)} is background for bins {bins}")
        return self.mask(labels, KEEP_LABEL, label=lab, invert=invert, fill=fill, box=box, out_type=out_type)

    # vv_distance_volume (no reference counterpart)
    def _distance(self, bins, have_labels, label, invert, spacing, box, within) -> vv_distance:
        """bins = (bin_lo, bin_hi) or one bin: VV_SEED_BINS; else labels with `label` (VV_SEED_LABEL) or without (VV_SEED_NONZERO).  `within`:
        None = VV_DIST_SQUARED, an integer r^2 = VV_DIST_WITHIN."""
        if (bins is None) != bool(have_labels):
            raise ValueError("give either bins or labels")
        d = _set_box(vv_distance(), box)
        if bins is not None:
            d.seed = SEED_BINS
            _set_bins(d, bins)
        else:
            d.seed, d.label = (SEED_NONZERO, 0) if label is None else (SEED_LABEL, int(label))
        d.invert = int(bool(invert))
        d.spacing[:] = [int(v) for v in spacing]
        d.out, d.within_r2 = (DIST_SQUARED, 0) if within is None else (DIST_WITHIN, int(within))
        return d

    def distance(self, bins=None, labels=None, label=None, invert=False, spacing=(1, 1, 1), box=None, within=None, prefill=None) -> np.ndarray:
        """vv_distance_volume into a host array [bz, by, bx] uint32: the squared distance to the nearest seed (DISTANCE_NONE everywhere without
        one), or with `within` = r^2 the 0 / 1 set of the voxels at most that far.  Seeds: the voxels in `bins`, or those of host `labels`
        [bz, by, bx] that equal `label` (label None: that are not 0); `invert`: the others.  `prefill`: the byte the output holds before the call."""
        d = self._distance(bins, labels is not None, label, invert, spacing, box, within)
        shape = self._out_dims(d)[::-1]
        labels = _words_like(labels, shape, "labels have")
        out = np.empty(shape, np.uint32)
        _prefill(prefill, out)
        self._chk(self.lib.vv_distance_volume(self.h, C.byref(d), labels.ctypes.data if labels is not None else None,
                                              out.ctypes.data if out.size else None, out.nbytes, 0, None))
        return out

    def distance_device(self, out_ptr: int, capacity: int, bins=None, label=None, invert=False, spacing=(1, 1, 1), box=None, within=None,
                        labels_ptr: int = 0, stream: int = 0):
        """vv_distance_volume on device buffers (4-byte aligned; labels_ptr may be out_ptr itself), enqueued on `stream`; returns the box's
        (bx, by, bz)."""
        d = self._distance(bins, bool(labels_ptr), label, invert, spacing, box, within)
        self._chk(self.lib.vv_distance_volume(self.h, C.byref(d), labels_ptr or None, out_ptr or None, int(capacity), 1, stream or None))
        return self._out_dims(d)

    def morphology(self, op, radius, bins=None, labels=None, label=None, spacing=(1, 1, 1), box=None) -> np.ndarray:
        """The set S of distance()'s seeds dilated, eroded, opened or closed (MORPH_*) with a ball of `radius` (in the units of `spacing`), as a
        0 / 1 uint32 array [bz, by, bx] that Context.mask(..., KEEP_FOREGROUND) takes as labels.  A voxel belongs to the ball iff its squared
        distance is at most r2 = floor(radius^2), formed in binary64.  dilate(S) = the voxels within r2 of S; erode(S) = the complement of the
        voxels within r2 of S's complement; open = dilate(erode), close = erode(dilate).  The box is the world: nothing lies outside it, so an
        erosion does not eat in from its faces.  Every step is a vv_distance_volume call in place on one device buffer of the call's own (a
        complement is taken by the next step's `invert`; a last one by a call with r2 = 0); only the result leaves the device."""
        if op not in (MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE):
            raise ValueError("op must be MORPH_DILATE, MORPH_ERODE, MORPH_OPEN or MORPH_CLOSE")
        radius = float(radius)
        if not (radius >= 0.0 and np.isfinite(radius)):
            raise ValueError("radius must be finite and not negative")
        r2 = min(int(np.floor(radius * radius)), 0xFFFFFFFE)
        probe = self._distance(bins, labels is not None, label, False, spacing, box, r2)
        shape = self._out_dims(probe)[::-1]
        out = np.empty(shape, np.uint32)
        labels = _words_like(labels, shape, "labels have")
        with _DeviceBuffers(self.lib, "morphology") as dev:
            p = dev.alloc(out.nbytes, "the working buffer")
            if labels is not None:
                dev.upload(p, labels, "the labels")
            src = dict(bins=bins, label=label, labels_ptr=p if labels is not None else 0)
            again = dict(labels_ptr=p, invert=True)                 # the complement of what the buffer holds
            first_invert = op in (MORPH_ERODE, MORPH_OPEN)
            self.distance_device(p, out.nbytes, invert=first_invert, spacing=spacing, box=box, within=r2, **src)
            if op in (MORPH_OPEN, MORPH_CLOSE):
                self.distance_device(p, out.nbytes, spacing=spacing, box=box, within=r2, **again)
            if op in (MORPH_ERODE, MORPH_CLOSE):
                self.distance_device(p, out.nbytes, spacing=spacing, box=box, within=0, **again)
            return dev.download(out, p, "the result")

    # vv_region_table (no reference counterpart)
    def _regions(self, source, box, max_regions) -> vv_regions:
        d = _set_box(vv_regions(), box)
        d.source, d.max_regions = int(source), int(max_regions)
        return d

    def regions(self, labels: np.ndarray, aux=None, source=REGION_LABELS, box=None, max_regions=None, return_compact=False, return_summary=False,
                prefill=None):
        """vv_region_table with host labels (and aux) [bz, by, bx] uint32: the table as a structured array of REGION_DTYPE with max_regions rows
        (None: as many as the labels have regions, counted here; rows beyond the regions keep `prefill`), then with return_compact the consecutive
        labels [bz, by, bx] uint32 and with return_summary a RegionSummary (in that order, as a tuple)."""
        labels = np.ascontiguousarray(labels, np.uint32)
        if max_regions is None:
            flat = labels.ravel()
            max_regions = int((flat == np.arange(1, flat.size + 1, dtype=np.uint64)).sum()) if source == REGION_LABELS else int(flat.any())
        d = self._regions(source, box, max_regions)
        shape = self._out_dims(d)[::-1]
        labels = _words_like(labels, shape, "labels have")
        aux = _words_like(aux, shape, "aux has")
        table = np.zeros(int(max_regions), REGION_DTYPE)
        compact = np.empty(shape, np.uint32)
        st = vv_region_summary() if return_summary else None
        _prefill(prefill, table, compact, st)
        self._chk(self.lib.vv_region_table(self.h, C.byref(d), labels.ctypes.data, aux.ctypes.data if aux is not None else None,
                                           compact.ctypes.data, compact.nbytes, table.ctypes.data if max_regions else None, table.nbytes,
                                           C.addressof(st) if return_summary else None, 0, None))
        return _one_or_tuple([table] + ([compact] if return_compact else []) + ([RegionSummary.from_bytes(st)] if return_summary else []))

    def regions_device(self, labels_ptr: int, compact_ptr: int, compact_capacity: int, table_ptr: int = 0, max_regions: int = 0, aux_ptr: int = 0,
                       summary_ptr: int = 0, source=REGION_LABELS, box=None, stream: int = 0):
        """vv_region_table on device buffers (labels, aux, compact: 4 bytes per voxel, 4-byte aligned; table: max_regions rows of 184 bytes and
        summary: 32 bytes, both 8-byte aligned), enqueued on `stream`; returns the box's (bx, by, bz)."""
        d = self._regions(source, box, max_regions)
        self._chk(self.lib.vv_region_table(self.h, C.byref(d), labels_ptr or None, aux_ptr or None, compact_ptr or None, int(compact_capacity),
                                           table_ptr or None, C.sizeof(vv_region) * int(max_regions), summary_ptr or None, 1, stream or None))
        return self._out_dims(d)

    def measure(self, bins, connectivity=6, box=None, spacing=(1, 1, 1), thickness=False) -> np.ndarray:
        """The region table of the components of `bins`, composed on device buffers of the call's own: label(bins, connectivity, box); with
        `thickness` the squared distance of every foreground voxel to the background (distance of the labels, inverted, with the integer `spacing`)
        as aux; then regions with one row per component.  Only the label statistics (32 bytes, for the row count) and the table leave the device.
        region_properties(table, spacing) turns the rows into centroids, areas and radii."""
        nbytes = 4 * int(np.prod(self._out_dims(self._label(bins, connectivity, box))))
        with _DeviceBuffers(self.lib, "measure") as dev:
            lab, comp, st = dev.alloc(nbytes), dev.alloc(nbytes), dev.alloc(32)
            self.label_device(lab, nbytes, bins, connectivity, box, stats_ptr=st)
            k = LabelStats.from_bytes(dev.download(np.empty(32, np.uint8), st, "the label statistics")).components
            aux = 0
            if thickness:
                aux = dev.alloc(nbytes)
                self.distance_device(aux, nbytes, invert=True, spacing=spacing, box=box, labels_ptr=lab)
            table = np.zeros(k, REGION_DTYPE)
            tab = dev.alloc(table.nbytes)
            self.regions_device(lab, comp, nbytes, tab if k else 0, k, aux_ptr=aux, box=box)
            return dev.download(table, tab, "the table")

    # vv_mesh_dims / vv_surface_mesh (no reference counterpart)
    def _mesh(self, level, bins, have_labels, label, cap, box, max_vertices=0, max_quads=0) -> vv_mesh:
        """Exactly one of level (MESH_INDEX), bins = (bin_lo, bin_hi) or one bin (MESH_BINS) and labels, with `label` (MESH_LABEL) or without
        (MESH_NONZERO)."""
        if (level is not None) + (bins is not None) + bool(have_labels) != 1:
            raise ValueError("give exactly one of level, bins and labels")
        d = _set_box(vv_mesh(), box)
        if level is not None:
            d.source, d.level = MESH_INDEX, int(level)
        elif bins is not None:
            d.source = MESH_BINS
            _set_bins(d, bins)
        else:
            d.source, d.label = (MESH_NONZERO, 0) if label is None else (MESH_LABEL, int(label))
        d.cap, d.max_vertices, d.max_quads = int(cap), int(max_vertices), int(max_quads)
        return d

    def _mesh_dims(self, d: vv_mesh):
        m = (C.c_int * 3)()
        self._chk(self.lib.vv_mesh_dims(self.h, C.byref(d), C.byref(m)))
        return int(m[0]), int(m[1]), int(m[2])

    def mesh_dims(self, cap=True, box=None):
        """vv_mesh_dims: (mx, my, mz) of the site grid of this box and cap (an extent may be 0)."""
        return self._mesh_dims(self._mesh(1, None, False, None, cap, box))

    def surface(self, level=None, bins=None, labels=None, label=None, cap=True, box=None, normals=False, return_index=False) -> Mesh:
        """vv_surface_mesh with host buffers: the surface-nets mesh of the voxels whose classification index is at least `level`, or lies in `bins`, or
        whose word of host `labels` [bz, by, bx] uint32 equals `label` (label None: is not 0).  cap: close the surface at the box's faces.  A
        count-only call, then the full call into exactly sized arrays."""
        d = self._mesh(level, bins, labels is not None, label, cap, box)
        labels = _words_like(labels, self._out_dims(d)[::-1], "labels have")
        lp = labels.ctypes.data if labels is not None else None
        st = vv_mesh_summary()
        self._chk(self.lib.vv_surface_mesh(self.h, C.byref(d), lp, None, 0, None, 0, None, None, 0, C.addressof(st), 0, None))
        V, Q = int(st.vertices), int(st.quads)
        d.max_vertices, d.max_quads = V, Q
        mx, my, mz = self._mesh_dims(d)
        words = np.zeros(max(mx * my * mz, 1), np.uint32)                # (an empty site grid still gives the full call an index to name)
        index = words[:mx * my * mz].reshape(mz, my, mx)
        vert = np.zeros(V, MESH_VERTEX_DTYPE)
        norm = np.zeros(V, MESH_NORMAL_DTYPE) if normals else None
        quads = np.zeros((Q, 4), np.uint32)
        self._chk(self.lib.vv_surface_mesh(self.h, C.byref(d), lp, words.ctypes.data, index.nbytes, vert.ctypes.data if V else None, vert.nbytes,
                                           norm.ctypes.data if normals and V else None, quads.ctypes.data if Q else None, quads.nbytes,
                                           C.addressof(st), 0, None))
        assert (int(st.vertices), int(st.quads), int(st.written_vertices), int(st.written_quads)) == (V, Q, V, Q)
        xyz = np.stack([vert["x"], vert["y"], vert["z"]], axis=1) if V else np.zeros((0, 3), np.float32)
        return Mesh(np.ascontiguousarray(xyz, np.float32), vert["site"].copy(), quads, norm, index if return_index else None)

    def surface_device(self, index_ptr: int, index_capacity: int, vertices_ptr: int = 0, max_vertices: int = 0, quads_ptr: int = 0, max_quads: int = 0,
                       normals_ptr: int = 0, summary_ptr: int = 0, level=None, bins=None, labels_ptr: int = 0, label=None, cap=True, box=None,
                       stream: int = 0):
        """vv_surface_mesh on device buffers (labels, index: 4-byte aligned; vertices, normals, quads: 16-byte records, 16-byte aligned; summary: 32
        bytes, 8-byte aligned), enqueued on `stream`; index_ptr 0 with both maxima 0: count only.  Returns the site grid's (mx, my, mz)."""
        d = self._mesh(level, bins, bool(labels_ptr), label, cap, box, max_vertices, max_quads)
        self._chk(self.lib.vv_surface_mesh(self.h, C.byref(d), labels_ptr or None, index_ptr or None, int(index_capacity), vertices_ptr or None,
                                           16 * int(max_vertices), normals_ptr or None, quads_ptr or None, 16 * int(max_quads), summary_ptr or None,
                                           1, stream or None))
        return self._mesh_dims(d)

    # VolumeGenerator::drawEllipsoid x n / drawDefaultBrain (volumegenerator.cpp:31-119)
    def generate_ellipsoids(self, nx: int, ny: int, nz: int, centers, axes, colors) -> np.ndarray:
        centers = np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
        axes = np.ascontiguousarray(axes, np.float32).reshape(-1, 3)
        colors = np.ascontiguousarray(colors, np.uint8).reshape(-1)
        out = np.zeros((nz, ny, nx), np.uint8)
        self._chk(self.lib.vv_generate_ellipsoids(self.h, out.ctypes.data, 0, nx, ny, nz, len(colors),
                                                  centers.ctypes.data, axes.ctypes.data, colors.ctypes.data, None))
        return out

    def draw_ellipsoid(self, vol: np.ndarray, center, axes, color: int) -> np.ndarray:
        """vv_draw_ellipsoid: one VolumeGenerator::drawEllipsoid applied in place to vol [nz,ny,nx]."""
        assert vol.dtype == np.uint8 and vol.flags.c_contiguous
        nz, ny, nx = vol.shape
        c = np.ascontiguousarray(center, np.float32); a = np.ascontiguousarray(axes, np.float32)
        self._chk(self.lib.vv_draw_ellipsoid(self.h, vol.ctypes.data, 0, nx, ny, nz, c.ctypes.data, a.ctypes.data,
                                             int(color), None))
        return vol

    def generate_default_brain(self, nx: int, ny: int, nz: int) -> np.ndarray:
        out = np.zeros((nz, ny, nx), np.uint8)
        self._chk(self.lib.vv_generate_default_brain(self.h, out.ctypes.data, 0, nx, ny, nz, None))
        return out

    def generate_default_brain_device(self, dev_ptr: int, nx: int, ny: int, nz: int, stream: int = 0):
        self._chk(self.lib.vv_generate_default_brain(self.h, dev_ptr, 1, nx, ny, nz, stream))

    def generate_noise_device(self, dev_ptr: int, nx: int, ny: int, nz: int, seed: int, stream: int = 0):
        self._chk(self.lib.vv_generate_noise_u8(self.h, dev_ptr, nx, ny, nz, seed, stream))

    def promote_device(self, dev_in: int, dev_out: int, n: int, stream: int = 0):
        self._chk(self.lib.vv_promote_u8_to_f32(self.h, dev_in, dev_out, n, stream))


def stencil_taps(shape: int, radius: int, sigma: float = 0.0) -> np.ndarray:
    """vv_stencil_taps: float32[5], taps[0] the centre, taps[k] at distance k, zeros beyond the radius."""
    t = (C.c_float * 5)()
    rc = load_library().vv_stencil_taps(int(shape), int(radius), float(sigma), C.byref(t))
    if rc != 0:
        raise VolvizError(rc, "vv_stencil_taps: bad shape, radius or sigma")
    return np.array(t[:], np.float32)


def resample_matrix(euler=(0.0, 0.0, 0.0), zoom: float = 1.0, centre=(0.5, 0.5, 0.5), scale=None) -> np.ndarray:
    """vv_resample_matrix: float32[12], the row-major 3 x 4 matrix of Context.resample for a rotation Rz Ry Rx (radians), a zoom about `centre`
    (texture coordinates) and the voxel scales of an anisotropic volume."""
    f3 = C.c_float * 3
    m = (C.c_float * 12)()
    s = None if scale is None else C.byref(f3(*[float(v) for v in scale]))
    rc = load_library().vv_resample_matrix(C.byref(f3(*[float(v) for v in euler])), float(zoom), C.byref(f3(*[float(v) for v in centre])), s, C.byref(m))
    if rc != 0:
        raise VolvizError(rc, "vv_resample_matrix: bad angle, zoom, centre or scale")
    return np.array(m[:], np.float32)


def cut_plane_canonical(orientation: int, displace: float):
    """vv_cut_plane_canonical: GLWidget::setSliceCanonical (glwidget.cpp:743-788)."""
    pt = np.zeros(3, np.float32); n = np.zeros(3, np.float32)
    rc = load_library().vv_cut_plane_canonical(orientation, displace, pt.ctypes.data, n.ctypes.data)
    if rc:
        raise VolvizError(rc, "bad orientation")
    return pt, n


def cut_plane_from_euler(dx, dy, dz, theta, phi, psi):
    """vv_cut_plane_from_euler: the free-form slice view's cutting plane (window.cpp:425-443 -> GLWidget::setSlicePro) -> (point, normal)."""
    pt = np.zeros(3, np.float32); n = np.zeros(3, np.float32)
    rc = load_library().vv_cut_plane_from_euler(dx, dy, dz, theta, phi, psi, pt.ctypes.data, n.ctypes.data)
    if rc:
        raise VolvizError(rc, "bad argument")
    return pt, n


def cut_plane_to_slice_params(slice_type: int, point, normal, flip: bool = False) -> slice_params:
    """vv_cut_plane_to_slice_params: glwidget.cpp:232-258."""
    sp = slice_params()
    pt = np.ascontiguousarray(point, np.float32); n = np.ascontiguousarray(normal, np.float32)
    rc = load_library().vv_cut_plane_to_slice_params(slice_type, pt.ctypes.data, n.ctypes.data, int(flip), C.byref(sp))
    if rc:
        raise VolvizError(rc, "bad slice type")
    return sp


def _f3(v) -> np.ndarray:
    return np.ascontiguousarray(v, np.float32).reshape(3).copy()


def camera_orbit_drag(position, dx: int, dy: int):
    """vv_camera_orbit_drag: right-button drag (glwidget.cpp:432-446) -> (position, look)."""
    p = _f3(position); out = np.zeros(3, np.float32); look = np.zeros(3, np.float32)
    rc = load_library().vv_camera_orbit_drag(p.ctypes.data, dx, dy, out.ctypes.data, look.ctypes.data)
    if rc:
        raise VolvizError(rc, "camera at the origin")
    return out, look


def camera_zoom(position, look, delta: int) -> np.ndarray:
    """vv_camera_zoom: wheel (glwidget.cpp:607-620)."""
    p = _f3(position); l = _f3(look); out = np.zeros(3, np.float32)
    rc = load_library().vv_camera_zoom(p.ctypes.data, l.ctypes.data, delta, out.ctypes.data)
    if rc:
        raise VolvizError(rc, "bad argument")
    return out


def cut_plane_from_drag(position, look, up, aspect: float, press, release):
    """vv_cut_plane_from_drag: left-button drag released (glwidget.cpp:482-535)
    -> (point, normal, plane_up, plane_right)."""
    p = _f3(position); l = _f3(look); u = _f3(up)
    a = np.ascontiguousarray(press, np.float32).reshape(2).copy()
    b = np.ascontiguousarray(release, np.float32).reshape(2).copy()
    out = [np.zeros(3, np.float32) for _ in range(4)]
    rc = load_library().vv_cut_plane_from_drag(p.ctypes.data, l.ctypes.data, u.ctypes.data, aspect, a.ctypes.data,
                                               b.ctypes.data, *[o.ctypes.data for o in out])
    if rc:
        raise VolvizError(rc, "bad argument")
    return tuple(out)


def cut_plane_drag(point, plane_up, plane_right, dx: int, dy: int, width: int, height: int) -> np.ndarray:
    """vv_cut_plane_drag: middle-button drag of an image plane (glwidget.cpp:447-452)."""
    p = _f3(point); u = _f3(plane_up); r = _f3(plane_right)
    rc = load_library().vv_cut_plane_drag(p.ctypes.data, u.ctypes.data, r.ctypes.data, dx, dy, width, height)
    if rc:
        raise VolvizError(rc, "bad argument")
    return p


def slice_to_bgra(buf: np.ndarray, height: int, width: int, fill: int = 0) -> np.ndarray:
    """vv_slice_to_bgra: the image SliceWidget shows (slicewidget.cpp:108-121)."""
    buf = np.ascontiguousarray(buf, np.float32)
    out = np.full((height * width, 4), fill, np.uint8)
    rc = load_library().vv_slice_to_bgra(buf.ctypes.data, height, width, out.ctypes.data)
    if rc:
        raise VolvizError(rc, "bad argument")
    return out


def slice_matrix(dx, dy, dz, theta, phi, psi) -> np.ndarray:
    """vv_slice_matrix: SliceWidget::getTransformationMatrix (slicewidget.cpp:147-165)."""
    m = np.zeros(16, np.float32)
    rc = load_library().vv_slice_matrix(dx, dy, dz, theta, phi, psi, m.ctypes.data)
    if rc:
        raise VolvizError(rc, "angles must be in [-3.2, 3.2)")
    return m.reshape(4, 4)
