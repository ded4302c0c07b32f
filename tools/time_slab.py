"""developer tool (1 GPU): time of a thick-slab slice (vv_slice_slab / vv_slice_advanced_slab) writing into device buffers, against the K single
vv_slice / vv_slice_advanced calls at the same positions that a host without the slab calls would make (their reduction not included).

Slab and baseline run in one process and alternate; every figure is the median over the repeats with their range, so that the spread is
known before a difference is read.  VV_LIB selects another build of the library (make variant), --no-baseline times the slab alone.
    python tools/time_slab.py [--n 1024] [--hw 1024] [--samples 32] [--iters 10] [--repeats 3] [--voxels f32,u8] [--out FILE]"""
import argparse, ctypes as C, os, statistics, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--hw", type=int, default=1024, help="image edge")
ap.add_argument("--samples", type=int, default=32)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--voxels", default="f32,u8")
ap.add_argument("--no-baseline", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.iters >= 1 and args.repeats >= 1

dev = torch.device("cuda", 0)
ctx = vv.Context(0)
n, hw, K = args.n, args.hw, args.samples
thick = K / n                                                   # one sample per voxel layer
v8 = torch.empty(n ** 3, dtype=torch.uint8, device=dev)
ctx.generate_noise_device(v8.data_ptr(), n, n, n, 3)
stream = vv.stream_handle(torch.cuda.current_stream())
buf = torch.zeros(hw * hw, dtype=torch.float32, device=dev)
aux = torch.zeros(hw * hw, dtype=torch.int32, device=dev)
sc = (C.c_float * 3)(1.0, 1.0, 1.0)
f32 = np.float32
off = [float((f32(k) - f32(0.5) * f32(K - 1)) * (f32(thick) / f32(K))) for k in range(K)]
oblique = np.asarray(vv.slice_matrix(0.0, 0.0, 0.0, 0.5, 0.4, 0.0), f32).reshape(4, 4)
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3               # us per call of fn


def views():
    # (name, slab call, the K single-slice calls): the slab runs about the volume's centre, the image covers the whole cross-section
    for orient, name, axis in ((vv.SAGITTAL, "sagittal (xy plane, slab along z)", 2), (vv.HORIZONTAL, "horizontal (xz plane, slab along y)", 1),
                               (vv.CORONAL, "coronal (yz plane, slab along x)", 0)):
        d = [0.0, 0.0, 0.0]; d[axis] = 0.5
        planes = []
        for o in off:
            dk = list(d); dk[axis] = float(f32(d[axis]) + f32(o))
            planes.append(tuple(dk))
        yield (name,
               lambda mode, d=tuple(d), orient=orient: ctx.slice_slab_device(hw, hw, *d, orient, buf.data_ptr(), aux.data_ptr(), mode=mode, samples=K, thickness=thick, stream=stream),
               lambda planes=planes, orient=orient: [ctx._chk(ctx.lib.vv_slice(ctx.h, buf.data_ptr(), hw, hw, *p, orient, C.byref(sc), 0, vv.FILTER_TEX8, 1, stream)) for p in planes])
    mats = []
    for o in off:                                               # rz = 0.5 + o  <=>  the fourth column takes o times the third
        m = oblique.copy(); m[:, 3] += m[:, 2] * f32(o)
        mats.append((C.c_float * 16)(*[float(v) for v in m.reshape(16)]))
    yield ("oblique (Rx 0.5, Ry 0.4 about the centre)",
           lambda mode: ctx.slice_advanced_slab_device(hw, hw, oblique, buf.data_ptr(), aux.data_ptr(), mode=mode, samples=K, thickness=thick, stream=stream),
           lambda: [ctx._chk(ctx.lib.vv_slice_advanced(ctx.h, buf.data_ptr(), hw, hw, C.byref(m), C.byref(sc), vv.FILTER_TEX8, 1, stream)) for m in mats])


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):9.1f} .. {max(v):9.1f}]"


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 noise, image {hw} x {hw} on the device, slab of {K} samples across {thick:.6f}, {args.iters} calls per timing, {args.repeats} repeats (median [min .. max]), us")
for voxel in args.voxels.split(","):
    if voxel == "f32":
        v32 = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        ctx.promote_device(v8.data_ptr(), v32.data_ptr(), n ** 3)
        ctx.load_volume_device(v32.data_ptr(), vv.VOXEL_F32, n, n, n, vv.transfer_preset(vv.TF_HEAD))
        del v32
    else:
        ctx.load_volume_device(v8.data_ptr(), vv.VOXEL_U8, n, n, n, vv.transfer_preset(vv.TF_HEAD))
    torch.cuda.synchronize()
    for name, slab, singles in views():
        for mode, mname in ((vv.SLAB_MAX, "max"), (vv.SLAB_MIN, "min"), (vv.SLAB_MEAN, "mean")):
            for _ in range(2):                                  # warm-up: code objects, caches
                slab(mode)
                if not args.no_baseline:
                    singles()
            torch.cuda.synchronize()
            ts, tb = [], []
            for _ in range(args.repeats):                       # alternated
                ts.append(timed(lambda: slab(mode)))
                if not args.no_baseline:
                    tb.append(timed(singles))
            gs = hw * hw * K / statistics.median(ts) / 1e3
            line = f"{voxel:3s} {name:42s} {mname:4s}: slab {spread(ts)}  {gs:7.1f} Gsamples/s"
            if tb:
                line += f"   {K} slices {spread(tb)}   slab / slices {statistics.median(ts) / statistics.median(tb):6.3f} [{min(ts) / max(tb):6.3f} .. {max(ts) / min(tb):6.3f}]"
            emit(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
