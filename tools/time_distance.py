"""developer tool (1 GPU): time of vv_distance_volume (the squared distances into a device buffer) on an n^3 u8 volume, for the inputs that bracket what the
lower-envelope passes can meet: no seed, one seed in a corner, seeds on the plane x = 0, the brain phantom's shells (bins 60..60 and 80..120), noise at
bins 0..108, and everything a seed.

  - the whole call, and its launches by difference: VV_DISTANCE_PHASES = 1, 2 stops the call behind the x and the y launch;
  - TB/s = the compulsory bytes / time: the x launch reads 1 byte per voxel and writes 4, the y and z launches read 4 and write 4 each (21 bytes per
    voxel for the call); vv_derive_volume at factor 1 of the same volume (1 byte in, 1 byte out per voxel) as the streaming yardstick of this library;
  - one Context.morphology(MORPH_OPEN, 3) of the brain's bins 80..120 (wall clock, the result's download included) and its two device calls alone;
  - context: scipy.ndimage.distance_transform_edt on the host for a --crop^3 corner of the brain (when scipy is installed; the call on the same crop
    beside it, and the words compared).

Every figure is the median over the repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library.
    python tools/time_distance.py [--n 1024] [--iters 2] [--repeats 3] [--crop 256] [--out FILE]"""
import argparse, os, statistics, sys, time
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge (at most 2048)")
ap.add_argument("--iters", type=int, default=2, help="calls per timing")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--crop", type=int, default=256, help="edge of the crop scipy transforms on the host (0: no host baseline)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.iters >= 1 and args.repeats >= 1 and args.n <= vv.DISTANCE_MAX_EXTENT


def emit(s):
    print(s, flush=True)
    if args.out:                                                # line by line: a run that is cut short keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")


dev = torch.device("cuda", 0)
ctx = vv.Context(0)
n = args.n
vox = n ** 3
stream = vv.stream_handle(torch.cuda.current_stream())


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                    # us per call of fn


def spread(v):
    return f"{statistics.median(v):10.1f} [{min(v):10.1f} .. {max(v):10.1f}]"


def phases(k):
    if k:
        os.environ["VV_DISTANCE_PHASES"] = str(k)
    else:
        os.environ.pop("VV_DISTANCE_PHASES", None)
    ctx.reread_env()


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 u8, {args.iters} calls per timing, {args.repeats} repeats (median [min .. max]); the squared distances into a device buffer, enqueue-only")
emit("TB/s = compulsory bytes / time: x launch (1 + 4) bytes per voxel, y and z launches (4 + 4) each, the call 21; derive 1x: (1 + 1) bytes per voxel")
tf = vv.transfer_preset(vv.TF_HEAD)
vol = torch.empty(vox, dtype=torch.uint8, device=dev)
dist = torch.empty(vox, dtype=torch.int32, device=dev)
out = torch.empty(vox, dtype=torch.uint8, device=dev)
cube = vol.view(n, n, n)
whole = []


def load():
    torch.cuda.synchronize()
    ctx.load_volume_device(vol.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
    torch.cuda.synchronize()


def measure(name, bins):
    call = lambda: ctx.distance_device(dist.data_ptr(), vox * 4, bins=bins, stream=stream)
    derive = lambda: ctx.derive_device(out.data_ptr(), out.numel(), None, 1, vv.REDUCE_MEAN, vv.VOXEL_U8, stream=stream)
    phases(0)
    call(); derive()
    torch.cuda.synchronize()
    seeds = int((dist == 0).sum())
    far = int(dist.max()) if int(dist.min()) >= 0 else int(dist[dist < 0].max()) + (1 << 32)      # (the words are uint32)
    t = {k: [] for k in (1, 2, 0, "derive")}
    for _ in range(args.repeats):                               # alternated
        for k in (1, 2, 0):
            phases(k)
            t[k].append(timed(call, args.iters))
        t["derive"].append(timed(derive, args.iters))
    phases(0)
    med = {k: statistics.median(v) for k, v in t.items()}
    x, y, z = med[1], med[2] - med[1], med[0] - med[2]
    whole.append((name, med[0]))
    emit(f"{name}: bins {bins[0]}..{bins[1]}, {seeds} seeds, largest word {far:#x}")
    emit(f"    whole call {spread(t[0])} us  {21 * vox / med[0] / 1e6:6.3f} TB/s   x {x:10.1f} us {5 * vox / x / 1e6:6.3f} TB/s   y {y:10.1f} us {8 * vox / y / 1e6:6.3f} TB/s   "
         f"z {z:10.1f} us {8 * vox / z / 1e6:6.3f} TB/s   (cumulative: {spread(t[1])} / {spread(t[2])})")
    emit(f"    derive 1x {spread(t['derive'])} us  {2 * vox / med['derive'] / 1e6:6.3f} TB/s, distance / derive {med[0] / med['derive']:7.2f}")


vol.zero_()
load()
measure("no seed", (1, 1))
cube[0, 0, 0] = 1
load()
measure("one seed in a corner", (1, 1))
cube[:, :, 0] = 1
load()
measure("seeds on the plane x = 0", (1, 1))
ctx.generate_default_brain_device(vol.data_ptr(), n, n, n)
load()
measure("brain shell", (60, 60))
measure("brain shells", (80, 120))
measure("everything a seed", (0, 255))

# the opening of the brain's inner shells with a ball of radius 3: the binding's call, and its device calls alone
w = dist.data_ptr()
opening = lambda: (ctx.distance_device(w, vox * 4, bins=(80, 120), invert=True, within=9, stream=stream),
                   ctx.distance_device(w, vox * 4, labels_ptr=w, invert=True, within=9, stream=stream))
opening()
torch.cuda.synchronize()
emit(f"morphology OPEN radius 3, bins 80..120: the two device calls in place {spread([timed(opening, 1) for _ in range(args.repeats)])} us")
t0 = time.perf_counter()
opened = ctx.morphology(vv.MORPH_OPEN, 3, bins=(80, 120))
t_wall = time.perf_counter() - t0
emit(f"    Context.morphology(MORPH_OPEN, 3): {t_wall * 1e3:10.1f} ms wall clock with its allocation and the download of {opened.nbytes >> 20} MiB; {int(opened.sum())} voxels in the opening")
del opened

try:
    from scipy import ndimage
except Exception:
    ndimage = None
if ndimage is not None and args.crop and args.crop <= n:
    c = args.crop
    o = (n - c) // 2                                            # the crop in the middle: the phantom's corner is empty
    box = ((o, o, o), (o + c, o + c, o + c))
    host = cube[o:o + c, o:o + c, o:o + c].contiguous().cpu().numpy()
    for bins in ((60, 60), (80, 120)):
        seed = (host >= bins[0]) & (host <= bins[1])
        t0 = time.perf_counter()
        e = ndimage.distance_transform_edt(~seed)
        t_host = (time.perf_counter() - t0) * 1e6
        fn = lambda: ctx.distance_device(dist.data_ptr(), c ** 3 * 4, bins=bins, box=box, stream=stream)
        fn()
        torch.cuda.synchronize()
        got = dist[:c ** 3].cpu().numpy().view(np.uint32).reshape(c, c, c)
        assert seed.any() and np.array_equal(got, np.rint(e * e).astype(np.uint32)), bins
        emit(f"brain {c}^3 crop bins {bins[0]}..{bins[1]}: scipy.ndimage.distance_transform_edt on the host {t_host:12.1f} us;"
             f" vv_distance_volume {spread([timed(fn, args.iters) for _ in range(args.repeats)])} us (the same words)")

ctx.generate_noise_device(vol.data_ptr(), n, n, n, 3)
load()
measure("noise", (0, 108))
best, worst = min(whole, key=lambda p: p[1]), max(whole, key=lambda p: p[1])
emit(f"spread over the inputs: best {best[0]} {best[1]:10.1f} us, worst {worst[0]} {worst[1]:10.1f} us, worst / best {worst[1] / best[1]:6.2f}")
