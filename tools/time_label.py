"""developer tool (1 GPU): time of vv_label_volume (labels, sizes and stats into device buffers) and of vv_mask_volume on an n^3 u8 volume: the brain
phantom of vv_generate_default_brain and the noise volume, each at two bin ranges (the noise volume's are picked from its histogram: the bins 0..k that
hold about 0.097 and 0.31 of the voxels, the percolation thresholds of 26- and 6-connectivity) and the three connectivities.

  - the whole call, and its launches by difference: VV_LABEL_PHASES = 1, 2, 3 stops the call behind the local, merge and flatten launch (the rest,
    the two stats launches, is the difference to the whole call);
  - GB/s = the call's compulsory bytes / time: one read of the box (1 byte per voxel) plus 4 bytes per voxel of labels written and another 4 of
    sizes; vv_derive_volume at factor 1 of the same volume (1 byte in, 1 byte out per voxel) as the streaming yardstick of this library;
  - context: scipy.ndimage.label on the host for a --crop^3 corner of the same volume and bins (when scipy is installed; the label call on the
    same crop beside it).

Every figure is the median over the repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library.
    python tools/time_label.py [--n 1024] [--iters 3] [--repeats 3] [--crop 256] [--out FILE]"""
import argparse, os, statistics, sys, time
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=3, help="calls per timing")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--crop", type=int, default=256, help="edge of the crop scipy labels on the host (0: no host baseline)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.iters >= 1 and args.repeats >= 1


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
        os.environ["VV_LABEL_PHASES"] = str(k)
    else:
        os.environ.pop("VV_LABEL_PHASES", None)
    ctx.reread_env()


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 u8, {args.iters} calls per timing, {args.repeats} repeats (median [min .. max]); labels, sizes and stats into device buffers, enqueue-only")
emit("GB/s = (1 + 4 + 4 bytes per voxel) / time of the whole label call; derive 1x: (1 + 1 bytes per voxel) / time")
tf = vv.transfer_preset(vv.TF_HEAD)
vol = torch.empty(vox, dtype=torch.uint8, device=dev)
labels = torch.empty(vox, dtype=torch.int32, device=dev)
sizes = torch.empty(vox, dtype=torch.int32, device=dev)
stats = torch.empty(4, dtype=torch.int64, device=dev)
out = torch.empty(vox, dtype=torch.uint8, device=dev)
try:
    from scipy import ndimage
except Exception:
    ndimage = None

for name, bin_ranges in (("brain", ((60, 60), (80, 120))), ("noise", None)):
    if name == "brain":
        ctx.generate_default_brain_device(vol.data_ptr(), n, n, n)
    else:
        ctx.generate_noise_device(vol.data_ptr(), n, n, n, 3)
    torch.cuda.synchronize()
    ctx.load_volume_device(vol.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
    torch.cuda.synchronize()
    if bin_ranges is None:                                      # the noise volume: bins 0..k with about `fraction` of the voxels, from its histogram
        cum = np.cumsum(ctx.histogram().counts.astype(np.float64)) / vox
        bin_ranges = tuple((0, int(np.argmin(np.abs(cum - fraction)))) for fraction in (0.097, 0.31))
        emit(f"noise: bins {bin_ranges[0]} hold {cum[bin_ranges[0][1]]:.4f} of the voxels, bins {bin_ranges[1]} {cum[bin_ranges[1][1]]:.4f} (the percolation thresholds of 26 and 6 are about 0.097 and 0.31)")
    derive = lambda: ctx.derive_device(out.data_ptr(), out.numel(), None, 1, vv.REDUCE_MEAN, vv.VOXEL_U8, stream=stream)
    for bins in bin_ranges:
        for conn in (6, 18, 26):
            label = lambda: ctx.label_device(labels.data_ptr(), vox * 4, bins, conn, sizes_ptr=sizes.data_ptr(), stats_ptr=stats.data_ptr(), stream=stream)
            mask = lambda: ctx.mask_device(out.data_ptr(), vox, labels.data_ptr(), vv.KEEP_MIN_SIZE, min_size=100, sizes_ptr=sizes.data_ptr(), stream=stream)
            phases(0)
            label(); mask(); derive()
            torch.cuda.synchronize()
            st = vv.LabelStats.from_bytes(stats.cpu().numpy().tobytes())
            t = {k: [] for k in (1, 2, 3, 0, "mask", "derive")}
            for _ in range(args.repeats):                       # alternated
                for k in (1, 2, 3, 0):
                    phases(k)
                    t[k].append(timed(label, args.iters))
                t["mask"].append(timed(mask, args.iters))
                t["derive"].append(timed(derive, args.iters))
            phases(0)
            label()                                             # (the mask of the next round reads finished labels)
            torch.cuda.synchronize()
            med = {k: statistics.median(v) for k, v in t.items()}
            emit(f"{name} bins {bins[0]:3d}..{bins[1]:3d} connectivity {conn:2d}: foreground {st.foreground} components {st.components} largest {st.largest_size} (label {st.largest_label})")
            emit(f"    whole call {spread(t[0])} us  {9 * vox / med[0] / 1e3:7.1f} GB/s   local {med[1]:9.1f}  merge {med[2] - med[1]:9.1f}  flatten {med[3] - med[2]:9.1f}  "
                 f"stats {med[0] - med[3]:9.1f} us   (cumulative: {spread(t[1])} / {spread(t[2])} / {spread(t[3])})")
            emit(f"    mask MIN_SIZE {spread(t['mask'])} us  {(1 + 4 + 4 + 1) * vox / med['mask'] / 1e3:7.1f} GB/s   derive 1x {spread(t['derive'])} us  {2 * vox / med['derive'] / 1e3:7.1f} GB/s,"
                 f" label / derive {med[0] / med['derive']:6.2f}")
        if ndimage is not None and args.crop and args.crop <= n and bins == bin_ranges[-1]:      # once per volume, behind its last bin range
            c = args.crop
            box = ((0, 0, 0), (c, c, c))
            host = vol.view(n, n, n)[:c, :c, :c].contiguous().cpu().numpy()
            for bins in bin_ranges:
                fg = (host >= bins[0]) & (host <= bins[1])
                for conn in (6, 26):
                    t0 = time.perf_counter()
                    _, ncomp = ndimage.label(fg, ndimage.generate_binary_structure(3, {6: 1, 26: 3}[conn]))
                    t_host = (time.perf_counter() - t0) * 1e6
                    fn = lambda: ctx.label_device(labels.data_ptr(), c ** 3 * 4, bins, conn, box, sizes_ptr=sizes.data_ptr(), stats_ptr=stats.data_ptr(), stream=stream)
                    fn()
                    torch.cuda.synchronize()
                    st = vv.LabelStats.from_bytes(stats.cpu().numpy().tobytes())
                    assert st.components == ncomp, (st, ncomp)
                    emit(f"{name} {c}^3 crop bins {bins[0]:3d}..{bins[1]:3d} connectivity {conn:2d}: scipy.ndimage.label on the host {t_host:10.1f} us ({ncomp} components);"
                         f" vv_label_volume {spread([timed(fn, args.iters) for _ in range(args.repeats)])} us")
