"""developer tool (1 GPU): time of vv_region_table (compact, one row per region and the summary into device buffers, aux = the squared distances of
vv_distance_volume to the background) on the labels of an n^3 u8 volume, on the inputs of profiles/label_c3.txt under connectivity 6: an empty
foreground, the two shells of the brain phantom, and the noise volume at the bins that hold about 0.09 and 0.31 of the voxels (the latter is one
component of a third of the volume beside millions of small ones).

  - the whole call, and its launches by difference: VV_REGION_PHASES = 1, 2, 3, 4 stops the call behind the count, scan, rank and measure launch (the
    rest, the finish launch, is the difference to the whole call);
  - vv_label_volume on the same input and vv_derive_volume at factor 1 of the same volume (the streaming yardstick), in the same run;
  - GB/s = the call's compulsory bytes / time: `labels` read once in each of the launches 1, 3 and 4 (3 x 4 bytes per voxel), `compact` written once
    (4 bytes per voxel: the roots in launch 3, every other word in launch 4), and per voxel of a region that has a row 1 byte of the volume and 4 of aux;
    the ownership gathers, the six face neighbours and the roots' compact words are re-reads that the caches may serve and are not counted;
  - context: scipy.ndimage measurements on the host for a --crop^3 corner (sum_labels, find_objects, center_of_mass, maximum of aux on the compact
    labels, which are downloaded first: 4 bytes per voxel), with the words compared against the table.

Every figure is the median over the repeats with their range, device events around --iters calls.  VV_LIB selects another build of the library.
    python tools/time_regions.py [--n 1024] [--iters 2] [--repeats 3] [--crop 256] [--out FILE]"""
import argparse, os, statistics, sys, time
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "volume-viz_amd", "python"))
import volviz_amd as vv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1024, help="volume edge")
ap.add_argument("--iters", type=int, default=2, help="calls per timing")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--crop", type=int, default=256, help="edge of the crop scipy measures on the host (0: no host baseline)")
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
ROW = vv.REGION_DTYPE.itemsize


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
        os.environ["VV_REGION_PHASES"] = str(k)
    else:
        os.environ.pop("VV_REGION_PHASES", None)
    ctx.reread_env()


emit(f"library {vv.LIB_PATH}")
emit(f"volume {n}^3 u8, connectivity 6, {args.iters} calls per timing, {args.repeats} repeats (median [min .. max]); compact, table (one row per region) and summary into device buffers, enqueue-only")
emit("GB/s = (3 x 4 + 4 bytes per voxel + 5 bytes per voxel of a measured region) / time of the whole region call; derive 1x: (1 + 1 bytes per voxel) / time")
tf = vv.transfer_preset(vv.TF_HEAD)
vol = torch.empty(vox, dtype=torch.uint8, device=dev)
labels = torch.empty(vox, dtype=torch.int32, device=dev)
aux = torch.empty(vox, dtype=torch.int32, device=dev)
compact = torch.empty(vox, dtype=torch.int32, device=dev)
stats = torch.empty(4, dtype=torch.int64, device=dev)
summary = torch.empty(4, dtype=torch.int64, device=dev)
out = torch.empty(vox, dtype=torch.uint8, device=dev)
try:
    from scipy import ndimage
except Exception:
    ndimage = None
whole_us = {}

for name, bin_ranges in (("brain", ((60, 60), (80, 120))), ("noise", None)):
    if name == "brain":
        ctx.generate_default_brain_device(vol.data_ptr(), n, n, n)
    else:
        ctx.generate_noise_device(vol.data_ptr(), n, n, n, 3)
    torch.cuda.synchronize()
    ctx.load_volume_device(vol.data_ptr(), vv.VOXEL_U8, n, n, n, tf)
    torch.cuda.synchronize()
    counts = ctx.histogram().counts
    if bin_ranges is None:                                      # the noise volume: an empty bin, and bins 0..k with about `fraction` of the voxels, from its histogram
        cum = np.cumsum(counts.astype(np.float64)) / vox
        bin_ranges = tuple((0, int(np.argmin(np.abs(cum - fraction)))) for fraction in (0.097, 0.31))
        emit(f"noise: bins {bin_ranges[0]} hold {cum[bin_ranges[0][1]]:.4f} of the voxels, bins {bin_ranges[1]} {cum[bin_ranges[1][1]]:.4f}")
        empty = np.flatnonzero(counts == 0)
        if len(empty):
            bin_ranges = ((int(empty[0]), int(empty[0])),) + bin_ranges
    derive = lambda: ctx.derive_device(out.data_ptr(), out.numel(), None, 1, vv.REDUCE_MEAN, vv.VOXEL_U8, stream=stream)
    for bins in bin_ranges:
        label = lambda: ctx.label_device(labels.data_ptr(), vox * 4, bins, 6, stats_ptr=stats.data_ptr(), stream=stream)
        label()
        ctx.distance_device(aux.data_ptr(), vox * 4, invert=True, labels_ptr=labels.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        st = vv.LabelStats.from_bytes(stats.cpu().numpy().tobytes())
        K = st.components
        table = torch.empty(max(K, 1) * ROW, dtype=torch.uint8, device=dev)
        region = lambda: ctx.regions_device(labels.data_ptr(), compact.data_ptr(), vox * 4, table.data_ptr() if K else 0, K, aux_ptr=aux.data_ptr(),
                                            summary_ptr=summary.data_ptr(), stream=stream)
        phases(0)
        region(); derive()
        torch.cuda.synchronize()
        sm = vv.RegionSummary.from_bytes(summary.cpu().numpy().tobytes())
        assert (sm.regions, sm.written, sm.foreground, sm.stray) == (K, K, st.foreground, 0), (sm, st)
        rows = table.cpu().numpy()[:K * ROW].view(vv.REGION_DTYPE)
        assert int(rows["voxels"].sum()) == st.foreground and (K == 0 or (np.diff(rows["label"].astype(np.int64)) > 0).all())
        t = {k: [] for k in (1, 2, 3, 4, 0, "label", "derive")}
        for _ in range(args.repeats):                           # alternated
            for k in (1, 2, 3, 4, 0):
                phases(k)
                t[k].append(timed(region, args.iters))
            t["derive"].append(timed(derive, args.iters))
        phases(0)
        labels2 = compact                                       # (the label call is timed into the compact buffer: `labels` stays the regions' input)
        relabel = lambda: ctx.label_device(labels2.data_ptr(), vox * 4, bins, 6, stats_ptr=stats.data_ptr(), stream=stream)
        for _ in range(args.repeats):
            t["label"].append(timed(relabel, args.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        nbytes = 16 * vox + 5 * st.foreground
        whole_us[(name, bins)] = med[0]
        emit(f"{name} bins {bins[0]:3d}..{bins[1]:3d}: foreground {st.foreground} regions {K} largest {int(rows['voxels'].max()) if K else 0}")
        emit(f"    whole call {spread(t[0])} us  {nbytes / med[0] / 1e3:7.1f} GB/s   count {med[1]:9.1f}  scan {med[2] - med[1]:9.1f}  rank {med[3] - med[2]:9.1f}  measure {med[4] - med[3]:9.1f}  "
             f"finish {med[0] - med[4]:9.1f} us   (cumulative: {spread(t[1])} / {spread(t[2])} / {spread(t[3])} / {spread(t[4])})")
        emit(f"    vv_label_volume {spread(t['label'])} us   derive 1x {spread(t['derive'])} us  {2 * vox / med['derive'] / 1e3:7.1f} GB/s,"
             f" regions / derive {med[0] / med['derive']:6.2f}, regions / label {med[0] / med['label']:6.3f}")
        del table
    if ndimage is not None and args.crop and args.crop <= n:    # once per volume
        c = args.crop
        box = ((0, 0, 0), (c, c, c))
        for bins in bin_ranges[-2:]:
            ctx.label_device(labels.data_ptr(), c ** 3 * 4, bins, 6, box, stats_ptr=stats.data_ptr(), stream=stream)
            ctx.distance_device(aux.data_ptr(), c ** 3 * 4, invert=True, box=box, labels_ptr=labels.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            K = vv.LabelStats.from_bytes(stats.cpu().numpy().tobytes()).components
            table = torch.empty(max(K, 1) * ROW, dtype=torch.uint8, device=dev)
            fn = lambda: ctx.regions_device(labels.data_ptr(), compact.data_ptr(), c ** 3 * 4, table.data_ptr(), K, aux_ptr=aux.data_ptr(), box=box, stream=stream)
            t_dev = [timed(fn, args.iters) for _ in range(args.repeats)]
            rows = table.cpu().numpy()[:K * ROW].view(vv.REGION_DTYPE)
            t0 = time.perf_counter()
            comp = compact[:c ** 3].cpu().numpy().view(np.uint32).reshape(c, c, c)
            dist = aux[:c ** 3].cpu().numpy().view(np.uint32).reshape(c, c, c)
            t_down = (time.perf_counter() - t0) * 1e6
            index = np.arange(1, K + 1)
            t0 = time.perf_counter()
            ones = np.ones(comp.shape, np.int64)
            h_vox = ndimage.sum_labels(ones, comp, index)
            h_obj = ndimage.find_objects(comp.astype(np.int32))
            h_com = ndimage.center_of_mass(ones, comp, index)
            h_max = ndimage.maximum(dist, comp, index)
            t_host = (time.perf_counter() - t0) * 1e6
            assert np.array_equal(np.asarray(h_vox, np.uint64), rows["voxels"]) and np.array_equal(np.asarray(h_max, np.uint32), rows["aux_max"])
            assert all(tuple(s.start for s in h_obj[k])[::-1] == tuple(rows["lo"][k]) and tuple(s.stop for s in h_obj[k])[::-1] == tuple(rows["hi"][k]) for k in range(K))
            assert np.allclose(np.asarray(h_com)[:, ::-1], rows["sum"] / rows["voxels"][:, None].astype(np.float64), rtol=1e-12, atol=1e-9)
            emit(f"{name} {c}^3 crop bins {bins[0]:3d}..{bins[1]:3d}: {K} regions; scipy.ndimage sum_labels + find_objects + center_of_mass + maximum on the host {t_host:12.1f} us"
                 f" (+ {t_down:10.1f} us to download compact and aux); vv_region_table {spread(t_dev)} us; voxels, boxes, centroids and aux_max agree")
            del table

keys = list(whole_us)
if len(keys) >= 2:
    floor = min(whole_us.values())
    for k in keys:
        emit(f"ratio to the fastest input: {k[0]} bins {k[1]}: {whole_us[k] / floor:6.2f}")
