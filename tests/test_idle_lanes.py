"""march_kernel parks its idle lanes (kParkIdle, vv_layout.h): a lane that has no sample in a slot of the trip loop -- the slot lies past the samples its
chunk holds, or the lane had crossed the ERT threshold when the last trip ended -- gathers texel 0 instead of marching on along its ray.  What a frame
computes does not change; what it gathers does, and the issued set (touched_lines_all = 1, touched_block_lines) shows it.  The tests hold that set to

    compulsory  <=  issued  <=  compulsory  +  the lines of texel 0  +  the lines of at most U - 1 samples past a lane's last live sample of a trip
                                (+ the lines under executed samples outside the volume, which the compulsory set leaves out by definition: _sets)

with the positions from the witness's march (its `visit` callback) and the loads from footprint_model.gathers, on the parked builds a small volume reaches, for both
samples-per-trip values, and at the places where parking can go wrong; pixels and sample counts against the oracle throughout.

  volumes   noise 40 x 36 x 96, values in [0.1, 0.9], as f32 and as its u8 twin (rows of 160 bytes: not line-sized; x and y multiples of 4, not of 8)
  frames    48 x 40 pixels (and 1 x 40, 48 x 120 for the shards), step 1/64: a sample advances 1.5 slices along z, a 30-sample chunk 45 slices
  cameras   along z from beside the centre; the oblique one of tests/test_footprint.py (the z-fastest copy serves that one only)
  builds    forced with the knobs of tests/test_footprint.py (LAYOUTS), checked through last_launch(); U through VV_UNROLL, read back as last_launch()["unroll"]"""
import functools

import numpy as np
import pytest

import footprint_model as FM
import mip_oracle as MO
import oracle_lib as O
import test_footprint as TF
import volviz_amd as vv
import witness as Wt

f32 = np.float32
W, H = 48, 40
STEP = 1.0 / 64
THR = 0.9
CAMS = {"axis": vv.Camera(origin=(0.3, 0.2, -3.0), look_at=(0.3, 0.2, 0.0)), "oblique": TF.CAMS["oblique"]}
# The builds whose march_kernel parks (vv_layout.h: VV_PARK_IDLE) and that a small volume reaches, and the camera each is driven with.  The third parked
# build, brick, samples the bricked copy of volumes beyond 1 GiB only: below that the policy takes the brick_cached build, which does not park and fails
# this bound as the parent's kernel does.  The brick build's frames are held by the full-size rotated frame of tests/test_gpu_parity.py.
PARKED = ("big", "zfast")
CAM_OF = {"big": "axis", "zfast": "oblique"}
UNROLLS = (2, 3)


@functools.lru_cache(maxsize=None)
def _volume(kind):
    v = (np.random.default_rng(7).random((96, 36, 40), dtype=f32) * f32(0.8) + f32(0.1)).astype(f32)
    if kind == "u8":
        v = np.rint(v * f32(255)).astype(np.uint8)
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


def _table(name):
    """opaque: every ray ends within four samples of entering the volume (index >= 1 everywhere: the volume's values are >= 0.1).  graded: a ray crosses
    the threshold after 20 .. 40 samples, around the end of its first chunk.  faint: no ray ever does.  above-one: opacities above 1 (alpha_unit false)."""
    tf = np.zeros((256, 4), f32)
    if name == "opaque":
        tf[1:128] = (0.8, 0.7, 0.6, 0.5); tf[128:] = (0.3, 0.9, 0.4, 1.0)
    elif name == "graded":
        tf[1:128] = (0.8, 0.7, 0.6, 0.05); tf[128:] = (0.3, 0.9, 0.4, 0.12)
    elif name == "faint":
        tf[1:] = (0.8, 0.7, 0.6, 0.004)
    else:
        assert name == "above-one"
        tf[1:128] = (0.8, 0.7, 0.6, 0.06); tf[128:] = (0.3, 0.9, 0.4, 1.5)
    return tf.reshape(1024)


class _Chunks:
    """`visit` callback of witness.render: every chunk's texture coordinates [rays, 32, 3] and which of its samples ran [rays, 32]."""
    def __init__(self):
        self.tex, self.ran = [], []

    def __call__(self, tex, ran, started):
        self.tex.append(np.array(tex, f32)); self.ran.append(np.array(ran, bool))


def _case(tf="opaque", ert_mode=vv.ERT_REFERENCE, slice_type=vv.SLICE_NONE, shard=None, size=(W, H), tail=1):
    return (tf, ert_mode, slice_type, shard, size, tail)


PLANE = ((0.5, 0.5, 0.4), (0.3, 0.2, 1.0))


@functools.lru_cache(maxsize=None)
def _frame_model(kind, cam_name, case):
    """The witness's frame of a case: rgba, executed samples, the chunks; and the oracle's frame, which must agree with it."""
    tf, ert_mode, slice_type, shard, size, _ = case
    vol, cam = _volume(kind), CAMS[cam_name]
    ch = _Chunks()
    rgba, n = Wt.render(vol, _table(tf), size[0], size[1], visit=ch, step=STEP, ert_threshold=THR, ert_mode=ert_mode, slice_type=slice_type,
                        plane=PLANE[0] + PLANE[1], shard=shard, **TF._cam_kw(cam))
    o_rgba, o_n = O.render(vol, _table(tf), size[0], size[1], cam, slice=vv.make_slice_params(slice_type, *PLANE),
                           options=vv.make_options(step=STEP, ert_threshold=THR, ert_mode=ert_mode, shard=shard))
    assert o_n == n and np.array_equal(o_rgba, rgba), (kind, cam_name, case, o_n, n)
    return o_rgba, o_n, ch


def _last_live(ran):
    """[rays]: the last sample of the chunk that ran, 0 where none did."""
    return np.where(ran.any(axis=1), 31 - np.argmax(ran[:, ::-1], axis=1), 0)


def _lines_at(tex, model, dtype, geom, dims, bits):
    """The lines under the gathers of samples at tex [n, 3], in the volume or not: the fetch clamps the base texel, and so does base_texels."""
    if len(tex) == 0:
        return FM._words([], bits)
    ix, iy, iz = FM.base_texels(np.asarray(tex, f32), dims)
    got = []
    for off, length in FM.gathers(model, dtype, geom, ix, iy, iz):
        got += [off >> 7, (off + length - 1) >> 7]
    return FM._words(np.concatenate(got), bits)


def _sets(ch, U, model, dtype, geom, dims, bits):
    """(compulsory, allowed, what the parent's kernel marks at least, what the executed samples outside the volume add to the bound) as bitmaps of `bits`
    lines.  allowed = compulsory + texel 0 + the samples L + 1 .. the end of L's trip, L a lane's last live sample of a chunk (trips are i0 = 1, 1 + U, ...:
    the same for every lane) + the lines under executed samples outside the volume: such a sample is live, its gathers are issued where the fetch clamps
    it to, and the compulsory bitmap does not hold it by definition.  From the axis camera that last term adds nothing (asserted below); from the oblique
    one the rays' way through the empty cube in front of the volume adds lines on the volume's faces.
    The parent's lanes march on to the longest n of their wave, at least to their own: a lane that stopped at L < 30 gathers its
    entries L + 1 .. 30 as far as they lie in the volume (a position in the volume lies before the ray's end)."""
    executed, overrun, onward = [], [], []
    for tex, ran in zip(ch.tex, ch.ran):
        executed.append(tex[ran])
        L = _last_live(ran)
        has = L > 0
        trip_end = (L + U - 1) // U * U
        for k in range(1, U):
            sel = has & (L + k <= trip_end)
            overrun.append(tex[sel, (L + k)[sel]])
        for i in range(2, 31):
            sel = has & (L < i)
            onward.append(tex[sel, i])
    executed = np.concatenate(executed); overrun = np.concatenate(overrun); onward = np.concatenate(onward)
    onward = onward[FM.in_volume(onward)]
    inside = FM.in_volume(executed)
    args = (model, dtype, geom, dims, bits)
    compulsory = _lines_at(executed[inside], *args)
    outside = _lines_at(executed[~inside], *args)
    allowed = compulsory | _lines_at(np.zeros((1, 3), f32), *args) | _lines_at(overrun, *args)
    return compulsory, allowed | outside, _lines_at(onward, *args), outside & ~allowed


def _slices(words, geom):
    """The z slices of the linear layout that the set lines of a bitmap begin in."""
    ln = np.flatnonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little"))
    return np.unique(ln * 128 // geom["slice"])


def _geom(kind, layout_name):
    vol = _volume(kind)
    return FM.dense_geom(TF.LAYOUTS[layout_name][2], vol.dtype, TF._dims(vol))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: every case is a working detector -- with the model, not with a second library
# ---------------------------------------------------------------------------------------------------------------------
def _stops(ch, U):
    """Where the rays of a frame stop, from the witness's chunks: (ERT stops on the last slot of a trip, ERT stops on sample 30 whose next chunk runs
    one sample, ray ends with n < 30 that are not the last slot of a trip, ERT stops inside a chunk after the first)."""
    last_slot = on_30 = mid_trip = later = 0
    for c, (tex, ran) in enumerate(zip(ch.tex, ch.ran)):
        L = _last_live(ran)
        rows = np.arange(len(L))
        nxt_in = FM.in_volume(tex[rows, np.minimum(L + 1, 31)])
        ert_stop = (L > 0) & (L < 30) & nxt_in                     # the next position lies in the volume, before the ray's end: the threshold stopped it
        last_slot += int((ert_stop & (L % U == 0)).sum())
        mid_trip += int(((L > 0) & (L < 30) & ~nxt_in & (L % U != 0)).sum())
        later += int((ert_stop & (L > 1)).sum()) if c > 0 else 0
        if c + 1 < len(ch.ran):
            n_next = ch.ran[c + 1].sum(axis=1)
            on_30 += int(((L == 30) & (n_next == 1) & FM.in_volume(ch.tex[c + 1][:, 2])).sum())
    return last_slot, on_30, mid_trip, later


@pytest.mark.parametrize("kind", ("f32", "u8"))
@pytest.mark.parametrize("cam_name", ("axis", "oblique"))
def test_the_opaque_case_is_a_working_detector(kind, cam_name):
    """Every ray of the opaque frame ends inside its first chunk, in both ERT modes.  On the linear layout the bound then reaches a few slices behind the
    volume's front (axis camera, f32, U = 3: slices 0 .. 11 of 96), while the parent's kernel, which marches every lane of a wave to the end of the chunk,
    marks lines in every slice up to 45 -- the depth of one chunk -- beyond it: the model of what the parent marks has lines outside the bound on every
    layout (more than 5 % of the copy's lines), in more than 20 further slices on the linear one.  From the axis camera the executed samples outside the volume add no line to the bound."""
    vol = _volume(kind)
    dims = TF._dims(vol)
    for ert_mode in (vv.ERT_REFERENCE, vv.ERT_TRUE):
        _, n, ch = _frame_model(kind, cam_name, _case("opaque", ert_mode))
        assert n > 1000
        first = _last_live(ch.ran[0])
        assert ((first > 0) & (first < 30)).sum() > 500
        # No ray takes more than four samples in the volume before it stops.  From the axis camera every ray that marches stops inside chunk 0, and the later
        # chunks hold sample 1 of a stopped ray or nothing.  (From the oblique camera the rays along the silhouette march through more than a chunk of empty
        # cube before they enter the volume -- they start on their slab's sphere -- and stop there.)
        if ert_mode == vv.ERT_TRUE:
            assert sum((ran & FM.in_volume(tex)).sum(axis=1) for tex, ran in zip(ch.tex, ch.ran)).max() <= 4
        if cam_name == "axis":
            assert not (first >= 30).any()
            for ran in ch.ran[1:]:
                assert (ran.sum(axis=1) <= 1).all() and (ert_mode == vv.ERT_REFERENCE or not ran.any())
        for U in UNROLLS:
            for layout_name in PARKED:
                if cam_name == "axis" and layout_name == "zfast":
                    continue
                geom = _geom(kind, layout_name)
                bits = TF._line_bits(geom)
                compulsory, allowed, parent, outside = _sets(ch, U, TF.LAYOUTS[layout_name][2], vol.dtype, geom, dims, bits)
                assert cam_name != "axis" or not outside.any(), (layout_name, U)
                beyond = parent & ~allowed
                # (f32, from the camera its edge cases run with: the small linear copy seen obliquely, and the u8 copies, whose lines hold 128 voxels, are
                # touched nearly whole by the bound alone -- the u8 twin is a detector on the linear layout from the axis camera, below)
                if cam_name == CAM_OF[layout_name] and kind == "f32":
                    assert FM.bit_count(beyond) * 20 > geom["alloc"] // 128, (layout_name, U, FM.bit_count(beyond), FM.bit_count(allowed))
                if layout_name == "big" and cam_name == "axis":
                    a, b = _slices(allowed, geom), _slices(beyond, geom)
                    print(f"{kind} {cam_name} ert {ert_mode} U {U}: the bound reaches slices {a.min()} .. {a.max()}, the parent marks {b.min()} .. {b.max()} beyond it")
                    assert len(np.setdiff1d(b, a)) > 20 and (ert_mode == vv.ERT_REFERENCE or (a.max() < 16 and b.max() >= 40))


EDGE_CASES = {
    # graded opacity: threshold crossings on every slot of a trip, on sample 30 (the next chunk then holds one sample), in the second chunk
    "graded": _case("graded"),
    "graded-ert-true": _case("graded", vv.ERT_TRUE),
    "graded-no-tail": _case("graded", tail=0),
    "opaque-no-tail": _case("opaque", tail=0),
    # no ray stops: rays end with n < 30, mid-trip
    "faint": _case("faint"),
    "faint-ert-true": _case("faint", vv.ERT_TRUE),
    # opacities above 1: a later chunk is marched in full again after a stop
    "above-one": _case("above-one"),
    "above-one-ert-true": _case("above-one", vv.ERT_TRUE),
    "plane": _case("graded", slice_type=vv.SLICE_PLANE),
    # two interleaved shards of a 48 x 120 frame (9 slab rows in bands of 4: shard 0 owns slab rows 0 .. 3 and 8, shard 1 rows 4 .. 7)
    "shard-0-of-2": _case("graded", shard=(4, 2, 0), size=(W, 120)),
    "shard-1-of-2": _case("graded", shard=(4, 2, 1), size=(W, 120)),
    "one-wide": _case("graded", size=(1, H)),
}


@pytest.mark.parametrize("cam_name", ("axis", "oblique"))
def test_the_edge_cases_hold_the_edges(cam_name):
    """The frames of EDGE_CASES contain what they are there for, by the witness's chunks."""
    for U in UNROLLS:
        last_slot, on_30, mid_trip, later = _stops(_frame_model("f32", cam_name, EDGE_CASES["graded"])[2], U)
        assert last_slot > 20 and on_30 > 0 and later > 20, (U, last_slot, on_30, later)
        last_slot, on_30, mid_trip, later = _stops(_frame_model("f32", cam_name, EDGE_CASES["faint"])[2], U)
        assert mid_trip > 20 and last_slot == 0 and on_30 == 0, (U, mid_trip, last_slot)
        # above 1: a ray that stopped runs more than one sample of a later chunk again
        ch = _frame_model("f32", cam_name, EDGE_CASES["above-one"])[2]
        again = sum(int(((_last_live(a) < 30) & (_last_live(a) > 0) & (b.sum(axis=1) > 1)).sum()) for a, b in zip(ch.ran[:-1], ch.ran[1:]))
        assert again > 20, again
    assert _frame_model("f32", cam_name, EDGE_CASES["one-wide"])[1] > 0
    a, b = (_frame_model("f32", cam_name, EDGE_CASES[k])[1] for k in ("shard-0-of-2", "shard-1-of-2"))
    assert a > 0 and b > 0 and a + b == _frame_model("f32", cam_name, _case("graded", size=(W, 120)))[1]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _check(ctx, kind, layout_name, cam_name, case, U, what):
    """One case on one build with U samples per trip: pixels and the sample count against the oracle (uninstrumented and instrumented frame), the
    compulsory bitmap against the model, and the three properties of the issued set."""
    tf, ert_mode, slice_type, shard, size, tail = case
    knobs, code, model, _, _ = TF.LAYOUTS[layout_name]
    vol, cam = _volume(kind), CAMS[cam_name]
    dims = TF._dims(vol)
    geom = _geom(kind, layout_name)
    bits = TF._line_bits(geom)
    want_rgba, want_n, ch = _frame_model(kind, cam_name, case)
    compulsory, allowed, _, _ = _sets(ch, U, model, vol.dtype, geom, dims, bits)
    sp = vv.make_slice_params(slice_type, *PLANE)
    okw = dict(step=STEP, ert_threshold=THR, ert_mode=ert_mode, shard=shard)
    with MO.knobs(ctx, dict(knobs, VV_UNROLL=str(U), VV_TAIL=str(tail))):
        ctx.load_volume(vol, _table(tf))
        plain = ctx.render(size[0], size[1], cam, slice=sp, options=vv.make_options(**okw))
        lay = ctx.last_launch()
        assert lay["layout"] == code and lay["unroll"] == U and lay["phong"] == 0, (what, lay)
        assert np.array_equal(plain, want_rgba), what + ": pixels of the uninstrumented frame"
        ins = TF._Instruments(dims, bits)
        counted = ctx.render(size[0], size[1], cam, slice=sp, options=ins.options(**okw))
        assert ctx.last_sample_count() == want_n, (what, ctx.last_sample_count(), want_n)
        assert np.array_equal(counted, plain), what + ": the instrumented frame differs from the uninstrumented one"
        _, got, _ = ins.read()
        TF._same_words(got, compulsory, what + ": touched_lines")
        ins = TF._Instruments(dims, bits, pairs=True)
        every = ctx.render(size[0], size[1], cam, slice=sp, options=ins.options(lines_all=True, **okw))
        lay = ctx.last_launch()
        assert lay["layout"] == code and lay["unroll"] == U, (what, lay)
        assert np.array_equal(every, plain), what + ": the frame that records the issued set differs"
        _, issued, table = ins.read()
    print(f"{what}: samples {want_n}, lines compulsory {FM.bit_count(compulsory)} <= issued {FM.bit_count(issued)} <= bound {FM.bit_count(allowed)}")
    assert FM.contains(issued, compulsory), what + ": the issued set does not contain the compulsory one"
    extra = issued & ~allowed
    assert not extra.any(), f"{what}: {FM.bit_count(extra)} issued lines outside the bound, first at line {int(np.flatnonzero(extra)[0]) * 32}"
    keys = table[table != 0]
    line_of = (keys & np.uint64((1 << 36) - 1)).astype(np.int64)
    TF._same_words(FM._words(np.unique(line_of), bits), issued, what + ": lines of touched_block_lines against the issued bitmap")


@pytest.mark.gpu
@pytest.mark.parametrize("layout_name", PARKED)
@pytest.mark.parametrize("kind", ("f32", "u8"))
def test_issued_set_of_rays_that_end_in_their_first_chunk(ctx, kind, layout_name):
    """Opaque table, both ERT modes, U = 2 and 3, both cameras the build serves: the issued bitmap contains the compulsory one, lies inside the bound, and
    is exactly the distinct lines of touched_block_lines.  (The parent's kernel marks the rest of the first chunk, down to slice 45 of the linear layout:
    test_the_opaque_case_is_a_working_detector.)"""
    cams = ("oblique",) if layout_name == "zfast" else ("axis", "oblique")
    for cam_name in cams:
        for ert_mode in (vv.ERT_REFERENCE, vv.ERT_TRUE):
            for U in UNROLLS:
                _check(ctx, kind, layout_name, cam_name, _case("opaque", ert_mode), U, f"{kind} {layout_name} {cam_name} opaque ert {ert_mode} U {U}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout_name", PARKED)
@pytest.mark.parametrize("case_name", list(EDGE_CASES))
def test_edge_cases(ctx, case_name, layout_name):
    """The same properties, with pixels and last_sample_count() against the oracle, where parking can go wrong (EDGE_CASES; what each frame holds:
    test_the_edge_cases_hold_the_edges)."""
    for U in UNROLLS:
        _check(ctx, "f32", layout_name, CAM_OF[layout_name], EDGE_CASES[case_name], U, f"f32 {layout_name} {case_name} U {U}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout_name", PARKED)
def test_instrumented_frames_equal_uninstrumented_ones(ctx, layout_name):
    """An instrumented and an uninstrumented frame of the same case are equal pixel for pixel (u8 twin, graded table, both ERT modes; _check compares
    the two on every other case as well)."""
    for ert_mode in (vv.ERT_REFERENCE, vv.ERT_TRUE):
        _check(ctx, "u8", layout_name, CAM_OF[layout_name], _case("graded", ert_mode), 3, f"u8 {layout_name} graded ert {ert_mode}")
