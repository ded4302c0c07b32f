"""What the tests of the volume-to-volume calls share (test_derive.py, test_stencil.py, test_resample.py): the environment and the volume load, the
report of a mismatch, and the guarded device buffer the calls write into.  Which voxels may differ is each test file's own rule.

And what the tests of the label, distance, region-table and mesh calls share on top of that (test_label.py, test_distance.py, test_regions.py,
test_mesh.py): the guarded device buffer of a call with several outputs (GuardedOuts), the layout sweep (layout_sweep, layout_context), the two
load paths that are not load_volume (load_paths), and the frame of the errors_and_state tests (Untouched, free_memory_unchanged)."""
import collections
import contextlib

import numpy as np
import pytest

import volviz_amd as vv

GARBAGE = 0xA5
GUARD = 64                                                 # bytes before and behind the output that must keep GARBAGE


def clear_env(monkeypatch, knobs):
    for k in knobs:
        monkeypatch.delenv(k, raising=False)


def load(ctx, monkeypatch, knobs, vol, tf):
    """`vol` loaded under an environment without `knobs` (the knobs are read at volume load and by reread_env)."""
    clear_env(monkeypatch, knobs)
    ctx.reread_env()
    ctx.load_volume(vol, tf)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def report(got, want, bad, what):
    """Fails with the first of the voxels `bad` (indices (z, y, x), as np.argwhere gives them) at which got and want differ; passes if there is none."""
    if len(bad):
        i = tuple(bad[0])
        g, w = got[i], want[i]
        if got.dtype == np.float32:
            g, w = f"{g!r} ({int(np.asarray(g).view(np.uint32)):#x})", f"{w!r} ({int(np.asarray(w).view(np.uint32)):#x})"
        raise AssertionError(f"{what}: {len(bad)} of {got.size} voxels differ, first at (z, y, x) = {i}: {g} vs {w}")


class DeviceOut:
    """A device buffer the calls write into: GARBAGE everywhere before each call, the output GUARD bytes in plus an offset that changes from
    call to call (0, 4, 8, 12 bytes; u8 outputs 0, 1, 2, 3); the bytes before and behind it must survive."""

    def __init__(self, nbytes):
        import torch
        self.torch = torch
        self.buf = torch.empty(nbytes + 2 * GUARD + 16, dtype=torch.uint8, device=torch.device("cuda", 0))
        self.calls = 0

    def run(self, call, shape, dtype, what):
        """call(out_ptr, capacity) -> the output's (bx, by, bz), complete on return; gives the output as an array of `shape` = (bz, by, bx)."""
        self.calls += 1
        off = GUARD + (self.calls % 4) * (4 if dtype == np.float32 else 1)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert off + nbytes + GUARD <= self.buf.numel()
        self.buf.fill_(GARBAGE)
        self.torch.cuda.synchronize()
        m = call(self.buf.data_ptr() + off, nbytes)
        assert tuple(m) == tuple(shape[::-1])
        raw = self.buf.cpu().numpy()
        assert (raw[:off] == GARBAGE).all() and (raw[off + nbytes:] == GARBAGE).all(), f"bytes outside the output were written ({what})"
        return raw[off:off + nbytes].copy().view(dtype).reshape(shape)


# ---- calls with several outputs ------------------------------------------------------------------------------------------------------------
# One output of a call, as GuardedOuts lays it out: `capacity` bytes are set aside for it, of which the call writes the first `written` (None: all of
# them; a table with rows to spare: fewer); its start is a multiple of `align` that visits the residues 0, 4, 8, 12 (align 4), 0, 8 (align 8) or
# 0, 16 (align 16) as the digit `digit` of the call count moves (digit 1: every call, 2: every second ...); absent: the call gets a NULL pointer.
Out = collections.namedtuple("Out", "capacity written align digit present", defaults=(None, 4, 1, True))


class GuardedOuts:
    """The guarded device buffer of a call with several outputs: GARBAGE everywhere before each call; the outputs lie GUARD bytes apart in list
    order, each at a start that moves from call to call on a digit of its own; every byte outside the written parts of the present outputs -- the
    guards, the rows beyond `written`, the room of an absent output -- must survive."""

    def __init__(self, nbytes, align):
        import torch
        self.torch = torch
        self.tdev = torch.device("cuda", 0)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.tdev)
        assert self.buf.data_ptr() % align == 0
        self.calls = 0

    def upload(self, a):
        """A word array as a device tensor (an input of the call)."""
        return self.torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(self.tdev)

    def run_outs(self, call, outs, what=""):
        """call(ptrs), complete on return, gets one device pointer per entry of `outs` (0: absent) -> the written bytes of each (None: absent)."""
        self.calls += 1
        end, spans = 0, []
        for o in outs:
            assert o.align in (4, 8, 16)
            start = -(-(end + GUARD) // o.align) * o.align + o.align * ((self.calls // o.digit) % (4 if o.align == 4 else 2))
            end = start + o.capacity
            spans.append((start, o.capacity if o.written is None else o.written))
            assert spans[-1][1] <= o.capacity
        assert end + GUARD <= self.buf.numel()
        self.buf.fill_(GARBAGE)
        self.torch.cuda.synchronize()
        base = self.buf.data_ptr()
        call([base + s if o.present else 0 for (s, _), o in zip(spans, outs)])
        self.torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        keep = np.ones(raw.size, bool)
        for (s, w), o in zip(spans, outs):
            if o.present:
                keep[s:s + w] = False
        assert (raw[keep] == GARBAGE).all(), f"bytes outside the outputs were written ({what})"
        return [raw[s:s + w].copy() if o.present else None for (s, w), o in zip(spans, outs)]


# ---- the layout sweep ------------------------------------------------------------------------------------------------------------------------
def layout_sweep(test):
    """The parametrisation of the test_*_layouts tests: four layout knobs x (u8 rows of 64 voxels, f32 rows of 20: a multiple of 16 bytes is re-pitched)."""
    knobs = [{"VV_PITCH_FORCE": "1"}, {"VV_PITCH_FORCE": "1", "VV_PITCH_ROWS": "1"}, {"VV_PITCH_FORCE": "1", "VV_FORCE_BIG": "1"}, {"VV_FORCE_BIG": "1"}]
    test = pytest.mark.parametrize("knobs", knobs, ids=["pitch", "pitch_rows", "pitch_big", "big"])(test)
    return pytest.mark.parametrize("kind,nx", [("u8", 64), ("f32", 20)])(test)


@contextlib.contextmanager
def layout_context(kind, nx, knobs, monkeypatch, layout_knobs, tf):
    """(context, volume) of one cell of the sweep: a context created under the knobs, holding a nx x 11 x 10 volume without a zero (so that padding
    read as data shows), re-pitched where the knobs say so: 32 bytes of zeros behind every row, with VV_PITCH_ROWS an extra row of zeros per slice."""
    clear_env(monkeypatch, layout_knobs)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ny, nz = 11, 10
    vol = np.random.default_rng(43).integers(1, 256, (nz, ny, nx), dtype=np.uint8)
    if kind == "f32":
        vol = (vol.astype(np.float32) / np.float32(255)).astype(np.float32)
    with vv.Context(0) as c:                                    # a context created under the environment
        c.load_volume(vol, tf)
        if "VV_PITCH_FORCE" in knobs:
            row = nx * vol.itemsize + 32
            rows = ny + 1 if "VV_PITCH_ROWS" in knobs else ny
            assert c.device_bytes()[0] == nz * rows * row + rows * row + 2 * row + 4096             # the volume is re-pitched
        yield c, vol


# ---- the load paths --------------------------------------------------------------------------------------------------------------------------
def load_paths(ctx, monkeypatch, layout_knobs, vol8, tf):
    """Loads the u8 volume `vol8` twice and yields (what, the volume the context now holds) after each: from a device buffer (a torch tensor that is
    gone before the caller's calls run), then promoted to f32 by the streamed upload, its slabs out of order."""
    import torch
    clear_env(monkeypatch, layout_knobs)
    ctx.reread_env()
    nz, ny, nx = vol8.shape
    t = torch.from_numpy(vol8.copy()).to(torch.device("cuda", 0))
    ctx.load_volume_device(t.data_ptr(), vv.VOXEL_U8, nx, ny, nz, tf)
    torch.cuda.synchronize()
    del t
    yield "load_volume_device", vol8
    ctx.load_volume_streamed([(4, vol8[4:]), (0, vol8[:4])], vv.VOXEL_F32, nx, ny, nz, tf)
    yield "streamed upload with promotion", (vol8.astype(np.float32) / np.float32(255)).astype(np.float32)


# ---- the frame of the errors_and_state tests -------------------------------------------------------------------------------------------------
class Untouched:
    """What a context shows of itself before a run of refused and accepted calls -- a frame, the volume's histogram, the layout state, the device
    bytes, the frame time -- and the assertion that it shows the same afterwards: volume, layout copies, residency, scratch, frame time."""

    def __init__(self, ctx):
        self.ctx, self.cam = ctx, vv.Camera.orbit(3.0, 1.0, 0.6)
        self.frame = ctx.render(57, 43, self.cam, fill=1)
        self.hist = ctx.histogram()
        self.state, self.dbytes, self.ms = ctx.layout_state(), ctx.device_bytes(), ctx.last_frame_ms()

    def check(self):
        import test_hist as TH
        ctx = self.ctx
        assert ctx.layout_state() == self.state and ctx.device_bytes() == self.dbytes and ctx.last_frame_ms() == self.ms
        TH._same(ctx.histogram(prefill=GARBAGE), self.hist, "the volume's histogram after the calls")
        assert np.array_equal(ctx.render(57, 43, self.cam, fill=1), self.frame)
        assert ctx.layout_state() == self.state and ctx.device_bytes() == self.dbytes


def free_memory_unchanged(calls, what="a device call"):
    """`calls()` makes device-output calls: a second round of them leaves the device's free bytes what they were after the first (no allocation)."""
    import torch
    tdev = torch.device("cuda", 0)
    calls()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(tdev)[0]
    calls()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(tdev)[0] == free_before, f"{what} changed the device's free memory"
