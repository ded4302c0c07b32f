"""What the tests of the volume-to-volume calls share (test_derive.py, test_stencil.py, test_resample.py): the environment and the volume load, the
report of a mismatch, and the guarded device buffer the calls write into.  Which voxels may differ is each test file's own rule."""
import numpy as np

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
