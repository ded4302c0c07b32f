"""The kernels' arithmetic helpers swept on the GPU (volume-viz_amd/host/device_math_check.hip): the Phong division and square-root cores, the
texture coordinate and its TEX8 weight, the bounds test, the index / channel conversions and the chunk count, each against a binary64 or integer
definition written in the check itself.  What an 8-bit frame cannot see: a wrong last bit in these places almost never moves a pixel.

Each GPU test runs one sweep in a child process and holds it to: exit status 0; no mismatch (`bounds`: exactly the pattern of -0.0); the number of
inputs the sweep reports equal to the number this file computes from the sweep's definition (a sweep that ran nothing fails); and the same sweep
over a deliberately wrong twin of the helper reporting mismatches (a sweep that cannot tell a wrong helper apart fails).

Time limits: four times the wall time of the child measured on an MI355X (profiles/EXPERIMENTS.md), start-up included."""
from __future__ import annotations

import json
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.normpath(os.path.join(HERE, ".."))
BINARY = os.path.join(REPO, "volume-viz_amd", "bin", "device_math_check")
SWEEPS = ["div", "sqrt", "axis", "bounds", "convert", "chunks"]

# the limits of vv_render's gates (csrc/vv_gate.h), restated: the ranges below are derived from them here as the check derives them there
STEP_MIN, STEP_MAX, TAN_LO, TAN_HI, SQRT3 = float(np.float32(1e-5)), 16.0, 2.0 ** -24, 2.0 ** 8, float(np.float32(1.73205081))
FEW_ULPS = 2.0 ** -20


def numerators():
    """Every value q255[i] - q255[j] in binary32, each once."""
    q = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.unique((q[:, None] - q[None, :]).astype(np.float32).view(np.uint32)).view(np.float32)


def denominator_binades():
    s_lo, s_hi = STEP_MIN * (1 - FEW_ULPS), STEP_MAX * (1 + FEW_ULPS)
    vd_lo, vd_hi = s_lo, SQRT3 + 30 * s_hi
    d_lo, d_hi = min(TAN_LO * vd_lo, 2 * s_lo), max(TAN_HI * vd_hi, 2 * s_hi)
    n = numerators()
    n_min = float(np.abs(n[n != 0]).min())
    # ... and the denominators of the quotient range the kernel's comment states, [2^-26, 2^42]
    lo = min(math.floor(math.log2(d_lo)), math.floor(math.log2(1.0 / 2.0 ** 42)))
    hi = max(math.floor(math.log2(d_hi)), math.floor(math.log2(n_min / 2.0 ** -26)))
    return lo, hi


AXIS_EXTRAS = 22          # -0, negative denormals and normals, 1 and beyond, +-Inf, three NaNs (the list is in the check)


def expected_visits(name):
    if name == "div":
        lo, hi = denominator_binades()
        return len(numerators()) * (hi - lo + 1) * 2 ** 23
    if name == "sqrt":
        return (86 - (-52) + 1) * 2 ** 23                       # every binary32 in [2^-52, 2^87)
    if name == "axis":
        return 12 * 2 * (0x3F800000 + AXIS_EXTRAS)              # sizes x {exact, TEX8} x (every pattern of [0, 1) + the out-of-range list)
    if name in ("bounds", "convert"):
        return 3 * 2 ** 32
    if name == "chunks":
        return 2 ** 28 + 2 ** 20 * 32 * 5 + 1024 + 1024
    raise KeyError(name)


# seconds: 4 x the measured wall time of `device_math_check --self-test <sweep>` on an MI355X, rounded up
# measured: div 2.51, axis 0.48, bounds 0.36, convert 0.31, chunks 0.30, sqrt 0.26
TIMEOUT = {"div": 11, "sqrt": 2, "axis": 2, "bounds": 2, "convert": 2, "chunks": 2}


def test_binary_is_built_and_lists_the_six_sweeps():
    assert os.access(BINARY, os.X_OK), BINARY
    r = subprocess.run([BINARY, "--list"], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == SWEEPS


def test_swept_ranges_follow_from_the_gate():
    """The header the gate and the check share still says what this file restates; the derived binades are the ones the sweeps are counted with."""
    text = open(os.path.join(REPO, "volume-viz_amd", "csrc", "vv_gate.h")).read()
    for line in ("kStepMin = 1e-5f;", "kSafeDivTanLo = 0x1p-24f;", "kSafeDivTanHi = 0x1p8f;", "kSafeDivStepMax = 16.f;"):
        assert line in text, line
    assert denominator_binades() == (-42, 18)
    assert len(numerators()) == 1195 and 0.0 in numerators() and numerators().min() == -1.0 and numerators().max() == 1.0


def run_sweep(name):
    r = subprocess.run([BINARY, "--self-test", name], capture_output=True, text=True, timeout=TIMEOUT[name])
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["sweep"] == name, r.stdout + r.stderr
    print(r.stdout)
    return r, lines[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s for s in SWEEPS if s != "bounds"])
def test_sweep_is_clean(name):
    r, out = run_sweep(name)
    assert out["visited"] == expected_visits(name), out
    assert out["mismatches"] == 0, out
    assert out["first"] == [], out
    assert out["self_test_mismatches"] > 0, out
    if name == "div":
        assert (out["binade_lo"], out["binade_hi"]) == denominator_binades() and out["numerators"] == len(numerators()), out
    if name == "sqrt":
        assert out["root_mismatches"] == 0 and out["reciprocal_mismatches"] == 0, out
        assert out["self_test_without_lower_test"] > 0, out      # both of the core's neighbour tests are live
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_bounds_sweep_disagrees_on_minus_zero_only():
    """bounds_check reads the bit pattern: over all 2^32 patterns in each coordinate it differs from x >= 0 && x < 1 on -0.0 and on nothing else."""
    r, out = run_sweep("bounds")
    assert out["visited"] == expected_visits("bounds"), out
    assert out["disagreeing_patterns"] == ["0x80000000"], out
    assert out["mismatches"] == 3, out                           # once per coordinate
    assert sorted((m[0], m[1]) for m in out["first"]) == [("0x80000000", f"0x{c:08x}") for c in range(3)], out
    assert out["self_test_mismatches"] > 3, out                  # the twin that admits 1.0
    assert r.returncode == 0, r.stdout + r.stderr
