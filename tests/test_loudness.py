"""Integrated loudness, host side (no GPU needed): the launch plan of vrvq_loudness, its
coefficients and chunk transition matrices, the argument errors, the CPU route of
vrvq_amd.loudness, and the tie between the long-double reference (tests/loudness_ref.py) and the
host yardstick codec.loudness on the inputs the GPU tests use."""
import ctypes
import math
import os
import unittest.mock

import numpy as np
import pytest
import torch

import loudness_cases as cases
import loudness_ref
import vrvq_amd
from vrvq_amd import _lib, codec

RATES = (44100, 48000, 16000, 11025)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "vrvq.h")
LD = np.longdouble


def test_version_and_constants():
    assert _lib.load().vrvq_version() >= 108
    src = open(HEADER).read()
    assert f"#define VRVQ_LOUDNESS_CHUNK {_lib.LOUDNESS_CHUNK}\n" in src
    assert f"#define VRVQ_LOUDNESS_PLAN_LEN {_lib.LOUDNESS_PLAN_LEN}\n" in src
    assert cases.CHUNK == _lib.LOUDNESS_CHUNK


@pytest.mark.parametrize("sr", RATES)
def test_plan_geometry(sr):
    """win = int(0.4 sr), step = int(0.1 sr), the padding rule and the block count, either side
    of 0.5 s."""
    for nt in (1, 5000, int(0.5 * sr) - 1, int(0.5 * sr), 3 * sr + 17):
        for nch in (1, 5):
            p = _lib.loudness_plan(sr, nch, nt)
            eff = nt + int((0.5 - nt / sr) * sr) if nt / sr < 0.5 else nt
            win, step = int(0.4 * sr), int(0.1 * sr)
            assert (p["eff_length"], p["win"], p["step"]) == (eff, win, step), (sr, nt)
            assert (eff, win, step, p["blocks"]) == loudness_ref.geometry(nt, sr)
            assert p["blocks"] == (eff - win) // step + 1 >= 1
            assert p["chunk"] == _lib.LOUDNESS_CHUNK
            assert p["chunks"] == -(-eff // p["chunk"])
            # partial sums are cut at the chunk edges and where a block begins or ends: one or
            # two cuts per step
            cuts = (eff - 1) // step * (1 if win % step == 0 else 2) + 2
            assert p["chunks"] <= p["pieces"] <= p["chunks"] + cuts
            # the workspace holds chunk states and partial sums, nothing of the signal's size
            assert p["ws_bytes"] % 8 == 0
            assert p["ws_bytes"] <= 8 * (nch * (4 * p["chunks"] + 2 * p["pieces"] + p["blocks"])
                                         + p["blocks"])
            assert p["ws_bytes"] < 4 * nch * eff / 4 + 4096
    assert int(0.4 * 11025) != 4 * int(0.1 * 11025)  # the rate at which win != 4 step


@pytest.mark.parametrize("sr", RATES)
def test_plan_coefficients(sr):
    """The ten normalised coefficients are codec._biquad's (the same float64 operations; one ulp
    is allowed for a libm that rounds sin / cos / pow differently)."""
    p = _lib.loudness_plan(sr, 1, sr)
    for key, (kind, g, q, fc) in zip(("shelf", "highpass"), loudness_ref.STAGES):
        b, a = codec._biquad(kind, g, q, fc, sr)
        want = np.array([b[0], b[1], b[2], a[1], a[2]])
        got = np.array(p[key])
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))), (key, got, want)


def _step_matrix(p, num):
    """The zero-input cascade's 4 x 4 step matrix over (s0, s1, t0, t1) from the plan's own
    coefficients, in the number type `num`: y1 = s0 feeds the second stage."""
    b0, b1, b2, a1, a2 = (num(v) for v in p["highpass"])
    zero, one = num(0), num(1)
    return [[-num(p["shelf"][3]), one, zero, zero],
            [-num(p["shelf"][4]), zero, zero, zero],
            [b1 - a1 * b0, zero, -a1, one],
            [b2 - a2 * b0, zero, -a2, zero]]


def _blocks(p):
    got = np.zeros((4, 4))
    got[:2, :2], got[2:, 2:], got[2:, :2] = p["M1"], p["M2"], p["K"]
    return got


@pytest.mark.parametrize("sr", RATES)
def test_plan_transition_matrices(sr):
    """M1, M2 and the coupling K are the blocks of the chunk-th power of the step matrix in long
    double (numpy.linalg.matrix_power on a longdouble array), rounded once: within 2 ulp of it,
    entry by entry. The same power in float64 is not: it is what loses 5-7e-12 LU through the high
    pass's double pole near 0.995 (Loudness)."""
    p = _lib.loudness_plan(sr, 2, 3 * sr)
    m = np.array(_step_matrix(p, LD), LD)
    r = np.linalg.matrix_power(m, p["chunk"])
    assert r.dtype == LD and np.all(r[:2, 2:] == 0)  # the first stage does not hear the second
    got = _blocks(p)
    ulp = np.spacing(np.abs(r.astype(np.float64))).astype(LD)
    assert np.all(np.abs(got.astype(LD) - r) <= 2 * ulp), (got, r)
    r64 = np.linalg.matrix_power(m.astype(np.float64), p["chunk"])
    assert np.abs(r64 - r).max() > 2 * ulp.max()  # why long double: float64 is tens of ulp off


@pytest.mark.parametrize("sr", RATES + (8000, 96000, 192000))
def test_plan_transition_matrices_against_the_exact_power(sr):
    """The same entries against the exact power (rational arithmetic on the float64
    coefficients). The step matrix is close to defective (a double pole), so repeated squaring
    amplifies its rounding: no power computed in floating point is within a few ulp of the exact
    one, the long-double one included. What long double buys is its 11 more mantissa bits (64
    against 53) through the same squarings: the plan's matrices are at least 2^8 times closer to
    the exact power than the float64 power is (3 of the 11 bits left to the luck of the
    roundings)."""
    from fractions import Fraction

    p = _lib.loudness_plan(sr, 1, sr)
    m = _step_matrix(p, Fraction)
    for _ in range(int(math.log2(p["chunk"]))):
        m = [[sum(m[i][k] * m[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    assert 2 ** int(math.log2(p["chunk"])) == p["chunk"]

    def distance(a):
        return float(max(abs(Fraction(float(a[i, j])) - m[i][j])
                         for i in range(4) for j in range(4)))

    plan = distance(_blocks(p))
    fp64 = distance(np.linalg.matrix_power(np.array(_step_matrix(p, float)), p["chunk"]))
    top = max(abs(float(v)) for row in m for v in row)
    print(f"{sr} Hz: largest entry {top:.3g}; distance from the exact power: plan {plan:.3g}, "
          f"float64 power {fp64:.3g}")
    assert plan * 256 <= fp64


def test_plan_argument_errors():
    lib = _lib.load()
    out = (ctypes.c_double * _lib.LOUDNESS_PLAN_LEN)()
    for sr, nch, nt, word in ((0, 1, 100, "sample rate"), (-44100, 1, 100, "sample rate"),
                              (44100, 0, 100, "channels"), (44100, 6, 100, "channels"),
                              (44100, 1, 0, "length"), (44100, 1, -5, "length")):
        assert lib.vrvq_loudness_plan(sr, nch, nt, out) == 10001, (sr, nch, nt)
        assert word in lib.vrvq_loudness_error().decode()
        with pytest.raises(RuntimeError, match=word):
            _lib.loudness_plan(sr, nch, nt)
    assert lib.vrvq_loudness_plan(44100, 1, 100, None) == 10001
    assert lib.vrvq_loudness_plan(44100, 1, 100, out) == 0
    assert lib.vrvq_loudness_error() == b""
    # the launcher checks the same on the host, before any launch
    p16 = ctypes.c_void_p(16)
    assert lib.vrvq_loudness(p16, 1, 6, 100, 44100, p16, p16, None) == 10001
    assert lib.vrvq_loudness(p16, 1, 1, 100, 0, p16, p16, None) == 10001
    assert lib.vrvq_loudness(None, 1, 1, 100, 44100, p16, p16, None) == 10001
    assert lib.vrvq_loudness(p16, 0, 1, 100, 44100, p16, p16, None) == 10001
    assert lib.vrvq_loudness(p16, 1, 1, 100, 44100, ctypes.c_void_p(12), p16, None) == 10001


def test_cpu_tensor_takes_the_host_path():
    x, sr = cases.tensor("44k1_5000_padded")
    want = codec.loudness(x, sr)
    got = vrvq_amd.loudness(x, sr)
    assert got.dtype == torch.float32 and got.device.type == "cpu"
    assert torch.equal(got, want)
    assert torch.equal(vrvq_amd.loudness(x[:, 0], sr), want)  # (nb, nt)
    y, before = vrvq_amd.normalize_loudness(x, sr, -16.0, return_loudness=True)
    assert torch.equal(before, want)
    assert torch.equal(y, codec.normalize(x, sr, -16.0))
    assert torch.equal(vrvq_amd.normalize_loudness(x[:, 0], sr, torch.tensor([-16.0, -20.0])),
                       codec.normalize(x, sr, torch.tensor([-16.0, -20.0]))[:, 0])
    with pytest.raises(ValueError, match="channels"):
        vrvq_amd.loudness(torch.zeros(1, 6, 100), sr)
    with pytest.raises(ValueError, match="sample rate"):
        vrvq_amd.loudness(x, 0)


def _host_fp64(x, sr):
    """codec.loudness's value before it is rounded to float32: the float64 array its last
    np.maximum (the floor at -70) returns, seen by a spy that changes nothing."""
    seen = []
    real = np.maximum

    def spy(a, b):
        seen.append(real(a, b))
        return seen[-1]

    with unittest.mock.patch.object(codec.np, "maximum", spy):
        out = codec.loudness(x, sr).numpy()
    return seen[-1], out


def test_reference_is_tied_to_the_yardstick():
    """On every input of the GPU tests codec.loudness (the host yardstick, float64 lfilter and a
    cumulative sum) agrees with the long-double restatement: within 1e-12 LU before rounding and
    in float32 bits after it. The reference's own preconditions hold too: every block is at least
    1e-3 LU from a gate, every value at least 1e-9 LU from a float32 rounding midpoint."""
    ref = cases.reference()
    worst = 0.0
    for name in cases.cases():
        x, sr = cases.tensor(name)
        lufs, margin = ref[name]
        host64, host = _host_fp64(x, sr)
        assert host64.dtype == np.float64 and np.array_equal(host64.astype(np.float32), host)
        err = np.abs(host64.astype(LD) - lufs).astype(np.float64)
        worst = max(worst, float(err.max()))
        assert np.all(err <= 1e-12), (name, err)
        assert np.array_equal(lufs.astype(np.float32), host), name
        assert np.all(margin >= 1e-3), (name, margin)
        assert all(cases.float32_midpoint_distance(v) >= 1e-9 for v in lufs), name
    print(f"codec.loudness vs long double: worst {worst:.3g} LU")
    assert float(ref["44k1_zeros"][0][1]) == -70.0
    assert math.isinf(ref["44k1_zeros"][1][1])
