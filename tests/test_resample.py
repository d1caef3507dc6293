"""The resampler's host side (no GPU): the plan, the tap table against the float64 formula, the
error statuses, the op schemas -- and the sanity of the float64 restatement itself
(tests/resample_ref.py), so the yardstick of tests/test_gpu_resample.py is known good."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import resample_ref as ref
import vrvq_amd
from vrvq_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# old_sr, new_sr, reduced ratio
RATIOS = [(48000, 44100, (160, 147)), (44100, 48000, (147, 160)), (16000, 44100, (160, 441)),
          (44100, 16000, (441, 160)), (44100, 22050, (2, 1)), (44100, 11025, (4, 1)),
          (22050, 44100, (1, 2)), (48000, 16000, (3, 1)), (44100, 8000, (441, 80))]
IDS = [f"{o}-{n}" for o, n, _ in RATIOS]
# kept taps and K of the specification's table (NumPy fp64, CPU)
KEPT = {(160, 147): (56, 216), (147, 160): (51, 199), (160, 441): (51, 212),
        (441, 160): (141, 581), (3, 1): (153, 157)}
ERR_ARG = 10001


def test_version_and_tile_constant():
    assert _lib.load().vrvq_version() >= 106
    header = open(os.path.join(REPO, "include", "vrvq.h")).read()
    m = re.search(r"#define\s+VRVQ_RESAMPLE_TILE\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.RESAMPLE_TILE


@pytest.mark.parametrize("old_sr,new_sr,reduced", RATIOS, ids=IDS)
def test_plan_matches_specification(old_sr, new_sr, reduced):
    old, new, sr, W, K = ref.plan(old_sr, new_sr)
    assert (old, new) == reduced
    keep = ref.kept(old_sr, new_sr)
    ntaps = int(keep.sum(axis=1).max())
    assert ntaps <= math.floor(2 * 24 * old / sr) + 1
    if reduced in KEPT:
        assert (ntaps, K) == KEPT[reduced]
    for L in (0, 1, 2, W, old + 1, 44100, 350_000_000):
        p = _lib.resample_plan(old_sr, new_sr, length=L)
        assert (p["old"], p["new"], p["W"], p["K"], p["ntaps"]) == (old, new, W, K, ntaps)
        # Python integers: exact at any length
        assert p["out_length"] == new * L // old
        assert p["out_length_max"] == -(-new * L // old)
        assert p["taps_len"] == new * ntaps


def test_output_length_is_integer_arithmetic():
    """3.5e8 samples (an hour of 48 kHz stereo in one call): new * L passes 2^32, and a float32
    round trip of the length (24 bits) would be off by up to 16 samples."""
    L = 350_000_001
    for old_sr, new_sr, (old, new) in RATIOS:
        p = _lib.resample_plan(old_sr, new_sr, length=L)
        assert p["out_length"] == new * L // old
        assert p["out_length_max"] - p["out_length"] == (1 if new * L % old else 0)


@pytest.mark.parametrize("old_sr,new_sr,reduced", RATIOS, ids=IDS)
def test_taps_match_formula(old_sr, new_sr, reduced):
    k, u = ref.kernels(old_sr, new_sr)
    keep = np.abs(u) < 24
    K = k.shape[1]
    taps, first = _lib.resample_taps(old_sr, new_sr)
    ntaps = taps.shape[1]
    assert taps.dtype == np.float32 and first.dtype == np.int32
    assert taps.shape == (reduced[1], int(keep.sum(axis=1).max()))
    # the rows' windows: inside K, non-decreasing starts, every kept tap inside its window
    assert first.min() >= 0 and (first + ntaps).max() <= K
    assert (np.diff(first) >= 0).all()
    # every dropped tap of the formula is the window's zero
    assert np.abs(k[~keep]).max(initial=0.0) < 1e-30
    worst = 0.0
    for i in range(taps.shape[0]):
        j = first[i] + np.arange(ntaps)
        inside = np.zeros(K, bool)
        inside[j] = True
        assert not (keep[i] & ~inside).any(), f"phase {i}: a kept tap is outside the row"
        want, live = k[i, j], keep[i, j]
        assert (taps[i][~live] == 0.0).all()
        err = np.abs(taps[i][live].astype(np.float64) - want[live])
        # one fp32 rounding: 2^-24 relative, or half the smallest subnormal where the tap lies
        # below fp32's range (160:441 has taps whose |u| is 24 less one fp64 ulp: about 1e-49)
        unit = np.maximum(np.abs(want[live]) * 2.0 ** -24, 2.0 ** -150)
        worst = max(worst, float((err / unit).max()))
        # each phase sums to 1 within ntaps roundings
        assert abs(float(taps[i].astype(np.float64).sum()) - 1.0) <= ntaps * 2.0 ** -24
    print(f"{old_sr}->{new_sr}: worst tap error {worst:.4f} of 2^-24 relative")
    assert worst <= 1.0


def test_error_statuses():
    lib = _lib.load()
    out = (ctypes.c_longlong * 8)()
    assert lib.vrvq_resample_plan(44100, 44101, 24, 0.945, 100, out) == ERR_ARG
    assert b"44100:44101" in lib.vrvq_resample_error()
    with pytest.raises(RuntimeError, match="44100:44101"):
        _lib.resample_plan(44100, 44101)
    for zeros in (0, -3):
        assert lib.vrvq_resample_plan(48000, 44100, zeros, 0.945, 100, out) == ERR_ARG
    for rolloff in (0.0, -0.5, 1.0001, float("nan")):
        assert lib.vrvq_resample_plan(48000, 44100, 24, rolloff, 100, out) == ERR_ARG
    assert lib.vrvq_resample_plan(48000, 44100, 24, 1.0, 100, out) == 0
    assert lib.vrvq_resample_plan(0, 44100, 24, 0.945, 100, out) == ERR_ARG
    assert lib.vrvq_resample_plan(48000, 44100, 24, 0.945, -1, out) == ERR_ARG
    assert lib.vrvq_resample_plan(48000, 44100, 24, 0.945, 100, None) == ERR_ARG
    assert lib.vrvq_resample_taps(48000, 44100, 24, 0.945, None, 0, None, 0) == ERR_ARG
    buf = (ctypes.c_float * 16)()
    ibuf = (ctypes.c_int * 147)()
    assert lib.vrvq_resample_taps(48000, 44100, 24, 0.945, buf, 16, ibuf, 147) == ERR_ARG
    # the launchers: null pointers, then shapes, rejected on the host before any launch
    p = ctypes.c_void_p(16)
    for fn in (lib.vrvq_resample, lib.vrvq_resample_adjoint):
        assert fn(None, 1, 100, 160, 147, 28, 56, None, None, None, 91, None) == ERR_ARG
        assert fn(p, 1, 100, 160, 147, 28, 56, p, p, p, 93, None) == ERR_ARG      # > ceil
        assert fn(p, 1, 100, 160, 147, 28, 56, p, p, p, 0, None) == ERR_ARG
        assert fn(p, 0, 100, 160, 147, 28, 56, p, p, p, 91, None) == ERR_ARG
        assert fn(p, 1, 100, 2000, 147, 28, 56, p, p, p, 7, None) == ERR_ARG      # ratio
        assert fn(p, 1, 100, 160, 147, 28, 999, p, p, p, 91, None) == ERR_ARG     # ntaps > K
    # (the adjoint's argument order is (dy, rows, out_length, ..., dx, length): 100 outputs of
    # 91 samples is as far outside the ceil as 93 of 100)


def test_op_schemas_registered():
    from vrvq_amd import ops
    ops.load_ops()
    s = str(torch.ops.vrvq.resample.default._schema)
    assert "Tensor x, Tensor taps, Tensor first, int old_rate, int width, int out_length" in s
    s = str(torch.ops.vrvq.resample_adjoint.default._schema)
    assert "Tensor dy, Tensor taps, Tensor first, int old_rate, int width, int length" in s
    # fake kernels: shapes propagate without a device
    x = torch.empty(3, 1000, device="meta")
    taps = torch.empty(147, 56, device="meta")
    first = torch.empty(147, dtype=torch.int32, device="meta")
    assert torch.ops.vrvq.resample(x, taps, first, 160, 28, 918).shape == (3, 918)
    assert torch.ops.vrvq.resample_adjoint(x, taps, first, 160, 28, 1089).shape == (3, 1089)


def test_equal_rates_return_the_argument():
    x = torch.zeros(2, 1, 100)
    assert vrvq_amd.resample(x, 44100, 44100) is x
    with pytest.raises(RuntimeError, match="GPU"):
        vrvq_amd.resample(x, 48000, 44100)


def test_audio_signal_resample_same_rate():
    from vrvq_amd.codec import AudioSignal
    x = torch.zeros(1, 1, 64)
    sig = AudioSignal(x, 44100)
    assert sig.resample(44100) is sig and sig.audio_data is x and sig.sample_rate == 44100


# ------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("old_sr,new_sr,reduced", RATIOS, ids=IDS)
def test_restatement_constant_and_sine(old_sr, new_sr, reduced):
    old, new, _sr, W, _K = ref.plan(old_sr, new_sr)
    L = max(4000, 6 * W + 64)
    y = ref.resample(np.full((1, L), 0.7), old_sr, new_sr)
    assert y.shape == (1, new * L // old)
    assert np.abs(y - 0.7).max() < 1e-15
    t_old = np.arange(L) / old_sr
    y = ref.resample(np.sin(2 * np.pi * 1000.0 * t_old)[None], old_sr, new_sr)[0]
    want = np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / new_sr)
    edge = 2 * W * new // old + 2
    err = float(np.abs(y - want)[edge:-edge].max())
    print(f"{old_sr}->{new_sr}: 1 kHz sine error {err:.2e}")
    assert err < 1e-4
    if new < 0.8 * old:
        # a tone at 1.25 x the new Nyquist. Only where that lies below the OLD Nyquist: at
        # 160:147 it is 27.6 kHz, which a 48 kHz signal cannot hold (it aliases to 20.4 kHz,
        # inside the new pass band).
        tone = np.sin(2 * np.pi * (1.25 * new_sr / 2) * t_old)[None]
        y = ref.resample(tone, old_sr, new_sr)[0][edge:-edge]
        rms = float(np.sqrt(np.mean(y * y)))
        print(f"{old_sr}->{new_sr}: stop-band tone rms {rms:.2e}")
        assert rms < 1e-4


def test_restatement_adjoint_is_the_transpose():
    """<R x, d> == <x, R^T d> in fp64, edges included (L shorter than the filter too)."""
    g = np.random.default_rng(5)
    for old_sr, new_sr, L in ((48000, 44100, 300), (44100, 16000, 97), (22050, 44100, 5),
                              (44100, 8000, 1)):
        n = ref.out_length_max(L, old_sr, new_sr)
        x, d = g.standard_normal((2, L)), g.standard_normal((2, n))
        lhs = (ref.resample(x, old_sr, new_sr, output_length=n) * d).sum()
        rhs = (x * ref.adjoint(d, L, old_sr, new_sr)).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
        cnt = ref.adjoint_counts(n, L, old_sr, new_sr)
        assert cnt.sum() == sum(ref.kept(old_sr, new_sr)[i % ref.plan(old_sr, new_sr)[1]].sum()
                                for i in range(n))
