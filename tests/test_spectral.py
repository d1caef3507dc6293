"""Spectral distances without a GPU: the NumPy float64 restatement (tests/spectral_ref.py, the
judge of tests/test_gpu_spectral.py) against vrvq_amd.losses on float64 tensors, the banded mel
tables against losses.mel_filters, the twiddle / window tables, the operator and C-ABI surface,
and the argument errors of spectral_distance, rd_sweep(spectral=...) and
solve_quality(metric="mel")."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spectral_ref as S
import vrvq_amd
from vrvq_amd import _lib, losses, ops, utils

BASE_WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)     # conf/base.yml MelSpectrogramLoss
BASE_MELS = (5, 10, 20, 40, 80, 160, 320)
PAIRS = list(zip(BASE_WINDOWS, BASE_MELS)) + [(2048, 150)]


def signals(B, T, seed=0):
    rng = np.random.default_rng(seed)
    ref = (0.3 * rng.standard_normal((B, T)) + 0.05).astype(np.float32)
    est = (0.7 * ref + 0.03 * rng.standard_normal((B, T))).astype(np.float32)
    return est, ref


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))[:, None, :]


# ------------------------------------------------------------------ restatement vs losses.py
CONFIGS = {
    "mel_reference_defaults": (losses.MelSpectrogramLoss, utils.MEL_DISTANCE,
                               dict(n_mels=(150, 80), window_lengths=(2048, 512), pow=2.0,
                                    mag_weight=1.0)),
    "stft_reference_defaults": (losses.MultiScaleSTFTLoss, utils.STFT_DISTANCE, dict()),
    "mel_base_yml": (losses.MelSpectrogramLoss,
                     dict(windows=BASE_WINDOWS, n_mels=BASE_MELS, pow=1.0, mag_weight=0.0), dict()),
    "stft_no_mag": (losses.MultiScaleSTFTLoss,
                    dict(windows=(2048, 512), pow=2.0, mag_weight=0.0), dict(mag_weight=0.0)),
    "mel_band_limited": (losses.MelSpectrogramLoss,
                         dict(windows=(512,), n_mels=(80,), pow=1.0, mag_weight=1.0,
                              mel_fmin=(50.0,), mel_fmax=(8000.0,)),
                         dict(n_mels=(80,), window_lengths=(512,), mag_weight=1.0,
                              mel_fmin=(50.0,), mel_fmax=(8000.0,))),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_restatement_equals_losses_on_float64(name):
    cls, ours, theirs = CONFIGS[name]
    for T in (1025, 4099):
        est, ref = signals(3, T, seed=T)
        want = float(cls(**theirs)(t64(est), t64(ref)))
        got = S.distance_rows(est, ref, **ours)
        assert got["distance"].shape == (3,) and np.isfinite(got["distance"]).all()
        assert abs(got["distance"].mean() - want) <= 1e-12 * abs(want), (T, got, want)
        # ... and row by row: a batch of one is that row's distance
        for r in range(3):
            one = float(cls(**theirs)(t64(est[r:r + 1]), t64(ref[r:r + 1])))
            assert abs(got["distance"][r] - one) <= 1e-12 * abs(one), (T, r)


def test_restatement_frames_and_lengths():
    x = np.arange(1, 12, dtype=np.float64)                # n = 11, hop = 2: 6 frames
    fr = S.frames(x, 8)
    assert fr.shape == (6, 8)
    assert fr[0].tolist() == [5, 4, 3, 2, 1, 2, 3, 4]     # -i -> i
    assert fr[5].tolist() == [7, 8, 9, 10, 11, 10, 9, 8]  # n-1+i -> n-1-i
    # the minimum length W/2 + 1: frame 1 reflects on both sides at once
    assert S.frames(np.arange(5.0), 8)[1].tolist() == [2, 1, 0, 1, 2, 3, 4, 3]
    with pytest.raises(AssertionError):
        S.frames(np.arange(4.0), 8)
    est, ref = signals(4, 700, seed=3)
    cut = S.distance_rows(est, ref[:2], windows=(64, 512), n_mels=(10, 0), lengths=[700, 256])
    assert np.isfinite(cut["distance"][[0, 2]]).all() and np.isnan(cut["distance"][[1, 3]]).all()
    assert np.isfinite(cut["log"][:, 0]).all() and np.isnan(cut["log"][[1, 3], 1]).all()
    alone = S.distance_rows(est[1:2, :256], ref[1:2, :256], windows=(64,), n_mels=(10,))
    assert alone["log"][0, 0] == cut["log"][1, 0] and alone["mag"][0, 0] == cut["mag"][1, 0]


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("pair", PAIRS + [(512, 80, 50.0, 8000.0)])
def test_band_tables_are_the_dense_filters(pair):
    window, n_mels = pair[:2]
    fmin, fmax = (pair[2], pair[3]) if len(pair) > 2 else (0.0, None)
    dense = losses.mel_filters(44100, window, n_mels, fmin, fmax)
    bands, weights = utils.mel_bands(44100, window, n_mels, fmin, fmax)
    assert bands.dtype == np.int32 and bands.shape == (3, n_mels) and weights.dtype == np.float32
    rebuilt = S.bands_to_dense(bands, weights, window)
    # bit for bit on every non-zero; mel_filters leaves -0.0 at some zeros (its np.maximum(0, .)
    # keeps the sign of a ramp that is exactly -0.0), which a band does not store: a zero of
    # either sign adds nothing to a sum of non-negative products
    nz = dense != 0
    assert (rebuilt != 0).tolist() == nz.tolist()
    assert rebuilt[nz].view(np.uint32).tolist() == dense[nz].view(np.uint32).tolist()
    assert np.array_equal(rebuilt, dense)
    if len(pair) == 2:  # the band-limited bank has filters narrower than a bin: empty bands
        assert (bands[1] >= 1).all(), "no empty filter"
    assert (bands[0] + bands[1] <= window // 2 + 1).all()
    assert bands[2].tolist() == np.concatenate([[0], np.cumsum(bands[1])[:-1]]).tolist()
    assert (dense != 0).sum(axis=0).max() <= 2, "at most two filters per bin"
    # the banded sum is the dense product
    mag = np.abs(np.random.default_rng(window).standard_normal((window // 2 + 1, 3)))
    np.testing.assert_allclose(S.banded_project(bands, weights, mag),
                               dense.astype(np.float64) @ mag, rtol=1e-14, atol=0)


def test_band_builder_refuses_a_split_row(monkeypatch):
    fb = losses.mel_filters(44100, 64, 10).copy()
    fb[3, 20] = 0.5  # a second run in row 3
    monkeypatch.setattr(losses, "mel_filters", lambda *a: fb)
    utils.mel_bands.cache_clear()
    try:
        with pytest.raises(ValueError, match="contiguous"):
            utils.mel_bands(44100, 64, 10)
    finally:
        utils.mel_bands.cache_clear()


@pytest.mark.parametrize("window", BASE_WINDOWS)
def test_twiddle_and_window_tables(window):
    tab = utils.spectral_tables(window)
    assert tab.dtype == np.float32 and tab.shape == (3 * window,)
    k = np.arange(window)
    tw = tab[:2 * window].reshape(window, 2).astype(np.float64)
    exact = np.exp(-2j * np.pi * k / window)
    assert np.abs(tw[:, 0] - exact.real).max() <= 2.0 ** -25
    assert np.abs(tw[:, 1] - exact.imag).max() <= 2.0 ** -25
    assert tw[0].tolist() == [1.0, 0.0] and tw[window // 2, 0] == -1.0
    hann = torch.hann_window(window, dtype=torch.float64).numpy()
    assert np.abs(tab[2 * window:] - hann).max() <= 2.0 ** -25


def test_tile_constant_mirrors_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "vrvq.h")).read()
    assert int(re.search(r"#define\s+VRVQ_SPECTRAL_TILE_SAMPLES\s+(\d+)", src).group(1)) \
        == _lib.SPECTRAL_TILE_SAMPLES
    assert re.search(r"#define\s+VRVQ_SPECTRAL_TILE_FRAMES\(window\)\s+"
                     r"\(VRVQ_SPECTRAL_TILE_SAMPLES / \(window\)\)", src)
    assert [_lib.spectral_tile_frames(w) for w in BASE_WINDOWS] == [256, 128, 64, 32, 16, 8, 4]


# ------------------------------------------------------------------ operator and fake
def test_spectral_op_registered_with_fake_kernel():
    lib = ops.load_ops()
    assert lib.spectral_distance.default._schema.name == "vrvq::spectral_distance"
    m = torch.device("meta")
    e = torch.empty(0, device=m)
    for est, ref in ((torch.empty(6, 5000, device=m), torch.empty(3, 5000, device=m)),
                     (torch.empty(6, 1, 5000, device=m), torch.empty(3, 1, 5000, device=m))):
        for lengths in (None, torch.empty(3, dtype=torch.int64, device=m)):
            terms, dist = lib.spectral_distance(est, ref, lengths, [2048, 512], [150, 0], [e, e],
                                                [e, e], [e, e], 1e-5, 2.0, 1.0, 1.0)
            assert terms.shape == (6, 2, 2) and dist.shape == (6,)
            assert terms.dtype == dist.dtype == torch.float64


def test_spectral_rejects_cpu_tensors():
    ops.load_ops()
    est, ref = torch.ones(4, 1, 3000), torch.ones(2, 1, 3000)
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.spectral_distance(est, ref, windows=(2048, 64), n_mels=(150, 0))
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.spectral_distance(est[:, 0], ref[:, 0], windows=[32], lengths=[3000, 10])
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.mel_distance(est, ref, lengths=[3000, 2000])
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.stft_distance(est, ref)
    tabs = [torch.from_numpy(utils.spectral_tables(64))]
    none = [torch.empty(0)]
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.spectral_distance(est, ref, None, [64], [0], tabs, none, none, 1e-5, 2.0)


# ------------------------------------------------------------------ argument errors
def test_python_argument_errors_raise_before_any_kernel():
    """On CPU tensors: a ValueError, not the kernels' "GPU only" RuntimeError, shows the check
    comes first."""
    est, ref = torch.ones(4, 1, 3000), torch.ones(2, 1, 3000)
    ok = dict(windows=(512,))
    for bad in (dict(windows=(48,)), dict(windows=(16,)), dict(windows=(4096,)), dict(windows=()),
                dict(windows=(32,) * 17), dict(windows=(512,), n_mels=(258,)),
                dict(windows=(512,), n_mels=(-1,)), dict(windows=(512, 64), n_mels=(80,)),
                dict(windows=(512,), clamp_eps=0.0), dict(windows=(512,), clamp_eps=-1e-5),
                dict(windows=(512,), mel_fmin=(0.0, 1.0)), dict(windows=(512,), lengths=[5])):
        with pytest.raises(ValueError):
            utils.spectral_distance(est, ref, **bad)
    with pytest.raises(ValueError):
        utils.spectral_distance(est[:3], ref, **ok)                  # 3 rows against 2
    with pytest.raises(ValueError):
        utils.spectral_distance(est, ref[..., :2999], **ok)          # sample counts differ
    with pytest.raises(ValueError):
        utils.spectral_distance(torch.ones(4, 2, 3000), ref, **ok)   # two channels
    with pytest.raises(ValueError, match="1024"):                    # T <= max(W) / 2, no lengths
        utils.spectral_distance(est[..., :1024], ref[..., :1024], windows=(64, 2048))
    with pytest.raises(ValueError, match="1024"):
        utils.mel_distance(est[..., :1024], ref[..., :1024])
    with pytest.raises(RuntimeError, match="GPU only"):              # with lengths it is per row
        utils.spectral_distance(est[..., :1024], ref[..., :1024], windows=(64, 2048),
                                lengths=[1024, 1024])


SMALL = dict(encoder_dim=8, decoder_dim=32, n_codebooks=2)


def test_sweep_and_solver_argument_errors_raise_before_any_kernel():
    vbr = vrvq_amd.DAC_VRVQ(level_min=0.5, level_max=2.0, **SMALL).eval()
    short, clip = torch.zeros(2, 1, 1024), torch.zeros(2, 1, 2560)
    for bad in (("mell",), "mels", ("mel", "l1"), ("si_sdr",)):
        with pytest.raises(ValueError, match="spectral"):
            utils.rd_sweep(vbr, clip, [1.0], spectral=bad)
    for cols in (("mel",), "stft", ("mel", "stft")):
        with pytest.raises(ValueError, match="1025"):
            utils.rd_sweep(vbr, short, [1.0], spectral=cols)
    for metric in ("mel", "stft"):
        with pytest.raises(ValueError, match="1025"):
            utils.solve_quality(vbr, short, 0.8, metric=metric)
        with pytest.raises(ValueError, match="targets for 2 clips"):
            utils.solve_quality(vbr, clip, [0.8], metric=metric)
        with pytest.raises(ValueError, match="iters"):
            utils.solve_quality(vbr, clip, 0.8, metric=metric, iters=-1)
    with pytest.raises(ValueError, match="metric"):
        utils.solve_quality(vbr, clip, 0.8, metric="mell")
    # valid arguments reach the kernels, which refuse CPU tensors
    with pytest.raises(RuntimeError, match="GPU"):
        vrvq_amd.solve_quality(vbr, clip, [0.8, 0.9], metric="mel")
    with pytest.raises(RuntimeError, match="GPU"):
        vrvq_amd.rd_sweep(vbr, clip, [0.5, 1.0], spectral=("mel", "stft"))


def test_capi_argument_errors():
    lib = _lib.load()
    assert lib.vrvq_version() >= 103
    ERR = 10001
    p = ctypes.c_void_p(16)  # non-null, never dereferenced: the checks return before a launch
    n = ctypes.c_longlong(0)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    def ws_bytes(rows, samples, windows, out=None):
        rc = lib.vrvq_spectral_distance_workspace(rows, samples, len(windows), ints(*windows),
                                                  ctypes.byref(n) if out is None else out)
        return rc, n.value

    def tiles(samples, w):
        frames = 1 + samples // (w // 4)
        return -(-frames // _lib.spectral_tile_frames(w))

    assert ws_bytes(12, 441000, (2048, 512)) == (0, 16 * 12 * (tiles(441000, 2048)
                                                               + tiles(441000, 512)))
    assert tiles(441000, 2048) == 216 and tiles(441000, 512) == 216
    assert ws_bytes(3, 4099, BASE_WINDOWS) == (0, 16 * 3 * sum(tiles(4099, w)
                                                               for w in BASE_WINDOWS))
    for rows, samples, windows in ((0, 4099, (512,)), (-1, 4099, (512,)), (65536, 4099, (512,)),
                                   (2, 0, (512,)), (2, -5, (512,)), (2, 2 ** 32 + 1, (512,)),
                                   (2, 4099, ()), (2, 4099, (32,) * 17), (2, 4099, (48,)),
                                   (2, 4099, (16,)), (2, 4099, (4096,)), (2, 4099, (0,)),
                                   (2, 4099, (-512,))):
        assert ws_bytes(rows, samples, windows)[0] == ERR, (rows, samples, windows)
    assert lib.vrvq_spectral_distance_workspace(2, 4099, 1, None, ctypes.byref(n)) == ERR
    assert ws_bytes(2, 4099, (512,), out=ctypes.c_void_p(0))[0] == ERR

    need = 16 * 4 * (tiles(4099, 2048) + tiles(4099, 512))

    def call(est=p, ref=p, rows=4, ref_rows=2, samples=4099, lengths=None, windows=(2048, 512),
             n_mels=(150, 0), tables=(16, 16), bands=(16, None), weights=(16, None), eps=1e-5,
             pow=2.0, terms=p, distance=p, ws=p, ws_size=need, no_windows=False, no_mels=False,
             no_tables=False, no_bands=False):
        return lib.vrvq_spectral_distance(
            est, ref, rows, ref_rows, samples, lengths, len(windows),
            None if no_windows else ints(*windows), None if no_mels else ints(*n_mels),
            None if no_tables else ptrs(*tables), None if no_bands else ptrs(*bands),
            ptrs(*weights), eps, pow, 1.0, 1.0, terms, distance, ws, ws_size, None)

    for kw in (dict(est=None), dict(ref=None), dict(terms=None), dict(ws=None),
               dict(no_windows=True), dict(no_mels=True), dict(no_tables=True),
               dict(no_bands=True), dict(tables=(16, None)), dict(tables=(20, 16)),
               dict(bands=(None, None)), dict(weights=(None, None)),
               dict(rows=0), dict(rows=-4), dict(rows=65536, ref_rows=1), dict(ref_rows=0),
               dict(ref_rows=-2), dict(ref_rows=3),
               dict(samples=0), dict(samples=-1), dict(samples=1024), dict(samples=2 ** 32 + 1),
               dict(windows=(2048, 48)), dict(windows=(4096, 512)), dict(windows=(2048, 16)),
               dict(n_mels=(150, -1)), dict(n_mels=(1026, 0)), dict(n_mels=(150, 258)),
               dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan")),
               dict(ws_size=need - 1), dict(ws_size=0), dict(ws=ctypes.c_void_p(20))):
        assert call(**kw) == ERR, kw
    # samples <= max(W) / 2 is refused without lengths only: with them it is a per-row NaN, and
    # this call fails on its workspace size (checked after the lengths rule), still before a launch
    assert call(samples=1024, lengths=p, ws_size=0) == ERR
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("vrvq_spectral_distance_workspace", 1, 1, 0, None, None)
