"""Inputs of the loudness tests and their long-double reference values, built once per session and
shared by tests/test_loudness.py (CPU: the reference is tied to the host yardstick on them) and
tests/test_gpu_loudness.py (the HIP path is judged on them).

Every case is a 220 Hz tone plus noise, as tests/test_codec.py `_signal` builds it, at the case's
own rate and with two items; the second item is scaled by 0.01 over its middle third, so the
relative gate drops blocks there."""
import functools

import numpy as np
import torch

import loudness_ref

CHUNK = 256  # VRVQ_LOUDNESS_CHUNK; tests/test_loudness.py compares it with the plan's


def signal(n, seed, sr, nch=1, items=2, dc=0.0):
    g = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.05 * g.standard_normal((items, nch, n)) + dc
    if items > 1:
        x[1, :, n // 3:2 * n // 3] *= 0.01
    return x.astype(np.float32)


def _gates(sr):
    """Item 0: its first second is exact zeros (blocks under the absolute gate); item 1: all
    zeros (reads exactly -70)."""
    x = signal(2 * sr + 5, 21, sr, items=2)
    x[1] = 0.0
    x[0, :, :sr] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (x float32 array (2, nch, nt), sample_rate)}"""
    k = 100  # k * CHUNK is past 0.5 s at 44.1 kHz: nothing is padded at the chunk edge
    c = {
        "44k1_3s17_stereo": (signal(3 * 44100 + 17, 1, 44100, nch=2), 44100),
        "44k1_5000_padded": (signal(5000, 2, 44100), 44100),
        "44k1_half_second_minus_1": (signal(22049, 3, 44100), 44100),
        "44k1_half_second": (signal(22050, 4, 44100), 44100),
        "44k1_chunk_edge_minus_1": (signal(k * CHUNK - 1, 5, 44100), 44100),
        "44k1_chunk_edge": (signal(k * CHUNK, 6, 44100), 44100),
        "44k1_chunk_edge_plus_1": (signal(k * CHUNK + 1, 7, 44100), 44100),
        "16k_2s3_dc_offset": (signal(2 * 16000 + 3, 8, 16000, dc=0.5), 16000),
        "11k025_2s_stereo": (signal(2 * 11025, 9, 11025, nch=2), 11025),  # win != 4 step
        "44k1_1s_5ch": (signal(44100, 10, 44100, nch=5), 44100),
        "44k1_zeros": (_gates(44100), 44100),
        # 8000 effective samples are 32 chunks: the carry's groups hold one chunk each
        "16k_3000_padded": (signal(3000, 11, 16000), 16000),
    }
    return c


@functools.lru_cache(maxsize=None)
def reference():
    """{name: (lufs (2,) long double, gate margin (2,) float)} from loudness_ref.measure, all
    cases in one walk of the time axis."""
    c = cases()
    names = list(c)
    return dict(zip(names, loudness_ref.measure([c[n] for n in names])))


def tensor(name):
    x, sr = cases()[name]
    return torch.from_numpy(x), sr


def float32_midpoint_distance(v):
    """Distance from v (long double) to the nearest midpoint between two neighbouring float32
    values: how far v is from rounding the other way."""
    f = np.float32(v)
    lo = np.nextafter(f, np.float32(-np.inf))
    hi = np.nextafter(f, np.float32(np.inf))
    LD = np.longdouble
    mids = [(LD(lo) + LD(f)) / 2, (LD(f) + LD(hi)) / 2]
    return float(min(abs(LD(v) - m) for m in mids))
