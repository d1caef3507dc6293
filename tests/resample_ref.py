"""NumPy float64 restatement of the resampler's specification (include/vrvq.h "Sample-rate
conversion"): julius.resample_frac as audiotools.AudioSignal.resample calls it, with the full
K = 2 W + old taps of every phase (nothing dropped), replicate padding, and its adjoint. The
yardstick of tests/test_resample.py and tests/test_gpu_resample.py; it shares no code with the
library."""
import math
from functools import lru_cache

import numpy as np


@lru_cache(maxsize=None)
def plan(old_sr, new_sr, zeros=24, rolloff=0.945):
    """(old, new, sr, W, K) of the reduced ratio."""
    g = math.gcd(int(old_sr), int(new_sr))
    old, new = int(old_sr) // g, int(new_sr) // g
    sr = min(old, new) * rolloff
    W = int(math.ceil(zeros * old / sr))
    return old, new, sr, W, 2 * W + old


@lru_cache(maxsize=None)
def kernels(old_sr, new_sr, zeros=24, rolloff=0.945):
    """(k, u): k (new, K) float64 normalised taps of every phase, u (new, K) the unclamped tap
    positions in zero crossings (|u| >= zeros: the window's zero, a tap the library drops)."""
    old, new, sr, W, K = plan(old_sr, new_sr, zeros, rolloff)
    i = np.arange(new, dtype=np.float64)[:, None]
    j = np.arange(K, dtype=np.int64)[None, :]
    u = (-i / float(new) + (j - W).astype(np.float64) / float(old)) * sr
    t = np.clip(u, -float(zeros), float(zeros)) * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(t) / t)
    k = sinc * np.cos(t / zeros / 2.0) ** 2
    k = k / k.sum(axis=1, keepdims=True)
    k.setflags(write=False)
    u.setflags(write=False)
    return k, u


def kept(old_sr, new_sr, zeros=24, rolloff=0.945):
    """Boolean (new, K): taps the clamp did not reach."""
    return np.abs(kernels(old_sr, new_sr, zeros, rolloff)[1]) < zeros


def out_length(length, old_sr, new_sr):
    old, new = plan(old_sr, new_sr)[:2]
    return new * int(length) // old


def out_length_max(length, old_sr, new_sr):
    old, new = plan(old_sr, new_sr)[:2]
    return -(-new * int(length) // old)


def _index(length, n_out, old_sr, new_sr, zeros, rolloff):
    old, new, _sr, W, K = plan(old_sr, new_sr, zeros, rolloff)
    frames = -(-n_out // new)
    idx = np.arange(frames, dtype=np.int64)[:, None] * old + np.arange(K, dtype=np.int64)[None, :] - W
    return frames, np.clip(idx, 0, length - 1)


def resample(x, old_sr, new_sr, zeros=24, rolloff=0.945, output_length=None, absolute=False):
    """x (rows, L) -> float64 (rows, n_out). absolute: sum_j |k_j| |x_j| per output instead, the
    scale of the fp32 error bound."""
    x = np.asarray(x, np.float64)
    rows, L = x.shape
    new = plan(old_sr, new_sr, zeros, rolloff)[1]
    n_out = out_length(L, old_sr, new_sr) if output_length is None else int(output_length)
    assert 0 <= n_out <= out_length_max(L, old_sr, new_sr)
    k = kernels(old_sr, new_sr, zeros, rolloff)[0]
    frames, idx = _index(L, n_out, old_sr, new_sr, zeros, rolloff)
    if absolute:
        x, k = np.abs(x), np.abs(k)
    y = np.einsum("rfk,ik->rfi", x[:, idx], k)
    return y.reshape(rows, frames * new)[:, :n_out]


def adjoint(dy, length, old_sr, new_sr, zeros=24, rolloff=0.945, absolute=False):
    """dy (rows, n_out) -> float64 (rows, length): the transpose of resample, the clamped indices
    folding onto the first and last sample. absolute: sum |k| |dy| per element."""
    dy = np.asarray(dy, np.float64)
    rows, n_out = dy.shape
    new = plan(old_sr, new_sr, zeros, rolloff)[1]
    k = kernels(old_sr, new_sr, zeros, rolloff)[0]
    frames, idx = _index(length, n_out, old_sr, new_sr, zeros, rolloff)
    if absolute:
        dy, k = np.abs(dy), np.abs(k)
    d = np.zeros((rows, frames * new))
    d[:, :n_out] = dy
    c = np.einsum("rfi,ik->rfk", d.reshape(rows, frames, new), k)
    dx = np.zeros((rows, length))
    for r in range(rows):
        np.add.at(dx[r], idx.ravel(), c[r].ravel())
    return dx


def adjoint_counts(n_out, length, old_sr, new_sr, zeros=24, rolloff=0.945):
    """(length,) number of kept-tap products that reach each input sample."""
    new = plan(old_sr, new_sr, zeros, rolloff)[1]
    frames, idx = _index(length, n_out, old_sr, new_sr, zeros, rolloff)
    live = (np.arange(frames * new) < n_out).reshape(frames, new).astype(np.float64)
    per = live @ kept(old_sr, new_sr, zeros, rolloff).astype(np.float64)   # (frames, K)
    cnt = np.zeros(length)
    np.add.at(cnt, idx.ravel(), per.ravel())
    return cnt
