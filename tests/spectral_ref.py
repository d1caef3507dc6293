"""NumPy float64 restatement of the spectral distance (include/vrvq.h "Spectral distance"), the
judge of tests/test_gpu_spectral.py; tests/test_spectral.py pins it to vrvq_amd.losses on float64
tensors. Written from the definition -- padded copy, gathered frames, np.fft.rfft, the dense mel
matrix -- not from the kernels' structure (no span tiles, no packed transform, no bands)."""
import numpy as np

from vrvq_amd.losses import mel_filters


def frames(x, window):
    """(frames, window): frame j holds samples j hop - W/2 .. j hop + W/2 - 1 of x, reflected at
    both ends without repeating the edge; hop = W / 4, 1 + n // hop frames. Needs n > W / 2."""
    x = np.asarray(x, np.float64).reshape(-1)
    n, hop = x.size, window // 4
    assert n > window // 2, "reflection needs more than W / 2 samples"
    padded = np.pad(x, window // 2, mode="reflect")
    idx = hop * np.arange(1 + n // hop)[:, None] + np.arange(window)[None, :]
    return padded[idx]


def magnitudes(x, window):
    """(W/2 + 1, frames) |rfft| of the periodic-Hann-windowed frames, no normalisation."""
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(window) / window)
    return np.abs(np.fft.rfft(frames(x, window) * hann, axis=1)).T


def spectrogram(x, window, n_mels=0, sample_rate=44100, fmin=0.0, fmax=None):
    """Magnitudes, projected on mel_filters' fp32 values (as float64) if n_mels > 0."""
    mag = magnitudes(x, window)
    if n_mels:
        mag = mel_filters(sample_rate, window, n_mels, fmin, fmax).astype(np.float64) @ mag
    return mag


def scale_terms(e, r, window, n_mels=0, *, clamp_eps=1e-5, pow=2.0, sample_rate=44100, fmin=0.0,
                fmax=None):
    """(log term, magnitude term, mean of E + R) of one row at one scale."""
    E = spectrogram(e, window, n_mels, sample_rate, fmin, fmax)
    R = spectrogram(r, window, n_mels, sample_rate, fmin, fmax)
    log = np.mean(np.abs(pow * np.log10(np.maximum(E, clamp_eps))
                         - pow * np.log10(np.maximum(R, clamp_eps))))
    return log, np.mean(np.abs(E - R)), np.mean(E + R)


def distance_rows(est, ref, *, windows, n_mels=None, clamp_eps=1e-5, pow=2.0, log_weight=1.0,
                  mag_weight=1.0, mel_fmin=None, mel_fmax=None, sample_rate=44100, lengths=None):
    """Every row of est (R, T) against row r % B of ref (B, T): {"distance" (R,), "log", "mag",
    "level" (R, S)} ("level" the mean of E + R, the scale of the magnitude term's error bar). A
    row with a length is cut to its first samples; one no longer than W / 2 is NaN at that scale
    and in its distance."""
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    R, B, S = est.shape[0], ref.shape[0], len(windows)
    n_mels = [0] * S if n_mels is None else [int(m or 0) for m in n_mels]
    fmin = [0.0] * S if mel_fmin is None else list(mel_fmin)
    fmax = [None] * S if mel_fmax is None else list(mel_fmax)
    out = {k: np.full((R, S), np.nan) for k in ("log", "mag", "level")}
    for i in range(R):
        n = est.shape[1] if lengths is None else int(np.clip(lengths[i % B], 0, est.shape[1]))
        for s, (w, m) in enumerate(zip(windows, n_mels)):
            if n > w // 2:
                out["log"][i, s], out["mag"][i, s], out["level"][i, s] = scale_terms(
                    est[i, :n], ref[i % B, :n], w, m, clamp_eps=clamp_eps, pow=pow,
                    sample_rate=sample_rate, fmin=fmin[s], fmax=fmax[s])
    out["distance"] = np.sum(log_weight * out["log"] + mag_weight * out["mag"], axis=1)
    return out


def bands_to_dense(bands, weights, window):
    """The (n_mels, W/2 + 1) matrix a (bands, weights) pair of utils.mel_bands stands for."""
    n_mels = bands.shape[1]
    dense = np.zeros((n_mels, window // 2 + 1), np.float32)
    for m in range(n_mels):
        start, ln, off = (int(v) for v in bands[:, m])
        dense[m, start:start + ln] = weights[off:off + ln]
    return dense


def banded_project(bands, weights, mag):
    """The banded projection of (bins, frames) magnitudes in float64, ascending bins."""
    out = np.zeros((bands.shape[1], mag.shape[1]))
    for m in range(bands.shape[1]):
        start, ln, off = (int(v) for v in bands[:, m])
        for j in range(ln):
            out[m] += np.float64(weights[off + j]) * mag[start + j]
    return out
