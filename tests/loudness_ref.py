"""numpy.longdouble restatement of the BS.1770-4 integrated loudness of vrvq_amd.codec.loudness
(audiotools' Meter.integrated_loudness): the K-weighting as a sequential recurrence, one sample
after the other, and every block as a direct sum over its own samples (no cumulative sum, no
chunking, no carried state). What the HIP scan and the host yardstick are both judged against.

The coefficients are codec._biquad's float64 values: they define the filter. Everything after
them runs in long double (64-bit mantissa on x86-64).

The recurrence cannot be vectorised over time, so it is vectorised over rows instead: `measure`
takes every case at once, pads the rows with zeros to the longest and walks the time axis once
with per-row coefficients. A row's result does not depend on the zeros after its end (they are
cut off before the block sums).
"""
import math

import numpy as np

from vrvq_amd.codec import _biquad

LD = np.longdouble
GAINS = (1.0, 1.0, 1.0, 1.41, 1.41)
STAGES = (("high_shelf", 4.0, 1.0 / math.sqrt(2.0), 1500.0), ("high_pass", 0.0, 0.5, 38.0))


def geometry(nt, sample_rate):
    """(effective length, win, step, blocks) of nt samples: the padding rule and the block grid
    in the float arithmetic of codec.loudness."""
    eff = nt
    if nt / sample_rate < 0.5:
        eff = nt + int((0.5 - nt / sample_rate) * sample_rate)
    win = int(0.400 * sample_rate)
    step = int(0.400 * sample_rate * 0.25)
    return eff, win, step, (eff - win) // step + 1


def kweight(rows, rates):
    """rows: list of 1-D float arrays (already at their effective length), rates: their sample
    rates. Returns the K-weighted rows as long double arrays."""
    n = max(len(r) for r in rows)
    x = np.zeros((len(rows), n), LD)
    for i, r in enumerate(rows):
        x[i, :len(r)] = np.asarray(r, LD)
    for kind, g, q, fc in STAGES:
        co = np.array([np.concatenate(_biquad(kind, g, q, fc, sr)) for sr in rates], LD)
        b0, b1, b2, a1, a2 = co[:, 0], co[:, 1], co[:, 2], co[:, 4], co[:, 5]
        s0 = np.zeros(len(rows), LD)
        s1 = np.zeros(len(rows), LD)
        xt = np.ascontiguousarray(x.T)  # time-major: one contiguous row of all signals per step
        yt = np.empty_like(xt)
        for t in range(n):  # transposed direct form II, sample by sample
            u = xt[t]
            v = b0 * u + s0
            s0 = b1 * u - a1 * v + s1
            s1 = b2 * u - a2 * v
            yt[t] = v
        x = np.ascontiguousarray(yt.T)
    return [x[i, :len(r)] for i, r in enumerate(rows)]


def _lufs(power):
    with np.errstate(divide="ignore"):
        return LD(-0.691) + LD(10.0) * np.log10(power)


def measure(cases):
    """cases: list of (x (nb, nch, nt) float32 array, sample_rate). Returns per case
    (lufs (nb,) long double floored at -70, margin (nb,) float: the smallest distance in LU from
    any finite block loudness to the absolute or the relative gate; inf where no block is finite)."""
    rows, rates, where = [], [], []
    for ci, (x, sr) in enumerate(cases):
        x = np.asarray(x)
        nb, nch, nt = x.shape
        eff = geometry(nt, sr)[0]
        for i in range(nb):
            for c in range(nch):
                r = np.zeros(eff, LD)
                r[:nt] = x[i, c]
                rows.append(r)
                rates.append(sr)
                where.append((ci, i, c))
    ys = kweight(rows, rates)
    out = []
    k = 0
    for x, sr in cases:
        nb, nch, nt = np.asarray(x).shape
        eff, win, step, nblk = geometry(nt, sr)
        G = np.array(GAINS[:nch], LD)
        lufs = np.empty(nb, LD)
        margin = np.empty(nb)
        for i in range(nb):
            y = np.stack(ys[k:k + nch])
            k += nch
            sq = y * y
            z = np.stack([sq[:, j * step:j * step + win].sum(-1) / LD(win) for j in range(nblk)], -1)
            l = _lufs((G[:, None] * z).sum(0))                       # (nblk,)
            abs_ok = l > -70
            if not abs_ok.any():
                lufs[i] = -70
                fin = l[np.isfinite(l)]
                margin[i] = float(np.abs(fin + 70).min()) if fin.size else math.inf
                continue
            gamma = _lufs((G * z[:, abs_ok].mean(-1)).sum()) - LD(10.0)
            ok = abs_ok & (l > gamma)
            v = _lufs((G * z[:, ok].mean(-1)).sum()) if ok.any() else LD(-70)
            lufs[i] = max(v, LD(-70))
            fin = l[np.isfinite(l)]
            margin[i] = float(min(np.abs(fin + 70).min(), np.abs(fin - gamma).min()))
        out.append((lufs, margin))
    return out
