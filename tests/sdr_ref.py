"""NumPy restatement of the BSS-eval SDR of include/vrvq.h "BSS SDR" (torchmetrics'
signal_distortion_ratio), written from the formulas and not from the kernels, in two independent
paths:

  yardstick    direct lag sums and Levinson-Durbin in np.longdouble: the judge
  composition  what torchmetrics runs in fp64: zero-padded rfft / irfft correlations and
               np.linalg.solve on the gathered Toeplitz matrix; also cond(R)

and a plain fp64 Levinson (levinson64: fp64 lag sums, fp64 recursion), the host stand-in for the
kernels' algorithm. Each returns a dict with "sdr" (dB), "coh" and "one_minus_coh".

CASES is the table tests/test_sdr.py and tests/test_gpu_sdr.py share; case_data / case_refs build
a case's rows and its references once per process."""
import functools

import numpy as np

LD = np.longdouble
NAN = float("nan")


def _prepared(p, t, zero_mean, dtype):
    """Steps 1 and 2: the optional mean removal and the clamped normalisation, in `dtype`. None
    for the special rows (n = 0 or a silent signal)."""
    p, t = np.asarray(p, dtype).reshape(-1), np.asarray(t, dtype).reshape(-1)
    if p.size == 0:
        return None
    if zero_mean:
        p, t = p - p.mean(dtype=dtype), t - t.mean(dtype=dtype)
    pp, tt = np.sum(p * p), np.sum(t * t)
    if not pp > 0 or not tt > 0:
        return None
    eps = dtype(1e-6)
    return p / max(np.sqrt(pp), eps), t / max(np.sqrt(tt), eps)


def _lag_sums(a, b, F):
    """c[l] = sum_i a[i] b[i + l], l < F, in the arrays' dtype; a lag l >= n is an empty sum."""
    n = a.size
    out = np.zeros(F, a.dtype)
    for l in range(min(F, n)):
        out[l] = np.dot(a[:n - l], b[l:])
    return out


def _levinson(r, b):
    """Solve R s = b, R[i][j] = r[|i - j|], by Levinson-Durbin in the arrays' dtype. Returns
    (s, ok): ok is False where a prediction error was not positive and finite."""
    dtype = r.dtype.type
    F = r.size
    a = np.zeros(F, r.dtype)
    a[0] = 1
    s = np.zeros(F, r.dtype)
    E = r[0]
    ok = bool(E > 0 and np.isfinite(E))
    s[0] = b[0] / E
    for m in range(1, F):
        k = -np.dot(a[:m], r[m:0:-1]) / E
        a[:m + 1] = a[:m + 1] + k * a[m::-1][:m + 1]
        E = E * (dtype(1) - k * k)
        ok = ok and bool(E > 0 and np.isfinite(E))
        q = (b[m] - np.dot(s[:m], r[m:0:-1])) / E
        s[:m + 1] = s[:m + 1] + q * a[m::-1][:m + 1]
    return s, ok


def _result(coh, ok=True):
    if not ok:
        return {"sdr": NAN, "coh": NAN, "one_minus_coh": NAN}
    with np.errstate(all="ignore"):
        one = type(coh)(1) - coh
        return {"sdr": float(10 * np.log10(coh / one)), "coh": float(coh),
                "one_minus_coh": float(one)}


def _direct(p, t, F, zero_mean, load_diag, dtype):
    rows = _prepared(p, t, zero_mean, dtype)
    if rows is None:
        return _result(dtype(NAN), False)
    p, t = rows
    r, b = _lag_sums(t, t, F), _lag_sums(t, p, F)
    if load_diag is not None:
        r[0] += dtype(load_diag)
    with np.errstate(all="ignore"):
        s, ok = _levinson(r, b)
    return _result(np.dot(b, s), ok)


def yardstick(p, t, filter_length=512, zero_mean=False, load_diag=None):
    """The judge: everything in np.longdouble."""
    return _direct(p, t, int(filter_length), zero_mean, load_diag, LD)


def levinson64(p, t, filter_length=512, zero_mean=False, load_diag=None):
    """The kernels' algorithm in plain fp64."""
    return _direct(p, t, int(filter_length), zero_mean, load_diag, np.float64)


def composition(p, t, filter_length=512, zero_mean=False, load_diag=None):
    """torchmetrics' fp64 path: FFT correlations of length 2^ceil(log2(2n - 1)) (lags past it are
    zeros, as empty sums are), the Toeplitz matrix gathered, an LU solve. Adds "cond"."""
    F = int(filter_length)
    rows = _prepared(p, t, zero_mean, np.float64)
    if rows is None:
        return dict(_result(np.float64(NAN), False), cond=NAN)
    p, t = rows
    n_fft = 1 << int(np.ceil(np.log2(max(2 * p.size - 1, 2))))
    tf, pf = np.fft.rfft(t, n_fft), np.fft.rfft(p, n_fft)
    r, b = np.zeros(F), np.zeros(F)
    k = min(F, n_fft)
    r[:k] = np.fft.irfft(tf.real ** 2 + tf.imag ** 2, n_fft)[:k]
    b[:k] = np.fft.irfft(np.conj(tf) * pf, n_fft)[:k]
    if load_diag is not None:
        r[0] += load_diag
    idx = np.abs(np.arange(F)[:, None] - np.arange(F)[None, :])
    R = r[idx]
    s = np.linalg.solve(R, b)
    return dict(_result(np.dot(b, s)), cond=float(np.linalg.cond(R)))


def bar_db(comp_dev_db, one_minus_coh):
    """The accuracy bar of a row in dB: 16 x the deviation of the fp64 composition from the
    yardstick on that row, plus the dB change of 256 fp64 roundings in coh."""
    return 16.0 * comp_dev_db + (10.0 / np.log(10.0)) * 256 * 2.0 ** -53 / one_minus_coh


# ------------------------------------------------------------------ the case table
CHUNK = 2048  # VRVQ_SDR_CHUNK (tests/test_sdr.py compares with the header)
SIGNALS = ("white", "ar1", "lowpass", "brown", "tones")
NOISE_DB = (10.0, 30.0, 60.0)   # the L = 3 estimates of each of the B = 2 references
# (signal, samples, filter_length): every sample count below, at and above F = 512 and around a
# chunk edge, ten chunks, every filter length, every signal family at F = 512
CASES = [
    ("white", 300, 512), ("ar1", 511, 512), ("lowpass", 512, 512), ("brown", 513, 512),
    ("tones", CHUNK - 1, 512), ("white", CHUNK + 1, 512), ("ar1", 20000, 512),
    ("lowpass", 20000, 512), ("brown", 20000, 512), ("tones", 20000, 512),
    ("lowpass", CHUNK + 1, 1), ("brown", 300, 1), ("ar1", CHUNK + 1, 2), ("tones", 513, 2),
    ("white", 20000, 64), ("lowpass", CHUNK - 1, 64),
]
COND_MAX = 1e8


def signal(kind: str, n: int, rng) -> np.ndarray:
    """One reference row of n samples, float64 before its fp32 rounding."""
    w = rng.standard_normal(n + 256)
    if kind == "white":
        x = 0.3 * w[:n]
    elif kind == "ar1":
        x = np.empty(n + 256)
        acc = 0.0
        for i, v in enumerate(w):
            acc = 0.9 * acc + v
            x[i] = acc
        x = 0.1 * x[256:]
    elif kind == "lowpass":  # 129-tap Hamming-windowed sinc, cutoff at half the band
        k = np.arange(129) - 64
        h = 0.5 * np.sinc(0.5 * k) * np.hamming(129)
        x = 0.5 * np.convolve(w, h, mode="full")[128:128 + n]
    elif kind == "brown":
        x = np.cumsum(w[:n])
        x = 0.5 * x / np.max(np.abs(x))
    elif kind == "tones":
        i = np.arange(n)
        x = 0.3 * np.sin(2 * np.pi * 0.0371 * i) + 0.3 * np.sin(2 * np.pi * 0.2113 * i + 1.0) \
            + 1e-3 * w[:n]
    else:
        raise ValueError(kind)
    return x


FIR = np.array([0.0, 0.9, 0.25, -0.1])  # the "light filter": a one-sample delay and a tilt


def make_rows(kind: str, n: int, seed: int = 0):
    """(est (6, n), ref (2, n)) float32, level-major: est row l * 2 + b is the FIR-filtered
    reference b plus white noise NOISE_DB[l] dB below it."""
    rng = np.random.default_rng(seed + 7919 * SIGNALS.index(kind) + n)
    ref = np.stack([signal(kind, n, rng) for _ in range(2)]).astype(np.float32)
    est = np.empty((6, n), np.float32)
    for l, db in enumerate(NOISE_DB):
        for b in range(2):
            y = np.convolve(ref[b].astype(np.float64), FIR)[:n]
            noise = rng.standard_normal(n)
            noise *= np.sqrt(np.sum(y * y) / np.sum(noise * noise) / 10 ** (db / 10))
            est[l * 2 + b] = (y + noise).astype(np.float32)
    return est, ref


@functools.lru_cache(maxsize=None)
def case_data(case: int):
    kind, n, _F = CASES[case]
    est, ref = make_rows(kind, n)
    est.setflags(write=False)
    ref.setflags(write=False)
    return est, ref


@functools.lru_cache(maxsize=None)
def case_refs(case: int):
    """Per row of the case: (yardstick, composition, levinson64) dicts, computed once."""
    _kind, _n, F = CASES[case]
    est, ref = case_data(case)
    return tuple((yardstick(est[r], ref[r % 2], F), composition(est[r], ref[r % 2], F),
                  levinson64(est[r], ref[r % 2], F)) for r in range(est.shape[0]))
