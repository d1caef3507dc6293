"""Distortion metrics and the quality solver without a GPU: the NumPy float64 restatement of the
metric formulas (the judge of tests/test_gpu_metrics.py) against hand values, the operator and
C-ABI surface, the solver's bisection update against a scalar restatement, and the argument
errors of solve_quality / rd_sweep.

The restatement computes each metric directly from the samples -- the noise per element as
alpha * t - p, the means removed per element -- not from the moment sums the kernels use."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import vrvq_amd
from vrvq_amd import _lib, ops, utils

EPS = 2.0 ** -23  # float32 eps: torchmetrics' regulariser for fp32 input


# ------------------------------------------------------------------ the NumPy restatement
def si_ratio_db(p, t):
    """torchmetrics scale_invariant_signal_distortion_ratio, zero_mean=False, in float64."""
    alpha = (np.sum(p * t) + EPS) / (np.sum(t * t) + EPS)
    scaled = alpha * t
    noise = scaled - p
    return 10 * np.log10((np.sum(scaled * scaled) + EPS) / (np.sum(noise * noise) + EPS))


def metrics_ref(p, t):
    """One row: {"si_sdr", "si_snr", "snr", "l1", "moments"} of est p against ref t."""
    p, t = np.asarray(p, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    n, d = p.size, p - t
    with np.errstate(all="ignore"):
        return {
            "si_sdr": si_ratio_db(p, t),
            "si_snr": si_ratio_db(p - p.mean(), t - t.mean()) if n else 0.0,
            "snr": 10 * np.log10((np.sum(t * t) + EPS) / (np.sum(d * d) + EPS)),
            "l1": np.sum(np.abs(d)) / n if n else float("nan"),
            "moments": np.array([p.sum(), t.sum(), (p * t).sum(), (p * p).sum(), (t * t).sum(),
                                 np.abs(d).sum(), (d * d).sum(), n], np.float64),
        }


def rows_ref(est, ref, lengths=None):
    """metrics_ref of every row of est (R, T) against row r % B of ref (B, T), stacked."""
    R, B = est.shape[0], ref.shape[0]
    out = []
    for r in range(R):
        n = est.shape[1] if lengths is None else int(np.clip(lengths[r % B], 0, est.shape[1]))
        out.append(metrics_ref(est[r, :n], ref[r % B, :n]))
    return {k: np.stack([np.asarray(o[k]) for o in out]) for k in out[0]}


# ------------------------------------------------------------------ restatement vs hand values
def test_restatement_hand_values():
    rng = np.random.default_rng(0)
    t = (0.3 * rng.standard_normal(1000) + 0.05).astype(np.float32).astype(np.float64)
    tt = float(np.sum(t * t))
    same = 10 * math.log10((tt + EPS) / EPS)
    m = metrics_ref(t, t)
    assert abs(m["si_sdr"] - same) < 1e-9 and abs(m["snr"] - same) < 1e-9 and m["l1"] == 0
    z = np.zeros_like(t)
    m = metrics_ref(z, t)      # alpha = eps / (tt + eps): S and N both vanish against eps
    assert abs(m["si_sdr"]) < 1e-9 and abs(m["si_snr"]) < 1e-9
    assert abs(m["snr"]) < 1e-9 and abs(m["l1"] - np.abs(t).mean()) < 1e-15
    m = metrics_ref(z, z)
    assert m["si_sdr"] == 0 and m["si_snr"] == 0 and m["snr"] == 0 and m["l1"] == 0
    e = metrics_ref(z[:0], z[:0])
    assert e["si_sdr"] == 0 and e["si_snr"] == 0 and e["snr"] == 0 and math.isnan(e["l1"])
    assert e["moments"].tolist() == [0.0] * 8


def test_restatement_scaled_estimate():
    """p = 2 t. SNR: sum (p - t)^2 = sum t^2, 0 dB. SI-SDR: the projection alpha t is p up to
    eps, so the noise vanishes and the formula gives 10 log10((4 tt + eps) / eps) -- the p = t
    value plus 20 log10(2), not the p = t value itself: with no noise left the eps in the
    denominator is all there is, and the numerator alpha^2 tt carries the scale. Scale invariance
    holds where there is noise: (2 p, t) and (p, t) then agree."""
    rng = np.random.default_rng(1)
    t = (0.3 * rng.standard_normal(1000) + 0.05).astype(np.float32).astype(np.float64)
    same = metrics_ref(t, t)["si_sdr"]
    m = metrics_ref(2 * t, t)
    assert abs(m["snr"]) < 1e-9
    assert abs(m["si_sdr"] - (same + 20 * math.log10(2))) < 1e-6
    assert abs(m["si_sdr"] - 10 * math.log10((4 * np.sum(t * t) + EPS) / EPS)) < 1e-6
    p = 0.7 * t + 0.01 * rng.standard_normal(1000)
    a, b = metrics_ref(p, t), metrics_ref(2 * p, t)
    # up to eps against the noise energy N = 1000 * 0.01^2 = 0.1: 4.34 dB * eps / N = 5e-6 dB
    assert abs(a["si_sdr"] - b["si_sdr"]) < 1e-5 and abs(a["si_snr"] - b["si_snr"]) < 1e-5
    assert 20 < a["si_sdr"] < 40


# ------------------------------------------------------------------ operators and fakes
def test_metrics_op_registered_with_fake_kernel():
    lib = ops.load_ops()
    assert lib.signal_metrics.default._schema.name == "vrvq::signal_metrics"
    m = torch.device("meta")
    for est, ref in ((torch.empty(6, 50, device=m), torch.empty(3, 50, device=m)),
                     (torch.empty(6, 1, 50, device=m), torch.empty(3, 1, 50, device=m))):
        for lengths in (None, torch.empty(3, dtype=torch.int64, device=m)):
            met, mom = lib.signal_metrics(est, ref, lengths)
            assert met.shape == (6, 4) and mom.shape == (6, 8)
            assert met.dtype == mom.dtype == torch.float64


def test_metrics_reject_cpu_tensors():
    ops.load_ops()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.signal_metrics(torch.ones(2, 8), torch.ones(1, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        utils.signal_metrics(torch.ones(2, 1, 8), torch.ones(2, 1, 8), lengths=[8, 4])
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.signal_metrics(torch.ones(2, 8), torch.ones(2, 8))


def test_chunk_constant_mirrors_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "vrvq.h")).read()
    assert int(re.search(r"#define\s+VRVQ_METRICS_CHUNK\s+(\d+)", src).group(1)) \
        == _lib.METRICS_CHUNK
    # whole float4 groups for 256 threads, and a per-thread chain far below 4096 terms
    assert _lib.METRICS_CHUNK % 1024 == 0 and _lib.METRICS_CHUNK // 256 <= 4096


# ------------------------------------------------------------------ C-ABI argument checks
def test_capi_argument_errors():
    lib = _lib.load()
    assert lib.vrvq_version() >= 102
    p = ctypes.c_void_p(16)  # non-null, never dereferenced: the checks return before a launch
    ERR = 10001
    C = _lib.METRICS_CHUNK
    n = ctypes.c_longlong(0)
    assert lib.vrvq_signal_metrics_workspace(12, 441000, ctypes.byref(n)) == 0
    assert n.value == 12 * 27 * 7 * 8
    assert lib.vrvq_signal_metrics_workspace(3, C, ctypes.byref(n)) == 0 and n.value == 3 * 56
    assert lib.vrvq_signal_metrics_workspace(3, C + 1, ctypes.byref(n)) == 0 and n.value == 6 * 56
    for rows, samples, out in ((0, 8, ctypes.byref(n)), (-1, 8, ctypes.byref(n)),
                               (2, 0, ctypes.byref(n)), (2, -5, ctypes.byref(n)), (2, 8, None),
                               (2, 2 ** 32 + 1, ctypes.byref(n)), (65536, 8, ctypes.byref(n))):
        assert lib.vrvq_signal_metrics_workspace(rows, samples, out) == ERR, (rows, samples)

    def call(est=p, ref=p, rows=4, ref_rows=2, samples=100, lengths=None, metrics=p, moments=p,
             ws=p, ws_bytes=4 * 56):
        return lib.vrvq_signal_metrics(est, ref, rows, ref_rows, samples, lengths, metrics,
                                       moments, ws, ws_bytes, None)

    for kw in (dict(est=None), dict(ref=None), dict(metrics=None), dict(ws=None), dict(rows=0),
               dict(rows=-4), dict(ref_rows=0), dict(ref_rows=-2), dict(ref_rows=3),
               dict(samples=0), dict(samples=-1), dict(ws_bytes=4 * 56 - 1), dict(ws_bytes=0),
               dict(samples=C + 1), dict(samples=2 ** 32 + 1, ws_bytes=2 ** 40)):
        assert call(**kw) == ERR, kw
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("vrvq_signal_metrics", None, None, 1, 1, 1, None, None, None, None, 0, None)


# ------------------------------------------------------------------ the bisection update
def solve_scalar(f, target, lmin, lmax, iters):
    """One clip in NumPy scalars: (lo, hi, value_lo, value_hi, status) after `iters` rounds."""
    lmin, lmax = np.float32(lmin), np.float32(lmax)
    v_min, v_max = f(lmin), f(lmax)
    if not v_max >= target:
        lo, hi, v_lo, v_hi, st = lmax, lmax, v_max, v_max, 1
    elif v_min >= target:
        lo, hi, v_lo, v_hi, st = lmin, lmin, v_min, v_min, 2
    else:
        lo, hi, v_lo, v_hi, st = lmin, lmax, v_min, v_max, 0
    for _ in range(iters):
        mid = np.float32(np.sqrt(np.float64(lo) * np.float64(hi)))
        v = f(mid)
        if v >= target:
            hi, v_hi = mid, v
        else:
            lo, v_lo = mid, v
    return lo, hi, v_lo, v_hi, st


STAIRS = [0.2, 0.35, 0.7, 1.1, 2.0, 3.3, 5.0]


def staircase(level):          # monotone: 3 dB per step passed
    return 3.0 * sum(float(level) >= s for s in STAIRS)


def bumpy(level):              # not monotone in the level
    x = math.log2(float(level))
    return 4.0 * x + 6.0 * math.sin(5.0 * x)


def nan_below_one(level):
    return float("nan") if float(level) < 1.0 else 2.0 * float(level)


CLIPS = [  # (metric function, target, expected status)
    (staircase, 10.0, 0), (staircase, 2.5, 0), (staircase, 21.0, 0), (bumpy, 3.0, 0),
    (bumpy, -1.0, 0), (staircase, 22.0, 1), (bumpy, 100.0, 1), (staircase, 0.0, 2),
    (bumpy, -100.0, 2), (nan_below_one, 5.0, 0), (lambda lv: float("nan"), 1.0, 1),
]


@pytest.mark.parametrize("iters", [0, 1, 6, 8, 12])
def test_bisection_update_equals_scalar_restatement(iters):
    LMIN, LMAX = 0.125, 6.0
    B = len(CLIPS)
    fs = [c[0] for c in CLIPS]
    target = torch.tensor([c[1] for c in CLIPS], dtype=torch.float64)

    def measure(levels):
        return torch.tensor([f(np.float32(lv)) for f, lv in zip(fs, levels.tolist())],
                            dtype=torch.float64)

    lmin, lmax = torch.full((B,), LMIN), torch.full((B,), LMAX)
    lo, hi, v_lo, v_hi, status = utils.quality_bisect_init(lmin, lmax, measure(lmin),
                                                           measure(lmax), target)
    assert status.dtype == torch.int32 and status.tolist() == [c[2] for c in CLIPS]
    for _ in range(iters):
        mid = utils.quality_midpoint(lo, hi)
        assert mid.dtype == torch.float32
        lo, hi, v_lo, v_hi = utils.quality_bisect_update(lo, hi, v_lo, v_hi, mid, measure(mid),
                                                         target)
    assert lo.dtype == hi.dtype == torch.float32 and v_lo.dtype == v_hi.dtype == torch.float64
    width = (LMAX / LMIN) ** (2.0 ** -iters) * (1 + 2.0 ** -20)
    for b, (f, tgt, st) in enumerate(CLIPS):
        want = solve_scalar(f, tgt, LMIN, LMAX, iters)
        assert want[4] == st
        got_lo, got_hi = lo[b].numpy(), hi[b].numpy()
        assert got_lo.view(np.uint32) == want[0].view(np.uint32), (b, got_lo, want[0])
        assert got_hi.view(np.uint32) == want[1].view(np.uint32), (b, got_hi, want[1])
        for got, ref in ((v_lo[b].item(), want[2]), (v_hi[b].item(), want[3])):
            assert got == ref or (math.isnan(got) and math.isnan(ref))
        if st == 0:  # the bracket contract (a NaN value_lo is a miss)
            assert v_hi[b].item() >= tgt and not v_lo[b].item() >= tgt
            assert v_hi[b].item() == f(got_hi)
            assert got_lo < got_hi and float(got_hi) / float(got_lo) <= width
        elif st == 1:
            assert got_lo == got_hi == np.float32(LMAX) and not v_hi[b].item() >= tgt
        else:
            assert got_lo == got_hi == np.float32(LMIN) and v_hi[b].item() >= tgt


# ------------------------------------------------------------------ argument errors
SMALL = dict(encoder_dim=8, decoder_dim=32, n_codebooks=2)


def test_quality_argument_errors_raise_before_any_kernel():
    """All on CPU models: a ValueError, not the kernels' "GPU only" RuntimeError, shows the check
    comes first."""
    x = torch.zeros(2, 1, 1024)
    vbr = vrvq_amd.DAC_VRVQ(level_min=0.5, level_max=2.0, **SMALL).eval()
    cbr = vrvq_amd.DAC_VRVQ(model_type="CBR", **SMALL).eval()
    with pytest.raises(ValueError, match="VBR"):
        utils.solve_quality(cbr, x, 10.0)
    with pytest.raises(ValueError, match="VBR"):
        utils.rd_sweep(cbr, x, [1.0])
    for kw in (dict(level_min=0.5), dict(level_max=2.0), dict()):
        open_range = vrvq_amd.DAC_VRVQ(**kw, **SMALL).eval()
        with pytest.raises(ValueError, match="level_min and level_max"):
            utils.solve_quality(open_range, x, 10.0)
    for bad in ([10.0], [1.0, 2.0, 3.0], torch.zeros(3), np.zeros(1)):
        with pytest.raises(ValueError, match="targets for 2 clips"):
            utils.solve_quality(vbr, x, bad)
    for name in ("l1", "sdr", "SI_SDR", ""):
        with pytest.raises(ValueError, match="metric"):
            utils.solve_quality(vbr, x, 10.0, metric=name)
    with pytest.raises(ValueError, match="iters"):
        utils.solve_quality(vbr, x, 10.0, iters=-1)
    with pytest.raises(ValueError, match="no levels"):
        utils.rd_sweep(vbr, x, [])
    with pytest.raises(ValueError, match="lengths"):
        utils.rd_sweep(vbr, x, [1.0], lengths=[5])
    vbr.train()
    with pytest.raises(ValueError, match="eval"):
        utils.solve_quality(vbr, x, 10.0)
    with pytest.raises(ValueError, match="eval"):
        utils.rd_sweep(vbr, x, [1.0])
    # valid arguments reach the kernels, which refuse CPU tensors
    vbr.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        vrvq_amd.solve_quality(vbr, x, [10.0, 12.0], metric="snr")
    with pytest.raises(RuntimeError, match="GPU"):
        vrvq_amd.rd_sweep(vbr, x, [0.5, 1.0])
