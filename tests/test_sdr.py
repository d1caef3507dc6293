"""BSS-eval SDR without a GPU: the two paths of the NumPy restatement (tests/sdr_ref.py) against
each other and against closed forms, the operator and C-ABI surface, and the argument errors of
bss_sdr, rd_sweep(bss_sdr=...) and solve_quality(metric="bss_sdr")."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import sdr_ref
import vrvq_amd
from vrvq_amd import _lib, ops, utils


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", range(len(sdr_ref.CASES)))
def test_restatement_paths_agree(case):
    """The long-double yardstick (direct lag sums, Levinson) and the fp64 composition (FFT
    correlations, LU) are independent; on every row they agree inside the dB change of an error
    of (cond(R) + 64 log2(N)) * 2^-53 in coh: the solve's share, and the share of the FFT of
    length N, whose lags of unit-norm rows each err by a few log2(N) ulps of 1 before the
    solution's weights add them up. The plain fp64 Levinson passes the GPU test's bar
    on the whole table (if it did not, the table would be wrong, not the bar), and every case's
    condition number is within the table's limit."""
    for row, (yard, comp, lev) in enumerate(sdr_ref.case_refs(case)):
        assert comp["cond"] <= sdr_ref.COND_MAX, (case, row, comp["cond"])
        dev = abs(comp["sdr"] - yard["sdr"])
        n_fft = 2 ** math.ceil(math.log2(2 * sdr_ref.CASES[case][1] - 1))
        loose = (10 / math.log(10)) * (comp["cond"] + 64 * math.log2(n_fft)) * 2.0 ** -53 \
            / yard["one_minus_coh"]
        bar = sdr_ref.bar_db(dev, yard["one_minus_coh"])
        lev_dev = abs(lev["sdr"] - yard["sdr"])
        print(f"case {case} row {row}: sdr {yard['sdr']:.3f} dB, cond {comp['cond']:.2e}, "
              f"composition off {dev:.2e}, Levinson off {lev_dev:.2e}, bar {bar:.2e}")
        assert dev <= loose, (case, row, dev, loose)
        assert lev_dev <= bar, (case, row, lev_dev, bar)


def test_filter_length_one_is_the_eps_free_si_sdr():
    """F = 1: s = b[0] / r[0], coh = b[0]^2 / r[0] = (sum t p)^2 / (sum t^2 sum p^2)."""
    rng = np.random.default_rng(3)
    t = (0.3 * rng.standard_normal(1500) + 0.02).astype(np.float32).astype(np.float64)
    p = (0.8 * t + 0.05 * rng.standard_normal(1500)).astype(np.float32).astype(np.float64)
    c = np.sum(t * p) ** 2 / (np.sum(t * t) * np.sum(p * p))
    want = 10 * math.log10(c / (1 - c))
    for f in (sdr_ref.yardstick, sdr_ref.composition, sdr_ref.levinson64):
        assert abs(f(p, t, 1)["sdr"] - want) <= 1e-10, f.__name__
    # and that is SI-SDR without its eps: alpha t against p - alpha t
    alpha = np.sum(t * p) / np.sum(t * t)
    si = 10 * math.log10(np.sum((alpha * t) ** 2) / np.sum((p - alpha * t) ** 2))
    assert abs(want - si) <= 1e-9


def test_fir_filtered_estimate_scores_far_above_its_si_sdr():
    """est = a causal 40-tap FIR of ref + independent noise 30 dB down: the F = 512 projection
    takes the filter out (30 dB less what the lag sums' truncation at the clip's ends costs, a
    share of about F / n of the energy), SI-SDR counts the filter as distortion."""
    rng = np.random.default_rng(4)
    t = (0.3 * rng.standard_normal(6000)).astype(np.float32)
    h = 0.5 * rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0)
    y = np.convolve(t.astype(np.float64), h)[:6000]
    noise = rng.standard_normal(6000)
    noise *= math.sqrt(np.sum(y * y) / np.sum(noise * noise) / 1000.0)
    p = (y + noise).astype(np.float32)
    sdr = sdr_ref.yardstick(p, t, 512)["sdr"]
    si = sdr_ref.yardstick(p, t, 1)["sdr"]
    print(f"bss sdr {sdr:.2f} dB, si-sdr {si:.2f} dB")
    assert 25 < sdr < 33 and si < 10 and sdr - si > 20


def test_restatement_special_rows_and_options():
    rng = np.random.default_rng(5)
    t = (0.3 * rng.standard_normal(800)).astype(np.float32)
    p = (t + 0.1 * rng.standard_normal(800)).astype(np.float32)
    z = np.zeros_like(t)
    for f in (sdr_ref.yardstick, sdr_ref.composition, sdr_ref.levinson64):
        assert math.isnan(f(z, t, 16)["sdr"]) and math.isnan(f(p, z, 16)["sdr"])
        assert math.isnan(f(p[:0], t[:0], 16)["sdr"])
    # zero_mean is the plain metric of the centred rows; load_diag lowers the score
    a = sdr_ref.yardstick(p + 2, t - 1, 16, zero_mean=True)["sdr"]
    b = sdr_ref.yardstick((p + 2) - (p + 2).astype(np.float64).mean(),
                          (t - 1) - (t - 1).astype(np.float64).mean(), 16)["sdr"]
    assert abs(a - b) <= 1e-9
    assert sdr_ref.yardstick(p, t, 16, load_diag=0.1)["sdr"] < sdr_ref.yardstick(p, t, 16)["sdr"]
    c, d = (sdr_ref.composition(p, t, 16, load_diag=0.1)["sdr"],
            sdr_ref.yardstick(p, t, 16, load_diag=0.1)["sdr"])
    assert abs(c - d) <= 1e-10


# ------------------------------------------------------------------ operator and constants
def test_op_registered_with_fake_kernel():
    lib = ops.load_ops()
    assert lib.bss_sdr.default._schema.name == "vrvq::bss_sdr"
    m = torch.device("meta")
    for est, ref in ((torch.empty(6, 50, device=m), torch.empty(3, 50, device=m)),
                     (torch.empty(6, 1, 50, device=m), torch.empty(3, 1, 50, device=m))):
        for lengths in (None, torch.empty(3, dtype=torch.int64, device=m)):
            out = lib.bss_sdr(est, ref, lengths, 512, False, None)
            assert out.shape == (6,) and out.dtype == torch.float64


def test_constants_mirror_header():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "include", "vrvq.h")).read()
    chunk = int(re.search(r"#define\s+VRVQ_SDR_CHUNK\s+(\d+)", src).group(1))
    assert chunk == _lib.SDR_CHUNK == sdr_ref.CHUNK
    assert _lib.SDR_MAX_FILTER == utils.BSS_SDR_MAX_FILTER == 512
    assert "bss_sdr" in vrvq_amd.__all__ and vrvq_amd.bss_sdr is utils.bss_sdr


# ------------------------------------------------------------------ argument validation
def test_bss_sdr_argument_errors_raise_before_any_kernel():
    """On CPU tensors: a ValueError, not the kernels' "GPU only" RuntimeError, shows the check
    comes first; valid arguments reach the kernels, which refuse CPU tensors."""
    e, r = torch.ones(4, 64), torch.ones(2, 64)
    for est, ref in ((torch.ones(64), r), (e, torch.ones(64)), (torch.ones(4, 2, 64), r),
                     (e, torch.ones(2, 63)), (torch.ones(3, 64), r), (torch.ones(4, 0), r[:, :0])):
        with pytest.raises(ValueError, match="bss_sdr"):
            utils.bss_sdr(est, ref)
    for F in (0, 513, -1):
        with pytest.raises(ValueError, match="filter_length"):
            utils.bss_sdr(e, r, filter_length=F)
    with pytest.raises(ValueError, match="65536 rows"):   # the C-ABI's bound on rows
        utils.bss_sdr(torch.ones(65536, 4), torch.ones(1, 4))
    for bad in ([64], [64, 64, 64]):
        with pytest.raises(ValueError, match="lengths"):
            utils.bss_sdr(e, r, lengths=bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.bss_sdr(e, r, lengths=[64, 32], filter_length=8, zero_mean=True, load_diag=1e-3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.bss_sdr(e.reshape(4, 1, 64), r.reshape(2, 1, 64))


def test_capi_argument_errors():
    lib = _lib.load()
    assert lib.vrvq_version() >= 112
    ERR, C = 10001, _lib.SDR_CHUNK
    n = ctypes.c_longlong(0)
    ref = ctypes.byref(n)
    assert lib.vrvq_bss_sdr_workspace(12, 1, 441000, 512, ref) == 0
    assert n.value == 8 * 13 * (1 + 216 * 514 + 512)
    assert lib.vrvq_bss_sdr_workspace(6, 2, C, 64, ref) == 0
    assert n.value == 8 * 8 * (1 + 66 + 64)
    assert lib.vrvq_bss_sdr_workspace(6, 2, C + 1, 1, ref) == 0 and n.value == 8 * 8 * (1 + 6 + 1)
    for rows, ref_rows, samples, F, out in (
            (0, 1, 8, 8, ref), (-2, 1, 8, 8, ref), (65536, 1, 8, 8, ref), (4, 0, 8, 8, ref),
            (4, -2, 8, 8, ref), (4, 3, 8, 8, ref), (4, 2, 0, 8, ref), (4, 2, -1, 8, ref),
            (4, 2, 2 ** 32 + 1, 8, ref), (4, 2, 8, 0, ref), (4, 2, 8, 513, ref),
            (4, 2, 8, -1, ref), (4, 2, 8, 8, None)):
        assert lib.vrvq_bss_sdr_workspace(rows, ref_rows, samples, F, out) == ERR, \
            (rows, ref_rows, samples, F)
    p = ctypes.c_void_p(16)  # non-null, never dereferenced: the checks return before a launch
    need = 8 * 6 * (1 + 10 + 8)

    def call(est=p, ref=p, rows=4, ref_rows=2, samples=100, lengths=None, F=8, out=p, ws=p,
             ws_bytes=need):
        return lib.vrvq_bss_sdr(est, ref, rows, ref_rows, samples, lengths, F, 0, float("nan"),
                                out, ws, ws_bytes, None)

    for kw in (dict(est=None), dict(ref=None), dict(out=None), dict(ws=None), dict(rows=0),
               dict(rows=-4), dict(ref_rows=0), dict(ref_rows=3), dict(samples=0),
               dict(samples=-1), dict(F=0), dict(F=513), dict(ws_bytes=need - 1),
               dict(ws_bytes=0), dict(samples=C + 1), dict(F=9), dict(ws=ctypes.c_void_p(20)),
               dict(samples=2 ** 32 + 1, ws_bytes=2 ** 50)):
        assert call(**kw) == ERR, kw
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("vrvq_bss_sdr", None, None, 1, 1, 1, None, 1, 0, 0.0, None, None, 0, None)


SMALL = dict(encoder_dim=8, decoder_dim=32, n_codebooks=2)


def test_quality_and_sweep_accept_the_new_name():
    x = torch.zeros(2, 1, 1024)
    vbr = vrvq_amd.DAC_VRVQ(level_min=0.5, level_max=2.0, **SMALL).eval()
    assert utils.METRICS == ("si_sdr", "si_snr", "snr", "l1")
    assert utils.QUALITY_METRICS == ("si_sdr", "si_snr", "snr")
    with pytest.raises(ValueError, match="metric"):
        utils.solve_quality(vbr, x, 10.0, metric="sdr")
    with pytest.raises(ValueError, match="iters"):   # the name passes, the next check fires
        utils.solve_quality(vbr, x, 10.0, metric="bss_sdr", iters=-1)
    with pytest.raises(RuntimeError, match="GPU"):   # valid arguments reach the kernels
        vrvq_amd.solve_quality(vbr, x, 10.0, metric="bss_sdr")
    with pytest.raises(RuntimeError, match="GPU"):
        vrvq_amd.rd_sweep(vbr, x, [1.0], bss_sdr=True)


def test_rd_sweep_without_the_flag_returns_the_old_keys(monkeypatch):
    """rd_sweep(bss_sdr=False) on a stand-in model whose kernels are replaced by tensor code: the
    dict's keys and the summary rows' are the ones before the flag existed, and bss_sdr is not
    called; with the flag, one more column and one more summary entry."""
    calls = []

    class Stub:
        model_type, training, n_codebooks, sample_rate, hop_length = "VBR", False, 2, 44100, 512

        def preprocess(self, audio, _sr):
            return audio

        def encode(self, x, n_quantizers=None, level=1):
            return {"imp_map": torch.full((x.shape[0], 1, 4), 0.5), "z_q_is": None}

        def decode(self, z):
            return z

    monkeypatch.setattr(utils, "sweep_latents", lambda imp, z, levels, nq:
                        (None, torch.zeros(len(levels) * imp.shape[0], 1, 64)))
    monkeypatch.setattr(utils, "signal_metrics", lambda recon, x, lengths: {
        k: torch.zeros(recon.shape[0] // x.shape[0], x.shape[0], dtype=torch.float64)
        for k in utils.METRICS} | {"moments": torch.zeros(1)})
    monkeypatch.setattr(utils, "rate_curve", lambda imp, levels, nq, bits=10:
                        torch.zeros(imp.shape[0], len(levels)))
    monkeypatch.setattr(utils, "check_errors", lambda device: None)
    monkeypatch.setattr(utils, "_bss_sdr", lambda recon, x, lengths: calls.append(1) or
                        torch.ones(recon.shape[0] // x.shape[0], x.shape[0], dtype=torch.float64))
    old = {"si_sdr", "si_snr", "snr", "l1", "moments", "levels", "bpf", "kbps", "recon", "summary"}
    out = utils.rd_sweep(Stub(), torch.zeros(2, 1, 64), [0.5, 1.0])
    assert set(out) == old and not calls
    assert all(set(row) == {"level", "level_scaled", "sisdr", "kbps"} for row in out["summary"])
    out = utils.rd_sweep(Stub(), torch.zeros(2, 1, 64), [0.5, 1.0], bss_sdr=True)
    assert set(out) == old | {"bss_sdr"} and calls == [1]
    assert out["bss_sdr"].shape == (2, 2)
    assert all(row["bss_sdr"] == 1.0 for row in out["summary"])
