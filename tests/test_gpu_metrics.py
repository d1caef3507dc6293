"""Distortion metrics, the rate-distortion sweep and the quality solver on the GPU, judged by the
NumPy float64 restatement of tests/test_metrics.py (each metric directly from the samples).
Needs an MI355X.

Tolerances (C = VRVQ_METRICS_CHUNK): no fp64 summation chain of the kernels exceeds 4096 terms,
so a moment carries at most 4096 * 2^-53 relative error against its sum of |terms|, about
4 sum p^2 for the noise energy S - 2 alpha sum p t + sum p^2. At 60 dB that energy is 1e-6 of
sum p^2: relative error <= 1.8e-6, or 7.8e-6 dB -- the 1e-5 dB of si_sdr / si_snr, and why no
row is built with its noise more than 60 dB down. snr has no such cancellation (1e-9 dB); l1 and
the moments are plain sums (1e-12 relative)."""
import numpy as np
import pytest
import torch

import vrvq_amd
from test_metrics import EPS, metrics_ref, rows_ref
from vrvq_amd import _lib, ops, utils
from vrvq_amd.recipe import load_recipe, synthetic_audio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = _lib.METRICS_CHUNK
NAMES = ("si_sdr", "si_snr", "snr", "l1")
# (R, B, T): one sample; rows at every 4-byte misalignment (odd T); one short of a chunk, a
# whole chunk, one past it (a one-sample last chunk), two chunks and five; many rows of a length
# that is no multiple of anything
SHAPES = [(1, 1, 1), (2, 1, 3), (6, 3, 7), (4, 2, C - 1), (4, 2, C), (3, 3, C + 1),
          (2, 1, 2 * C + 5), (12, 3, 4099)]
DB = [-20.0, 0.0, 20.0, 40.0, 60.0]


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def make_rows(R, B, T, seed=0):
    """ref = 0.3 N(0, 1) + 0.05 (a DC offset); est row r = 0.7 ref[r % B] + noise, the noise
    scaled for DB[r % 5] dB below the scaled reference."""
    rng = np.random.default_rng(1000 * R + 10 * B + T + seed)
    ref = (0.3 * rng.standard_normal((B, T)) + 0.05).astype(np.float32)
    est = np.empty((R, T), np.float32)
    for r in range(R):
        s = 0.7 * ref[r % B].astype(np.float64)
        noise = rng.standard_normal(T)
        scale = np.sqrt(np.sum(s * s) / max(np.sum(noise * noise), 1e-30) / 10 ** (DB[r % 5] / 10))
        est[r] = (s + scale * noise).astype(np.float32)
    return est, ref


def run(est, ref, lengths=None):
    """(metrics (R, 4), moments (R, 8)) as NumPy, from the op."""
    met, mom = ops.signal_metrics(t(est), t(ref), None if lengths is None else t(lengths, np.int64))
    assert met.dtype == mom.dtype == torch.float64
    assert met.shape == (est.shape[0], 4) and mom.shape == (est.shape[0], 8)
    return met.cpu().numpy(), mom.cpu().numpy()


def check_rows(met, mom, want, rows=None):
    """The tolerances of the module docstring, every figure printed before it is judged."""
    rows = range(met.shape[0]) if rows is None else rows
    for r in rows:
        err = {n: abs(met[r, i] - want[n][r]) for i, n in enumerate(NAMES)}
        print(f"row {r}: si_sdr {want['si_sdr'][r]:.4f} dB, |err| " +
              ", ".join(f"{n} {e:.2e}" for n, e in err.items()))
        assert err["si_sdr"] <= 1e-5 and err["si_snr"] <= 1e-5, (r, err)
        assert err["snr"] <= 1e-9, (r, err)
        np.testing.assert_allclose(met[r, 3], want["l1"][r], rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(mom[r], want["moments"][r], rtol=1e-12, atol=0)


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("shape", SHAPES)
def test_metrics_equal_restatement(shape):
    R, B, T = shape
    est, ref = make_rows(R, B, T)
    met, mom = run(est, ref)
    want = rows_ref(est, ref)
    if T >= 4099:  # the rows do span the decades (short rows are capped by eps)
        assert want["si_sdr"].max() - want["si_sdr"].min() > 50 or R < 5
    check_rows(met, mom, want)
    # the (R, 1, T) layout and the dict of utils.signal_metrics: the same bits, (L, B)
    out = utils.signal_metrics(t(est).reshape(R, 1, T), t(ref).reshape(B, 1, T))
    for i, n in enumerate(NAMES):
        assert out[n].shape == (R // B, B)
        np.testing.assert_array_equal(out[n].cpu().numpy().reshape(-1), met[:, i])
    assert out["moments"].shape == (R // B, B, 8)
    np.testing.assert_array_equal(out["moments"].cpu().numpy().reshape(R, 8), mom)


# ------------------------------------------------------------------ 2. special values
def test_special_values():
    T = C + 1
    _, ref = make_rows(1, 1, T)
    zero = np.zeros_like(ref)
    tt = float(np.sum(ref.astype(np.float64) ** 2))
    same = 10 * np.log10((tt + EPS) / EPS)
    met, _ = run(ref, ref)                      # est == ref
    assert abs(met[0, 0] - same) <= 1e-9 and abs(met[0, 2] - same) <= 1e-9 and met[0, 3] == 0
    assert abs(met[0, 1] - metrics_ref(ref, ref)["si_snr"]) <= 1e-9
    met, _ = run(zero, ref)                     # est == 0: 0 dB
    assert np.all(np.abs(met[0, :3]) <= 1e-9)
    assert abs(met[0, 3] - np.abs(ref.astype(np.float64)).mean()) <= 1e-12
    met, mom = run(zero, zero)                  # both zero: 0 dB
    assert np.all(met[0] == 0) and np.all(mom[0, :7] == 0) and mom[0, 7] == T
    met, _ = run(2 * ref, ref)                  # est = 2 ref (tests/test_metrics.py)
    assert abs(met[0, 0] - (same + 20 * np.log10(2))) <= 1e-6 and abs(met[0, 2]) <= 1e-9


def test_nan_stays_in_its_row():
    R, B, T = 6, 3, C + 1
    est, ref = make_rows(R, B, T)
    clean_met, clean_mom = run(est, ref)
    for pos in (0, C - 3, C):                   # first chunk's head and tail, the one-sample chunk
        bad = est.copy()
        bad[4, pos] = np.nan
        met, mom = run(bad, ref)
        assert np.all(np.isnan(met[4])), pos
        keep = [r for r in range(R) if r != 4]
        np.testing.assert_array_equal(met[keep].view(np.uint64), clean_met[keep].view(np.uint64))
        np.testing.assert_array_equal(mom[keep].view(np.uint64), clean_mom[keep].view(np.uint64))


def test_large_mean_row():
    """mean = 10 x standard deviation: si_snr's centred moments lose two decimal digits to the
    cancellation and stay inside the tolerance."""
    T = 2 * C + 5
    rng = np.random.default_rng(7)
    ref = (0.3 * rng.standard_normal((1, T)) + 3.0).astype(np.float32)
    est = (ref + 0.03 * rng.standard_normal((1, T))).astype(np.float32)
    assert 9 < ref.mean() / ref.std() < 11
    want = rows_ref(est, ref)
    assert 15 < want["si_snr"][0] < 25 < want["si_sdr"][0]
    check_rows(*run(est, ref), want)


# ------------------------------------------------------------------ 3. lengths
def test_lengths():
    T = C + 1
    lengths = np.array([0, 1, C, C + 1, T + 5], np.int64)
    est, ref = make_rows(10, 5, T)
    want = rows_ref(est, ref, lengths)
    for r in range(10):                         # what lies past the length must not be read
        n = int(min(lengths[r % 5], T))
        est[r, n:] = np.nan
    for b in range(5):
        ref[b, int(min(lengths[b], T)):] = np.nan
    met, mom = run(est, ref, lengths)
    check_rows(met, mom, want)
    for r in (0, 5):                            # length 0: l1 NaN, 0 dB, n = 0
        assert np.isnan(met[r, 3]) and np.all(met[r, :3] == 0) and np.all(mom[r] == 0)
    np.testing.assert_array_equal(mom[:, 7], np.tile([0, 1, C, C + 1, T], 2))
    neg = run(est, ref, np.array([-3, 1, C, C + 1, T + 5], np.int64))   # clamps at 0 too
    np.testing.assert_array_equal(neg[0].view(np.uint64), met.view(np.uint64))
    out = utils.signal_metrics(t(est), t(ref), lengths=lengths.tolist())
    np.testing.assert_array_equal(out["snr"].cpu().numpy().reshape(-1).view(np.uint64),
                                  met[:, 2].copy().view(np.uint64))


# ------------------------------------------------------------------ 4. batch invariance
def test_rows_do_not_depend_on_the_batch():
    R, B, T = 12, 3, 4099
    est, ref = make_rows(R, B, T)
    est_d, ref_d = t(est), t(ref)
    met, mom = ops.signal_metrics(est_d, ref_d, None)
    again = ops.signal_metrics(est_d, ref_d, None)
    assert torch.equal(met, again[0]) and torch.equal(mom, again[1])
    for r in range(R):
        # as views (the row's address in the batch: T is odd, so rows sit at every 4-byte
        # misalignment) and as copies of their own (16-byte aligned)
        for e, f in ((est_d[r:r + 1], ref_d[r % B:r % B + 1]),
                     (est_d[r:r + 1].clone(), ref_d[r % B:r % B + 1].clone())):
            one_met, one_mom = ops.signal_metrics(e, f, None)
            assert torch.equal(one_met[0], met[r]) and torch.equal(one_mom[0], mom[r]), r


# ------------------------------------------------------------------ 5. graph capture
def test_graph_capture():
    R, B, T = 4, 2, C + 1
    e0, r0 = make_rows(R, B, T)
    e1, r1 = make_rows(R, B, T, seed=1)
    lengths = t([T, C], np.int64)
    eager0 = ops.signal_metrics(t(e0), t(r0), lengths)
    eager1 = ops.signal_metrics(t(e1), t(r1), lengths)
    se, sr = t(e0).clone(), t(r0).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.signal_metrics(se, sr, lengths)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.signal_metrics(se, sr, lengths)
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager0, outs):
        assert torch.equal(e, o)
    se.copy_(t(e1))
    sr.copy_(t(r1))
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager1, outs):
        assert torch.equal(e, o)


# ------------------------------------------------------------------ through the model
LO, HI = 0.125, 6.0
_cache = {}


def golden_model(manifest):
    """The golden_nq8 model (its kwargs and weights) with a level range, and three clips of its
    audio recipe."""
    if not _cache:
        m = manifest["golden_nq8"]
        model = vrvq_amd.DAC_VRVQ(**m["kwargs"], level_min=LO, level_max=HI)
        load_recipe(model, m["weight_seed"])
        _cache["model"] = model.to(DEV).eval()
        _cache["audio"] = t(synthetic_audio(3, m["length"], seed=m["audio_seed"]))
    return _cache["model"], _cache["audio"]


def test_rd_sweep(manifest):
    model, audio = golden_model(manifest)
    levels, nq, B = [0.25, 1.0, 2.0], model.n_codebooks, 3
    out = utils.rd_sweep(model, audio, levels)
    sweep = utils.level_sweep(model, audio, levels)
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
        imp = model.encode(x, None, 1)["imp_map"]
    T, frames = x.shape[-1], imp.shape[-1]
    recon = torch.cat([s["recon"] for s in sweep])
    assert torch.equal(out["recon"], recon)
    direct = utils.signal_metrics(recon, x)
    for n in NAMES + ("moments",):
        assert out[n].dtype == torch.float64 and torch.equal(out[n], direct[n]), n
        assert out[n].shape[:2] == (3, B)
    assert out["levels"].tolist() == levels and out["levels"].dtype == torch.float32
    assert torch.equal(out["bpf"], utils.rate_curve(imp, levels, nq).t())
    assert out["kbps"].shape == (3, B) and out["kbps"].dtype == torch.float64
    for li, s in enumerate(sweep):
        bits = (out["bpf"][li].to(torch.float64) * frames).round().sum().item()
        assert bits == round(s["bpf"] * B * frames), li
        row = out["summary"][li]
        assert set(row) == {"level", "level_scaled", "sisdr", "kbps"}
        assert row["level"] == levels[li] and row["level_scaled"] == levels[li] * nq
        assert row["sisdr"] == out["si_sdr"][li].mean().item()
        assert abs(row["kbps"] - s["kbps"]) <= 1e-6 * s["kbps"]
    met = np.stack([out[n].cpu().numpy().reshape(-1) for n in NAMES], 1)
    mom = out["moments"].cpu().numpy().reshape(-1, 8)
    check_rows(met, mom, rows_ref(recon.cpu().numpy().reshape(-1, T),
                                  x.cpu().numpy().reshape(-1, T)))
    # lengths (the samples before padding) and a decode cap of one level's clips
    n0 = audio.shape[-1]
    cut = utils.rd_sweep(model, audio, levels, lengths=[n0] * B, max_decode_clips=B)
    assert cut["moments"][..., 7].eq(n0).all() and torch.equal(cut["bpf"], out["bpf"])
    met = np.stack([cut[n].cpu().numpy().reshape(-1) for n in NAMES], 1)
    check_rows(met, cut["moments"].cpu().numpy().reshape(-1, 8),
               rows_ref(cut["recon"].cpu().numpy().reshape(-1, T), x.cpu().numpy().reshape(-1, T),
                        [n0] * B))


def measure_at(model, x, enc, levels, col):
    """The solver's pass at per-clip levels, from the ops: (mask, z_q, recon, value)."""
    B, nq = x.shape[0], model.n_codebooks
    imp = enc["imp_map"].reshape(B, -1)
    rows = ops.scale_imp_rows(imp, levels)
    mask = ops.mask_hard(ops.scale_imp(rows, 1.0, float(nq)).reshape(B, 1, -1), nq)
    z_q = ops.masked_sum(enc["z_q_is"], mask)
    recon = model.decode(z_q)
    return mask, z_q, recon, ops.signal_metrics(recon, x, None)[0][:, col]


def test_solve_quality(manifest):
    model, audio = golden_model(manifest)
    B, nq, iters = 3, model.n_codebooks, 6
    ends = utils.rd_sweep(model, audio, [LO, HI])
    v_lo, v_hi = ends["si_sdr"][0].cpu().numpy(), ends["si_sdr"][1].cpu().numpy()
    print("si_sdr at level_min", v_lo, "at level_max", v_hi)
    targets = ((v_lo + v_hi) / 2).tolist()
    out = utils.solve_quality(model, audio, targets, iters=iters)
    assert set(out) == {"level", "value", "level_lo", "value_lo", "status", "bpf", "kbps",
                        "mask_imp", "z_q", "codes", "recon"}
    assert (out["level"].dtype, out["value"].dtype, out["status"].dtype) == \
        (torch.float32, torch.float64, torch.int32)
    status = out["status"].tolist()
    level, level_lo = out["level"].cpu().numpy(), out["level_lo"].cpu().numpy()
    value, value_lo = out["value"].cpu().numpy(), out["value_lo"].cpu().numpy()
    print("status", status, "level", level, "value", value, "level_lo", level_lo, "value_lo",
          value_lo)
    width = (HI / LO) ** (2.0 ** -iters) * (1 + 2.0 ** -20)
    assert 0 in status  # the bracket contract below is exercised
    for b in range(B):
        if v_hi[b] - v_lo[b] > 1e-3:
            assert status[b] == 0
            assert value[b] >= targets[b] and not value_lo[b] >= targets[b]
            assert np.float32(LO) <= level_lo[b] < level[b] <= np.float32(HI)
            assert float(level[b]) / float(level_lo[b]) <= width
        elif v_lo[b] - v_hi[b] > 1e-3:
            # the synthetic weights' SI-SDR is not monotone in the level: a clip that is worse at
            # level_max than at level_min misses the midpoint at level_max, which is status 1
            assert status[b] == 1 and level[b] == level_lo[b] == np.float32(HI)
            assert value[b] < targets[b] and value_lo[b] < targets[b]
        else:  # a flat clip: which side of the target an end falls on is rounding
            assert status[b] in (0, 1, 2)
            if status[b]:
                assert level[b] == level_lo[b] == np.float32(HI if status[b] == 1 else LO)
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
        enc = model.encode(x, None, out["level"])
        assert torch.equal(enc["mask_imp"], out["mask_imp"])
        assert torch.equal(enc["codes"], out["codes"])
        frames = enc["mask_imp"].shape[-1]
        for b in range(B):
            bits = round(utils.cal_bpf_from_mask(enc["mask_imp"][b:b + 1].contiguous(),
                                                 [10] * nq) * frames)
            assert bits == round(out["bpf"][b].item() * frames)
        plain = model.encode(x, None, 1)
        mask, z_q, recon, val = measure_at(model, x, plain, out["level"], 0)
        assert torch.equal(mask, out["mask_imp"]) and torch.equal(z_q, out["z_q"])
        assert torch.equal(recon, out["recon"]) and torch.equal(val, out["value"])
    rate = np.floor(44100 / 512) / 1000
    np.testing.assert_allclose(out["kbps"].cpu().numpy(),
                               out["bpf"].cpu().numpy().astype(np.float64) * rate, rtol=1e-15)
    # out of reach on either side, one target for all clips, another metric
    high = utils.solve_quality(model, audio, 1e9, iters=2, metric="snr")
    assert high["status"].tolist() == [1] * B and high["level"].tolist() == [HI] * B
    assert high["level_lo"].tolist() == [HI] * B
    low = utils.solve_quality(model, audio, torch.full((B,), -1e9), iters=2, metric="si_snr")
    assert low["status"].tolist() == [2] * B and low["level"].tolist() == [LO] * B
    with torch.no_grad():
        val = measure_at(model, x, plain, low["level"], 1)[3]
    assert torch.equal(val, low["value"])
    utils.check_errors(DEV)
