"""Spectral distances on the GPU (csrc/spectral.hip), judged by the NumPy float64 restatement of
tests/spectral_ref.py. Needs an MI355X.

The bar, per (row, scale) and per term: |got - want| <= 4 t + (log2 W + 4) 2^-24 s.
  t  the largest error, over all the test's rows and lengths at that scale, of the torch fp32
     composition of vrvq_amd/losses.py (torch.stft, abs, the dense mel product, clamp / pow /
     log10, a mean per row) on the same inputs on the same GPU, judged by the same restatement;
     4 is the project's factor for "as good as torch fp32" (DESIGN.md section 4).
  s  pow * 0.4343 for the log term (d log10(x) = 0.4343 dx / x: a relative error of the magnitude
     becomes that much of the term), the restatement's mean of E + R for the magnitude term.
  (log2 W + 4) 2^-24: one fp32 rounding per butterfly stage of a length-W transform plus window,
     magnitude, projection and the pairing of two magnitudes, all taken to align.
Independently of it, on the noise rows, |got - want| <= 1e-4 max(1, |want|), the README's parity
bar (the pure tone of test_silent_estimate_against_a_full_scale_sine is judged by the bar alone;
its docstring says why). Every figure is printed before it is judged. Largest |err| / bar measured
on an MI355X: 0.29 on the noise rows ((512, 0)), 0.57 on the tone ((2048, 150))."""
import math

import numpy as np
import pytest
import torch

import spectral_ref as S
import vrvq_amd
from vrvq_amd import _lib, losses, ops, utils
from vrvq_amd.discriminator import stft
from vrvq_amd.recipe import load_recipe, synthetic_audio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCALES = [(32, 5), (64, 10), (128, 20), (256, 40), (512, 80), (1024, 160), (2048, 320),
          (2048, 150), (2048, 0), (512, 0)]
BASE = dict(windows=(32, 64, 128, 256, 512, 1024, 2048), n_mels=(5, 10, 20, 40, 80, 160, 320),
            pow=1.0, mag_weight=0.0)                       # conf/base.yml MelSpectrogramLoss
DB = [-20.0, 0.0, 20.0, 40.0, 60.0]
EPS, POW = 1e-5, 2.0


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def make_rows(R, B, T, seed=0):
    """ref = 0.3 N(0, 1) + 0.05; est row r = 0.7 ref[r % B] + noise DB[r % 5] dB below it."""
    rng = np.random.default_rng(1000 * R + 10 * B + T + seed)
    ref = (0.3 * rng.standard_normal((B, T)) + 0.05).astype(np.float32)
    est = np.empty((R, T), np.float32)
    for r in range(R):
        s = 0.7 * ref[r % B].astype(np.float64)
        noise = rng.standard_normal(T)
        scale = np.sqrt(np.sum(s * s) / max(np.sum(noise * noise), 1e-30) / 10 ** (DB[r % 5] / 10))
        est[r] = (s + scale * noise).astype(np.float32)
    return est, ref


def lengths_of(window):
    """W/2 + 1 (the minimum: frame 1 reflects on both sides at once), W = 4 hop (a whole number
    of hops), the lengths of exactly F - 1, F and F + 1 frames (one short of a tile, a whole tile,
    one frame in a second tile) and 4099 (odd: every 4-byte misalignment of a row)."""
    hop, F = window // 4, _lib.spectral_tile_frames(window)
    by_frames = [(f - 1) * hop + 1 for f in (F - 1, F, F + 1)]
    assert [1 + n // hop for n in by_frames] == [F - 1, F, F + 1]
    return sorted({window // 2 + 1, window, 4099, *by_frames})


def run(est, ref, lengths=None, **kw):
    """spectral_distance on NumPy rows -> NumPy {"distance" (R,), "log", "mag" (R, S)}."""
    out = utils.spectral_distance(t(est), t(ref), lengths=lengths, **kw)
    B, S_ = ref.shape[0], len(kw["windows"])
    L = est.shape[0] // B
    assert out["distance"].shape == (L, B) and out["log"].shape == out["mag"].shape == (L, B, S_)
    assert all(v.dtype == torch.float64 and v.device.type == "cuda" for v in out.values())
    return {"distance": out["distance"].reshape(-1).cpu().numpy(),
            "log": out["log"].reshape(-1, S_).cpu().numpy(),
            "mag": out["mag"].reshape(-1, S_).cpu().numpy()}


def torch_fp32_terms(est, ref, window, n_mels, pow=POW, eps=EPS):
    """The per-row torch composition of losses.py in fp32 on the GPU: (log (R,), mag (R,))."""
    e = t(est)[:, None, :]
    r = t(ref)[:, None, :].repeat(est.shape[0] // ref.shape[0], 1, 1)
    if n_mels:
        E = losses.mel_spectrogram(e, 44100, n_mels, window, window // 4)
        R_ = losses.mel_spectrogram(r, 44100, n_mels, window, window // 4)
    else:
        E, R_ = stft(e, window, window // 4).abs(), stft(r, window, window // 4).abs()
    log = (E.clamp(eps).pow(pow).log10() - R_.clamp(eps).pow(pow).log10()).abs().mean(dim=(1, 2, 3))
    mag = (E - R_).abs().mean(dim=(1, 2, 3))
    return log.double().cpu().numpy(), mag.double().cpu().numpy()


def judge(cases, window, pow=POW, parity=True):
    """cases: [(label, got, want, (torch log, torch mag))] at one scale (S = 1). Applies the
    module docstring's bar with t over all the cases' rows, and with `parity` the 1e-4 bar as
    well; returns the largest ratio to the former."""
    t_log = max(np.abs(tl - w["log"][:, 0]).max() for _, _, w, (tl, _) in cases)
    t_mag = max(np.abs(tm - w["mag"][:, 0]).max() for _, _, w, (_, tm) in cases)
    k = (math.log2(window) + 4) * 2.0 ** -24
    print(f"W {window}: torch fp32 error t: log {t_log:.3e}, mag {t_mag:.3e}; "
          f"floor: log {k * pow * 0.4343:.3e}")
    worst, fails = 0.0, []
    for label, got, want, _ in cases:
        for r in range(want["log"].shape[0]):
            bars = {"log": 4 * t_log + k * pow * 0.4343, "mag": 4 * t_mag + k * want["level"][r, 0]}
            for term in ("log", "mag"):
                g, w = got[term][r, 0], want[term][r, 0]
                err, bar = abs(g - w), bars[term]
                print(f"  {label} row {r} {term}: want {w:.9g} got {g:.9g} |err| {err:.3e} "
                      f"bar {bar:.3e} ratio {err / bar:.3f}")
                worst = max(worst, err / bar)
                if not (err <= bar and (not parity or err <= 1e-4 * max(1.0, abs(w)))):
                    fails.append((label, r, term, err, bar))
            d = abs(got["distance"][r] - want["distance"][r])
            if not d <= bars["log"] + bars["mag"]:
                fails.append((label, r, "distance", d, bars["log"] + bars["mag"]))
    print(f"W {window}: largest |err| / bar {worst:.3f}")
    assert not fails, fails
    return worst


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("scale", SCALES, ids=[f"{w}-{m}" for w, m in SCALES])
def test_terms_equal_restatement(scale):
    window, n_mels = scale
    kw = dict(windows=(window,), n_mels=(n_mels,), pow=POW, clamp_eps=EPS)
    cases = []
    for T in lengths_of(window):
        est, ref = make_rows(6, 3, T)
        got, want = run(est, ref, **kw), S.distance_rows(est, ref, **kw)
        cases.append((f"T {T}", got, want, torch_fp32_terms(est, ref, window, n_mels)))
    judge(cases, window)


# ------------------------------------------------------------------ 2. special values
def test_equal_signals_give_exact_zero():
    est, ref = make_rows(6, 3, 4099)
    same = np.concatenate([ref, ref])
    for kw in (BASE, utils.MEL_DISTANCE, utils.STFT_DISTANCE):
        got = run(same, ref, **kw)
        assert not got["log"].any() and not got["mag"].any() and not got["distance"].any()
        zero = run(np.zeros_like(same), np.zeros_like(ref), **kw)   # every magnitude at the clamp
        assert not zero["log"].any() and not zero["mag"].any() and not zero["distance"].any()


def test_silent_estimate_against_a_full_scale_sine():
    """Every estimate magnitude must be exactly 0, below the clamp: a transform that packed est
    and ref into one complex signal would leak 2^-24 |R| > eps into est's bins.

    Judged by the bar alone, not by the 1e-4 parity bar of the noise rows: a pure tone's linear
    bins far from the tone are, exactly, below or near clamp_eps = 1e-5, while any fp32 transform
    carries rounding of the order 2^-24 x the peak (0.9 * W / 4 = 115 at W = 512: 7e-6) into
    every bin, so which of those bins clear the clamp, and by how much, is rounding. Measured at
    (512, 0): log term 2.74871 against 2.74832 (|err| 3.9e-4, 1.4e-4 of the value; the torch fp32
    composition on the same GPU: 6.5e-4); at (2048, 150) 1.5e-5 (torch: 6.4e-6). That is what the
    4 t part of the bar stands for."""
    T = 4099
    sine = (0.9 * np.sin(2 * np.pi * 1000.0 * np.arange(T) / 44100.0)).astype(np.float32)[None]
    zero = np.zeros_like(sine)
    for window, n_mels in ((2048, 150), (512, 0)):
        kw = dict(windows=(window,), n_mels=(n_mels,), pow=POW, clamp_eps=EPS)
        got, want = run(zero, sine, **kw), S.distance_rows(zero, sine, **kw)
        if (window, n_mels) == (2048, 150):
            assert abs(want["log"][0, 0] - 4.443) < 2e-3 and abs(want["mag"][0, 0] - 0.3845) < 2e-4
        judge([("silent est", got, want, torch_fp32_terms(zero, sine, window, n_mels))], window,
              parity=False)
        # est at the clamp exactly: the log term is then a function of ref alone, the same bits
        # as against an estimate that is silent in another way (-0.0)
        neg = run(-zero, sine, **kw)
        assert neg["log"].tobytes() == got["log"].tobytes()
        # ... and the magnitude term is the mean of R: the other way round gives the same bits
        back = run(sine, zero, **kw)
        assert back["mag"].tobytes() == got["mag"].tobytes()
        assert back["log"].tobytes() == got["log"].tobytes()


def test_digital_silence_in_the_second_half():
    T = 4099
    est, ref = make_rows(6, 3, T)
    est[:, T // 2:] = 0
    ref[:, T // 2:] = 0
    for window, n_mels in ((2048, 150), (512, 0), (32, 5)):
        kw = dict(windows=(window,), n_mels=(n_mels,), pow=POW, clamp_eps=EPS)
        got, want = run(est, ref, **kw), S.distance_rows(est, ref, **kw)
        judge([("half silent", got, want, torch_fp32_terms(est, ref, window, n_mels))], window)


# ------------------------------------------------------------------ 3. determinism
ALL = dict(windows=(32, 64, 128, 256, 512, 1024, 2048, 2048, 512),
           n_mels=(5, 10, 20, 40, 80, 160, 320, 150, 0), pow=POW, mag_weight=1.0)


def raw(est_d, ref_d, kw=ALL, lengths=None):
    out = utils.spectral_distance(est_d, ref_d, lengths=lengths, **kw)
    return torch.cat([out["distance"].reshape(-1, 1), out["log"].flatten(0, 1),
                      out["mag"].flatten(0, 1)], 1)


@pytest.mark.parametrize("T", [4099, 4 * 512 + 1])   # 4 * 512 + 1: F + 1 frames at W = 2048
def test_rows_do_not_depend_on_the_batch(T):
    R, B = 6, 3
    est, ref = make_rows(R, B, T)
    est_d, ref_d = t(est), t(ref)
    full = raw(est_d, ref_d)
    assert torch.isfinite(full).all()
    assert torch.equal(full, raw(est_d, ref_d))
    for r in range(R):
        # as views (the row's address in the batch: T is odd, so rows sit at every 4-byte
        # misalignment) and as copies of their own
        e, f = est_d[r:r + 1], ref_d[r % B:r % B + 1]
        for ee, ff in ((e, f), (e.clone(), f.clone())):
            assert torch.equal(raw(ee, ff)[0], full[r]), r
    # row 4 (against reference 1) as row 0 and as row R - 1 of other batches, whose references are
    # rotated so that the row still meets its own
    for pos in (0, R - 1):
        other, _ = make_rows(R, B, T, seed=7 + pos)
        other[pos] = est[4]
        refs = np.roll(ref, pos % B - 1, axis=0)
        assert (refs[pos % B] == ref[1]).all()
        assert torch.equal(raw(t(other), t(refs))[pos], full[4]), pos


def test_nan_stays_in_its_row():
    R, B, T = 6, 3, 4099
    est, ref = make_rows(R, B, T)
    full = raw(t(est), t(ref))
    bad = est.copy()
    bad[4, 1234] = np.nan
    got = raw(t(bad), t(ref))
    assert torch.isnan(got[4]).all()
    keep = [r for r in range(R) if r != 4]
    assert torch.equal(got[keep], full[keep])
    # with mag_weight = 0 the distance is NaN as well
    out = utils.spectral_distance(t(bad), t(ref), **BASE)
    assert torch.isnan(out["distance"].reshape(-1)[4]) and torch.isfinite(
        out["distance"].reshape(-1)[keep]).all()


# ------------------------------------------------------------------ 4. lengths
def test_lengths_equal_truncated_rows():
    R, B, T = 6, 3, 4099
    est, ref = make_rows(R, B, T)
    kw = dict(windows=(2048, 512, 32), n_mels=(150, 80, 5), pow=POW)
    # W/2 + 1 of the largest window; the middle of a tile at every scale; the full length
    lengths = [1025, 2900, T]
    got = raw(t(est), t(ref), kw, lengths)
    assert torch.isfinite(got).all()
    assert torch.equal(got, raw(t(est), t(ref), kw, t(lengths, np.int64)))
    for r in range(R):
        n = lengths[r % B]
        alone = raw(t(est[r:r + 1, :n]), t(ref[r % B:r % B + 1, :n]), kw)
        assert torch.equal(alone[0], got[r]), r
    want = S.distance_rows(est, ref, lengths=lengths, **kw)
    np.testing.assert_allclose(got[:, 0].cpu().numpy(), want["distance"], rtol=1e-4)


def test_short_rows_are_nan_at_their_scale_only():
    R, B, T = 4, 2, 3000
    est, ref = make_rows(R, B, T)
    kw = dict(windows=(64, 512, 2048), n_mels=(10, 0, 150), pow=POW)
    got = run(est, ref, lengths=[1024, 256], **kw)
    want = S.distance_rows(est, ref, lengths=[1024, 256], **kw)
    for r in range(R):
        short = (2,) if r % B == 0 else (1, 2)          # 1024 <= 2048 / 2; 256 <= 512 / 2 too
        for s in range(3):
            for term in ("log", "mag"):
                assert np.isnan(got[term][r, s]) == (s in short), (r, s, term)
                if s not in short:
                    assert abs(got[term][r, s] - want[term][r, s]) <= 1e-4 * max(
                        1.0, abs(want[term][r, s]))
        assert np.isnan(got["distance"][r])


# ------------------------------------------------------------------ 5. layouts and wrappers
def test_layouts_and_wrappers():
    R, B, T = 6, 3, 4099
    est, ref = make_rows(R, B, T)
    est_d, ref_d = t(est), t(ref)
    flat = utils.spectral_distance(est_d, ref_d, **utils.MEL_DISTANCE)
    deep = utils.spectral_distance(est_d.reshape(R, 1, T), ref_d.reshape(B, 1, T),
                                   **utils.MEL_DISTANCE)
    for k in ("distance", "log", "mag"):
        assert torch.equal(flat[k], deep[k]), k
    assert flat["distance"].shape == (2, B) and flat["log"].shape == (2, B, 2)
    want = S.distance_rows(est, ref, **utils.MEL_DISTANCE)
    np.testing.assert_allclose(flat["distance"].cpu().numpy().reshape(-1), want["distance"],
                               rtol=1e-4)
    np.testing.assert_allclose(flat["log"].cpu().numpy().reshape(R, 2), want["log"], rtol=1e-4)
    # the operator's (R, S, 2) terms and (R,) distance are what the dict reshapes
    tabs, bands, weights = utils._spectral_device_tables(DEV, 44100, [2048, 512], [150, 80],
                                                         [0.0, 0.0], [None, None])
    terms, dist = ops.spectral_distance(est_d, ref_d, None, [2048, 512], [150, 80], tabs, bands,
                                        weights, 1e-5, 2.0)
    assert terms.shape == (R, 2, 2) and dist.shape == (R,)
    assert torch.equal(terms[:, :, 0].reshape(2, B, 2), flat["log"])
    assert torch.equal(terms[:, :, 1].reshape(2, B, 2), flat["mag"])
    assert torch.equal(dist.reshape(2, B), flat["distance"])
    # the wrappers are spectral_distance with the reference classes' defaults
    assert torch.equal(vrvq_amd.mel_distance(est_d, ref_d), flat["distance"])
    assert torch.equal(vrvq_amd.mel_distance(est_d, ref_d, lengths=[T, 2000, 1500]),
                       utils.spectral_distance(est_d, ref_d, lengths=[T, 2000, 1500],
                                               **utils.MEL_DISTANCE)["distance"])
    stft_d = utils.spectral_distance(est_d, ref_d, windows=(2048, 512))["distance"]
    assert torch.equal(vrvq_amd.stft_distance(est_d, ref_d), stft_d)
    # the weights: distance = sum_s (log_weight log_s + mag_weight mag_s)
    w = utils.spectral_distance(est_d, ref_d, windows=(2048, 512), n_mels=(150, 80),
                                log_weight=0.25, mag_weight=3.0)
    np.testing.assert_allclose(
        w["distance"].cpu().numpy(),
        (0.25 * flat["log"] + 3.0 * flat["mag"]).sum(-1).cpu().numpy(), rtol=1e-14)
    # the batch mean is the training loss of losses.py (one clip per row of the batch)
    e3, r3 = est_d[:B].reshape(B, 1, T), ref_d.reshape(B, 1, T)
    for mine, theirs in ((BASE, losses.MelSpectrogramLoss()),
                         (utils.MEL_DISTANCE, losses.MelSpectrogramLoss(
                             n_mels=(150, 80), window_lengths=(2048, 512), pow=2.0,
                             mag_weight=1.0)),
                         (utils.STFT_DISTANCE, losses.MultiScaleSTFTLoss())):
        got = utils.spectral_distance(e3, r3, **mine)["distance"].mean().item()
        loss = float(theirs(e3, r3))
        print(f"batch mean {got:.9g} against losses.py {loss:.9g}")
        assert abs(got - loss) <= 1e-4 * max(1.0, abs(loss))


# ------------------------------------------------------------------ 6. graph capture
def test_graph_capture():
    R, B, T = 4, 2, 4099
    e0, r0 = make_rows(R, B, T)
    e1, r1 = make_rows(R, B, T, seed=1)
    lengths = t([T, 3001], np.int64)
    eager0, eager1 = raw(t(e0), t(r0), ALL, lengths), raw(t(e1), t(r1), ALL, lengths)
    se, sr = t(e0).clone(), t(r0).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        raw(se, sr, ALL, lengths)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = raw(se, sr, ALL, lengths)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    se.copy_(t(e1))
    sr.copy_(t(r1))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager1)


# ------------------------------------------------------------------ 7. through the model
LO, HI = 0.125, 6.0
_cache = {}


def golden_model(manifest):
    """The golden_nq8 model (its kwargs and weights) with a level range, and three clips of its
    audio recipe (44100 samples each)."""
    if not _cache:
        m = manifest["golden_nq8"]
        model = vrvq_amd.DAC_VRVQ(**m["kwargs"], level_min=LO, level_max=HI)
        load_recipe(model, m["weight_seed"])
        _cache["model"] = model.to(DEV).eval()
        _cache["audio"] = t(synthetic_audio(3, m["length"], seed=m["audio_seed"]))
    return _cache["model"], _cache["audio"]


def test_rd_sweep_spectral_columns(manifest):
    model, audio = golden_model(manifest)
    levels, B = [0.25, 1.0, 2.0], 3
    plain = utils.rd_sweep(model, audio, levels)
    assert set(plain) == {"si_sdr", "si_snr", "snr", "l1", "moments", "levels", "bpf", "kbps",
                          "recon", "summary"}
    assert all(set(row) == {"level", "level_scaled", "sisdr", "kbps"} for row in plain["summary"])
    again = utils.rd_sweep(model, audio, levels, spectral=None)
    assert set(again) == set(plain) and again["summary"] == plain["summary"]
    out = utils.rd_sweep(model, audio, levels, spectral=("mel", "stft"))
    assert set(out) == set(plain) | {"mel", "stft"}
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
    for k in plain:
        if k != "summary":
            assert torch.equal(out[k], plain[k]), k
    mel, st = utils.mel_distance(out["recon"], x), utils.stft_distance(out["recon"], x)
    assert out["mel"].shape == (3, B) and out["mel"].dtype == torch.float64
    assert torch.equal(out["mel"], mel) and torch.equal(out["stft"], st)
    assert torch.isfinite(mel).all() and (mel > 0).all() and (st > 0).all()
    for li, row in enumerate(out["summary"]):
        assert set(row) == {"level", "level_scaled", "sisdr", "kbps", "mel", "stft"}
        assert row["mel"] == mel[li].mean().item() and row["stft"] == st[li].mean().item()
        assert {k: row[k] for k in plain["summary"][li]} == plain["summary"][li]
    only = utils.rd_sweep(model, audio, levels, spectral="stft")
    assert set(only) == set(plain) | {"stft"} and torch.equal(only["stft"], st)
    # lengths reach the distances too
    n0 = audio.shape[-1] - 1000
    cut = utils.rd_sweep(model, audio, levels, lengths=[n0] * B, spectral=("mel",))
    assert torch.equal(cut["mel"], utils.mel_distance(cut["recon"], x, lengths=[n0] * B))
    assert not torch.equal(cut["mel"], mel)
    # against the restatement, one level
    T = x.shape[-1]
    want = S.distance_rows(out["recon"][:B].cpu().numpy().reshape(B, T),
                           x.cpu().numpy().reshape(B, T), **utils.MEL_DISTANCE)
    np.testing.assert_allclose(mel[0].cpu().numpy(), want["distance"], rtol=1e-4)
    utils.check_errors(DEV)


def test_solve_quality_on_the_mel_distance(manifest):
    model, audio = golden_model(manifest)
    B, nq, iters = 3, model.n_codebooks, 5
    ends = utils.rd_sweep(model, audio, [LO, HI], spectral=("mel",))
    d_lo, d_hi = ends["mel"][0].cpu().numpy(), ends["mel"][1].cpu().numpy()
    print("mel distance at level_min", d_lo, "at level_max", d_hi)
    targets = ((d_lo + d_hi) / 2).tolist()
    out = utils.solve_quality(model, audio, targets, metric="mel", iters=iters)
    assert set(out) == {"level", "value", "level_lo", "value_lo", "status", "bpf", "kbps",
                        "mask_imp", "z_q", "codes", "recon"}
    assert (out["level"].dtype, out["value"].dtype, out["status"].dtype) == \
        (torch.float32, torch.float64, torch.int32)
    status = out["status"].tolist()
    level, level_lo = out["level"].cpu().numpy(), out["level_lo"].cpu().numpy()
    value, value_lo = out["value"].cpu().numpy(), out["value_lo"].cpu().numpy()
    print("status", status, "level", level, "value", value, "level_lo", level_lo, "value_lo",
          value_lo)
    assert (value > 0).all() and (value_lo > 0).all()      # the distances, not their negation
    width = (HI / LO) ** (2.0 ** -iters) * (1 + 2.0 ** -20)
    assert 0 in status  # the flipped bracket contract below is exercised
    for b in range(B):
        if status[b] == 0:
            assert value[b] <= targets[b] < value_lo[b]
            assert np.float32(LO) <= level_lo[b] < level[b] <= np.float32(HI)
            assert float(level[b]) / float(level_lo[b]) <= width
        else:
            assert level[b] == level_lo[b] == np.float32(HI if status[b] == 1 else LO)
        if d_lo[b] - d_hi[b] > 1e-6:       # closer at level_max than at level_min: solvable
            assert status[b] == 0
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
        enc = model.encode(x, None, out["level"])
        assert torch.equal(enc["mask_imp"], out["mask_imp"])
        assert torch.equal(enc["codes"], out["codes"])
        assert torch.equal(utils.mel_distance(out["recon"], x).reshape(-1), out["value"])
    # out of reach on either side; the other distance
    never = utils.solve_quality(model, audio, 0.0, metric="mel", iters=2)
    assert never["status"].tolist() == [1] * B and never["level"].tolist() == [HI] * B
    assert never["level_lo"].tolist() == [HI] * B and (never["value"] > 0).all()
    always = utils.solve_quality(model, audio, torch.full((B,), 1e9), metric="stft", iters=2)
    assert always["status"].tolist() == [2] * B and always["level"].tolist() == [LO] * B
    with torch.no_grad():
        assert torch.equal(utils.stft_distance(always["recon"], x).reshape(-1), always["value"])
    utils.check_errors(DEV)
