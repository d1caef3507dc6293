"""BSS-eval SDR on the GPU (vrvq_amd/csrc/sdr.hip), judged per row by the long-double yardstick
of tests/sdr_ref.py, never by the kernels' own other paths. Needs an MI355X.

The bar of a row (sdr_ref.bar_db): 16 x the deviation of the fp64 reference composition (FFT
correlations + LU, what torchmetrics runs) from the yardstick on that row, plus the dB change of
256 fp64 roundings in coh, (10 / ln 10) * 256 * 2^-53 / (1 - coh): the length of a chunked sum
tree plus the recursion's depth. Every case of the table has cond(R) <= 1e8 (asserted), and a
plain fp64 Levinson on the host passes the same bar on the whole table (asserted before the GPU
is asked)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sdr_ref
import vrvq_amd
from vrvq_amd import _lib, ops, utils
from vrvq_amd.recipe import load_recipe, synthetic_audio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = _lib.SDR_CHUNK


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def run(est, ref, lengths=None, **kw):
    """(R,) float64 as NumPy, from the op."""
    out = ops.bss_sdr(t(est), t(ref), None if lengths is None else t(lengths, np.int64), **kw)
    assert out.dtype == torch.float64 and out.shape == (est.shape[0],)
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host_checked(refs, what):
    """Before the GPU is asked: every row's cond(R) is within the table's limit, and the plain
    fp64 Levinson on the host passes the row's bar (if not, the table is wrong, not the bar).
    Returns refs."""
    for row, (yard, comp, lev) in enumerate(refs):
        assert comp["cond"] <= sdr_ref.COND_MAX, (what, row, comp["cond"])
        bar = sdr_ref.bar_db(abs(comp["sdr"] - yard["sdr"]), yard["one_minus_coh"])
        assert abs(lev["sdr"] - yard["sdr"]) <= bar, (what, row, "the table, not the kernel")
    return refs


def judge(got, refs, what):
    """Every row against the yardstick under its own bar; every figure printed first. Returns
    the largest ratio to the bar."""
    worst = 0.0
    for row, (yard, comp, _lev) in enumerate(refs):
        bar = sdr_ref.bar_db(abs(comp["sdr"] - yard["sdr"]), yard["one_minus_coh"])
        err = abs(got[row] - yard["sdr"])
        worst = max(worst, err / bar)
        print(f"{what} row {row}: sdr {yard['sdr']:.4f} dB, cond {comp['cond']:.2e}, "
              f"|err| {err:.2e}, bar {bar:.2e}, ratio {err / bar:.3f}")
    for row, (yard, comp, _lev) in enumerate(refs):
        bar = sdr_ref.bar_db(abs(comp["sdr"] - yard["sdr"]), yard["one_minus_coh"])
        assert abs(got[row] - yard["sdr"]) <= bar, (what, row, got[row], yard["sdr"], bar)
    return worst


# ------------------------------------------------------------------ 1. accuracy, per row
@pytest.mark.parametrize("case", range(len(sdr_ref.CASES)))
def test_accuracy_per_row(case):
    """Largest ratio to the bar measured on an MI355X over the table: see DESIGN.md section 4
    "BSS SDR"."""
    kind, n, F = sdr_ref.CASES[case]
    est, ref = sdr_ref.case_data(case)
    what = f"case {case} ({kind}, n {n}, F {F})"
    refs = host_checked(sdr_ref.case_refs(case), what)
    got = run(est, ref, filter_length=F)
    worst = judge(got, refs, what)
    print(f"case {case}: largest ratio to the bar {worst:.3f}")
    # the (R, 1, T) layout and the (L, B) result of utils.bss_sdr: the same bits
    out = utils.bss_sdr(t(est).reshape(6, 1, n), t(ref).reshape(2, 1, n), filter_length=F)
    assert out.shape == (3, 2) and out.dtype == torch.float64
    np.testing.assert_array_equal(bits(out.cpu().numpy().reshape(-1)), bits(got))


# ------------------------------------------------------------------ 2. sharing is invisible
def test_sharing_is_invisible():
    est, ref = sdr_ref.make_rows("ar1", 2 * C + 77, seed=11)
    full = run(est, ref)
    assert np.all(np.isfinite(full))
    np.testing.assert_array_equal(bits(run(est, ref)), bits(full))
    for r in range(6):
        b = r % 2
        alone = run(est[r:r + 1], ref[b:b + 1])
        np.testing.assert_array_equal(bits(alone), bits(full[r:r + 1]))
    for b in range(2):  # the L = 3 estimates of one reference, without the other reference
        three = run(est[b::2], ref[b:b + 1])
        np.testing.assert_array_equal(bits(three), bits(full[b::2]))
    # five estimates of one reference: a second wave of the solve, partly filled
    five = np.concatenate([est[0::2], est[4:5], est[0:1]])
    got = run(five, ref[0:1])
    np.testing.assert_array_equal(bits(got), bits(full[[0, 2, 4, 4, 0]]))
    # lengths against truncated copies; what lies past a length is never read
    lengths = np.array([C + 5, 700], np.int64)
    cut = run(est, ref, lengths)
    poisoned_e, poisoned_r = est.copy(), ref.copy()
    for r in range(6):
        poisoned_e[r, lengths[r % 2]:] = np.nan
    for b in range(2):
        poisoned_r[b, lengths[b]:] = np.nan
    np.testing.assert_array_equal(bits(run(poisoned_e, poisoned_r, lengths)), bits(cut))
    for b in range(2):
        n = int(lengths[b])
        trunc = run(est[b::2, :n], ref[b:b + 1, :n])
        np.testing.assert_array_equal(bits(trunc), bits(cut[b::2]))
    over = run(est, ref, np.array([C + 5, 10 ** 9], np.int64))  # clamped at the row's samples
    np.testing.assert_array_equal(bits(over[1::2]), bits(full[1::2]))


# ------------------------------------------------------------------ 3. special rows
def test_special_rows():
    est, ref = sdr_ref.make_rows("white", C + 1, seed=12)
    n = C + 1
    clean = run(est, ref)
    assert np.all(np.isfinite(clean))

    def same(got, rows):
        np.testing.assert_array_equal(bits(got[rows]), bits(clean[rows]))

    e = est.copy()
    e[3] = 0                                        # a silent estimate
    got = run(e, ref)
    assert np.isnan(got[3])
    same(got, [0, 1, 2, 4, 5])
    r = ref.copy()
    r[1] = 0                                        # a silent reference
    got = run(est, r)
    assert np.all(np.isnan(got[1::2]))
    same(got, [0, 2, 4])
    got = run(est, ref, np.array([0, n], np.int64))  # n = 0
    assert np.all(np.isnan(got[0::2]))
    same(got, [1, 3, 5])
    got = run(est, ref, np.array([-4, n], np.int64))
    assert np.all(np.isnan(got[0::2]))
    for pos in (0, C - 1, C):                       # a NaN sample stays in its row
        e = est.copy()
        e[4, pos] = np.nan
        got = run(e, ref)
        assert np.isnan(got[4]), pos
        same(got, [0, 1, 2, 3, 5])
    r = ref.copy()
    r[0, 100] = np.nan                              # in a reference: in the rows of that reference
    got = run(est, r)
    assert np.all(np.isnan(got[0::2]))
    same(got, [1, 3, 5])
    # est == ref: coh = 1 and no clamp; the call returns (one launch set, no retries)
    got = run(np.concatenate([ref, ref]), ref)
    print("est == ref:", got)
    assert all(math.isnan(v) or v == math.inf for v in got)
    # a singular R: load_diag = -r[0] leaves the first prediction error at 0
    got = run(est[:2], ref, filter_length=8, load_diag=-1.0)
    assert np.all(np.isnan(got))


# ------------------------------------------------------------------ 4. zero_mean and load_diag
def test_zero_mean_and_load_diag():
    n, F = C + 300, 64
    rng = np.random.default_rng(13)
    ref = (1.0 + 0.01 * rng.standard_normal((2, n))).astype(np.float32)
    est = np.empty((6, n), np.float32)
    for r in range(6):
        y = np.convolve(ref[r % 2].astype(np.float64) - 1.0, sdr_ref.FIR)[:n]
        noise = rng.standard_normal(n)
        noise *= math.sqrt(np.sum(y * y) / np.sum(noise * noise) / 10 ** (sdr_ref.NOISE_DB[r // 2] / 10))
        est[r] = (y + noise - 2.5).astype(np.float32)
    assert 90 < abs(ref.mean()) / ref.std() < 110
    for kw in (dict(zero_mean=True), dict(zero_mean=True, load_diag=1e-3), dict(load_diag=1e-3)):
        refs = host_checked([(sdr_ref.yardstick(est[r], ref[r % 2], F, **kw),
                              sdr_ref.composition(est[r], ref[r % 2], F, **kw),
                              sdr_ref.levinson64(est[r], ref[r % 2], F, **kw))
                             for r in range(6)], str(kw))
        got = run(est, ref, filter_length=F, **kw)
        judge(got, refs, str(kw))
    centred = run(est, ref, filter_length=F, zero_mean=True)
    assert np.all(centred[:2] > 5) and np.all(centred[4:] > 25)  # the rows are not degenerate
    # the default path is zero_mean=False, load_diag=None, bit for bit
    np.testing.assert_array_equal(bits(run(est, ref)),
                                  bits(run(est, ref, filter_length=512, zero_mean=False,
                                           load_diag=None)))
    lengths = np.array([n, C - 3], np.int64)         # the means are those of the counted samples
    got = run(est, ref, lengths, filter_length=F, zero_mean=True)
    for b in range(2):
        m = int(lengths[b])
        np.testing.assert_array_equal(
            bits(run(est[b::2, :m], ref[b:b + 1, :m], filter_length=F, zero_mean=True)),
            bits(got[b::2]))


# ------------------------------------------------------------------ 5. graph capture
@pytest.mark.parametrize("zero_mean", [False, True])
def test_graph_capture(zero_mean):
    n = C + 1
    e0, r0 = sdr_ref.make_rows("ar1", n, seed=14)
    e1, r1 = sdr_ref.make_rows("white", n, seed=15)
    lengths = t([n, C], np.int64)
    kw = dict(filter_length=512, zero_mean=zero_mean)
    eager0 = ops.bss_sdr(t(e0), t(r0), lengths, **kw)
    eager1 = ops.bss_sdr(t(e1), t(r1), lengths, **kw)
    se, sr = t(e0).clone(), t(r0).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.bss_sdr(se, sr, lengths, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.bss_sdr(se, sr, lengths, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager0, out)
    se.copy_(t(e1))
    sr.copy_(t(r1))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager1, out)


# ------------------------------------------------------------------ 6. through the model
LO, HI = 0.125, 6.0
_cache = {}


def golden_model(manifest):
    """The small model of tests/test_gpu_metrics.py: golden_nq8 with a level range, three clips."""
    if not _cache:
        m = manifest["golden_nq8"]
        model = vrvq_amd.DAC_VRVQ(**m["kwargs"], level_min=LO, level_max=HI)
        load_recipe(model, m["weight_seed"])
        _cache["model"] = model.to(DEV).eval()
        _cache["audio"] = t(synthetic_audio(3, m["length"], seed=m["audio_seed"]))
    return _cache["model"], _cache["audio"]


def test_rd_sweep_column(manifest):
    model, audio = golden_model(manifest)
    levels, B = [0.25, 1.0, 2.0], 3
    plain = utils.rd_sweep(model, audio, levels)
    out = utils.rd_sweep(model, audio, levels, bss_sdr=True)
    assert set(out) == set(plain) | {"bss_sdr"}
    for k in plain:
        if torch.is_tensor(plain[k]):
            assert torch.equal(plain[k], out[k]), k
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
    col = out["bss_sdr"]
    assert col.shape == (3, B) and col.dtype == torch.float64
    assert torch.equal(col, utils.bss_sdr(out["recon"], x))
    print("bss_sdr", col.cpu().numpy(), "si_sdr", out["si_sdr"].cpu().numpy())
    for li, (row, old) in enumerate(zip(out["summary"], plain["summary"])):
        assert set(row) == set(old) | {"bss_sdr"}
        assert all(row[k] == old[k] for k in old)
        assert row["bss_sdr"] == col[li].mean().item()
    # the projection only adds to the explained energy: not below the eps-free SI-SDR
    assert torch.all(col >= out["si_sdr"] - 1e-6)
    n0 = audio.shape[-1]
    lengths = [n0, n0 - 1000, 5000]
    cut = utils.rd_sweep(model, audio, levels, lengths=lengths, bss_sdr=True, spectral="stft")
    assert torch.equal(cut["bss_sdr"], utils.bss_sdr(cut["recon"], x, lengths))
    assert all(set(row) == set(plain["summary"][0]) | {"bss_sdr", "stft"}
               for row in cut["summary"])


def test_solve_quality_on_bss_sdr(manifest):
    model, audio = golden_model(manifest)
    B, iters = 3, 5
    ends = utils.rd_sweep(model, audio, [LO, HI], bss_sdr=True)
    v_lo, v_hi = ends["bss_sdr"][0].cpu().numpy(), ends["bss_sdr"][1].cpu().numpy()
    print("bss_sdr at level_min", v_lo, "at level_max", v_hi)
    targets = ((v_lo + v_hi) / 2).tolist()
    out = utils.solve_quality(model, audio, targets, metric="bss_sdr", iters=iters)
    status = out["status"].tolist()
    level, level_lo = out["level"].cpu().numpy(), out["level_lo"].cpu().numpy()
    value, value_lo = out["value"].cpu().numpy(), out["value_lo"].cpu().numpy()
    print("status", status, "level", level, "value", value, "level_lo", level_lo, "value_lo",
          value_lo)
    assert out["value"].dtype == torch.float64
    width = (HI / LO) ** (2.0 ** -iters) * (1 + 2.0 ** -20)
    for b in range(B):  # the bracket contract: a returned level reaches the target, or status 1
        assert status[b] in (0, 1, 2)
        if status[b] == 0:
            assert value[b] >= targets[b] and not value_lo[b] >= targets[b]
            assert np.float32(LO) <= level_lo[b] < level[b] <= np.float32(HI)
            assert float(level[b]) / float(level_lo[b]) <= width
        elif status[b] == 1:
            assert level[b] == level_lo[b] == np.float32(HI) and not value[b] >= targets[b]
        else:
            assert level[b] == level_lo[b] == np.float32(LO) and value[b] >= targets[b]
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
    assert torch.equal(out["value"], utils.bss_sdr(out["recon"], x).reshape(-1))
    high = utils.solve_quality(model, audio, 1e9, iters=1, metric="bss_sdr")
    assert high["status"].tolist() == [1] * B and high["level"].tolist() == [HI] * B
    low = utils.solve_quality(model, audio, -1e9, iters=1, metric="bss_sdr")
    assert low["status"].tolist() == [2] * B and low["level"].tolist() == [LO] * B
    utils.check_errors(DEV)


# ------------------------------------------------------------------ 7. the C-ABI
def test_capi_writes_only_what_it_states():
    lib = _lib.load()
    R, B, n, F, GUARD = 6, 2, C + 9, 64, 512
    est, ref = sdr_ref.make_rows("lowpass", n, seed=16)
    want = run(est, ref, filter_length=F)
    need = ctypes.c_longlong(0)
    assert lib.vrvq_bss_sdr_workspace(R, B, n, F, ctypes.byref(need)) == 0
    words = need.value // 8
    assert need.value == 8 * (R + B) * (1 + 2 * (F + 2) + F)
    e, r = t(est), t(ref)
    out = torch.full((GUARD + R + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.full((GUARD + words + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    out_p, ws_p = out.data_ptr() + 8 * GUARD, ws.data_ptr() + 8 * GUARD
    torch.cuda.synchronize()

    def call(ws_bytes):
        return lib.vrvq_bss_sdr(ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(r.data_ptr()), R, B,
                                n, None, F, 0, float("nan"), ctypes.c_void_p(out_p),
                                ctypes.c_void_p(ws_p), ws_bytes, None)

    assert call(need.value - 8) == 10001   # a workspace too small: refused before any launch
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()
    assert call(need.value) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(bits(got[GUARD:GUARD + R]), bits(want))
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + R:]).all()
    guard = ws.cpu().numpy()
    assert np.isnan(guard[:GUARD]).all() and np.isnan(guard[GUARD + words:]).all()
