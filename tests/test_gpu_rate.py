"""Rate control on the GPU: the rate kernels against the NumPy restatement of tests/test_rate.py
and against the existing mask kernels, per-clip levels and target_kbps through the model, and
target-bitrate compress. Totals are integers and levels fp32 bit patterns: every comparison is
equality. Needs an MI355X."""
import numpy as np
import pytest
import torch

import vrvq_amd
from conftest import load_golden
from test_rate import frame_counts, solve_level, total_bits
from vrvq_amd import codec, ops, utils
from vrvq_amd.recipe import load_recipe, synthetic_audio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (B, T, nq). One workgroup serves a row (curve) or a group (solve); the solver holds a group of
# up to 4096 elements in registers and re-reads a larger one, so 5000 frames in one row, and the
# five 1000-frame rows pooled, take the second path, and 4096 / 4097 sit on the bound.
SHAPES = [(1, 1, 8), (3, 87, 8), (2, 257, 32), (5, 1000, 28), (1, 5000, 8)]
BOUND_SHAPES = [(1, 4096, 8), (1, 4097, 8)]
LEVELS = [0.05, 0.125, 1.0, 3.7, 6.0, 1e4]
LO, HI = 0.125, 6.0


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def bits_table(nq, uniform):
    return [10] * nq if uniform else [10 - (i // 2) % 3 for i in range(nq)]  # 10,10,9,9,8,8,10,..


def planted(B, T, nq, nan):
    """Uniform (0, 1) with planted edge values: 0, 1, the smallest denormal, NaN, and both
    neighbours of thresholds k / (nq * level), where the count steps."""
    rng = np.random.default_rng(1000 * B + T + nq)
    imp = rng.random((B, T), dtype=np.float32)
    imp[imp == 0] = 0.5
    plants = [0.0, 1.0, float(np.float32(1e-45))] + ([float("nan")] if nan else [])
    for level in LEVELS:
        for k in (1, 2, nq - 1, nq // 2):
            x = np.float32(k / (nq * level))
            if 0 < x < 1:
                plants += [float(np.nextafter(x, np.float32(0))), float(x),
                           float(np.nextafter(x, np.float32(1)))]
    flat = imp.reshape(-1)
    n = min(len(plants), flat.size // 2)
    pos = rng.choice(flat.size, size=n, replace=False)
    flat[pos] = np.asarray(plants[:n], np.float32)
    return imp


def mask_total(imp_rows, level, nq, bits):
    """Bits of imp_rows (R, T) at a level from the existing kernels: scale_imp -> imp_mask, then
    bits . mask summed (integers)."""
    R, T = imp_rows.shape
    s = ops.scale_imp(imp_rows.contiguous(), float(level), float(nq))
    mask = ops.mask_hard(s.reshape(R, 1, T), nq)
    return (mask.sum(2).to(torch.int64) * t(bits, np.int64)).sum(1)


# ------------------------------------------------------------------ rate_curve
@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_rate_curve_equals_restatement(shape, uniform):
    B, T, nq = shape
    imp, bits = planted(B, T, nq, nan=True), bits_table(nq, uniform)
    got = ops.rate_curve(t(imp), t(LEVELS, np.float32), t(bits, np.int32)).cpu().numpy()
    want = np.array([[total_bits(imp[b], lv, nq, bits) for lv in LEVELS] for b in range(B)])
    assert got.dtype == np.int64 and got.shape == (B, len(LEVELS))
    np.testing.assert_array_equal(got, want)
    bpf = utils.rate_curve(t(imp).reshape(B, 1, T), LEVELS, nq, bits)
    assert bpf.dtype == torch.float32
    np.testing.assert_array_equal(bpf.cpu().numpy(), (want / T).astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES)
def test_rate_curve_agrees_with_mask_kernels(shape):
    B, T, nq = shape
    imp, bits = t(planted(B, T, nq, nan=True)), bits_table(nq, False)
    got = ops.rate_curve(imp, t(LEVELS, np.float32), t(bits, np.int32))
    for li, level in enumerate(LEVELS):
        assert torch.equal(got[:, li], mask_total(imp, level, nq, bits)), level


def test_scale_imp_rows():
    imp = planted(5, 1000, 28, nan=True)
    lv = np.asarray([0.3, 1.0, 2.5, 1e4, 0.05], np.float32)
    got = ops.scale_imp_rows(t(imp), t(lv)).cpu().numpy()
    np.testing.assert_array_equal(got, imp * lv[:, None])
    got3 = ops.scale_imp_rows(t(imp).reshape(5, 1, 1000), t(lv))
    assert got3.shape == (5, 1, 1000)
    np.testing.assert_array_equal(got3.cpu().numpy().reshape(5, 1000), got)


# ------------------------------------------------------------------ rate_solve
def between(imp_rows, nq, bits, frac):
    """A budget strictly between the totals at LO and HI."""
    t_lo, t_hi = total_bits(imp_rows, LO, nq, bits), total_bits(imp_rows, HI, nq, bits)
    budget = t_lo + int((t_hi - t_lo) * frac)
    assert t_lo < budget < t_hi, (t_lo, budget, t_hi)
    return budget


def check_solve(imp, nq, bits, off, budgets, want_status):
    """Run rate_solve and compare every valid group with the restatement; for a solved group
    the next level up must exceed the budget by the existing mask kernels."""
    imp_d = t(imp)
    level, total, status = ops.rate_solve(imp_d, t(bits, np.int32), t(off, np.int32),
                                          t(budgets, np.int64), LO, HI)
    assert (level.dtype, total.dtype, status.dtype) == (torch.float32, torch.int64, torch.int32)
    level, total, status = level.cpu().numpy(), total.cpu().numpy(), status.cpu().numpy()
    assert status.tolist() == want_status
    for g, st in enumerate(want_status):
        r0, r1 = off[g], off[g + 1]
        if st == -1:
            continue
        if r0 == r1:
            assert (level[g], total[g]) == (np.float32(HI), 0)
            continue
        lv, tot, st_ref = solve_level(imp[r0:r1], nq, bits, budgets[g], LO, HI)
        assert st_ref == st
        assert level[g].view(np.uint32) == lv.view(np.uint32), (g, level[g], lv)
        assert int(total[g]) == tot == total_bits(imp[r0:r1], level[g], nq, bits)
        if st == 0:
            assert tot <= budgets[g]
            up = np.nextafter(level[g], np.float32(np.inf))
            assert int(mask_total(imp_d[r0:r1], up, nq, bits).sum()) > budgets[g]
        elif st == 1:
            assert level[g] == np.float32(LO) and tot > budgets[g]
        else:
            assert level[g] == np.float32(HI) and tot <= budgets[g]


@pytest.mark.parametrize("shape", SHAPES)
def test_rate_solve_per_clip(shape):
    B, T, nq = shape
    imp, bits = planted(B, T, nq, nan=False), bits_table(nq, B != 3)
    budgets, want = [], []
    for b in range(B):
        if B >= 3 and b == 1:    # fewer bits than frames: infeasible
            budgets.append(T - 1), want.append(1)
        elif B >= 3 and b == 2:  # every code of every frame fits: saturated
            budgets.append(nq * T * 10), want.append(2)
        else:
            budgets.append(between(imp[b], nq, bits, 0.2 + 0.15 * b)), want.append(0)
    check_solve(imp, nq, bits, list(range(B + 1)), budgets, want)


@pytest.mark.parametrize("shape", SHAPES + BOUND_SHAPES)
def test_rate_solve_pooled(shape):
    B, T, nq = shape
    imp, bits = planted(B, T, nq, nan=False), bits_table(nq, True)
    check_solve(imp, nq, bits, [0, B], [between(imp, nq, bits, 0.4)], [0])


def test_rate_solve_uneven_groups():
    B, T, nq = 5, 1000, 28
    imp, bits = planted(B, T, nq, nan=False), bits_table(nq, False)
    off = [0, 1, 4, 5]
    budgets = [T - 1, between(imp[1:4], nq, bits, 0.6), nq * T * 10]
    check_solve(imp, nq, bits, off, budgets, [1, 0, 2])


def test_rate_solve_empty_and_bad_groups():
    B, T, nq = 5, 87, 8
    imp, bits = planted(B, T, nq, nan=False), bits_table(nq, True)
    off = [0, 2, 2, 5, 3, 5]   # [2, 2) is empty; [5, 3) is not monotone
    budgets = [between(imp[0:2], nq, bits, 0.5), 0, between(imp[2:5], nq, bits, 0.3), 10 ** 9,
               between(imp[3:5], nq, bits, 0.7)]
    check_solve(imp, nq, bits, off, budgets, [0, 2, 0, -1, 0])
    check_solve(imp, nq, bits, [0, 6], [10 ** 9], [-1])     # past the last row
    check_solve(imp, nq, bits, [-1, 2], [10 ** 9], [-1])


def test_solve_levels_pooled_and_per_clip():
    B, T, nq = 3, 87, 8
    imp = planted(B, T, nq, nan=False)
    kw = dict(nq=nq, sample_rate=44100, hop_length=512, level_min=LO, level_max=HI)
    lv, bpf, st = utils.solve_levels(t(imp).reshape(B, 1, T), [3.0, 4.0, 5.0], **kw)
    for b, k in enumerate([3.0, 4.0, 5.0]):
        ref = solve_level(imp[b], nq, [10] * nq, utils.kbps_to_budget(k, T, 44100, 512), LO, HI)
        assert (lv[b].item(), st[b].item()) == (float(ref[0]), ref[2])
        assert bpf[b].item() == float(np.float32(ref[1] / T))
    lv, bpf, st = utils.solve_levels(t(imp), 4.0, pooled=True, **kw)
    ref = solve_level(imp, nq, [10] * nq, utils.kbps_to_budget(4.0, B * T, 44100, 512), LO, HI)
    assert lv.shape == (1,) and (lv.item(), st.item()) == (float(ref[0]), ref[2])
    assert bpf.item() == float(np.float32(ref[1] / (B * T)))


# ------------------------------------------------------------------ through the model
_model = []


def golden_model(manifest):
    """The golden_nq8 model (its kwargs and weights) with a level range for target_kbps."""
    if not _model:
        m = manifest["golden_nq8"]
        model = vrvq_amd.DAC_VRVQ(**m["kwargs"], level_min=LO, level_max=HI)
        load_recipe(model, m["weight_seed"])
        _model.append(model.to(DEV).eval())
    return _model[0]


def test_per_clip_levels_equal_scalar_encodes(manifest):
    """Three clips of the golden_nq8 audio recipe (the fixture itself holds its first two)."""
    m = manifest["golden_nq8"]
    model = golden_model(manifest)
    audio = synthetic_audio(3, m["length"], seed=m["audio_seed"])
    np.testing.assert_array_equal(audio[:2], load_golden("golden_nq8")["audio_in"])
    levels = torch.tensor([0.3, 1.0, 2.5], device=DEV)
    keys = {"z_q", "z_q_is", "codes", "latents", "commitment_loss", "codebook_loss", "imp_map",
            "mask_imp"}
    with torch.no_grad():
        x = model.preprocess(t(audio), 44100)
        per = model.encode(x, None, levels)
        assert set(per) == keys
        for i in range(3):
            one = model.encode(x, None, float(levels[i]))
            assert set(one) == keys
            assert torch.equal(per["imp_map"], one["imp_map"])
            for k in ("mask_imp", "z_q", "codes", "latents"):
                assert torch.equal(per[k][i], one[k][i]), (i, k)
        full = model(t(audio), 44100, None, levels)
        assert torch.equal(full["mask_imp"], per["mask_imp"]) and "level" not in full
    assert len({int(per["mask_imp"][i].sum()) for i in range(3)}) == 3  # the levels do differ


def clip_bits(mask_row, nq, T):
    return round(utils.cal_bpf_from_mask(mask_row[None].contiguous(), [10] * nq) * T)


def test_encode_target_kbps(manifest):
    g = load_golden("golden_nq8")
    model = golden_model(manifest)
    nq, sr, hop = model.n_codebooks, model.sample_rate, model.hop_length
    # two targets from the reference's imp_map, a third and two thirds of the way through the
    # range every clip can reach: status 0 for all
    ref = g["imp_map"][:, 0]
    B, T = ref.shape
    lo = max(total_bits(ref[b], LO, nq, [10] * nq) for b in range(B))
    hi = min(total_bits(ref[b], HI, nq, [10] * nq) for b in range(B))
    k1, k2 = ((lo + (hi - lo) * f) / T * (sr // hop) / 1000 for f in (1 / 3, 2 / 3))
    kw = dict(nq=nq, sample_rate=sr, hop_length=hop, level_min=LO, level_max=HI)
    with torch.no_grad():
        x = model.preprocess(t(g["audio_in"]), 44100)
        plain = model.encode(x, None, 1)
        for target in (k1, [k1, k2]):
            out = model.encode(x, target_kbps=target)
            assert set(out) == set(plain) | {"level", "bpf", "rate_status"}
            assert torch.equal(out["imp_map"], plain["imp_map"])
            assert torch.equal(out["codes"], plain["codes"])
            lv, bpf, st = utils.solve_levels(out["imp_map"], target, **kw)
            assert torch.equal(out["level"], lv) and torch.equal(out["bpf"], bpf)
            assert out["rate_status"].tolist() == [0] * B == st.tolist()
            ks = target if isinstance(target, list) else [target] * B
            for b in range(B):
                bits = clip_bits(out["mask_imp"][b], nq, T)
                assert bits <= utils.kbps_to_budget(ks[b], T, sr, hop)
                assert bits == round(out["bpf"][b].item() * T)
                one = model.encode(x, None, out["level"][b].item())
                assert torch.equal(one["mask_imp"][b], out["mask_imp"][b])
                assert torch.equal(one["z_q"][b], out["z_q"][b])
        full = model(t(g["audio_in"]), 44100, target_kbps=k1)
        assert torch.equal(full["level"], model.encode(x, target_kbps=k1)["level"])

    # the same call under graph capture: no host sync, replay equals eager
    a1 = t(synthetic_audio(B, g["audio_in"].shape[-1], seed=2))

    def run(audio):
        with torch.no_grad():
            o = model.encode(model.preprocess(audio, 44100), target_kbps=[k1, k2])
        return [o[k] for k in ("codes", "z_q", "mask_imp", "level", "bpf", "rate_status")]

    eager0, eager1 = run(t(g["audio_in"])), run(a1)
    static = t(g["audio_in"]).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager0, outs):
        assert torch.equal(e, o)
    static.copy_(a1)
    graph.replay()
    torch.cuda.synchronize()
    for e, o in zip(eager1, outs):
        assert torch.equal(e, o)


def test_compress_target_kbps(manifest):
    model = golden_model(manifest)
    n = 3 * 44100 + 123
    sig = torch.from_numpy(synthetic_audio(1, n, seed=7))
    target = 4.0
    dac = codec.compress(model, sig, win_duration=1.0, target_kbps=target)
    items, nq, frames = dac.codes.shape
    assert frames // dac.chunk_length >= 3  # several windows in the one group
    kept = int((dac.codes < model.codebook_size).sum())
    assert 0 < kept * 10 <= utils.kbps_to_budget(target, items * frames, model.sample_rate,
                                                 model.hop_length)
    level = codec.solve_file_level(model, sig, target, win_duration=1.0)
    assert isinstance(level, float) and LO <= level <= HI
    same = codec.compress(model, sig, win_duration=1.0, level=level)
    assert torch.equal(dac.codes, same.codes)
    assert dac.chunk_length == same.chunk_length
    assert codec.decompress(model, dac).audio_data.shape[-1] == n
    utils.check_errors(DEV)
