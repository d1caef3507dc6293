"""Capped rate control on the GPU: vrvq_rate_solve_capped and vrvq_scale_imp_packets against the
NumPy restatement of tests/rate_capped_ref.py and against the uncapped solver, capped encodes
through the model (eager and under graph capture), and capped compress in both containers.
Totals are integers and levels fp32 bit patterns: every comparison is equality. Needs an MI355X."""
import numpy as np
import pytest
import torch

from rate_capped_ref import (HI, LO, SHAPES, bits_table, case, checkerboard, make_imp,
                             packet_frames_of, packet_totals, packets_of, solve_capped)
from test_gpu_rate import golden_model, planted
from test_rate import solve_level, total_bits
from vrvq_amd import codec, ops, utils
from vrvq_amd.codes_io import VRVQFile, count_bits_of
from vrvq_amd.recipe import synthetic_audio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("level", "total", "status", "packet_level", "packet_total", "packet_status")


def t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def run(imp, P, bits, off, budgets, packet_budget):
    out = ops.rate_solve_capped(t(imp), t(bits, np.int32), t(off, np.int32), t(budgets, np.int64),
                                t(packet_budget, np.int64), P, LO, HI)
    assert [o.dtype for o in out] == [torch.float32, torch.int64, torch.int32] * 2
    return [o.cpu().numpy() for o in out]


def assert_same(got, want):
    """All six outputs, levels by their bit patterns."""
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape, name
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), np.asarray(w, np.float32).view(np.uint32)
        np.testing.assert_array_equal(g, w, err_msg=name)


# ------------------------------------------------------------------ 1: kernel = restatement
@pytest.mark.parametrize("pooled", [False, True], ids=["clip", "pooled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_capped_solve_equals_restatement(shape, pooled):
    (imp, bits, off, budgets, packet_budget), want = case(shape, pooled)
    # what tests/test_rate_capped.py shows of these inputs: nothing here passes vacuously
    if shape == SHAPES[0]:
        assert want[2].tolist() == [2] and (want[5] == 2).all()
    else:
        assert (want[2] == 0).all()
        if pooled:
            assert (want[5] == 2).any() and (want[5] == 0).any()
            assert want[0][0] > solve_level(imp, shape[3], bits, budgets[0], LO, HI)[0]
    assert_same(run(imp, shape[2], bits, off, budgets, packet_budget), want)


def test_capped_solve_empty_bad_groups_and_loose_rows():
    B, T, P, nq = 5, 87, 20, 8
    imp, bits = make_imp(B, T, P), bits_table(nq, True)
    packet_budget = [int(0.7 * sum(bits) * n) for n in packet_frames_of(T, P)]

    def between(rows, frac):
        lo, hi = total_bits(rows, LO, nq, bits), total_bits(rows, HI, nq, bits)
        return lo + int((hi - lo) * frac)

    # rows 0-1 a group, an empty group, rows 2-3 a group, a range that is not monotone, and one
    # past the last row; row 4 is in no group and keeps its caps
    off = [0, 2, 2, 4, 3, 6]
    budgets = [between(imp[0:2], 0.5), 0, between(imp[2:4], 0.7), 10 ** 9, 10 ** 9]
    want = solve_capped(imp, P, nq, bits, off, budgets, packet_budget)
    assert want[2].tolist() == [0, 2, 0, -1, -1]
    got = run(imp, P, bits, off, budgets, packet_budget)
    assert_same(got, want)
    np.testing.assert_array_equal(got[5][4], np.full(packets_of(T, P), 2))
    assert_same(run(imp, P, bits, [-1, 2], [10 ** 9], packet_budget),
                solve_capped(imp, P, nq, bits, [-1, 2], [10 ** 9], packet_budget))
    # a group status 1: the group over its budget with every packet at LO
    want = solve_capped(imp, P, nq, bits, [0, B], [B * T - 1], packet_budget)
    assert want[2].tolist() == [1] and (want[3] == np.float32(LO)).all()
    assert_same(run(imp, P, bits, [0, B], [B * T - 1], packet_budget), want)


# ------------------------------------------------------------------ 2, 3: against rate_solve
@pytest.mark.parametrize("pooled", [False, True], ids=["clip", "pooled"])
@pytest.mark.parametrize("shape", [(3, 50, 16, 9), (2, 257, 64, 32), (1, 4097, 256, 8),
                                   (5, 1000, 87, 28)])
def test_loose_caps_equal_rate_solve(shape, pooled):
    """A packet budget of every code of every frame: the caps are HI and nothing changes."""
    B, T, P, nq = shape
    (imp, bits, off, budgets, _), _ = case(shape, pooled)
    loose = [sum(bits) * P] * packets_of(T, P)
    level, total, status, p_level, p_total, p_status = run(imp, P, bits, off, budgets, loose)
    lv, tot, st = ops.rate_solve(t(imp), t(bits, np.int32), t(off, np.int32),
                                 t(budgets, np.int64), LO, HI)
    np.testing.assert_array_equal(level.view(np.uint32), lv.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(total, tot.cpu().numpy())
    np.testing.assert_array_equal(status, st.cpu().numpy())
    assert (status == 0).all() and (p_status == 0).all()
    rows = np.repeat(level, np.diff(off))
    np.testing.assert_array_equal(p_level, np.repeat(rows[:, None], packets_of(T, P), 1))
    assert int(p_total.sum()) == int(total.sum())


@pytest.mark.parametrize("shape", [(3, 48, 16, 9), (4, 87, 87, 9), (1, 4096, 256, 8),
                                   (2, 1024, 512, 28)])
def test_huge_group_budget_gives_the_caps_of_rate_solve(shape):
    """With P | T the packets are the rows of imp.reshape(B * NP, P): the caps are what
    rate_solve gives for them, one group per row. (2, 1024, 512, 28): packets longer than the 256
    frames a wave holds in registers."""
    B, T, P, nq = shape
    imp, bits = make_imp(B, T, P), bits_table(nq, True)
    NP = T // P
    packet_budget = [int(0.7 * sum(bits) * P)] * NP
    level, total, status, p_level, p_total, p_status = run(imp, P, bits, [0, B], [10 ** 15],
                                                           packet_budget)
    lv, tot, st = ops.rate_solve(t(imp.reshape(B * NP, P)), t(bits, np.int32),
                                 t(np.arange(B * NP + 1), np.int32),
                                 t([packet_budget[0]] * (B * NP), np.int64), LO, HI)
    np.testing.assert_array_equal(p_level.view(np.uint32).reshape(-1),
                                  lv.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(p_total.reshape(-1), tot.cpu().numpy())
    assert status.tolist() == [2] and level[0] == np.float32(HI)
    st = st.cpu().numpy().reshape(B, NP)
    assert (st != 1).all() and (st == 0).any()               # some caps do bind
    np.testing.assert_array_equal(p_status, np.where(st == 0, 2, 0))


# ------------------------------------------------------------------ 4: planted values
@pytest.mark.parametrize("shape,pooled", [((3, 87, 20, 8), False), ((2, 257, 64, 32), True),
                                          ((5, 1000, 87, 28), True)])
def test_capped_solve_planted_values(shape, pooled):
    """NaN (0 bits), 0, 1, a denormal and both neighbours of the thresholds where a count steps
    (planted() of tests/test_gpu_rate.py), under the checkerboard gain (exact: 1 or 1/4)."""
    B, T, P, nq = shape
    imp, bits = planted(B, T, nq, nan=True) * checkerboard(B, T, P), bits_table(nq, False)
    assert np.isnan(imp).any() and (imp == 0).any()
    off = [0, B] if pooled else list(range(B + 1))
    clean = np.nan_to_num(imp, nan=-1.0)                     # a NaN costs nothing, as -1 does
    budgets = []
    for g in range(len(off) - 1):
        rows = clean[off[g]:off[g + 1]]
        lo, hi = total_bits(rows, LO, nq, bits), total_bits(rows, HI, nq, bits)
        budgets.append(lo + (hi - lo) * 6 // 10)
    packet_budget = [int(0.7 * sum(bits) * n) for n in packet_frames_of(T, P)]
    want = solve_capped(imp, P, nq, bits, off, budgets, packet_budget)
    assert (want[2] == 0).all() and (want[5] == 2).any()
    assert_same(run(imp, P, bits, off, budgets, packet_budget), want)


# ------------------------------------------------------------------ 5: infeasible packets
@pytest.mark.parametrize("shape", [(3, 50, 16, 9), (2, 257, 64, 32), (1, 4097, 256, 8)])
def test_infeasible_tail_packets(shape):
    B, T, P, nq = shape
    (imp, bits, off, budgets, packet_budget), ref = case(shape, True)
    tail = packets_of(T, P) - 1
    pb = list(packet_budget)
    pb[tail] = packet_frames_of(T, P)[tail] * bits[0] - 1     # one bit short of a code per frame
    want = solve_capped(imp, P, nq, bits, off, budgets, pb)
    got = run(imp, P, bits, off, budgets, pb)
    assert_same(got, want)
    level, total, status, p_level, p_total, p_status = got
    assert (p_status[:, tail] == 1).all() and (p_level[:, tail] == np.float32(LO)).all()
    assert (p_total[:, tail] > pb[tail]).all()
    assert (p_status[:, :tail] != 1).all()
    # the other packets keep their caps: whichever of them was capped before is capped at the
    # same level now
    was = ref[5][:, :tail] == 2
    assert was.any() and (p_status[:, :tail][was] == 2).all()
    np.testing.assert_array_equal(p_level[:, :tail][was], ref[3][:, :tail][was])


# ------------------------------------------------------------------ 6: scale_imp_packets
def test_scale_imp_packets():
    B, T, P = 5, 1000, 87
    imp = planted(B, T, 28, nan=True)
    NP = packets_of(T, P)
    lv = np.random.default_rng(3).uniform(0.05, 6.0, (B, NP)).astype(np.float32)
    lv[0, 0], lv[1, NP - 1] = 1e4, 1.0
    got = ops.scale_imp_packets(t(imp), t(lv), P).cpu().numpy()
    np.testing.assert_array_equal(got, imp * np.repeat(lv, P, axis=1)[:, :T])
    got3 = ops.scale_imp_packets(t(imp).reshape(B, 1, T), t(lv), P)
    assert got3.shape == (B, 1, T)
    np.testing.assert_array_equal(got3.cpu().numpy().reshape(B, T), got)
    one = ops.scale_imp_packets(t(imp), t(lv[:, :1]), 4096).cpu().numpy()    # P > T: rows
    np.testing.assert_array_equal(one, ops.scale_imp_rows(t(imp), t(lv[:, 0])).cpu().numpy())
    with pytest.raises(RuntimeError, match="packet_level"):
        ops.scale_imp_packets(t(imp), t(lv), P + 1000)


def test_solve_levels_capped_budgets():
    """The dict of utils.solve_levels_capped: budgets by kbps_to_budget over each packet's own
    frames (a pro-rata tail), less the side bits, per clip and pooled."""
    B, T, P, nq = 3, 87, 20, 8
    imp, bits = make_imp(B, T, P), [10] * nq
    kw = dict(nq=nq, sample_rate=44100, hop_length=512, level_min=LO, level_max=HI)
    for pooled, target, side in ((False, [3.0, 4.0, 5.0], 0), (True, 4.0, 4)):
        r = utils.solve_levels_capped(t(imp).reshape(B, 1, T), target, 4.5, P, pooled=pooled,
                                      side_bits_per_frame=side, **kw)
        off = [0, B] if pooled else list(range(B + 1))
        n = B * T if pooled else T
        ks = [target] if pooled else target
        budgets = [utils.kbps_to_budget(k, n, 44100, 512) - side * n for k in ks]
        pb = [utils.kbps_to_budget(4.5, f, 44100, 512) - side * f for f in packet_frames_of(T, P)]
        assert len(set(pb)) == 2
        want = solve_capped(imp, P, nq, bits, off, budgets, pb)
        assert (want[5] == 2).any() and (want[5] == 0).any()
        got = [r[k].cpu().numpy() for k in ("level", "bpf", "status", "packet_level",
                                            "packet_bits", "packet_status")]
        np.testing.assert_array_equal(got[1], (want[1] / n).astype(np.float32))
        got[1] = want[1]
        assert_same(got, want)


# ------------------------------------------------------------------ 7: through the model
def test_encode_max_kbps(manifest):
    from conftest import load_golden
    g = load_golden("golden_nq8")
    model = golden_model(manifest)
    nq, sr, hop = model.n_codebooks, model.sample_rate, model.hop_length
    rate, bits, P = sr // hop, [10] * nq, 20
    with torch.no_grad():
        x = model.preprocess(t(g["audio_in"]), 44100)
        plain = model.encode(x, None, 1)
    imp = plain["imp_map"][:, 0].cpu().numpy()
    B, T = imp.shape
    NP, frames = packets_of(T, P), np.array(packet_frames_of(T, P))
    # a target half way through the range every clip can reach, and a cap at the median rate of
    # the packets at the clips' uncapped levels: some packets are capped, some are not
    lo = max(total_bits(imp[b], LO, nq, bits) for b in range(B))
    hi = min(total_bits(imp[b], HI, nq, bits) for b in range(B))
    target = (lo + (hi - lo) * 0.5) / T * rate / 1000
    budget = utils.kbps_to_budget(target, T, sr, hop)
    unc = np.array([solve_level(imp[b], nq, bits, budget, LO, HI)[0] for b in range(B)])
    at_unc = packet_totals(imp, P, np.repeat(unc[:, None], NP, 1), nq, bits)
    max_kbps = float(np.median(at_unc / frames[None])) * rate / 1000
    pb = [utils.kbps_to_budget(max_kbps, int(n), sr, hop) for n in frames]
    want = solve_capped(imp, P, nq, bits, list(range(B + 1)), [budget] * B, pb)
    assert (want[2] == 0).all() and (want[5] == 2).any() and (want[5] == 0).any()

    def encode(audio, **kw):
        with torch.no_grad():
            return model.encode(model.preprocess(audio, 44100), **kw)

    kw = dict(target_kbps=target, max_kbps=max_kbps, packet_frames=P)
    out = encode(t(g["audio_in"]), **kw)
    assert set(out) == set(plain) | {"level", "bpf", "rate_status", "packet_level",
                                     "packet_bits", "packet_status"}
    assert torch.equal(out["imp_map"], plain["imp_map"])
    assert torch.equal(out["codes"], plain["codes"])
    assert torch.equal(out["latents"], plain["latents"])
    got = [out[k].cpu().numpy() for k in ("level", "bpf", "rate_status", "packet_level",
                                          "packet_bits", "packet_status")]
    np.testing.assert_array_equal(got[1], (want[1] / T).astype(np.float32))
    got[1] = want[1]
    assert_same(got, want)
    # the mask's own bits: every packet what the solver says and within the cap, every clip
    # within its budget
    kept = out["mask_imp"].sum(1).to(torch.int64).cpu().numpy() * 10          # (B, T)
    per_packet = np.add.reduceat(kept, np.arange(0, T, P), axis=1)
    np.testing.assert_array_equal(per_packet, got[4])
    assert (per_packet[got[5] != 1] <= np.repeat(np.array(pb)[None], B, 0)[got[5] != 1]).all()
    assert (per_packet.sum(1) <= budget).all()
    # packet p of every clip = the same frames of a per-clip encode at that packet's levels
    for p in range(NP):
        cols = slice(p * P, (p + 1) * P)
        one = encode(t(g["audio_in"]), level=out["packet_level"][:, p].contiguous())
        assert torch.equal(one["mask_imp"][..., cols], out["mask_imp"][..., cols]), p
        assert torch.equal(one["z_q"][..., cols], out["z_q"][..., cols]), p
    # the caller's own levels per packet give the same encode
    own = encode(t(g["audio_in"]), level=out["packet_level"].clone(), packet_frames=P)
    assert set(own) == set(plain)
    for k in ("mask_imp", "z_q", "codes", "latents"):
        assert torch.equal(own[k], out[k]), k
    full = model(t(g["audio_in"]), 44100, **kw)
    assert torch.equal(full["packet_level"], out["packet_level"])
    assert torch.equal(full["mask_imp"], out["mask_imp"])

    # the same call under graph capture: no host sync, replay equals eager
    keys = ("codes", "z_q", "mask_imp", "level", "bpf", "rate_status", "packet_level",
            "packet_bits", "packet_status")
    a1 = t(synthetic_audio(B, g["audio_in"].shape[-1], seed=2))
    eager0 = [out[k] for k in keys]
    eager1 = [encode(a1, **kw)[k] for k in keys]
    static = t(g["audio_in"]).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        encode(static, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = encode(static, **kw)
        outs = [o[k] for k in keys]
    graph.replay()
    torch.cuda.synchronize()
    for k, e, o in zip(keys, eager0, outs):
        assert torch.equal(e, o), k
    static.copy_(a1)
    graph.replay()
    torch.cuda.synchronize()
    for k, e, o in zip(keys, eager1, outs):
        assert torch.equal(e, o), k


# ------------------------------------------------------------------ 8: compress
def window_kbps(file, model):
    """Realised rate of every window, (items, windows): count fields + codes of a .vrvq file by
    packet_kbps, the kept codes of a .dac file from its markers."""
    rate = model.sample_rate // model.hop_length
    if isinstance(file, VRVQFile):
        return file.packet_kbps(model.sample_rate, model.hop_length, file.chunk_length)
    items, nq, frames = file.codes.shape
    kept = (file.codes < model.codebook_size).sum(1).numpy().reshape(items, -1, file.chunk_length)
    return kept.sum(2) * 10 / file.chunk_length * rate / 1000.0


@pytest.mark.parametrize("container", ["dac", "vrvq"])
def test_compress_max_kbps(manifest, container, tmp_path):
    model = golden_model(manifest)
    n = 3 * 44100 + 123
    # a loud second between quiet ones, so that the windows' rates differ
    audio = synthetic_audio(1, n, seed=7)
    audio[..., :44100] *= 0.05
    audio[..., 2 * 44100:] *= 0.2
    sig = torch.from_numpy(audio)
    target = 4.0
    kw = dict(win_duration=1.0, container=container)
    base = codec.compress(model, sig, target_kbps=target, **kw)
    per_window = window_kbps(base, model)
    assert per_window.shape[1] >= 3
    rate = model.sample_rate // model.hop_length
    peak, least = float(per_window.max()), float(per_window.min())
    assert peak > least
    max_kbps = (peak + least) / 2        # the cap binds the windows above it, not those below
    capped = codec.compress(model, sig, target_kbps=target, max_kbps=max_kbps, **kw)
    got = window_kbps(capped, model)
    assert got.shape == per_window.shape and (got <= max_kbps).all()
    # a window the cap does not bind runs at a level no lower than before: it loses no bits
    fit = per_window <= max_kbps
    assert fit.any() and not fit.all() and (got[fit] >= per_window[fit]).all()
    items, frames = got.shape[0], capped.chunk_length * got.shape[1]
    total = float((got * capped.chunk_length).sum()) / rate * 1000           # bits of the file
    assert round(total) <= utils.kbps_to_budget(target, items * frames, model.sample_rate,
                                                model.hop_length)
    if container == "vrvq":
        assert (capped.max_kbps, capped.packet_frames) == (max_kbps, capped.chunk_length)
        assert capped.level >= base.level
        assert capped.bitstream.count_bits == count_bits_of(model.n_codebooks)
        back = VRVQFile.load(capped.save(tmp_path / "capped"))
        assert (back.max_kbps, back.packet_frames) == (max_kbps, capped.chunk_length)
        np.testing.assert_array_equal(back.packet_kbps(model.sample_rate, model.hop_length), got)
    assert codec.decompress(model, capped).audio_data.shape[-1] == n
    # packets shorter than a window: every packet of 20 frames within the cap
    short = codec.compress(model, sig, target_kbps=target, max_kbps=max_kbps, packet_frames=20,
                           **kw)
    if container == "vrvq":
        assert short.packet_frames == 20
        assert (short.packet_kbps(model.sample_rate, model.hop_length) <= max_kbps).all()
    else:
        kept = (short.codes < model.codebook_size).sum(1).numpy()
        kept = kept.reshape(items, -1, short.chunk_length)
        starts = np.arange(0, short.chunk_length, 20)
        n_f = np.minimum(20, short.chunk_length - starts)
        kbps = np.add.reduceat(kept, starts, axis=2) * 10 / n_f * rate / 1000.0
        assert (kbps <= max_kbps).all()
    # a cap far above any window changes nothing: the same file, byte for byte
    loose = codec.compress(model, sig, target_kbps=target, max_kbps=1000.0, **kw)
    if container == "vrvq":
        assert torch.equal(loose.bitstream.words, base.bitstream.words)
        assert loose.bitstream.row_words == base.bitstream.row_words
        h = loose._header()
        assert (h.pop("max_kbps"), h.pop("packet_frames")) == (1000.0, base.chunk_length)
        assert h == base._header()                           # the two new fields apart
        assert loose.level == base.level
    else:
        assert torch.equal(loose.codes, base.codes)
        a, b = loose.save(tmp_path / "loose"), base.save(tmp_path / "base")
        assert a.read_bytes() == b.read_bytes()
    # a cap below the rate at level_min: no level helps
    with pytest.raises(ValueError, match="level_min"):
        codec.compress(model, sig, target_kbps=target, max_kbps=0.5, **kw)
    utils.check_errors(DEV)
