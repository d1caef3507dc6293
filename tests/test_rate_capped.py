"""Capped rate control without a GPU: the properties of the NumPy restatement
(tests/rate_capped_ref.py, the yardstick of tests/test_gpu_rate_capped.py) on the very inputs the
GPU tests use, the operator and C-ABI surface, the argument conflicts of encode and compress, and
the .vrvq header fields with the per-packet rate read back from a stream."""
import ctypes
import json

import numpy as np
import pytest
import torch

import vrvq_amd
from rate_capped_ref import (HI, LO, SHAPES, case, packet_caps, packet_frames_of, packets_of,
                             solve_capped)
from test_rate import solve_level, total_bits
from vrvq_amd import _lib, codec, ops, utils
from vrvq_amd.codes_io import BITSTREAM_VERSION, VRVQFile, pack_bitstream


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("pooled", [False, True], ids=["clip", "pooled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_properties(shape, pooled):
    B, T, P, nq = shape
    (imp, bits, off, budgets, packet_budget), out = case(shape, pooled)
    level, total, status, p_level, p_total, p_status = out
    frames = packet_frames_of(T, P)
    cap, bad = packet_caps(imp, P, nq, bits, packet_budget, LO, HI)
    assert not bad.any()                                     # 0.7 of all codes: never infeasible
    for g in range(len(off) - 1):
        rows = slice(off[g], off[g + 1])
        lam = level[g]
        # the packets of the group add up to its total, within its budget
        assert int(p_total[rows].sum()) == int(total[g]) <= budgets[g]
        # every packet within its own budget, at min(lambda, cap)
        assert (p_total[rows] <= np.asarray(packet_budget)[None]).all()
        np.testing.assert_array_equal(p_level[rows], np.minimum(lam, cap[rows]))
        np.testing.assert_array_equal(p_status[rows], np.where(cap[rows] < lam, 2, 0))
        unc = solve_level(imp[rows], nq, bits, budgets[g], LO, HI)[0]
        assert lam >= unc                                    # the capped packets' bits move on
        if status[g] == 0:                                   # maximal: one step up is too much
            up = np.minimum(np.nextafter(lam, np.float32(np.inf)), cap[rows])
            over = sum(total_bits(imp[rows][b, p * P:(p + 1) * P], up[b, p], nq, bits)
                       for b in range(up.shape[0]) for p in range(len(frames)))
            assert over > budgets[g]
    # what the issue states of these inputs, so that no GPU comparison passes vacuously
    if shape == (1, 1, 1, 8):
        assert status.tolist() == [2] * len(status) and (p_status == 2).all()
    else:
        assert (status == 0).all()
        if pooled:
            unc = solve_level(imp, nq, bits, budgets[0], LO, HI)[0]
            assert level[0] > unc
            assert (p_status == 2).any() and (p_status == 0).any()


def test_restatement_infeasible_packets_and_loose_rows():
    shape = (3, 50, 16, 9)
    (imp, bits, off, budgets, packet_budget), ref = case(shape, True)
    B, T, P, nq = shape
    tail = packets_of(T, P) - 1
    pb = list(packet_budget)
    pb[tail] = packet_frames_of(T, P)[tail] * bits[0] - 1     # one bit short of one code a frame
    level, total, status, p_level, p_total, p_status = solve_capped(imp, P, nq, bits, off,
                                                                    budgets, pb)
    assert (p_status[:, tail] == 1).all() and (p_level[:, tail] == np.float32(LO)).all()
    assert (p_total[:, tail] > pb[tail]).all()
    assert (p_status[:, :tail] != 1).all() and (p_total[:, :tail] <= np.asarray(pb[:tail])).all()
    # rows of no valid group keep their caps; an empty and a bad group as in vrvq_rate_solve
    level, total, status, p_level, p_total, p_status = solve_capped(
        imp, P, nq, bits, [0, 1, 1, 4, 2], [budgets[0] // 3, 0, 10 ** 9, 10 ** 9], packet_budget)
    assert status.tolist() == [0, 2, -1, -1]
    cap, _ = packet_caps(imp, P, nq, bits, packet_budget, LO, HI)
    np.testing.assert_array_equal(p_level[1:], cap[1:])
    assert (p_status[1:] == 2).all()


# ------------------------------------------------------------------ operators and fakes
def test_capped_ops_registered_with_fake_kernels():
    lib = ops.load_ops()
    for name in ("rate_solve_capped", "scale_imp_packets"):
        assert getattr(lib, name).default._schema.name == f"vrvq::{name}"
    m = torch.device("meta")
    imp = torch.empty(5, 1, 87, device=m)
    bits = torch.empty(8, dtype=torch.int32, device=m)
    out = lib.rate_solve_capped(imp, bits, torch.empty(4, dtype=torch.int32, device=m),
                                torch.empty(3, dtype=torch.int64, device=m),
                                torch.empty(5, dtype=torch.int64, device=m), 20, 0.125, 6.0)
    assert [tuple(o.shape) for o in out] == [(3,)] * 3 + [(5, 5)] * 3
    assert [o.dtype for o in out] == [torch.float32, torch.int64, torch.int32] * 2
    s = lib.scale_imp_packets(imp, torch.empty(5, 5, device=m), 20)
    assert s.shape == imp.shape and s.dtype == torch.float32
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.scale_imp_packets(torch.ones(2, 4), torch.ones(2, 2), 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        utils.solve_levels_capped(torch.ones(2, 1, 4), 6.0, 8.0, 2, nq=8, sample_rate=44100,
                                  hop_length=512, level_min=LO, level_max=HI)
    with pytest.raises(ValueError, match="packet_frames"):
        utils.solve_levels_capped(torch.ones(2, 1, 4), 6.0, 8.0, 0, nq=8, sample_rate=44100,
                                  hop_length=512, level_min=LO, level_max=HI)


# ------------------------------------------------------------------ C-ABI argument checks
def test_capped_capi_argument_errors():
    lib = _lib.load()
    assert lib.vrvq_version() >= 111
    p = ctypes.c_void_p(16)  # non-null, never dereferenced: the checks return before a launch
    ERR = 10001

    def solve(imp=p, B=2, T=8, nq=8, bits=p, off=p, G=2, budget=p, pb=p, P=4, lo=0.125, hi=6.0,
              lv=p, tot=p, st=p, plv=p, ptot=p, pst=p):
        return lib.vrvq_rate_solve_capped(imp, B, T, nq, bits, off, G, budget, pb, P, lo, hi, lv,
                                          tot, st, plv, ptot, pst, None)

    for kw in (dict(imp=None), dict(bits=None), dict(off=None), dict(budget=None), dict(pb=None),
               dict(lv=None), dict(tot=None), dict(st=None), dict(plv=None), dict(ptot=None),
               dict(pst=None), dict(nq=0), dict(nq=33), dict(B=0), dict(T=0), dict(G=0),
               dict(P=0), dict(P=-1), dict(lo=2.0, hi=1.0), dict(lo=0.0), dict(lo=-1.0),
               dict(lo=float("nan")), dict(hi=float("nan")), dict(hi=float("inf"))):
        assert solve(**kw) == ERR, kw

    def scale(imp=p, B=2, T=8, plv=p, P=4, out=p):
        return lib.vrvq_scale_imp_packets(imp, B, T, plv, P, out, None)

    for kw in (dict(imp=None), dict(plv=None), dict(out=None), dict(B=0), dict(T=0), dict(P=0)):
        assert scale(**kw) == ERR, kw
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("vrvq_scale_imp_packets", None, 1, 1, None, 1, None, None)


# ------------------------------------------------------------------ argument conflicts
SMALL = dict(encoder_dim=8, decoder_dim=32, n_codebooks=2)


def test_capped_argument_conflicts_raise_before_any_kernel():
    """All on CPU models: a ValueError, not the kernels' "GPU only" RuntimeError, shows the check
    comes first."""
    x = torch.zeros(2, 1, 1024)
    vbr = vrvq_amd.DAC_VRVQ(level_min=0.5, level_max=2.0, **SMALL).eval()
    per_packet = torch.ones(2, 3)
    for call in (vbr.encode, lambda a, **kw: vbr(a, 44100, **kw)):
        with pytest.raises(ValueError, match="max_kbps needs target_kbps"):
            call(x, max_kbps=8.0, packet_frames=4)
        with pytest.raises(ValueError, match="max_kbps needs packet_frames"):
            call(x, target_kbps=6.0, max_kbps=8.0)
        for bad in (0, -3, 2.5):
            with pytest.raises(ValueError, match="packet_frames must be"):
                call(x, target_kbps=6.0, max_kbps=8.0, packet_frames=bad)
        with pytest.raises(ValueError, match="needs packet_frames"):
            call(x, level=per_packet)
        with pytest.raises(ValueError, match="packet_frames needs"):
            call(x, level=2.0, packet_frames=4)
        with pytest.raises(ValueError, match="packet_frames needs"):
            call(x, level=torch.ones(2), packet_frames=4)
        with pytest.raises(ValueError, match="not both"):
            call(x, level=per_packet, target_kbps=6.0, max_kbps=8.0, packet_frames=4)
        with pytest.raises(ValueError, match="n_quantizers"):
            call(x, n_quantizers=2, target_kbps=6.0, max_kbps=8.0, packet_frames=4)
        with pytest.raises(ValueError, match="n_quantizers"):
            call(x, n_quantizers=2, level=per_packet, packet_frames=4)
    # the quantizer knows the frame count: the wrong NP raises there before any kernel
    z = torch.zeros(2, vbr.latent_dim, 10)
    with pytest.raises(ValueError, match="NP = 3"):
        vbr.quantizer(z, None, z, torch.ones(2, 4), packet_frames=4)
    with pytest.raises(ValueError, match="NP = 1"):
        vbr.quantizer(z, None, z, per_packet, packet_frames=16)
    with pytest.raises(ValueError, match="max_kbps needs"):
        vbr.quantizer(z, None, z, None, max_kbps=8.0, packet_frames=4)
    vbr.train()
    with pytest.raises(ValueError, match="eval"):
        vbr.encode(x, target_kbps=6.0, max_kbps=8.0, packet_frames=4)
    with pytest.raises(ValueError, match="eval"):
        vbr.encode(x, level=per_packet, packet_frames=4)
    vbr.eval()
    cbr = vrvq_amd.DAC_VRVQ(model_type="CBR", **SMALL).eval()
    with pytest.raises(ValueError, match="VBR"):
        cbr.encode(x, target_kbps=6.0, max_kbps=8.0, packet_frames=4)
    with pytest.raises(ValueError, match="VBR"):
        cbr.encode(x, level=per_packet, packet_frames=4)
    sig = torch.zeros(1, 1, 4096)
    with pytest.raises(ValueError, match="VBR"):
        codec.compress(cbr, sig, target_kbps=6.0, max_kbps=8.0)
    with pytest.raises(ValueError, match="max_kbps needs target_kbps"):
        codec.compress(vbr, sig, max_kbps=8.0)
    with pytest.raises(ValueError, match="packet_frames"):
        codec.compress(vbr, sig, target_kbps=6.0, packet_frames=4)
    with pytest.raises(ValueError, match="packet_frames"):
        codec.compress(vbr, sig, target_kbps=6.0, max_kbps=8.0, packet_frames=0)
    # a valid capped call reaches the kernels, which refuse CPU tensors
    with pytest.raises(RuntimeError, match="GPU"):
        vbr.encode(x, target_kbps=6.0, max_kbps=8.0, packet_frames=4)


# ------------------------------------------------------------------ .vrvq header and packet_kbps
def hand_built(**fields):
    """2 rows x 2 chunks of 5 frames, nq = 3, 8-entry codebooks (3-bit codes, 2-bit counts)."""
    counts = np.array([[3, 0, 1, 2, 3, 0, 0, 0, 1, 1],
                       [1, 1, 1, 1, 1, 3, 3, 3, 3, 3]])
    mask = (np.arange(3)[None, :, None] < counts[:, None, :]).astype(np.float32)
    codes = (np.arange(60).reshape(2, 3, 10) % 8) * mask.astype(np.int64)
    bs = pack_bitstream(torch.from_numpy(codes), torch.from_numpy(mask), 8)
    return counts, VRVQFile(bitstream=bs, chunk_length=5, original_length=999,
                            input_db=torch.tensor([-20.0]), channels=2, sample_rate=44100,
                            padding=True, level=1.5, target_kbps=6.0, **fields)


def test_vrvq_header_round_trip_with_and_without_cap(tmp_path):
    _, plain = hand_built()
    # without the new fields: today's field set, nothing more, and the same bytes on disk
    assert list(plain._header()) == [
        "format", "version", "n_codebooks", "codebook_size", "frames", "count_bits", "code_bits",
        "row_words", "chunk_length", "original_length", "input_db", "channels", "sample_rate",
        "padding", "level", "target_kbps"]
    bs = plain.bitstream
    today = {"format": "VRVQ bitstream", "version": BITSTREAM_VERSION, "n_codebooks": 3,
             "codebook_size": 8, "frames": 10, "count_bits": 2, "code_bits": 3,
             "row_words": [int(v) for v in bs.row_words], "chunk_length": 5,
             "original_length": 999, "input_db": [-20.0], "channels": 2, "sample_rate": 44100,
             "padding": True, "level": 1.5, "target_kbps": 6.0}
    header = json.dumps(today).encode("utf-8")
    header += b" " * (-len(header) % 4)
    want = (b"VRVQBS%02d" % BITSTREAM_VERSION + np.array([len(header)], "<u4").tobytes() + header
            + bs.words.numpy().view(np.uint32).astype("<u4").tobytes())
    path = plain.save(tmp_path / "plain")
    assert path.read_bytes() == want
    back = VRVQFile.load(path)
    assert back.max_kbps is None and back.packet_frames is None and back.target_kbps == 6.0
    # with them: written, read back, and the stream is the same
    _, capped = hand_built(max_kbps=9.5, packet_frames=2)
    h = capped._header()
    assert (h["max_kbps"], h["packet_frames"]) == (9.5, 2)
    assert {k: v for k, v in h.items() if k not in ("max_kbps", "packet_frames")} == today
    back = VRVQFile.load(capped.save(tmp_path / "capped"))
    assert (back.max_kbps, back.packet_frames, back.level) == (9.5, 2, 1.5)
    assert torch.equal(back.bitstream.words, bs.words)
    # a header with a packet_frames that is no positive integer is refused
    blob = (tmp_path / "capped.vrvq").read_bytes()
    (tmp_path / "bad.vrvq").write_bytes(blob.replace(b'"packet_frames": 2', b'"packet_frames": 0'))
    with pytest.raises(RuntimeError, match="bad .vrvq header"):
        VRVQFile.load(tmp_path / "bad.vrvq")


def test_packet_kbps_on_a_hand_built_stream():
    counts, f = hand_built()
    rate = 44100 // 512                                      # 86 frames per second
    np.testing.assert_array_equal(f.frame_counts(), counts)
    # one packet per chunk of 5 frames: 3-bit codes + a 2-bit count per frame
    want = np.array([[(9 * 3 + 5 * 2), (2 * 3 + 5 * 2)],
                     [(5 * 3 + 5 * 2), (15 * 3 + 5 * 2)]]) / 5 * rate / 1000
    got = f.packet_kbps(44100, 512)
    assert got.shape == (2, 2) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)
    # packets of 2 frames restart at every chunk: 2, 2, 1 frames per chunk
    got = f.packet_kbps(44100, 512, packet_frames=2)
    bits = np.array([[3 * 3 + 4, 3 * 3 + 4, 3 * 3 + 2, 0 + 4, 1 * 3 + 4, 1 * 3 + 2],
                     [2 * 3 + 4, 2 * 3 + 4, 1 * 3 + 2, 6 * 3 + 4, 6 * 3 + 4, 3 * 3 + 2]])
    np.testing.assert_array_equal(got, bits / np.array([2, 2, 1, 2, 2, 1]) * rate / 1000)
    # the file's own packet_frames is the default, and P >= chunk_length is one packet per chunk
    _, g = hand_built(max_kbps=9.0, packet_frames=2)
    np.testing.assert_array_equal(g.packet_kbps(44100, 512), got)
    np.testing.assert_array_equal(g.packet_kbps(44100, 512, packet_frames=64), want)
    # pooled over packets with their frames as weights, the packets give the stream's own bits
    total = f.bitstream.code_bits_total + f.bitstream.count_bits_total
    assert round(float((got * np.array([2, 2, 1, 2, 2, 1])).sum() / rate * 1000)) == total
    with pytest.raises(ValueError, match="packet_frames"):
        f.packet_kbps(44100, 512, packet_frames=0)
    # a fixed-count stream has no count plane: every frame keeps all codes
    full = VRVQFile(bitstream=pack_bitstream(torch.zeros(1, 3, 10, dtype=torch.int64), None, 8),
                    chunk_length=5, original_length=1, input_db=torch.tensor([0.0]), channels=1,
                    sample_rate=44100, padding=True)
    np.testing.assert_array_equal(full.packet_kbps(44100, 512), np.full((1, 2), 9 * rate / 1000))
