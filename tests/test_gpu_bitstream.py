"""VRVQ bitstream 1 on the GPU: the HIP bit packer against the reference packer
(tests/bitstream_ref.py) word for word, its bounds-checked rejections, the `.vrvq` container
through compress / decompress, the side information in the target_kbps budget, and the C-ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bitstream_ref as ref
import vrvq_amd
from oracle.vrvq_oracle import generate_mask_hard
from test_codec import KW, SR, _signal
from vrvq_amd import _lib, codec, utils
from vrvq_amd.codes_io import (BITSTREAM_CHUNK_FRAMES, Bitstream, DACFile, VRVQFile,
                               pack_bitstream, unpack_bitstream)
from vrvq_amd.recipe import load_recipe

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = BITSTREAM_CHUNK_FRAMES

# (R, Nq, codebook_size, T)
CASES = [(1, 9, 1024, 1), (3, 9, 1024, C - 1), (3, 9, 1024, C), (3, 9, 1024, C + 1),
         (2, 8, 1024, 2 * C + 3), (2, 32, 1024, 70), (2, 5, 2, 131), (2, 4, 65536, 67),
         (2, 7, 1000, 97), (300, 3, 16, 5)]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_case(R, nq, size, T, seed=0, extremes=True):
    """Random codes, masks as tests/test_gpu_parity.py draws them for pack_codes (hard masks of
    random scores: counts cover 0 .. Nq), the first row all counts 0 and the last all Nq."""
    g = np.random.default_rng(seed)
    codes = g.integers(0, size, (R, nq, T)).astype(np.int64)
    mask = generate_mask_hard(g.uniform(-0.5, nq + 0.5, (R, 1, T)).astype(np.float32), nq)
    mask = mask.astype(np.float32)
    if extremes and R > 1:
        mask[0] = 0
        mask[-1] = 1
    return codes, mask


_refs = {}


def reference(case):
    if case not in _refs:
        codes, mask = make_case(*case, seed=case[3])
        _refs[case] = (codes, mask) + ref.pack(codes, mask, case[2])
    return _refs[case]


def u32(words: torch.Tensor) -> np.ndarray:
    return words.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_words_equal_reference_and_round_trip(case):
    R, nq, size, T = case
    codes, mask, words, row_words, info = reference(case)
    bs = pack_bitstream(t(codes), t(mask), size)
    assert bs.words.is_cuda and bs.words.dtype == torch.int32
    assert list(bs.row_words) == row_words
    np.testing.assert_array_equal(u32(bs.words), words)
    assert (bs.n_codebooks, bs.codebook_size, bs.frames) == (nq, size, T)
    assert (bs.count_bits, bs.code_bits) == (info["count_bits"], info["code_bits"])
    assert (bs.code_bits_total, bs.count_bits_total, bs.padding_bits) == (
        info["code_bits_total"], info["count_bits_total"], info["padding_bits"])
    c2, m2 = unpack_bitstream(bs)
    assert c2.dtype == torch.int64 and m2.dtype == torch.float32
    np.testing.assert_array_equal(m2.cpu().numpy(), mask)
    np.testing.assert_array_equal(c2.cpu().numpy(), codes * (mask != 0))
    # the reference's own words unpack to the same on the device
    c3, m3 = unpack_bitstream(Bitstream(**dict(bs.__dict__, words=t(words.view(np.int32)))))
    assert torch.equal(c3, c2) and torch.equal(m3, m2)


@pytest.mark.parametrize("case", [(1, 9, 1024, 1), (3, 9, 1024, C + 1), (2, 7, 1000, 97)],
                         ids=lambda c: "x".join(map(str, c)))
def test_fixed_count_stream(case):
    R, nq, size, T = case
    codes = reference(case)[0]
    words, row_words, info = ref.pack(codes, None, size)
    bs = pack_bitstream(t(codes), None, size)
    assert bs.count_bits == 0 and bs.count_bits_total == 0
    assert list(bs.row_words) == row_words == [-(-ref.code_bits(size) * nq * T // 32)] * R
    np.testing.assert_array_equal(u32(bs.words), words)
    c2, m2 = unpack_bitstream(bs)
    np.testing.assert_array_equal(c2.cpu().numpy(), codes)
    assert bool((m2 == 1).all())


def test_rows_do_not_depend_on_the_batch():
    case = (2, 8, 1024, 2 * C + 3)
    codes, mask = make_case(*case, seed=11, extremes=False)   # both rows with mixed counts
    words, row_words, _ = ref.pack(codes, mask, 1024)
    bs = pack_bitstream(t(codes), t(mask), 1024)
    np.testing.assert_array_equal(u32(bs.words), words)
    off = 0
    for r in range(2):
        alone = pack_bitstream(t(codes[r:r + 1]), t(mask[r:r + 1]), 1024)
        assert alone.row_words == (row_words[r],)
        np.testing.assert_array_equal(u32(alone.words), words[off:off + row_words[r]])
        off += row_words[r]
    again = pack_bitstream(t(codes), t(mask), 1024)            # a pure function of the input
    assert torch.equal(again.words, bs.words)


# ------------------------------------------------------------------------------ rejections
def _put(words: np.ndarray, bit: int, width: int, value: int):
    """Overwrite the `width`-bit field at stream bit `bit` of a uint32 array."""
    for j in range(width):
        q = bit + j
        words[q >> 5] = (int(words[q >> 5]) & ~(1 << (q & 31))) | (((value >> j) & 1) << (q & 31))


def test_pack_rejects_bad_input():
    codes, mask = make_case(2, 9, 1024, C + 1, seed=5, extremes=False)
    bad = mask.copy()
    bad[1, :, C] = 0
    bad[1, 4, C] = 1                                          # a 1 after a 0 along Nq
    with pytest.raises(ValueError, match="prefix"):
        pack_bitstream(t(codes), t(bad), 1024)
    big = codes.copy()
    keep = mask.copy()
    keep[1, 0, C] = 1
    big[1, 0, C] = 1024                                       # = codebook_size under a kept mask
    with pytest.raises(IndexError):
        pack_bitstream(t(big), t(keep), 1024)
    hidden = codes.copy()
    keep[0, :, 3] = 0
    hidden[0, 2, 3] = 5000                                    # masked out: not part of the stream
    pack_bitstream(t(hidden), t(keep), 1024)
    neg = codes.copy()
    neg[1, 0, C] = -1
    with pytest.raises(IndexError):
        pack_bitstream(t(neg), t(keep), 1024)


def test_unpack_rejects_corrupt_streams():
    """Every case is a bounds-checked rejection: the words tensor has its exact size."""
    nq, T = 9, 70
    codes, mask = make_case(2, nq, 1024, T, seed=9, extremes=False)
    mask[:, 0, :] = 1                                         # every frame keeps a code
    mask[0, 1:, :3] = 0                                       # ... and row 0's first three just one
    bs = pack_bitstream(t(codes), t(mask), 1024)
    good = u32(bs.words).copy()
    a_words = -(-T * 4 // 32)

    def stream(words, **kw):
        w = t(words.view(np.int32).copy())                    # exactly the stream's words
        return Bitstream(**dict(bs.__dict__, words=w, **kw))

    for row in (0, 1):                                        # a count of Nq + 1 = 10 in 4 bits
        w = good.copy()
        _put(w, 32 * (bs.row_words[0] * row) + 4 * 5, 4, nq + 1)
        with pytest.raises(ValueError):
            unpack_bitstream(stream(w))
    w = good.copy()                                           # counts that claim more words
    _put(w, 0, 4, nq)
    _put(w, 4, 4, nq)
    _put(w, 8, 4, nq)
    with pytest.raises(ValueError):                           # 24 codes more than the row holds
        unpack_bitstream(stream(w))
    with pytest.raises(ValueError):                           # one row_words entry patched
        unpack_bitstream(stream(good, row_words=(bs.row_words[0] + 1, bs.row_words[1])))
    with pytest.raises(ValueError):                           # two, so that the sum still fits
        unpack_bitstream(stream(good, row_words=(bs.row_words[0] + 1, bs.row_words[1] - 1)))
    with pytest.raises(ValueError):
        unpack_bitstream(stream(good, row_words=(bs.row_words[0] - 1, bs.row_words[1] + 1)))
    with pytest.raises(ValueError):                           # shorter than its count plane
        unpack_bitstream(stream(good, row_words=(a_words - 1, sum(bs.row_words) - a_words + 1)))
    # a code field of 1001 at codebook_size 1000
    codes7 = codes % 1000
    bs7 = pack_bitstream(t(codes7), t(mask), 1000)
    w = u32(bs7.words).copy()
    _put(w, 32 * a_words, 10, 1001)                           # the first code of row 0
    with pytest.raises(IndexError):
        unpack_bitstream(Bitstream(**dict(bs7.__dict__, words=t(w.view(np.int32).copy()))))
    c2, m2 = unpack_bitstream(bs7)                            # the untouched stream still decodes
    np.testing.assert_array_equal(c2.cpu().numpy(), codes7 * (mask != 0))


def test_corrupt_row_leaves_the_other_rows_alone():
    """Offsets come from the header's row_words: a corrupt row decodes to zeros and cannot move
    the rows after it (seen through the ops, which return the outputs beside the flags)."""
    nq, T = 9, 70
    codes, mask = make_case(3, nq, 1024, T, seed=4, extremes=False)
    bs = pack_bitstream(t(codes), t(mask), 1024)
    w = u32(bs.words).copy()
    _put(w, 32 * bs.row_words[0] + 4 * 7, 4, 12)              # row 1, frame 7
    ops = torch.ops.vrvq
    words = t(w.view(np.int32).copy())
    row_off = torch.tensor([0] + list(bs.row_words), dtype=torch.int64).cumsum(0).to(DEV)
    counts, chunk_off, flags = ops.bitunpack_plan(words, row_off, nq, T, 1024, 4)
    c2, m2 = ops.bitunpack_read(words, counts, chunk_off, row_off, flags, nq, 1024, 4)
    f = flags.tolist()                                        # row_err x 3, plan err, read err
    assert f[0] == 0 and f[1] != 0 and f[2] == 0 and f[3] in (3, 4) and f[4] == 0
    for r in (0, 2):
        np.testing.assert_array_equal(m2[r].cpu().numpy(), mask[r])
        np.testing.assert_array_equal(c2[r].cpu().numpy(), codes[r] * (mask[r] != 0))
    assert not bool(c2[1].any()) and not bool(m2[1].any())


# ------------------------------------------------------------------------------ end to end
_models = {}


def small_model(model_type="VBR"):
    if model_type not in _models:
        model = vrvq_amd.DAC_VRVQ(**{**KW, "model_type": model_type}, level_min=0.125,
                                  level_max=6.0)
        load_recipe(model, 0)
        _models[model_type] = model.to(DEV).eval()
    return _models[model_type]


@pytest.mark.parametrize("seconds,model_type", [(2.6, "VBR"), (0.7, "VBR"), (2.6, "CBR")])
def test_compress_decompress_vrvq_equals_dac(tmp_path, seconds, model_type):
    model = small_model(model_type)
    audio = _signal(int(seconds * SR), 7)
    kw = dict(win_duration=1.0, max_batch=2)
    dac = model.compress(audio, **kw)
    vf = model.compress(audio, container="vrvq", **kw)
    assert isinstance(dac, DACFile) and isinstance(vf, VRVQFile)
    assert not vf.bitstream.words.is_cuda
    assert torch.equal(vf.to_dac().codes, dac.codes)
    for k in ("chunk_length", "original_length", "channels", "sample_rate", "padding"):
        assert getattr(vf, k) == getattr(dac, k), k
    assert torch.equal(torch.as_tensor(vf.input_db), torch.as_tensor(dac.input_db))
    kept = int((dac.codes < model.codebook_size).sum())
    assert vf.bitstream.code_bits_total == 10 * kept
    if model_type == "VBR":
        assert vf.bitstream.count_bits == 4 and kept < dac.codes.numel()
    else:
        assert vf.bitstream.count_bits == 0 and kept == dac.codes.numel()
    p_dac, p_vf = dac.save(tmp_path / "x"), vf.save(tmp_path / "x")
    assert os.path.getsize(p_vf) < os.path.getsize(p_dac)
    a = model.decompress(p_dac).audio_data
    b = model.decompress(p_vf).audio_data
    assert a.shape == audio.shape and torch.equal(a, b)        # same codes, same kernels
    assert torch.equal(model.decompress(vf).audio_data, a)
    assert VRVQFile.load(p_vf).payload_kbps(model.sample_rate, model.hop_length) == pytest.approx(
        vf.bitstream.total_bits * (SR // model.hop_length) / dac.codes.shape[0]
        / dac.codes.shape[-1] / 1000.0)
    if model_type == "VBR":                                    # a VBR stream and a CBR model
        with pytest.raises(ValueError, match="quantizer is CBR"):
            codec.decompress(small_model("CBR"), vf)
    utils.check_errors(DEV)


def test_target_kbps_budgets_the_count_plane():
    model = small_model()
    audio = _signal(int(2.6 * SR), 7)
    nq, cb = model.n_codebooks, 4
    lo, hi = model.quantizer.level_min, model.quantizer.level_max
    kw = dict(win_duration=1.0, max_batch=2)
    # the file's rates at level_min and level_max, from the importance maps of its windows
    at = {}
    for lv in (lo, hi):
        f = model.compress(audio, level=lv, container="vrvq", **kw)
        at[lv] = f.bitstream.code_bits_total / (f.bitstream.rows * f.bitstream.frames)
    enc = model.encode(model.preprocess(audio.to(DEV).reshape(1, 1, -1), SR), None, 1,
                       want_z_q_is=False)
    curve = utils.rate_curve(enc["imp_map"], [lo, hi], nq).cpu().numpy()[0]
    assert curve[1] > curve[0] + cb and at[hi] > at[lo] + cb   # room between the two rates
    fps = SR // model.hop_length
    k = ((max(curve[0], at[lo]) + cb) + min(curve[1], at[hi])) / 2 * fps / 1000.0
    vf = model.compress(audio, target_kbps=k, container="vrvq", **kw)
    bs = vf.bitstream
    budget = utils.kbps_to_budget(k, bs.rows * bs.frames, model.sample_rate, model.hop_length)
    print(f"k {k:.3f} kbps: budget {budget}, counts {bs.count_bits_total}, codes "
          f"{bs.code_bits_total}, level {vf.level}")
    assert bs.count_bits_total == cb * bs.rows * bs.frames
    assert 0 < bs.count_bits_total + bs.code_bits_total <= budget
    plain = codec.solve_file_level(model, audio, k, **kw)
    assert vf.level <= plain and vf.target_kbps == pytest.approx(k)
    assert vf.level == codec.solve_file_level(model, audio, k, container="vrvq", **kw)
    # container="dac" budgets no side information: the codes of the plain solve, as before
    dac = model.compress(audio, target_kbps=k, **kw)
    assert torch.equal(dac.codes, model.compress(audio, level=plain, **kw).codes)
    assert torch.equal(vf.to_dac().codes, model.compress(audio, level=vf.level, **kw).codes)
    # the budget arithmetic of the solver itself
    imp = enc["imp_map"]
    T = imp.shape[-1]
    skw = dict(nq=nq, sample_rate=SR, hop_length=model.hop_length, level_min=lo, level_max=hi)
    l0, _, s0 = utils.solve_levels(imp, k, **skw)
    l1, bpf1, s1 = utils.solve_levels(imp, k, side_bits_per_frame=cb, **skw)
    assert int(s0) in (0, 2) and int(s1) == 0 and float(l1) <= float(l0)
    assert round(float(bpf1) * T) <= utils.kbps_to_budget(k, T, SR, model.hop_length) - cb * T
    # side information alone above the budget: status 1
    tiny = (cb - 1) * fps / 1000.0
    assert int(utils.solve_levels(imp, tiny, side_bits_per_frame=cb, **skw)[2]) == 1
    utils.check_errors(DEV)


# ------------------------------------------------------------------------------ C-ABI
def test_c_abi_plan_write_unpack():
    case = (2, 9, 1024, C + 1)
    R, nq, size, T = case
    codes, mask, words, row_words, info = reference(case)
    nchunk = -(-T // C)
    assert _lib.load().vrvq_bitstream_chunk_frames() == C
    P = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None  # noqa: E731
    z = lambda *s, dtype: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
    d_codes, d_mask = t(codes), t(mask)
    counts, ctot = z(R, T, dtype=torch.int32), z(R, nchunk, dtype=torch.int32)
    coff, rcodes = z(R, nchunk, dtype=torch.int64), z(R, dtype=torch.int64)
    rwords, roff, err = z(R, dtype=torch.int64), z(R + 1, dtype=torch.int64), z(1, dtype=torch.int32)
    torch.cuda.synchronize()
    _lib.call("vrvq_bitpack_plan", P(d_codes), P(d_mask), R, nq, T, size, P(counts), P(ctot),
              P(coff), P(rcodes), P(rwords), P(roff), P(err), None)
    torch.cuda.synchronize()
    assert int(err) == 0 and rwords.tolist() == row_words
    assert roff.tolist() == [0, row_words[0], sum(row_words)]
    assert rcodes.tolist() == [int(mask[r].sum()) for r in range(R)]
    np.testing.assert_array_equal(counts.cpu().numpy(), mask.sum(1).astype(np.int32))
    total = sum(row_words)
    out = torch.full((total,), -1, dtype=torch.int32, device=DEV)   # the op zeroes what it returns
    torch.cuda.synchronize()
    _lib.call("vrvq_bitpack_write", P(d_codes), P(counts), P(coff), P(roff), R, nq, T, size, 4,
              P(out), total, None)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(out), words)
    counts2, ctot2 = z(R, T, dtype=torch.int32), z(R, nchunk, dtype=torch.int32)
    coff2 = z(R, nchunk, dtype=torch.int64)
    row_err, err2 = z(R, dtype=torch.int32), z(1, dtype=torch.int32)
    c2 = z(R, nq, T, dtype=torch.int64)
    m2 = z(R, nq, T, dtype=torch.float32)
    torch.cuda.synchronize()
    _lib.call("vrvq_bitunpack_plan", P(out), total, P(roff), R, nq, T, size, 4, P(counts2),
              P(ctot2), P(coff2), P(row_err), P(err2), None)
    _lib.call("vrvq_bitunpack_read", P(out), total, P(counts2), P(coff2), P(roff), P(row_err),
              R, nq, T, size, 4, P(c2), P(m2), P(err2), None)
    torch.cuda.synchronize()
    assert int(err2) == 0 and row_err.tolist() == [0, 0]
    assert torch.equal(counts2, counts) and torch.equal(coff2, coff)
    np.testing.assert_array_equal(m2.cpu().numpy(), mask)
    np.testing.assert_array_equal(c2.cpu().numpy(), codes * (mask != 0))
    # host-side argument checks reject before any launch
    with pytest.raises(RuntimeError):
        _lib.call("vrvq_bitpack_plan", P(d_codes), P(d_mask), R, 256, T, size, P(counts), P(ctot),
                  P(coff), P(rcodes), P(rwords), P(roff), P(err), None)
    with pytest.raises(RuntimeError):
        _lib.call("vrvq_bitpack_write", P(d_codes), P(counts), P(coff), P(roff), R, nq, T, 65537,
                  4, P(out), total, None)
    with pytest.raises(RuntimeError):
        _lib.call("vrvq_bitunpack_plan", P(out), total, P(roff), R, nq, T, size, 3, P(counts2),
                  P(ctot2), P(coff2), P(row_err), P(err2), None)
