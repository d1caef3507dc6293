"""VRVQ bitstream 1 on the host: the reference packer (tests/bitstream_ref.py) against a
hand-written known answer, the package's host packer against it, the `.vrvq` container, and the
budget arithmetic of solve_levels(side_bits_per_frame=...). No GPU."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import bitstream_ref as ref
from oracle.vrvq_oracle import generate_mask_hard
from vrvq_amd import _lib, codes_io, utils
from vrvq_amd.codes_io import Bitstream, DACFile, VRVQFile, pack_bitstream, unpack_bitstream


def _case(R, nq, size, T, seed=0):
    g = np.random.default_rng(seed)
    codes = g.integers(0, size, (R, nq, T)).astype(np.int64)
    mask = generate_mask_hard(g.uniform(-0.5, nq + 0.5, (R, 1, T)).astype(np.float32), nq)
    return codes, mask.astype(np.float32)


# ------------------------------------------------------------------------------ the format
def test_known_answer():
    """R = 1, Nq = 3, codebook_size = 8: cb = 2, w = 3. 12 frames, 19 kept codes.

    Plane A, 2-bit counts from bit 0 (t = 0 lowest): t11..t8 = 01 11 10 01 = 0x79,
    t7..t4 = 00 00 11 11 = 0x0F, t3..t0 = 10 01 00 11 = 0x93 -> 0x00790F93 (24 bits, one word).
    Plane B, the kept codes in frame-major order are 1,2,3,4,5,6,7,0,1,2,3,4,5,6,7,0,1,2,3 at
    3 bits each, i.e. the octal digits of the plane from the lowest: codes 0..9 fill bits 0..29
    (octal 2107654321 = 0x111F58D1), code 10 (= 3 = 0b011) straddles: its low two bits 11 are
    bits 30..31 -> word 0 = 0xD11F58D1; its high bit 0 is bit 0 of word 1, and codes 11..18
    (4,5,6,7,0,1,2,3: octal 32107654 = 0x688FAC) follow from bit 1 -> word 1 = 0x00D11F58."""
    counts = [3, 0, 1, 2, 3, 3, 0, 0, 1, 2, 3, 1]
    codes = np.full((1, 3, 12), 7, np.int64)          # 7 where masked: must not reach the stream
    mask = np.zeros((1, 3, 12), np.float32)
    k = 0
    for t, c in enumerate(counts):
        for i in range(c):
            codes[0, i, t] = (k + 1) % 8
            mask[0, i, t] = 1
            k += 1
    assert k == 19
    words, row_words, info = ref.pack(codes, mask, 8)
    assert (info["count_bits"], info["code_bits"]) == (2, 3)
    assert (info["count_bits_total"], info["code_bits_total"], info["padding_bits"]) == (24, 57, 15)
    expect = [0x00790F93, 0xD11F58D1, 0x00D11F58]
    assert [int(v) for v in words] == expect and row_words == [3]
    c2, m2 = ref.unpack(words, row_words, 3, 8, 12, 2)
    np.testing.assert_array_equal(m2, mask)
    np.testing.assert_array_equal(c2, codes * (mask != 0))
    # the package's host packer writes the same words
    bs = pack_bitstream(torch.from_numpy(codes), torch.from_numpy(mask), 8)
    assert [int(v) for v in bs.words.numpy().view(np.uint32)] == expect
    assert bs.row_words == (3,) and (bs.count_bits, bs.code_bits) == (2, 3)
    assert (bs.count_bits_total, bs.code_bits_total, bs.padding_bits) == (24, 57, 15)


def test_field_widths():
    assert [ref.code_bits(n) for n in (2, 3, 16, 1000, 1024, 1025, 65536)] == [1, 2, 4, 10, 10, 11, 16]
    assert [ref.count_bits(n) for n in (1, 3, 8, 9, 32, 255)] == [1, 2, 4, 4, 6, 8]
    for n in (2, 3, 16, 1000, 1024, 1025, 65536):
        assert codes_io.code_bits_of(n) == ref.code_bits(n)
    for n in (1, 3, 8, 9, 32, 255):
        assert codes_io.count_bits_of(n) == ref.count_bits(n)
    assert codes_io.BITSTREAM_CHUNK_FRAMES == _lib.BITSTREAM_CHUNK_FRAMES
    lib = _lib.load()
    assert lib.vrvq_version() >= 110
    assert lib.vrvq_bitstream_chunk_frames() == _lib.BITSTREAM_CHUNK_FRAMES
    header = (Path(__file__).resolve().parents[1] / "include" / "vrvq.h").read_text()
    assert f"#define VRVQ_BITSTREAM_CHUNK_FRAMES {_lib.BITSTREAM_CHUNK_FRAMES}\n" in header


CASES = [(1, 9, 1024, 1), (3, 9, 1024, 40), (2, 32, 1024, 23), (2, 5, 2, 67), (2, 4, 65536, 33),
         (2, 7, 1000, 29), (5, 3, 16, 5)]


@pytest.mark.parametrize("R,nq,size,T", CASES)
def test_reference_round_trip_and_row_words(R, nq, size, T):
    codes, mask = _case(R, nq, size, T, seed=T)
    if T > 2:
        mask[0, :, :] = 0                                 # an empty plane B
        mask[-1, :, :] = 1                                # every count Nq
    words, row_words, info = ref.pack(codes, mask, size)
    w, cb = ref.code_bits(size), ref.count_bits(nq)
    for r in range(R):
        kept = int(mask[r].sum())
        assert row_words[r] == -(-T * cb // 32) + -(-w * kept // 32)
    assert len(words) == sum(row_words)
    assert info["code_bits_total"] == w * int(mask.sum())
    assert info["count_bits_total"] == R * T * cb
    c2, m2 = ref.unpack(words, row_words, nq, size, T, cb)
    np.testing.assert_array_equal(m2, mask)
    np.testing.assert_array_equal(c2, codes * (mask != 0))
    # rows do not depend on each other
    off = 0
    for r in range(R):
        alone, rw, _ = ref.pack(codes[r:r + 1], mask[r:r + 1], size)
        np.testing.assert_array_equal(alone, words[off:off + row_words[r]])
        off += row_words[r]
    # the host packer of the package: same words, same accounting, and its own round trip
    bs = pack_bitstream(torch.from_numpy(codes), torch.from_numpy(mask), size)
    np.testing.assert_array_equal(bs.words.numpy().view(np.uint32), words)
    assert list(bs.row_words) == row_words
    assert (bs.code_bits_total, bs.count_bits_total, bs.padding_bits) == (
        info["code_bits_total"], info["count_bits_total"], info["padding_bits"])
    c3, m3 = unpack_bitstream(bs)
    np.testing.assert_array_equal(m3.numpy(), mask)
    np.testing.assert_array_equal(c3.numpy(), c2)


def test_fixed_count_stream_has_no_plane_a():
    codes, _ = _case(2, 9, 1024, 13)
    words, row_words, info = ref.pack(codes, None, 1024)
    assert info["count_bits"] == 0 and info["count_bits_total"] == 0
    assert row_words == [-(-10 * 9 * 13 // 32)] * 2
    bs = pack_bitstream(torch.from_numpy(codes), None, 1024)
    np.testing.assert_array_equal(bs.words.numpy().view(np.uint32), words)
    assert bs.count_bits == 0
    c2, m2 = unpack_bitstream(bs)
    assert torch.equal(c2, torch.from_numpy(codes)) and bool((m2 == 1).all())


def test_reference_and_host_packer_reject_bad_input():
    codes, mask = _case(1, 9, 1000, 8)
    bad = mask.copy()
    bad[0, :, 3] = 0
    bad[0, 4, 3] = 1
    big = codes.copy()
    mask[0, 0, 2] = 1
    big[0, 0, 2] = 1000
    for pack in (lambda c, m: ref.pack(c, m, 1000),
                 lambda c, m: pack_bitstream(torch.from_numpy(c), torch.from_numpy(m), 1000)):
        with pytest.raises(ValueError):
            pack(codes, bad)
        with pytest.raises(IndexError):
            pack(big, mask)
    bs = pack_bitstream(torch.from_numpy(codes), torch.from_numpy(mask), 1000)
    with pytest.raises(ValueError):
        unpack_bitstream(Bitstream(**dict(bs.__dict__, row_words=(bs.row_words[0] + 1,))))
    with pytest.raises(ValueError):
        pack_bitstream(torch.zeros(1, 256, 4, dtype=torch.int64), None, 1024)
    with pytest.raises(ValueError):
        pack_bitstream(torch.zeros(1, 4, 4, dtype=torch.int64), None, 65537)


# ------------------------------------------------------------------------------ the container
def _file(R=2, nq=9, size=1024, chunk=29, nwin=3, seed=3, vbr=True):
    codes, mask = _case(R, nq, size, chunk * nwin, seed)
    bs = pack_bitstream(torch.from_numpy(codes), torch.from_numpy(mask) if vbr else None, size)
    f = VRVQFile(bitstream=bs, chunk_length=chunk, original_length=12345,
                 input_db=torch.tensor([-23.5]), channels=R, sample_rate=48000, padding=False,
                 level=2.5, target_kbps=4.0)
    return f, codes, mask


def _split(path):
    blob = open(path, "rb").read()
    hlen = int.from_bytes(blob[8:12], "little")
    return blob, hlen


def test_vrvqfile_save_load_round_trip_and_exact_size(tmp_path):
    f, codes, mask = _file()
    path = f.save(tmp_path / "clip")
    assert path.suffix == ".vrvq"
    blob, hlen = _split(path)
    assert blob[:8] == b"VRVQBS01" and hlen % 4 == 0
    header = json.loads(blob[12:12 + hlen].decode("utf-8"))
    assert header["row_words"] == list(f.bitstream.row_words)
    assert len(blob) == 12 + hlen + 4 * sum(f.bitstream.row_words)        # header + words, exactly
    assert blob[12 + hlen:] == f.bitstream.words.numpy().astype("<i4").tobytes()
    assert b"numpy" not in blob and b"pickle" not in blob
    g = VRVQFile.load(path)
    assert g.bitstream.row_words == f.bitstream.row_words
    assert torch.equal(g.bitstream.words, f.bitstream.words)
    for k in ("n_codebooks", "codebook_size", "frames", "count_bits", "code_bits", "code_bits_total",
              "count_bits_total", "padding_bits"):
        assert getattr(g.bitstream, k) == getattr(f.bitstream, k), k
    for k in ("chunk_length", "original_length", "channels", "sample_rate", "padding", "level",
              "target_kbps"):
        assert getattr(g, k) == getattr(f, k), k
    assert torch.equal(torch.as_tensor(g.input_db), f.input_db)
    c2, m2 = unpack_bitstream(g.bitstream)
    np.testing.assert_array_equal(m2.numpy(), mask)
    np.testing.assert_array_equal(c2.numpy(), codes * (mask != 0))
    # 32 * sum(row_words) bits over rows * frames frames at floor(44100 / 512) = 86 frames/s
    bits = 32 * sum(f.bitstream.row_words)
    assert f.payload_kbps(44100, 512) == pytest.approx(bits * 86 / (2 * 87) / 1000.0, rel=1e-12)


def test_to_dac_from_dac_round_trip():
    for vbr in (True, False):
        f, codes, mask = _file(vbr=vbr)
        dac = f.to_dac()
        assert isinstance(dac, DACFile) and dac.codes.dtype == torch.int64
        expect = np.where(mask != 0, codes, 1024) if vbr else codes
        np.testing.assert_array_equal(dac.codes.numpy(), expect)
        assert (dac.chunk_length, dac.original_length, dac.channels, dac.sample_rate,
                dac.padding) == (29, 12345, 2, 48000, False)
        g = VRVQFile.from_dac(dac, 1024)
        assert torch.equal(g.bitstream.words, f.bitstream.words)
        assert g.bitstream.row_words == f.bitstream.row_words
        assert g.bitstream.count_bits == f.bitstream.count_bits
        assert torch.equal(g.to_dac().codes, dac.codes)


def test_load_rejects_corrupt_files(tmp_path):
    f, _, _ = _file()
    path = f.save(tmp_path / "ok")
    blob, hlen = _split(path)
    VRVQFile.load(path)

    def check(name, data, match):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(RuntimeError, match=match):
            VRVQFile.load(p)

    check("magic.vrvq", b"VRVQXX01" + blob[8:], "magic")
    check("version.vrvq", b"VRVQBS02" + blob[8:], "version")
    check("short.vrvq", blob[:-4], "payload")
    check("cut.vrvq", blob[:-1], "payload")
    check("long.vrvq", blob + b"\0\0\0\0", "payload")
    check("header.vrvq", blob[:12 + hlen // 2], "header")

    def with_header(change):
        h = json.loads(blob[12:12 + hlen].decode("utf-8"))
        change(h)
        hb = json.dumps(h).encode("utf-8")
        hb += b" " * (-len(hb) % 4)
        return blob[:8] + len(hb).to_bytes(4, "little") + hb + blob[12 + hlen:]

    def bump(h):
        h["row_words"][0] += 1
    check("rows.vrvq", with_header(bump), "payload")               # row_words against the payload
    check("nq.vrvq", with_header(lambda h: h.update(n_codebooks=300)), "header")
    check("cb.vrvq", with_header(lambda h: h.update(count_bits=3)), "header")
    check("w.vrvq", with_header(lambda h: h.update(code_bits=16)), "header")
    check("frames.vrvq", with_header(lambda h: h.update(frames=0)), "header")
    check("chunk.vrvq", with_header(lambda h: h.update(chunk_length=7)), "header")
    check("neg.vrvq", with_header(lambda h: h.update(row_words=[-1, 1])), "header")
    check("type.vrvq", with_header(lambda h: h.update(frames="87")), "header")
    check("missing.vrvq", with_header(lambda h: h.pop("sample_rate")), "header")
    assert codes_io.is_vrvq_file(path)
    other = tmp_path / "x.dac"
    other.write_bytes(b"\x93NUMPY\x01\x00")
    assert not codes_io.is_vrvq_file(other)


# ------------------------------------------------------------------------------ the budget
def test_side_information_budget_arithmetic():
    """solve_levels takes frames * side_bits_per_frame off every group's budget on the host
    (the solve itself runs on the GPU: tests/test_gpu_bitstream.py)."""
    b = utils.kbps_to_budget(4.0, 174, 44100, 512)
    assert utils.net_budgets([b], 174, 0) == [b]
    assert utils.net_budgets([b], 174, 4) == [b - 4 * 174]
    assert utils.net_budgets([100, 2000], 87, 4) == [100 - 348, 2000 - 348]
    assert utils.net_budgets([100], 87, 4)[0] < 0           # negative: solve_levels status 1
    with pytest.raises(ValueError):
        utils.net_budgets([100], 87, -1)
    with pytest.raises(ValueError):
        utils.net_budgets([100], 87, 0.5)
