"""Code containers either side of the path.

* `DACFile` — the reference's `.dac` container (`models/dac_base.py:19-58`): same fields, same
  on-disk layout (an `np.save`d dict holding uint16 codes + metadata, dac_version "1.0.0"), so
  files round-trip with the reference. Loading uses a restricted unpickler that only rebuilds
  numpy arrays / scalars and plain containers, never arbitrary objects.
* `pack_codes` / `unpack_codes` — variable-length packing of VBR codes by their importance mask
  on the GPU (`vrvq_pack_*` kernels, include/vrvq.h): only the codes whose mask is 1 are kept,
  frame-major, plus one count per frame. `save_packed` / `load_packed` store that as a
  pickle-free `.npz` (uint16 stream, uint8 counts, JSON metadata).
* `pack_bitstream` / `unpack_bitstream` — "VRVQ bitstream 1" (include/vrvq.h "Bitstream"): the
  same kept codes at their exact width (10 bits of a 1024-entry codebook, 4 bits of a count of
  0..9), one count plane and one code plane per row, packed and unpacked on the GPU
  (`vrvq_bitpack_*` / `vrvq_bitunpack_*`) by workgroups of `BITSTREAM_CHUNK_FRAMES` frames.
  `VRVQFile` is the `.dac` counterpart holding such a stream: an 8-byte magic, a JSON header and
  the words, no pickle.
"""
from __future__ import annotations

import io
import json
import pickle
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

from ._lib import BITSTREAM_CHUNK_FRAMES  # frames one workgroup packs / unpacks
from .ops import _ops

SUPPORTED_VERSIONS = ["1.0.0"]
MAX_CODEBOOKS = 255  # counts are stored as uint8 (save_packed)


# ----------------------------------------------------------------------------- GPU packing
def pack_codes(codes: torch.Tensor, mask: torch.Tensor, codebook_size: int = 1024
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """codes (B, Nq, T) int64 + prefix-shaped mask (B, Nq, T) -> (packed uint16 stream as int16
    storage, counts (B, T) int32). Raises ValueError for a non-prefix mask column and
    IndexError for a code outside [0, codebook_size). The packed length is data-dependent, so
    this synchronises the host once (like torch.nonzero)."""
    if codes.dim() != 3 or mask.shape != codes.shape:
        raise RuntimeError("pack_codes: codes and mask must both be (B, Nq, T)")
    if codes.shape[1] > MAX_CODEBOOKS:
        raise ValueError(f"pack_codes: at most {MAX_CODEBOOKS} codebooks")
    counts, off, err = _ops().pack_counts(mask)
    B = codes.shape[0]
    total = int(off[B].item())
    if int(err.item()) == 1:
        raise ValueError("pack_codes: mask is not prefix-shaped (a 1 after a 0 along Nq)")
    packed, err2 = _ops().pack_codes(codes, counts, off, total, int(codebook_size))
    if total and int(err2.item()) == 2:
        raise IndexError(f"pack_codes: code outside [0, {codebook_size})")
    return packed, counts


def unpack_codes(packed: torch.Tensor, counts: torch.Tensor, n_codebooks: int
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of pack_codes: -> codes (B, Nq, T) int64 (0 where masked), mask (B, Nq, T).
    n_codebooks must be the value the stream was packed with (load_packed returns it in the
    metadata); a stream whose counts exceed it, or whose length disagrees with the counts,
    raises ValueError."""
    if not 0 < int(n_codebooks) <= MAX_CODEBOOKS:
        raise ValueError(f"unpack_codes: n_codebooks must be in [1, {MAX_CODEBOOKS}]")
    if packed.dim() != 1:
        raise ValueError("unpack_codes: packed must be a 1-D stream")
    if counts.dim() != 2:
        raise ValueError("unpack_codes: counts must be (B, T)")
    if int(counts.min()) < 0 or int(counts.max()) > n_codebooks:
        raise ValueError(f"unpack_codes: counts outside [0, {n_codebooks}]")
    off = _ops().unpack_offsets(counts)
    B = counts.shape[0]
    if int(off[B].item()) != packed.numel():
        raise ValueError(f"unpack_codes: stream holds {packed.numel()} codes, counts say "
                         f"{int(off[B].item())}")
    return _ops().unpack_codes(packed, counts, off, int(n_codebooks))


def save_packed(path, packed: torch.Tensor, counts: torch.Tensor, n_codebooks: int,
                **metadata) -> Path:
    """Pickle-free container of a packed stream: packed (uint16), counts (uint8), metadata."""
    path = Path(path).with_suffix(".vrvq.npz")
    meta = dict(metadata, n_codebooks=int(n_codebooks), dac_version=SUPPORTED_VERSIONS[-1])
    np.savez(path, packed=packed.cpu().numpy().view(np.uint16),
             counts=counts.cpu().numpy().astype(np.uint8), metadata=np.array(json.dumps(meta)))
    return path


def load_packed(path, device="cuda"):
    with np.load(path, allow_pickle=False) as z:
        meta = json.loads(str(z["metadata"]))
        if meta.get("dac_version") not in SUPPORTED_VERSIONS:
            raise RuntimeError(f"{path}: unsupported version {meta.get('dac_version')}")
        packed = torch.from_numpy(z["packed"].view(np.int16).copy()).to(device)
        counts = torch.from_numpy(z["counts"].astype(np.int32)).to(device)
    return packed, counts, meta


# ----------------------------------------------------------------------------- .dac files
class _ArrayUnpickler(pickle.Unpickler):
    """Rebuilds only what `np.save` of a dict of arrays / scalars / plain values contains."""
    _ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
                ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                ("numpy", "ndarray"), ("numpy", "dtype")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f".dac file references {module}.{name}: refused")


@dataclass
class DACFile:
    """models/dac_base.py:19-58 (same fields, same file layout)."""
    codes: torch.Tensor
    chunk_length: int
    original_length: int
    input_db: object
    channels: int
    sample_rate: int
    padding: bool
    dac_version: str

    def save(self, path) -> Path:
        input_db = self.input_db
        if isinstance(input_db, torch.Tensor):
            input_db = input_db.detach().cpu().numpy()
        artifacts = {
            "codes": self.codes.detach().cpu().numpy().astype(np.uint16),
            "metadata": {
                "input_db": np.asarray(input_db).astype(np.float32),
                "original_length": self.original_length,
                "sample_rate": self.sample_rate,
                "chunk_length": self.chunk_length,
                "channels": self.channels,
                "padding": self.padding,
                "dac_version": SUPPORTED_VERSIONS[-1],
            },
        }
        path = Path(path).with_suffix(".dac")
        with open(path, "wb") as f:
            np.save(f, artifacts)
        return path

    @classmethod
    def load(cls, path) -> "DACFile":
        with open(path, "rb") as f:
            version = np.lib.format.read_magic(f)
            read = (np.lib.format.read_array_header_1_0 if version == (1, 0)
                    else np.lib.format.read_array_header_2_0)
            shape, _, dtype = read(f)
            if dtype != np.dtype(object) or shape != ():
                raise RuntimeError(f"{path}: not a .dac container")
            artifacts = _ArrayUnpickler(io.BytesIO(f.read())).load()
        if not isinstance(artifacts, np.ndarray) or artifacts.shape != ():
            raise RuntimeError(f"{path}: not a .dac container")
        artifacts = artifacts[()]
        if artifacts["metadata"].get("dac_version", None) not in SUPPORTED_VERSIONS:
            raise RuntimeError(
                f"Given file {path} can't be loaded with this version of descript-audio-codec.")
        codes = torch.from_numpy(artifacts["codes"].astype(int))
        return cls(codes=codes, **artifacts["metadata"])


# ----------------------------------------------------------------------------- bitstream
BITSTREAM_MAGIC = b"VRVQBS"       # followed by the two-digit format version
BITSTREAM_VERSION = 1
MAX_FRAMES = 1 << 24
MAX_ROWS = 1 << 30


def code_bits_of(codebook_size: int) -> int:
    """Bits of one code field: max(1, ceil(log2(codebook_size)))."""
    return max(1, (int(codebook_size) - 1).bit_length())


def count_bits_of(n_codebooks: int) -> int:
    """Bits of one count field (values 0 .. n_codebooks): ceil(log2(n_codebooks + 1))."""
    return int(n_codebooks).bit_length()


def _words_of(bits: int) -> int:
    return (int(bits) + 31) // 32


def _check_stream_fields(n_codebooks, codebook_size, frames, count_bits, code_bits, what):
    if not 0 < int(n_codebooks) <= MAX_CODEBOOKS:
        raise ValueError(f"{what}: n_codebooks must be in [1, {MAX_CODEBOOKS}]")
    if not 2 <= int(codebook_size) <= 65536:
        raise ValueError(f"{what}: codebook_size must be in [2, 65536]")
    if not 0 < int(frames) <= MAX_FRAMES:
        raise ValueError(f"{what}: frames must be in [1, {MAX_FRAMES}]")
    if int(code_bits) != code_bits_of(codebook_size):
        raise ValueError(f"{what}: code_bits {code_bits} does not belong to codebook_size "
                         f"{codebook_size}")
    if int(count_bits) not in (0, count_bits_of(n_codebooks)):
        raise ValueError(f"{what}: count_bits {count_bits} does not belong to n_codebooks "
                         f"{n_codebooks}")


@dataclass
class Bitstream:
    """A packed "VRVQ bitstream 1" and what is needed to read it. `words` is the stream, a 1-D
    int32 tensor holding little-endian uint32 words; `row_words[r]` words belong to row r.
    count_bits = 0: every frame keeps all n_codebooks stages and there is no count plane.
    code_bits_total + count_bits_total + padding_bits = 32 * sum(row_words)."""
    words: torch.Tensor
    row_words: Tuple[int, ...]
    n_codebooks: int
    codebook_size: int
    frames: int
    count_bits: int
    code_bits: int
    code_bits_total: int
    count_bits_total: int
    padding_bits: int

    @property
    def rows(self) -> int:
        return len(self.row_words)

    @property
    def total_bits(self) -> int:
        return 32 * sum(self.row_words)

    def to(self, device) -> "Bitstream":
        return Bitstream(**dict(self.__dict__, words=self.words.to(device)))


def _make_bitstream(words, row_words, row_codes, nq, codebook_size, T, cb) -> Bitstream:
    w = code_bits_of(codebook_size)
    row_words = tuple(int(v) for v in row_words)
    code_total = w * sum(int(v) for v in row_codes)
    count_total = len(row_words) * T * cb
    return Bitstream(words=words, row_words=row_words, n_codebooks=nq,
                     codebook_size=int(codebook_size), frames=T, count_bits=cb, code_bits=w,
                     code_bits_total=code_total, count_bits_total=count_total,
                     padding_bits=32 * sum(row_words) - code_total - count_total)


def _fields_to_words(values: np.ndarray, width: int) -> np.ndarray:
    """`width`-bit fields, back to back from bit 0, zero-padded to whole uint32 words."""
    if values.size == 0 or width == 0:
        return np.zeros(0, np.uint32)
    bits = ((values.astype(np.uint32)[:, None] >> np.arange(width, dtype=np.uint32)) & 1)
    bits = bits.astype(np.uint8).reshape(-1)
    bits = np.concatenate([bits, np.zeros(-bits.size % 32, np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def _words_to_fields(words: np.ndarray, width: int, n: int) -> np.ndarray:
    if n == 0 or width == 0:
        return np.zeros(n, np.int64)
    bits = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")[:n * width]
    return bits.reshape(n, width).astype(np.int64) @ (1 << np.arange(width, dtype=np.int64))


def _pack_host(codes, mask, codebook_size) -> Bitstream:
    """pack_bitstream for host tensors (container conversion without a GPU), in NumPy."""
    c = codes.numpy()
    R, nq, T = c.shape
    cb = 0 if mask is None else count_bits_of(nq)
    w = code_bits_of(codebook_size)
    m = np.ones(c.shape, bool) if mask is None else mask.numpy() != 0
    if (m[:, 1:] & ~m[:, :-1]).any():
        raise ValueError("pack_bitstream: mask is not prefix-shaped (a 1 after a 0 along Nq)")
    if ((c < 0) | (c >= codebook_size))[m].any():
        raise IndexError(f"pack_bitstream: code outside [0, {codebook_size})")
    out, row_words, row_codes = [], [], []
    for r in range(R):
        a = _fields_to_words(m[r].sum(0), cb)
        b = _fields_to_words(c[r].T[m[r].T], w)              # frame-major, stage-minor
        out += [a, b]
        row_words.append(a.size + b.size)
        row_codes.append(int(m[r].sum()))
    words = torch.from_numpy(np.concatenate(out).astype(np.uint32).view(np.int32).copy())
    return _make_bitstream(words, row_words, row_codes, nq, codebook_size, T, cb)


def pack_bitstream(codes: torch.Tensor, mask: Optional[torch.Tensor], codebook_size: int = 1024
                   ) -> Bitstream:
    """codes (R, Nq, T) int64 + prefix-shaped mask (R, Nq, T) -> Bitstream: per row a plane of T
    counts (count_bits each) and a plane of the kept codes (code_bits each), frame-major.
    mask=None keeps every stage and writes no count plane (count_bits = 0). Raises ValueError for
    a non-prefix mask column and IndexError for a kept code outside [0, codebook_size). A row's
    words do not depend on the other rows. The length is data-dependent, so this synchronises the
    host once, between the plan and the write (as pack_codes does). Tensors on a GPU are packed
    there by the HIP kernels; host tensors (container conversion) in NumPy, to the same words."""
    if codes.dim() != 3 or (mask is not None and mask.shape != codes.shape):
        raise RuntimeError("pack_bitstream: codes and mask must both be (R, Nq, T)")
    R, nq, T = codes.shape
    cb = 0 if mask is None else count_bits_of(nq)
    _check_stream_fields(nq, codebook_size, T, cb, code_bits_of(codebook_size), "pack_bitstream")
    if not 0 < R <= MAX_ROWS:
        raise ValueError("pack_bitstream: unsupported number of rows")
    codes = codes.to(torch.int64).contiguous()
    if mask is not None:
        mask = mask.to(torch.float32).contiguous()
    if not codes.is_cuda:
        return _pack_host(codes, mask, int(codebook_size))
    counts, chunk_off, info = _ops().bitpack_plan(codes, mask, int(codebook_size))
    h = info.cpu().numpy()                                   # the one host sync
    err = int(h[3 * R + 1]) & 0xFFFFFFFF
    if err == 1:
        raise ValueError("pack_bitstream: mask is not prefix-shaped (a 1 after a 0 along Nq)")
    if err == 2:
        raise IndexError(f"pack_bitstream: code outside [0, {codebook_size})")
    words = _ops().bitpack_write(codes, counts, chunk_off, info, int(h[R]), int(codebook_size),
                                 cb)
    return _make_bitstream(words, h[2 * R + 1:3 * R + 1], h[R + 1:2 * R + 1], nq, codebook_size,
                           T, cb)


def _check_bitstream(bs: Bitstream, what: str) -> None:
    _check_stream_fields(bs.n_codebooks, bs.codebook_size, bs.frames, bs.count_bits,
                         bs.code_bits, what)
    if bs.words.dim() != 1 or bs.words.dtype != torch.int32:
        raise ValueError(f"{what}: words must be a 1-D int32 tensor")
    if not 0 < len(bs.row_words) <= MAX_ROWS or any(int(v) < 0 for v in bs.row_words):
        raise ValueError(f"{what}: row_words must be non-negative, one per row")
    if sum(int(v) for v in bs.row_words) != bs.words.numel():
        raise ValueError(f"{what}: stream holds {bs.words.numel()} words, row_words say "
                         f"{sum(int(v) for v in bs.row_words)}")


def _unpack_host(bs: Bitstream):
    nq, T, cb, w = bs.n_codebooks, bs.frames, bs.count_bits, bs.code_bits
    words = bs.words.numpy().view(np.uint32)
    R = len(bs.row_words)
    codes = np.zeros((R, nq, T), np.int64)
    mask = np.zeros((R, nq, T), np.float32)
    a_words, off = _words_of(T * cb), 0
    for r, n in enumerate(bs.row_words):
        row, off = words[off:off + n], off + n
        if n < a_words:
            raise ValueError(f"unpack_bitstream: row {r} is shorter than its count plane")
        counts = _words_to_fields(row[:a_words], cb, T) if cb else np.full(T, nq, np.int64)
        if counts.max() > nq:
            raise ValueError(f"unpack_bitstream: counts outside [0, {nq}]")
        total = int(counts.sum())
        if a_words + _words_of(total * w) != n:
            raise ValueError(f"unpack_bitstream: row {r} holds {n} words, its counts say "
                             f"{a_words + _words_of(total * w)}")
        m = np.arange(nq)[None, :] < counts[:, None]          # (T, nq)
        vals = _words_to_fields(row[a_words:], w, total)
        if (vals >= bs.codebook_size).any():
            raise IndexError(f"unpack_bitstream: code outside [0, {bs.codebook_size})")
        ct = np.zeros((T, nq), np.int64)
        ct[m] = vals
        codes[r], mask[r] = ct.T, m.T
    return torch.from_numpy(codes), torch.from_numpy(mask)


def unpack_bitstream(bs: Bitstream) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of pack_bitstream: -> codes (R, Nq, T) int64 (0 where masked), mask (R, Nq, T)
    float32, on the stream's device. Raises ValueError for a count above n_codebooks or a row
    whose counts disagree with row_words, IndexError for a code >= codebook_size. Nothing outside
    the sum(row_words) words is read, whatever the counts say."""
    _check_bitstream(bs, "unpack_bitstream")
    if not bs.words.is_cuda:
        return _unpack_host(bs)
    # the rows' offsets are the scan of the header's row_words, not of anything in the stream
    row_off = torch.from_numpy(np.concatenate([[0], np.cumsum(bs.row_words, dtype=np.int64)])
                               ).to(bs.words.device)
    words = bs.words.contiguous()
    counts, chunk_off, flags = _ops().bitunpack_plan(words, row_off, bs.n_codebooks, bs.frames,
                                                     bs.codebook_size, bs.count_bits)
    codes, mask = _ops().bitunpack_read(words, counts, chunk_off, row_off, flags, bs.n_codebooks,
                                        bs.codebook_size, bs.count_bits)
    e = flags[-2:].tolist()                                  # the plan's code, the read's
    if e[0] == 3:
        raise ValueError(f"unpack_bitstream: counts outside [0, {bs.n_codebooks}]")
    if e[0] or e[1] == 4:
        raise ValueError("unpack_bitstream: a row's counts disagree with its row_words")
    if e[1] == 2:
        raise IndexError(f"unpack_bitstream: code outside [0, {bs.codebook_size})")
    return codes, mask


@dataclass
class VRVQFile:
    """The `.vrvq` container: a Bitstream plus the DACFile metadata. Rows are the DACFile's items
    (batch x channels), frames = windows x chunk_length. On disk: 8-byte magic (format version
    included), little-endian uint32 header length, UTF-8 JSON header space-padded to a multiple
    of 4 bytes, then the stream's words, little-endian. No pickle, no NumPy container."""
    bitstream: Bitstream
    chunk_length: int
    original_length: int
    input_db: object
    channels: int
    sample_rate: int
    padding: bool
    level: Optional[float] = None
    target_kbps: Optional[float] = None
    max_kbps: Optional[float] = None       # compress(max_kbps=...): the cap of every packet of
    packet_frames: Optional[int] = None    # packet_frames frames; in the header only when set

    def _header(self) -> dict:
        bs = self.bitstream
        input_db = self.input_db
        if isinstance(input_db, torch.Tensor):
            input_db = input_db.detach().cpu().numpy()
        # a file written without a cap has the header, byte for byte, it had before caps existed
        capped = {k: v for k, v in (
            ("max_kbps", None if self.max_kbps is None else float(self.max_kbps)),
            ("packet_frames", None if self.packet_frames is None else int(self.packet_frames)))
            if v is not None}
        return {
            "format": "VRVQ bitstream", "version": BITSTREAM_VERSION,
            "n_codebooks": bs.n_codebooks, "codebook_size": bs.codebook_size,
            "frames": bs.frames, "count_bits": bs.count_bits, "code_bits": bs.code_bits,
            "row_words": [int(v) for v in bs.row_words],
            "chunk_length": int(self.chunk_length), "original_length": int(self.original_length),
            "input_db": [float(v) for v in np.asarray(input_db, np.float32).reshape(-1)],
            "channels": int(self.channels), "sample_rate": int(self.sample_rate),
            "padding": bool(self.padding),
            "level": None if self.level is None else float(self.level),
            "target_kbps": None if self.target_kbps is None else float(self.target_kbps),
            **capped,
        }

    def save(self, path) -> Path:
        header = json.dumps(self._header()).encode("utf-8")
        header += b" " * (-len(header) % 4)
        words = self.bitstream.words.detach().cpu().numpy().view(np.uint32).astype("<u4")
        path = Path(path).with_suffix(".vrvq")
        with open(path, "wb") as f:
            f.write(BITSTREAM_MAGIC + b"%02d" % BITSTREAM_VERSION)
            f.write(np.array([len(header)], "<u4").tobytes())
            f.write(header)
            f.write(words.tobytes())
        return path

    @classmethod
    def load(cls, path) -> "VRVQFile":
        """Reads and validates a `.vrvq` file on the host; the words stay a host tensor until
        decompress moves them. RuntimeError: bad magic or version, a payload that is not exactly
        4 * sum(row_words) bytes, header fields out of range."""
        with open(path, "rb") as f:
            blob = f.read()
        if len(blob) < 12 or blob[:6] != BITSTREAM_MAGIC:
            raise RuntimeError(f"{path}: not a .vrvq container (bad magic)")
        if blob[6:8] != b"%02d" % BITSTREAM_VERSION:
            raise RuntimeError(f"{path}: unsupported .vrvq format version {blob[6:8]!r}")
        hlen = int(np.frombuffer(blob[8:12], "<u4")[0])
        if hlen % 4 or 12 + hlen > len(blob):
            raise RuntimeError(f"{path}: truncated .vrvq header")
        try:
            h = json.loads(blob[12:12 + hlen].decode("utf-8"))
            rw = h["row_words"]
            ints = {k: h[k] for k in ("n_codebooks", "codebook_size", "frames", "count_bits",
                                       "code_bits", "chunk_length", "original_length", "channels",
                                       "sample_rate")}
            if (h.get("version") != BITSTREAM_VERSION or not isinstance(rw, list)
                    or any(type(v) is not int for v in list(ints.values()) + rw)
                    or not isinstance(h["padding"], bool)):
                raise ValueError("field types")
            _check_stream_fields(ints["n_codebooks"], ints["codebook_size"], ints["frames"],
                                 ints["count_bits"], ints["code_bits"], "header")
            nq, T, cb, w = (ints[k] for k in ("n_codebooks", "frames", "count_bits", "code_bits"))
            lo = _words_of(T * cb)
            if not 0 < len(rw) <= MAX_ROWS or any(
                    not lo <= v <= lo + _words_of(w * nq * T) for v in rw):
                raise ValueError("row_words out of range")
            if (ints["chunk_length"] <= 0 or T % ints["chunk_length"] or ints["channels"] <= 0
                    or len(rw) % ints["channels"] or ints["sample_rate"] <= 0
                    or ints["original_length"] < 0):
                raise ValueError("metadata out of range")
            input_db = np.asarray([float(v) for v in h["input_db"]], np.float32)
            if input_db.size == 0 or len(rw) % input_db.size:
                raise ValueError("input_db does not match the rows")
            level, kbps = h.get("level"), h.get("target_kbps")
            max_kbps, packet_frames = h.get("max_kbps"), h.get("packet_frames")
            if packet_frames is not None and (type(packet_frames) is not int
                                              or packet_frames < 1):
                raise ValueError("packet_frames out of range")
        except (KeyError, TypeError, ValueError, UnicodeDecodeError) as e:
            raise RuntimeError(f"{path}: bad .vrvq header ({e})") from None
        payload = len(blob) - 12 - hlen
        if payload != 4 * sum(rw):
            raise RuntimeError(f"{path}: payload is {payload} bytes, row_words say {4 * sum(rw)}")
        words = np.frombuffer(blob, "<u4", offset=12 + hlen).astype(np.uint32).view(np.int32)
        # the bit accounting needs the counts: read plane A here (unpacking validates them)
        n_codes, off = 0, 0
        for n in rw:
            n_codes += int(_words_to_fields(words[off:off + lo].view(np.uint32), cb, T).sum()) \
                if cb else nq * T
            off += n
        count_total = len(rw) * T * cb
        bs = Bitstream(words=torch.from_numpy(words.copy()), row_words=tuple(rw), n_codebooks=nq,
                       codebook_size=ints["codebook_size"], frames=T, count_bits=cb, code_bits=w,
                       code_bits_total=w * n_codes, count_bits_total=count_total,
                       padding_bits=32 * sum(rw) - w * n_codes - count_total)
        return cls(bitstream=bs, chunk_length=ints["chunk_length"],
                   original_length=ints["original_length"], input_db=torch.from_numpy(input_db),
                   channels=ints["channels"], sample_rate=ints["sample_rate"],
                   padding=h["padding"], level=level, target_kbps=kbps, max_kbps=max_kbps,
                   packet_frames=packet_frames)

    def frame_counts(self) -> np.ndarray:
        """Codes kept per frame, (rows, frames) int64, read from the count planes on the host
        (a stream without a count plane keeps n_codebooks everywhere)."""
        bs = self.bitstream
        if not bs.count_bits:
            return np.full((bs.rows, bs.frames), bs.n_codebooks, np.int64)
        words = bs.words.detach().cpu().numpy().view(np.uint32)
        lo, off, out = _words_of(bs.frames * bs.count_bits), 0, []
        for n in bs.row_words:
            out.append(_words_to_fields(words[off:off + lo], bs.count_bits, bs.frames))
            off += int(n)
        return np.stack(out)

    def packet_kbps(self, model_sample_rate: int, hop_length: int,
                    packet_frames: Optional[int] = None) -> np.ndarray:
        """The realised rate of every packet, (rows, packets) float64 in kbps: its count fields
        plus its kept codes (no padding) over its own frames, at the frame rate
        floor(model_sample_rate / hop_length) of kbps_to_budget. Packets are runs of
        packet_frames frames that restart at every chunk_length, the last of a chunk may be
        short (default: the file's packet_frames, else chunk_length: one packet per window). Its
        maximum is the peak rate of the file at that packet length; a file that
        compress(max_kbps=...) wrote has none above max_kbps at its own packet_frames."""
        bs = self.bitstream
        cl = int(self.chunk_length)
        P = int(packet_frames if packet_frames is not None else self.packet_frames or cl)
        if P < 1:
            raise ValueError("packet_kbps: packet_frames must be >= 1")
        counts = self.frame_counts().reshape(bs.rows, bs.frames // cl, cl)
        starts = np.arange(0, cl, P)
        n_f = np.minimum(P, cl - starts)                      # frames of each packet of a chunk
        bits = np.add.reduceat(counts, starts, axis=2) * bs.code_bits + n_f * bs.count_bits
        rate = int(model_sample_rate) // int(hop_length)
        return (bits / n_f * rate / 1000.0).reshape(bs.rows, -1)

    def payload_kbps(self, model_sample_rate: int, hop_length: int) -> float:
        """The stream's rate on disk: 32 * sum(row_words) bits over the duration of its
        rows x frames frames at the frame rate floor(model_sample_rate / hop_length) that
        kbps_to_budget uses (rows are pooled, as compress(target_kbps=...) pools them)."""
        bs = self.bitstream
        rate = int(model_sample_rate) // int(hop_length)
        return bs.total_bits * rate / (bs.rows * bs.frames) / 1000.0

    def marker_codes(self, device=None) -> torch.Tensor:
        """The DACFile form of the codes, (rows, Nq, frames) int64 with codebook_size where a
        code is masked out, unpacked on `device` (default: where the words are)."""
        bs = self.bitstream if device is None else self.bitstream.to(device)
        codes, mask = unpack_bitstream(bs)
        if bs.count_bits:
            codes = codes.masked_fill(mask == 0, bs.codebook_size)
        return codes

    def to_dac(self) -> DACFile:
        return DACFile(codes=self.marker_codes().cpu(), chunk_length=self.chunk_length,
                       original_length=self.original_length, input_db=self.input_db,
                       channels=self.channels, sample_rate=self.sample_rate,
                       padding=self.padding, dac_version=SUPPORTED_VERSIONS[-1])

    @classmethod
    def from_dac(cls, dac: DACFile, codebook_size: int) -> "VRVQFile":
        """A DACFile whose masked-out codes are the marker `codebook_size` (none: a fixed-count
        stream) as a VRVQFile. to_dac() gives the same codes back."""
        codes = dac.codes.to(torch.int64)
        keep = codes != int(codebook_size)
        mask = None if bool(keep.all()) else keep.to(torch.float32)
        bs = pack_bitstream(torch.where(keep, codes, torch.zeros_like(codes)), mask,
                            int(codebook_size))
        return cls(bitstream=bs, chunk_length=dac.chunk_length,
                   original_length=dac.original_length, input_db=dac.input_db,
                   channels=dac.channels, sample_rate=dac.sample_rate, padding=dac.padding)


def is_vrvq_file(path) -> bool:
    """True where the file starts with the `.vrvq` magic (whatever its version)."""
    with open(path, "rb") as f:
        return f.read(6) == BITSTREAM_MAGIC
