"""Reference packer of "VRVQ bitstream 1" in plain NumPy arrays and Python ints, field by field.

The format (include/vrvq.h "Bitstream"): a stream is little-endian uint32 words; a field of width
n at bit position p puts bit j of its value at stream bit p + j; stream bit q is bit q & 31 of
word q >> 5. A code takes w = max(1, ceil(log2(codebook_size))) bits, a count
cb = Nq.bit_length() bits (0 for a fixed-count stream, which has no plane A). Row r is plane A
(T counts, t ascending, zero-padded to a word) then plane B (for t ascending, i < c_t:
codes[r, i, t]; zero-padded to a word); rows are concatenated.

This is the oracle of the byte comparisons in tests/test_bitstream.py and
tests/test_gpu_bitstream.py. It does not import the package under test."""
import numpy as np


def code_bits(codebook_size: int) -> int:
    w = 1
    while (1 << w) < codebook_size:
        w += 1
    return w


def count_bits(n_codebooks: int) -> int:
    return int(n_codebooks).bit_length()


class _Plane:
    """Fields appended at ascending bit positions, as one Python int."""

    def __init__(self):
        self.value, self.bits = 0, 0

    def put(self, v: int, n: int):
        assert 0 <= v < (1 << n) or n == 0
        self.value |= v << self.bits
        self.bits += n

    def words(self):
        n = (self.bits + 31) // 32
        return [(self.value >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


def pack(codes: np.ndarray, mask, codebook_size: int):
    """codes (R, Nq, T) ints, mask (R, Nq, T) of 0 / 1 (prefix-shaped along Nq) or None (every
    stage kept, cb = 0) -> (words uint32 (sum row_words,), row_words list, info dict)."""
    R, nq, T = codes.shape
    w = code_bits(codebook_size)
    cb = 0 if mask is None else count_bits(nq)
    words, row_words, n_codes = [], [], 0
    for r in range(R):
        a, b = _Plane(), _Plane()
        for t in range(T):
            if mask is None:
                c = nq
            else:
                col = [int(mask[r, i, t] != 0) for i in range(nq)]
                c = sum(col)
                if col != [1] * c + [0] * (nq - c):
                    raise ValueError("mask is not prefix-shaped")
                a.put(c, cb)
            for i in range(c):
                v = int(codes[r, i, t])
                if not 0 <= v < codebook_size:
                    raise IndexError("code out of range")
                b.put(v, w)
            n_codes += c
        row = a.words() + b.words()
        assert len(row) == (T * cb + 31) // 32 + (b.bits + 31) // 32
        words += row
        row_words.append(len(row))
    info = dict(count_bits=cb, code_bits=w, code_bits_total=w * n_codes,
                count_bits_total=R * T * cb)
    info["padding_bits"] = 32 * len(words) - info["code_bits_total"] - info["count_bits_total"]
    return np.array(words, dtype=np.uint32), row_words, info


def _get(words, base: int, p: int, n: int) -> int:
    """The n-bit field at bit p of the words starting at word `base`."""
    v = 0
    for j in range(n):
        q = p + j
        v |= ((int(words[base + (q >> 5)]) >> (q & 31)) & 1) << j
    return v


def unpack(words, row_words, n_codebooks: int, codebook_size: int, frames: int, cb: int):
    """-> codes (R, Nq, T) int64 (0 where masked), mask (R, Nq, T) float32."""
    nq, T, w = n_codebooks, frames, code_bits(codebook_size)
    R = len(row_words)
    if sum(row_words) != len(words):
        raise ValueError("stream length disagrees with row_words")
    codes = np.zeros((R, nq, T), np.int64)
    mask = np.zeros((R, nq, T), np.float32)
    base = 0
    for r in range(R):
        a_words = (T * cb + 31) // 32
        if row_words[r] < a_words:
            raise ValueError("row shorter than its count plane")
        counts = [_get(words, base, t * cb, cb) if cb else nq for t in range(T)]
        if max(counts) > nq:
            raise ValueError("count above n_codebooks")
        if a_words + (w * sum(counts) + 31) // 32 != row_words[r]:
            raise ValueError("row_words disagrees with the counts")
        p = 0
        for t in range(T):
            for i in range(counts[t]):
                v = _get(words, base + a_words, p, w)
                if v >= codebook_size:
                    raise IndexError("code out of range")
                codes[r, i, t], mask[r, i, t] = v, 1.0
                p += w
        base += row_words[r]
    return codes, mask
