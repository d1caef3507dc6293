"""Times and sizes of the bit-granular VBR stream (profiles/bitstream.json; DESIGN.md
"Bitstream").

  times      at 2 rows x 51,680 frames (a 10-minute stereo file) and 64 rows x 87 frames, Nq = 9,
             1024 entries, masks = generate_mask_hard of uniform scores; HIP events around runs of
             launches, medians:
               a  bitpack_plan + bitpack_write            (new)
               b  bitunpack_plan + bitunpack_read         (new)
               c  pack_counts + pack_codes                (the byte-granular packer)
               d  unpack_offsets + unpack_codes
               e  what compress does to build a DACFile: masked_fill + the int64 .cpu() copy
                  (host clock: the copy ends in a sync)
             The data-dependent length is read once before the timed runs, so a .. d are the
             launches alone.
  sizes      one compress of a 10-s synthetic signal at three levels: bytes of the .dac, the
             .vrvq.npz and the .vrvq file beside bpf * frames / 8

Needs an MI355X; there is no CPU path. Usage: python tools/bitstream_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrvq_amd  # noqa: E402
from vrvq_amd import codes_io, ops, utils  # noqa: E402

NQ, NCODE = 9, 1024


def event_ms(fn, calls: int, repeats: int, warmup: int):
    """Per-call milliseconds of fn over `repeats` windows of `calls` back-to-back calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5),
            "max_ms": round(max(xs), 5), "windows": len(xs)}


def time_case(R: int, T: int, dev, calls: int):
    g = torch.Generator().manual_seed(R * 100003 + T)
    codes = torch.randint(0, NCODE, (R, NQ, T), generator=g).to(dev)
    scores = (torch.rand(R, 1, T, generator=g) * (NQ + 1) - 0.5).to(dev)
    mask = utils.generate_mask_hard(scores, NQ)
    vr = ops.load_ops()
    cb = codes_io.count_bits_of(NQ)

    # the lengths, read once
    bs = codes_io.pack_bitstream(codes, mask, NCODE)
    total_words = sum(bs.row_words)
    row_off = torch.tensor([0] + list(bs.row_words), dtype=torch.int64).cumsum(0).to(dev)
    packed, counts = codes_io.pack_codes(codes, mask, NCODE)
    total_codes = packed.numel()
    c2, m2 = codes_io.unpack_bitstream(bs)
    assert torch.equal(m2, mask) and torch.equal(c2, codes * mask.long())
    assert bs.code_bits_total == 10 * total_codes

    def a():
        cn, co, info = vr.bitpack_plan(codes, mask, NCODE)
        return vr.bitpack_write(codes, cn, co, info, total_words, NCODE, cb)

    def b():
        cn, co, fl = vr.bitunpack_plan(bs.words, row_off, NQ, T, NCODE, cb)
        return vr.bitunpack_read(bs.words, cn, co, row_off, fl, NQ, NCODE, cb)

    def c():
        cn, off, _ = vr.pack_counts(mask)
        return vr.pack_codes(codes, cn, off, total_codes, NCODE)

    def d():
        return vr.unpack_codes(packed, counts, vr.unpack_offsets(counts), NQ)

    def e():
        return codes.masked_fill(mask == 0, NCODE).cpu()

    res = {}
    for _ in range(3):  # alternate so that drift hits all of them
        for name, fn in (("a_bitpack", a), ("b_bitunpack", b), ("c_pack_codes", c),
                         ("d_unpack_codes", d)):
            res.setdefault(name, []).extend(event_ms(fn, calls=calls, repeats=3, warmup=10))
    e()
    host = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e()
        host.append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in res.items()}
    return {"rows": R, "frames": T, "nq": NQ, "codebook_size": NCODE,
            "stream_bytes": 4 * total_words, "packed_uint16_bytes": 2 * total_codes + R * T,
            "dac_uint16_bytes": 2 * R * NQ * T,
            **{k: stats(v) for k, v in res.items()},
            "e_masked_fill_cpu_copy": stats(host),
            "pack_ratio_a_over_c": round(med["a_bitpack"] / med["c_pack_codes"], 3),
            "unpack_ratio_b_over_d": round(med["b_bitunpack"] / med["d_unpack_codes"], 3)}


def size_case(dev, levels):
    from vrvq_amd.config import A2_KWARGS
    from vrvq_amd.recipe import load_recipe, synthetic_audio
    model = vrvq_amd.DAC_VRVQ(**A2_KWARGS)
    load_recipe(model, 0)
    model = model.to(dev).eval()
    audio = torch.from_numpy(synthetic_audio(1, 10 * model.sample_rate, seed=3))
    rows = []
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for level in levels:
            dac = model.compress(audio, level=level)
            vf = model.compress(audio, level=level, container="vrvq")
            assert torch.equal(vf.to_dac().codes, dac.codes)
            codes, mask = codes_io.unpack_bitstream(vf.bitstream.to(dev))
            packed, counts = codes_io.pack_codes(codes, mask, model.codebook_size)
            npz = codes_io.save_packed(os.path.join(tmp, "x"), packed, counts, model.n_codebooks)
            bs = vf.bitstream
            frames = bs.rows * bs.frames
            rows.append({
                "level": level, "frames": frames,
                "bpf": round(bs.code_bits_total / frames, 4),
                "bpf_frames_over_8_bytes": bs.code_bits_total / 8,
                "dac_bytes": os.path.getsize(dac.save(os.path.join(tmp, "x"))),
                "vrvq_npz_bytes": os.path.getsize(npz),
                "vrvq_bytes": os.path.getsize(vf.save(os.path.join(tmp, "x"))),
                "vrvq_payload_bytes": 4 * sum(bs.row_words),
                "count_plane_bytes": bs.count_bits_total / 8,
                "payload_kbps": round(vf.payload_kbps(model.sample_rate, model.hop_length), 4)})
    utils.check_errors(dev)
    return {"seconds": 10, "n_codebooks": model.n_codebooks,
            "codebook_size": model.codebook_size, "levels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--levels", type=float, nargs=3, default=[0.5, 1.0, 3.0])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bitstream_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "chunk_frames": codes_io.BITSTREAM_CHUNK_FRAMES,
           "times": [time_case(2, 51680, dev, calls=50), time_case(64, 87, dev, calls=100)],
           "sizes": size_case(dev, args.levels)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
