"""Times of the HIP loudness measurement against the host path it replaces
(profiles/loudness.json; DESIGN.md §4 "Loudness").

Two shapes -- 2 x 10 min stereo at 44.1 kHz (a file as compress sees it) and 32 x 1 s mono (a
training batch as VolumeNorm sees it) -- each measured two ways on the same machine in the same
run, alternating:

  device  vrvq_amd.loudness on the GPU tensor: four launches, nothing leaves the device. Timed
          between HIP events around windows of back-to-back calls.
  host    codec.loudness on the same GPU tensor, as compress and decompress called it before: the
          float64 copy to the host, two scipy.signal.lfilter passes, the cumulative sum. Timed by
          the host clock; the call ends in the copy's synchronise and host work.

and reports both times, their ratio (device / host: below 1 means the device path is faster),
the largest difference between the two float32 results, and the device path's achieved rate from
the bytes the algorithm needs: 2 reads of x (4 bytes a sample each; the chunk states and partial
sums it writes and reads back are about 2 % of that). It is a whole-call rate (four launches and
the Python around them included), not a kernel's share of peak.

Then model.compress on the first shape, as it is and with the measurement done as before (the
host path, twice: once for input_db and once more inside normalize), host clock around a call that
ends in the codes' copy to the host.

Needs an MI355X; there is no CPU path. Usage: python tools/loudness_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrvq_amd  # noqa: E402
from vrvq_amd import _lib, codec, metering  # noqa: E402
from vrvq_amd.recipe import load_recipe  # noqa: E402

SR = 44100
# name, items, channels, samples, device calls per window, host calls per repeat
SHAPES = (("2 x 10 min stereo 44.1 kHz", 2, 2, 600 * SR, 10, 1),
          ("32 x 1 s mono 44.1 kHz", 32, 1, SR, 200, 5))
KW = dict(encoder_dim=64, encoder_rates=[2, 4, 8, 8], decoder_dim=1536,
          decoder_rates=[8, 8, 4, 2], n_codebooks=8, codebook_size=1024, codebook_dim=8,
          quantizer_dropout=1.0, sample_rate=SR)


def signal(items, nch, n, dev):
    g = torch.Generator().manual_seed(items * 1000 + n % 997)
    t = torch.arange(n, dtype=torch.float64) / SR
    tone = (0.3 * torch.sin(2 * torch.pi * 220 * t)).to(torch.float32)
    return (tone + 0.05 * torch.randn(items, nch, n, generator=g)).to(dev)


def window_ms(fn, calls: int):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def host_ms(fn, calls: int):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5),
            "max_ms": round(max(xs), 5), "windows": len(xs)}


def case(name, items, nch, n, d_calls, h_calls, dev, repeats):
    x = signal(items, nch, n, dev)
    plan = _lib.loudness_plan(SR, nch, n)

    def device():
        return vrvq_amd.loudness(x, SR)

    def host():
        return codec.loudness(x, SR)

    for _ in range(3):
        got = device()
    want = host()
    torch.cuda.synchronize()
    res = {"shape": name, "items": items, "channels": nch, "samples": n,
           "chunks_per_row": plan["chunks"], "blocks": plan["blocks"],
           "workspace_bytes": items * plan["ws_bytes"],
           "max_abs_diff_float32": float((got.cpu() - want).abs().max()),
           "float32_bits_equal": bool(torch.equal(got.cpu(), want))}
    d_ms, h_ms = [], []
    for _ in range(repeats):  # alternate the two so that drift hits both
        d_ms.append(window_ms(device, d_calls))
        h_ms.append(host_ms(host, h_calls))
    dm = statistics.median(d_ms)
    nbytes = 2 * 4 * items * nch * n
    res["device"] = dict(stats(d_ms), calls_per_window=d_calls)
    res["host"] = dict(stats(h_ms), calls_per_window=h_calls)
    res["ratio_device_over_host"] = round(dm / statistics.median(h_ms), 6)
    res.update(bytes=nbytes, device_gb_per_s=round(nbytes / (dm * 1e-3) / 1e9, 1),
               audio_seconds_per_second=round(items * n / SR / (dm * 1e-3), 1))
    return res


def compress_case(name, items, nch, n, dev, repeats):
    model = vrvq_amd.DAC_VRVQ(**KW)
    load_recipe(model, seed=0)
    model = model.to(dev).eval()
    x = signal(items, nch, n, dev)
    device_measure = metering.loudness

    def as_before(audio, sample_rate):
        """What _compress did before: codec.loudness for input_db, then once more in normalize."""
        codec.loudness(audio, sample_rate)
        return codec.loudness(audio, sample_rate).to(audio.device)

    def run(measure):
        metering.loudness = measure
        try:
            return model.compress(x, win_duration=1.0, max_batch=64)
        finally:
            metering.loudness = device_measure

    a = run(device_measure)
    b = run(as_before)
    res = {"shape": name, "codes_equal": bool(torch.equal(a.codes, b.codes)),
           "input_db_equal": bool(torch.equal(a.input_db, b.input_db))}
    now, before = [], []
    for _ in range(repeats):
        now.append(host_ms(lambda: run(device_measure), 1))
        before.append(host_ms(lambda: run(as_before), 1))
    res["compress_device_loudness"] = stats(now)
    res["compress_host_loudness_twice"] = stats(before)
    res["ratio_now_over_before"] = round(statistics.median(now) / statistics.median(before), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-compress", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "clock": "device path: HIP events around windows of back-to-back calls; host path and "
                    "compress: host clock around calls that end synchronised; alternating",
           "cases": []}
    for shape in SHAPES:
        res["cases"].append(case(*shape, dev, args.repeats))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    if not args.skip_compress:
        name, items, nch, n = SHAPES[0][:4]
        res["compress"] = compress_case(name, items, nch, n, dev, max(2, args.repeats - 1))
        print(json.dumps(res["compress"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
