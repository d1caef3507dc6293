"""Times of the HIP resampler against the torch composition julius runs
(profiles/resample.json; DESIGN.md §4 "Resampling").

Four shapes -- 2 x 10 min at 48 -> 44.1 kHz, 44.1 -> 48 kHz and 16 -> 44.1 kHz, and 32 x 1 s at
44.1 -> 22.05 kHz (the scale discriminator's) -- each measured two ways on the same GPU in the
same run, in alternating windows of back-to-back calls between HIP events:

  kernel  vrvq_amd.resample: one launch, the kept taps of every phase
  torch   julius.resample_frac's composition: F.pad(replicate) by (W, W + old), F.conv1d of the
          (new, 1, K) kernel with stride old, transpose, reshape, crop -- all K = 2 W + old taps

and reports both times, their ratio (kernel / torch: below 1 means the kernel is faster), the
largest difference between the two results, and the kernel's achieved rates from the bytes and
operations the algorithm needs: bytes = 4 (rows L + rows n_out) (x read once, y written once; the
tap table is a few tens of KB), FLOPs = 2 ntaps rows n_out. Both are whole-call rates (the launch
and the Python around it included), not a kernel's share of peak.

Needs an MI355X; there is no CPU path. Usage: python tools/resample_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrvq_amd  # noqa: E402
from vrvq_amd import _lib  # noqa: E402

# name, rows, samples, old_sr, new_sr
SHAPES = (("2 x 10 min 48 -> 44.1 kHz", 2, 600 * 48000, 48000, 44100),
          ("2 x 10 min 44.1 -> 48 kHz", 2, 600 * 44100, 44100, 48000),
          ("2 x 10 min 16 -> 44.1 kHz", 2, 600 * 16000, 16000, 44100),
          ("32 x 1 s 44.1 -> 22.05 kHz (MSD)", 32, 44100, 44100, 22050))


def window_ms(fn, calls: int):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5),
            "max_ms": round(max(xs), 5), "windows": len(xs)}


def dense_kernel(old: int, new: int, W: int, zeros: int = 24, rolloff: float = 0.945):
    """julius' (new, 1, K) conv kernel: every tap of every phase, fp64 rounded to fp32."""
    sr = min(old, new) * rolloff
    i = np.arange(new, dtype=np.float64)[:, None]
    j = np.arange(2 * W + old, dtype=np.float64)[None, :]
    t = np.clip((-i / new + (j - W) / old) * sr, -zeros, zeros) * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t) * np.cos(t / zeros / 2) ** 2
    k /= k.sum(axis=1, keepdims=True)
    return torch.from_numpy(k.astype(np.float32))[:, None, :]


def case(name, rows, L, old_sr, new_sr, dev, repeats):
    plan = _lib.resample_plan(old_sr, new_sr, length=L)
    old, new, W, n_out = plan["old"], plan["new"], plan["W"], plan["out_length"]
    g = torch.Generator().manual_seed(rows * 1000 + L % 997)
    x = (0.3 * torch.randn(rows, L, generator=g) + 0.05).to(dev)
    kern = dense_kernel(old, new, W).to(dev)

    def kernel():
        return vrvq_amd.resample(x, old_sr, new_sr)

    def composed():
        xp = F.pad(x[:, None], (W, W + old), mode="replicate")
        ys = F.conv1d(xp, kern, stride=old)                       # (rows, new, frames)
        return ys.transpose(1, 2).reshape(rows, -1)[..., :n_out]

    res = {"shape": name, "rows": rows, "samples": L, "ratio": f"{old}:{new}",
           "out_samples": n_out, "ntaps": plan["ntaps"], "K": plan["K"]}
    k_calls = 20
    for _ in range(5):
        got = kernel()
    torch.cuda.synchronize()
    try:
        t_calls = 2
        for _ in range(2):
            want = composed()
        torch.cuda.synchronize()
        res["max_abs_diff_kernel_vs_torch"] = float((got - want).abs().max())
        del want
    except RuntimeError as e:  # the library convolution may refuse the shape
        composed = None
        res["torch_composition"] = {"failed": str(e).splitlines()[0][:200]}
    del got
    k_ms, t_ms = [], []
    for _ in range(repeats):  # alternate the two so that drift hits both
        k_ms.append(window_ms(kernel, k_calls))
        if composed is not None:
            t_ms.append(window_ms(composed, t_calls))
    km = statistics.median(k_ms)
    nbytes = 4 * (rows * L + rows * n_out)
    flops = 2 * plan["ntaps"] * rows * n_out
    res["kernel"] = dict(stats(k_ms), calls_per_window=k_calls)
    if t_ms:
        res["torch_composition"] = dict(stats(t_ms), calls_per_window=t_calls)
        res["ratio_kernel_over_torch"] = round(km / statistics.median(t_ms), 4)
    res.update(bytes=nbytes, flops=flops,
               kernel_gb_per_s=round(nbytes / (km * 1e-3) / 1e9, 1),
               kernel_gflop_per_s=round(flops / (km * 1e-3) / 1e9, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "clock": "HIP events around windows of back-to-back calls, alternating",
           "cases": []}
    for shape in SHAPES:
        res["cases"].append(case(*shape, dev, args.repeats))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
