"""Forward + backward times of the fused spectral losses against the torch composition of
vrvq_amd/losses.py (profiles/spectral_grad.json; DESIGN.md "Spectral distance").

  loss cases   MelSpectrogramLoss (conf/base.yml's 7 scales) and MultiScaleSTFTLoss (2048, 512) at
               32 x 44,100 and 12 x 441,000: loss(x, y).backward() with fused=True and fused=False
               on the same GPU in the same run, in alternating windows of back-to-back calls
               between HIP events after warm-up; the median of the windows, the ratio fused / torch
               of every window pair, and the peak allocator bytes of one forward + backward.
               Each case runs on two kinds of input: "white" (noise with a flat spectrum, the
               estimate a noisy copy) and "coloured" (Brownian noise, -6 dB per octave, the
               estimate the reference plus 1 % white noise: the roll-off of speech and music,
               where most bins lie far under their frame's level). The gradient kernel's fp64
               pass over isolated small bins depends on that, so both are reported.
  train_step   trainer.train_step at bench.py --train's shape (vrvq_a2, 32 x 16,758) with
               fused_losses off and on, alternating.

Needs an MI355X; there is no CPU path. Usage: python tools/spectral_grad_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrvq_amd  # noqa: E402
from vrvq_amd import losses  # noqa: E402

LOSSES = {"mel_base_yml_7_scales": losses.MelSpectrogramLoss,
          "stft_2048_512": losses.MultiScaleSTFTLoss}
SHAPES = ((32, 44100), (12, 441000))


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


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def signals(kind: str, R: int, T: int, dev):
    g = torch.Generator().manual_seed(R * 1000 + T % 997)
    if kind == "white":
        y = (0.3 * torch.randn(R, 1, T, generator=g) + 0.05).to(dev)
        x = 0.7 * y + 0.01 * torch.randn(R, 1, T, generator=g).to(dev)
    else:  # Brownian: the running sum of white noise, scaled to 0.3 rms
        y = torch.cumsum(torch.randn(R, 1, T, generator=g, dtype=torch.float64), -1)
        y = y - y.mean(-1, keepdim=True)
        y = (0.3 * y / y.std(-1, keepdim=True)).float().to(dev)
        x = y + 0.003 * torch.randn(R, 1, T, generator=g).to(dev)
    return x.contiguous().requires_grad_(), y


def loss_case(name: str, kind: str, R: int, T: int, dev, repeats: int):
    x, y = signals(kind, R, T, dev)
    mods = {flag: LOSSES[name](fused=flag) for flag in (True, False)}

    def step(flag):
        def run():
            x.grad = None
            mods[flag](x, y).backward()
        return run

    fused, composed = step(True), step(False)
    calls = {True: 20 if T < 100000 else 5, False: 5 if T < 100000 else 2}
    for fn, n in ((fused, 10), (composed, 3)):  # warm both at this shape
        for _ in range(n):
            fn()
    torch.cuda.synchronize()
    f_ms, t_ms = [], []
    for _ in range(repeats):  # alternate the two so that drift hits both
        f_ms.append(window_ms(fused, calls[True]))
        t_ms.append(window_ms(composed, calls[False]))
    ratios = [f / t for f, t in zip(f_ms, t_ms)]
    return {"loss": name, "input": kind, "rows": R, "samples": T,
            "fused_fwd_bwd": dict(stats(f_ms), calls_per_window=calls[True]),
            "torch_fwd_bwd": dict(stats(t_ms), calls_per_window=calls[False]),
            "ratio_fused_over_torch": round(statistics.median(f_ms) / statistics.median(t_ms), 4),
            "ratio_per_window": [round(r, 4) for r in ratios],
            "ratio_below_1_in_every_window": all(r < 1.0 for r in ratios),
            "peak_bytes_fused": peak_bytes(fused), "peak_bytes_torch": peak_bytes(composed)}


def train_case(dev, repeats: int, batch: int = 32, clip: int = 16758):
    from vrvq_amd.config import A2_KWARGS
    from vrvq_amd.recipe import load_recipe, synthetic_audio
    from vrvq_amd.trainer import LAMBDAS_A2, build_state, train_step
    audio = torch.from_numpy(synthetic_audio(batch, clip, seed=1234)).to(dev)
    states = {}
    for flag in (False, True):
        model = vrvq_amd.DAC_VRVQ(**A2_KWARGS)
        load_recipe(model, seed=0)
        torch.manual_seed(0)
        states[flag] = build_state(model, dev, fused_losses=flag)
    steps = {flag: (lambda s=states[flag]: train_step(s, audio, LAMBDAS_A2)) for flag in states}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(repeats):
        for flag in (False, True):
            ms[flag].append(window_ms(steps[flag], 3))
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {"batch": batch, "samples": clip, "torch_losses": stats(ms[False]),
            "fused_losses": stats(ms[True]), "difference_ms": round(on - off, 4),
            "ratio_fused_over_torch": round(on / off, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_grad_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "clock": "HIP events around windows of back-to-back calls, alternating, after warm-up",
           "loss_cases": [loss_case(name, kind, R, T, dev, args.repeats)
                          for kind in ("white", "coloured") for R, T in SHAPES
                          for name in LOSSES]}
    if not args.no_train:
        res["train_step"] = train_case(dev, args.repeats)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
