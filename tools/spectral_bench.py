"""Times of the fused spectral distances against the torch composition they restate
(profiles/spectral_metrics.json; DESIGN.md "Spectral distance").

Two configurations, mel_distance (n_mels (150, 80), windows (2048, 512), pow 2, log + magnitude
terms) and the seven scales of conf/base.yml (n_mels 5..320, windows 32..2048, pow 1, log term
only), at two shapes, 12 x 441,000 samples (the reference driver's sweep: 12 levels of a 10 s clip)
and 32 x 44,100, each measured two ways on the same GPU in the same run, in alternating windows of
back-to-back calls between HIP events:

  fused   utils.spectral_distance: one launch per scale plus one, per-row results
  torch   the per-row composition of vrvq_amd/losses.py: mel_spectrogram (torch.stft, abs, the
          dense mel product) of both signals, clamp / pow / log10, a mean over each row, fp32

and reports both times, their ratio (fused / torch: below 1 means the fused path is faster) and
the rate of sample reads of the fused path: every scale's launch reads both signals once, so
bytes = scales x 2 x rows x samples x 4 over the fused time. That is an end-to-end rate of the
whole call (all launches and the Python around them), not a kernel's share of peak.

Needs an MI355X; there is no CPU path. Usage: python tools/spectral_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vrvq_amd import losses, utils  # noqa: E402

CONFIGS = {
    "mel_distance": dict(utils.MEL_DISTANCE),
    "base_yml_7_scales": dict(windows=(32, 64, 128, 256, 512, 1024, 2048),
                              n_mels=(5, 10, 20, 40, 80, 160, 320), clamp_eps=1e-5, pow=1.0,
                              log_weight=1.0, mag_weight=0.0),
}
SHAPES = ((12, 441000), (32, 44100))


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


def torch_rows(est, ref, cfg):
    """The distance of every row in torch ops, as losses.MelSpectrogramLoss forms it but with a
    mean per row: (R,) float32."""
    total = 0.0
    for w, m in zip(cfg["windows"], cfg["n_mels"]):
        xm = losses.mel_spectrogram(est, 44100, m, w, w // 4)
        ym = losses.mel_spectrogram(ref, 44100, m, w, w // 4)
        total = total + cfg["log_weight"] * (
            xm.clamp(cfg["clamp_eps"]).pow(cfg["pow"]).log10()
            - ym.clamp(cfg["clamp_eps"]).pow(cfg["pow"]).log10()).abs().mean(dim=(1, 2, 3))
        if cfg["mag_weight"]:
            total = total + cfg["mag_weight"] * (xm - ym).abs().mean(dim=(1, 2, 3))
    return total


def case(name: str, cfg: dict, R: int, T: int, dev, repeats: int):
    g = torch.Generator().manual_seed(R * 1000 + T % 997)
    ref = (0.3 * torch.randn(R, 1, T, generator=g) + 0.05).to(dev)
    est = (0.7 * ref + 0.01 * torch.randn(R, 1, T, generator=g).to(dev)).contiguous()

    def fused():
        return utils.spectral_distance(est, ref, **cfg)["distance"]

    def composed():
        return torch_rows(est, ref, cfg)

    got, want = fused().reshape(-1).cpu(), composed().double().cpu()
    for fn, n in ((fused, 20), (composed, 5)):  # warm both at this shape
        for _ in range(n):
            fn()
    torch.cuda.synchronize()
    f_calls = 50
    t_calls = 10
    f_ms, t_ms = [], []
    for _ in range(repeats):  # alternate the two so that drift hits both
        f_ms.append(window_ms(fused, f_calls))
        t_ms.append(window_ms(composed, t_calls))
    S = len(cfg["windows"])
    read = S * 2 * R * T * 4
    fm, tm = statistics.median(f_ms), statistics.median(t_ms)
    return {"configuration": name, "rows": R, "samples": T, "scales": S,
            "launches_fused": S + 1,
            "max_rel_diff_fused_vs_torch": float(((got - want).abs() / want.abs()).max()),
            "fused": dict(stats(f_ms), calls_per_window=f_calls),
            "torch_composition": dict(stats(t_ms), calls_per_window=t_calls),
            "ratio_fused_over_torch": round(fm / tm, 4),
            "sample_bytes_read": read,
            "fused_sample_read_gb_per_s": round(read / (fm * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spectral_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "clock": "HIP events around windows of back-to-back calls, alternating",
           "cases": [case(name, cfg, R, T, dev, args.repeats)
                     for R, T in SHAPES for name, cfg in CONFIGS.items()]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
