"""Times of the on-GPU BSS-eval SDR (profiles/bss_sdr.json; DESIGN.md "BSS SDR").

  bss_sdr       ops.bss_sdr at its defaults (three launches; HIP events around runs of calls)
  torch_fp64    the composition torchmetrics runs, in torch fp64 ops on the same GPU: torch.fft
                correlations of length 2^ceil(log2(2 T - 1)), the gathered 512 x 512 Toeplitz
                matrix per row, torch.linalg.solve
  launches      the split of bss_sdr between its three launches, by difference, through the
                C-ABI on one set of buffers: the correlation launch costs the same at
                filter_length 1 (every workgroup forms all 512 lags), the solve the same at one
                sample per row (F - 1 steps whatever the data), and both at once leave the three
                launches' overheads. Not exact: at filter_length 1 the reduction still walks its
                chunk chains for sum t^2, sum p^2 and lag 0 (three of the four a thread walks at
                512), so "correlation_ms" carries most of the reduction's latency and
                "reduction_ms_by_difference" is understated by as much; their sum is exact

at (L * B, T) = (12 * 1, 441000) (the reference driver's sweep), (1 * 32, 44100) and (1 * 1,
441000). The two sides are timed in alternating windows, so drift hits both.

Needs an MI355X; there is no CPU path. Usage: python tools/sdr_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vrvq_amd import _lib, ops  # noqa: E402

F = 512


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


def torch_composition(est: torch.Tensor, ref: torch.Tensor, filter_length: int = F):
    """signal_distortion_ratio (zero_mean False, no load_diag) of rows est (R, T) against rows
    r % B of ref (B, T), in torch fp64 ops."""
    R, T = est.shape
    p, t = est.to(torch.float64), ref.to(torch.float64).repeat(R // ref.shape[0], 1)
    t = t / torch.clamp(torch.linalg.norm(t, dim=-1, keepdim=True), min=1e-6)
    p = p / torch.clamp(torch.linalg.norm(p, dim=-1, keepdim=True), min=1e-6)
    n_fft = 2 ** math.ceil(math.log2(2 * T - 1))
    tf, pf = torch.fft.rfft(t, n=n_fft), torch.fft.rfft(p, n=n_fft)
    r = torch.fft.irfft(tf.real ** 2 + tf.imag ** 2, n=n_fft)[..., :filter_length]
    b = torch.fft.irfft(tf.conj() * pf, n=n_fft)[..., :filter_length]
    i = torch.arange(filter_length, device=est.device)
    mat = r[..., (i[:, None] - i[None, :]).abs()]
    sol = torch.linalg.solve(mat, b)
    coh = (b * sol).sum(-1)
    return 10 * torch.log10(coh / (1 - coh))


def launch_split(est, ref, R: int, B: int, T: int):
    n = ctypes.c_longlong(0)
    _lib.call("vrvq_bss_sdr_workspace", R, B, T, F, ctypes.byref(n))
    ws = torch.empty(n.value // 8, dtype=torch.float64, device=est.device)
    out = torch.empty(R, dtype=torch.float64, device=est.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    e, r = ctypes.c_void_p(est.data_ptr()), ctypes.c_void_p(ref.data_ptr())

    def call(samples, filter_length):
        _lib.call("vrvq_bss_sdr", e, r, R, B, samples, None, filter_length, 0, float("nan"),
                  ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), n.value, stream)

    full = statistics.median(event_ms(lambda: call(T, F), 20, 5, 5))
    corr = statistics.median(event_ms(lambda: call(T, 1), 20, 5, 5))
    solve = statistics.median(event_ms(lambda: call(1, F), 20, 5, 5))
    idle = statistics.median(event_ms(lambda: call(1, 1), 20, 5, 5))
    return {"all_three_ms": round(full, 5),
            "correlation_ms": round(corr - idle, 5), "solve_ms": round(solve - idle, 5),
            "reduction_ms_by_difference": round(full - corr - solve + idle, 5),
            "three_empty_launches_ms": round(idle, 5),
            "note": "correlation_ms includes the reduction's chains for the energies and lag 0; "
                    "reduction_ms_by_difference is understated by as much; their sum is exact"}


def case(L: int, B: int, T: int, dev):
    g = torch.Generator().manual_seed(L * 1000 + B)
    ref = (0.3 * torch.randn(B, T, generator=g)).to(dev)
    est = (0.7 * ref.repeat(L, 1) + 0.2 * ref.repeat(L, 1).roll(3, -1)
           + 0.01 * torch.randn(L * B, T, generator=g).to(dev)).contiguous()
    R = L * B

    def kernel():
        return ops.bss_sdr(est, ref)

    def composition():
        return torch_composition(est, ref)

    diff = float((kernel() - composition()).abs().max())
    k_ms, c_ms = [], []
    for _ in range(4):  # alternate the two
        k_ms += event_ms(kernel, 20, 2, 5)
        c_ms += event_ms(composition, 3, 2, 1)
    return {"levels": L, "clips": B, "rows": R, "samples": T, "filter_length": F,
            "max_abs_diff_db": diff, "bss_sdr": stats(k_ms), "torch_fp64": stats(c_ms),
            "ratio_torch_over_bss_sdr": round(statistics.median(c_ms) / statistics.median(k_ms), 2),
            "launches": launch_split(est, ref, R, B, T)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdr_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "clock": "HIP events",
           "sdr_chunk": _lib.SDR_CHUNK,
           "cases": [case(12, 1, 441000, dev), case(1, 32, 44100, dev), case(1, 1, 441000, dev)]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
