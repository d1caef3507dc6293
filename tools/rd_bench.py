"""Times of the on-GPU distortion metrics and what is built on them (profiles/rd_metrics.json;
DESIGN.md "Distortion metrics").

  metrics    ops.signal_metrics (two launches, HIP events around a run of calls) at (L * B, T) =
             (4 * 32, 44100) and (12 * 1, 441000), against the same four numbers
               host     device -> host copy of the reconstructions + the fp64 formulas in torch on
                        the CPU (what a caller of the reference's cal_metrics pays; host clock)
               torch    the fp64 formulas in torch ops on the GPU (HIP events)
             and the rate of the first launch from its byte count: the two launches through the
             C-ABI minus the same call at one sample per row, once on one pair of buffers (which
             the 256 MiB Infinity Cache keeps between back-to-back calls: a cache-resident
             rate) and once rotating through copies of 512 MiB and more in all, so that each call
             reads rows streamed out of the caches since their last use (the HBM rate)
  sweep      utils.rd_sweep against utils.level_sweep at both shapes (host clock; both end in a
             device synchronise)
  quality    utils.solve_quality(iters=8) against one plain model(audio) step at B = 32 x 1 s

Needs an MI355X; there is no CPU path. Usage: python tools/rd_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrvq_amd  # noqa: E402
from vrvq_amd import _lib, ops, utils  # noqa: E402

EPS = 2.0 ** -23
HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


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


def host_ms(fn, repeats: int, warmup: int):
    """Milliseconds of fn by the host clock; fn ends synchronised with the device."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 5), "min_ms": round(min(xs), 5),
            "max_ms": round(max(xs), 5), "windows": len(xs)}


def formulas(p, t):
    """The four metrics of rows p against rows t (same shape) in fp64 torch ops, any device."""
    p, t = p.to(torch.float64), t.to(torch.float64)

    def si(p, t):
        alpha = ((p * t).sum(-1, keepdim=True) + EPS) / ((t * t).sum(-1, keepdim=True) + EPS)
        s = alpha * t
        return 10 * torch.log10(((s * s).sum(-1) + EPS) / (((s - p) ** 2).sum(-1) + EPS))

    d = p - t
    return torch.stack([si(p, t), si(p - p.mean(-1, keepdim=True), t - t.mean(-1, keepdim=True)),
                        10 * torch.log10(((t * t).sum(-1) + EPS) / ((d * d).sum(-1) + EPS)),
                        d.abs().mean(-1)], 1)


def first_launch_ms(pairs, R, B, T, repeats: int):
    """The two launches through the C-ABI, call i on pairs[i % len(pairs)], and the same with one
    sample per row (the second launch and the launch overheads alone): per-call ms of each."""
    n = ctypes.c_longlong(0)
    _lib.call("vrvq_signal_metrics_workspace", R, T, ctypes.byref(n))
    dev = pairs[0][0].device
    ws = torch.empty(n.value // 8, dtype=torch.float64, device=dev)
    met = torch.empty(R, 4, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = [(ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(r.data_ptr())) for e, r in pairs]
    turn = [0]

    def call(samples):
        e, r = ptrs[turn[0] % len(ptrs)]
        turn[0] += 1
        _lib.call("vrvq_signal_metrics", e, r, R, B, samples, None,
                  ctypes.c_void_p(met.data_ptr()), None, ctypes.c_void_p(ws.data_ptr()), n.value,
                  stream)

    calls = 5 * len(pairs) if len(pairs) > 1 else 100
    return (event_ms(lambda: call(T), calls, repeats, len(pairs) + 20),
            event_ms(lambda: call(1), calls, repeats, 20))


def rate(read: int, both, tiny):
    first = max(statistics.median(both) - statistics.median(tiny), 1e-6)
    return {"two_launches": stats(both), "one_sample_rows": stats(tiny),
            "first_launch_ms_by_difference": round(first, 5),
            "bytes_per_s": round(read / (first * 1e-3), 0),
            "share_of_hbm_peak": round(read / (first * 1e-3) / HBM_BYTES_PER_S, 4)}


def metrics_case(L: int, B: int, T: int, dev):
    g = torch.Generator().manual_seed(L * 1000 + B)
    ref = (0.3 * torch.randn(B, T, generator=g) + 0.05).to(dev)
    est = (0.7 * ref.repeat(L, 1) + 0.01 * torch.randn(L * B, T, generator=g).to(dev)).contiguous()
    R = L * B

    def kernel():
        return ops.signal_metrics(est, ref, None)[0]

    def torch_gpu():
        return formulas(est, ref.repeat(L, 1))

    def host():
        return formulas(est.cpu(), ref.cpu().repeat(L, 1))

    got, want = kernel().cpu(), host()
    k_ms = event_ms(kernel, 100, 7, 20)
    g_ms = event_ms(torch_gpu, 20, 7, 5)
    h_ms = host_ms(host, 5, 2)
    read = 2 * R * T * 4
    pair_bytes = (R + B) * T * 4
    copies = -(-(512 << 20) // pair_bytes)
    pairs = [(est.clone(), ref.clone()) for _ in range(copies)]
    warm = rate(read, *first_launch_ms(pairs[:1], R, B, T, 7))
    cold = rate(read, *first_launch_ms(pairs, R, B, T, 7))
    return {"rows": R, "clips": B, "samples": T,
            "workgroups_first_launch": R * -(-T // _lib.METRICS_CHUNK),
            "max_abs_diff_db_vs_host_formula": float((got[:, :3] - want[:, :3]).abs().max()),
            "signal_metrics": stats(k_ms), "torch_ops_gpu": stats(g_ms),
            "copy_to_host_and_cpu_formula": stats(h_ms), "bytes_read": read,
            "capi_same_buffers": warm, "capi_rotating_buffers": dict(cold, copies=copies)}


def model_cases(dev):
    from vrvq_amd.config import A2_KWARGS
    from vrvq_amd.recipe import load_recipe, synthetic_audio
    model = vrvq_amd.DAC_VRVQ(**A2_KWARGS)
    load_recipe(model, 0)
    model = model.to(dev).eval()
    out = {"sweep": []}
    for L, B, n in ((4, 32, 44100), (12, 1, 441000)):
        audio = torch.from_numpy(synthetic_audio(B, n, seed=3)).to(dev)
        levels = [0.125 * 48 ** (i / max(L - 1, 1)) for i in range(L)]
        cap = 32  # a level's clips per decode at the first shape, all 12 at the second

        def rd():
            return utils.rd_sweep(model, audio, levels, max_decode_clips=cap)

        def plain():
            return utils.level_sweep(model, audio, levels, max_decode_clips=cap)

        a, b = [], []
        for _ in range(3):  # alternate the two so that drift hits both
            a += host_ms(plain, 2, 1)
            b += host_ms(rd, 2, 1)
        out["sweep"].append({"levels": L, "clips": B, "samples": n, "max_decode_clips": cap,
                             "level_sweep": stats(a), "rd_sweep": stats(b),
                             "difference_ms": round(statistics.median(b) - statistics.median(a),
                                                    4)})
    audio = torch.from_numpy(synthetic_audio(32, 44100, seed=3)).to(dev)
    ends = utils.rd_sweep(model, audio, [model.quantizer.level_min, model.quantizer.level_max])
    target = ends["si_sdr"].mean(0).tolist()

    def step():
        with torch.no_grad():
            return model(audio, 44100, None, 1)

    def solve():
        return utils.solve_quality(model, audio, target, iters=8)

    status = solve()["status"].cpu().tolist()
    a, b = [], []
    for _ in range(3):
        a += event_ms(step, 10, 1, 3)
        b += event_ms(solve, 3, 1, 1)
    utils.check_errors(dev)
    out["quality"] = {"clips": 32, "seconds": 1.0, "iters": 8, "decodes_of_B": 10,
                      "status_counts": {str(s): status.count(s) for s in sorted(set(status))},
                      "model_step": stats(a), "solve_quality": stats(b),
                      "ratio": round(statistics.median(b) / statistics.median(a), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rd_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "clock": "HIP events (host clock where noted)",
           "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
           "metrics": [metrics_case(4, 32, 44100, dev), metrics_case(12, 1, 441000, dev)]}
    res.update(model_cases(dev))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
