"""Times of the on-GPU level solver (profiles/rate_solve.json; DESIGN.md "Rate control").

  solver     vrvq_rate_solve (HIP events around a run of launches) against the same answer from
             the ops that existed before it: a host bisection over the float32 bit patterns, each
             round scale_imp -> imp_mask -> bpf -> .item() (one host sync per round), at
             B = 32 x T = 87 per clip and 600 x 86 pooled
  encode     model.encode(target_kbps=...) against model.encode(level=1) at B = 32 x 1 s,
             alternating, HIP events

Needs an MI355X; there is no CPU path. Usage: python tools/rate_bench.py --out FILE.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vrvq_amd  # noqa: E402
from vrvq_amd import ops, utils  # noqa: E402

LO, HI, NQ = 0.125, 6.0, 8


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


def host_bisect(imp_rows, bits_f, budget: int):
    """The solver's answer from scale_imp / imp_mask / bpf: (level, total, rounds)."""
    R, T = imp_rows.shape
    rounds = 0

    def total(level):
        nonlocal rounds
        rounds += 1
        s = ops.scale_imp(imp_rows, float(level), float(NQ))
        bpf = ops.bpf(ops.mask_hard(s.reshape(R, 1, T), NQ), bits_f).item()  # host sync
        return round(bpf * R * T)

    lo, hi = np.float32(LO), np.float32(HI)
    t_lo = total(lo)
    if t_lo > budget:
        return float(lo), t_lo, rounds
    t_hi = total(hi)
    if t_hi <= budget:
        return float(hi), t_hi, rounds
    a, b, tot = int(lo.view(np.uint32)), int(hi.view(np.uint32)), t_lo
    while b - a > 1:
        m = a + (b - a) // 2
        t = total(np.uint32(m).view(np.float32))
        if t <= budget:
            a, tot = m, t
        else:
            b = m
    return float(np.uint32(a).view(np.float32)), tot, rounds


def solver_case(B: int, T: int, pooled: bool, dev):
    g = torch.Generator().manual_seed(B * 1000 + T)
    imp = torch.rand(B, T, generator=g).to(dev)
    bits_i = torch.full((NQ,), 10, dtype=torch.int32, device=dev)
    bits_f = torch.full((NQ,), 10.0, device=dev)
    groups = [(0, B)] if pooled else [(b, b + 1) for b in range(B)]
    off = torch.tensor([g0 for g0, _ in groups] + [B], dtype=torch.int32, device=dev)
    # budgets half way between the totals at the two ends of the level range
    ends = ops.rate_curve(imp, torch.tensor([LO, HI], device=dev), bits_i).cpu()
    budgets = [int((ends[g0:g1, 0].sum() + ends[g0:g1, 1].sum()) // 2) for g0, g1 in groups]
    budget = torch.tensor(budgets, dtype=torch.int64, device=dev)

    def kernel():
        return ops.rate_solve(imp, bits_i, off, budget, LO, HI)

    def host():
        return [host_bisect(imp[g0:g1], bits_f, budgets[i]) for i, (g0, g1) in enumerate(groups)]

    level, total, status = (x.cpu().tolist() for x in kernel())
    ref = host()
    same = all(level[i] == ref[i][0] and total[i] == ref[i][1] for i in range(len(groups)))
    k_ms = event_ms(kernel, calls=200, repeats=7, warmup=50)
    host()  # warm-up
    h_ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()  # every round ends in .item(): the host clock sees the whole of it
        h_ms.append((time.perf_counter() - t0) * 1e3)
    return {"rows": B, "frames": T, "groups": len(groups), "status": sorted(set(status)),
            "host_rounds_per_group": ref[0][2], "same_answer": same,
            "rate_solve": stats(k_ms), "host_bisection": stats(h_ms),
            "speedup": round(statistics.median(h_ms) / statistics.median(k_ms), 1)}


def encode_case(dev, target_kbps: float):
    from vrvq_amd.config import A2_KWARGS
    from vrvq_amd.recipe import load_recipe, synthetic_audio
    model = vrvq_amd.DAC_VRVQ(**A2_KWARGS)
    load_recipe(model, 0)
    model = model.to(dev).eval()
    x = model.preprocess(torch.from_numpy(synthetic_audio(32, 44100, seed=3)).to(dev), 44100)

    def plain():
        return model.encode(x, None, 1, want_z_q_is=False)

    def target():
        return model.encode(x, target_kbps=target_kbps, want_z_q_is=False)

    with torch.no_grad():
        status = target()["rate_status"].cpu().tolist()
        p, q = [], []
        for _ in range(5):  # alternate the two so that drift hits both
            p += event_ms(plain, calls=20, repeats=1, warmup=5)
            q += event_ms(target, calls=20, repeats=1, warmup=5)
    utils.check_errors(dev)
    return {"clips": 32, "seconds": 1.0, "target_kbps": target_kbps,
            "status_counts": {str(s): status.count(s) for s in sorted(set(status))},
            "encode_level_1": stats(p), "encode_target_kbps": stats(q),
            "difference_ms": round(statistics.median(q) - statistics.median(p), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--target-kbps", type=float, default=4.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "solver": [solver_case(32, 87, False, dev), solver_case(600, 86, True, dev)],
           "encode": encode_case(dev, args.target_kbps)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
