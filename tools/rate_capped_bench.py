"""Times of capped rate control (profiles/rate_capped.json; DESIGN.md "Capped rate control"), by
the method of tools/rate_bench.py: HIP events over windows of back-to-back calls after warm-up,
the median of several windows.

  solver   vrvq_rate_solve_capped (two launches) against vrvq_rate_solve (one) on the same maps,
           alternated: B = 32 x T = 87 per clip with packets of 20 frames, and 600 x 86 pooled
           with packets of 86 (one per row). The maps are uniform noise under a 1 / 0.25
           checkerboard over (row, packet), the group budget half way between the totals at the
           two ends of the level range and a packet's budget 0.7 of all its codes, so that the
           cap binds some packets and not others.
  encode   model.encode(target_kbps, max_kbps, packet_frames) against model.encode(target_kbps)
           at B = 32 x 1 s, alternated.

Each step is a process of its own and merges its result into --out; run them under a time limit
each and stop at the first that fails:

  timeout -k 10 300 python tools/rate_capped_bench.py --step solver --out profiles/rate_capped.json \\
    && timeout -k 10 600 python tools/rate_capped_bench.py --step encode --out profiles/rate_capped.json

Needs an MI355X; there is no CPU path.
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
from vrvq_amd import ops, utils  # noqa: E402
from tools.rate_bench import HI, LO, NQ, event_ms, stats  # noqa: E402


def solver_case(B: int, T: int, P: int, pooled: bool, dev):
    g = torch.Generator().manual_seed(B * 1000 + T)
    NP = utils.packets_of(T, P)
    rows, packets = torch.arange(B)[:, None], torch.arange(NP)[None]
    gain = torch.where((rows + packets) % 2 == 0, 1.0, 0.25).repeat_interleave(P, 1)[:, :T]
    imp = (torch.rand(B, T, generator=g) * gain).to(dev)
    bits_i = torch.full((NQ,), 10, dtype=torch.int32, device=dev)
    groups = [(0, B)] if pooled else [(b, b + 1) for b in range(B)]
    off = torch.tensor([g0 for g0, _ in groups] + [B], dtype=torch.int32, device=dev)
    ends = ops.rate_curve(imp, torch.tensor([LO, HI], device=dev), bits_i).cpu()
    budget = torch.tensor([int((ends[g0:g1, 0].sum() + ends[g0:g1, 1].sum()) // 2)
                           for g0, g1 in groups], dtype=torch.int64, device=dev)
    frames = [min(P, T - p * P) for p in range(NP)]
    packet_budget = torch.tensor([int(0.7 * 10 * NQ * n) for n in frames], dtype=torch.int64,
                                 device=dev)

    def plain():
        return ops.rate_solve(imp, bits_i, off, budget, LO, HI)

    def capped():
        return ops.rate_solve_capped(imp, bits_i, off, budget, packet_budget, P, LO, HI)

    out = capped()
    status, p_status = out[2].cpu().tolist(), out[5].cpu().reshape(-1).tolist()
    raised = bool((out[0] >= plain()[0]).all())
    a, b = [], []
    for _ in range(7):  # alternate the two so that drift hits both
        a += event_ms(plain, calls=200, repeats=1, warmup=50)
        b += event_ms(capped, calls=200, repeats=1, warmup=50)
    return {"rows": B, "frames": T, "packet_frames": P, "groups": len(groups),
            "status": sorted(set(status)),
            "packet_status_counts": {str(s): p_status.count(s) for s in sorted(set(p_status))},
            "level_not_below_uncapped": raised, "rate_solve": stats(a),
            "rate_solve_capped": stats(b),
            "ratio": round(statistics.median(b) / statistics.median(a), 2)}


def encode_case(dev, target_kbps: float, max_kbps: float, P: int):
    from vrvq_amd.config import A2_KWARGS
    from vrvq_amd.recipe import load_recipe, synthetic_audio
    model = vrvq_amd.DAC_VRVQ(**A2_KWARGS)
    load_recipe(model, 0)
    model = model.to(dev).eval()
    x = model.preprocess(torch.from_numpy(synthetic_audio(32, 44100, seed=3)).to(dev), 44100)

    def target():
        return model.encode(x, target_kbps=target_kbps, want_z_q_is=False)

    def capped():
        return model.encode(x, target_kbps=target_kbps, max_kbps=max_kbps, packet_frames=P,
                            want_z_q_is=False)

    with torch.no_grad():
        out = capped()
        status = out["rate_status"].cpu().tolist()
        p_status = out["packet_status"].cpu().reshape(-1).tolist()
        p, q = [], []
        for _ in range(5):
            p += event_ms(target, calls=20, repeats=1, warmup=5)
            q += event_ms(capped, calls=20, repeats=1, warmup=5)
    utils.check_errors(dev)
    return {"clips": 32, "seconds": 1.0, "target_kbps": target_kbps, "max_kbps": max_kbps,
            "packet_frames": P,
            "status_counts": {str(s): status.count(s) for s in sorted(set(status))},
            "packet_status_counts": {str(s): p_status.count(s) for s in sorted(set(p_status))},
            "encode_target_kbps": stats(p), "encode_max_kbps": stats(q),
            "difference_ms": round(statistics.median(q) - statistics.median(p), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--step", choices=["solver", "encode"], required=True)
    ap.add_argument("--target-kbps", type=float, default=4.0)
    ap.add_argument("--max-kbps", type=float, default=4.5)
    ap.add_argument("--packet-frames", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_capped_bench: needs a GPU")
    dev = torch.device("cuda:0")
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    if args.step == "solver":
        res["solver"] = [solver_case(32, 87, 20, False, dev), solver_case(600, 86, 86, True, dev)]
    else:
        res["encode"] = encode_case(dev, args.target_kbps, args.max_kbps, args.packet_frames)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res[args.step]))


if __name__ == "__main__":
    main()
