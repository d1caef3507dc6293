"""The x3 K loop's refill addressing (csrc/conv_x3.h), through the C-ABI. Needs an MI355X.

conv_mainloop_x3 keeps a thread's W and x offsets in registers and walks the K chunks with
workgroup-uniform base pointers. What that can break is a wrong base for some (clip, M tile,
chunk, split-K part): a neighbouring row, chunk or clip read instead of the right one. So the
inputs are exact: x, w, bias and residual are integers in [-8, 8] (one bf16 plane each, the other
two zero), every sum stays far below 2^24 whatever its order, and the result must EQUAL torch
fp64 on the CPU on every element. No Snake. Buffers sit between the NaN guards of
tests/test_gpu_conv_edges.py, and vrvq_conv_last_launch must report the intended tile.

The shapes are the smallest that reach each path with more than one clip, M tile, N tile (a
ragged last one) and K chunk; each case pins its plan (BM, BN, KS, x3, S) with vrvq_conv_plan."""
import pytest
import torch

import conv_cases as C
import test_gpu_conv_edges as E

pytestmark = pytest.mark.gpu

# name, kind, B, cin, tin, cout, k, stride, pad, dil, residual, the plan (BM, BN, KS, x3, S)
CASES = [
    # pair k7 chunks on the 64 x 256 tile: three M tiles, three N tiles (ragged last), three chunks
    ("pair_k7_d1", "conv", 3, 48, 645, 192, 7, 1, 3, 1, False, (64, 256, 7, 2, 0)),
    ("pair_k7_d9", "conv", 3, 48, 645, 192, 7, 1, 27, 9, False, (64, 256, 7, 2, 0)),
    # plain k7 chunks, 128-row tile: two M tiles (ragged), six chunks with a ragged last one
    ("plain_k7_ragged", "conv", 2, 44, 200, 160, 7, 1, 3, 1, False, (128, 128, 7, 1, 0)),
    # k1 + residual on the 192 x 64 tile: four chunks of 32 channels, the last one ragged
    ("k1_res_192x64", "conv", 2, 104, 130, 192, 1, 1, 0, 1, True, (192, 64, 1, 1, 0)),
    # k3 split-K: 16 chunks in two parts, the second starts at chunk 8
    ("k3_splitk", "conv", 2, 256, 87, 128, 3, 1, 1, 1, False, (128, 96, 3, 1, 2)),
    # the phase-split view of a strided conv (64 -> 128 k4 s2): pair chunks of the view's channels
    ("view_k4_s2", "conv", 2, 64, 262, 128, 4, 2, 1, 1, False, (128, 128, 2, 2, 0)),
    # the polyphase ConvTranspose (128 -> 64 k4 s2): M = 128 phase rows, 71 columns
    ("convt_k4_s2", "convt", 2, 128, 70, 64, 4, 2, 1, 1, False, (128, 96, 2, 1, 0)),
]


def _ints(shape, g):
    return torch.randint(-8, 9, shape, generator=g).float()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_refill_bases_exact(case):
    name, kind, B, cin, tin, cout, k, stride, pad, dil, res, want = case
    c = C.case("refill_" + name, "refill", kind, B, cin, tin, cout, k, stride, pad, dil, x3=True,
               ws=True, snake=False, bias=True, res=res)
    plan = C.plan_of(c)
    assert plan["path"] == 0 and tuple(plan[n] for n in E.KEYS) == want, (name, plan)
    g = torch.Generator(device="cpu").manual_seed(C._seed(c))
    tout = C.out_len(c)
    d = dict(x=_ints((B, cin, tin), g),
             w=_ints((cin, cout, k) if kind == "convt" else (cout, cin, k), g),
             b=_ints((cout,), g), res=_ints((B, cout, tout), g),
             alpha=torch.ones(cin), alpha_out=torch.ones(cout))
    out = E._launch(c, d, E._device_side(c, d), want_y=True)   # plan record and guards inside
    ref = C._forward(c, d, torch.float64)[1]
    assert float(ref.abs().max()) < 2.0 ** 24
    got = out.y.cpu().double()
    bad = got != ref
    nbad = int(bad.sum())
    first = tuple(int(v) for v in bad.nonzero()[0]) if nbad else None
    print(f"\n[conv-refill] {name}: {got.numel()} elements, {nbad} differ"
          + (f", first at (clip, channel, t) = {first}: got {float(got[first])}, "
             f"want {float(ref[first])}" if nbad else ""))
    assert nbad == 0, (name, nbad, first)
