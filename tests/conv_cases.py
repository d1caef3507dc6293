"""The forward convs' case table, shared by tests/test_conv_cases.py (host only: the table runs
the plans it claims, carries their edges and stays small) and tests/test_gpu_conv_edges.py (the
HIP kernels are judged on it per element against fp64). Importable without a GPU.

Groups
  plan      one case per distinct plan (entry kind, path, BM, BN, taps, x3 kind, split-K parts) of
            tests/golden/conv_plan_parent.json plus the five plans only the direct kernel tests of
            tests/test_gpu_parity.py reach (EXTRA_PLANS). The fixture gives the plan keys only:
            every shape comes from the planner's rules (csrc/conv_plan.h) restated in plan_shape(),
            the smallest that still has B >= 2, three K chunks with a ragged last one, a ragged
            last N tile, tout % 4 != 0 and a ragged last M tile wherever the plan admits them.
  epilogue  two cases per distinct epilogue (kind, BM, BN): tout % 4 == 0 with a residual, tanh
            and the next layer's Snake next to y (the 16-byte stores and vector residual loads);
            tout % 4 != 0 with sigmoid and the next layer's Snake alone (y = NULL).
  convt     ConvTranspose strides 2, 4, 8 (vector walk) and 3, 6 (generic walk): pad 0 and
            (s + 1) // 2, tin = 1 and a tin that leaves the last tile ragged.
  off       the kernels off the MFMA tiles: the Cin = 1 k7 stream kernel and its MFMA fallback,
            the Cout = 1 stream kernel at its `interior` boundaries, the small-Cout kernel across
            its 256-sample blocks.
  ru        the fused ResidualUnit: every C, with and without x3 planes, around its time tile.

Inputs (inputs()): a seeded CPU generator; x scaled per input channel by 2^-e, e uniform in
0..10, w per output channel by 2^-e' and per input channel by 2^+e (products stay O(1) within a
row, row sums differ by up to 2^10), bias and residual in proportion to their row's scale, Snake
alpha in [0.5, 2]."""
import functools
import json
import os
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from vrvq_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN_ARGS = ("kind", "B", "cin", "tin", "cout", "k", "stride", "pad", "dil", "x3", "ws")
PLAN_KEYS = ("path", "BM", "BN", "KS", "x3", "S")

# The table's size: the sum over all cases of B (cin tin + cout tout) + cin k cout (floats of
# x, y and w), and the largest single case outside the B = 48 ones (the 96-wide rule needs 384
# workgroups, i.e. 48 clips of 8 row tiles).
TOTAL_FLOATS_CAP = 80_000_000
CASE_FLOATS_CAP = 4_000_000

# Plans that only the direct kernel-versus-torch tests of test_gpu_parity.py produce.
EXTRA_PLANS = [("conv", 0, 32, 128, 8, 0, 0), ("conv", 0, 32, 128, 16, 0, 0),
               ("conv", 0, 32, 128, 2, 2, 0), ("convt", 0, 32, 128, 2, 0, 0),
               ("convt", 0, 32, 128, 2, 1, 0)]

Case = namedtuple("Case", "name group kind B cin tin cout k stride pad dil x3 ws snake bias res "
                          "epi out_snake want_raw")


def case(name, group, kind, B, cin, tin, cout, k, stride=1, pad=0, dil=1, x3=False, ws=True,
         snake=True, bias=True, res=False, epi=0, out_snake=False, want_raw=True):
    return Case(name, group, kind, B, cin, tin, cout, k, stride, pad, dil, bool(x3), bool(ws),
                snake, bias, res, epi, out_snake, want_raw)


def out_len(c):
    if c.kind == "convt":
        return (c.tin - 1) * c.stride - 2 * c.pad + 2 * c.stride
    return (c.tin + 2 * c.pad - c.dil * (c.k - 1) - 1) // c.stride + 1


def floats(c):
    return c.B * (c.cin * c.tin + c.cout * out_len(c)) + c.cin * c.k * c.cout


def plan_of(c):
    """The plan of a case, from the code that launches it (host only)."""
    return _lib.conv_plan(*(getattr(c, a) for a in PLAN_ARGS))


def plan_key(c):
    p = plan_of(c)
    return (c.kind,) + tuple(p[n] for n in PLAN_KEYS)


def fixture_plans():
    """The distinct plans of the status-0 rows of conv_plan_parent.json, in sorted order."""
    with open(os.path.join(HERE, "golden", "conv_plan_parent.json")) as f:
        grid = json.load(f)
    keys = set()
    for r in grid:
        if r["status"] == 0:
            p = _lib.conv_plan(*(r[a] for a in PLAN_ARGS))
            keys.add((r["kind"],) + tuple(p[n] for n in PLAN_KEYS))
    return sorted(keys)


# ------------------------------------------------------------------ the dispatch rules, inverted
def chunk_channels(KS, BM, BN, x3):
    """Input channels per K chunk of a plan: conv_core.h ChunkCfg (fp32-input loop), conv_x3.h
    X3Cfg (x3 = 1 plain, 2 pair chunks)."""
    if x3:
        return (2 if x3 == 2 else 1) * (32 if KS == 1 else 16 if KS <= 3 else 8)
    ck0 = 32 if KS == 1 else 16 if KS <= 3 else 8 if KS in (4, 7) else 4 if KS == 8 else \
        (4 if BN > 32 else 2)
    return ck0 // 2 if BM > 128 and ck0 >= 8 else ck0


# GEMM columns that give a tile width with a ragged last tile of two or more (conv_plan.h tile_width():
# <= 32 -> 32; <= 96 -> 32, or 96 at 384 workgroups / for the x3 ConvTranspose; above, 64 where
# that pads under 0.7 of what 128 pads), and the same with tout % 4 == 0.
COLUMNS = {32: 70, 96: 87, 64: 130, 128: 197, 256: 641}
COLUMNS4 = {32: 68, 96: 88, 64: 132, 128: 196, 256: 644}
K7_DILATIONS = (1, 3, 9)


def plan_shape(key, aligned=False, n=0):
    """A case's shape arguments for a plan key (kind, path, BM, BN, KS, x3, S) by the rules of
    choose_tile() / tile_width() / splitk_parts() of csrc/conv_plan.h; n varies what the plan leaves free (the
    k7 dilation, the ConvTranspose's stride). aligned: tout % 4 == 0."""
    kind, path, BM, BN, KS, x3, S = key
    assert path == 0
    cols = (COLUMNS4 if aligned else COLUMNS)[BN]
    if kind == "convt":
        return _convt_shape(BM, BN, x3, cols, n)
    B = 2
    if kind == "proj":
        cout = 1024
    elif BM == 32:
        cout = 24
    elif BM == 64:
        cout = 128 if BN == 256 else 40     # 64 x 256: M >= 128 and a multiple of 64
    elif BM == 96:
        cout = 72
    elif BM == 192:
        cout = 384 if (KS == 1 and x3 == 0) else 192   # fp32 k1: M % 192 == 0 and % 128 == 0
    elif S > 0:
        cout = 128                          # split-K: M % 128 == 0
    elif BN == 96:
        cout = 900                          # 96-wide unsplit: ceil(M / 128) B >= 384
    else:
        cout = 200
    if BN == 96 and S == 0:
        B = 48
    if BN == 32 and kind == "proj":
        B = 3
    tout, dil, stride, has_x3 = cols, 1, 1, x3 > 0
    if KS in (4, 8, 16):                    # the strided convs on the fp32-input loop
        k, stride = KS, KS // 2
    elif KS == 2 and x3 and (BN in (32, 128) or S > 0):
        # x3 2-tap tiles of a conv: the phase-split view of a strided conv (k = 2 s)
        stride = 8 if S > 0 else (2, 4, 8)[n % 3]
        k = 2 * stride
    else:
        k = KS
    if KS == 7:
        dil = K7_DILATIONS[n % 3]
        if BN == 256 and x3 == 0:
            dil, has_x3 = 10, True          # past the x3 window: the fp32-input loop on 64 x 256
    # channels: three chunks with a ragged last one; pair chunks and the view's split take whole
    # chunks; split-K takes 8 S chunks
    ck = chunk_channels(KS, BM, BN, x3)
    if KS == 2 and stride > 1:
        if x3 == 2:
            cin = (8 * S if S else 3) * ck // stride
        else:
            cin = {2: 21, 4: 9, 8: 5}[stride]   # cin s = 42 / 36 / 40: no multiple of 32
    elif x3 == 2 or (BN == 256 and x3 == 0):
        cin = 3 * 16                        # k7 pair chunks (Cin % 16 == 0)
    elif S > 0:
        cin = (8 * S - 1) * ck + 5
    else:
        cin = 2 * ck + 5
    if stride > 1:
        pad = stride // 2
        tin = (tout - 1) * stride + k - 2 * pad
    elif k % 2:
        pad = dil * (k - 1) // 2
        tin = tout
    else:
        pad = 0
        tin = tout + k - 1
    return dict(kind=kind, B=B, cin=cin, tin=tin, cout=cout, k=k, stride=stride, pad=pad, dil=dil,
                x3=has_x3, ws=True)


def _convt_shape(BM, BN, x3, cols, n):
    """Polyphase ConvTranspose: M = cout s rows, tin + 1 columns."""
    B = 2
    if BM == 192:
        stride = 3 if BN == 64 else 6       # strides that do not divide 128
        rows = 240
        cols = 87 if BN == 64 else cols     # 192 rows: 64-wide up to 96 columns
    else:
        stride = (2, 4, 8)[n % 3]
        rows = {32: 24, 64: 40, 96: 72, 128: 200}[BM]
        if BM == 128 and BN == 96 and x3 == 0:
            B, stride, rows = 48, 8, 904    # 96-wide fp32-input: ceil(M / 128) B >= 384
    if BN == 32:
        cols = 30                           # the x3 ConvTranspose is 96-wide from 33 columns
    cin = 96 if x3 == 2 else 37             # pair chunks of 32 / three plain chunks of 16
    return dict(kind="convt", B=B, cin=cin, tin=cols - 1, cout=rows // stride, k=2 * stride,
                stride=stride, pad=(stride + 1) // 2, dil=1, x3=x3 > 0, ws=False)


def _name(key, tag=""):
    kind, _path, BM, BN, KS, x3, S = key
    return f"{kind}_{BM}x{BN}_k{KS}_{('f32', 'x3', 'x3pair')[x3]}" + (f"_S{S}" if S else "") + tag


# ------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in a fixed order."""
    out = []
    plans = [k for k in fixture_plans() if k[1] == 0] + EXTRA_PLANS
    for n, key in enumerate(plans):
        out.append(case(_name(key), "plan", **plan_shape(key, n=n)))
    # k7 with pad = 27 > T (dilation 9 on a 23-sample row)
    out.append(case("conv_k7_pad27_T23", "plan", "conv", 2, 21, 23, 200, 7, 1, 27, 9, x3=True))

    # epilogues: the smallest plan case of each (kind, BM, BN)
    epi = {}
    for n, key in enumerate(plans):
        e = (key[0], key[2], key[3])
        c = case("", "", **plan_shape(key, n=n))
        if e not in epi or floats(c) <= epi[e][2]:   # ties: the x3 loop
            epi[e] = (key, n, floats(c))
    for e in sorted(epi):
        key, n, _ = epi[e]
        conv = key[0] == "conv"
        out.append(case(_name(key, "_vec"), "epilogue", **plan_shape(key, aligned=True, n=n),
                        res=conv, epi=1 if conv else 0, out_snake=key[0] != "proj",
                        want_raw=True))
        out.append(case(_name(key, "_noraw"), "epilogue", **plan_shape(key, n=n),
                        epi=2 if conv else 0, out_snake=key[0] != "proj", want_raw=False))

    # ConvTranspose walks
    for s in (2, 4, 8, 3, 6):
        rows = 192 if s in (3, 6) else 128
        for pad in (0, (s + 1) // 2):
            for tin in (1, 99):      # 100 columns: a ragged last tile at every width
                for x3 in (False, True):
                    if x3 != (pad == 0) and tin == 1:
                        continue     # tin = 1 once per (stride, pad), alternating the loop
                    out.append(case(f"convt_s{s}_p{pad}_t{tin}_{'x3' if x3 else 'f32'}", "convt",
                                    "convt", 2, 37, tin, (rows + 40) // s, 2 * s, s, pad, 1, x3=x3,
                                    ws=False, out_snake=True))

    # off the MFMA tiles
    for tout in (4, 1024, 1028, 701, 1027):      # Cin = 1: stream (one block, two), fallback
        out.append(case(f"cin1_k7_t{tout}", "off", "conv", 2, 1, tout, 64, 7, 1, 3, 1, x3=False,
                        snake=False, out_snake=True))
    for k, pad in ((7, 3), (3, 1)):              # Cout = 1 stream: `interior` at both row ends
        for tin in (4, 8, 1024, 1028):
            for cin in (5, 8, 13):
                out.append(case(f"cout1_k{k}_t{tin}_c{cin}", "off", "conv", 2, cin, tin, 1, k, 1,
                                pad, 1, x3=False, snake=cin != 8, res=cin == 13,
                                epi=1 if cin == 5 else 0))
    n = 0
    for T in (255, 256, 257, 600):               # small Cout: the 256-sample blocks
        for dil in (1, 9):
            for cout in (1, 3, 8):
                cin = (5, 16, 17)[n % 3]
                k = 7 if (dil == 9 or n % 2) else 3
                n += 1
                pad = dil * (k - 1) // 2
                out.append(case(f"small_c{cin}_o{cout}_k{k}_d{dil}_t{T}", "off", "conv", 2, cin, T,
                                cout, k, 1, pad, dil, x3=False, res=cout == 3,
                                epi=2 if cout == 8 else 0, out_snake=cout == 1))
        n += 1

    # fused ResidualUnit (kind "ru": cin = cout = C, k = 7, pad = 3 dil; x3 = w7_x3 / w1_x3 given)
    for C in (64, 96, 128, 192, 256):
        bn = 64 if C >= 192 else 128
        for x3 in (True, False):
            for i, T in enumerate((bn - 1, bn + 1, 2 * bn + 3, 5)):
                for j, dil in enumerate((1, 9)):
                    raw = (i + j) % 2 == 0
                    out.append(case(f"ru{C}_{'x3' if x3 else 'f32'}_t{T}_d{dil}", "ru", "ru", 2, C,
                                    T, C, 7, 1, 3 * dil, dil, x3=x3, ws=False, out_snake=True,
                                    want_raw=raw))
    names = [c.name for c in out]
    assert len(set(names)) == len(names), "case names must be unique"
    return tuple(out)


def group(name):
    return [c for c in cases() if c.group == name]


# ------------------------------------------------------------------ inputs and references
def _seed(c):
    return zlib.crc32(c.name.encode()) & 0x7FFFFFFF


def _pow2(e):
    return torch.ldexp(torch.ones(e.shape), e.to(torch.int32))


def inputs(c):
    """CPU fp32 tensors of a case: x, w (Conv1d (cout, cin, k) / ConvTranspose1d (cin, cout, k)
    layout), b, alpha, res, alpha_out; for "ru" also x_snk, w1, b1, alpha2 (w / b: the k7 stage's)."""
    g = torch.Generator(device="cpu").manual_seed(_seed(c))
    ei = torch.randint(0, 11, (c.cin,), generator=g)
    eo = torch.randint(0, 11, (c.cout,), generator=g)
    si, so = _pow2(-ei), _pow2(-eo)
    x = (torch.rand(c.B, c.cin, c.tin, generator=g) - 0.5) * si.view(1, -1, 1)
    alpha = torch.rand(c.cin, generator=g) * 1.5 + 0.5
    alpha_out = torch.rand(c.cout, generator=g) * 1.5 + 0.5
    fan = (c.cin * (2 if c.kind == "convt" else c.k)) ** 0.5
    if c.kind == "convt":
        w = torch.randn(c.cin, c.cout, c.k, generator=g) / fan
        w = w * so.view(1, -1, 1) / si.view(-1, 1, 1)
    else:
        w = torch.randn(c.cout, c.cin, c.k, generator=g) / fan
        w = w * so.view(-1, 1, 1) / si.view(1, -1, 1)
    d = dict(x=x, w=w, alpha=alpha, alpha_out=alpha_out,
             b=torch.randn(c.cout, generator=g) * 0.1 * so,
             res=torch.randn(c.B, c.cout, out_len(c), generator=g) * 0.5 * so.view(1, -1, 1))
    if c.kind == "ru":
        # h rows scaled 2^-eo, y rows back on x's scale 2^-ei (the skip adds x)
        d["alpha2"] = torch.rand(c.cout, generator=g) * 1.5 + 0.5
        w1 = torch.randn(c.cout, c.cout, 1, generator=g) / c.cout ** 0.5
        d["w1"] = w1 * si.view(-1, 1, 1) / so.view(1, -1, 1)
        d["b1"] = torch.randn(c.cout, generator=g) * 0.1 * si
        d["x_snk"] = snake(x, alpha)      # an input of the unit (the producer's epilogue Snake)
    return d


def snake(x, alpha):
    """models/layers.py:30 in x's precision."""
    a = alpha.to(x.dtype).view(1, -1, 1)
    return x + (a + 1e-9).reciprocal() * torch.sin(a * x).pow(2)


def _conv(c, x, w, b):
    if c.kind == "convt":
        return F.conv_transpose1d(x, w, b, stride=c.stride, padding=c.pad)
    return F.conv1d(x, w, b, stride=c.stride, padding=c.pad, dilation=c.dil)


def _forward(c, d, dtype):
    """(y before the activation, y) in dtype, the reference's op order."""
    x = d["x"].to(dtype)
    if c.snake:
        x = snake(x, d["alpha"])
    y = _conv(c, x, d["w"].to(dtype), d["b"].to(dtype) if c.bias else None)
    if c.res:
        y = d["res"].to(dtype) + y
    return y, (y, torch.tanh(y), torch.sigmoid(y))[c.epi]


def reference(c, d):
    """ref64 (the fp64 result), scale (the per-element size of the terms: the same operation on
    absolute values before the activation, or |ref64| where the activation's output is larger:
    a sigmoid's final rounding is relative to its output) and y32 (torch fp32 on the CPU)."""
    if c.kind == "ru":
        return _reference_ru(c, d)
    _, ref = _forward(c, d, torch.float64)
    x = d["x"].double()
    xs = snake(x, d["alpha"]).abs() if c.snake else x.abs()
    S = _conv(c, xs, d["w"].double().abs(), d["b"].double().abs() if c.bias else None)
    if c.res:
        S = S + d["res"].double().abs()
    _, y32 = _forward(c, d, torch.float32)
    return ref, torch.maximum(S, ref.abs()), y32


def _ru_forward(c, d, dtype):
    x = d["x"].to(dtype)
    h = F.conv1d(d["x_snk"].to(dtype), d["w"].to(dtype), d["b"].to(dtype), padding=c.pad,
                 dilation=c.dil)
    hs = snake(h, d["alpha2"])
    return h, hs, x + F.conv1d(hs, d["w1"].to(dtype), d["b1"].to(dtype))


def _reference_ru(c, d):
    """y = x + b1 + W1 snake2(b7 + W7 *_dil x_snk); scale = |W1| |snake2(h)| + |b1| + |x| +
    2 |W1| S_h, S_h the k7 stage's scale (Snake's slope is at most 2 for alpha >= 0.5)."""
    _h, hs, ref = _ru_forward(c, d, torch.float64)
    x = d["x"].double()
    Sh = F.conv1d(d["x_snk"].double().abs(), d["w"].double().abs(), d["b"].double().abs(),
                  padding=c.pad, dilation=c.dil)
    w1 = d["w1"].double().abs()
    S = F.conv1d(hs.abs(), w1, d["b1"].double().abs()) + x.abs() + 2 * F.conv1d(Sh, w1)
    return ref, S, _ru_forward(c, d, torch.float32)[2]


UNIT = 2.0 ** -24


def units(got, ref64, scale):
    """max over elements of |got - ref64| / (2^-24 scale)."""
    err = (got.double() - ref64).abs() / (UNIT * scale.clamp_min(1e-300))
    return float(err.max())
