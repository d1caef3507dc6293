"""The forward conv kernels on the case table of tests/conv_cases.py, through the C-ABI
(vrvq_conv1d_ws, vrvq_conv1d_proj, vrvq_conv_transpose1d_pad, vrvq_residual_unit). Needs an MI355X.

Every case checks, in one launch:

(a) The plan ran: vrvq_conv_last_launch equals vrvq_conv_plan's answer for the case (a case off
    the MFMA tiles leaves the record of the launch before it in place).

(b) A per-element bar against torch fp64 on the CPU. With `scale` the same operation on absolute
    values (|w|, |snake x|, |b|, |res|; conv_cases.reference), u = max over elements of
    |got - ref64| / (2^-24 scale) and u32 the same figure of torch fp32 on the CPU:

        u <= 4 u32 + c,    c = 1 + 2 [x3 planes] + 9 [input Snake]   (the unit: see below)

    The factor 4 is the project's convention (e3 <= 4 e32 + 2e-7). c holds what the kernels do
    and torch fp32 does not, from what the code states, not from what the kernels measure:
      1  one final rounding: at most 2^-24 |y| <= one unit.
      2  conv_x3.h:9-11: the x3 loop drops a_m b_l + a_l b_m + a_l b_l <= 2^-23 |ab| of every
         product, at most 2 units of 2^-24 sum |a||b|.
      9  common.h: sin^2 from the degree-13 polynomial has a max abs error of 2.2e-7 = 3.7 units
         where sin^2 <= 1; taken as relative to sin^2 (the reduction is exact below 2^20 and the
         odd polynomial's error is relative to sin r; this reading is a supposition). Snake adds
         sin^2(t) / alpha to x, t = alpha |x| <= 1 for |x| <= 0.5 and alpha <= 2, while the scale
         counts |snake x| >= |x| (1 - sin^2(t) / t): the ratio (sin^2 t / t) / (1 - sin^2 t / t)
         is at most 2.43 (t = 1), 3.7 x 2.43 = 9.0 units.
    The fused ResidualUnit: c = 2 + 9 + 4 [x3 planes]: the final rounding and that of h (inside
    the 2 |W1| S_h term, slope <= 2), its Snake in the kernel, and both GEMMs' dropped terms.
    The yardstick is never another launch of the code under test. The next layer's Snake next to
    y is held to the existing convention, rel_err < 1e-6 against torch's Snake of the stored y;
    with y = NULL it equals, bit for bit, what the launch with y writes.

(c) Guarded buffers: y, y_snake, the split-K workspace and the projection partials are carved
    out of tensors pre-filled with a quiet NaN that carries a payload, GUARD floats on both
    sides (a multiple of 64, so every pointer keeps the allocator's alignment: the vector paths
    assume 16-byte-aligned pointers). After the launch the guards still hold the pattern, every
    element inside is finite and the workspace past vrvq_conv1d_workspace's bytes is untouched.
    x and the residual sit between the same NaN guards: a read outside them that reaches a
    result shows as NaN.

(d) test_x3_six_products pins the set of bf16 plane products (see there).

Every case prints u, u32 and the bar (pytest -s; profiles/r07_conv_edges_pytest_gpu.log)."""
import ctypes
import types

import pytest
import torch

import conv_cases as C
from conftest import rel_err
from vrvq_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("BM", "BN", "KS", "x3", "S")
SENTINEL = 0x7FC0BEEF   # a quiet NaN with a payload
GUARD = 4096            # floats on both sides, a multiple of 64


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """n floats between two guards, all of it pre-filled with SENTINEL."""

    def __init__(self, n, src=None):
        self.n = int(n)
        room = (self.n + 63) // 64 * 64
        self.raw = torch.full((GUARD + room + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.n].view(torch.float32)
        assert self.t.data_ptr() % 256 == self.raw.data_ptr() % 256
        if src is not None:
            self.t.copy_(src.reshape(-1).to(DEV))

    def check(self, what, written=None):
        """Guards (and everything past `written` floats) untouched, the rest finite."""
        written = self.n if written is None else int(written)
        assert bool((self.raw[:GUARD] == SENTINEL).all()), f"{what}: write before the buffer"
        assert bool((self.raw[GUARD + written:] == SENTINEL).all()), \
            f"{what}: write past the buffer"
        assert bool(torch.isfinite(self.t[:written]).all()), f"{what}: element not written"


def _snake_dev(y, alpha):
    a = alpha.reshape(1, -1, 1)
    return y + (a + 1e-9).reciprocal() * torch.sin(a * y).pow(2)


def _mark_record():
    """Overwrite the last-launch record: an 8 -> 16 k4 conv on the 32 x 128 fp32-input tile."""
    sx = torch.zeros(8 * 43, device=DEV)
    sw = torch.zeros(8 * 4 * 128, device=DEV)
    sy = torch.zeros(16 * 40, device=DEV)
    assert _lib.load().vrvq_conv1d(P(sx), 1, 8, 43, None, None, P(sw), None, 16, 128, 4, 1, 0, 1,
                                   None, None, 0, P(sy), 40, None, None, None, None) == 0
    before = _lib.conv_last_launch()
    assert [before[n] for n in KEYS] == [32, 128, 4, 0, 0]
    return before


def _check_record(c, before):
    plan = C.plan_of(c)
    after = _lib.conv_last_launch()
    if plan["path"] == 0:
        assert after == {n: plan[n] for n in KEYS}, (c.name, after, plan)
    else:
        assert after == before, (c.name, after, plan)


def _bar(c, u32):
    if c.kind == "ru":
        return 4 * u32 + 2 + 9 + (4 if c.x3 else 0)
    return 4 * u32 + 1 + (2 if c.x3 else 0) + (9 if c.snake else 0)


def _judge(c, got, ref):
    """(b): print and assert the per-element bar; got: device tensor of ref's shape."""
    ref64, scale, y32 = ref
    u = C.units(got.cpu(), ref64, scale)
    u32 = C.units(y32, ref64, scale)
    bar = _bar(c, u32)
    print(f"\n[conv-edges] {c.name}: u = {u:.2f}, u32 = {u32:.2f}, bar = {bar:.2f}, "
          f"u / bar = {u / bar:.3f}")
    assert u <= bar, (c.name, u, u32, bar)


def _weights(c, d):
    """Packed weight, its padded rows, the x3 planes (or None)."""
    w = d["w"].to(DEV)
    if c.kind == "convt":
        wp, cout_pad = ops.pack_convt1d_weight(w, c.stride)
        return wp, cout_pad, ops.pack_x3_weight(wp, 2) if c.x3 else None
    wp, cout_pad = ops.pack_conv1d_weight(w)
    w3 = None
    if c.x3:
        w3 = ops.pack_x3_strided_weight(w, c.stride) if c.stride > 1 else \
            ops.pack_x3_weight(wp, c.k)
    return wp, cout_pad, w3


def _launch(c, d, dev, want_y):
    """One launch of a conv / proj / convt case on guarded buffers; returns the buffers."""
    B, tout = c.B, C.out_len(c)
    wp, cout_pad, w3 = dev["w"]
    n = B * c.cout * tout
    y = Guarded(n) if want_y else None
    ys = Guarded(n) if c.out_snake else None
    x = Guarded(B * c.cin * c.tin, d["x"])
    res = Guarded(n, d["res"]) if c.res else None
    alpha, inv = (dev["alpha"], dev["inv"]) if c.snake else (None, None)
    ao, io = (dev["alpha_out"], dev["inv_out"]) if c.out_snake else (None, None)
    bias = dev["b"] if c.bias else None
    lib = _lib.load()
    ws, need, part = None, 0, None
    before = _mark_record()
    if c.kind == "convt":
        rc = lib.vrvq_conv_transpose1d_pad(P(x.t), B, c.cin, c.tin, P(alpha), P(inv), P(wp), P(w3),
                                           c.cout, cout_pad, c.stride, c.pad, P(bias),
                                           P(y.t) if y else None, P(ao), P(io),
                                           P(ys.t) if ys else None, None)
    else:
        nb = ctypes.c_longlong(0)
        _lib.call("vrvq_conv1d_workspace", B, c.cin, c.tin, c.cout, c.k, c.stride, c.pad, c.dil,
                  1 if c.x3 else 0, ctypes.byref(nb))
        need = nb.value // 4
        assert nb.value % 4 == 0 and (need > 0) == (C.plan_of(c)["S"] > 0)
        ws = Guarded(need + 1024)
        if c.kind == "proj":
            part = Guarded(8 * B * tout * 64)
            rc = lib.vrvq_conv1d_proj(P(x.t), B, c.cin, c.tin, P(alpha), P(inv), P(wp), P(w3),
                                      c.cout, cout_pad, c.k, c.pad, c.dil, P(bias),
                                      P(y.t) if y else None, tout, P(dev["w3in"]), 8, P(part.t),
                                      P(ws.t), ws.n * 4, None)
        else:
            rc = lib.vrvq_conv1d_ws(P(x.t), B, c.cin, c.tin, P(alpha), P(inv), P(wp), P(w3), c.cout,
                                    cout_pad, c.k, c.stride, c.pad, c.dil, P(bias),
                                    P(res.t) if res else None, c.epi, P(y.t) if y else None, tout,
                                    P(ao), P(io), P(ys.t) if ys else None, P(ws.t), ws.n * 4, None)
    assert rc == 0, (c.name, rc)
    torch.cuda.synchronize()
    _check_record(c, before)                                   # (a)
    for name, buf in (("y", y), ("y_snake", ys), ("partials", part)):   # (c)
        if buf is not None:
            buf.check(f"{c.name} {name}")
    if ws is not None:
        ws.check(f"{c.name} workspace", written=need)
    shape = (B, c.cout, tout)
    return types.SimpleNamespace(y=y.t.view(shape) if y else None,
                                 ys=ys.t.view(shape) if ys else None,
                                 part=part.t.view(8, B * tout, 64) if part else None)


def _device_side(c, d):
    dev = {k: d[k].to(DEV) for k in ("alpha", "alpha_out", "b")}
    dev["inv"] = ops.snake_inv_alpha(dev["alpha"])
    dev["inv_out"] = ops.snake_inv_alpha(dev["alpha_out"])
    dev["w"] = _weights(c, d)
    return dev


def run_case(c):
    d = C.inputs(c)
    ref = C.reference(c, d)
    dev = _device_side(c, d)
    if c.kind == "proj":
        return _run_proj(c, d, dev, ref)
    out = _launch(c, d, dev, want_y=True)
    _judge(c, out.y, ref)                                      # (b)
    if c.out_snake:
        assert rel_err(out.ys.cpu().numpy(),
                       _snake_dev(out.y, dev["alpha_out"]).cpu().numpy()) < 1e-6
        if not c.want_raw:   # y = NULL: the same Snake bits, no y
            alone = _launch(c, d, dev, want_y=False)
            assert alone.y is None and torch.equal(alone.ys, out.ys), c.name


def _run_proj(c, d, dev, ref):
    """The partials equal vrvq_rvq_project's on the launch's own z bit for bit, z equals the
    plain conv's and meets the bar (y = NULL: the partials of the plain conv's z)."""
    from test_gpu_rvq_part import _project
    g = torch.Generator(device="cpu").manual_seed(C._seed(c) ^ 0x5A5A)
    st = types.SimpleNamespace(w_in_t=(torch.randn(8, 1024, 8, generator=g) * 0.1).to(DEV),
                               b_in=torch.zeros(8, 8, device=DEV))
    dev["w3in"] = ops.rvq_pack_w_in(st.w_in_t)
    plain = _launch(c._replace(kind="conv"), d, dev, want_y=True)
    _judge(c, plain.y, ref)
    out = _launch(c, d, dev, want_y=c.want_raw)
    if c.want_raw:
        assert torch.equal(out.y, plain.y), c.name
    want = _project(plain.y.contiguous(), st)
    torch.cuda.synchronize()
    assert torch.equal(out.part, want), c.name


def _ids(group):
    return [pytest.param(c, id=c.name) for c in C.group(group)]


@pytest.mark.parametrize("c", _ids("plan"))
def test_every_plan_per_element(c):
    """One case per plan the dispatch can choose, at the plan's edges."""
    run_case(c)


@pytest.mark.parametrize("c", _ids("epilogue"))
def test_every_epilogue_variant(c):
    """Each tile's epilogue with 16-byte stores, residual, activation, the next Snake, y = NULL."""
    run_case(c)


@pytest.mark.parametrize("c", _ids("convt"))
def test_conv_transpose_walks(c):
    """The vector (strides 2, 4, 8) and generic (3, 6) walks: pad 0 and (s + 1) // 2, one
    input sample, a ragged last tile."""
    run_case(c)


@pytest.mark.parametrize("c", _ids("off"))
def test_kernels_off_the_mfma_tiles(c):
    """Cin = 1 stream kernel and its MFMA fallback, the Cout = 1 stream kernel's `interior`
    switch at its boundaries, the small-Cout kernel across its 256-sample blocks."""
    run_case(c)


@pytest.mark.parametrize("c", _ids("ru"))
def test_residual_unit_per_element(c):
    """vrvq_residual_unit around every unit's time tile, with and without x3 planes, y wanted
    or not: bar, guards and the next layer's Snake as for the convs."""
    d = C.inputs(c)
    ref = C.reference(c, d)
    Cn, T, B = c.cin, c.tin, c.B
    w7, cout_pad = ops.pack_conv1d_weight(d["w"].to(DEV))
    w1, _ = ops.pack_conv1d_weight(d["w1"].to(DEV))
    w7x3 = ops.pack_x3_weight(w7, 7) if c.x3 else None
    w1x3 = ops.pack_x3_weight(w1, 1) if c.x3 else None
    b7, b1 = d["b"].to(DEV), d["b1"].to(DEV)
    a2, ao = d["alpha2"].to(DEV), d["alpha_out"].to(DEV)
    i2, io = ops.snake_inv_alpha(a2), ops.snake_inv_alpha(ao)
    x, xs = Guarded(B * Cn * T, d["x"]), Guarded(B * Cn * T, d["x_snk"])

    def launch(want_y):
        y = Guarded(B * Cn * T) if want_y else None
        ys = Guarded(B * Cn * T)
        rc = _lib.load().vrvq_residual_unit(
            P(x.t), P(xs.t), B, Cn, T, c.dil, P(w7), P(w7x3), P(w1x3), P(b7), P(a2), P(i2), P(w1),
            P(b1), cout_pad, P(y.t) if y else None, P(ao), P(io), P(ys.t), None)
        assert rc == 0, (c.name, rc)
        torch.cuda.synchronize()
        for name, buf in (("y", y), ("y_snake", ys)):
            if buf is not None:
                buf.check(f"{c.name} {name}")
        return (y.t.view(B, Cn, T) if y else None), ys.t.view(B, Cn, T)

    y, ys = launch(True)
    _judge(c, y, ref)
    assert rel_err(ys.cpu().numpy(), _snake_dev(y, ao).cpu().numpy()) < 1e-6
    if not c.want_raw:
        none, ys2 = launch(False)
        assert none is None and torch.equal(ys2, ys), c.name


# ------------------------------------------------------------------ (d) the six x3 products
def _exact(shape, g):
    """2^e (1 + 2^-9 + 2^-17), e in -3..3: bf16 planes 2^e, 2^(e-9), 2^(e-17), all positive."""
    e = torch.randint(-3, 4, shape, generator=g)
    return torch.ldexp(torch.full(shape, 1 + 2.0 ** -9 + 2.0 ** -17), e.to(torch.int32))


# name, kind, B, cin, tin, cout, k, stride, pad, live channel ranges (None: all), the plan
# (BM, BN, KS, x3, S)
X3_PRODUCT_CASES = [
    ("k1_plain", "conv", 1, 32, 70, 200, 1, 1, 0, None, (128, 32, 1, 1, 0)),
    ("k3_plain", "conv", 1, 16, 70, 200, 3, 1, 1, None, (128, 32, 3, 1, 0)),
    ("k7_plain", "conv", 1, 8, 70, 200, 7, 1, 3, None, (128, 32, 7, 1, 0)),
    ("k7_pair_64x256", "conv", 1, 16, 641, 128, 7, 1, 3, None, (64, 256, 7, 2, 0)),
    ("view_2tap_plain", "conv", 1, 8, 140, 200, 4, 2, 1, None, (128, 32, 2, 1, 0)),
    ("view_2tap_pair", "conv", 1, 16, 140, 200, 4, 2, 1, None, (128, 32, 2, 2, 0)),
    ("convt_2tap_plain", "convt", 1, 16, 29, 100, 4, 2, 1, None, (128, 32, 2, 1, 0)),
    ("convt_2tap_pair", "convt", 1, 32, 29, 100, 4, 2, 1, None, (128, 32, 2, 2, 0)),
    # split-K: 16 chunks in two parts of 8; the first chunk of each part is live (K = 96 / 112
    # live products, 36 / 48 MFMA accumulations that add a non-zero term), the rest zero
    ("splitk_k3", "conv", 1, 256, 87, 128, 3, 1, 1, ((0, 16), (128, 144)), (128, 96, 3, 1, 2)),
    ("splitk_k7", "conv", 1, 128, 87, 128, 7, 1, 3, ((0, 8), (64, 72)), (128, 96, 7, 1, 2)),
]


@pytest.mark.parametrize("case", X3_PRODUCT_CASES, ids=[c[0] for c in X3_PRODUCT_CASES])
def test_x3_six_products(case):
    """conv_x3.h keeps six of the nine bf16 plane products. One K chunk deep (K <= 112 live
    products per output, pad channels zero), no Snake, bias or residual, every operand
    2^e (1 + 2^-9 + 2^-17): all three planes positive and exactly known, so nothing cancels.
    In plane arithmetic the correct six-term sum is 0.5 unit of 2^-24 of the result off and
    leaving out any one kept product moves it by >= 64 units (m m 64, h l / l h 128, h m / m h
    3.3e4); the bar of 32 units leaves room for at most 42 accumulator roundings of half a unit."""
    name, kind, B, cin, tin, cout, k, s, pad, live, want = case
    c = C.case(name, "x3", kind, B, cin, tin, cout, k, s, pad, 1, x3=True, ws=True, snake=False,
               bias=False)
    plan = C.plan_of(c)
    assert tuple(plan[n] for n in KEYS) == want
    g = torch.Generator(device="cpu").manual_seed(len(name) * 131 + cin)
    x = _exact((B, cin, tin), g)
    w = _exact((cin, cout, k) if kind == "convt" else (cout, cin, k), g)
    dead = torch.ones(cin, dtype=torch.bool)
    for lo, hi in (live or ((0, cin),)):
        dead[lo:hi] = False
    assert kind == "conv" or not bool(dead.any())
    if kind == "conv":      # w is (cout, cin, k)
        x[:, dead] = 0.0
        w[:, dead] = 0.0
    assert int((~dead).sum()) * (2 if s > 1 else k) <= 112   # k = 2 s: two taps per output
    d = dict(x=x, w=w, alpha=torch.ones(cin), alpha_out=torch.ones(cout), b=torch.zeros(cout))
    out = _launch(c, d, _device_side(c, d), want_y=True)
    ref64 = C._conv(c, x.double(), w.double(), None)
    got = out.y.cpu().double()
    assert bool((ref64 > 0).all())
    u = float(((got - ref64).abs() / (C.UNIT * ref64)).max())
    print(f"\n[conv-edges] x3 products {name}: u = {u:.2f}, bar = 32")
    assert u <= 32, (name, u)
