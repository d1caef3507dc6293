"""Backward kernels of the training step (csrc/train.hip, the backward branches of
csrc/torch_ops.cpp) judged per element against torch fp64 on the CPU, at the edges of every path:

  A  wgrad_kernel (the fp32-input MFMA weight gradient) through the C ABI: every tap-group size,
     the 64 / 32 / 16-sample time chunks, two tap groups, partial tiles, dilation under a stride;
  B  the phase-split weight gradient of ops.conv1d_wgrad (vrvq_phase_split + the 2-tap x3 kernel
     + a permute) against fp64 and against A's result for the same inputs; vrvq_phase_split alone,
     bit for bit;
  D  snake_backward / bias_grad / act_backward / weight_norm_backward at the chunking edges.

(C and E, the stride-1 x3 weight gradients and the input gradients of the adjoint convs, are in
test_gpu_train.py, beside the tests they tighten.)

Bars. GEMM-like results (dW): e = rel_err (max-abs difference over max-abs of the fp64
reference) must be < 1e-5 and <= 4 e32 + 2e-7, e32 the same operation in torch fp32 on the CPU
(the convention of test_conv1d_x3_vs_torch). Per-channel reductions (dalpha, db, dg): per output
element |got - ref64| <= 64 * 2^-24 * S, S the fp64 sum of the absolute values of the element's
terms -- the worst-case rounding of at most 16 serial adds per thread in a 4096-sample chunk
(42 at cols = 10752), 8 tree levels, at most 9 split partials and a few ulp for sine and cosine.
Pure elementwise outputs: rel_err < 1e-6. Every case prints its figures."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from vrvq_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS24 = 2.0 ** -24
RED_ULPS = 64.0


# ------------------------------------------------------------------ references and bars
def snake(x, alpha):
    """Snake1d in x's own precision (fp64 reference / fp32 yardstick)."""
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


def gemm_bar(tag, got, ref64, ref32):
    e, e32 = rel_err(got.numpy(), ref64.numpy()), rel_err(ref32.numpy(), ref64.numpy())
    print(f"{tag}: e={e:.3e} e32={e32:.3e} bar={min(1e-5, 4 * e32 + 2e-7):.3e}")
    assert e < 1e-5, f"{tag}: e {e:.3e}"
    assert e <= 4 * e32 + 2e-7, f"{tag}: e {e:.3e} > 4 * {e32:.3e} + 2e-7"
    return e


def reduction_bar(tag, got, ref64, s_abs):
    """|got - ref64| <= 64 * 2^-24 * S per element (S: fp64 sum of |terms|)."""
    margin = RED_ULPS * EPS24 * s_abs
    diff = (got.double() - ref64).abs()
    used = float((diff / margin.clamp_min(1e-300)).max())
    print(f"{tag}: worst |got - ref| = {used * RED_ULPS:.2f} x 2^-24 S (bar {RED_ULPS:.0f})")
    bad = (diff > margin).nonzero()
    assert bad.numel() == 0, (f"{tag}: {bad.shape[0]} elements over the bar, first {bad[0].tolist()}"
                              f" diff {float(diff[tuple(bad[0])]):.3e}")


def P(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def cur_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ A / B: weight gradients
# (B, M, C, k, stride, pad, dil, TX); a is (B, M, TA), x is (B, C, TX)
WGRAD_CASES = [
    # kg = 4: W = 63 * 2 + 3 * 1 + 1 = 130 <= WG_WMAX = 192 -> 64-sample chunks, one tap group;
    # TA = 65: a full chunk and a one-sample one per clip
    (2, 70, 33, 4, 2, 1, 1, 131),
    # kg = 8: 63 * 4 + 7 + 1 = 260 > 192, 31 * 4 + 7 + 1 = 132 <= 192 -> kt_sh = 5 (32-sample
    # chunks), one tap group; TA = 67: three chunks per clip, the last of 3 samples
    (3, 64, 64, 8, 4, 2, 1, 270),
    # k = 16 -> kg = 8, two tap groups; 31 * 8 + 7 + 1 = 256 > 192, 15 * 8 + 7 + 1 = 128 <= 192
    # -> kt_sh = 4 (16-sample chunks); TA = 37: three chunks per clip, the last of 5 samples
    (2, 40, 24, 16, 8, 4, 1, 300),
    (1, 8, 130, 3, 2, 1, 1, 50),      # KG 3, one clip, three C tiles
    (2, 33, 8, 7, 2, 3, 1, 77),       # KG 7
    (2, 16, 16, 5, 2, 2, 1, 64),      # KG 1, five tap groups
    (2, 16, 16, 2, 2, 0, 1, 64),      # KG 2, no padding
    (2, 64, 64, 7, 2, 9, 3, 200),     # dilation 3 under a stride
    (2, 32, 16, 6, 3, 2, 1, 100),     # stride 3 (KG 1, six tap groups): the torch op's own route
]
CONVT_CASE = (2, 40, 24, 8, 4, 2, 1, 76)  # ConvTranspose orientation: a the layer input, TA = 19
SNAKE_CASES = WGRAD_CASES[:3] + [WGRAD_CASES[7]]
ids = lambda c: "-".join(map(str, c))  # noqa: E731


def out_frames(case):
    _, _, _, k, s, p, d, tx = case
    return (tx + 2 * p - d * (k - 1) - 1) // s + 1


@functools.lru_cache(maxsize=None)
def wgrad_inputs(case):
    B, M, C, k, s, p, d, TX = case
    g0 = torch.Generator().manual_seed(sum(case) + 1000 * k)
    a = torch.randn(B, M, out_frames(case), generator=g0)
    x = torch.randn(B, C, TX, generator=g0)
    al_a = torch.rand(M, generator=g0) + 0.5
    al_x = torch.rand(C, generator=g0) + 0.5
    return a, x, al_a, al_x


@functools.lru_cache(maxsize=None)
def wgrad_refs(case, mode):
    """(fp64 reference, torch fp32 CPU result) of the weight gradient; mode: which operands carry
    a Snake ("none", "a", "x", "both")."""
    B, M, C, k, s, p, d, TX = case
    a, x, al_a, al_x = wgrad_inputs(case)
    out = []
    for dt in (torch.float64, torch.float32):
        aa, xx = a.to(dt), x.to(dt)
        if mode in ("a", "both"):
            aa = snake(aa, al_a.to(dt)[None, :, None])
        if mode in ("x", "both"):
            xx = snake(xx, al_x.to(dt)[None, :, None])
        out.append(torch.nn.grad.conv1d_weight(xx, (M, C, k), aa, s, p, d))
    return tuple(out)


def c_abi_wgrad(case, mode, n_split=None):
    """vrvq_wgrad_plan + vrvq_conv1d_wgrad (n_split: override the plan's, workspace sized for it).
    The workspace is poisoned: a partial the kernels do not write must not be read either."""
    B, M, C, k, s, p, d, TX = case
    a, x, al_a, al_x = (v.to(DEV) for v in wgrad_inputs(case))
    ta = a.shape[-1]
    inv_a, inv_x = ops.snake_inv_alpha(al_a), ops.snake_inv_alpha(al_x)
    if mode not in ("a", "both"):
        al_a = inv_a = None
    if mode not in ("x", "both"):
        al_x = inv_x = None
    split, ws_bytes = ctypes.c_int(0), ctypes.c_longlong(0)
    _lib.call("vrvq_wgrad_plan", B, M, ta, C, k, ctypes.byref(split), ctypes.byref(ws_bytes))
    ns = split.value
    assert ws_bytes.value == ns * M * C * k * 4
    if n_split is not None:
        ns = n_split
    ws = torch.full((ns * M * C * k,), float("nan"), device=DEV)
    out = torch.full((M, C, k), float("nan"), device=DEV)
    _lib.call("vrvq_conv1d_wgrad", P(a), B, M, ta, P(al_a), P(inv_a), P(x), C, TX, P(al_x),
              P(inv_x), k, s, p, d, ns, P(ws), ws.numel() * 4, P(out), cur_stream())
    torch.cuda.synchronize()
    return out.cpu(), ns


@functools.lru_cache(maxsize=None)
def c_abi_result(case, mode):
    return c_abi_wgrad(case, mode)[0]


@pytest.mark.parametrize("case", WGRAD_CASES + [CONVT_CASE], ids=ids)
def test_wgrad_kernel_c_abi_vs_torch64(case):
    """wgrad_kernel (stride > 1 always takes it from the C ABI), both alphas null."""
    assert case[4] > 1
    gemm_bar(f"wgrad_kernel {case}", c_abi_result(case, "none"), *wgrad_refs(case, "none"))


@pytest.mark.parametrize("case", SNAKE_CASES, ids=ids)
def test_wgrad_kernel_c_abi_in_kernel_snake_vs_torch64(case):
    """The same with alpha and alpha_a set (Snake applied while staging), against the fp64
    gradient of the Snake'd operands."""
    gemm_bar(f"wgrad_kernel snake {case}", c_abi_result(case, "both"), *wgrad_refs(case, "both"))


def test_wgrad_kernel_n_split_past_chunks():
    """n_split larger than the (clip, time chunk) count: clamped by the host code, the workspace
    sized for the passed value, the same bits as under the plan's own split."""
    case = WGRAD_CASES[0]                      # 2 clips x 2 chunks of 64 samples = 4 units
    chunks = case[0] * ((out_frames(case) + 63) // 64)
    want = c_abi_result(case, "none")
    got, ns = c_abi_wgrad(case, "none", n_split=10 * chunks)
    assert ns > chunks
    assert torch.equal(got, want)
    got1, _ = c_abi_wgrad(case, "none", n_split=1)  # and a single split is within the bar too
    gemm_bar(f"wgrad_kernel n_split=1 {case}", got1, *wgrad_refs(case, "none"))


def torch_op_wgrad(case, mode):
    B, M, C, k, s, p, d, TX = case
    a, x, al_a, al_x = (v.to(DEV) for v in wgrad_inputs(case))
    sa = (al_a, ops.snake_inv_alpha(al_a)) if mode in ("a", "both") else None
    sx = (al_x, ops.snake_inv_alpha(al_x)) if mode in ("x", "both") else None
    return ops.conv1d_wgrad(a, x, k, s, p, d, snake_a=sa, snake_x=sx).cpu()


PHASE_CASES = ([(c, m) for c in WGRAD_CASES[:3] for m in ("none", "x")]
               + [((1, 16, 3, 4, 2, 0, 1, 37), "none"), ((1, 16, 3, 4, 2, 0, 1, 37), "x"),
                  (CONVT_CASE, "a")])


@pytest.mark.parametrize("case,mode", PHASE_CASES, ids=lambda v: v if isinstance(v, str) else ids(v))
def test_phase_split_wgrad_vs_torch64_and_fp32_kernel(case, mode):
    """ops.conv1d_wgrad on k = 2 s layers (the phase-split path: vrvq_phase_split, the 2-tap x3
    kernel over C s virtual channels with TV = TA + 1, a permute) against fp64, and against the
    fp32 kernel's result for the same inputs within the sum of the two measured errors."""
    B, M, C, k, s, p, d, TX = case
    assert k == 2 * s and d == 1
    ref64, ref32 = wgrad_refs(case, mode)
    got = torch_op_wgrad(case, mode)
    assert got.shape == ref64.shape
    e_b = gemm_bar(f"phase wgrad {case} {mode}", got, ref64, ref32)
    kern = c_abi_result(case, mode)
    e_a = gemm_bar(f"  fp32 kernel {case} {mode}", kern, ref64, ref32)
    scale = float(ref64.abs().max())
    cross = float((got.double() - kern.double()).abs().max()) / scale
    print(f"  phase vs fp32 kernel: {cross:.3e} (e_a + e_b = {e_a + e_b:.3e})")
    assert cross <= e_a + e_b


def test_torch_op_stride3_takes_fp32_kernel():
    """Stride 3 is no power of two: the torch op runs wgrad_kernel too, with the same bits as
    the C ABI, the Snake applied up front."""
    case = WGRAD_CASES[8]
    got = torch_op_wgrad(case, "none")
    assert torch.equal(got, c_abi_result(case, "none"))
    gemm_bar(f"torch op stride 3 snake {case}", torch_op_wgrad(case, "x"), *wgrad_refs(case, "x"))


@pytest.mark.parametrize("with_alpha", [False, True], ids=["plain", "snake"])
@pytest.mark.parametrize("shape", [(2, 3, 37, 2, 0), (2, 5, 131, 4, 2), (1, 8, 300, 8, 4)], ids=ids)
def test_phase_split_bit_exact(shape, with_alpha):
    """vrvq_phase_split: xv[c s + r][m] = snake(x)[c][m s + r - pad], zero outside [0, T), with
    TV = Tout + 1 columns (k = 2 s); snake(x) from vrvq_snake, bit for bit."""
    B, C, T, s, pad = shape
    tv = (T + 2 * pad - 2 * s) // s + 1 + 1
    g0 = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, C, T, generator=g0).to(DEV)
    al = (torch.rand(C, generator=g0) + 0.5).to(DEV)
    inv = ops.snake_inv_alpha(al)
    xs = x
    if with_alpha:
        xs = torch.empty_like(x)
        _lib.call("vrvq_snake", P(x), B, C, T, P(al), P(inv), P(xs), cur_stream())
    xv = torch.full((B, C * s, tv), float("nan"), device=DEV)
    _lib.call("vrvq_phase_split", P(x), B, C, T, s, pad, tv, P(al if with_alpha else None),
              P(inv if with_alpha else None), P(xv), cur_stream())
    torch.cuda.synchronize()
    xs = xs.cpu()
    t = (torch.arange(tv)[None, :] * s + torch.arange(s)[:, None]) - pad       # [r][m]
    inside = (t >= 0) & (t < T)
    want = torch.where(inside, xs[:, :, t.clamp(0, T - 1)], torch.zeros(()))   # (B, C, s, tv)
    assert int((~inside).sum()) > 0 or pad == 0
    assert torch.equal(xv.cpu(), want.reshape(B, C * s, tv))


# ------------------------------------------------------------------ D: elementwise / reductions
BCT = [(3, 5, 4097), (2, 3, 8200), (1, 1, 1), (2, 300, 7)]


def bct_inputs(shape):
    B, C, T = shape
    g0 = torch.Generator().manual_seed(B * 1000 + C * 10 + T)
    x = torch.randn(B, C, T, generator=g0)
    g = torch.randn(B, C, T, generator=g0)
    alpha = torch.rand(C, generator=g0) + 0.5
    return x, g, alpha


@pytest.mark.parametrize("shape", BCT, ids=ids)
def test_snake_backward_direct(shape):
    """snake_backward_kernel at T just above RCH = 4096 (a one-sample last chunk), a ragged third
    chunk, a single element and many short rows: dx per element, dalpha at the reduction bar,
    against the closed forms of train.hip in fp64 (checked against fp64 autograd)."""
    x, g, alpha = bct_inputs(shape)
    x64, g64, a64 = x.double(), g.double(), alpha.double()[None, :, None]
    inv = 1.0 / (a64 + 1e-9)
    sn, cs = torch.sin(a64 * x64), torch.cos(a64 * x64)
    dx64 = g64 * (1.0 + inv * (2.0 * sn * cs) * a64)
    terms = g64 * (-(inv * inv) * sn * sn + inv * (2.0 * sn * cs) * x64)
    xa, aa = x.double().requires_grad_(), alpha.double().requires_grad_()
    snake(xa, aa[None, :, None]).backward(g64)
    assert rel_err(dx64.numpy(), xa.grad.numpy()) < 1e-12
    assert rel_err(terms.sum((0, 2)).numpy(), aa.grad.numpy()) < 1e-9
    xd, gd, ad = x.to(DEV), g.to(DEV), alpha.to(DEV)
    invd = ops.snake_inv_alpha(ad)
    dx, da = ops.snake_backward(xd, ad, invd, gd)
    e = rel_err(dx.cpu().numpy(), dx64.numpy())
    print(f"snake_backward {shape}: dx e={e:.3e}")
    assert e < 1e-6
    reduction_bar(f"snake_backward {shape} dalpha", da.cpu(), terms.sum((0, 2)),
                  terms.abs().sum((0, 2)))
    if shape == BCT[0]:
        none, da2 = ops.snake_backward(xd, ad, invd, gd, want_dx=False)
        assert none is None
        assert torch.equal(da2, da)


@pytest.mark.parametrize("shape", BCT, ids=ids)
def test_bias_grad_direct(shape):
    g = bct_inputs(shape)[1]
    db = ops.bias_grad(g.to(DEV))
    reduction_bar(f"bias_grad {shape}", db.cpu(), g.double().sum((0, 2)), g.double().abs().sum((0, 2)))


@functools.lru_cache(maxsize=None)
def act_inputs():
    n = 65536 * 256 + 5
    g0 = torch.Generator().manual_seed(11)
    return torch.rand(n, generator=g0), torch.randn(n, generator=g0)


@pytest.mark.parametrize("epi", [ops.EPI_TANH, ops.EPI_SIGMOID], ids=["tanh", "sigmoid"])
@pytest.mark.parametrize("n", [1, 257, 65536 * 256 + 5])
def test_act_backward_direct(n, epi):
    """act_backward_kernel from the stored output y; the last size is five elements past the
    65536-block cap of its grid, so the grid-stride loop wraps."""
    u, g = (v[-n:] for v in act_inputs())
    y = 2.0 * u - 1.0 if epi == ops.EPI_TANH else u
    y64, g64 = y.double(), g.double()
    ref = g64 * (1.0 - y64 * y64) if epi == ops.EPI_TANH else g64 * (y64 * (1.0 - y64))
    out = ops.act_backward(y.to(DEV), g.to(DEV), epi).cpu()
    e = rel_err(out.numpy(), ref.numpy())
    print(f"act_backward n={n} epi={epi}: e={e:.3e}")
    assert e < 1e-6
    # per element too (the max-abs measure alone passes a wrong element where |g| is small):
    # three roundings of factors <= 1 times g, so 4 x 2^-24 |g| bounds a correct result
    assert bool(((out.double() - ref).abs() <= 4 * EPS24 * g64.abs()).all())


@pytest.mark.parametrize("rows,cols", [(1, 1), (5, 7), (3, 256), (2, 257), (4, 10752)])
def test_weight_norm_backward_direct(rows, cols):
    """weight_norm_backward_kernel with fewer columns than threads, a ragged second pass and 42
    passes, against fp64 autograd of torch._weight_norm."""
    g0 = torch.Generator().manual_seed(rows * 100003 + cols)
    v = torch.randn(rows, cols, generator=g0) * 0.1
    g = torch.rand(rows, generator=g0) + 0.5
    dw = torch.randn(rows, cols, generator=g0)
    v64, g64 = v.double().requires_grad_(), g.double().requires_grad_()
    torch._weight_norm(v64, g64[:, None], 0).backward(dw.double())
    dg, dv = ops.weight_norm_backward(g.to(DEV), v.to(DEV), dw.to(DEV))
    n64 = v.double().norm(dim=1)
    s_abs = (dw.double() * v.double()).abs().sum(1) / n64
    reduction_bar(f"weight_norm_backward ({rows}, {cols}) dg", dg.cpu(), g64.grad, s_abs)
    if cols == 1:
        # dv of a one-element row is exactly zero (the two terms g dw / n cancel): max-abs of
        # the reference is no scale, so the difference is measured against the terms' size
        scale = (g.double() * dw.double()[:, 0] / n64).abs().max()
        e = float(dv.cpu().double().abs().max() / scale)
        assert float(v64.grad.abs().max()) <= 1e-15 * float(scale)
    else:
        e = rel_err(dv.cpu().numpy(), v64.grad.numpy())
    print(f"weight_norm_backward ({rows}, {cols}): dv e={e:.3e}")
    assert e < 1e-5
