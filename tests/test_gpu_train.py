"""Training step on the MI355X: generator gradients of the HIP autograd
path (vrvq_amd/train.py) against

  - fixtures from the reference's own autograd (tests/golden/make_golden.py train_fixture:
    vrvq_a2, 28 codebooks, 0.38 s clips, seeded training-mode quantizer, surrogate loss
    L = mean|audio - x| + 0.25 commitment + codebook + 2 mean(imp_map));
  - torch fp64 autograd restatements of each backward operator (conv / ConvT / Snake / weight
    norm / activations, the mask STE and the quantizer with the straight-through estimator).

Bar: seed-controlled draws bit-exact, codes bit-exact, every gradient tensor within 1e-4
relative (L2 norm of the difference over the L2 norm of the reference, per tensor); the weight
gradients and the adjoint convs' input gradients also per element (fp32_bar: max-abs below 1e-5
and within 4x torch fp32's own error + 2e-7). The backward kernels' shape edges are in
test_gpu_backward_edges.py.

The quantizer's bars: here, the three gradient sources added (dL/dz_q + 0.25 commitment +
codebook), each gradient as one tensor at 1e-4 L2 (test_rvq_backward_vs_torch64, the module-level
tests, the generator fixtures) -- the whole-path and reference-parity checks. Per source, per
stage and per element (4 e32 + 2e-7, exact zeros, the codebook gradient's reduction bar, nq = 1 /
8 / 32 / 33, N = 256 / 768, decaying residuals, many hits per row) and the mask STE per element
are in test_gpu_rvq_backward.py; the fp64 loop `rvq64` and `logcosh64` used here live with those
references in rvq_grad_ref.py."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rvq_ref as R
import vrvq_amd
from rvq_grad_ref import logcosh64, rvq64
from conftest import load_golden, rel_err
from vrvq_amd import ops, train
from vrvq_amd.recipe import load_recipe

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def l2rel(a, b):
    a = np.asarray(a, np.float64).reshape(-1)
    b = np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------ torch fp64 references
def snake64(x, alpha):
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


def wn64(g, v):
    return torch._weight_norm(v, g, 0)


CONV_CASES = [
    # kind, cin, cout, k, stride, pad, dil, snake, residual, epi, T
    ("conv", 64, 64, 7, 1, 9, 3, True, False, 0, 300),
    ("conv", 96, 96, 1, 1, 0, 1, True, True, 0, 257),
    ("conv", 1, 64, 7, 1, 3, 1, False, False, 0, 400),
    ("conv", 64, 128, 4, 2, 1, 1, True, False, 0, 256),
    ("conv", 128, 256, 16, 8, 4, 1, True, False, 0, 512),
    ("conv", 512, 1, 3, 1, 1, 1, True, False, 2, 40),
    ("conv", 96, 1, 7, 1, 3, 1, True, False, 1, 333),
    ("convt", 256, 128, 16, 8, 4, 1, True, False, 0, 40),
    ("convt", 192, 96, 4, 2, 1, 1, True, False, 0, 100),
    ("convt", 384, 192, 8, 4, 2, 1, True, False, 0, 64),
    ("conv", 33, 70, 7, 1, 9, 3, True, False, 0, 65),      # flipped-weight adjoint, ragged channels
    ("conv", 1, 64, 7, 1, 3, 1, False, False, 0, 401),     # adjoint: one output channel, a length
                                                           # the stream kernel declines
    ("convt", 40, 24, 8, 4, 2, 1, True, False, 0, 19),
]


# Margin over e32 of the per-element dx / dv bar where it is not 4. The 512 -> 1 k3 + Sigmoid layer
# runs its FORWARD on the Cout = 1 kernels of conv.hip, one serial chain of cin k = 1536 fmaf per
# output, where torch's blocked fp32 sum keeps chains 16x shorter (~4x less rounding): measured
# forward pre-activation e = 1.48e-6 against e32 = 1.48e-7. The backward differentiates through the
# stored y, so gy (1 - y) y inherits it: dx e = 1.07e-6 at e32 = 1.83e-7 (4 e32 + 2e-7 = 9.3e-7).
# The backward kernels themselves are at fp32's error there: act_backward 7.0e-8 against fp64 of
# the kernel's own y, the adjoint conv on the exact gy 1.14e-7 (torch fp32: 1.32e-7). Hence 4 x 4
# for dx; dv (e = 7.1e-7 at e32 = 3.4e-7) sums the same gy over time and keeps 4.
GRAD_MARGIN = {("dx", ("conv", 512, 1, 3, 1, 1, 1, True, False, 2, 40)): 16}


def fp32_bar(tag, got, ref64, ref32, margin=4):
    """Per element: e = max-abs difference over max-abs of the fp64 reference, below 1e-5 and
    within 4x the error of the same operation in torch fp32 on the CPU + 2e-7 (the forward
    convs' bar, test_conv1d_x3_vs_torch)."""
    e, e32 = rel_err(got.cpu().numpy(), ref64.numpy()), rel_err(ref32.numpy(), ref64.numpy())
    print(f"{tag}: e={e:.3e} e32={e32:.3e}")
    assert e < 1e-5, f"{tag}: e {e:.3e}"
    assert e <= margin * e32 + 2e-7, f"{tag}: e {e:.3e} > {margin} * {e32:.3e} + 2e-7"


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_snake_conv_grads_vs_torch64(case):
    kind, cin, cout, k, s, p, d, use_snake, use_res, epi, T = case
    g0 = torch.Generator().manual_seed(17)
    B = 2
    x = torch.randn(B, cin, T, generator=g0)
    alpha = torch.rand(cin, generator=g0) + 0.5
    if kind == "conv":
        v = torch.randn(cout, cin, k, generator=g0) * 0.1
        g = torch.rand(cout, generator=g0) + 0.5
    else:
        v = torch.randn(cin, cout, k, generator=g0) * 0.1
        g = torch.rand(cin, generator=g0) + 0.5
    bias = torch.randn(cout, generator=g0) * 0.1

    def ref(x, alpha, g, v, bias, res):
        xs = snake64(x, alpha[None, :, None]) if use_snake else x
        w = wn64(g.reshape(-1, 1, 1), v)
        if kind == "conv":
            y = F.conv1d(xs, w, bias, s, p, d)
        else:
            y = F.conv_transpose1d(xs, w, bias, stride=s, padding=p)
        if res is not None:
            y = y + res
        return torch.tanh(y) if epi == 1 else (torch.sigmoid(y) if epi == 2 else y)

    leaves64 = [a.double().requires_grad_() for a in (x, alpha, g, v, bias)]
    with torch.no_grad():
        tout = ref(*[a.double() for a in (x, alpha, g, v, bias)], None).shape[-1]
    res = torch.randn(B, cout, tout, generator=g0) if use_res else None
    res64 = res.double().requires_grad_() if use_res else None
    y64 = ref(*leaves64, res64)
    gy = torch.randn(y64.shape, generator=g0)
    y64.backward(gy.double())
    leaves32 = [a.clone().requires_grad_() for a in (x, alpha, g, v, bias)]   # fp32 on the CPU
    ref(*leaves32, res.clone().requires_grad_() if use_res else None).backward(gy)

    leaves = [a.to(DEV).requires_grad_() for a in (x, alpha, g, v, bias)]
    resd = res.to(DEV).requires_grad_() if use_res else None
    spec = (kind, cout, k, s, p, d, epi)
    y = train._SnakeConv.apply(leaves[0], leaves[1] if use_snake else None, leaves[2], leaves[3],
                               leaves[4], resd, spec)
    assert rel_err(y.detach().cpu().numpy(), y64.detach().numpy()) < TOL
    y.backward(gy.to(DEV))
    names = ["dx", "dalpha", "dg", "dv", "dbias"]
    for nm, a, r in zip(names, leaves, leaves64):
        if nm == "dalpha" and not use_snake:
            continue
        e = l2rel(a.grad.cpu().numpy(), r.grad.numpy())
        assert e < TOL, f"{nm}: rel {e}"
    for i in (0, 3):  # the adjoint conv's dx and the weight gradient's dv, per element
        fp32_bar(f"{names[i]} {case}", leaves[i].grad, leaves64[i].grad, leaves32[i].grad,
                 GRAD_MARGIN.get((names[i], case), 4))
    if use_res:
        assert l2rel(resd.grad.cpu().numpy(), res64.grad.numpy()) < TOL


def test_strided_conv_remainder_fails_cleanly():
    """k = 4, s = 2, p = 1 on T = 257: the conv drops the last input sample, the polyphase adjoint
    returns 256 columns; backward raises instead of returning a short gradient."""
    g0 = torch.Generator().manual_seed(5)
    cin, cout, k, s, p, T = 8, 16, 4, 2, 1, 257
    x = torch.randn(2, cin, T, generator=g0).to(DEV).requires_grad_()
    alpha = (torch.rand(cin, generator=g0) + 0.5).to(DEV).requires_grad_()
    g = (torch.rand(cout, generator=g0) + 0.5).to(DEV).requires_grad_()
    v = (torch.randn(cout, cin, k, generator=g0) * 0.1).to(DEV).requires_grad_()
    bias = torch.zeros(cout, device=DEV, requires_grad=True)
    y = train._SnakeConv.apply(x, alpha, g, v, bias, None, ("conv", cout, k, s, p, 1, 0))
    assert y.shape == (2, cout, 128)
    with pytest.raises(RuntimeError, match="adjoint conv shape"):
        y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert x.grad is None and alpha.grad is None


@pytest.mark.parametrize("cin,cout,k,pad,dil,T,snake", [
    (64, 96, 7, 9, 3, 700, True), (96, 96, 1, 0, 1, 257, True), (1024, 1024, 3, 1, 1, 87, True),
    (192, 192, 7, 27, 9, 300, False), (33, 70, 7, 3, 1, 65, True), (8, 1, 3, 1, 1, 40, True),
    (1, 64, 7, 3, 1, 65, False), (16, 16, 7, 3, 1, 1, True), (64, 64, 3, 1, 1, 64, True)])
def test_wgrad_x3_vs_torch64(cin, cout, k, pad, dil, T, snake):
    """Stride-1 weight gradients run on the split bf16 MFMA (wgrad_x3_kernel): against a torch
    fp64 conv1d_weight within 1e-5 (l2 rel), and within 4x the fp32 error bound, for partial
    tiles, every tap-group size, dilations 1/3/9 and a Snake on the layer input."""
    check_wgrad_x3(2, cin, cout, k, pad, dil, T, snake)


def test_wgrad_x3_uneven_splits_vs_torch64():
    """B = 3 at the (1024, 1024, 3) shape: six (clip, chunk) units over the plan's four splits,
    so the splits hold 1, 2, 1 and 2 of them."""
    check_wgrad_x3(3, 1024, 1024, 3, 1, 1, 87, True)


def check_wgrad_x3(B, cin, cout, k, pad, dil, T, snake):
    g0 = torch.Generator().manual_seed(cin + k)
    a = torch.randn(B, cout, T, generator=g0)
    x = torch.randn(B, cin, T, generator=g0)
    alpha = torch.rand(cin, generator=g0) + 0.5
    snk = None
    xs64, xs32 = x.double(), x
    if snake:
        al = alpha.to(DEV)
        snk = (al, 1.0 / (al + 1e-9))
        xs64 = snake64(x.double(), alpha.double()[None, :, None])
        xs32 = snake64(x, alpha[None, :, None])
    r = ops.conv1d_wgrad(a.to(DEV), x.to(DEV), k, 1, pad, dil, snake_x=snk)
    ref = torch.nn.grad.conv1d_weight(xs64, (cout, cin, k), a.double(), 1, pad, dil)
    assert l2rel(r.cpu().numpy(), ref.numpy()) < 1e-5
    ref32 = torch.nn.grad.conv1d_weight(xs32, (cout, cin, k), a, 1, pad, dil)
    fp32_bar(f"wgrad_x3 {(B, cin, cout, k, pad, dil, T, snake)}", r, ref, ref32)


def test_wgrad_deterministic():
    g0 = torch.Generator().manual_seed(3)
    a = torch.randn(3, 96, 700, generator=g0).to(DEV)
    x = torch.randn(3, 64, 700, generator=g0).to(DEV)
    r1 = ops.conv1d_wgrad(a, x, 7, 1, 9, 3)
    r2 = ops.conv1d_wgrad(a, x, 7, 1, 9, 3)
    assert torch.equal(r1, r2)
    ref = torch.nn.grad.conv1d_weight(x.double().cpu(), (96, 64, 7), a.double().cpu(), 1, 9, 3)
    assert l2rel(r1.cpu().numpy(), ref.numpy()) < TOL


@pytest.mark.parametrize("m,c,k,stride,pad,dil,T", [
    (96, 64, 7, 1, 9, 3, 300),     # wgrad_x3_kernel (stride-1 taps)
    (64, 96, 1, 1, 0, 1, 257),     # wgrad_x3_reg_kernel (k = 1)
    (128, 64, 4, 2, 1, 1, 128),    # wgrad_kernel (strided, fp32-input MFMA)
])
def test_wgrad_c_abi_in_kernel_snake(m, c, k, stride, pad, dil, T):
    """vrvq_conv1d_wgrad with alpha / alpha_a set (the Snake applied by the kernels while they
    stage the operands) returns the same bits as with the operands Snake'd up front by vrvq_snake
    and nullptr alphas (the form the torch op uses): the public C entry point, per kernel."""
    from vrvq_amd import _lib
    import ctypes
    g0 = torch.Generator().manual_seed(m + c + k)
    B = 2
    ta = (T + 2 * pad - dil * (k - 1) - 1) // stride + 1
    a = torch.randn(B, m, ta, generator=g0).to(DEV)
    x = torch.randn(B, c, T, generator=g0).to(DEV)
    al_a = (torch.rand(m, generator=g0) + 0.5).to(DEV)
    al_x = (torch.rand(c, generator=g0) + 0.5).to(DEV)
    inv_a, inv_x = ops.snake_inv_alpha(al_a), ops.snake_inv_alpha(al_x)
    P = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a_s, x_s = torch.empty_like(a), torch.empty_like(x)
    _lib.call("vrvq_snake", P(a), B, m, ta, P(al_a), P(inv_a), P(a_s), stream)
    _lib.call("vrvq_snake", P(x), B, c, T, P(al_x), P(inv_x), P(x_s), stream)
    split, ws_bytes = ctypes.c_int(0), ctypes.c_longlong(0)
    _lib.call("vrvq_wgrad_plan", B, m, ta, c, k, ctypes.byref(split), ctypes.byref(ws_bytes))
    ws = torch.empty((ws_bytes.value + 3) // 4, device=DEV)

    def wgrad(aa, a_al, a_ia, xx, x_al, x_ia):
        out = torch.empty(m, c, k, device=DEV)
        _lib.call("vrvq_conv1d_wgrad", P(aa), B, m, ta, P(a_al), P(a_ia), P(xx), c, T, P(x_al),
                  P(x_ia), k, stride, pad, dil, split.value, P(ws), ws.numel() * 4, P(out), stream)
        return out
    got = wgrad(a, al_a, inv_a, x, al_x, inv_x)
    want = wgrad(a_s, None, None, x_s, None, None)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ------------------------------------------------------------------ mask STE
def test_mask_ste_vs_torch64():
    B, T, nq, alpha = 5, 77, 28, 2.0
    g0 = torch.Generator().manual_seed(9)
    imp = torch.rand(B, 1, T, generator=g0)
    levels = torch.rand(B, generator=g0) * 5.875 + 0.125
    dropout = torch.randint(1, nq + 1, (B,), generator=g0)
    n_imps, n_drop = 3, 1
    imp64 = imp.double().requires_grad_()
    x = imp64 * levels.double()[:, None, None] * nq
    pm = x - torch.arange(nq, dtype=torch.float64)[None, :, None]
    sm = logcosh64(alpha, pm)
    q = (pm >= 0).double()
    m64 = sm + (q - sm).detach()
    m64 = m64.clone()
    m64[n_imps:n_imps + n_drop] = ((dropout[:n_drop].double()[:, None, None]
                                    - torch.arange(nq, dtype=torch.float64)[None, :, None]) >= 0).double()
    m64[n_imps + n_drop:] = 1.0
    gm = torch.randn(B, nq, T, generator=g0)
    (m64 * gm.double()).sum().backward()
    impd = imp.to(DEV).requires_grad_()
    m = train._MaskSte.apply(impd, levels.to(DEV), dropout.to(DEV), nq, alpha, n_imps, n_drop)
    np.testing.assert_allclose(m.detach().cpu().numpy(), m64.detach().numpy(), atol=1e-6)
    (m * gm.to(DEV)).sum().backward()
    assert l2rel(impd.grad.cpu().numpy(), imp64.grad.numpy()) < TOL


def test_generate_mask_ste_public_vs_torch64():
    """vrvq_amd.generate_mask_ste (the public helper, models/utils.py:45-53) is differentiable:
    hard-mask forward, log-cosh backward, against the fp64 restatement."""
    B, T, nq, alpha = 3, 61, 8, 2.0
    g0 = torch.Generator().manual_seed(21)
    x = torch.rand(B, 1, T, generator=g0) * (nq + 2) - 1.0
    x64 = x.double().requires_grad_()
    pm = x64 - torch.arange(nq, dtype=torch.float64)[None, :, None]
    sm = logcosh64(alpha, pm)
    m64 = sm + ((pm >= 0).double() - sm).detach()
    gm = torch.randn(B, nq, T, generator=g0)
    (m64 * gm.double()).sum().backward()
    xd = x.to(DEV).requires_grad_()
    m = vrvq_amd.generate_mask_ste(xd, nq, alpha)
    np.testing.assert_array_equal(m.detach().cpu().numpy(), m64.detach().numpy())
    np.testing.assert_array_equal(m.detach().cpu().numpy(),
                                  vrvq_amd.generate_mask_hard(x.to(DEV), nq).cpu().numpy())
    (m * gm.to(DEV)).sum().backward()
    assert l2rel(xd.grad.cpu().numpy(), x64.grad.numpy()) < TOL
    with torch.no_grad():  # no tape: the plain hard-mask kernel
        np.testing.assert_array_equal(vrvq_amd.generate_mask_ste(xd, nq, alpha).cpu().numpy(),
                                      m64.detach().numpy())


# ------------------------------------------------------------------ quantizer backward
@pytest.mark.parametrize("nq,B,T", [(4, 2, 20), (28, 2, 33), (9, 3, 70)])
def test_rvq_backward_vs_torch64(nq, B, T):
    D, d, N = 1024, 8, 1024
    g0 = torch.Generator().manual_seed(nq * 100 + T)
    z = torch.randn(B, D, T, generator=g0) * 0.5
    g_in = torch.rand(nq * d, generator=g0) + 0.5
    v_in = torch.randn(nq * d, D, generator=g0) * 0.03
    b_in = torch.randn(nq, d, generator=g0) * 0.1
    g_out = torch.rand(nq * D, generator=g0) + 0.5
    v_out = torch.randn(nq * D, d, generator=g0) * 0.3
    b_out = torch.randn(nq, D, generator=g0) * 0.1
    cb = torch.randn(nq, N, d, generator=g0)
    mask = (torch.rand(B, nq, T, generator=g0) < 0.7).float()
    mask[:, 0] = 1.0
    leaves = [a.to(DEV).requires_grad_() for a in (z, mask, g_in, v_in, b_in, g_out, v_out, b_out, cb)]
    z_q, commit, cbl, codes, lat = train._RvqTrain.apply(*leaves)
    # the forward's own argmin against fp64 (the comparisons below are teacher-forced on it)
    R.check_codes(codes, z, R.Params(g_in, v_in, b_in, g_out, v_out, b_out, cb))
    leaves64 = [a.double().requires_grad_() for a in (z, mask, g_in, v_in, b_in, g_out, v_out, b_out, cb)]
    zq64, c64, cb64 = rvq64(*leaves64, codes.cpu())
    assert rel_err(z_q.detach().cpu().numpy(), zq64.detach().numpy()) < TOL
    assert float(commit) == pytest.approx(float(c64), rel=TOL)
    gz = torch.randn(B, D, T, generator=g0)
    lc, lcb = 0.25, 1.0
    (zq64 * gz.double()).sum().add(lc * c64 + lcb * cb64).backward()
    ((z_q * gz.to(DEV)).sum() + lc * commit + lcb * cbl).backward()
    names = ["dz", "dmask", "dg_in", "dv_in", "db_in", "dg_out", "dv_out", "db_out", "dcb"]
    for nm, a, r in zip(names, leaves, leaves64):
        e = l2rel(a.grad.cpu().numpy(), r.grad.numpy())
        assert e < TOL, f"{nm}: rel {e}"


def _rvq_train_forward(params, z, mask):
    with torch.no_grad():
        out = train._RvqTrain.apply(z.to(DEV), mask.to(DEV), *(p.to(DEV) for p in params))
    torch.cuda.synchronize()
    return out


def test_rvq_train_forward_diverse_vs_fp64():
    """rvq_encode_train's own argmin on inputs that exercise it (tests/rvq_ref.py: 100+ distinct
    codes per stage, every quarter of the codebook): every decision within 8 eps_d of its
    stage's fp64 minimum (check_codes), latents and z_q against the fp64 chain on those codes."""
    nq, B, T = 8, 3, 87
    params, z, _ = R.diverse_case(nq, 1024, B, T)
    mask = (torch.rand(B, nq, T, generator=torch.Generator().manual_seed(5)) < 0.7).float()
    mask[:, 0] = 1.0
    z_q, _commit, _cbl, codes, lat = _rvq_train_forward(params, z, mask)
    distinct = R.assert_diverse(codes, 1024)
    res = R.check_codes(codes, z, params)
    print(f"train diverse: eps_d={res['eps_d']:.2e} margin={res['margin']:.2e} "
          f"worst={res['worst']:.2e} mismatch={res['share']:.4%} min distinct={distinct}")
    ref = res["ref"]
    assert rel_err(lat.cpu().numpy(), ref.latents.numpy()) < 1e-5
    zq64 = (ref.z_q_is * mask.double()[:, :, None, :]).sum(1)
    assert rel_err(z_q.cpu().numpy(), zq64.numpy()) < 1e-5


def test_rvq_train_exact_ties_take_lowest_index():
    """cb[N/2 + j] = cb[j] in every stage: every decision of the training forward is an exact tie
    of two identical rows and takes the lower index, as the eval kernels do
    (test_gpu_parity.py test_rvq_exact_ties_take_lowest_index)."""
    nq, N = 8, 1024
    params, gen = R.diverse_rvq_params(nq, N, 900 + nq + N)
    params = params._replace(cb=R.tie_codebook(params.cb, "half"))
    z = R.diverse_z(2, 87, gen)
    codes = _rvq_train_forward(params, z, torch.ones(2, nq, 87))[3].cpu()
    R.check_codes(codes, z, params)
    high = ~R.lower_twin(codes, N, "half")
    assert not bool(high.any()), (f"{int(high.sum())} of {codes.numel()} decisions took the "
                                  f"higher twin, first at {high.nonzero()[0].tolist()}")


def _quantizer_leaves(q):
    leaves = [a.detach().double().cpu().requires_grad_() for a in train._stage_params(q.quantizers)]
    return leaves


def _check_quantizer_train(q, z, out, mask_ref):
    """z_q / losses / gradients of a training-mode quantizer output against rvq64 with the
    reference's mask (codes fixed, as the straight-through estimator uses them)."""
    leaves64 = _quantizer_leaves(q)
    # the forward's own argmin against fp64 (everything below is teacher-forced on its codes)
    R.check_codes(out["codes"], z, R.Params(*leaves64))
    z64 = z.detach().double().cpu().requires_grad_()
    zq64, c64, cb64 = rvq64(z64, mask_ref.double(), *leaves64, out["codes"].cpu())
    assert rel_err(out["z_q"].detach().cpu().numpy(), zq64.detach().numpy()) < TOL
    assert float(out["commitment_loss"]) == pytest.approx(float(c64), rel=TOL)
    assert float(out["codebook_loss"]) == pytest.approx(float(cb64), rel=TOL)
    g0 = torch.Generator().manual_seed(77)
    gz = torch.randn(z.shape, generator=g0)
    (zq64 * gz.double()).sum().add(0.25 * c64 + cb64).backward()
    ((out["z_q"] * gz.to(DEV)).sum() + 0.25 * out["commitment_loss"]
     + out["codebook_loss"]).backward()
    assert l2rel(z.grad.cpu().numpy(), z64.grad.numpy()) < TOL
    names = ["g_in", "v_in", "b_in", "g_out", "v_out", "b_out", "cb"]
    got = [torch.cat([qq.in_proj.weight_g.grad.reshape(-1) for qq in q.quantizers]),
           torch.cat([qq.in_proj.weight_v.grad.reshape(qq.in_proj.out_channels, -1)
                      for qq in q.quantizers]),
           torch.stack([qq.in_proj.bias.grad for qq in q.quantizers]),
           torch.cat([qq.out_proj.weight_g.grad.reshape(-1) for qq in q.quantizers]),
           torch.cat([qq.out_proj.weight_v.grad.reshape(qq.out_proj.out_channels, -1)
                      for qq in q.quantizers]),
           torch.stack([qq.out_proj.bias.grad for qq in q.quantizers]),
           torch.stack([qq.codebook.weight.grad for qq in q.quantizers])]
    for nm, a, r in zip(names, got, leaves64):
        e = l2rel(a.cpu().numpy(), r.grad.numpy())
        assert e < TOL, f"{nm}: rel {e}"


def _random_quantizer(q, seed):
    g0 = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in q.named_parameters():
            if "codebook" in name:
                p.copy_(torch.randn(p.shape, generator=g0))
            elif "weight_g" in name:
                p.copy_(torch.rand(p.shape, generator=g0) + 0.5)
            elif "weight_v" in name:
                p.copy_(torch.randn(p.shape, generator=g0) * (0.03 if "in_proj" in name else 0.3))
            else:
                p.copy_(torch.randn(p.shape, generator=g0) * 0.1)
    return q.to(DEV).train()


def test_cbr_train_quantizer_vs_torch64():
    """ResidualVectorQuantize in training mode with quantizer dropout (models/quantize.py:165-214):
    row b keeps stages i < n_quantizers[b] for the first int(B * dropout) rows (randint draws
    under the same seed), all stages otherwise."""
    from vrvq_amd.model import ResidualVectorQuantize
    nq, B, T = 5, 6, 37
    q = _random_quantizer(ResidualVectorQuantize(input_dim=1024, n_codebooks=nq,
                                                 codebook_size=1024, codebook_dim=8,
                                                 quantizer_dropout=0.5), 31)
    z = (torch.randn(B, 1024, T, generator=torch.Generator().manual_seed(32)) * 0.5).to(DEV)
    z.requires_grad_()
    torch.manual_seed(123)
    out = q(z)
    torch.manual_seed(123)  # the reference's draws (models/quantize.py:176-179)
    n_q = torch.ones((B,)) * nq + 1
    dropout = torch.randint(1, nq + 1, (B,))
    n_drop = int(B * 0.5)
    n_q[:n_drop] = dropout[:n_drop]
    mask_ref = (torch.arange(nq)[None, :, None] < n_q[:, None, None]).float().expand(B, nq, T)
    assert 0 < int((mask_ref == 0).sum())  # some stages dropped under this seed
    np.testing.assert_array_equal(out["dropout"].numpy(), dropout.numpy())
    _check_quantizer_train(q, z, out, mask_ref)


def test_vbr_quantizer_cbr_mode_train_vs_torch64():
    """VBRResidualVectorQuantize in training mode with n_quantizers = Nq (models/quantize.py:
    346-414): mask rows ones / dropout / full codebook, no level draw, imp_map None."""
    from vrvq_amd.model import VBRResidualVectorQuantize
    nq, B, T = 6, 8, 29
    q = _random_quantizer(VBRResidualVectorQuantize(
        input_dim=1024, n_codebooks=nq, codebook_size=1024, codebook_dim=8, quantizer_dropout=0.5,
        full_codebook_rate=0.25, level_min=0.125, level_max=6.0), 41)
    z = (torch.randn(B, 1024, T, generator=torch.Generator().manual_seed(42)) * 0.5).to(DEV)
    z.requires_grad_()
    torch.manual_seed(7)
    out = q(z, nq, None, None)
    torch.manual_seed(7)
    dropout = torch.randint(1, nq + 1, (B, 1, 1)).expand(B, 1, T)
    n_full, n_drop = int(B * 0.25), int(B * 0.5)
    n_imps = B - n_full - n_drop
    mask_ref = torch.ones(B, nq, T)
    mask_ref[n_imps:n_imps + n_drop] = (dropout[:n_drop] - torch.arange(nq)[None, :, None]
                                        >= 0).float()
    assert out["imp_map"] is None
    np.testing.assert_array_equal(out["mask_imp"].cpu().numpy(), mask_ref.numpy())
    with pytest.raises(RuntimeError):
        q(z, nq - 1, None, None)
    _check_quantizer_train(q, z, out, mask_ref)


# ------------------------------------------------------------------ whole generator vs reference
_train_models = {}


def train_model(manifest, name):
    m = manifest[name]
    model = vrvq_amd.DAC_VRVQ(**m["kwargs"])
    load_recipe(model, m["weight_seed"])
    return model.to(DEV).train()


def generator_step(model, g, m):
    """The fixture's step (make_golden.train_fixture) on the HIP autograd path."""
    x = t(g["audio_in"])
    L = x.shape[-1]
    torch.manual_seed(m["rng_seed"])
    xp = model.preprocess(x, 44100)
    z, feat = model.encoder(xp, return_feat=True)
    z.retain_grad()
    feat.retain_grad()
    enc = model.quantizer(z, None, feat, 1)
    zq = enc["z_q"]
    zq.retain_grad()
    y = model.decode(zq)[..., :L]
    lam = m["lambdas"]
    terms = {"waveform": (y - x).abs().mean(), "commitment": enc["commitment_loss"],
             "codebook": enc["codebook_loss"], "rate": enc["imp_map"].mean()}
    loss = sum(lam[k] * v for k, v in terms.items())
    loss.backward()
    return enc, y, z, feat, zq, terms, loss


@pytest.mark.parametrize("name", ["golden_train_a2", "golden_train_a2_rows"])
def test_generator_grads_vs_reference(manifest, name):
    m = manifest[name]
    g = load_golden(name)
    model = train_model(manifest, name)
    enc, y, z, feat, zq, terms, loss = generator_step(model, g, m)
    # seed-controlled draws, bit-exact
    kw = m["kwargs"]  # the fixture holds the raw torch.rand draws; scale them as the reference
    lv = torch.from_numpy(g["draws_levels"]) * (kw["level_max"] - kw["level_min"]) + kw["level_min"]
    np.testing.assert_array_equal(enc["random_levels"].numpy(), lv.numpy())
    np.testing.assert_array_equal(enc["dropout"].numpy(), g["draws_dropout"])
    np.testing.assert_array_equal(enc["codes"].cpu().numpy(), g["codes"])
    np.testing.assert_allclose(enc["mask_imp"].detach().cpu().numpy(), g["mask_imp"], atol=1e-6)
    assert rel_err(enc["imp_map"].detach().cpu().numpy(), g["imp_map"]) < TOL
    assert rel_err(y.detach().cpu().numpy(), g["audio_out"]) < TOL
    for k, v in terms.items():
        assert float(v) == pytest.approx(float(g["term_" + k]), rel=TOL), k
    for nm, a in (("grad_z_q", zq), ("grad_z", z), ("grad_feat", feat)):
        e = l2rel(a.grad.cpu().numpy(), g[nm])
        assert e < TOL, f"{nm}: rel {e}"
    bad = []
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(m["params"])
    for pname in m["params"]:
        gr = params[pname].grad.detach().reshape(-1).double().cpu()
        ref_norm = m["grad_norms"][pname]
        if abs(float(gr.norm()) - ref_norm) > TOL * max(ref_norm, 1e-30):
            bad.append((pname, "norm", float(gr.norm()), ref_norm))
        if "g_full/" + pname in g:
            e = l2rel(gr.numpy(), g["g_full/" + pname])
        else:
            idx = np.unique(np.linspace(0, gr.numel() - 1, min(gr.numel(), 256)).round()
                            .astype(np.int64))
            e = l2rel(gr.numpy()[idx], g["g_s/" + pname])
        if e > TOL:
            bad.append((pname, "values", e))
    assert not bad, bad[:10]


def test_train_step_deterministic(manifest):
    """Two identical seeded steps give bitwise identical gradients (fixed-order reductions)."""
    name = "golden_train_a2"
    m = manifest[name]
    g = load_golden(name)
    grads = []
    for _ in range(2):
        model = train_model(manifest, name)
        generator_step(model, g, m)
        grads.append([p.grad.detach().clone() for p in model.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ full step + data parallel
def test_full_train_step_runs(manifest):
    """scripts/train.py:262-335 at B=2, 0.38 s: discriminator + generator updates with every loss
    of vrvq_a2 (mel / adv / feat / commitment / codebook / rate); finite, parameters move."""
    from vrvq_amd.trainer import LAMBDAS_A2, build_state, train_step
    m = manifest["golden_train_a2"]
    model = vrvq_amd.DAC_VRVQ(**m["kwargs"])
    load_recipe(model, m["weight_seed"])
    torch.manual_seed(0)
    state = build_state(model, DEV)
    x = t(load_golden("golden_train_a2")["audio_in"])
    before = [p.detach().clone() for p in model.parameters()]
    for _ in range(2):
        out = train_step(state, x, LAMBDAS_A2)
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    moved = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, model.parameters()))
    assert moved == len(before)


def test_train_step_config4_shape():
    """BASELINE configs[3]'s per-GPU shape (B = 32 x 0.38 s, vrvq_a2, the bench.py --train step):
    two identically seeded states take one full step on the same batch -- every loss finite and
    bitwise equal (the forward is deterministic), the gradient norms within 1e-5 and every
    parameter within 2.5 lr of the other run's: the generator's gradient through the
    discriminator comes from MIOpen's backward-data convolutions, which accumulate in a
    run-dependent order (measured 3250.7571 vs 3250.7561 for the generator's gradient norm), and
    AdamW's first step moves a parameter by ~lr * sign(grad), so a near-zero gradient element may
    move either way; the HIP kernels' own gradients are bitwise deterministic
    (test_train_step_deterministic)."""
    from vrvq_amd.config import A2_KWARGS
    from vrvq_amd.recipe import synthetic_audio
    from vrvq_amd.trainer import LAMBDAS_A2, build_state, train_step
    x = torch.from_numpy(synthetic_audio(32, 16758, seed=4321)).to(DEV)
    outs, params = [], []
    for _ in range(2):
        model = vrvq_amd.DAC_VRVQ(**A2_KWARGS)
        load_recipe(model, 0)
        torch.manual_seed(0)
        state = build_state(model, DEV)
        torch.manual_seed(1)
        out = train_step(state, x, LAMBDAS_A2)
        torch.cuda.synchronize()
        outs.append({k: v.detach().clone() for k, v in out.items()})
        params.append([p.detach().clone() for p in model.parameters()])
        del state, model
    for k, v in outs[0].items():
        assert torch.isfinite(v).all(), k
        if "grad_norm" in k:
            assert rel_err(v.cpu().numpy(), outs[1][k].cpu().numpy()) < 1e-5, k
        else:
            assert torch.equal(v, outs[1][k]), k
    lr = 1e-4  # trainer.build_state default (conf/base.yml)
    for a, b in zip(*params):
        assert float((a - b).abs().max()) <= 2.5 * lr


def _gen_ddp_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from vrvq_amd.recipe import synthetic_audio
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        kw = dict(n_codebooks=8, level_min=0.125, level_max=6.0, full_codebook_rate=0.25,
                  imp2mask_alpha=2.0)
        model = vrvq_amd.DAC_VRVQ(**kw)
        load_recipe(model, 0)
        model = model.to(dev).train()
        ddp = DDP(model, device_ids=[0])
        x = torch.from_numpy(synthetic_audio(2, 4410, seed=50 + rank)).to(dev)

        def loss_of(out):
            return ((out["audio"] - x).abs().mean() + 0.25 * out["vq/commitment_loss"]
                    + out["vq/codebook_loss"] + 2.0 * out["imp_map"].mean())

        torch.manual_seed(7 + rank)
        with ddp.no_sync():
            loss_of(ddp(x, 44100)).backward()
        local = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
        want = local.clone()
        dist.all_reduce(want)
        want /= world
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7 + rank)
        loss_of(ddp(x, 44100)).backward()
        got = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
        err = float((got - want).norm() / want.norm())
        diff_ranks = float((local - want).norm() / want.norm())
        q.put((rank, err, diff_ranks))
    finally:
        dist.destroy_process_group()


def test_generator_ddp_two_ranks():
    """DistributedDataParallel over the HIP autograd path: two ranks (gloo, both on cuda:0 of
    the one-GPU box) — the synchronised gradient equals the mean of the ranks' local ones."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gen_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, err, diff in res:
        assert err < 1e-5, (rank, err)
        assert diff > 1e-3  # the shards differ: the all-reduce did something
