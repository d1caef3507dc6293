"""The training-mode quantizer's backward (csrc/rvq_train.hip through train._RvqTrain and
train._MaskSte) on the MI355X, judged per gradient source, per stage and per element against
fp64 autograd of the reference loop (tests/rvq_grad_ref.py; its bars are shown to bite on the CPU
by tests/test_rvq_grad_ref.py).

Quantizer. One _RvqTrain.apply per case, then one backward per source ("dzq": (z_q gz).sum(),
"commit", "codebook", each alone with weight 1), teacher-forced on the kernel's own codes, which
go through rvq_ref.check_codes. (autograd hands a custom Function zeros for the outputs a loss
does not reach, so _RvqTrain.backward's `is None` branches are run by one direct call and
compared bit for bit with what autograd's zeros give.) Shapes (nq, N, B, T): one frame; B T = 32 and 64, exact
multiples of the chain's 32-frame workgroup; 33 frames with clips straddling a workgroup; nq = 1
(no cross terms), 8 (one packed b_out block, bdz row 7, last stage masked off), 9, 17 and 32
(BW_NQMAX, four blocks); N = 256 and 768; a decaying-residual case (|r_i| falls ~0.8 per stage,
the trained regime where dW_in cancels) and a many-hits case (one codebook row summed over 289
frames of both clips).

Bars. Per source, tensor and stage slice (dz, dmask whole): e = rel_err < 1e-5 and
e <= 4 e32 + 2e-7, e32 the same loop in torch fp32 on the CPU; a slice whose reference is
exactly zero is exactly zero (only dcb under "codebook", dcb = 0 otherwise, dmask = 0 under
"commit", never-chosen codebook rows, the parameters of a last stage that is masked off). Seven
tensors of the decaying case (rvq_grad_ref.HEADER_BARRED) are judged by 4 max(e32, e32h) + 2e-7,
e32h the header comment's own algebra (and the forward's projected z_e) in fp32 einsums, which
misses 4 e32 there itself. dcb of the many-hits case also per row against the fp64 sum of the
terms the kernel adds: |got - sum| <= 64 * 2^-24 * S (test_gpu_backward_edges.reduction_bar).

Mask STE. mask_ste_backward per element against fp64 autograd of logcosh64 within
4 e32 + 2e-7 at alpha 1 / 2 / 4, nq 8 / 32, x = 0, exact integers (p = 0), x = 192, with and
without levels, every row split; the forward equal to the fp64 hard mask wherever |p| > 1e-6,
one all-STE case eight elements past the 65536-block cap of its grid.

What these tests found, and the fix. With M_ij = W_in(i) W_out(j) formed by one fp32 fmaf chain
over the 1024 channels (cross_prep_kernel, 1.0e-6 of |M|), the kernels missed 4 e32 + 2e-7 in 92
of 1152 slices and the 1e-5 cap in one: 17-256-2-20 "commit" dg_in[5], e = 1.45e-5 at
e32 = 2.5e-6, where the same algebra in fp32 with M from an ordinary einsum gives 1.2e-6. The
training step now forms M and Qb with fp64 accumulation (vrvq_rvq_cross_prep_precise, 3.0e-8
and 4.3e-8 of their largest entry; the inference path keeps its bits). Measured on the MI355X
after that (every case prints e / e32 / e32h per tensor and stage):

  case           slices  over 4 e32 + 2e-7   worst e     there: e32   where
  1-1024-1-1         13          0           8.5e-07       3.5e-07   dzq dmask
  1-1024-2-16        13          0           3.5e-07       4.4e-07   dzq db_in[0]
  8-1024-2-32        78          0           6.0e-07       8.7e-07   dzq dg_in[2]
  9-1024-3-11       116          0           9.0e-07       8.0e-07   dzq db_in[0]
  32-1024-2-33      415          0           2.6e-06       1.5e-06   commit dz
  17-256-2-20       220          0           1.2e-06       2.2e-06   commit db_in[1]
  4-768-2-40         51          0           6.3e-07       9.6e-07   dzq dg_in[1]
  decay             207         16           2.0e-06       8.1e-07   dzq dv_in[15]
  hits               39          0           6.5e-07       4.7e-07   dzq db_in[0]

17-256-2-20 "commit" dg_in[5] is now at 6.5e-7. The tightest slice outside the decaying case
uses 0.87 of 4 e32 + 2e-7 (32-1024-2-33 "dzq" db_in[22], e = 1.9e-6 at e32 = 5.0e-7). The
decaying case's 16 slices over 4 e32 are in db_in, db_out, dcb, dg_in and dv_out, mostly under
"commit", worst e = 1.4e-6 at e32 = 9.9e-8 and e32h = 3.9e-7 (db_in[9]): z_e(i) there is a
small difference of W_in(i) z and the cross terms, and the "commit" and "codebook" gradients
are proportional to z_e - cb[code]. Conditioning max|P_i| / max|dW_in(i)| per stage of that
case, "dzq": 1.0 1.2 1.8 2.3 3.4 3.9 4.4 4.3 8.8 5.9 14.3 8.9 8.1 11.7 10.6 13.8; "commit":
1.0 1.2 1.8 1.8 3.0 2.4 3.9 4.9 4.0 4.5 6.2 3.9 4.1 4.3 6.0 7.1 (the random-codebook cases:
1.0 falling to 0.1, the residual grows there). dcb, many-hits: worst |got - sum| =
4.6 x 2^-24 S against the bar of 64 (against the fp64 chain's z_e instead of the stored
latents: 856, all of it the forward's rounding of z_e at rows hit once). Mask STE backward:
e = e32 to two digits in most cases, worst e = 8.1e-7 at e32 = 8.1e-7 (alpha 4, nq 32, levels).
"""
import ctypes
import functools

import pytest
import torch

import rvq_grad_ref as G
import rvq_ref as R
from test_gpu_backward_edges import reduction_bar
from vrvq_amd import _lib, ops, train

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ------------------------------------------------------------------ quantizer
def run_rvq(c0):
    """One forward and one backward per source on the GPU: (case teacher-forced on the kernel's
    codes, forward outputs on the CPU, {source: {name: gradient on the CPU}})."""
    leaves = [a.to(DEV).requires_grad_() for a in (c0.z, c0.mask) + tuple(c0.params)]
    z_q, commit, cbl, codes, lat = train._RvqTrain.apply(*leaves)
    losses = {"dzq": (z_q * c0.gz.to(DEV)).sum(), "commit": commit, "codebook": cbl}
    grads = {}
    for source in G.SOURCES:
        g = torch.autograd.grad(losses[source], leaves, retain_graph=True)
        grads[source] = {nm: t.cpu() for nm, t in zip(G.NAMES, g)}
    torch.cuda.synchronize()
    fwd = (z_q.detach().cpu(), float(commit.detach()), float(cbl.detach()), codes.cpu(), lat.cpu())
    return c0.with_codes(codes), fwd, grads


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    return run_rvq(G.case(name))


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_rvq_forward_codes_and_both_losses_vs_fp64(name):
    c, (z_q, commit, cbl, codes, lat), _ = gpu_case(name)
    res = R.check_codes(codes, c.z, c.params)
    zq64, c64, cb64 = G.forward64(c)
    e_zq, e_lat = G.rel_err(z_q, zq64), G.rel_err(lat, res["ref"].latents)
    print(f"{name}: code mismatch={res['share']:.4%} z_q e={e_zq:.2e} latents e={e_lat:.2e} "
          f"commit {commit:.8e} / {float(c64):.8e} codebook {cbl:.8e} / {float(cb64):.8e}")
    assert e_zq < 1e-5 and e_lat < 1e-5
    assert commit == pytest.approx(float(c64), rel=1e-5)
    assert cbl == pytest.approx(float(cb64), rel=1e-5)


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_rvq_backward_per_source_and_stage_vs_autograd64(name):
    c, _, grads = gpu_case(name)
    nq, N, B, T = c.shape
    fails = []
    for source in G.SOURCES:
        fails += G.judge(grads[source], c, source)
    for source in ("dzq", "commit"):
        print(f"{name} max|P_i| / max|dW_in(i)| ({source}):",
              " ".join(f"{x:.1f}" for x in G.conditioning(c, source)))
    assert not fails, "\n".join(fails)
    # exact zeros, stated once more where the algebra promises them
    zero = torch.zeros(())
    for nm in G.NAMES:
        if nm != "dcb":
            assert torch.equal(grads["codebook"][nm], zero.expand_as(grads["codebook"][nm])), nm
    dcb = grads["codebook"]["dcb"]
    assert float(dcb.abs().max()) > 0
    for source in ("dzq", "commit"):
        assert torch.equal(grads[source]["dcb"], torch.zeros_like(dcb)), source
    assert torch.equal(grads["commit"]["dmask"], torch.zeros_like(c.mask))
    both, _ = G.hit_counts(c)
    assert torch.equal(dcb[both == 0], torch.zeros_like(dcb[both == 0]))
    for i in range(nq):  # a stage that is masked off everywhere has no codebook gradient
        if bool((c.mask[:, i] == 0).all()):
            assert torch.equal(dcb[i], torch.zeros_like(dcb[i])), i


def test_rvq_codebook_grad_many_hits_per_row():
    """rvq_codebook_grad_kernel's frame-order sum over both clips with up to 289 terms in a row:
    per row and component within 64 * 2^-24 S of the fp64 sum of the terms it adds, S the fp64
    sum of their absolute values. The terms are formed in fp64 from the forward's stored fp32
    latents, the backward's input: against the fp64 chain's z_e the bar would also charge the
    sum with the forward's rounding of z_e, an absolute error of a few 2^-24 |z_e| that is
    unrelated to how small a component of cb[n] - z_e is (measured then: 856 x 2^-24 S at a
    row hit once, stage 1; the latents have their own check above, and dcb against the fp64
    chain its per-stage bar)."""
    c, fwd, grads = gpu_case("hits")
    both, first = G.hit_counts(c)
    row = int(both[0].argmax())
    assert int(both[0, row]) >= 64 and 0 < int(first[0, row]) < int(both[0, row])
    tot, s_abs = G.dcb_terms(c, latents=fwd[4])
    reduction_bar(f"dcb hits (stage 0 row {row}: {int(both[0, row])} frames)",
                  grads["codebook"]["dcb"], tot, s_abs)


@pytest.mark.parametrize("name", ["9-1024-3-11", "32-1024-2-33"])
def test_rvq_backward_deterministic(name):
    """"All sums deterministic": a second forward and backward gives the same bits."""
    _, fwd, grads = gpu_case(name)
    _, fwd2, grads2 = run_rvq(G.case(name))
    assert torch.equal(fwd[3], fwd2[3]) and torch.equal(fwd[0], fwd2[0])
    for source in G.SOURCES:
        for nm in G.NAMES:
            assert torch.equal(grads[source][nm], grads2[source][nm]), (source, nm)


class _Ctx:
    """What _RvqTrain.forward / backward use of an autograd context, for a direct call."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


@pytest.mark.parametrize("name", ["9-1024-3-11"])
def test_rvq_backward_none_gradients_direct(name):
    """autograd hands a custom Function zeros for the outputs a loss does not reach, so
    _RvqTrain.backward's `dzq is None` / `gc is None` / `gcb is None` branches are only reached
    by a direct call: with None they give the bits autograd's zeros give."""
    c, _, grads = gpu_case(name)
    ctx = _Ctx()
    with torch.no_grad():
        train._RvqTrain.forward(ctx, *(a.to(DEV) for a in (c.z, c.mask) + tuple(c.params)))
        one = torch.ones((), device=DEV)
        for source, args in (("commit", (None, one, None)), ("codebook", (None, None, one)),
                             ("dzq", (c.gz.to(DEV), None, None))):
            got = train._RvqTrain.backward(ctx, *args, None, None)
            for nm, t in zip(G.NAMES, got):
                assert torch.equal(t.cpu(), grads[source][nm]), (source, nm)


def test_cross_prep_precise_rounds_each_entry_once():
    """The training step's M_ij = W_in(i) W_out(j) and Qb (vrvq_rvq_cross_prep_precise, fp64
    accumulation): within one fp32 rounding of the fp64 value, where the inference path's fp32
    chain over the 1024 channels is at 1e-6 of |M|; same layout, same zeros (i <= j)."""
    nq, d, D = 17, R.D_CODE, R.D_MODEL
    p = G.case("17-256-2-20").params
    w_in = torch._weight_norm(p.v_in, p.g_in.reshape(-1, 1), 0).reshape(nq, d, D)
    w_out = torch._weight_norm(p.v_out, p.g_out.reshape(-1, 1), 0).reshape(nq, D, d)
    w_in_t = w_in.transpose(1, 2).contiguous().to(DEV)
    m64 = torch.einsum("ikc,jcm->jikm", w_in.double(), w_out.double())
    lower = (torch.arange(nq)[None, :] > torch.arange(nq)[:, None])[:, :, None, None]
    m64 = m64 * lower
    cumb = torch.cumsum(p.b_out.double(), 0) - p.b_out.double()
    qb64 = torch.einsum("ikc,ic->ik", w_in.double(), cumb)
    mp, qp = ops.rvq_cross_prep_precise(w_in_t, w_out.to(DEV), p.b_out.to(DEV))
    mf, qf = ops.rvq_cross_prep(w_in_t, w_out.to(DEV), p.b_out.to(DEV))
    e_p, e_f = G.rel_err(mp.cpu(), m64), G.rel_err(mf.cpu(), m64)
    print(f"mcol: precise e={e_p:.2e} fp32 chain e={e_f:.2e}; qb: precise "
          f"e={G.rel_err(qp.cpu(), qb64):.2e} fp32 chain e={G.rel_err(qf.cpu(), qb64):.2e}")
    assert bool(((mp.cpu().double() - m64).abs() <= 2.0 ** -24 * m64.abs()).all())
    assert bool(((qp.cpu().double() - qb64).abs() <= 2.0 ** -24 * qb64.abs()).all())
    assert torch.equal(mp.cpu()[~lower.expand_as(mp)], torch.zeros(int((~lower.expand_as(mp)).sum())))
    assert e_f < 1e-5


def test_rvq_33_stages_refused_cleanly():
    """nq = 33 > BW_NQMAX: the forward and ops.rvq_backward raise, the workspace query returns a
    status, nothing is launched, and the next valid call works."""
    nq, B, T, D, d, N = 33, 2, 5, R.D_MODEL, R.D_CODE, 1024
    params, gen = R.diverse_rvq_params(nq, N, 33)
    z = R.diverse_z(B, T, gen)
    leaves = [a.to(DEV).requires_grad_() for a in (z, torch.ones(B, nq, T)) + tuple(params)]
    with pytest.raises(RuntimeError):
        train._RvqTrain.apply(*leaves)
    f = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="vrvq_rvq_backward_workspace"):
        ops.rvq_backward(f(B, D, T), f(()), f(()), f(B, D, T), f(B, nq, T, d), f(B, nq * d, T),
                         torch.zeros(B, nq, T, dtype=torch.long, device=DEV), f(B, nq, T),
                         f(nq, D, d), f(nq, D, d), f(nq, D), f(nq, nq, d, d), f(nq, N, d))
    nbytes = ctypes.c_longlong(-1)
    with pytest.raises(RuntimeError, match=r"vrvq_rvq_backward_workspace failed \(-?[1-9]"):
        _lib.call("vrvq_rvq_backward_workspace", B, T, 33, ctypes.byref(nbytes))
    assert nbytes.value == -1
    _lib.call("vrvq_rvq_backward_workspace", B, T, 32, ctypes.byref(nbytes))
    assert nbytes.value > 0
    torch.cuda.synchronize()
    c, _, grads = run_rvq(G.case("1-1024-2-16"))
    assert not G.judge(grads["dzq"], c, "dzq", verbose=False)


# ------------------------------------------------------------------ mask STE
def ste_inputs(nq, with_levels, B=5, T=77):
    """x (levels None) or (imp, levels) with planted x = 0, exact integers (p = 0 for one i),
    x = level_max nq = 192 at nq = 32, and p down to -31."""
    gen = torch.Generator().manual_seed(100 * nq + with_levels)
    if with_levels:
        imp = torch.rand(B, T, generator=gen)
        levels = torch.rand(B, generator=gen) * 5.875 + 0.125
        levels[0], levels[1] = 6.0, 0.5
        imp[0, :3] = torch.tensor([1.0, 0.0, 0.5])      # x = 6 nq (192), 0, 3 nq
        imp[1, :3] = torch.tensor([0.25, 0.0, 0.75])    # x = nq / 8 (p = 0 at i = 1 or 4), 0
    else:
        imp = torch.rand(B, T, generator=gen) * (nq + 2) - 1.0
        levels = None
        imp[0, :4] = torch.tensor([0.0, 192.0, float(nq - 1), 3.0])
        imp[1, :3] = torch.tensor([1.0, float(nq), -1.0])
    dropout = torch.randint(1, nq + 1, (B,), generator=gen)
    gm = torch.randn(B, nq, T, generator=gen)
    return imp, levels, dropout, gm


def check_ste(imp, levels, dropout, gm, nq, alpha, n_imps, n_drop, tag):
    B, T = imp.shape
    m64, d64, p64 = G.mask_ste_ref(imp, levels, dropout, nq, alpha, n_imps, n_drop, gm, torch.float64)
    _, d32, _ = G.mask_ste_ref(imp, levels, dropout, nq, alpha, n_imps, n_drop, gm, torch.float32)
    if levels is not None:
        # a condition on the inputs: x = (imp level) nq rounds in fp32 by up to 2 ulp, which may
        # only move the sign of p where |p| <= 1e-6, the band the comparison leaves out
        x64 = p64[:, 0]
        band = (p64.abs() > 1e-6) & (p64.abs() < 4 * 2.0 ** -24 * x64.abs()[:, None, :])
        assert int(band[:n_imps].sum()) == 0
    impd = imp.reshape(B, 1, T).to(DEV).requires_grad_()
    m = train._MaskSte.apply(impd, None if levels is None else levels.to(DEV), dropout.to(DEV),
                             nq, alpha, n_imps, n_drop)
    dimp, = torch.autograd.grad((m * gm.to(DEV)).sum(), impd)
    m, dimp = m.detach().cpu(), dimp.reshape(B, T).cpu()
    # forward: the hard mask exactly; STE rows wherever |p| > 1e-6 or p = 0
    hard = (p64 >= 0).float()
    hard[n_imps:] = m64[n_imps:].float()
    sure = (p64.abs() > 1e-6) | (p64 == 0)
    sure[n_imps:] = True
    assert int((p64[:n_imps] == 0).sum()) > 0 or n_imps == 0
    assert torch.equal(m[sure], hard[sure]), tag
    assert bool(((m == 0) | (m == 1)).all())
    # backward
    assert torch.equal(dimp[n_imps:], torch.zeros(B - n_imps, T)), tag
    if n_imps == 0:
        return
    e, e32 = G.rel_err(dimp, d64), G.rel_err(d32, d64)
    print(f"mask_ste_backward {tag}: e={e:.3e} e32={e32:.3e}")
    assert e <= 4 * e32 + 2e-7, f"{tag}: e {e:.3e} > 4 * {e32:.3e} + 2e-7"


@pytest.mark.parametrize("split", [(0, 0), (5, 0), (2, 2)], ids=lambda s: f"imps{s[0]}-drop{s[1]}")
@pytest.mark.parametrize("with_levels", [False, True], ids=["x", "levels"])
@pytest.mark.parametrize("nq", [8, 32])
@pytest.mark.parametrize("alpha", [1.0, 2.0, 4.0])
def test_mask_ste_per_element_vs_fp64(alpha, nq, with_levels, split):
    imp, levels, dropout, gm = ste_inputs(nq, with_levels)
    check_ste(imp, levels, dropout, gm, nq, alpha, split[0], split[1],
              f"alpha={alpha} nq={nq} levels={with_levels} split={split}")


@pytest.mark.parametrize("x", [0.0, 3.0, 2.5, 192.0, -1.0])
def test_mask_ste_one_frame(x):
    """B T = 1."""
    nq, alpha = 32, 4.0
    gm = torch.randn(1, nq, 1, generator=torch.Generator().manual_seed(1))
    imp = torch.tensor([[x]])
    m64, d64, p64 = G.mask_ste_ref(imp, None, None, nq, alpha, 1, 0, gm, torch.float64)
    _, d32, _ = G.mask_ste_ref(imp, None, None, nq, alpha, 1, 0, gm, torch.float32)
    xd = imp.reshape(1, 1, 1).to(DEV).requires_grad_()
    m = train.mask_ste(xd, nq, alpha)
    dx, = torch.autograd.grad((m * gm.to(DEV)).sum(), xd)
    assert torch.equal(m.detach().cpu(), (p64 >= 0).float())
    e, e32 = G.rel_err(dx.cpu().reshape(1, 1), d64), G.rel_err(d32, d64)
    print(f"mask_ste_backward one frame x={x}: e={e:.3e} e32={e32:.3e} d64={float(d64):.3e}")
    assert e <= 4 * e32 + 2e-7


def test_mask_ste_forward_past_the_grid_cap():
    """B nq T = 65536 * 256 + 8 with every row an STE row: mask_ste_kernel's grid-stride loop
    wraps, and the eight elements past the 65536-block cap (the last clip's last stage, last
    eight frames) are computed values of both kinds. x is given in fp32, so the sign of
    p = x - i is exact and the hard mask is compared wherever |p| > 1e-6 or p = 0."""
    B, nq, T, alpha = 3, 8, 699051, 2.0
    assert B * nq * T == 65536 * 256 + 8
    gen = torch.Generator().manual_seed(12)
    x = torch.rand(B, T, generator=gen) * (nq + 2) - 1.0
    x[0, :4] = torch.tensor([0.0, 5.0, 192.0, -1.0])
    x[2, -8:] = torch.tensor([7.0, 9.0, 6.5, 7.5, 0.0, 8.0, 6.999, 7.001])
    m = ops.mask_ste(x.to(DEV), None, None, nq, alpha, B, 0).cpu()
    ar = torch.arange(nq, dtype=torch.float64)[None, :, None]
    p = x.double()[:, None, :] - ar
    sure = (p.abs() > 1e-6) | (p == 0)
    tail = (p >= 0).float()[2, nq - 1, -8:]
    assert tail.tolist() == [1, 1, 0, 1, 0, 1, 0, 1]
    assert torch.equal(m[2, nq - 1, -8:], tail)
    assert torch.equal(m[sure], (p >= 0).float()[sure])
