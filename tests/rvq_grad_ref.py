"""References, inputs and bars for the training-mode quantizer's backward (csrc/rvq_train.hip),
in plain torch on the CPU (no vrvq_amd import: tests/test_rvq_grad_ref.py checks this module
without a GPU; tests/test_gpu_rvq_backward.py judges the kernels with it).

References, one gradient SOURCE at a time ("dzq": (z_q gz).sum(), "commit": the commitment loss
alone, "codebook": the codebook loss alone), teacher-forced on given codes:
  autograd64 / autograd32   the reference loop `rvq64` under torch autograd, one forward and three
                            backward passes; fp64 is the truth, fp32 the project's yardstick e32;
  header_formulas           the algebra of rvq_train.hip's header comment (Q, bdz, dm, the reverse
                            chain with M_ji, S, P, G, the four fix-ups, dcb, dz) in einsums from
                            the forward state. In fp64 it equals autograd64 (which proves the
                            comment); in fp32 it is the yardstick e32h of the SAME algorithm, with
                            the kernels' cancellation in dW_in / dW_out; with `mutate` it is wrong
                            on purpose, to show that the bars see each mistake.

Bars (`judge`): per source, per tensor and per stage slice (dz and dmask whole),
e = rel_err(got, ref64) < 1e-5 and <= 4 e32 + 2e-7, the project's standing bar; a slice whose
fp64 reference is exactly zero must be exactly zero. HEADER_BARRED names the tensors (of the
decaying case only) whose yardstick is max(e32, e32h): there fp32 header_formulas itself misses
4 e32, so the algorithm's own cancellation, not a kernel's arithmetic, explains a miss.
header_formulas sums everything with einsums, in no kernel's order, so e32h excuses no
summation order of a kernel.

The nine gradients are those of vrvq_amd.train._RvqTrain's inputs: dz, dmask, dg_in, dv_in,
db_in, dg_out, dv_out, db_out, dcb, stacked over stages as rvq_ref.Params."""
import math

import numpy as np
import torch

import rvq_ref as R

NAMES = ["dz", "dmask", "dg_in", "dv_in", "db_in", "dg_out", "dv_out", "db_out", "dcb"]
SOURCES = ["dzq", "commit", "codebook"]
MUTANTS = ["commit_dropped", "commit_x0.8", "commit_without_mask", "inv_t_for_inv_bt",
           "dm_without_bdz", "dw_in_without_sdz_cumb", "db_out_without_chain",
           "m_ji_dropped_for_last_stage", "bdz7_from_stage0", "dcb_first_clip_only"]


# ------------------------------------------------------------------ the reference loop
def rvq64(z, mask, g_in, v_in, b_in, g_out, v_out, b_out, cb, codes):
    """The reference quantizer loop (models/quantize.py:42-79, 353-423) under autograd, in the
    precision of its arguments, with the given codes (argmin decisions fixed: the
    straight-through estimator only uses them as indices)."""
    nq, N, d = cb.shape
    D = z.shape[1]
    w_in = torch._weight_norm(v_in, g_in.reshape(-1, 1), 0).reshape(nq, d, D)
    w_out = torch._weight_norm(v_out, g_out.reshape(-1, 1), 0).reshape(nq, D, d)
    residual = z
    z_q = 0
    commit = 0
    cbl = 0
    for i in range(nq):
        z_e = torch.einsum("kc,bct->bkt", w_in[i], residual) + b_in[i][None, :, None]
        zq = cb[i][codes[:, i]].permute(0, 2, 1)                       # (B, d, T)
        commit_i = (z_e - zq.detach()).pow(2).mean(1)
        cbl_i = (zq - z_e.detach()).pow(2).mean(1)
        zst = z_e + (zq - z_e).detach()
        z_q_i = torch.einsum("cm,bmt->bct", w_out[i], zst) + b_out[i][None, :, None]
        residual = residual - z_q_i
        z_q = z_q + z_q_i * mask[:, i][:, None, :]
        commit = commit + commit_i * mask[:, i].detach()
        cbl = cbl + cbl_i * mask[:, i].detach()
    return z_q, commit.mean(), cbl.mean()


def logcosh64(alpha, pmk):  # models/utils.py:11-32 restated, in pmk's precision
    EPS = 1e-10
    mask1 = pmk >= 0
    pmk1 = pmk * mask1.detach()
    ms1 = (torch.log(math.exp(alpha) + torch.exp(-2 * pmk1 * alpha) + EPS)
           - torch.log(torch.exp(alpha * (-2 * pmk1 + 1)) + 1 + EPS)) / (2 * alpha) + 0.5
    mask2 = pmk < 0
    pmk2 = pmk * mask2.detach()
    ms2 = (torch.log(torch.exp(alpha * (2 * pmk2 + 1)) + 1 + EPS)
           - torch.log(math.exp(alpha) + torch.exp(alpha * 2 * pmk2) + EPS)) / (2 * alpha) + 0.5
    return ms1 * mask1 + ms2 * mask2


# ------------------------------------------------------------------ cases
class Case:
    """Inputs of one backward case (fp32 CPU tensors) and the codes the references are
    teacher-forced on: the fp64 argmin's by default, a kernel's through with_codes()."""

    def __init__(self, name, params, z, mask, gz, codes=None):
        self.name, self.params, self.z, self.mask, self.gz = name, params, z, mask, gz
        self.codes = R.chain_fp64(z, params).codes if codes is None else codes.detach().cpu().long()
        self.cache = {}

    @property
    def shape(self):
        nq, N, _ = self.params.cb.shape
        return nq, N, self.z.shape[0], self.z.shape[2]

    def with_codes(self, codes):
        codes = codes.detach().cpu().long()
        return self if torch.equal(codes, self.codes) else Case(self.name, self.params, self.z,
                                                                self.mask, self.gz, codes)


def make_mask(nq, B, T, gen, dead_last=False):
    """Rows of exact 0 / 1 (stage 0 always on), a few non-binary entries (the kernel is linear
    in m), stage 1 off for every frame of the first clip and, from nq = 4, stage nq - 2 off
    everywhere; dead_last: the last stage off everywhere too, so that nothing reaches its
    parameters under "dzq" and their gradients are exact zeros."""
    mask = (torch.rand(B, nq, T, generator=gen) < 0.7).float()
    mask[:, 0] = 1.0
    if B * T > 1:
        flat = mask.view(-1)
        idx = torch.randperm(flat.numel(), generator=gen)[:max(2, flat.numel() // 16)]
        flat[idx] = torch.tensor([0.3, 0.75])[torch.arange(idx.numel()) % 2]
    if nq >= 3:
        mask[0, 1] = 0.0
    if nq >= 4:
        mask[:, nq - 2] = 0.0
    if dead_last:
        mask[:, nq - 1] = 0.0
    return mask


# (nq, N, B, T): one seed per shape; test_rvq_grad_ref.py checks on the fp64 reference alone that
# the inputs suit rvq_ref.check_codes (near-ties)
PLAIN_SHAPES = [(1, 1024, 1, 1), (1, 1024, 2, 16), (8, 1024, 2, 32), (9, 1024, 3, 11),
                (32, 1024, 2, 33), (17, 256, 2, 20), (4, 768, 2, 40)]
DEAD_LAST_SHAPE = (8, 1024, 2, 32)      # nq = 8: bdz of the last stage is row 7 of the packed block
DECAY_SHAPE = (16, 1024, 2, 40)
DECAY_COND_MAX = 15.0
HITS_SHAPE = (3, 256, 2, 160)
CASE_NAMES = ["-".join(map(str, s)) for s in PLAIN_SHAPES] + ["decay", "hits"]
_cases = {}


def _plain_case(nq, N, B, T):
    params, gen = R.diverse_rvq_params(nq, N, 5300 + 100 * nq + T + B + N)
    z = R.diverse_z(B, T, gen)
    mask = make_mask(nq, B, T, gen, dead_last=(nq, N, B, T) == DEAD_LAST_SHAPE)
    gz = torch.randn(B, R.D_MODEL, T, generator=gen)
    return params, z, mask, gz


def _decay_case():
    """A trained model's regime: every stage sees (nearly) the same 8-dim projection A of the
    residual and removes a share of it, W_out(i) = (0.30 + 0.012 i) pinv(W_in(i)), with the
    codebook's scale following the residual's: |r_i| falls by ~0.8 per stage, so
    dW_in(i) = P_i - corrections cancels more and more of P_i. The seed keeps that cancellation,
    max|P_i| / max|dW_in(i)| in fp64, under DECAY_COND_MAX at every stage (a condition on the
    inputs, test_rvq_grad_ref.py): at 24 the fp32 restatement itself reaches 1.1e-5 in dv_in."""
    nq, N, B, T = DECAY_SHAPE
    D, d = R.D_MODEL, R.D_CODE
    gen = torch.Generator().manual_seed(8120)
    A = torch.randn(d, D, generator=gen, dtype=torch.float64) / math.sqrt(D)
    u = torch.randn(B, d, T, generator=gen, dtype=torch.float64)
    z = torch.einsum("ck,bkt->bct", torch.linalg.pinv(A), u)
    z = (z + 0.0005 * torch.randn(B, D, T, generator=gen, dtype=torch.float64)).float()
    g_in, v_in, b_in, g_out, v_out, b_out, cb = [], [], [], [], [], [], []
    r = z.double()
    for i in range(nq):
        w_in = A + 0.01 * torch.randn(d, D, generator=gen, dtype=torch.float64) / math.sqrt(D)
        w_out = (0.30 + 0.012 * i) * torch.linalg.pinv(w_in)
        z_e0 = torch.einsum("kc,bct->bkt", w_in, r)
        scale = float(z_e0.pow(2).mean().sqrt())
        bi = 0.02 * scale * torch.randn(d, generator=gen, dtype=torch.float64)
        bo = 0.02 * scale * torch.randn(D, generator=gen, dtype=torch.float64) / math.sqrt(D)
        cbi = scale * torch.randn(N, d, generator=gen, dtype=torch.float64)
        v_in.append(w_in.float()), g_in.append(w_in.float().norm(dim=1))
        v_out.append(w_out.float()), g_out.append(w_out.float().norm(dim=1))
        b_in.append(bi.float()), b_out.append(bo.float()), cb.append(cbi.float())
        p1 = R.Params(g_in[-1], v_in[-1], b_in[-1][None], g_out[-1], v_out[-1], b_out[-1][None],
                      cb[-1][None])
        r = r - R.chain_fp64(r, p1).z_q_is[:, 0]
    params = R.Params(torch.cat(g_in), torch.cat(v_in), torch.stack(b_in), torch.cat(g_out),
                      torch.cat(v_out), torch.stack(b_out), torch.stack(cb))
    mask = make_mask(nq, B, T, gen)
    gz = torch.randn(B, D, T, generator=gen)
    return params, z, mask, gz


def _hits_case():
    """Stage 0's in_proj bias is large next to W_in z, and a few codebook rows lie along it:
    one row is chosen by >= 64 frames of both clips, most rows of that stage by none."""
    nq, N, B, T = HITS_SHAPE
    params, gen = R.diverse_rvq_params(nq, N, 8642)
    b_in = params.b_in.clone()
    b_in[0] = b_in[0] / b_in[0].norm() * 4.0
    cb = params.cb.clone()
    cb[0, 5] = b_in[0] * 0.5
    cb[0, 200] = b_in[0] * 0.4 + 0.3 * cb[0, 200]
    params = params._replace(b_in=b_in, cb=cb)
    z = R.diverse_z(B, T, gen)
    mask = make_mask(nq, B, T, gen)
    mask[:, 0] = torch.where(torch.rand(B, T, generator=gen) < 0.8, 1.0, 0.3)  # hit stage: on
    gz = torch.randn(B, R.D_MODEL, T, generator=gen)
    return params, z, mask, gz


def case(name):
    if name not in _cases:
        if name == "decay":
            parts = _decay_case()
        elif name == "hits":
            parts = _hits_case()
        else:
            parts = _plain_case(*map(int, name.split("-")))
        _cases[name] = Case(name, *parts)
    return _cases[name]


def residual_norms(c):
    """|r_i| in fp64, i = 0 .. nq (r_0 = z), teacher-forced on the case's codes."""
    ref = R.chain_fp64(c.z, c.params, c.codes)
    r = c.z.double()
    out = [float(r.norm())]
    for i in range(ref.z_q_is.shape[1]):
        r = r - ref.z_q_is[:, i]
        out.append(float(r.norm()))
    return out


def hit_counts(c):
    """(nq, N) frames per codebook row, and the same over the first clip only."""
    nq, N, B, T = c.shape
    both = torch.stack([torch.bincount(c.codes[:, i].reshape(-1), minlength=N) for i in range(nq)])
    first = torch.stack([torch.bincount(c.codes[0, i], minlength=N) for i in range(nq)])
    return both, first


# ------------------------------------------------------------------ autograd references
def _zeros_for_none(grads, leaves):
    return [torch.zeros_like(a.detach()) if g is None else g for g, a in zip(grads, leaves)]


def _autograd(c, dtype):
    key = ("autograd", dtype)
    if key not in c.cache:
        leaves = [a.detach().clone().to(dtype).requires_grad_()
                  for a in (c.z, c.mask) + tuple(c.params)]
        z_q, commit, cbl = rvq64(*leaves, c.codes)
        losses = {"dzq": (z_q * c.gz.to(dtype)).sum(), "commit": commit, "codebook": cbl}
        out = {"forward": (z_q.detach(), commit.detach(), cbl.detach())}
        for src in SOURCES:
            g = torch.autograd.grad(losses[src], leaves, retain_graph=True, allow_unused=True)
            out[src] = dict(zip(NAMES, _zeros_for_none(g, leaves)))
        c.cache[key] = out
    return c.cache[key]


def autograd64(c, source):
    """The nine gradients of one source, fp64 autograd of rvq64."""
    return _autograd(c, torch.float64)[source]


def autograd32(c, source):
    """The same loop in fp32 on the CPU: the yardstick e32."""
    return _autograd(c, torch.float32)[source]


def forward64(c):
    """(z_q, commitment_loss, codebook_loss) in fp64."""
    return _autograd(c, torch.float64)["forward"]


# ------------------------------------------------------------------ the header's algebra
def _wn_backward(g, v, dw):
    n = v.norm(dim=1)
    dot = (dw * v).sum(1)
    return dot / n, (g / n)[:, None] * dw - (g * dot / n.pow(3))[:, None] * v


def _over_channels(eq, w, x):
    """einsum(eq, w, x) contracting the 1024 channels `c` in 32 blocks of 32 (eq names the block
    index `g`), the blocks then added by torch.sum: a blocked fp32 sum whose error does not
    depend on which path a machine's BLAS takes for a 1024-term dot."""
    ws = list(w.shape)
    ci = ws.index(R.D_MODEL)
    w = w.reshape(ws[:ci] + [32, 32] + ws[ci + 1:])
    x = x.reshape(x.shape[0], 32, 32, x.shape[2])
    return torch.einsum(eq, w, x).sum(1)


def header_formulas(c, source, dtype, mutate=None):
    """rvq_train.hip lines 5-18 in einsums (see the module docstring); mutate: one of MUTANTS.
    Besides the nine gradients it returns "_P" and "_dw_in" (nq, d, D), for the conditioning
    figure max|P_i| / max|dW_in(i)|, and "_dze" (B, nq d, T)."""
    assert source in SOURCES and (mutate is None or mutate in MUTANTS)
    key = ("header", source, dtype, mutate)
    if key in c.cache:
        return c.cache[key]
    p = R.Params(*(x.to(dtype) for x in c.params))
    z, m, codes = c.z.to(dtype), c.mask.to(dtype), c.codes
    nq, N, d = p.cb.shape
    B, D, T = z.shape
    w_in = torch._weight_norm(p.v_in, p.g_in.reshape(-1, 1), 0).reshape(nq, d, D)
    w_out = torch._weight_norm(p.v_out, p.g_out.reshape(-1, 1), 0).reshape(nq, D, d)
    # forward state as the forward kernels form it (csrc/rvq.hip lines 8-9), without the
    # residuals either: z_e(i) = ((W_in(i) z + b_in(i)) - Qb_i) - sum_{j<i} M_ij zst_j with
    # Qb_i = W_in(i) sum_{j<i} b_out(j); the chosen rows; the straight-through vectors
    # M[j][i] = W_in(j) W_out(i) (d, d) and Qb, as the training step forms them
    # (vrvq_rvq_cross_prep_precise): accumulated in fp64 from the weights, rounded once
    M = torch.einsum("jkc,icm->jikm", w_in.double(), w_out.double()).to(dtype)
    ze, zq, zst = [], [], []
    cumb = torch.zeros(D, dtype=dtype)
    for i in range(nq):
        e = (_over_channels("kgc,bgct->bgkt", w_in[i], z) + p.b_in[i][None, :, None]) \
            - (w_in[i].double() @ cumb.double()).to(dtype)[None, :, None]
        for j in range(i):
            e = e - torch.einsum("km,bmt->bkt", M[i][j], zst[j])
        q = p.cb[i][codes[:, i]].permute(0, 2, 1)
        ze.append(e), zq.append(q), zst.append(e + (q - e))
        cumb = cumb + p.b_out[i]
    dZ = c.gz.to(dtype) if source == "dzq" else torch.zeros_like(z)
    gc = 1.0 if source == "commit" else 0.0
    gcb = 1.0 if source == "codebook" else 0.0
    inv_bt = 1.0 / (T if mutate == "inv_t_for_inv_bt" else B * T)
    mi = [m[:, i][:, None, :] for i in range(nq)]
    Q = [_over_channels("gcm,bgct->bgmt", w_out[i], dZ) for i in range(nq)]
    bdz = [_over_channels("gc,bgct->bgt", p.b_out[i], dZ) for i in range(nq)]
    if mutate == "bdz7_from_stage0" and nq > 7:
        bdz[7] = bdz[0]
    dm = torch.stack([(Q[i] * zst[i]).sum(1) + (0 if mutate == "dm_without_bdz" else bdz[i])
                      for i in range(nq)], 1)
    # reverse chain
    gcm = {"commit_dropped": 0.0, "commit_x0.8": 0.8 * gc}.get(mutate, gc)
    dze = [None] * nq
    for i in range(nq - 1, -1, -1):
        acc = torch.zeros_like(Q[i])
        for j in range(i + 1, nq):
            if mutate == "m_ji_dropped_for_last_stage" and j == nq - 1:
                continue
            acc = acc + torch.einsum("km,bkt->bmt", M[j][i], dze[j])
        mc = 1.0 if mutate == "commit_without_mask" else mi[i]
        dze[i] = mi[i] * Q[i] - acc + (gcm * inv_bt) * mc * (0.25 * (ze[i] - zq[i]))
    dz = sum(torch.einsum("kc,bkt->bct", w_in[i], dze[i]) for i in range(nq))
    # weight gradients without the residuals
    S = [[torch.einsum("bkt,bmt->km", dze[i], zst[j]) for j in range(nq)] for i in range(nq)]
    sdz = [dze[i].sum((0, 2)) for i in range(nq)]
    P = [torch.einsum("bkt,bct->kc", dze[i], z) for i in range(nq)]
    dw_in, dw_out, db_out = [], [], []
    for i in range(nq):
        w = P[i]
        cumb = torch.zeros(D, dtype=dtype)
        for j in range(i):
            w = w - S[i][j] @ w_out[j].T
            cumb = cumb + p.b_out[j]
        if mutate != "dw_in_without_sdz_cumb":
            w = w - sdz[i][:, None] * cumb[None, :]
        dw_in.append(w)
        wo = torch.einsum("bct,bmt->cm", dZ, mi[i] * zst[i])
        bo = torch.einsum("bct,bt->c", dZ, m[:, i])
        for j in range(i + 1, nq):
            wo = wo - w_in[j].T @ S[j][i]
            if mutate != "db_out_without_chain":
                bo = bo - w_in[j].T @ sdz[j]
        dw_out.append(wo), db_out.append(bo)
    dcb = torch.zeros_like(p.cb)
    nb = 1 if mutate == "dcb_first_clip_only" else B
    for i in range(nq):
        f = (gcb * inv_bt) * mi[i] * (0.25 * (zq[i] - ze[i]))             # (B, d, T)
        dcb[i].index_add_(0, codes[:nb, i].reshape(-1), f[:nb].permute(0, 2, 1).reshape(-1, d))
    dw_in, dw_out = torch.stack(dw_in), torch.stack(dw_out)
    dg_in, dv_in = _wn_backward(p.g_in, p.v_in, dw_in.reshape(nq * d, D))
    dg_out, dv_out = _wn_backward(p.g_out, p.v_out, dw_out.reshape(nq * D, d))
    out = dict(zip(NAMES, [dz, dm, dg_in, dv_in, torch.stack(sdz), dg_out, dv_out,
                           torch.stack(db_out), dcb]))
    out["_P"], out["_dw_in"], out["_dze"] = torch.stack(P), dw_in, torch.cat(dze, 1)
    c.cache[key] = out
    return out


def conditioning(c, source):
    """max|P_i| / max|dW_in(i)| per stage, in fp64 (inf where dW_in(i) is zero): how much of the
    big GEMM the corrections cancel."""
    h = header_formulas(c, source, torch.float64)
    nq = c.shape[0]
    top = h["_P"].reshape(nq, -1).abs().max(1).values
    bot = h["_dw_in"].reshape(nq, -1).abs().max(1).values
    return [float(a / b) if float(b) > 0 else float("inf") for a, b in zip(top, bot)]


def dcb_terms(c, latents=None):
    """(sum, sum of absolute values), each (nq, N, d) in fp64, of the codebook gradient's terms
    gcb m_i / (B T) 2 (cb[n] - z_e_i) / 8 per codebook row and component (source "codebook",
    gcb = 1). latents (B, nq d, T): the z_e the terms are formed from -- the fp64 chain's by
    default (the sum is then autograd64's dcb), or a forward's stored fp32 latents, which is
    what the backward sums: the reduction bar then judges the sum alone."""
    nq, N, B, T = c.shape
    if latents is None:
        latents = R.chain_fp64(c.z, c.params, c.codes).latents
    lat = latents.detach().cpu().double().reshape(B, nq, R.D_CODE, T)
    cb = c.params.cb.double()
    tot = torch.zeros(nq, N, R.D_CODE, dtype=torch.float64)
    s_abs = torch.zeros_like(tot)
    for i in range(nq):
        zq = cb[i][c.codes[:, i]].permute(0, 2, 1)
        f = (c.mask[:, i].double()[:, None, :] / (B * T)) * (0.25 * (zq - lat[:, i]))
        f = f.permute(0, 2, 1).reshape(-1, R.D_CODE)
        tot[i].index_add_(0, c.codes[:, i].reshape(-1), f)
        s_abs[i].index_add_(0, c.codes[:, i].reshape(-1), f.abs())
    return tot, s_abs


# ------------------------------------------------------------------ bars
# case -> tensors judged by 4 max(e32, e32h) + 2e-7 instead of 4 e32 + 2e-7: only the decaying
# case's, whose projected z_e(i) = W_in(i) z - cross terms is a small difference of large terms
# (the reference loop forms it from the residual itself). fp32 header_formulas misses 4 e32 there
# too, and the kernels' misses (16 slices of db_in, db_out, dcb, dg_in, dv_out where they were
# measured) are within 4 e32h + 2e-7. Every other case is held to 4 e32 + 2e-7 alone.
HEADER_BARRED = {"decay": ("dg_in", "dv_in", "db_in", "dg_out", "dv_out", "db_out", "dcb")}


def rel_err(a, b):  # conftest.rel_err on tensors
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def slices(name, t, nq):
    """[(stage or None, 2-d view)]: dz and dmask whole, every other tensor per stage."""
    if name in ("dz", "dmask"):
        return [(None, t.reshape(1, -1))]
    return [(i, row) for i, row in enumerate(t.reshape(nq, -1))]


def judge(got, c, source, verbose=True, tag=""):
    """Judge the nine gradients `got` (dict by NAMES, any float dtype, CPU) of one source against
    autograd64 by the bars of the module docstring. Returns the failures as strings; prints
    e, e32 and e32h of every tensor and stage."""
    nq = c.shape[0]
    r64, r32 = autograd64(c, source), autograd32(c, source)
    r32h = header_formulas(c, source, torch.float32)
    fails = []
    for name in NAMES:
        g = got[name].detach().cpu()
        assert g.shape == r64[name].shape, (name, g.shape, r64[name].shape)
        rows = []
        for (i, a), (_, b64), (_, b32), (_, b32h) in zip(slices(name, g, nq), slices(name, r64[name], nq),
                                                         slices(name, r32[name], nq),
                                                         slices(name, r32h[name], nq)):
            where = f"{tag}{c.name} {source} {name}" + ("" if i is None else f"[{i}]")
            if float(b64.abs().max()) == 0.0:
                if not torch.equal(a, torch.zeros_like(a)):
                    fails.append(f"{where}: reference is exactly 0, got max {float(a.abs().max()):.3e}")
                continue
            if not bool(torch.isfinite(a).all()):
                fails.append(f"{where}: not finite")
                continue
            e, e32, e32h = rel_err(a, b64), rel_err(b32, b64), rel_err(b32h, b64)
            yard = max(e32, e32h) if name in HEADER_BARRED.get(c.name, ()) else e32
            ok = e < 1e-5 and e <= 4 * yard + 2e-7
            rows.append(f"{'' if i is None else i}:{e:.2e}/{e32:.2e}/{e32h:.2e}" + ("" if ok else "!"))
            if not ok:
                fails.append(f"{where}: e {e:.3e}, e32 {e32:.3e}, e32h {e32h:.3e}, "
                             f"bar {min(1e-5, 4 * yard + 2e-7):.3e}")
        if verbose and rows:
            print(f"{tag}{c.name} {source} {name} e/e32/e32h " + " ".join(rows))
    return fails


# ------------------------------------------------------------------ mask STE
def mask_ste_ref(imp, levels, dropout, nq, alpha, n_imps, n_drop, gm, dtype):
    """(mask, dimp, p) of the training mask (models/quantize.py:377-414) in `dtype` under
    autograd: rows < n_imps the STE of x = imp level nq (levels None: x = imp), then n_drop
    dropout rows, then ones; dimp the gradient of (mask gm).sum()."""
    B, T = imp.shape
    x = imp.detach().clone().to(dtype).requires_grad_()
    xs = x if levels is None else (x * levels.to(dtype)[:, None]) * nq
    ar = torch.arange(nq, dtype=dtype)[None, :, None]
    p = xs[:, None, :] - ar
    sm = logcosh64(alpha, p)
    m = (sm + ((p >= 0).to(dtype) - sm).detach()).clone()
    if n_drop:
        m[n_imps:n_imps + n_drop] = ((dropout[:n_drop].to(dtype)[:, None, None] - ar) >= 0).to(dtype)
    m[n_imps + n_drop:] = 1.0
    dimp, = torch.autograd.grad((m * gm.to(dtype)).sum(), x, allow_unused=True)
    dimp = torch.zeros_like(x.detach()) if dimp is None else dimp
    return m.detach(), dimp, p.detach()
