"""Inputs and references for the RVQ argmin tests, in plain torch on the CPU (no vrvq_amd import:
tests/test_rvq_inputs.py checks this module without a GPU).

Inputs. The quantizer tests used to draw every 3-dim parameter at 0.05 and biases at unit scale
(`_random_rvq`): z_e is then the bias for every frame and each stage picks 1 to 3 distinct codes, so
a scan that is wrong over part of the index range goes unseen. `diverse_rvq_params` / `diverse_z`
use the training tests' recipe (weight_g ~ U(0.5, 1.5), in_proj v ~ 0.03 N, out_proj v ~ 0.3 N,
biases 0.1 N, codebook N(0, 1), z ~ 0.5 N): hundreds of distinct codes per stage, every 256-code
quarter of the codebook hit. `assert_diverse` keeps it so. `tie_codebook` duplicates rows so that
every decision is an exact tie of two indices.

Reference. `chain_fp64` restates the reference loop (models/quantize.py:42-103, 353-421) in
fp64, either with its own argmin or teacher-forced on given codes; `chain_fp32` is the same loop
at the precision the reference model runs at. `check_codes` judges EVERY decision of a code
tensor: teacher-forced on those codes, the chosen code's fp64 distance may exceed the stage's
minimum by at most margin = 8 eps_d, and at most `cap` of the decisions may differ from the
fp64 argmin of their stage. eps_d is the largest |d32 - d64| over all decisions and codes
between chain_fp32 and chain_fp64 teacher-forced on the same codes -- the reference arithmetic's
own error, never a kernel's: a pick made from distances each within eps of the truth can be
suboptimal by 2 eps, and the factor 4 on top is the project's allowance for a reordered fp32
evaluation (e3 <= 4 e32, test_x3_error_over_the_whole_chain).

Parameters are the stacked per-stage tensors of vrvq_amd.train._stage_params: g_in (nq*d,),
v_in (nq*d, D), b_in (nq, d), g_out (nq*D,), v_out (nq*D, d), b_out (nq, D), cb (nq, N, d)."""
from collections import namedtuple

import torch
import torch.nn.functional as F

D_MODEL, D_CODE = 1024, 8

Params = namedtuple("Params", "g_in v_in b_in g_out v_out b_out cb")
Chain = namedtuple("Chain", "codes dist z_q_is latents")


# ------------------------------------------------------------------ inputs
def diverse_rvq_params(nq, ncode, seed, D=D_MODEL, d=D_CODE):
    """(Params, generator): the training tests' recipe (tests/test_gpu_train.py
    _random_quantizer), fp32 CPU tensors; the generator goes on to draw z / imp."""
    gen = torch.Generator().manual_seed(seed)
    g_in = torch.rand(nq * d, generator=gen) + 0.5
    v_in = torch.randn(nq * d, D, generator=gen) * 0.03
    b_in = torch.randn(nq, d, generator=gen) * 0.1
    g_out = torch.rand(nq * D, generator=gen) + 0.5
    v_out = torch.randn(nq * D, d, generator=gen) * 0.3
    b_out = torch.randn(nq, D, generator=gen) * 0.1
    cb = torch.randn(nq, ncode, d, generator=gen)
    return Params(g_in, v_in, b_in, g_out, v_out, b_out, cb), gen


def diverse_z(B, T, gen, D=D_MODEL):
    return torch.randn(B, D, T, generator=gen) * 0.5


# (nq, ncode, B, T, vbr) of test_rvq_diverse_vs_fp64: every codebook size (N / 256 = 1 .. 4), odd
# nq, nq = 1 / 28 / 32, partial frame tiles, T > 96, VBR and CBR; the last four are the shapes
# only the retired projection-variant test covered (T = 97: the fused entry takes three launches
# and the expansion two windows; one frame; odd nq at T = 200 and 40)
DIVERSE_SHAPES = [
    (8, 1024, 3, 87, True), (32, 1024, 2, 87, True), (4, 256, 3, 40, True), (4, 512, 2, 87, True),
    (4, 768, 2, 40, False), (9, 1024, 2, 87, True), (1, 1024, 4, 87, False),
    (8, 1024, 5, 200, True), (28, 1024, 2, 70, True), (8, 1024, 2, 13, True),
    (12, 1024, 2, 97, True), (2, 1024, 1, 1, True), (9, 1024, 2, 200, True), (5, 1024, 3, 40, True)]


def diverse_case(nq, ncode, B, T, vbr=True):
    """(params, z, imp) of one shape, one seed per shape, shared by the CPU and the GPU tests.
    The seeds are a condition on the inputs that tests/test_rvq_inputs.py checks on the fp64
    reference alone: at most 0.25 % of the decisions are near-ties (at nq = 1 the 348 decisions
    allow none: one would be 0.29 %)."""
    params, gen = diverse_rvq_params(nq, ncode, 7100 + 100 * nq + T + B + ncode)
    z = diverse_z(B, T, gen)
    imp = torch.rand(B, T, generator=gen) if vbr else None
    return params, z, imp


def weak_rvq_params(nq, ncode, seed, D=D_MODEL, d=D_CODE):
    """`_random_rvq`'s distributions (tests/test_gpu_parity.py), drawn in stage order: every 3-dim
    parameter (weight_g, weight_v) at 0.05 N, biases and codebooks N(0, 1). Kept to record why
    the diverse inputs exist: z_e is the bias for every frame."""
    gen = torch.Generator().manual_seed(seed)
    rows = {k: [] for k in Params._fields}
    for _ in range(nq):
        for name, n_out, n_in in (("in", d, D), ("out", D, d)):
            rows["b_" + name].append(torch.randn(n_out, generator=gen))
            rows["g_" + name].append(torch.randn(n_out, generator=gen) * 0.05)
            rows["v_" + name].append(torch.randn(n_out, n_in, generator=gen) * 0.05)
        rows["cb"].append(torch.randn(ncode, d, generator=gen))
    p = Params(torch.cat(rows["g_in"]), torch.cat(rows["v_in"]), torch.stack(rows["b_in"]),
               torch.cat(rows["g_out"]), torch.cat(rows["v_out"]), torch.stack(rows["b_out"]),
               torch.stack(rows["cb"]))
    return p, gen


def tie_codebook(cb, pattern):
    """cb (nq, N, d) with every row duplicated at a second index, in every stage:
    "half" cb[N/2 + j] = cb[j], "pair" cb[2m + 1] = cb[2m], "mirror" cb[N - 1 - j] = cb[j]."""
    cb = cb.clone()
    N = cb.shape[1]
    h = N // 2
    if pattern == "half":
        cb[:, h:] = cb[:, :h]
    elif pattern == "pair":
        cb[:, 1::2] = cb[:, 0::2]
    elif pattern == "mirror":
        cb[:, h:] = cb[:, :h].flip(1)
    else:
        raise ValueError(pattern)
    return cb


def lower_twin(codes, ncode, pattern):
    """True where a code is the lower index of its pair under tie_codebook(pattern)."""
    return codes % 2 == 0 if pattern == "pair" else codes < ncode // 2


def twin_of(codes, ncode, pattern):
    h = ncode // 2
    if pattern == "pair":
        return codes ^ 1
    if pattern == "half":
        return (codes + h) % ncode
    return ncode - 1 - codes


# ------------------------------------------------------------------ the reference loop
def _chain(z, params, codes, dtype):
    p = Params(*(x.detach().to("cpu", dtype) for x in params))
    z = z.detach().to("cpu", dtype)
    nq, N, d = p.cb.shape
    B, D, T = z.shape
    w_in = torch._weight_norm(p.v_in, p.g_in.reshape(-1, 1), 0).reshape(nq, d, D)
    w_out = torch._weight_norm(p.v_out, p.g_out.reshape(-1, 1), 0).reshape(nq, D, d)
    if codes is not None:
        codes = codes.detach().cpu().long()
    r = z.clone()
    out_codes, dists, z_q_is, lat = [], [], [], []
    for i in range(nq):
        z_e = torch.einsum("kc,bct->bkt", w_in[i], r) + p.b_in[i][None, :, None]
        e = F.normalize(z_e, dim=1)
        cn = F.normalize(p.cb[i], dim=1)
        # the dot one term at a time: a row's distance does not depend on where the row sits, so
        # duplicated rows tie exactly and argmin returns the lower index
        dot = torch.zeros(B, N, T, dtype=dtype)
        for k in range(d):
            dot += e[:, k, None, :] * cn[None, :, k, None]
        e2 = torch.zeros(B, 1, T, dtype=dtype)
        c2 = torch.zeros(1, N, 1, dtype=dtype)
        for k in range(d):
            e2 += e[:, k, None, :] ** 2
            c2 += cn[None, :, k, None] ** 2
        dist = e2 - 2 * dot + c2
        idx = dist.argmin(1) if codes is None else codes[:, i]
        zq = p.cb[i][idx].permute(0, 2, 1)
        q = torch.einsum("ck,bkt->bct", w_out[i], zq) + p.b_out[i][None, :, None]
        r = r - q
        out_codes.append(idx)
        dists.append(dist)
        z_q_is.append(q)
        lat.append(z_e)
    return Chain(torch.stack(out_codes, 1), torch.stack(dists, 1), torch.stack(z_q_is, 1),
                 torch.cat(lat, 1))


def chain_fp64(z, params, codes=None):
    """Chain(codes (B, nq, T), dist (B, nq, N, T), z_q_is (B, nq, D, T), latents (B, nq*d, T)) in
    fp64; codes=None takes the argmin (lowest index on a tie), else stage i's residual follows
    the given codes."""
    return _chain(z, params, codes, torch.float64)


def chain_fp32(z, params, codes=None):
    return _chain(z, params, codes, torch.float32)


def mask_fp64(imp, level, nq, B, T):
    """models/utils.py:55-61: stage i of frame t is kept when imp * level * nq - i >= 0."""
    if imp is None:
        return torch.ones(B, nq, T, dtype=torch.float64)
    s = imp.detach().double().cpu()[:, None, :] * level * nq
    return (s - torch.arange(nq, dtype=torch.float64)[None, :, None] >= 0).double()


# ------------------------------------------------------------------ judging codes
def judge(codes, d64, margin, cap):
    """Every decision (b, i, t) of `codes` against its stage's fp64 distances d64 (B, nq, N, T):
    excess = d64[code] - min_n d64 <= margin, and the share of decisions that differ from the
    fp64 argmin <= cap. Returns (worst excess, mismatch share)."""
    codes = codes.detach().cpu().long()
    N = d64.shape[2]
    assert codes.shape == (d64.shape[0], d64.shape[1], d64.shape[3]), (codes.shape, d64.shape)
    assert int(codes.min()) >= 0 and int(codes.max()) < N, (int(codes.min()), int(codes.max()))
    chosen = d64.gather(2, codes[:, :, None, :])[:, :, 0, :]
    best, arg = d64.min(2)
    excess = chosen - best
    worst = float(excess.max())
    share = float((codes != arg).double().mean())
    n_bad = int((excess > margin).sum())
    assert n_bad == 0, (f"{n_bad} of {codes.numel()} decisions are worse than the fp64 minimum by "
                        f"more than the margin {margin:.3e} (worst {worst:.3e}); first at "
                        f"(b, stage, t) = {tuple((excess > margin).nonzero()[0].tolist())}")
    assert share <= cap, f"{share:.4%} of the decisions differ from the fp64 argmin (cap {cap:.2%})"
    return worst, share


def near_tie_share(d64, margin):
    """Share of decisions whose fp64 top-2 gap is under margin."""
    top2 = d64.topk(2, dim=2, largest=False).values
    return float(((top2[:, :, 1] - top2[:, :, 0]) < margin).double().mean())


def check_codes(codes, z, params, cap=0.005):
    """See the module docstring. Returns the figures: eps_d, margin, worst excess, mismatch share,
    the teacher-forced fp64 chain."""
    ref = chain_fp64(z, params, codes)
    d32 = chain_fp32(z, params, codes).dist
    eps_d = float((d32.double() - ref.dist).abs().max())
    margin = 8 * eps_d
    worst, share = judge(codes, ref.dist, margin, cap)
    return {"eps_d": eps_d, "margin": margin, "worst": worst, "share": share, "ref": ref}


def distinct_per_stage(codes):
    codes = codes.detach().cpu()
    return [int(codes[:, i].unique().numel()) for i in range(codes.shape[1])]


def assert_diverse(codes, ncode):
    """Per stage >= min(frames, ncode) / 8 distinct codes, and with >= 80 frames and >= 512 codes
    every 256-code quarter of the codebook occurs. Returns the smallest distinct count."""
    codes = codes.detach().cpu()
    B, nq, T = codes.shape
    frames = B * T
    distinct = distinct_per_stage(codes)
    need = min(frames, ncode) / 8
    assert min(distinct) >= need, f"distinct codes per stage {distinct}, need >= {need}"
    if frames >= 80 and ncode >= 512:
        for i in range(nq):
            quarters = set((codes[:, i] // 256).unique().tolist())
            assert quarters == set(range((ncode + 255) // 256)), (i, quarters)
    return min(distinct)
