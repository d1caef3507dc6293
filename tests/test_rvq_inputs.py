"""The RVQ tests' inputs and judge (tests/rvq_ref.py), checked on the CPU: the diverse recipe
really exercises the argmin (many distinct codes, every quarter of the codebook, few near-ties),
check_codes accepts the reference's own fp32 arithmetic and rejects corrupted codes, the fp64
reference breaks exact ties towards the lower index, and the recipe the older tests draw from is
near-constant (why the new inputs exist)."""
import pytest
import torch

import rvq_ref as R

from rvq_ref import DIVERSE_SHAPES, diverse_case


@pytest.mark.parametrize("nq,ncode,B,T,vbr", DIVERSE_SHAPES)
def test_diverse_inputs_exercise_the_argmin(nq, ncode, B, T, vbr):
    params, z, _ = diverse_case(nq, ncode, B, T, vbr)
    ref = R.chain_fp64(z, params)
    distinct = R.assert_diverse(ref.codes, ncode)
    c32 = R.chain_fp32(z, params).codes
    res = R.check_codes(c32, z, params)
    # on the reference's own codes the teacher-forced chain is the free-running one
    free = R.check_codes(ref.codes, z, params)
    assert free["share"] == 0.0 and free["worst"] == 0.0
    near = R.near_tie_share(ref.dist, free["margin"])
    print(f"distinct>={distinct} eps_d={res['eps_d']:.2e} margin={res['margin']:.2e} "
          f"fp32 mismatch={res['share']:.4%} near-ties={near:.4%}")
    assert near <= 0.0025  # half check_codes' cap: the cap is a condition on the inputs too


def test_check_codes_rejects_corrupted_codes():
    nq, ncode, B, T = 8, 1024, 3, 87
    params, z, _ = diverse_case(nq, ncode, B, T, True)
    ref = R.chain_fp64(z, params)
    ok = R.check_codes(ref.codes, z, params)
    margin = ok["margin"]
    top2 = ref.dist.topk(2, dim=2, largest=False)
    gap = top2.values[:, :, 1] - top2.values[:, :, 0]
    # one decision replaced by the fp64 second-best code, at a late stage (its own distances do
    # not depend on it) where the gap exceeds the margin
    b, i, t = 1, nq - 1, 40
    assert float(gap[b, i, t]) > margin
    bad = ref.codes.clone()
    bad[b, i, t] = top2.indices[b, i, 1, t]
    with pytest.raises(AssertionError, match="worse than the fp64 minimum"):
        R.check_codes(bad, z, params)
    # ... and at the first stage, where every later residual follows the wrong code
    assert float(gap[0, 0, 5]) > margin
    bad = ref.codes.clone()
    bad[0, 0, 5] = top2.indices[0, 0, 1, 5]
    with pytest.raises(AssertionError, match="worse than the fp64 minimum"):
        R.check_codes(bad, z, params)
    # one decision replaced by a random code
    bad = ref.codes.clone()
    bad[2, 3, 11] = (bad[2, 3, 11] + 517) % ncode
    with pytest.raises(AssertionError, match="worse than the fp64 minimum"):
        R.check_codes(bad, z, params)
    # a code outside the codebook
    bad = ref.codes.clone()
    bad[0, 0, 0] = -1
    with pytest.raises(AssertionError):
        R.check_codes(bad, z, params)


def test_judge_caps_the_share_of_near_tie_flips():
    """Synthetic distances: every decision has a second code within the margin. Flipping up to
    the cap passes, flipping more fails though each flip alone is within the margin."""
    B, nq, N, T = 2, 4, 16, 125                  # 1000 decisions
    gen = torch.Generator().manual_seed(3)
    d = torch.rand(B, nq, N, T, generator=gen, dtype=torch.float64) + 1.0
    best = torch.randint(0, N, (B, nq, T), generator=gen)
    second = (best + 5) % N
    d.scatter_(2, best[:, :, None, :], 0.5)
    d.scatter_(2, second[:, :, None, :], 0.5 + 1e-7)
    margin, cap = 8e-7, 0.005
    assert R.judge(best, d, margin, cap) == (0.0, 0.0)
    flat_best, flat_second = best.reshape(-1), second.reshape(-1)
    codes = flat_best.clone()
    codes[:5] = flat_second[:5]                  # 0.5 %: at the cap
    worst, share = R.judge(codes.reshape(B, nq, T), d, margin, cap)
    assert share == 0.005 and 0 < worst <= margin
    codes[5] = flat_second[5]                    # 0.6 %
    with pytest.raises(AssertionError, match="differ from the fp64 argmin"):
        R.judge(codes.reshape(B, nq, T), d, margin, cap)


@pytest.mark.parametrize("pattern", ["half", "pair", "mirror"])
@pytest.mark.parametrize("nq,ncode", [(8, 1024), (4, 768), (4, 256)])
def test_fp64_reference_breaks_ties_towards_the_lower_index(pattern, nq, ncode):
    params, gen = R.diverse_rvq_params(nq, ncode, 900 + nq + ncode)
    params = params._replace(cb=R.tie_codebook(params.cb, pattern))
    z = R.diverse_z(2, 87, gen)
    ref = R.chain_fp64(z, params)
    twin = R.twin_of(ref.codes, ncode, pattern)
    # every decision is an exact tie of the two twins
    d_twin = ref.dist.gather(2, twin[:, :, None, :])[:, :, 0, :]
    assert torch.equal(d_twin, ref.dist.min(2).values)
    assert bool(R.lower_twin(ref.codes, ncode, pattern).all())
    assert bool((twin > ref.codes).all())
    # the fp32 restatement ties exactly too, and takes the same twins
    c32 = R.chain_fp32(z, params).codes
    assert bool(R.lower_twin(c32, ncode, pattern).all())
    R.check_codes(c32, z, params)


def test_old_recipe_is_near_constant():
    """`_random_rvq`'s distributions (3-dim parameters at 0.05, biases at unit scale): z_e is the
    bias for every frame, so the fp64 codes take <= 4 distinct values per stage over 261 frames;
    the diverse recipe takes >= 100 on the same shape."""
    nq, ncode, B, T = 8, 1024, 3, 87
    params, gen = R.weak_rvq_params(nq, ncode, 1000 * nq + T)
    z = torch.randn(B, 1024, T, generator=gen) * 0.3
    weak = R.distinct_per_stage(R.chain_fp64(z, params).codes)
    assert max(weak) <= 4, weak
    with pytest.raises(AssertionError):
        R.assert_diverse(R.chain_fp64(z, params).codes, ncode)
    params, z, _ = diverse_case(nq, ncode, B, T, True)
    assert min(R.distinct_per_stage(R.chain_fp64(z, params).codes)) >= 100
