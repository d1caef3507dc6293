"""The quantizer-backward references, inputs and bars (tests/rvq_grad_ref.py), checked on the
CPU: the header comment of csrc/rvq_train.hip restated in einsums equals fp64 autograd of the
reference loop for every source, case and tensor; the decaying-residual and many-hits cases are
what they claim on the fp64 reference alone; and the bars that tests/test_gpu_rvq_backward.py
puts on the kernels bite: each deliberate mistake in the restated algebra fails them against
autograd64, the unmutated fp32 restatement passes them."""
import pytest
import torch

import rvq_grad_ref as G
import rvq_ref as R

# the case each mutant is judged on (the first where it changes anything: bdz of stage 7 needs
# nq >= 8, M_ji two stages, the first-clip sum two clips) and, beside it, the trained-regime one
MUTANT_CASES = ["9-1024-3-11", "decay"]


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_header_formulas_fp64_equal_autograd64(name):
    """rvq_train.hip lines 5-18 are the gradient: per element to 1e-12 of each tensor's largest
    value, for every source, exact zeros included."""
    c = G.case(name)
    for source in G.SOURCES:
        ref, h = G.autograd64(c, source), G.header_formulas(c, source, torch.float64)
        for nm in G.NAMES:
            if float(ref[nm].abs().max()) == 0.0:
                assert torch.equal(h[nm], ref[nm]), (source, nm)
            else:
                e = G.rel_err(h[nm], ref[nm])
                assert e < 1e-12, f"{name} {source} {nm}: {e:.3e}"


def test_sources_add_up_to_the_combined_gradient():
    """The three sources are the parts of the loss the older tests differentiate at once."""
    c = G.case("9-1024-3-11")
    leaves = [a.double().requires_grad_() for a in (c.z, c.mask) + tuple(c.params)]
    z_q, commit, cbl = G.rvq64(*leaves, c.codes)
    ((z_q * c.gz.double()).sum() + 0.25 * commit + cbl).backward()
    for nm, leaf in zip(G.NAMES, leaves):
        parts = (G.autograd64(c, "dzq")[nm] + 0.25 * G.autograd64(c, "commit")[nm]
                 + G.autograd64(c, "codebook")[nm])
        grad = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        assert G.rel_err(parts, grad) < 1e-12, nm


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_case_inputs_suit_check_codes(name):
    """What rvq_ref.check_codes needs of the inputs, on the fp64 reference alone: at most 0.25 %
    of the decisions are near-ties (none where a case has fewer than 400 decisions)."""
    c = G.case(name)
    ref = R.chain_fp64(c.z, c.params)
    assert torch.equal(ref.codes, c.codes)
    free = R.check_codes(ref.codes, c.z, c.params)
    assert free["share"] == 0.0 and free["worst"] == 0.0
    R.check_codes(R.chain_fp32(c.z, c.params).codes, c.z, c.params)
    near = R.near_tie_share(ref.dist, free["margin"])
    print(f"{name}: eps_d={free['eps_d']:.2e} near-ties={near:.4%}")
    assert near <= 0.0025


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_masks_have_binary_rows_fractions_and_dead_stages(name):
    c = G.case(name)
    nq, _, B, T = c.shape
    m = c.mask
    assert bool((m[:, 0] > 0).all())
    if B * T > 1:
        assert int(((m > 0) & (m < 1)).sum()) >= 2
        assert int((m == 1).sum()) > 0
    if nq >= 3:
        assert any(bool((m[0, i] == 0).all()) and bool((m[1:, i] != 0).any()) for i in range(nq))
    if nq >= 4:
        assert bool((m[:, nq - 2] == 0).all())
    if c.shape == G.DEAD_LAST_SHAPE:
        # nothing reaches the last stage's parameters from z_q: exact zeros in the reference,
        # which judge() then demands of the kernels bit for bit; dmask there is not zero
        assert bool((m[:, nq - 1] == 0).all())
        ref = G.autograd64(c, "dzq")
        for nm in ("dg_in", "dv_in", "db_in", "dg_out", "dv_out", "db_out"):
            assert float(ref[nm].reshape(nq, -1)[nq - 1].abs().max()) == 0.0, nm
        assert float(ref["dmask"][:, nq - 1].abs().min()) > 0.0


def test_decay_case_residual_falls_by_about_a_fifth_per_stage():
    c = G.case("decay")
    n = G.residual_norms(c)
    ratios = [n[i + 1] / n[i] for i in range(len(n) - 1)]
    print("decay |r_i+1| / |r_i|:", " ".join(f"{r:.3f}" for r in ratios), f"overall {n[-1] / n[0]:.4f}")
    assert len(ratios) == 16
    assert all(0.7 <= r <= 0.95 for r in ratios), ratios
    assert 0.75 ** 16 <= n[-1] / n[0] <= 0.85 ** 16
    # ... which is what makes dW_in a small difference of large terms: the corrections cancel
    # most of P_i at the late stages, and nothing of it in the random-codebook cases
    cond = G.conditioning(c, "dzq")
    print("decay max|P_i| / max|dW_in(i)|:", " ".join(f"{x:.1f}" for x in cond))
    assert max(cond[8:]) > 4.0 and max(cond) < G.DECAY_COND_MAX
    assert max(G.conditioning(G.case("9-1024-3-11"), "dzq")) < 2.0


def test_hits_case_sums_many_frames_of_both_clips_into_one_row():
    c = G.case("hits")
    nq, N, B, T = c.shape
    both, first = G.hit_counts(c)
    row = int(both[0].argmax())
    n_all, n_first = int(both[0, row]), int(first[0, row])
    print(f"hits: stage 0 row {row} chosen by {n_all} frames ({n_first} of the first clip); "
          f"rows never chosen per stage {(both == 0).sum(1).tolist()}")
    assert n_all >= 64 and 0 < n_first < n_all
    assert bool(((both == 0).sum(1) > 0).all())
    # the frames of that row carry weight: masked-on terms on both clips
    on = (c.codes[:, 0] == row) & (c.mask[:, 0] > 0)
    assert int(on[0].sum()) >= 16 and int(on[1].sum()) >= 16
    tot, s_abs = G.dcb_terms(c)
    ref = G.autograd64(c, "codebook")["dcb"]
    assert G.rel_err(tot, ref) < 1e-12
    assert bool((ref.abs() <= s_abs * (1 + 1e-12)).all())
    assert bool((s_abs[both == 0] == 0).all())


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_fp32_header_formulas_pass_the_bars(name):
    """The same algorithm in fp32 einsums is within the bars the kernels are held to. Its own
    error is one of the two yardsticks, so what this asks of the inputs is the 1e-5 cap and
    the exact zeros."""
    c = G.case(name)
    worst = 0.0
    for source in G.SOURCES:
        h = G.header_formulas(c, source, torch.float32)
        fails = G.judge(h, c, source)
        assert not fails, fails
        for nm in G.NAMES:
            for (_, a), (_, b) in zip(G.slices(nm, h[nm], c.shape[0]),
                                      G.slices(nm, G.autograd64(c, source)[nm], c.shape[0])):
                if float(b.abs().max()) > 0:
                    worst = max(worst, G.rel_err(a, b))
    print(f"{name}: worst e32h {worst:.2e}")


# what each mistake must break: source -> tensors of which at least one slice each fails; the
# sources a mutant is not listed under must come out clean (it is that mistake alone)
_COMMIT_ALL = {"dz", "dv_in", "db_in", "dv_out", "db_out"}
MUTANT_BREAKS = {
    "commit_dropped": {"commit": _COMMIT_ALL},
    "commit_x0.8": {"commit": _COMMIT_ALL},
    "commit_without_mask": {"commit": {"dz", "dv_in", "db_in"}},
    "inv_t_for_inv_bt": {"commit": _COMMIT_ALL, "codebook": {"dcb"}},
    "dm_without_bdz": {"dzq": {"dmask"}},
    "dw_in_without_sdz_cumb": {"dzq": {"dv_in"}, "commit": {"dv_in"}},
    "db_out_without_chain": {"dzq": {"db_out"}, "commit": {"db_out"}},
    "m_ji_dropped_for_last_stage": {"dzq": {"dz", "dv_in", "db_in"},
                                    "commit": {"dz", "dv_in", "db_in"}},
    "bdz7_from_stage0": {"dzq": {"dmask"}},
    "dcb_first_clip_only": {"codebook": {"dcb"}},
}


@pytest.mark.parametrize("name", MUTANT_CASES)
@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_bars_reject_mutant(mutant, name):
    """Each deliberate mistake, computed in fp64 so that nothing but the mistake separates it
    from the truth, fails the bars on every tensor it reaches, and leaves the sources it has no
    part in within them."""
    c = G.case(name)
    assert sorted(MUTANT_BREAKS) == sorted(G.MUTANTS)
    for source in G.SOURCES:
        fails = G.judge(G.header_formulas(c, source, torch.float64, mutate=mutant), c, source,
                        verbose=False)
        hit = {f.split()[2].rstrip(":").split("[")[0] for f in fails}
        want = MUTANT_BREAKS[mutant].get(source)
        if want is None:
            assert not fails, fails
        else:
            assert want <= hit, f"{mutant} on {name} {source}: the bars only see it in {sorted(hit)}"


def test_bars_see_a_late_stage_alone():
    """A stage judged on its own scale: the last stage's dv_in slice scaled by 1.001 fails,
    though it moves the stacked tensor's L2 norm by far less than the older 1e-4 bar."""
    c = G.case("32-1024-2-33")
    got = {k: v.clone() for k, v in G.autograd64(c, "dzq").items()}
    got["dv_in"][-8:] *= 1.001
    ref = G.autograd64(c, "dzq")["dv_in"]
    assert float((got["dv_in"] - ref).norm() / ref.norm()) < 1e-4
    fails = G.judge(got, c, "dzq", verbose=False)
    assert [f.split()[2].rstrip(":") for f in fails] == ["dv_in[31]"], fails
