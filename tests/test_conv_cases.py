"""The forward convs' case table (tests/conv_cases.py) checked on the host, through
vrvq_conv_plan: it reaches every plan the dispatch can choose, every case carries the edges its
plan admits, the table stays small, and the torch fp32 reference alone meets the condition the
GPU bar of tests/test_gpu_conv_edges.py is built on. No GPU needed (python -m vrvq_amd.build)."""
import pytest

import conv_cases as C
from vrvq_amd import _lib


def _table_plans():
    return {C.plan_key(c) for c in C.cases() if c.kind != "ru"}


def test_table_covers_every_fixture_plan():
    """The plans of the table's cases are a superset of the fixture's distinct plans, and each
    `plan` case runs the plan it is named for."""
    want = set(C.fixture_plans())
    assert len(want) >= 107
    uncovered = sorted(want - _table_plans())
    assert not uncovered, f"{len(uncovered)} plans without a case: {uncovered}"
    keys = [k for k in C.fixture_plans() if k[1] == 0] + C.EXTRA_PLANS
    cases = C.group("plan")
    assert len(cases) == len(keys) + 1
    for key, c in zip(keys, cases):
        assert C.plan_key(c) == key, c


def _direct_test_plans():
    """The plans of the direct kernel-versus-torch tests of test_gpu_parity.py, by case."""
    import test_gpu_parity as P

    def params(fn):
        (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
        return mark.args[1]

    def conv(case, x3):
        B, cin, cout, T, k, s, p, d = case[:8]
        return ("conv",) + tuple(_lib.conv_plan("conv", B, cin, T, cout, k, s, p, d, x3, True)[n]
                                 for n in C.PLAN_KEYS)

    def convt(case, x3):
        B, cin, cout, T, s = case
        return ("convt",) + tuple(
            _lib.conv_plan("convt", B, cin, T, cout, 2 * s, s, (s + 1) // 2, 1, x3, False)[n]
            for n in C.PLAN_KEYS)

    plans = {conv(c, False) for c in P.CONV_CASES}
    for c in list(P.X3_CONV_CASES) + list(params(P.test_conv1d_x3_long_rows_vs_torch)):
        plans |= {conv(c, False), conv(c, True)}
    for B, cin, cout, T, s, p, _snake in params(P.test_conv1d_strided_x3_vs_torch):
        c = (B, cin, cout, T, 2 * s, s, p, 1)
        plans |= {conv(c, False), conv(c, True)}
    for c in P.SPLITK_CASES:
        B, cin, cout, T, k, s, p, d = c[:8]
        plans.add(conv(c, True))
        plans.add(("conv",) + tuple(
            _lib.conv_plan("conv", B, cin, T, cout, k, s, p, d, True, False)[n]
            for n in C.PLAN_KEYS))
        plans.add(conv((1,) + tuple(c[1:]), True))
    plans |= {convt(c, False) for c in params(P.test_conv_transpose1d_vs_torch)}
    for c in params(P.test_conv_transpose1d_x3_vs_torch):
        plans |= {convt(c, False), convt(c, True)}
    return plans


def test_table_covers_the_direct_tests_plans():
    """Every plan the existing direct tests' cases produce has a case here; five of them are not
    in the fixture (32 x 128 k8 / k16 / 2-tap pair, the ConvTranspose's 32 x 128 on the fp32-input
    loop and on plain x3 chunks)."""
    direct = _direct_test_plans()
    assert not sorted(direct - _table_plans())
    assert direct - set(C.fixture_plans()) == set(C.EXTRA_PLANS)
    # what the direct tests leave to the table: plans they never compare with a reference
    assert len(set(C.fixture_plans()) - direct) >= 60


def _edges(c):
    """The edge properties of a case and whether its plan admits each, from the plan's BM / BN /
    chunk size: {name: (admitted, held)}."""
    p = C.plan_of(c)
    BM, BN, KS, x3, S = (p[n] for n in ("BM", "BN", "KS", "x3", "S"))
    convt = c.kind == "convt"
    view = c.kind == "conv" and c.stride > 1 and x3 > 0       # the phase-split view's GEMM
    M = c.cout * c.stride if convt else c.cout
    ng = c.tin + 1 if convt else C.out_len(c)
    gcin = c.cin * c.stride if view else c.cin
    ck = C.chunk_channels(KS, BM, BN, x3)
    whole = x3 == 2 or (KS == 2 and S > 0) or BN == 256      # rules that take whole chunks
    return {
        "B >= 2": (True, c.B >= 2),
        "three K chunks": (True, -(-gcin // ck) >= 3),
        "S parts of 8 chunks": (S > 0, S == 0 or -(-gcin // ck) // 8 == S),
        "ragged last chunk": (not whole, gcin % ck != 0 and c.cin % 8 != 0),
        "whole chunks": (whole, gcin % ck == 0),
        "ragged last N tile": (True, ng % BN != 0),
        "tout % 4 != 0": (not convt, C.out_len(c) % 4 != 0),
        # 192-row tiles, split-K, the 64 x 256 tile and the projection take whole row tiles
        "ragged last M tile": (BM != 192 and S == 0 and BN != 256 and c.kind != "proj",
                               M % BM != 0),
    }


def test_plan_cases_carry_their_edges():
    bad = []
    for c in C.group("plan"):
        for name, (admitted, held) in _edges(c).items():
            if admitted and not held:
                bad.append((c.name, name))
    assert not bad, bad
    # shape limits: B <= 3 but for the 96-wide rule's B = 48, T = 87 rows; dilation from {1, 3, 9}
    # but for the one case past the x3 window; one k7 case with pad = 27 > T
    for c in C.cases():
        assert c.B <= 3 or (c.B == 48 and (c.tin + (c.kind == "convt")) in (87, 88)
                            or C.out_len(c) in (87, 88)), c
        assert c.dil in (1, 3, 9) or c.name == "conv_64x256_k7_f32", c
    assert any(c.k == 7 and c.pad == 27 and c.pad > c.tin for c in C.group("plan"))
    assert {c.dil for c in C.group("plan") if c.k == 7} >= {1, 3, 9}


def test_epilogue_cases_cover_every_epilogue():
    """Each (kind, BM, BN) of the table's plans: a tout % 4 == 0 case with the next layer's Snake
    next to y (convs: residual and tanh too) and a y = NULL case (convs: sigmoid)."""
    epis = {(k[0], k[2], k[3]) for k in _table_plans() if k[1] == 0}
    seen = {}
    for c in C.group("epilogue"):
        p = C.plan_of(c)
        seen.setdefault((c.kind, p["BM"], p["BN"]), []).append(c)
    assert set(seen) == epis
    for e, (vec, noraw) in seen.items():
        assert vec.want_raw and not noraw.want_raw, e
        if e[0] != "convt":
            assert C.out_len(vec) % 4 == 0 and C.out_len(noraw) % 4 != 0, e
        if e[0] == "conv":
            assert vec.res and vec.out_snake and noraw.out_snake and {vec.epi, noraw.epi} == {1, 2}


def test_off_tile_and_unit_cases():
    """The kernels off the MFMA tiles are the ones their cases name, at the sizes where their
    code switches; the ResidualUnit cases sit around every unit's time tile."""
    off = {c.name: C.plan_of(c) for c in C.group("off")}
    for t, path in ((4, 2), (1024, 2), (1028, 2), (701, 0), (1027, 0)):
        assert off[f"cin1_k7_t{t}"]["path"] == path
        assert path == 2 or off[f"cin1_k7_t{t}"]["KS"] == 7
    rest = [c for c in C.group("off") if not c.name.startswith("cin1")]
    assert all(off[c.name]["path"] == 1 for c in rest)
    stream = [c for c in rest if c.name.startswith("cout1")]
    assert {(c.k, c.tin, c.cin) for c in stream} == \
        {(k, t, ci) for k in (7, 3) for t in (4, 8, 1024, 1028) for ci in (5, 8, 13)}
    small = [c for c in rest if c.name.startswith("small")]
    assert {(c.tin, c.dil) for c in small} == {(t, d) for t in (255, 256, 257, 600) for d in (1, 9)}
    assert {c.cin for c in small} == {5, 16, 17} and {c.cout for c in small} == {1, 3, 8}
    assert all(c.cin * c.k * 8 <= 2048 for c in small)
    for C_ in (64, 96, 128, 192, 256):
        bn = 64 if C_ >= 192 else 128
        for x3 in (True, False):
            mine = [c for c in C.group("ru") if c.cin == C_ and c.x3 == x3]
            assert {c.tin for c in mine} == {bn - 1, bn + 1, 2 * bn + 3, 5}
            assert {(c.tin, c.dil) for c in mine} == {(t, d) for t in {c.tin for c in mine}
                                                      for d in (1, 9)}
            assert {c.want_raw for c in mine} == {True, False}
    strides = {(c.stride, c.pad, c.tin) for c in C.group("convt")}
    assert strides == {(s, p, t) for s in (2, 4, 8, 3, 6) for p in (0, (s + 1) // 2)
                       for t in (1, 99)}


def test_table_stays_small():
    total = sum(C.floats(c) for c in C.cases())
    assert total < C.TOTAL_FLOATS_CAP, total
    for c in C.cases():
        assert c.B == 48 or C.floats(c) <= C.CASE_FLOATS_CAP, c


@pytest.mark.parametrize("name", ["plan", "epilogue", "convt", "off", "ru"])
def test_fp32_reference_meets_the_bars_condition(name):
    """u32, the torch fp32 result's distance from fp64 in units of 2^-24 of the terms' size, is
    at most 16 for every case: the bar 4 u32 + c of the GPU tests then stays a few tens of units
    (measured here: 1.0 .. 5.9)."""
    worst = (0.0, None)
    for c in C.group(name):
        d = C.inputs(c)
        ref, scale, y32 = C.reference(c, d)
        assert ref.shape == (c.B, c.cout, C.out_len(c))
        worst = max(worst, (C.units(y32, ref, scale), c.name))
    assert worst[0] <= 16, worst
