"""What the Python layer launches, pinned without a GPU: tests/launch_table.py walks every model
configuration of tests/golden/manifest.json plus one off-default width through the eval chained
path and the training step's convs, and the rows -- shape, planes yes / no, residual unit in one
launch or two, the planner's answer at 8 and 87 latent frames -- must equal
tests/golden/launch_table_parent.json, recorded from the commit before vrvq_amd/paths.py by that
commit's own prepared_x3 / runs_fused / train._x3 / _x3s.

The only rows allowed to differ are PLANES_DROPPED: convs of fewer than 8 input channels that
the parent's training step packed planes for and its layers did not. Their planes flip to no, and
their plan, asked with and without planes, is the same kernel off the MFMA tiles."""
import json

import pytest

import launch_table
from vrvq_amd import _lib, paths

# role -> why the parent's step reached it with planes: train._x3 had no Cin floor
PLANES_DROPPED = {
    "train/encoder.block.0": "the Cin = 1 first conv, forward",
    "train/decoder.model.6/adjoint": "adjoint of the Cout = 1 last decoder conv: Cin = 1",
    "train/quantizer.imp_subnet.blocks.4.1/adjoint":
        "adjoint of the importance subnet's Cout = 1 last conv: Cin = 1",
}
ROLE, KIND, CIN, COUT, K, STRIDE, PAD, DIL, PLANES, RU = range(10)


@pytest.fixture(scope="module")
def golden():
    with open(launch_table.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    return launch_table.tables()


def test_fixture_names_its_source(golden):
    head = golden["header"]
    assert len(head["commit"]) == 40 and "prepared_x3" in head["method"]
    assert set(golden["models"]) == set(launch_table.model_configs())
    assert "off_default_48_768" in golden["models"] and len(golden["models"]) >= 5


def test_same_launches_as_the_parent(golden, current):
    for name, want in golden["models"].items():
        got = json.loads(json.dumps(current[name]))
        assert [r[ROLE] for r in got] == [r[ROLE] for r in want], name
        dropped = set()
        for g, w in zip(got, want):
            if g == w:
                continue
            assert g[ROLE] in PLANES_DROPPED, (name, g, w)
            assert w[PLANES] == 1 and g[PLANES] == 0 and g[CIN] < 8, (name, g, w)
            assert g[:PLANES] + g[PLANES + 1:] == w[:PLANES] + w[PLANES + 1:], (name, g, w)
            dropped.add(g[ROLE])
        has = {r[ROLE] for r in want}
        assert dropped == set(PLANES_DROPPED) & has, name


def test_dropped_planes_change_no_plan(golden):
    """Every PLANES_DROPPED row, at both lengths: the planner's answer with planes is its answer
    without them, and it is a kernel off the MFMA tiles (path 1 small Cout, path 2 Cin = 1)."""
    seen = set()
    for name, rows in golden["models"].items():
        for r in rows:
            if r[ROLE] not in PLANES_DROPPED:
                continue
            seen.add(r[ROLE])
            for tin in (r[10], r[12]):
                args = (r[KIND], 1, r[CIN], tin, r[COUT], r[K], r[STRIDE], r[PAD], r[DIL])
                with_planes = _lib.conv_plan(*args, True, True)
                assert with_planes == _lib.conv_plan(*args, False, True), (name, r)
                assert with_planes["path"] in (1, 2) and with_planes["x3"] == 0, (name, r)
    assert seen == set(PLANES_DROPPED)


def test_every_form_is_in_the_table(golden):
    rows = [r for m in golden["models"].values() for r in m]
    assert {r[RU] for r in rows} == {"", "fused", "two"}
    assert {r[KIND] for r in rows} == {"conv", "proj", "convt", "ru"}
    assert {r[CIN] for r in rows if r[RU] == "fused"} == {64, 96, 128}
    assert {48, 192, 256, 384, 512, 768} <= {r[CIN] for r in rows if r[RU] == "two"}
    assert {r[PLANES] for r in rows} == {0, 1, "1,1"}
    assert any(r[ROLE].endswith("/adjoint") and r[KIND] == "convt" for r in rows)
    assert any(r[ROLE].endswith("/adjoint") and r[STRIDE] > 1 and r[KIND] == "conv" for r in rows)


def test_residual_unit_rule():
    for x3 in (True, False):
        assert [c for c in (48, 64, 96, 128, 192, 256, 384, 512, 768) if paths.ru_fused(c, x3)] \
            == [64, 96, 128] + ([] if x3 else [256])
