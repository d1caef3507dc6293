"""The planner over a wide grid (tests/conv_plan_grid.py: 675,648 shapes, every tap count, the
strided and transposed forms, four batch sizes, with and without x3 planes and a workspace)
against what the commit before conv_plan.h answered: per group the row count, the status
histogram and a hash of every row's status and plan, and the set of distinct plans. A rule that
moves any shape of the grid to another kernel, another status or a plan with no kernel behind it
(vrvq_conv_plan: VRVQ_ERR_UNSUPPORTED) shows here without a GPU."""
import json

import conv_plan_grid


def test_grid_matches_parent():
    with open(conv_plan_grid.GOLDEN) as f:
        want = json.load(f)
    got = conv_plan_grid.summary()
    assert sum(g["rows"] for g in want["groups"]) == 675648 and len(want["keys"]) == 161
    assert [g["group"] for g in got["groups"]] == [g["group"] for g in want["groups"]]
    bad = [(g, w) for g, w in zip(got["groups"], want["groups"]) if g != w]
    assert not bad, f"{len(bad)} of {len(want['groups'])} groups differ, first: {bad[:2]}"
    assert got["keys"] == want["keys"]
