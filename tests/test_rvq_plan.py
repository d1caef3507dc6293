"""The launch plan of vrvq_rvq_encode_part, answered on the host (include/vrvq.h vrvq_rvq_plan)
and pinned by tests/golden/rvq_plan_parent.json: what the commit before the plan existed returned
from vrvq_rvq_workspace_part / vrvq_rvq_workspace (host only) for frames x nq x ncode x batch over
{1, 7, 15, 16, 17, 40, 87, 96, 97, 200, 862} x {1, 2, 5, 8, 9, 12, 28, 32} x {256 .. 1024} x
{1, 3, 32, 64} plus rejected shapes (`host`: the arguments, each call's status and bytes), and,
on an MI355X, from vrvq_rvq_fused_clips for 22 of those shapes (`clips`).

The plan's geometry shows in those bytes: the granule area of a captured launch is
batch x nq x P x 16 frames x 8 dims x 8 B behind the 8448-byte sync block, and it always exceeds
the two-launch form's zst rows (batch x nq x frames x 32 B, frames <= 16 P)."""
import ctypes
import json
import os

import pytest

from vrvq_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SYNC_BYTES = 8448
# the host part's resident count: geometry and workspace do not depend on it; small enough that a
# 10-s clip at nq = 32 does not fit, so both kinds of plan occur
ANY_RESIDENT = 128


def fixture():
    with open(os.path.join(HERE, "golden", "rvq_plan_parent.json")) as f:
        return json.load(f)


def test_workspace_and_geometry_match_parent_record():
    rows = fixture()["host"]
    assert len(rows) > 1400
    lib = _lib.load()
    assert lib.vrvq_version() >= 105
    n = ctypes.c_longlong(0)
    out = (ctypes.c_longlong * 10)()
    for batch, frames, nq, ncode, status_part, ws_part, status, ws in rows:
        row = (batch, frames, nq, ncode)
        assert lib.vrvq_rvq_workspace_part(batch, frames, nq, ncode, ctypes.byref(n)) == status_part, row
        assert status_part or n.value == ws_part, row
        assert lib.vrvq_rvq_workspace(batch, frames, nq, ctypes.byref(n)) == status, row
        assert status or n.value == ws, row
        assert lib.vrvq_rvq_plan(batch, frames, nq, ncode, ANY_RESIDENT, out) == status_part, row
        if status_part:
            continue
        plan = _lib.rvq_plan(batch, frames, nq, ncode, ANY_RESIDENT)
        assert [plan[k] for k in _lib.RVQ_PLAN_KEYS] == list(out), row
        assert plan["ws_bytes"] == ws_part, row
        assert plan["P"] * batch * nq * 1024 == ws_part - SYNC_BYTES, row
        assert 1 <= plan["F"] <= 16 and plan["lds"] <= 80 * 1024, row
        assert -(-frames // plan["F"]) == plan["P"], row
        assert plan["n_fb"] == -(-frames // 96), row
        assert plan["wg_per_clip"] == plan["P"] + 8 * plan["n_fb"], row
        assert plan["resident"] == ANY_RESIDENT, row
        # clips per launch and launches follow from the resident count alone
        clips = min(ANY_RESIDENT // plan["wg_per_clip"], batch)
        if clips:
            assert (plan["kind"], plan["clips"], plan["launches"]) == \
                (_lib.RVQ_PLAN_PT, clips, -(-batch // clips)), row
        else:
            assert (plan["kind"], plan["clips"], plan["launches"]) == \
                (_lib.RVQ_PLAN_CHAIN_EXPAND, 0, 2), row


def test_encode_workspace_bound_covers_partials_and_plan():
    """vrvq_rvq_workspace keeps the parent's bytes (the `ws` column, checked above) as an upper
    bound: vrvq_rvq_encode needs the projection partials (8 splits x B T x 8 nq floats) followed
    by the plan's workspace, and that fits at every accepted shape of the fixture."""
    lib = _lib.load()
    n = ctypes.c_longlong(0)
    accepted = 0
    for batch, frames, nq, ncode, status_part, _ws_part, status, _ws in fixture()["host"]:
        if status_part or status:
            continue
        accepted += 1
        assert lib.vrvq_rvq_workspace(batch, frames, nq, ctypes.byref(n)) == 0
        need = 256 * batch * frames * nq + \
            _lib.rvq_plan(batch, frames, nq, ncode, ANY_RESIDENT)["ws_bytes"]
        assert need <= n.value, (batch, frames, nq, ncode)
    assert accepted > 1400


def test_fixture_covers_the_rules():
    fx = fixture()
    assert {r[4] for r in fx["host"]} == {0, 10001, 10002}
    plans = [_lib.rvq_plan(*r[:4], ANY_RESIDENT) for r in fx["host"] if r[4] == 0]
    assert {p["F"] for p in plans} >= {1, 7, 15, 16}          # short clips and the full 16
    assert any(p["F"] < 16 and p["P"] > 1 for p in plans)      # the chain's LDS forcing fewer
    assert {p["n_fb"] for p in plans} == {1, 2, 3, 9}
    assert {p["kind"] for p in plans} == {_lib.RVQ_PLAN_PT, _lib.RVQ_PLAN_CHAIN_EXPAND}
    assert any(p["launches"] > 2 for p in plans)
    assert 18 <= len(fx["clips"]) <= 24


def test_plan_hooks_and_bad_calls():
    lib = _lib.load()
    out = (ctypes.c_longlong * 10)()
    assert lib.vrvq_rvq_plan(3, 87, 8, 1024, 512, None) == 10001
    assert lib.vrvq_rvq_plan(3, 87, 8, 1024, -1, out) == 10001
    assert lib.vrvq_rvq_plan(3, 87, 33, 1024, 512, out) == 10002
    assert _lib.rvq_plan(64, 87, 8, 1024, 512)["clips"] == 36
    prev = _lib.rvq_debug_capacity(2)
    try:
        capped = _lib.rvq_plan(5, 40, 4, 256, 512)
        assert (capped["kind"], capped["clips"], capped["launches"]) == (_lib.RVQ_PLAN_PT, 2, 3)
        _lib.rvq_debug_capacity(0)
        assert _lib.rvq_plan(5, 40, 4, 256, 512)["kind"] == _lib.RVQ_PLAN_CHAIN_EXPAND
    finally:
        _lib.rvq_debug_capacity(prev)
    prev = _lib.rvq_path(1)
    try:
        three = _lib.rvq_plan(5, 40, 4, 256, 512)
        assert (three["kind"], three["clips"], three["launches"]) == \
            (_lib.RVQ_PLAN_CHAIN_EXPAND, 0, 2)
    finally:
        _lib.rvq_path(prev)
    assert _lib.rvq_plan(5, 40, 4, 256, 512)["clips"] == 5


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
def test_fused_clips_match_parent_record():
    """vrvq_rvq_fused_clips as the parent returned it on an MI355X, and the host-only plan fed
    with the device's resident count agrees with it."""
    for frames, nq, ncode, clips in fixture()["clips"]:
        row = (frames, nq, ncode)
        assert _lib.rvq_fused_clips(frames, nq, ncode) == clips, row
        on_device = _lib.rvq_plan(64, frames, nq, ncode)
        assert on_device["resident"] > 0, row
        host = _lib.rvq_plan(64, frames, nq, ncode, on_device["resident"])
        assert host == on_device, row
        assert host["clips"] == min(clips, 64), row


@pytest.mark.gpu
@pytest.mark.parametrize("cap,B,T,nq,ncode", [(2, 5, 40, 4, 256), (1, 3, 97, 8, 1024)])
def test_chunked_launches_match_three_launches(cap, B, T, nq, ncode):
    """A call split into consecutive rvq_pt_kernel launches by the capacity cap (each chunk's
    inputs and outputs offset into the call's; z is absent on this path): all six outputs equal
    the three launches bit for bit, with and without z_q_is, in the 3 launches the plan says."""
    import torch
    from test_gpu_parity import _random_rvq
    from test_gpu_rvq_part import DEV, _equal, _part_call, _project, _three_launches
    q, gen = _random_rvq(nq, ncode, 4000 + 10 * nq + T)
    st = q.stacked()
    z = (torch.randn(B, 1024, T, generator=gen) * 0.3).to(DEV)
    imp = torch.rand(B, T, generator=gen).to(DEV)
    part = _project(z, st)
    prev = _lib.rvq_debug_capacity(cap)
    try:
        plan = _lib.rvq_plan(B, T, nq, ncode)
        assert (plan["kind"], plan["clips"], plan["launches"]) == (_lib.RVQ_PLAN_PT, cap, 3)
        for zqis in (True, False):
            want = _three_launches(z, st, imp, 0.8, zqis)
            _lib.rvq_timing_read()
            prev_t = _lib.rvq_timing(True)
            try:
                got = _part_call(part, T, st, imp, 0.8, zqis)
                torch.cuda.synchronize()
                assert _lib.rvq_timing_read()[1] == 3
            finally:
                _lib.rvq_timing(prev_t)
            _equal(got, want)
            assert (got[3] is None) == (not zqis)
    finally:
        _lib.rvq_debug_capacity(prev)
    assert _lib.rvq_sync_error(torch.cuda.current_stream().cuda_stream) == 0
