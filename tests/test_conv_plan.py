"""Which kernel a conv shape runs, answered on the host (include/vrvq.h vrvq_conv_plan) and
pinned by tests/golden/conv_plan_parent.json: what vrvq_conv_last_launch reported, at the commit
before the planner existed, for a grid of shapes launched through the C-ABI -- every conv of
conf/base.yml / base_24kbps.yml at 1 s (the T <= 96 layers at four batch sizes), the
PROJ_TILE_CASES of test_gpu_rvq_part.py and the edges of every tile rule. Each row: the call's
arguments, its status, `launch` = [BM, BN, KS, x3, S] (null: no MFMA tile ran, the record before
the call was still there afterwards) and `ws_need` = vrvq_conv1d_workspace's bytes.

The planner is csrc/conv_plan.h (plan_conv1d / plan_conv_transpose1d); vrvq_conv_plan also looks
the plan's kernel up in the launch tables of csrc/conv_k*.hip. A change of a tile rule shows here,
without a GPU, as the rows whose kernel it moves."""
import ctypes
import json
import os

import pytest

from vrvq_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("BM", "BN", "KS", "x3", "S")
ARGS = ("kind", "B", "cin", "tin", "cout", "k", "stride", "pad", "dil", "x3", "ws")


def rows():
    with open(os.path.join(HERE, "golden", "conv_plan_parent.json")) as f:
        return json.load(f)


def plan_of(r):
    """(status, plan dict or None) of a fixture row."""
    out = (ctypes.c_int * 7)()
    rc = _lib.load().vrvq_conv_plan(_lib.PLAN_KINDS[r["kind"]], *(r[a] for a in ARGS[1:]), out)
    if rc:
        return rc, None
    plan = _lib.conv_plan(*(r[a] for a in ARGS))
    assert [plan[n] for n in KEYS + ("path", "WM")] == list(out)
    return 0, plan


def tile(plan):
    """The plan as vrvq_conv_last_launch would report it (None: it records nothing)."""
    return [plan[k] for k in KEYS] if plan["path"] == 0 else None


def test_plan_matches_parent_record():
    """Every row: status, tile, x3 kind and S as the parent launched them; the workspace is
    non-zero exactly where the plan with a workspace splits K."""
    grid = rows()
    assert len(grid) > 300
    bad = []
    n = ctypes.c_longlong(0)
    for r in grid:
        status, plan = plan_of(r)
        got = tile(plan) if status == 0 else None
        if status != r["status"] or got != r["launch"]:
            bad.append((r, status, plan))
            continue
        if status == 0 and r["kind"] != "convt":
            _lib.call("vrvq_conv1d_workspace", r["B"], r["cin"], r["tin"], r["cout"], r["k"],
                      r["stride"] if r["kind"] == "conv" else 1, r["pad"], r["dil"], r["x3"],
                      ctypes.byref(n))
            assert n.value == r["ws_need"], r
            with_ws = _lib.conv_plan(*(dict(r, ws=1)[a] for a in ARGS))
            assert (n.value > 0) == (with_ws["S"] > 0), r
            if not r["ws"]:
                assert plan["S"] == 0, r
    assert not bad, f"{len(bad)} of {len(grid)} rows differ, first: {bad[:5]}"


def test_plan_covers_every_rule():
    """The fixture holds what its docstring says: each tile the dispatch can choose, the three
    chunk kinds, split and unsplit, the two non-MFMA paths and rejected shapes."""
    grid = rows()
    tiles = {tuple(r["launch"][:2]) for r in grid if r["launch"]}
    assert tiles >= {(32, 128), (64, 64), (64, 128), (64, 256), (96, 128), (128, 32), (128, 64),
                     (128, 96), (128, 128), (192, 64), (192, 128)}
    assert {r["launch"][3] for r in grid if r["launch"]} == {0, 1, 2}
    assert {r["launch"][4] for r in grid if r["launch"]} >= {0, 2, 3, 4}
    assert {r["launch"][2] for r in grid if r["launch"]} == {1, 2, 3, 4, 7, 8, 16}
    assert {r["status"] for r in grid} == {0, 10002}
    paths = {plan_of(r)[1]["path"] for r in grid if r["status"] == 0 and r["launch"] is None}
    assert paths == {1, 2}


def test_plan_reproduces_proj_tile_cases():
    from test_gpu_rvq_part import PROJ_TILE_CASES
    assert len(PROJ_TILE_CASES) == 10
    for _name, cin, B, T, mode, launch in PROJ_TILE_CASES:
        plan = _lib.conv_plan("proj", B, cin, T, 1024, 3, 1, 1, 1, mode != "fp32", mode != "nows")
        assert tuple(plan[k] for k in KEYS) == launch, _name
        # the plain conv of the same shape takes the same tile (the test launches both)
        conv = _lib.conv_plan("conv", B, cin, T, 1024, 3, 1, 1, 1, mode != "fp32", mode != "nows")
        assert conv == plan, _name


def test_plan_rejects_bad_calls():
    lib = _lib.load()
    out = (ctypes.c_int * 7)()
    assert lib.vrvq_conv_plan(0, 1, 64, 100, 64, 3, 1, 1, 1, 1, 1, None) == 10001
    assert lib.vrvq_conv_plan(3, 1, 64, 100, 64, 3, 1, 1, 1, 1, 1, out) == 10001
    assert lib.vrvq_conv_plan(0, 0, 64, 100, 64, 3, 1, 1, 1, 1, 1, out) == 10001
    assert lib.vrvq_conv_plan(0, 1, 64, 2, 64, 7, 1, 0, 1, 1, 1, out) == 10001      # tout <= 0
    assert lib.vrvq_conv_plan(1, 1, 64, 100, 512, 3, 1, 1, 1, 1, 1, out) == 10002   # proj: 1024 only
    assert lib.vrvq_conv_plan(2, 1, 64, 100, 32, 7, 4, 2, 1, 1, 0, out) == 10001    # k != 2 stride
    assert lib.vrvq_conv_plan(0, 1, 64, 100, 64, 5, 1, 2, 1, 0, 0, out) == 10002    # no k5 tiles
    assert lib.vrvq_version() >= 104


# ------------------------------------------------------------------ on the GPU: plan == launch
def _smallest_per_plan(grid):
    """The fixture's 99 distinct records come from 27 (tile, chunk kind) pairs x 7 tap counts; a
    launch each would be 2.5 x the budget. Rows in order of their bytes, a row taken when it is
    the first (hence smallest) with its tile and chunk kind, its taps and chunk kind, its
    split-K part count, its entry point, the phase-split view, or its kernel off the MFMA tiles:
    45 launches. B <= 3 except the B = 48, T = 87 width cases."""
    def size(r):
        up = r["stride"] if r["kind"] == "convt" else 1
        return (r["B"] * (r["cin"] * r["tin"] + r["cout"] * r["tin"] * up) +
                r["cin"] * r["k"] * r["cout"])

    seen, picked = set(), []
    for r in sorted(grid, key=size):
        if r["status"] != 0 or (r["B"] > 3 and not (r["B"] == 48 and r["tin"] == 87)):
            continue
        rec = r["launch"]
        if rec:
            BM, BN, KS, x3, S = rec
            what = {("tile", BM, BN, x3), ("taps", KS, x3), ("S", S), ("entry", r["kind"], x3),
                    ("view", r["stride"] > 1 and x3 > 0)}
        else:
            what = {("off-tile", r["k"], r["cout"] == 1, r["cin"] == 1)}
        if what - seen:
            seen |= what
            picked.append(r)
    return picked


@pytest.mark.gpu
def test_launch_runs_the_plan():
    """The smallest shape of each kind of plan in the fixture (_smallest_per_plan), launched
    through the entry point its row names on throw-away buffers: status 0 and
    vrvq_conv_last_launch == the plan (a plan off the MFMA tiles leaves the record of the launch
    before it in place). Numerics are other tests' business."""
    import torch
    from vrvq_amd import ops
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def P(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def zeros(n, dtype=torch.float32):
        return torch.zeros(max(int(n), 1), dtype=dtype, device=dev)

    def x3_planes(cin, k, cout_pad):
        return zeros(ops.x3_size(cin, k, cout_pad), torch.int16)

    w3in = ops.rvq_pack_w_in(torch.zeros(8, 1024, 8, device=dev))
    sx, sw, sy = zeros(8 * 43), zeros(8 * 4 * 128), zeros(16 * 40)
    picked = _smallest_per_plan(rows())
    assert 40 <= len(picked) <= 48
    assert {(r["launch"][0], r["launch"][1], r["launch"][3]) for r in picked if r["launch"]} == \
        {(r["launch"][0], r["launch"][1], r["launch"][3]) for r in rows() if r["launch"]}
    for r in picked:
        B, cin, tin, cout, k, s, pad, dil = (r[n] for n in ARGS[1:9])
        plan = _lib.conv_plan(*(r[a] for a in ARGS))
        # the record to overwrite: an 8 -> 16 k4 conv on the 32 x 128 fp32-input tile
        assert lib.vrvq_conv1d(P(sx), 1, 8, 43, None, None, P(sw), None, 16, 128, 4, 1, 0, 1,
                               None, None, 0, P(sy), 40, None, None, None, None) == 0
        before = _lib.conv_last_launch()
        assert [before[n] for n in KEYS] == [32, 128, 4, 0, 0]
        if r["kind"] == "convt":
            cout_pad = ops.round_up(cout * s, 128 if 128 % s == 0 else 192)
            x, w, y = zeros(B * cin * tin), zeros(cin * 2 * cout_pad), \
                zeros(B * cout * ops.convt_out_len(tin, s, pad))
            w3 = x3_planes(cin, 2, cout_pad) if r["x3"] else None
            rc = lib.vrvq_conv_transpose1d_pad(P(x), B, cin, tin, None, None, P(w), P(w3), cout,
                                               cout_pad, s, pad, None, P(y), None, None, None,
                                               None)
        else:
            cout_pad = ops.round_up(cout, 128)
            tout = ops.conv_out_len(tin, k, s, pad, dil)
            x, w, y = zeros(B * cin * tin), zeros(cin * k * cout_pad), zeros(B * cout * tout)
            w3 = None
            if r["x3"]:
                w3 = x3_planes(cin * s, 2, cout_pad) if s > 1 else x3_planes(cin, k, cout_pad)
            ws = zeros(max(r["ws_need"], 256) // 4) if r["ws"] else None
            wsb = ws.numel() * 4 if r["ws"] else 0
            if r["kind"] == "proj":
                part = zeros(8 * B * tout * 64)
                rc = lib.vrvq_conv1d_proj(P(x), B, cin, tin, None, None, P(w), P(w3), cout,
                                          cout_pad, k, pad, dil, None, P(y), tout, P(w3in), 8,
                                          P(part), P(ws), wsb, None)
            else:
                rc = lib.vrvq_conv1d_ws(P(x), B, cin, tin, None, None, P(w), P(w3), cout,
                                        cout_pad, k, s, pad, dil, None, None, 0, P(y), tout,
                                        None, None, None, P(ws), wsb, None)
        assert rc == 0, r
        after = _lib.conv_last_launch()
        if plan["path"] == 0:
            assert after == {n: plan[n] for n in KEYS}, r
        else:
            assert after == before and r["launch"] is None, r
    torch.cuda.synchronize()
