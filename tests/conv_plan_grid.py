"""A wide grid of conv shapes through vrvq_conv_plan, summarised: tests/golden/conv_plan_grid.json
was written by `python tests/conv_plan_grid.py` at the commit before the planner became ordinary
host code (conv_plan.h), tests/test_conv_plan_grid.py recomputes it from the library under test.

Per group (kind, k, stride, pad, dil): the row count, the status histogram and a SHA-256 over the
rows' (status, out[0..6]) in iteration order (zeros for a row whose status is not 0: the query
leaves `out` alone). Over the whole grid: the sorted distinct (kind, view, BM, BN, KS, x3, S,
path, WM), view = stride > 1 and x3. No GPU is touched."""
import ctypes
import hashlib
import itertools
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run as a script
from vrvq_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_grid.json")

BATCH = (1, 32, 47, 48)
CIN = (1, 7, 8, 24, 64, 96, 200, 512, 1024)
TIN = (1, 32, 33, 87, 96, 97, 639, 640, 696, 4095, 4096, 5568)
COUT = (1, 8, 9, 32, 33, 64, 96, 128, 192, 256, 320, 384, 768, 1024, 1536)
# (k, stride, pad, dil)
CONV_STRIDE1 = ((1, 1, 0, 1), (3, 1, 1, 1), (7, 1, 3, 1), (7, 1, 9, 3), (7, 1, 27, 9),
                (7, 1, 30, 10), (2, 1, 0, 1), (4, 1, 0, 1), (5, 1, 2, 1), (8, 1, 0, 1),
                (16, 1, 0, 1))
CONV_STRIDED = ((4, 2, 1, 1), (4, 2, 0, 1), (8, 4, 2, 1), (8, 4, 0, 1), (16, 8, 4, 1),
                (16, 8, 0, 1), (16, 8, 8, 1), (6, 3, 2, 1), (4, 4, 0, 1))
CONVT_STRIDES = (2, 3, 4, 5, 6, 8)
KINDS = {"conv": 0, "proj": 1, "convt": 2}


def groups():
    """(kind, k, stride, pad, dil) and the group's (B, cin, tin, cout, x3, ws) rows, in order."""
    for k, s, pad, dil in CONV_STRIDE1 + CONV_STRIDED:
        yield ("conv", k, s, pad, dil), itertools.product(BATCH, CIN, TIN, COUT, (0, 1), (0, 1))
    for s in CONVT_STRIDES:
        for pad in ((s + 1) // 2, 0):
            yield ("convt", 2 * s, s, pad, 1), itertools.product(BATCH, CIN, TIN, COUT, (0, 1),
                                                                 (0,))
    yield ("proj", 3, 1, 1, 1), itertools.product(BATCH, CIN, TIN, (1024,), (0, 1), (0, 1))


def summary():
    lib = _lib.load()
    out = (ctypes.c_int * 7)()
    zeros = (0,) * 7
    result, keys = [], set()
    for (kind, k, s, pad, dil), rows in groups():
        sha, hist, n = hashlib.sha256(), {}, 0
        for B, cin, tin, cout, x3, ws in rows:
            rc = lib.vrvq_conv_plan(KINDS[kind], B, cin, tin, cout, k, s, pad, dil, x3, ws, out)
            plan = tuple(out) if rc == 0 else zeros
            sha.update(struct.pack("<8i", rc, *plan))
            hist[str(rc)] = hist.get(str(rc), 0) + 1
            n += 1
            if rc == 0:
                keys.add((kind, int(s > 1 and x3 == 1)) + plan)
        result.append({"group": [kind, k, s, pad, dil], "rows": n, "status": hist,
                       "sha256": sha.hexdigest()})
    return {"groups": result, "keys": [list(t) for t in sorted(keys)]}


if __name__ == "__main__":
    got = summary()
    with open(GOLDEN, "w") as f:
        f.write("{\n \"groups\": [\n")
        f.write(",\n".join("  " + json.dumps(g, sort_keys=True) for g in got["groups"]))
        f.write("\n ],\n \"keys\": [\n")
        f.write(",\n".join("  " + json.dumps(k) for k in got["keys"]))
        f.write("\n ]\n}\n")
    total = {}
    for g in got["groups"]:
        for rc, c in g["status"].items():
            total[rc] = total.get(rc, 0) + c
    print("rows", sum(g["rows"] for g in got["groups"]), "status", total, "keys", len(got["keys"]))
