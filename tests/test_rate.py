"""Rate control without a GPU: the NumPy restatement of the rate kernels (the yardstick of
tests/test_gpu_rate.py) against the reference's own masks, the operator and C-ABI surface, the
kbps -> bits budget, and the argument conflicts of encode.

The restatement is the frame count of the RVQ kernels (include/vrvq.h "Rate control") in
np.float32 products -- IEEE, so the same two roundings -- with Python-int totals and a plain
bisection over the float32 bit patterns. Everything compared with it is an integer or an fp32
bit pattern: every comparison is equality."""
import ctypes

import numpy as np
import pytest
import torch

import vrvq_amd
from conftest import load_golden
from vrvq_amd import _lib, codec, ops, utils


# ------------------------------------------------------------------ the NumPy restatement
def frame_counts(imp, level, nq):
    """n(imp, level) = s >= 0 ? floor(min(s, nq - 1)) + 1 : 0, s = fl(fl(imp * level) * nq)."""
    imp = np.asarray(imp, np.float32)
    with np.errstate(all="ignore"):
        s = (imp * np.float32(level)) * np.float32(nq)
    n = np.zeros(imp.shape, np.int64)
    ok = s >= 0  # False for NaN
    n[ok] = np.floor(np.minimum(s[ok], np.float32(nq - 1))).astype(np.int64) + 1
    return n


def total_bits(imp, level, nq, bits):
    """Bits of all of imp at one level, a Python int."""
    cum = np.concatenate([[0], np.cumsum(np.asarray(bits, np.int64))])
    return int(cum[frame_counts(imp, level, nq)].sum())


def solve_level(imp, nq, bits, budget, lo, hi):
    """(level, total, status): the largest float32 level in [lo, hi] with total <= budget."""
    lo, hi = np.float32(lo), np.float32(hi)
    t_lo = total_bits(imp, lo, nq, bits)
    if t_lo > budget:
        return lo, t_lo, 1
    t_hi = total_bits(imp, hi, nq, bits)
    if t_hi <= budget:
        return hi, t_hi, 2
    a, b, tot = int(lo.view(np.uint32)), int(hi.view(np.uint32)), t_lo
    while b - a > 1:
        m = a + (b - a) // 2
        t = total_bits(imp, np.uint32(m).view(np.float32), nq, bits)
        if t <= budget:
            a, tot = m, t
        else:
            b = m
    return np.uint32(a).view(np.float32), tot, 0


# ------------------------------------------------------------------ restatement vs reference
def test_restatement_matches_reference_masks(manifest):
    """Counts = column sums of the reference's masks, bpf = its recorded bpf (golden_nq8: the
    level-1 forward mask, and the sweep masks of scripts/inference.py, whose imp * (level * nq)
    is the same number as (imp * level) * nq for nq = 8 and these power-of-two levels)."""
    g = load_golden("golden_nq8")
    nq = manifest["golden_nq8"]["kwargs"]["n_codebooks"]
    imp = g["imp_map"][:, 0]
    B, T = imp.shape
    np.testing.assert_array_equal(frame_counts(imp, 1.0, nq), g["mask_imp"].sum(1).astype(np.int64))
    for i, level in enumerate(manifest["levels"]):
        mask = g[f"sweep{i}_mask"]
        np.testing.assert_array_equal(frame_counts(imp, level, nq), mask.sum(1).astype(np.int64))
        tot = total_bits(imp, level, nq, [10] * nq)
        assert tot == int(mask.sum()) * 10
        # cal_bpf_from_mask: an exact fp32 sum divided by B * T in fp32
        assert np.float32(tot) / np.float32(B * T) == np.float32(g[f"sweep{i}_bpf"])


def test_restatement_solver_is_exact_and_bounded():
    rng = np.random.default_rng(5)
    imp = rng.random(200, dtype=np.float32)
    bits = [10] * 8
    lo, hi = 0.125, 6.0
    budget = (total_bits(imp, lo, 8, bits) + total_bits(imp, hi, 8, bits)) // 2
    lvl, tot, st = solve_level(imp, 8, bits, budget, lo, hi)
    assert st == 0 and tot == total_bits(imp, lvl, 8, bits) <= budget
    assert total_bits(imp, np.nextafter(lvl, np.float32(np.inf)), 8, bits) > budget
    assert solve_level(imp, 8, bits, 199 * 10, lo, hi)[2] == 1
    assert solve_level(imp, 8, bits, 200 * 80, lo, hi) == (np.float32(hi), total_bits(imp, hi, 8, bits), 2)


# ------------------------------------------------------------------ operators and fakes
def test_rate_ops_registered_with_fake_kernels():
    lib = ops.load_ops()
    for name in ("rate_curve", "rate_solve", "scale_imp_rows"):
        assert getattr(lib, name).default._schema.name == f"vrvq::{name}"
    m = torch.device("meta")
    imp = torch.empty(5, 1, 87, device=m)
    bits = torch.empty(8, dtype=torch.int32, device=m)
    tot = lib.rate_curve(imp, torch.empty(4, device=m), bits)
    assert tot.shape == (5, 4) and tot.dtype == torch.int64
    lv, tt, st = lib.rate_solve(imp, bits, torch.empty(4, dtype=torch.int32, device=m),
                                torch.empty(3, dtype=torch.int64, device=m), 0.125, 6.0)
    assert lv.shape == tt.shape == st.shape == (3,)
    assert (lv.dtype, tt.dtype, st.dtype) == (torch.float32, torch.int64, torch.int32)
    out = lib.scale_imp_rows(imp, torch.empty(5, device=m))
    assert out.shape == imp.shape and out.dtype == torch.float32


def test_rate_ops_reject_cpu_tensors():
    ops.load_ops()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.scale_imp_rows(torch.ones(2, 4), torch.ones(2))
    with pytest.raises(RuntimeError, match="GPU only"):
        utils.rate_curve(torch.ones(2, 1, 4), [1.0], 8)


# ------------------------------------------------------------------ budget
def test_kbps_to_budget():
    # 44.1 kHz / hop 512: floor(86.13) = 86 frames per second
    assert utils.kbps_to_budget(6, 87, 44100, 512) == 6069        # 6000 / 86 * 87 = 6069.77
    assert utils.kbps_to_budget(0.86, 1, 44100, 512) == 10        # 860 / 86 = 10
    assert utils.kbps_to_budget(0.85, 1, 44100, 512) == 9         # 9.88
    assert utils.kbps_to_budget(1.5, 100, 24000, 320) == 2000     # 1500 / 75 * 100
    assert utils.kbps_to_budget(8, 3 * 87, 44100, 512) == 24279   # 8000 / 86 * 261 = 24279.07
    assert utils.kbps_to_budget(0, 87, 44100, 512) == 0
    assert isinstance(utils.kbps_to_budget(6.5, 87, 44100, 512), int)


# ------------------------------------------------------------------ argument conflicts
SMALL = dict(encoder_dim=8, decoder_dim=32, n_codebooks=2)


def test_encode_argument_conflicts_raise_before_any_kernel():
    """All on CPU models: a ValueError, not the kernels' "GPU only" RuntimeError, shows the check
    comes first."""
    x = torch.zeros(2, 1, 1024)
    per_clip = torch.tensor([0.5, 1.0])
    vbr = vrvq_amd.DAC_VRVQ(level_min=0.5, level_max=2.0, **SMALL).eval()
    with pytest.raises(ValueError, match="not both"):
        vbr.encode(x, level=2.0, target_kbps=6.0)
    with pytest.raises(ValueError, match="not both"):
        vbr.encode(x, level=per_clip, target_kbps=6.0)
    with pytest.raises(ValueError, match="n_quantizers"):
        vbr.encode(x, n_quantizers=2, target_kbps=6.0)
    with pytest.raises(ValueError, match="n_quantizers"):
        vbr.encode(x, n_quantizers=2, level=per_clip)
    with pytest.raises(ValueError, match="not both"):
        vbr(x, 44100, None, 2.0, target_kbps=6.0)
    with pytest.raises(ValueError, match="n_quantizers"):
        vbr.quantizer(None, 2, None, per_clip)
    with pytest.raises(ValueError, match="not both"):
        vbr.quantizer(None, None, None, 1.0, target_kbps=6.0)
    vbr.train()
    with pytest.raises(ValueError, match="eval"):
        vbr.encode(x, target_kbps=6.0)
    with pytest.raises(ValueError, match="eval"):
        vbr.encode(x, level=per_clip)
    cbr = vrvq_amd.DAC_VRVQ(model_type="CBR", **SMALL).eval()
    with pytest.raises(ValueError, match="VBR"):
        cbr.encode(x, target_kbps=6.0)
    with pytest.raises(ValueError, match="VBR"):
        cbr.encode(x, level=per_clip)
    with pytest.raises(ValueError, match="VBR"):
        codec.compress(cbr, torch.zeros(1, 1, 4096), target_kbps=6.0)
    with pytest.raises(ValueError, match="not both"):
        codec.compress(vbr, torch.zeros(1, 1, 4096), level=2.0, target_kbps=6.0)
    # today's calls are untouched: they reach the kernels, which refuse CPU tensors
    vbr.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        vbr.encode(x, None, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        cbr.encode(x, level=3)


# ------------------------------------------------------------------ C-ABI argument checks
def test_capi_argument_errors():
    lib = _lib.load()
    assert lib.vrvq_version() >= 101
    p = ctypes.c_void_p(16)  # non-null, never dereferenced: the checks return before a launch
    ERR = 10001

    def curve(imp=p, B=2, T=8, nq=8, bits=p, levels=p, L=3, out=p):
        return lib.vrvq_rate_curve(imp, B, T, nq, bits, levels, L, out, None)

    def solve(imp=p, B=2, T=8, nq=8, bits=p, off=p, G=2, budget=p, lo=0.125, hi=6.0, lv=p, tot=p,
              st=p):
        return lib.vrvq_rate_solve(imp, B, T, nq, bits, off, G, budget, lo, hi, lv, tot, st, None)

    for kw in (dict(imp=None), dict(bits=None), dict(levels=None), dict(out=None), dict(nq=0),
               dict(nq=33), dict(nq=-1), dict(B=0), dict(T=0), dict(L=0)):
        assert curve(**kw) == ERR, kw
    for kw in (dict(imp=None), dict(bits=None), dict(off=None), dict(budget=None), dict(lv=None),
               dict(tot=None), dict(st=None), dict(nq=0), dict(nq=33), dict(B=0), dict(T=0),
               dict(G=0), dict(lo=2.0, hi=1.0), dict(lo=0.0), dict(lo=-1.0),
               dict(lo=float("nan")), dict(hi=float("nan")), dict(hi=float("inf"))):
        assert solve(**kw) == ERR, kw
    assert lib.vrvq_scale_imp_rows(None, 2, 8, p, p, None) == ERR
    assert lib.vrvq_scale_imp_rows(p, 2, 8, None, p, None) == ERR
    assert lib.vrvq_scale_imp_rows(p, 2, 8, p, None, None) == ERR
    assert lib.vrvq_scale_imp_rows(p, 0, 8, p, p, None) == ERR
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.call("vrvq_rate_solve", None, 1, 1, 8, None, None, 1, None, 1.0, 2.0, None, None,
                  None, None)
