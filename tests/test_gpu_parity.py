"""HIP path (through the C-ABI) against the reference's golden fixtures, the CPU oracle and a
plain PyTorch fp32 reference of each conv kernel. Needs an MI355X.

Bar (north_star): integer codes and masks bit-exact; z_q / latents / waveform within 1e-4
relative (max-abs normalised)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vrvq_amd
import rvq_ref as R
from conftest import load_golden, rel_err
from oracle.vrvq_oracle import Oracle
from vrvq_amd import ops
from vrvq_amd.recipe import load_recipe, recipe_state_dict, shapes_of, synthetic_audio

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device("cuda:0")

_models = {}


def model_for(manifest, name):
    m = manifest[name]
    key = (tuple(sorted((k, str(v)) for k, v in m["kwargs"].items())), m["weight_seed"])
    if key not in _models:
        model = vrvq_amd.DAC_VRVQ(**m["kwargs"])
        load_recipe(model, m["weight_seed"])
        _models[key] = model.to(DEV).eval()
    return _models[key]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_native_library_loaded():
    from vrvq_amd import _lib
    _lib.load()
    maps = open("/proc/self/maps").read()
    assert "libvrvq_hip.so" in maps


# ------------------------------------------------------------------ whole model vs reference
@pytest.mark.parametrize("name", ["golden_nq8", "golden_nq28", "golden_nq32", "golden_cbr",
                                  "golden_cbr_n4"])
def test_model_forward_vs_reference(manifest, name):
    m = manifest[name]
    g = load_golden(name)
    model = model_for(manifest, name)
    with torch.no_grad():
        if m["kwargs"].get("model_type", "VBR") == "VBR":
            out = model(t(g["audio_in"]), 44100, m["n_quantizers"], 1)
        else:
            out = model(t(g["audio_in"]), 44100, m["n_quantizers"])
    np.testing.assert_array_equal(out["codes"].cpu().numpy(), g["codes"])
    assert rel_err(out["latents"].cpu().numpy(), g["latents"]) < TOL
    assert rel_err(out["z"].cpu().numpy(), g["z_q"]) < TOL
    assert rel_err(out["audio"].cpu().numpy(), g["audio_out"]) < TOL
    assert float(out["vq/commitment_loss"]) == pytest.approx(float(g["commitment_loss"]), rel=TOL)
    assert float(out["vq/codebook_loss"]) == pytest.approx(float(g["codebook_loss"]), rel=TOL)
    if "imp_map" in g:
        assert rel_err(out["imp_map"].cpu().numpy(), g["imp_map"]) < TOL
        np.testing.assert_array_equal(out["mask_imp"].cpu().numpy(), g["mask_imp"])


def test_x3_error_over_the_whole_chain(manifest):
    """The split-bf16 ("x3") convs over the ~60 chained layers of encoder + decoder: their end-
    to-end error against the reference's own outputs stays at the fp32-input MFMA path's level
    (z, latents and audio within 4x that path's error and within 2e-5), and codes agree."""
    g = load_golden("golden_nq8")
    name = "golden_nq8"
    m = manifest[name]
    errs = {}
    prev = ops.X3
    try:
        for x3 in (False, True):
            ops.X3 = x3
            model = vrvq_amd.DAC_VRVQ(**m["kwargs"])
            load_recipe(model, m["weight_seed"])
            model = model.to(DEV).eval()
            with torch.no_grad():
                out = model(t(g["audio_in"]), 44100, m["n_quantizers"], 1)
            np.testing.assert_array_equal(out["codes"].cpu().numpy(), g["codes"])
            errs[x3] = {k: rel_err(out[k].cpu().numpy(), g[r])
                        for k, r in (("z", "z_q"), ("latents", "latents"), ("audio", "audio_out"))}
    finally:
        ops.X3 = prev
    for k in errs[True]:
        assert errs[True][k] < 2e-5, (k, errs)
        assert errs[True][k] <= 4 * max(errs[False][k], 1e-6), (k, errs)


@pytest.mark.parametrize("name", ["golden_nq8", "golden_nq28"])
def test_encoder_and_decoder_units(manifest, name):
    g = load_golden(name)
    model = model_for(manifest, name)
    with torch.no_grad():
        x = model.preprocess(t(g["audio_in"]), 44100)
        z, feat = model.encoder(x, return_feat=True)
        assert rel_err(z.cpu().numpy(), g["z"]) < TOL
        assert rel_err(feat.cpu().numpy(), g["feat"]) < TOL
        y = model.decode(t(g["z_q"]))[..., :44100]
    assert rel_err(y.cpu().numpy(), g["audio_out"]) < TOL


@pytest.mark.parametrize("name", ["golden_nq8", "golden_nq28", "golden_nq32", "golden_rvq_stress_nq8",
                                  "golden_rvq_stress_nq32"])
def test_rvq_unit_vs_reference(manifest, name):
    """Quantizer fed the reference's own z / feat: isolates the RVQ kernels' numerics."""
    g = load_golden(name)
    model = model_for(manifest, name)
    with torch.no_grad():
        out = model.quantizer(t(g["z"]), None, t(g["feat"]), 1)
    np.testing.assert_array_equal(out["codes"].cpu().numpy(), g["codes"])
    np.testing.assert_array_equal(out["mask_imp"].cpu().numpy(), g["mask_imp"])
    assert rel_err(out["z_q"].cpu().numpy(), g["z_q"]) < TOL
    assert rel_err(out["latents"].cpu().numpy(), g["latents"]) < TOL
    assert rel_err(out["imp_map"].cpu().numpy(), g["imp_map"]) < TOL
    assert rel_err(out["z_q_is"].norm(dim=(2, 3)).cpu().numpy(), g["z_q_is_norm"]) < TOL
    if "z_q_is_s16" in g:
        assert rel_err(out["z_q_is"][:, :, ::16, :].cpu().numpy(), g["z_q_is_s16"]) < TOL


def test_level_sweep_vs_reference(manifest):
    """scripts/inference.py:88-112 on the GPU: masks bit-exact, recon within 1e-4, bpf/kbps."""
    g = load_golden("golden_nq8")
    model = model_for(manifest, "golden_nq8")
    res = vrvq_amd.level_sweep(model, t(g["audio_in"]), manifest["levels"])
    for li, r in enumerate(res):
        np.testing.assert_array_equal(r["mask"].cpu().numpy(), g[f"sweep{li}_mask"])
        assert rel_err(r["z_q"].norm(dim=1).cpu().numpy(), g[f"sweep{li}_zq_norm"]) < TOL
        assert rel_err(r["recon"][..., ::8].cpu().numpy(), g[f"sweep{li}_recon_s8"]) < TOL
        assert r["bpf"] == pytest.approx(float(g[f"sweep{li}_bpf"]), rel=1e-6)
        assert r["kbps"] == pytest.approx(float(g[f"sweep{li}_kbps"]), rel=1e-6)


def test_mask_kat(manifest):
    kat = manifest["mask_kat"]
    s = t(np.asarray(kat["s"], np.float32).reshape(1, 1, -1))
    for nq in (8, 28, 32):
        r = kat["results"][str(nq)]
        mask = vrvq_amd.generate_mask_hard(s, nq)
        np.testing.assert_array_equal(mask[0].cpu().numpy(), np.asarray(r["mask"], np.float32))
        assert vrvq_amd.cal_bpf_from_mask(mask, [10] * nq) == pytest.approx(r["bpf10"], rel=1e-7)
    ste = vrvq_amd.generate_mask_ste(s, 8, alpha=2.0)
    np.testing.assert_array_equal(ste[0].cpu().numpy(), np.asarray(kat["results"]["ste8_alpha2"], np.float32))


# ------------------------------------------------------------------ kernels vs torch fp32
def _snake_ref(x, alpha):
    a = alpha.reshape(1, -1, 1)
    return x + (a + 1e-9).reciprocal() * torch.sin(a * x).pow(2)


CONV_CASES = [
    # (B, cin, cout, T, k, stride, pad, dil, snake, residual, epi)
    (2, 64, 64, 1000, 7, 1, 3, 1, True, False, 0),
    (2, 64, 64, 1000, 7, 1, 9, 3, True, False, 0),
    (2, 96, 96, 777, 7, 1, 27, 9, True, False, 0),
    (3, 64, 64, 513, 1, 1, 0, 1, True, True, 0),
    (2, 1, 64, 700, 7, 1, 3, 1, False, False, 0),
    (2, 64, 128, 1024, 4, 2, 1, 1, True, False, 0),
    (2, 128, 256, 512, 8, 4, 2, 1, True, False, 0),
    (2, 256, 512, 256, 16, 8, 4, 1, True, False, 0),
    (2, 1024, 1024, 87, 3, 1, 1, 1, True, False, 0),
    (2, 96, 1, 1000, 7, 1, 3, 1, True, False, 1),
    (1, 96, 1, 2052, 7, 1, 3, 1, False, True, 1),    # Cout = 1 stream: tail tile + residual
    (2, 5, 1, 36, 3, 1, 1, 1, True, False, 0),       # stream k3: channel remainder, edges
    (2, 8, 1, 87, 3, 1, 1, 1, True, False, 2),
    (2, 32, 8, 87, 3, 1, 1, 1, True, False, 0),
    (1, 1024, 1536, 87, 7, 1, 3, 1, False, False, 0),
    (1, 768, 768, 5, 7, 1, 3, 1, True, True, 0),
    (1, 16, 16, 1, 7, 1, 3, 1, True, False, 0),
    (1, 192, 192, 600, 7, 1, 9, 3, True, False, 0),
    (1, 192, 192, 300, 1, 1, 0, 1, True, True, 0),
    (1, 96, 96, 300, 1, 1, 0, 1, True, True, 0),
    (2, 768, 768, 100, 7, 1, 27, 9, True, False, 0),
    (2, 512, 512, 96, 7, 1, 3, 1, True, False, 0),
    (1, 96, 8, 500, 7, 1, 3, 1, True, True, 2),
    (1, 384, 384, 5000, 1, 1, 0, 1, True, True, 0),
    (2, 768, 768, 696, 1, 1, 0, 1, True, True, 0),
    (1, 384, 384, 700, 1, 1, 0, 1, True, True, 0),
    (2, 512, 512, 696, 1, 1, 0, 1, True, True, 0),
    (2, 768, 768, 696, 7, 1, 27, 9, True, False, 0),
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv1d_vs_torch(case):
    B, cin, cout, T, k, s, p, d, use_snake, use_res, epi = case
    gen = torch.Generator(device="cpu").manual_seed(hash(case) & 0xFFFF)
    x = (torch.rand(B, cin, T, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(cout, cin, k, generator=gen) / np.sqrt(cin * k)).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(cin, generator=gen) * 1.5 + 0.5).to(DEV)
    tout = (T + 2 * p - d * (k - 1) - 1) // s + 1
    res = (torch.randn(B, cout, tout, generator=gen)).to(DEV) if use_res else None
    xin = _snake_ref(x, alpha) if use_snake else x
    ref = F.conv1d(xin.double(), w.double(), b.double(), stride=s, padding=p, dilation=d)
    if use_res:
        ref = res.double() + ref
    ref = [ref, torch.tanh(ref), torch.sigmoid(ref)][epi]
    wp, cout_pad = ops.pack_conv1d_weight(w)
    y = ops.conv1d(x, wp, cout, cout_pad, k, s, p, d, bias=b,
                   alpha=alpha if use_snake else None,
                   inv_alpha=ops.snake_inv_alpha(alpha) if use_snake else None,
                   residual=res, epilogue=epi)
    assert y.shape == ref.shape
    assert rel_err(y.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    # producer-side Snake of the next layer: bit-identical to snake applied to the stored y
    a_next = (torch.rand(cout, generator=gen) * 1.5 + 0.5).to(DEV)
    for want_raw in (True, False):
        y2, ys = ops.conv1d(x, wp, cout, cout_pad, k, s, p, d, bias=b,
                            alpha=alpha if use_snake else None,
                            inv_alpha=ops.snake_inv_alpha(alpha) if use_snake else None,
                            residual=res, epilogue=epi,
                            out_snake=(a_next, ops.snake_inv_alpha(a_next)), want_raw=want_raw)
        if want_raw:
            assert torch.equal(y2, y)
        else:
            assert y2 is None
        assert rel_err(ys.cpu().numpy(), _snake_ref(y, a_next).cpu().numpy()) < 1e-6


@pytest.mark.parametrize("mag", [1e3, 1e5, 1e7])
def test_snake_large_arguments(mag):
    """Snake (models/layers.py:26-32) for |alpha x| in [0.67, 1.33] * mag: the conv prologue
    (fp32 and x3 paths), the producer-side epilogue Snake and the Snake backward against fp64
    evaluated at the fp32 product u = fl(alpha * x) -- what the reference's fp32 torch.sin sees.
    Past 2^20 the kernels' Cody-Waite reduction hands over to the Payne-Hanek sinf."""
    gen = torch.Generator(device="cpu").manual_seed(int(mag) & 0xFFFF)
    C, T = 16, 300
    x = (torch.rand(2, C, T, generator=gen) * 0.5 + 0.5) * torch.sign(torch.rand(2, C, T, generator=gen) - 0.5)
    alpha = (torch.rand(C, generator=gen) * 0.1 + 0.95) * mag
    xd, ad = x.to(DEV), alpha.to(DEV)
    ia = ops.snake_inv_alpha(ad)
    u = (alpha.reshape(1, -1, 1) * x).double()          # fp32 product, then exact sin / cos
    inv = (alpha.double() + 1e-9).reciprocal().reshape(1, -1, 1)
    snk64 = x.double() + inv * torch.sin(u).pow(2)
    w = torch.eye(C).reshape(C, C, 1).to(DEV)
    wp, cp = ops.pack_conv1d_weight(w)
    for w3 in (None, ops.pack_x3_weight(wp, 1)):
        y = ops.conv1d(xd, wp, C, cp, 1, 1, 0, 1, alpha=ad, inv_alpha=ia, w_x3=w3)
        assert rel_err(y.cpu().numpy(), snk64.numpy()) < 1e-5
    # producer-side Snake of the next layer (epilogue) with the large alpha
    _, ys = ops.conv1d(xd, wp, C, cp, 1, 1, 0, 1, out_snake=(ad, ia), want_raw=False)
    assert rel_err(ys.cpu().numpy(), snk64.numpy()) < 1e-6
    # backward: dx = g (1 + inv 2 sin cos alpha), dalpha = sum g (-inv^2 sin^2 + inv 2 sin cos x)
    g = torch.randn(2, C, T, generator=gen)
    s2 = 2 * torch.sin(u) * torch.cos(u)
    dx64 = g.double() * (1 + inv * s2 * alpha.double().reshape(1, -1, 1))
    da64 = (g.double() * (-(inv * inv) * torch.sin(u).pow(2) + inv * s2 * x.double())).sum((0, 2))
    dx, da = ops.snake_backward(xd, ad, ia, g.to(DEV))
    assert rel_err(dx.cpu().numpy(), dx64.numpy()) < 1e-5
    assert rel_err(da.cpu().numpy(), da64.numpy()) < 1e-4


@pytest.mark.parametrize("k,p", [(7, 3), (3, 1)])
def test_cout1_stream_matches_small_kernel(k, p):
    """The Cout = 1 stream kernel (tin % 4 == 0) and the LDS-staged small-Cout kernel (other
    lengths) share the (channel, tap) fmaf order: outputs away from the right edge agree bit
    for bit between a length-1000 input and the same input extended to 1001."""
    gen = torch.Generator(device="cpu").manual_seed(11 + k)
    x = (torch.rand(2, 96, 1001, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(1, 96, k, generator=gen) / np.sqrt(96 * k)).to(DEV)
    b = (torch.randn(1, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(96, generator=gen) * 1.5 + 0.5).to(DEV)
    wp, cp = ops.pack_conv1d_weight(w)
    ia = ops.snake_inv_alpha(alpha)
    y0 = ops.conv1d(x[..., :1000].contiguous(), wp, 1, cp, k, 1, p, 1, bias=b, alpha=alpha,
                    inv_alpha=ia, epilogue=ops.EPI_TANH)
    y1 = ops.conv1d(x, wp, 1, cp, k, 1, p, 1, bias=b, alpha=alpha, inv_alpha=ia,
                    epilogue=ops.EPI_TANH)
    assert torch.equal(y0[..., :990], y1[..., :990])


@pytest.mark.parametrize("case", [(2, 1536, 768, 87, 8), (2, 768, 384, 100, 8), (2, 384, 192, 333, 4),
                                  (2, 192, 96, 1000, 2), (1, 16, 8, 1, 2), (1, 64, 32, 3, 8),
                                  (2, 64, 40, 77, 3), (1, 32, 16, 50, 6)])
def test_conv_transpose1d_vs_torch(case):
    B, cin, cout, T, s = case
    gen = torch.Generator(device="cpu").manual_seed(s * 1000 + T)
    x = (torch.rand(B, cin, T, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(cin, cout, 2 * s, generator=gen) / np.sqrt(cin * 2)).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(cin, generator=gen) * 1.5 + 0.5).to(DEV)
    ref = F.conv_transpose1d(_snake_ref(x, alpha).double(), w.double(), b.double(), stride=s,
                             padding=(s + 1) // 2)
    wp, cout_pad = ops.pack_convt1d_weight(w, s)
    y = ops.conv_transpose1d(x, wp, cout, cout_pad, s, bias=b, alpha=alpha,
                             inv_alpha=ops.snake_inv_alpha(alpha))
    assert y.shape == ref.shape
    assert rel_err(y.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    a_next = (torch.rand(cout, generator=gen) * 1.5 + 0.5).to(DEV)
    y2, ys = ops.conv_transpose1d(x, wp, cout, cout_pad, s, bias=b, alpha=alpha,
                                  inv_alpha=ops.snake_inv_alpha(alpha),
                                  out_snake=(a_next, ops.snake_inv_alpha(a_next)))
    assert torch.equal(y2, y)
    assert rel_err(ys.cpu().numpy(), _snake_ref(y, a_next).cpu().numpy()) < 1e-6


X3_CONV_CASES = [c for c in CONV_CASES if c[5] == 1 and c[4] in (1, 3, 7) and c[1] >= 8]


@pytest.mark.parametrize("case", X3_CONV_CASES)
def test_conv1d_x3_vs_torch(case):
    """The bf16x3 split MFMA path (csrc/conv_x3.h) against torch fp64, at the fp32 path's
    tolerance, and its error no larger than a small multiple of the fp32 MFMA path's."""
    B, cin, cout, T, k, s, p, d, use_snake, use_res, epi = case
    gen = torch.Generator(device="cpu").manual_seed(hash(case) & 0xFFFF)
    x = (torch.rand(B, cin, T, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(cout, cin, k, generator=gen) / np.sqrt(cin * k)).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(cin, generator=gen) * 1.5 + 0.5).to(DEV)
    tout = (T + 2 * p - d * (k - 1) - 1) // s + 1
    res = (torch.randn(B, cout, tout, generator=gen)).to(DEV) if use_res else None
    xin = _snake_ref(x, alpha) if use_snake else x
    ref = F.conv1d(xin.double(), w.double(), b.double(), stride=s, padding=p, dilation=d)
    if use_res:
        ref = res.double() + ref
    ref = [ref, torch.tanh(ref), torch.sigmoid(ref)][epi].cpu().numpy()
    wp, cout_pad = ops.pack_conv1d_weight(w)
    w3 = ops.pack_x3_weight(wp, k)
    kw = dict(bias=b, alpha=alpha if use_snake else None,
              inv_alpha=ops.snake_inv_alpha(alpha) if use_snake else None, residual=res,
              epilogue=epi)
    y32 = ops.conv1d(x, wp, cout, cout_pad, k, s, p, d, **kw)
    y3 = ops.conv1d(x, wp, cout, cout_pad, k, s, p, d, w_x3=w3, **kw)
    e32 = rel_err(y32.cpu().numpy(), ref)
    e3 = rel_err(y3.cpu().numpy(), ref)
    assert e3 < 1e-5
    assert e3 <= 4 * e32 + 2e-7, (e3, e32)


@pytest.mark.parametrize("case", [(1, 256, 256, 4500, 7, 1, 3, 1, True, True, 0),
                                  (2, 384, 384, 4100, 7, 1, 27, 9, True, False, 0),
                                  (1, 128, 320, 5000, 7, 1, 3, 1, False, True, 0),
                                  (1, 384, 384, 4500, 1, 1, 0, 1, False, True, 0),
                                  (2, 256, 512, 700, 1, 1, 0, 1, True, True, 0),
                                  (2, 96, 128, 600, 1, 1, 0, 1, False, True, 0)])
def test_conv1d_x3_long_rows_vs_torch(case):
    """x3 convs over long rows, as vrvq_conv_plan places them: the three k7 cases (rows of >= 640
    samples, >= 128 output channels, Cin % 16 == 0) run the pair-chunk 64 x 256 tiles of
    conv_x3.h (choose_tile takes them only for such Cin; plan_mfma runs a pair tile on plain
    chunks for any other), the k1 + skip GEMMs run 192 x 64, 128 x 64 and 128 x 128 tiles on
    plain 32-channel chunks; every case ends in a ragged last tile."""
    test_conv1d_x3_vs_torch(case)


@pytest.mark.parametrize("case", [(2, 64, 128, 1000, 2, 1, True), (2, 128, 256, 401, 4, 2, True),
                                  (2, 256, 512, 100, 8, 4, False), (2, 512, 1024, 696, 8, 4, False),
                                  (1, 64, 128, 513, 2, 0, True), (1, 8, 16, 37, 4, 2, True),
                                  (3, 24, 40, 77, 2, 1, False), (1, 16, 32, 31, 8, 0, True)])
def test_conv1d_strided_x3_vs_torch(case):
    """Strided convs (k = 2s) on the x3 loop through the phase-split view of x (vrvq_conv1d with
    w_x3 for stride > 1) against torch fp64, within a small multiple of the fp32 path's error."""
    B, cin, cout, T, s, p, use_snake = case
    gen = torch.Generator(device="cpu").manual_seed(s * 7919 + T + cin)
    x = (torch.rand(B, cin, T, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(cout, cin, 2 * s, generator=gen) / np.sqrt(cin * 2 * s)).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(cin, generator=gen) * 1.5 + 0.5).to(DEV)
    xin = _snake_ref(x, alpha) if use_snake else x
    ref = F.conv1d(xin.double(), w.double(), b.double(), stride=s, padding=p).cpu().numpy()
    wp, cout_pad = ops.pack_conv1d_weight(w)
    kw = dict(bias=b, alpha=alpha if use_snake else None,
              inv_alpha=ops.snake_inv_alpha(alpha) if use_snake else None)
    y32 = ops.conv1d(x, wp, cout, cout_pad, 2 * s, s, p, 1, **kw)
    y3 = ops.conv1d(x, wp, cout, cout_pad, 2 * s, s, p, 1,
                    w_x3=ops.pack_x3_strided_weight(w, s), **kw)
    assert y3.shape == ref.shape
    e32 = rel_err(y32.cpu().numpy(), ref)
    e3 = rel_err(y3.cpu().numpy(), ref)
    assert e3 < 1e-5
    assert e3 <= 4 * e32 + 2e-7, (e3, e32)
    a_next = (torch.rand(cout, generator=gen) * 1.5 + 0.5).to(DEV)
    y4, ys = ops.conv1d(x, wp, cout, cout_pad, 2 * s, s, p, 1,
                        w_x3=ops.pack_x3_strided_weight(w, s),
                        out_snake=(a_next, ops.snake_inv_alpha(a_next)), **kw)
    assert torch.equal(y4, y3)
    assert rel_err(ys.cpu().numpy(), _snake_ref(y3, a_next).cpu().numpy()) < 1e-6


# The split-K T <= 96 layers (conv_plan.h splitk_parts: 128 x 96 tiles, the K chunks cut into parts
# whose sums the workspace holds): (B, cin, cout, tin, k, stride, pad, dil, snake, residual, epi)
SPLITK_CASES = [(3, 512, 1024, 696, 16, 8, 4, 1, True, False, 0),   # EncoderBlock 512 -> 1024 s8
                (3, 1024, 1024, 87, 3, 1, 1, 1, True, False, 0),    # ImportanceSubnet in_block
                (3, 1024, 512, 87, 3, 1, 1, 1, True, False, 0),
                (3, 512, 128, 87, 3, 1, 1, 1, True, True, 0),
                (3, 1024, 1536, 87, 7, 1, 3, 1, False, False, 0),   # decoder's first conv
                (2, 1024, 1024, 40, 3, 1, 1, 1, True, False, 2)]


@pytest.mark.parametrize("case", SPLITK_CASES)
def test_conv1d_splitk_vs_torch_and_batch_invariant(case):
    """The deep-K T <= 96 layers run split-K through the torch op (vrvq_conv1d_ws): against
    torch fp64 at the x3 path's tolerance, within a small multiple of the unsplit x3 launch's
    error (vrvq_conv1d, no workspace), and every clip bit-identical to the clip run alone (the
    part count depends on the layer, not on the batch)."""
    from vrvq_amd import _lib
    B, cin, cout, T, k, s, p, d, use_snake, use_res, epi = case
    need = ctypes.c_longlong(0)
    _lib.call("vrvq_conv1d_workspace", B, cin, T, cout, k, s, p, d, 1, ctypes.byref(need))
    assert need.value > 0, "the case must take the split-K path"
    gen = torch.Generator(device="cpu").manual_seed(cin * 31 + cout + k)
    x = (torch.rand(B, cin, T, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(cout, cin, k, generator=gen) / np.sqrt(cin * k)).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(cin, generator=gen) * 1.5 + 0.5).to(DEV)
    tout = (T + 2 * p - d * (k - 1) - 1) // s + 1
    res = torch.randn(B, cout, tout, generator=gen).to(DEV) if use_res else None
    xin = _snake_ref(x, alpha) if use_snake else x
    ref = F.conv1d(xin.double(), w.double(), b.double(), stride=s, padding=p, dilation=d)
    if use_res:
        ref = res.double() + ref
    ref = [ref, torch.tanh(ref), torch.sigmoid(ref)][epi].cpu().numpy()
    wp, cout_pad = ops.pack_conv1d_weight(w)
    w3 = ops.pack_x3_weight(wp, k) if s == 1 else ops.pack_x3_strided_weight(w, s)
    inv = ops.snake_inv_alpha(alpha) if use_snake else None
    kw = dict(bias=b, alpha=alpha if use_snake else None, inv_alpha=inv, residual=res,
              epilogue=epi)
    y = ops.conv1d(x, wp, cout, cout_pad, k, s, p, d, w_x3=w3, **kw)
    e = rel_err(y.cpu().numpy(), ref)
    assert e < 1e-5, e
    # the unsplit x3 launch (C-ABI without a workspace)
    y1 = torch.empty_like(y)
    P = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None  # noqa: E731
    _lib.call("vrvq_conv1d", P(x), B, cin, T, P(alpha if use_snake else None), P(inv), P(wp),
              P(w3), cout, cout_pad, k, s, p, d, P(b), P(res), epi, P(y1), tout, None, None,
              None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    e1 = rel_err(y1.cpu().numpy(), ref)
    assert e <= 4 * e1 + 2e-7, (e, e1)
    for i in range(B):
        kwi = dict(kw, residual=res[i:i + 1].contiguous() if use_res else None)
        yi = ops.conv1d(x[i:i + 1].contiguous(), wp, cout, cout_pad, k, s, p, d, w_x3=w3, **kwi)
        assert torch.equal(yi[0], y[i]), i


@pytest.mark.parametrize("case", [(2, 1536, 768, 87, 8), (2, 768, 384, 100, 8),
                                  (2, 384, 192, 333, 4), (2, 192, 96, 1000, 2),
                                  (1, 16, 8, 1, 2), (2, 64, 40, 77, 3)])
def test_conv_transpose1d_x3_vs_torch(case):
    B, cin, cout, T, s = case
    gen = torch.Generator(device="cpu").manual_seed(s * 1000 + T + 1)
    x = (torch.rand(B, cin, T, generator=gen) - 0.5).to(DEV)
    w = (torch.randn(cin, cout, 2 * s, generator=gen) / np.sqrt(cin * 2)).to(DEV)
    b = (torch.randn(cout, generator=gen) * 0.1).to(DEV)
    alpha = (torch.rand(cin, generator=gen) * 1.5 + 0.5).to(DEV)
    ref = F.conv_transpose1d(_snake_ref(x, alpha).double(), w.double(), b.double(), stride=s,
                             padding=(s + 1) // 2).cpu().numpy()
    wp, cout_pad = ops.pack_convt1d_weight(w, s)
    w3 = ops.pack_x3_weight(wp, 2)
    kw = dict(bias=b, alpha=alpha, inv_alpha=ops.snake_inv_alpha(alpha))
    e32 = rel_err(ops.conv_transpose1d(x, wp, cout, cout_pad, s, **kw).cpu().numpy(), ref)
    e3 = rel_err(ops.conv_transpose1d(x, wp, cout, cout_pad, s, w_x3=w3, **kw).cpu().numpy(), ref)
    assert e3 < 1e-5
    assert e3 <= 4 * e32 + 2e-7, (e3, e32)


def test_conv_transpose1d_unsupported_stride_raises():
    """Strides whose phase rows cannot tile 128 or 192 rows (5, 7) are rejected, not computed
    wrong (the epilogue maps whole output channels per tile)."""
    x = torch.rand(1, 16, 20, device=DEV)
    w = torch.rand(16, 8, 10, device=DEV)
    wp, cout_pad = ops.pack_convt1d_weight(w, 5)
    with pytest.raises(RuntimeError, match="instantiated kernel set"):
        ops.conv_transpose1d(x, wp, 8, cout_pad, 5)


def test_weight_norm_and_codebook_prep_vs_torch():
    gen = torch.Generator(device="cpu").manual_seed(5)
    v = torch.randn(300, 64, 7, generator=gen).to(DEV)
    g = torch.rand(300, 1, 1, generator=gen).to(DEV) + 0.5
    w = ops.weight_norm(g, v)
    ref = v.double() * (g.double() / v.double().norm(dim=(1, 2), keepdim=True))
    assert rel_err(w.cpu().numpy(), ref.cpu().numpy()) < 1e-6
    cb = torch.randn(3, 1024, 8, generator=gen).to(DEV)
    cbn, c2 = ops.codebook_prep(cb)
    rn = F.normalize(cb.double(), dim=-1)
    assert rel_err(cbn.cpu().numpy(), rn.cpu().numpy()) < 1e-6
    assert rel_err(c2.cpu().numpy(), rn.pow(2).sum(-1).cpu().numpy()) < 1e-6


# ------------------------------------------------------------------ full-size parity
# BASELINE.json configs at their full batch on the GPU, each compared clip by clip with the CPU
# oracle run on that clip's own input (clips are independent through the whole path, so the
# oracle on a subset equals the oracle on the batch, restricted to that subset). Codes and
# masks bit-exact, z_q / audio / imp_map within 1e-4 (max-abs normalised).
_full = {}


def _full_run(manifest, name, B, nq=None, sel=(), seed=4321):
    key = (name, B, nq, seed)
    if key in _full:
        return _full[key]
    kw = dict(manifest[name]["kwargs"])
    if nq is not None:
        kw["n_codebooks"] = nq
    model = vrvq_amd.DAC_VRVQ(**kw)
    load_recipe(model, 0)
    model = model.to(DEV).eval()
    audio = synthetic_audio(B, 44100, seed=seed)
    with torch.no_grad():
        out = model(t(audio), 44100, None, 1)
        enc = model.encode(model.preprocess(t(audio), 44100), None, 1)
    torch.cuda.synchronize()
    o = Oracle(recipe_state_dict(shapes_of(model.state_dict()), 0), **kw)
    ref = o.forward(audio[list(sel)], None, 1.0)
    _full[key] = (model, audio, out, enc, o, ref)
    return _full[key]


def _check_clips(out, enc, ref, sel):
    sel = list(sel)
    codes = out["codes"][sel].cpu().numpy()
    bad = np.argwhere(codes != ref["codes"])
    assert bad.size == 0, f"codes differ at (clip, stage, frame) {bad[:8].tolist()}"
    np.testing.assert_array_equal(out["mask_imp"][sel].cpu().numpy(), ref["mask_imp"])
    assert rel_err(out["imp_map"][sel].cpu().numpy(), ref["imp_map"]) < TOL
    assert rel_err(out["latents"][sel].cpu().numpy(), ref["latents"]) < TOL
    assert rel_err(out["z"][sel].cpu().numpy(), ref["z_q"]) < TOL
    assert rel_err(out["audio"][sel].cpu().numpy(), ref["audio"]) < TOL
    zqis = enc["z_q_is"][sel].cpu().numpy()
    assert rel_err(zqis, ref["z_q_is"]) < TOL
    # batch-level invariants over every clip
    mask = out["mask_imp"]
    assert torch.all(mask[:, 0] == 1) and torch.all(mask[:, 1:] <= mask[:, :-1])
    assert torch.equal(vrvq_amd.masked_sum(enc["z_q_is"], enc["mask_imp"]), enc["z_q"])


CFG2_CLIPS = tuple(range(32))


def test_config2_full_batch_vs_oracle(manifest):
    """BASELINE config 2: conf/base.yml (8 cb VBR), B = 32 x 1 s, level 1: every clip of the
    batch vs the oracle (models/dac_vrvq.py:222-252)."""
    _model, _a, out, enc, _o, ref = _full_run(manifest, "golden_nq8", 32, sel=CFG2_CLIPS)
    assert out["codes"].shape == (32, 8, 87) and out["audio"].shape == (32, 1, 44100)
    _check_clips(out, enc, ref, CFG2_CLIPS)


@pytest.mark.parametrize("nq", [28, 32])
def test_config3_full_batch_vs_oracle(manifest, nq):
    """BASELINE config 3: conf/base_24kbps.yml (n_codebooks 28 as in the file, and the 32
    override), B = 64, whole model: 16 clips spread over the batch vs the oracle."""
    sel = tuple(range(0, 64, 4)) + (63,)
    _model, _a, out, enc, _o, ref = _full_run(manifest, "golden_nq28", 64, nq=nq, sel=sel, seed=77)
    assert out["codes"].shape == (64, nq, 87)
    _check_clips(out, enc, ref, sel)


def test_level_sweep_full_batch_vs_oracle(manifest):
    """scripts/inference.py:88-112 at B = 32 (BASELINE config 5's per-GPU shape x2): for every
    level, masks bit-exact and z_q within 1e-4 on every clip, recon of 8 clips vs the
    oracle decoder, bpf / kbps over the whole batch equal to the reference formula on the
    masks (models/utils.py:64-73) and, over the oracle clips, to the oracle's own bpf."""
    from oracle.vrvq_oracle import cal_bpf_from_mask as bpf_np, generate_mask_hard as mask_np
    from oracle.vrvq_oracle import masked_sum as msum_np
    model, audio, _out, _enc, o, ref = _full_run(manifest, "golden_nq8", 32, sel=CFG2_CLIPS)
    res = vrvq_amd.level_sweep(model, t(audio), manifest["levels"])
    sel = list(CFG2_CLIPS)
    nq = model.n_codebooks
    for r in res:
        lv = float(r["level"])
        s = (ref["imp_map"] * np.float32(lv * nq)).astype(np.float32)
        m_ref = mask_np(s, nq)
        mask = r["mask"].cpu().numpy()
        np.testing.assert_array_equal(mask[sel], m_ref)
        assert rel_err(r["z_q"][sel].cpu().numpy(), msum_np(ref["z_q_is"], m_ref)) < TOL
        pick = sel[::4]  # 8 clips spread over the batch
        y = o.decoder(msum_np(ref["z_q_is"][pick], m_ref[pick]))
        assert rel_err(r["recon"][pick].cpu().numpy(), y) < TOL
        assert r["bpf"] == pytest.approx(bpf_np(mask, [10] * nq), rel=1e-6)
        assert r["kbps"] == pytest.approx(r["bpf"] * 86 / 1000, rel=1e-12)
        sub = vrvq_amd.cal_bpf_from_mask(r["mask"][sel].contiguous(), [10] * nq)
        assert sub == pytest.approx(bpf_np(m_ref, [10] * nq), rel=1e-6)


@pytest.mark.parametrize("length", [1, 511, 512, 513, 3000])
def test_ragged_lengths_vs_oracle(manifest, length):
    model = model_for(manifest, "golden_nq8")
    audio = synthetic_audio(1, length, seed=length)
    with torch.no_grad():
        out = model(t(audio), 44100, None, 1)
    o = Oracle(recipe_state_dict(shapes_of(model.state_dict()), 0), **manifest["golden_nq8"]["kwargs"])
    ref = o.forward(audio, None, 1.0)
    np.testing.assert_array_equal(out["codes"].cpu().numpy(), ref["codes"])
    assert out["audio"].shape[-1] == length
    assert rel_err(out["audio"].cpu().numpy(), ref["audio"]) < TOL


def test_deterministic(manifest):
    model = model_for(manifest, "golden_nq8")
    audio = t(synthetic_audio(4, 44100, seed=9))
    with torch.no_grad():
        a = model(audio, 44100, None, 1)
        b = model(audio, 44100, None, 1)
    for k in ("audio", "z", "codes", "latents", "mask_imp"):
        assert torch.equal(a[k], b[k]), k


def test_batch_invariance_full_batch(manifest):
    """Every clip of the configs[1] batch (B = 32) against the same clip run in small batches
    (the oracle checks 8 of the 32 clips): every output bit-identical, so no clip position of
    the full batch is computed differently from the small-batch path the oracle pins. (Tile
    widths that change a layer's K order -- the 2-tap x3 GEMMs' 32-wide pair tile vs the
    96-wide one -- are fixed per layer, not chosen by batch: conv_plan.h tile_width.)"""
    model = model_for(manifest, "golden_nq8")
    audio = t(synthetic_audio(32, 44100, seed=2024))
    with torch.no_grad():
        full = model(audio, 44100, None, 1)
        for part in (range(0, 4), range(4, 13), range(13, 32)):
            idx = list(part)
            sub = model(audio[idx].contiguous(), 44100, None, 1)
            for k in ("codes", "mask_imp", "imp_map", "latents", "z", "audio"):
                a, b = full[k][idx], sub[k]
                assert torch.equal(a, b), (k, idx[0], rel_err(a.cpu().numpy(), b.cpu().numpy()))


def test_cbr_mode_of_vbr_model(manifest):
    model = model_for(manifest, "golden_nq8")
    audio = t(synthetic_audio(1, 44100, seed=3))
    with torch.no_grad():
        x = model.preprocess(audio, 44100)
        out = model.encode(x, n_quantizers=8)
        assert out["imp_map"] is None and torch.all(out["mask_imp"] == 1)
        with pytest.raises(RuntimeError):
            model.encode(x, n_quantizers=4)


# ------------------------------------------------------------------ RVQ operator
def _rvq_fp64_reference(z, st, imp, level):
    """Plain PyTorch fp64 restatement of the RVQ chain + gating (models/quantize.py:42-103,
    353-421; models/utils.py:55-61) on the kernels' stacked weights."""
    z = z.double().cpu()
    w_in_t, b_in, cb, w_out, b_out = (x.double().cpu() for x in
                                      (st.w_in_t, st.b_in, st.cb, st.w_out, st.b_out))
    nq = cb.shape[0]
    B, D, T = z.shape
    r = z.clone()
    codes, z_q_is = [], []
    for i in range(nq):
        ze = torch.einsum("dk,bdt->bkt", w_in_t[i], r) + b_in[i][None, :, None]
        e = F.normalize(ze, dim=1)
        cn = F.normalize(cb[i], dim=1)
        dist = (e * e).sum(1, keepdim=True) - 2 * torch.einsum("bkt,nk->bnt", e, cn) + \
            (cn * cn).sum(1)[None, :, None]
        idx = dist.argmin(1)
        zq = cb[i][idx].permute(0, 2, 1)
        q = torch.einsum("dk,bkt->bdt", w_out[i], zq) + b_out[i][None, :, None]
        r = r - q
        codes.append(idx)
        z_q_is.append(q)
    codes = torch.stack(codes, 1)
    z_q_is = torch.stack(z_q_is, 1)
    if imp is None:
        mask = torch.ones(B, nq, T, dtype=torch.float64)
    else:
        s = imp.double().cpu()[:, None, :] * level * nq
        mask = (s - torch.arange(nq, dtype=torch.float64)[None, :, None] >= 0).double()
    z_q = (z_q_is * mask[:, :, None, :]).sum(1)
    return codes, z_q_is, z_q, mask


def _random_rvq(nq, ncode, seed):
    """Unit-scale biases and codebooks, every 3-dim parameter (weight_g, weight_v) at 0.05: the
    folded in_proj rows have norm ~0.04, so z_e is the bias for every frame and each stage picks
    1 to 3 distinct codes (tests/test_rvq_inputs.py test_old_recipe_is_near_constant). Good for
    launch structure and bit-identity between paths, NOT for the argmin: the tests that judge the
    distance scan draw from tests/rvq_ref.py diverse_rvq_params instead."""
    gen = torch.Generator().manual_seed(seed)
    q = vrvq_amd.model.ResidualVectorQuantize(input_dim=1024, n_codebooks=nq, codebook_size=ncode,
                                              codebook_dim=8)
    with torch.no_grad():
        for p in q.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.05 if p.ndim == 3 else 1.0))
    return q.to(DEV).eval(), gen


@pytest.mark.parametrize("nq,ncode,B,T,vbr", [
    (8, 1024, 3, 87, True), (8, 1024, 2, 1, True), (8, 1024, 2, 13, True), (8, 1024, 1, 25, False),
    (1, 1024, 4, 87, False), (32, 1024, 2, 87, True), (4, 256, 3, 40, True), (4, 512, 2, 87, True),
    (4, 768, 2, 12, False), (28, 1024, 2, 70, True), (8, 1024, 5, 200, True),
    (9, 1024, 2, 87, True), (5, 1024, 3, 40, False), (1, 1024, 3, 50, True)])
def test_rvq_encode_vs_fp64(nq, ncode, B, T, vbr):
    """torch.ops.vrvq.rvq_encode against a torch fp64 reference: every codebook size variant
    (N/256 = 1..4), partial and exact frame ranges, nq = 1 .. 32, VBR and CBR; z_q_is also
    against the codes -> rows -> out_proj path (rvq_gather + rvq_expand)."""
    q, gen = _random_rvq(nq, ncode, 1000 * nq + T)
    st = q.stacked()
    z = (torch.randn(B, 1024, T, generator=gen) * 0.3).to(DEV)
    imp = torch.rand(B, T, generator=gen).to(DEV) if vbr else None
    level = 0.75
    codes, lat, loss, zqis, zq, mask = ops.rvq_encode(z, *st.codes_args(), imp=imp, level=level)
    torch.cuda.synchronize()
    rc, rzqis, rzq, rmask = _rvq_fp64_reference(z, st, imp, level)
    assert (codes.cpu() == rc).float().mean().item() == 1.0
    np.testing.assert_array_equal(mask.cpu().numpy(), rmask.numpy())
    assert rel_err(zqis.cpu().numpy(), rzqis.numpy()) < 1e-5
    assert rel_err(zq.cpu().numpy(), rzq.numpy()) < 1e-5
    zst, _ = ops.rvq_gather(codes, st.cb)
    zqis2, _, _ = ops.rvq_expand(zst, st.w_out, st.b_out)
    assert rel_err(zqis.cpu().numpy(), zqis2.cpu().numpy()) < 1e-5
    # latents are the z_e of each stage; the loss is mean_k (z_e - z_q)^2 (models/quantize.py:69-71)
    zrows = zst.permute(0, 1, 3, 2).reshape(B, nq * 8, T)
    ref_loss = (lat - zrows).pow(2).reshape(B, nq, 8, T).mean(2)
    assert rel_err(loss.cpu().numpy(), ref_loss.cpu().numpy()) < 1e-4
    # the masked sum of the op's own z_q_is, in stage order, is its z_q bit for bit
    assert torch.equal(vrvq_amd.masked_sum(zqis, mask), zq)


def load_rvq(params):
    """A ResidualVectorQuantize on the device holding rvq_ref.Params (stacked per-stage tensors)."""
    nq, N, d = params.cb.shape
    D = params.v_in.shape[1]
    q = vrvq_amd.model.ResidualVectorQuantize(input_dim=D, n_codebooks=nq, codebook_size=N,
                                              codebook_dim=d)
    with torch.no_grad():
        for i, s in enumerate(q.quantizers):
            s.in_proj.weight_g.copy_(params.g_in[i * d:(i + 1) * d].reshape(d, 1, 1))
            s.in_proj.weight_v.copy_(params.v_in[i * d:(i + 1) * d].reshape(d, D, 1))
            s.in_proj.bias.copy_(params.b_in[i])
            s.out_proj.weight_g.copy_(params.g_out[i * D:(i + 1) * D].reshape(D, 1, 1))
            s.out_proj.weight_v.copy_(params.v_out[i * D:(i + 1) * D].reshape(D, d, 1))
            s.out_proj.bias.copy_(params.b_out[i])
            s.codebook.weight.copy_(params.cb[i])
    return q.to(DEV).eval()


_NAMES = ("codes", "latents", "loss_pf", "z_q_is", "z_q", "mask")


def rvq_three_entries(z, st, imp, level):
    """The quantizer's three eval entry points on the same inputs: rvq_encode as three launches
    (path 1), rvq_encode as its projection launch + rvq_pt_kernel (path 2), and rvq_project's
    partials -> rvq_encode_part (the default encode's rvq_pt_kernel). Asserts all six outputs
    bit-equal and returns them."""
    from test_gpu_rvq_part import _part_call, _project
    from vrvq_amd import _lib
    outs = []
    # forget the code a timeout test may have left in this stream's word (only this read clears it)
    _lib.rvq_sync_error(torch.cuda.current_stream().cuda_stream)
    prev = _lib.rvq_path(0)
    try:
        for path in (1, 2):
            _lib.rvq_path(path)
            outs.append(ops.rvq_encode(z, *st.codes_args(), imp=imp, level=level))
            torch.cuda.synchronize()
    finally:
        _lib.rvq_path(prev)
    outs.append(_part_call(_project(z, st), z.shape[2], st, imp, level))
    torch.cuda.synchronize()
    assert _lib.rvq_sync_error(torch.cuda.current_stream().cuda_stream) == 0
    for o, entry in zip(outs[1:], ("fused", "part")):
        for name, x, y in zip(_NAMES, outs[0], o):
            assert torch.equal(x, y), (entry, name)
    return outs[0]


def check_rvq_vs_fp64(out, z, params, imp, level, label):
    """Codes under rvq_ref.check_codes (every decision judged on the fp64 chain teacher-forced
    on the GPU's codes), mask exact, z_q_is / z_q / latents within 1e-5 of that chain, and the
    masked sum of the op's own z_q_is its z_q bit for bit. Prints the figures."""
    codes, lat, _loss, zqis, zq, mask = out
    nq, B, T = codes.shape[1], codes.shape[0], codes.shape[2]
    res = R.check_codes(codes, z, params)
    ref = res["ref"]
    print(f"{label}: eps_d={res['eps_d']:.2e} margin={res['margin']:.2e} "
          f"worst={res['worst']:.2e} mismatch={res['share']:.4%} "
          f"min distinct={min(R.distinct_per_stage(codes))}")
    rmask = R.mask_fp64(imp, level, nq, B, T)
    np.testing.assert_array_equal(mask.cpu().numpy(), rmask.numpy())
    assert rel_err(zqis.cpu().numpy(), ref.z_q_is.numpy()) < 1e-5
    assert rel_err(zq.cpu().numpy(), (ref.z_q_is * rmask[:, :, None, :]).sum(1).numpy()) < 1e-5
    assert rel_err(lat.cpu().numpy(), ref.latents.numpy()) < 1e-5
    assert torch.equal(vrvq_amd.masked_sum(zqis, mask), zq)
    return res


@pytest.mark.parametrize("nq,ncode,B,T,vbr", R.DIVERSE_SHAPES)
def test_rvq_diverse_vs_fp64(nq, ncode, B, T, vbr):
    """The argmin on inputs that exercise it (tests/rvq_ref.py: 100+ distinct codes per stage,
    every 256-code quarter of the codebook): the three launches, the fused launch and the default
    rvq_pt_kernel agree bit for bit, and EVERY decision is within 8 eps_d of its stage's fp64
    minimum with <= 0.5 % differing from the fp64 argmin (check_codes)."""
    params, z, imp = R.diverse_case(nq, ncode, B, T, vbr)
    st = load_rvq(params).stacked()
    zd = z.to(DEV)
    impd = None if imp is None else imp.to(DEV)
    out = rvq_three_entries(zd, st, impd, 0.75)
    R.assert_diverse(out[0], ncode)
    check_rvq_vs_fp64(out, z, params, imp, 0.75, f"diverse {(nq, ncode, B, T)}")


TIE_CASES = [(p, nq, n) for p in ("half", "pair", "mirror")
             for nq, n in ((8, 1024), (4, 512), (4, 768), (4, 256)) if (p, n) != ("mirror", 768)]


@pytest.mark.parametrize("pattern,nq,ncode", TIE_CASES)
def test_rvq_exact_ties_take_lowest_index(pattern, nq, ncode):
    """Every codebook row duplicated at a second index (rvq_ref.tie_codebook), so every decision
    at every stage is an exact tie of two identical rows: all three entry points and rvq_nearest
    (from_latents) return the LOWER index of the pair -- README / DESIGN's lowest-index argmin --
    and the codes pass check_codes. Strict: it assumes identical rows get bit-identical distances
    (the same codebook_prep row, the same 8-term dot), whatever their position."""
    params, gen = R.diverse_rvq_params(nq, ncode, 900 + nq + ncode)
    params = params._replace(cb=R.tie_codebook(params.cb, pattern))
    z = R.diverse_z(2, 87, gen)
    st = load_rvq(params).stacked()
    out = rvq_three_entries(z.to(DEV), st, None, 1.0)
    codes = out[0].cpu()
    res = check_rvq_vs_fp64(out, z, params, None, 1.0, f"ties {pattern} {(nq, ncode)}")
    near = ops.rvq_nearest(out[1], st.cbn, st.c2, nq).cpu()
    R.judge(near, res["ref"].dist, res["margin"], 0.005)
    for name, c in (("chain", codes), ("nearest", near)):
        high = ~R.lower_twin(c, ncode, pattern)
        assert not bool(high.any()), (f"{name}: {int(high.sum())} of {c.numel()} decisions took "
                                      f"the higher twin, first at {high.nonzero()[0].tolist()}")


def _rvq_both_paths(nq, ncode, B, T, imp_on, zqis, seed, repeats=3, side_load=False):
    """ops.rvq_encode on channel-major z under vrvq_rvq_path(2) (projection + rvq_pt_kernel)
    against path 1 (project -> chain -> expand): bit-equal outputs on every repeat, no wait ran
    out, and exactly the rvq_pt_kernel launches the plan says (none where it plans chain +
    expand, e.g. under rvq_debug_capacity(0))."""
    from vrvq_amd import _lib
    q, gen = _random_rvq(nq, ncode, seed)
    st = q.stacked()
    z = (torch.randn(B, 1024, T, generator=gen) * 0.3).to(DEV)
    imp = torch.rand(B, T, generator=gen).to(DEV) if imp_on else None
    run = lambda: ops.rvq_encode(z, *st.codes_args(), imp=imp, level=0.8,  # noqa: E731
                                 want_z_q_is=zqis)
    prev = _lib.rvq_path(1)
    try:
        want = run()
        torch.cuda.synchronize()
        _lib.rvq_path(2)
        p = _lib.rvq_plan(B, T, nq, ncode)  # with the hooks set now (path 2, any capacity cap)
        got = []
        side = torch.cuda.Stream() if side_load else None
        a = torch.randn(2048, 2048, device=DEV) if side_load else None
        _lib.rvq_timing_read()  # forget earlier timed launches
        _lib.rvq_timing(True)   # counts the rvq_pt_kernel launches that actually ran
        for r in range(repeats):
            if side is not None:  # uneven load: a GEMM stream on part of the chip meanwhile
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(r + 1):
                        a = (a @ a) * (1.0 / 2048)
            got.append(run())
        torch.cuda.synchronize()
        _lib.rvq_timing(False)
        _ms, launched = _lib.rvq_timing_read()
        assert _lib.rvq_sync_error(torch.cuda.current_stream().cuda_stream) == 0
    finally:
        _lib.rvq_timing(False)
        _lib.rvq_path(prev)
    # the launches the plan says ran, at every T (an exact count: no silent fallback)
    assert launched == repeats * (p["launches"] if p["kind"] == _lib.RVQ_PLAN_PT else 0), launched
    names = ("codes", "latents", "loss_pf", "z_q_is", "z_q", "mask")
    for g in got:
        for name, x, y in zip(names, want, g):
            assert (x is None and y is None) or torch.equal(x, y), name
    return launched


@pytest.mark.parametrize("nq,ncode,B,T,imp_on,zqis", [
    (8, 1024, 32, 87, True, True),     # configs[1]: one launch of 32 clips
    (32, 1024, 64, 87, True, True),    # configs[2]: the launches of the plan's resident clips
    (28, 1024, 40, 87, True, True),    # a ragged batch
    (5, 512, 3, 40, True, True), (1, 1024, 4, 87, False, True), (9, 256, 2, 7, True, False),
    (2, 1024, 1, 1, True, True), (12, 768, 2, 96, True, True), (3, 1024, 5, 65, False, False),
    (8, 1024, 3, 97, True, True)])     # T > 96: the in-launch path too (two expansion windows)
def test_rvq_fused_bit_identical_to_three_launches(nq, ncode, B, T, imp_on, zqis):
    """rvq_encode on channel-major z as the projection launch + rvq_pt_kernel (chain parts that
    publish each stage -> the expansion workgroups, in-launch hand-offs) returns every output of
    the three launches bit for bit, on repeated calls (stale granules of the previous call never
    pass a wait), with one frame, T below / at / above an expansion window, odd nq, every
    codebook size and a ragged batch; no wait ran out."""
    _rvq_both_paths(nq, ncode, B, T, imp_on, zqis, 77 * nq + T + B)


def test_rvq_fused_capacity_zero_takes_chain_and_expansion():
    """With the resident-clip capacity forced to 0 (a clip too long for the grid), rvq_encode
    on channel-major z runs project -> chain -> expand under path 2 as well: no timed
    rvq_pt_kernel launch, and path 1's bits."""
    from vrvq_amd import _lib
    prev = _lib.rvq_debug_capacity(0)
    try:
        assert _rvq_both_paths(4, 256, 2, 40, True, True, 4 * 77 + 40 + 2) == 0
    finally:
        _lib.rvq_debug_capacity(prev)


def test_rvq_fused_under_uneven_load():
    """Projection + rvq_pt_kernel while GEMMs on another stream hold part of the chip
    (workgroups start late and unevenly): same bits as the three launches, no wait ran out."""
    _rvq_both_paths(8, 1024, 32, 87, True, True, 4242, repeats=4, side_load=True)


def test_rvq_fused_graph_replay():
    """Captured in a CUDA graph (the projection launch, the memset nodes of the sync block and
    the granules in the workspace, the rvq_pt_kernel launch): replays give the three launches'
    bits, also after eager calls on the same stream."""
    from vrvq_amd import _lib
    q, gen = _random_rvq(8, 1024, 99)
    st = q.stacked()
    z = (torch.randn(32, 1024, 87, generator=gen) * 0.3).to(DEV)
    imp = torch.rand(32, 87, generator=gen).to(DEV)
    prev = _lib.rvq_path(1)
    try:
        want = ops.rvq_encode(z, *st.codes_args(), imp=imp, level=1.0)
        _lib.rvq_path(2)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.rvq_encode(z, *st.codes_args(), imp=imp, level=1.0)  # warm-up: the flag block
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ops.rvq_encode(z, *st.codes_args(), imp=imp, level=1.0)
        for _ in range(3):
            g.replay()
            torch.cuda.synchronize()
            for x, y in zip(want, out):
                assert (x is None and y is None) or torch.equal(x, y)
            eager = ops.rvq_encode(z, *st.codes_args(), imp=imp, level=1.0)
            torch.cuda.synchronize()
            for x, y in zip(want, eager):
                assert (x is None and y is None) or torch.equal(x, y)
    finally:
        _lib.rvq_path(prev)


def test_rvq_big_batch_nq32_properties():
    """BASELINE config 3 shape (B=64, 32 codebooks) on random weights: fp64 codes agreement
    and the invariants at full size."""
    q, gen = _random_rvq(32, 1024, 5)
    st = q.stacked()
    z = (torch.randn(64, 1024, 87, generator=gen) * 0.3).to(DEV)
    imp = torch.rand(64, 87, generator=gen).to(DEV)
    codes, lat, loss, zqis, zq, mask = ops.rvq_encode(z, *st.codes_args(), imp=imp, level=1.0)
    rc, rzqis, rzq, rmask = _rvq_fp64_reference(z[:4], st, imp[:4], 1.0)
    assert torch.equal(codes[:4].cpu(), rc)
    assert rel_err(zqis[:4].cpu().numpy(), rzqis.numpy()) < 1e-5
    assert torch.all(mask[:, 1:] <= mask[:, :-1])
    assert torch.equal(vrvq_amd.masked_sum(zqis, mask), zq)


# ------------------------------------------------------------------ fused ResidualUnit
@pytest.mark.parametrize("C,T,dil,want_raw", [(64, 1000, 1, True), (64, 333, 9, False),
                                              (96, 777, 3, True), (128, 512, 9, True),
                                              (192, 600, 1, False), (192, 70, 3, True),
                                              (96, 5, 9, True), (256, 300, 3, True),
                                              (256, 64, 9, False)])
def test_residual_unit_fused_vs_two_launch(C, T, dil, want_raw):
    """vrvq_residual_unit (one launch, snake2(h) kept in LDS) is bit-identical to the
    two-launch form (k7 conv with producer-side snake2, then k1 conv + skip), and both match a
    torch fp64 ResidualUnit (models/layers.py:52-68)."""
    from vrvq_amd.layers import ResidualUnit, Snake1d
    gen = torch.Generator().manual_seed(C * 100 + T + dil)
    ru = ResidualUnit(C, dilation=dil)
    nxt = Snake1d(C)
    with torch.no_grad():
        for p in list(ru.parameters()) + list(nxt.parameters()):
            if p.ndim == 3 and p.shape[0] == 1:           # Snake alpha (1, C, 1)
                p.copy_(torch.rand(p.shape, generator=gen) * 1.5 + 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
    ru, nxt = ru.to(DEV), nxt.to(DEV)
    x = (torch.rand(2, C, T, generator=gen) - 0.5).to(DEV)
    a1, _ = ru.block[0].prepared()
    x_snk = _snake_ref(x, a1).contiguous()
    y_f, ys_f = ru.run(x, x_snk, nxt, want_raw=want_raw)
    y_2, ys_2 = ru.run_two_launch(x, x_snk, nxt, want_raw=want_raw)
    torch.cuda.synchronize()
    # Bit-identical whenever both forms run the k7 GEMM with the same K chunking (C <= 128, and
    # C = 192 at T > 96, where the two-launch k7 also uses a 192-row tile). For C = 256, and
    # C = 192 at T <= 96, the two-launch k7 runs 128-row tiles with 8-channel K chunks against
    # the fused kernel's 4: a different fp32 summation order, compared at 1e-6.
    # With the x3 path on, both forms run the k7 and k1 GEMMs on the split bf16 MFMA in the
    # same K order for C = 64 / 96 / 128 / 192 (bit-identical; C = 128 runs its phase 2 in two
    # K-halves) and C = 256 an fp32 fused kernel: same sums, another rounding, compared at 1e-6.
    if ops.X3:
        close = C not in (64, 96, 128, 192)
    else:
        close = C > 192 or (C == 192 and T <= 96)
    if close:
        assert rel_err(ys_f.cpu().numpy(), ys_2.cpu().numpy()) < 1e-6
    else:
        assert torch.equal(ys_f, ys_2)
        if want_raw:
            assert torch.equal(y_f, y_2)
    if not want_raw:
        assert y_f is None and y_2 is None
    # torch fp64 reference of the unit
    with torch.no_grad():
        w7 = ru.block[1].folded_weight().double()
        w1 = ru.block[3].folded_weight().double()
        h = F.conv1d(x_snk.double(), w7, ru.block[1].bias.double(), padding=3 * dil, dilation=dil)
        hs = _snake_ref(h, ru.block[2].alpha.reshape(-1).double())
        ref = x.double() + F.conv1d(hs, w1, ru.block[3].bias.double())
        ys_ref = _snake_ref(ref, nxt.alpha.reshape(-1).double())
    assert rel_err(ys_f.cpu().numpy(), ys_ref.cpu().numpy()) < 1e-5


# ------------------------------------------------------------------ codes -> latents -> audio
@pytest.mark.parametrize("name", ["golden_from_codes_cbr", "golden_from_codes_vbr"])
def test_from_codes_vs_reference(manifest, name):
    """ResidualVectorQuantize.from_codes (models/quantize.py:217-249) through vrvq_rvq_gather +
    vrvq_rvq_expand, then decode; VBR with the mask (scripts/inference.py:99-100 masked sum)."""
    m = manifest[name]
    g = load_golden(name)
    model = model_for(manifest, name)
    codes = t(g["codes"])
    with torch.no_grad():
        if m["vbr"]:
            z_q, z_p, codes_out, z_q_is = model.quantizer.from_codes(
                codes, return_z_q_is=True, mask_imp=t(g["mask"]))
        else:
            z_q, z_p, codes_out, z_q_is = model.quantizer.from_codes(codes, return_z_q_is=True)
        audio = model.decode(z_q)
    np.testing.assert_array_equal(z_p.cpu().numpy(), g["z_p"])   # bit-exact gather
    np.testing.assert_array_equal(codes_out.cpu().numpy(), g["codes"])
    assert rel_err(z_q_is.cpu().numpy(), g["z_q_is"]) < TOL
    assert rel_err(z_q.cpu().numpy(), g["z_q"]) < TOL
    assert rel_err(audio.cpu().numpy(), g["audio"]) < TOL
    # without z_q_is: same z_q, and the plain (unmasked) sum for CBR
    with torch.no_grad():
        out = model.quantizer.from_codes(codes) if not m["vbr"] else \
            model.quantizer.from_codes(codes, mask_imp=t(g["mask"]))
    assert len(out) == 3
    assert torch.equal(out[0], z_q)


def test_from_codes_prefix_and_errors(manifest):
    model = model_for(manifest, "golden_from_codes_cbr")
    g = load_golden("golden_from_codes_cbr")
    o = Oracle(recipe_state_dict(shapes_of(model.state_dict()), 0),
               **manifest["golden_from_codes_cbr"]["kwargs"])
    codes = g["codes"][:, :3].copy()                     # fewer codebooks than the model
    z_q, z_p, _ = model.quantizer.from_codes(t(codes))
    zq_o, zp_o, _ = o.from_codes(codes)
    np.testing.assert_array_equal(z_p.cpu().numpy(), zp_o)
    assert rel_err(z_q.cpu().numpy(), zq_o) < TOL
    bad = codes.copy()
    bad[0, 1, 5] = 1024                                  # == codebook_size
    with pytest.raises(IndexError):
        model.quantizer.from_codes(t(bad))
    bad[0, 1, 5] = -1
    with pytest.raises(IndexError):
        model.quantizer.from_codes(t(bad))
    too_many = np.zeros((1, model.quantizer.n_codebooks + 1, 4), np.int64)
    with pytest.raises(IndexError):
        model.quantizer.from_codes(t(too_many))


def test_encode_from_codes_roundtrip_full_batch(manifest):
    """Size-independent property at BASELINE batch 32: encode -> codes -> from_codes with the
    encode's mask reproduces the encode's z_q (z_q_i from raw rows vs the straight-through
    z_e + (z_q - z_e): equal up to fp32 rounding) and its z_q_is."""
    model = model_for(manifest, "golden_nq8")
    audio = t(synthetic_audio(32, 44100, seed=99))
    with torch.no_grad():
        enc = model.encode(model.preprocess(audio, 44100), None, 1.0)
        z_q, z_p, _, z_q_is = model.quantizer.from_codes(enc["codes"], return_z_q_is=True,
                                                         mask_imp=enc["mask_imp"])
    assert rel_err(z_q.cpu().numpy(), enc["z_q"].cpu().numpy()) < TOL
    assert rel_err(z_q_is.cpu().numpy(), enc["z_q_is"].cpu().numpy()) < TOL


# ------------------------------------------------------------------ variable-length code packing
@pytest.mark.parametrize("B,nq,T", [(1, 8, 1), (3, 8, 87), (300, 8, 87), (2, 32, 1000),
                                    (5, 28, 257)])
def test_pack_codes_vs_oracle(B, nq, T):
    """vrvq_pack_*  vs the numpy oracle: packed stream and counts bit-exact,
    unpack restores the codes where the mask is 1 and the mask itself. Covers B > 256 (clip
    scan carry), T > 256 (frame scan carry), empty and full frames."""
    from oracle.vrvq_oracle import generate_mask_hard, pack_codes as pack_np
    from vrvq_amd.codes_io import pack_codes, unpack_codes
    rng = np.random.default_rng(B * 1000 + T)
    codes = rng.integers(0, 1024, (B, nq, T)).astype(np.int64)
    codes[0, :, 0] = 1023
    s = (rng.random((B, 1, T)) * (nq + 2) - 1.0).astype(np.float32)
    s[0, 0, 0] = nq           # full frame
    if T > 1:
        s[0, 0, 1] = -0.5     # empty frame
    mask = generate_mask_hard(s, nq)
    packed, counts = pack_codes(t(codes), t(mask))
    want_p, want_c = pack_np(codes, mask)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_c)
    np.testing.assert_array_equal(packed.cpu().numpy().view(np.uint16), want_p)
    codes2, mask2 = unpack_codes(packed, counts, nq)
    np.testing.assert_array_equal(mask2.cpu().numpy(), mask)
    np.testing.assert_array_equal(codes2.cpu().numpy(), np.where(mask != 0, codes, 0))


def test_pack_codes_errors_and_empty():
    from vrvq_amd.codes_io import pack_codes, unpack_codes
    codes = torch.zeros((2, 4, 10), dtype=torch.int64, device=DEV)
    mask = torch.zeros((2, 4, 10), device=DEV)
    packed, counts = pack_codes(codes, mask)
    assert packed.numel() == 0 and int(counts.sum()) == 0
    c2, m2 = unpack_codes(packed, counts, 4)
    assert int(m2.sum()) == 0 and int(c2.abs().sum()) == 0
    bad = mask.clone(); bad[0, 2, 3] = 1.0         # a 1 after a 0: not prefix-shaped
    with pytest.raises(ValueError):
        pack_codes(codes, bad)
    ok = mask.clone(); ok[1, 0, 4] = 1.0
    big = codes.clone(); big[1, 0, 4] = 1024
    with pytest.raises(IndexError):
        pack_codes(big, ok)
    p, c = pack_codes(codes, ok)
    with pytest.raises(ValueError):
        unpack_codes(p, c, 0)                       # counts > n_codebooks


def test_pack_roundtrip_full_batch_and_file(manifest, tmp_path):
    """BASELINE batch 32: encode -> pack by mask_imp -> save/load -> unpack -> from_codes with
    the unpacked mask reproduces the encode's z_q; packed size = bpf * B*T / 10."""
    from vrvq_amd.codes_io import load_packed, pack_codes, save_packed, unpack_codes
    model = model_for(manifest, "golden_nq8")
    audio = t(synthetic_audio(32, 44100, seed=7))
    with torch.no_grad():
        enc = model.encode(model.preprocess(audio, 44100), None, 1.0)
    packed, counts = pack_codes(enc["codes"], enc["mask_imp"])
    bpf = vrvq_amd.cal_bpf_from_mask(enc["mask_imp"], [10] * 8)
    assert packed.numel() == pytest.approx(bpf * counts.numel() / 10, abs=0.5)
    path = save_packed(tmp_path / "clip", packed, counts, 8, sample_rate=44100)
    p2, c2, meta = load_packed(path, device=DEV)
    assert meta["n_codebooks"] == 8 and torch.equal(p2, packed) and torch.equal(c2, counts)
    codes, mask = unpack_codes(p2, c2, 8)
    assert torch.equal(mask, enc["mask_imp"])
    with torch.no_grad():
        z_q, _, _ = model.quantizer.from_codes(codes, mask_imp=mask)
    assert rel_err(z_q.cpu().numpy(), enc["z_q"].cpu().numpy()) < TOL


@pytest.mark.parametrize("tag", ["full", "part"])
def test_from_latents_vs_reference(manifest, tag):
    """ResidualVectorQuantize.from_latents (models/quantize.py:251-285) on the HIP path against
    the reference's own outputs: codes and raw rows bit-exact, z_q within 1e-4."""
    g = load_golden("golden_from_latents_cbr")
    model = model_for(manifest, "golden_from_latents_cbr")
    with torch.no_grad():
        z_q, z_p, codes = model.quantizer.from_latents(t(g[f"{tag}_latents"]))
    np.testing.assert_array_equal(codes.cpu().numpy(), g[f"{tag}_codes"])
    np.testing.assert_array_equal(z_p.cpu().numpy(), g[f"{tag}_z_p"])
    assert rel_err(z_q.cpu().numpy(), g[f"{tag}_z_q"]) < TOL
