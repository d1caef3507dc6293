"""The spectral distance's gradient without a GPU: the NumPy float64 reference
(tests/spectral_grad_ref.py, the judge of tests/test_gpu_spectral_grad.py) against torch autograd
of vrvq_amd.losses on float64 tensors, the margins of the fixed rows the GPU test judges per
element, the operator and C-ABI surface, and the fused=True losses' argument errors and
defaults."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import spectral_grad_ref as G
import spectral_ref as S
import vrvq_amd
from vrvq_amd import _lib, losses, ops, trainer, utils


def module_of(scales, fused=False):
    """The losses.py module of a list of (window, n_mels) scales, all mel or all linear."""
    windows, mels = [w for w, _ in scales], [m for _, m in scales]
    if mels[0]:
        return losses.MelSpectrogramLoss(n_mels=mels, window_lengths=windows, fused=fused,
                                         **G.scale_kw(1))
    return losses.MultiScaleSTFTLoss(window_lengths=windows, fused=fused, **G.scale_kw(0))


def autograd64(est, ref, scales):
    """d loss / d est of the losses.py composition on float64 CPU tensors, (B, T)."""
    x = torch.from_numpy(np.asarray(est, np.float64))[:, None, :].requires_grad_()
    y = torch.from_numpy(np.asarray(ref, np.float64))[:, None, :]
    module_of(scales)(x, y).backward()
    return x.grad[:, 0].numpy()


def reference(est, ref, scales, **kw):
    return G.gradient_rows(est, ref, windows=[w for w, _ in scales],
                           n_mels=[m for _, m in scales], **G.scale_kw(scales[0][1]), **kw)


# ------------------------------------------------------------------ reference vs autograd
@pytest.mark.parametrize("scales", [[s] for s in G.SCALES] + [G.MEL_SCALES, G.STFT_SCALES],
                         ids=lambda s: "+".join(f"{w}.{m}" for w, m in s))
def test_reference_equals_autograd_on_float64(scales):
    """Per row within 1e-10 of max |grad|. losses.py means over the batch, so one row at a time
    (its gradient is then the row's own) and a batch of two (each row gets half)."""
    T = max(4099 if len(scales) > 1 else 0, scales[0][0] // 2 + 1, 1500)
    for n in sorted({T, 4099}):
        rows = [G.noise_rows(seed, n) for seed in (2, 3)]
        est, ref = np.stack([e for e, _ in rows]), np.stack([r for _, r in rows])
        got = reference(est, ref, scales)
        for i in range(2):
            want = autograd64(est[i:i + 1], ref[i:i + 1], scales)[0]
            assert np.abs(got[i] - want).max() <= 1e-10 * np.abs(want).max(), (n, i)
        both = autograd64(est, ref, scales)
        got = reference(est, ref, scales, upstream=[0.5, 0.5])
        for i in range(2):
            assert np.abs(got[i] - both[i]).max() <= 1e-10 * np.abs(both[i]).max(), (n, i)


def test_reference_lengths_short_rows_and_minimum_length():
    e, r = G.noise_rows(2, 600)
    est, ref = np.stack([e, e, e]), np.stack([r, r, r])
    got = G.gradient_rows(est, ref, windows=[512, 64], lengths=[600, 257, 256],
                          upstream=[1.0, -2.0, 1.0])
    alone = G.gradient_rows(est[:1, :257], ref[:1, :257], windows=[512, 64])[0]
    assert np.array_equal(got[1, :257], -2.0 * alone) and not got[1, 257:].any()
    assert np.isnan(got[2]).all() and np.isfinite(got[:2]).all()
    want = autograd64(est[:1, :257], ref[:1, :257], [(512, 0), (64, 0)])[0]  # n = W/2 + 1
    assert np.abs(alone - want).max() <= 1e-10 * np.abs(want).max()


def test_reference_zero_cases():
    e, r = G.noise_rows(2, 1500)
    for w, m in G.SCALES:
        kw = dict(windows=[w], n_mels=[m], **G.scale_kw(m))
        if w // 2 < 1500:
            assert not G.gradient_rows(r[None], r[None], **kw).any()          # est == ref
            assert not G.gradient_rows(0 * r[None], r[None], **kw).any()      # clamp and |X| = 0


# ------------------------------------------------------------------ the fixed rows are decided
def test_fixed_rows_are_decided():
    """Every row the GPU test judges per element keeps every sign and clamp decision at least
    2^-16 (relative) away from its threshold in fp64, about 16x the forward's relative error on
    noise: a kernel inside the forward's bar takes the decisions the reference takes. All pairs
    of a row count (decided() leaves none out but those whose gradient is exactly 0)."""
    worst = {}
    for w, m in G.SCALES:
        for n in G.lengths_of(w):
            d = G.decided(*G.noise_rows(G.seed_of(w, m, n), n), (w, m), **G.scale_kw(m))
            worst[(w, m, n)] = d
    for name, scales in (("mel", G.MEL_SCALES), ("stft", G.STFT_SCALES)):
        for T, seeds in G.MODULE_SEEDS[name].items():
            for seed in seeds:
                worst[(name, T, seed)] = min(G.decided(*G.noise_rows(seed, T), sc,
                                                       **G.scale_kw(sc[1])) for sc in scales)
    low = {k: v for k, v in worst.items() if not v >= G.MARGIN}
    print(f"smallest margin {min(worst.values()):.3e} at {min(worst, key=worst.get)}")
    assert not low, low


def test_decided_sees_a_tie_and_the_clamp():
    e, r = G.noise_rows(2, 700)
    assert G.decided(e, r, (512, 0)) > 0
    assert G.decided(e, r, (512, 0), clamp_eps=float(S.spectrogram(e, 512)[7, 1])) == 0.0
    # a pair with equal magnitudes has no gradient and is left out: the margin is the others'
    assert G.decided(r, r, (512, 0)) == np.abs(S.spectrogram(r, 512) - 1e-5).min() / 1e-5


# ------------------------------------------------------------------ operator and C-ABI surface
def test_grad_op_registered_with_fake_kernel():
    lib = ops.load_ops()
    assert lib.spectral_distance_grad.default._schema.name == "vrvq::spectral_distance_grad"
    m = torch.device("meta")
    e = torch.empty(0, device=m)
    gd = torch.empty(6, dtype=torch.float64, device=m)
    for est, ref in ((torch.empty(6, 5000, device=m), torch.empty(3, 5000, device=m)),
                     (torch.empty(6, 1, 5000, device=m), torch.empty(3, 1, 5000, device=m))):
        for lengths in (None, torch.empty(3, dtype=torch.int64, device=m)):
            grad = lib.spectral_distance_grad(est, ref, lengths, [2048, 512], [150, 0], [e, e],
                                              [e, e], [e, e], 1e-5, 2.0, 1.0, 1.0, gd)
            assert grad.shape == (6, 5000) and grad.dtype == torch.float32


def test_grad_rejects_cpu_tensors():
    ops.load_ops()
    est, ref = torch.ones(4, 3000), torch.ones(2, 3000)
    tabs, none = [torch.from_numpy(utils.spectral_tables(64))], [torch.empty(0)]
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.spectral_distance_grad(est, ref, None, [64], [0], tabs, none, none, 1e-5, 2.0, 1.0,
                                   1.0, torch.ones(4, dtype=torch.float64))
    x = torch.ones(2, 1, 3000, requires_grad=True)   # the autograd path launches the same forward
    with pytest.raises(RuntimeError, match="GPU only"):
        vrvq_amd.spectral_distance(x, torch.ones(2, 1, 3000), windows=(64,))


def test_grad_capi_argument_errors_and_workspace():
    lib = _lib.load()
    assert lib.vrvq_version() >= 109
    ERR = 10001
    p = ctypes.c_void_p(16)  # non-null, never dereferenced: the checks return before a launch
    n = ctypes.c_longlong(0)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    def ws_bytes(rows, samples, windows):
        rc = lib.vrvq_spectral_distance_grad_workspace(rows, samples, len(windows),
                                                       ints(*windows), ctypes.byref(n))
        return rc, n.value

    def floats(rows, samples, windows):
        total = 0
        for w in windows:
            F = _lib.spectral_tile_frames(w)
            tiles = -(-(1 + samples // (w // 4)) // F)
            total += rows * tiles * (w + (F - 1) * (w // 4))
        return total

    for rows, samples, windows in ((12, 441000, (2048, 512)),
                                   (3, 4099, (32, 64, 128, 256, 512, 1024, 2048))):
        want = -(-4 * floats(rows, samples, windows) // 8) * 8
        assert ws_bytes(rows, samples, windows) == (0, want)
    for rows, samples, windows in ((0, 4099, (512,)), (65536, 4099, (512,)), (2, 0, (512,)),
                                   (2, 2 ** 32 + 1, (512,)), (2, 4099, ()), (2, 4099, (32,) * 17),
                                   (2, 4099, (48,)), (2, 4099, (16,)), (2, 4099, (4096,))):
        assert ws_bytes(rows, samples, windows)[0] == ERR, (rows, samples, windows)
    assert lib.vrvq_spectral_distance_grad_workspace(2, 4099, 1, ints(512), None) == ERR

    need = ws_bytes(4, 4099, (2048, 512))[1]

    def call(est=p, ref=p, rows=4, ref_rows=2, samples=4099, lengths=None, windows=(2048, 512),
             n_mels=(150, 0), tables=(16, 16), bands=(16, None), weights=(16, None), eps=1e-5,
             grad_distance=p, grad_est=p, ws=p, ws_bytes_=None):
        return lib.vrvq_spectral_distance_grad(
            est, ref, rows, ref_rows, samples, lengths, len(windows), ints(*windows),
            ints(*n_mels), ptrs(*tables), ptrs(*bands), ptrs(*weights), eps, 2.0, 1.0, 1.0,
            grad_distance, grad_est, ws, need if ws_bytes_ is None else ws_bytes_, None)

    for bad in (dict(est=None), dict(ref=None), dict(grad_distance=None), dict(grad_est=None),
                dict(ws=None), dict(rows=3), dict(ref_rows=0), dict(eps=0.0), dict(samples=1024),
                dict(windows=(2048, 48)), dict(n_mels=(1026, 0)), dict(n_mels=(-1, 0)),
                dict(tables=(16, None)), dict(tables=(16, 12)), dict(bands=(None, None)),
                dict(weights=(None, None)), dict(ws_bytes_=need - 8), dict(ws=ctypes.c_void_p(20))):
        assert call(**bad) == ERR, bad


# ------------------------------------------------------------------ fused=True: errors, defaults
def test_fused_argument_errors_raise_before_any_launch():
    """On CPU tensors: a ValueError, not the kernels' "GPU only" RuntimeError."""
    x, y = torch.ones(2, 1, 3000), torch.ones(2, 1, 3000)
    for cls in (losses.MelSpectrogramLoss, losses.MultiScaleSTFTLoss):
        extra = dict(n_mels=[5]) if cls is losses.MelSpectrogramLoss else {}
        for w in (48, 16, 4096):
            with pytest.raises(ValueError, match="power of two"):
                cls(window_lengths=[w], fused=True, **extra)(x, y)
        ok = cls(window_lengths=[64], fused=True, **extra)
        for bx, by in ((x[:, 0], y[:, 0]), (x.repeat(1, 2, 1), y.repeat(1, 2, 1)),
                       (x[None], y[None]), (x, y[..., :2999]), (x, y[:1])):
            with pytest.raises(ValueError, match=r"\(B, 1, T\)|against"):
                ok(bx, by)
        with pytest.raises(ValueError, match="gradient"):
            ok(x, y.clone().requires_grad_())
        with pytest.raises(RuntimeError, match="GPU only"):   # valid arguments reach the kernels
            ok(x, y)
        with pytest.raises(RuntimeError, match="GPU only"):
            ok(x.clone().requires_grad_(), y)


def test_defaults_stay_the_torch_composition():
    assert losses.MelSpectrogramLoss().fused is False
    assert losses.MultiScaleSTFTLoss().fused is False
    assert inspect.signature(losses.MelSpectrogramLoss).parameters["fused"].default is False
    assert inspect.signature(losses.MultiScaleSTFTLoss).parameters["fused"].default is False
    assert inspect.signature(trainer.build_state).parameters["fused_losses"].default is False
    e, r = G.noise_rows(2, 2500)
    x = torch.from_numpy(e.astype(np.float64))[None, None].requires_grad_()
    y = torch.from_numpy(r.astype(np.float64))[None, None]
    for mod, kw in ((losses.MelSpectrogramLoss(),
                     dict(windows=(32, 64, 128, 256, 512, 1024, 2048),
                          n_mels=(5, 10, 20, 40, 80, 160, 320), pow=1.0, mag_weight=0.0)),
                    (losses.MultiScaleSTFTLoss(), dict(windows=(2048, 512)))):
        loss = mod(x, y)                      # CPU float64: the fused path could not run here
        want = S.distance_rows(e[None], r[None], **kw)["distance"][0]
        assert loss.dtype == torch.float64 and loss.requires_grad
        assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)


def test_build_state_passes_the_flag():
    gen = vrvq_amd.DAC_VRVQ(encoder_dim=8, decoder_dim=32, n_codebooks=2)
    cpu = torch.device("cpu")
    off = trainer.build_state(gen, cpu)
    assert off.mel_loss.fused is False and off.stft_loss.fused is False
    on = trainer.build_state(gen, cpu, fused_losses=True, mel_kwargs=dict(pow=2.0))
    assert on.mel_loss.fused is True and on.stft_loss.fused is True and on.mel_loss.pow == 2.0
