"""The HIP resampler on the GPU: forward and adjoint per element against the float64 restatement
(tests/resample_ref.py, full K taps) at every ratio and edge length, batch independence, graph
capture, and the three callers -- compress / decompress at 48 kHz, MSD(2) / MSD(4).

Bounds. An output is an fp32 fma chain over ntaps products of taps that were rounded once to
fp32: to first order |y - y64| <= (ntaps + 1) 2^-24 sum_j |k_j| |x_j|; the bar is (ntaps + 3).
The adjoint's element is a chain (or, at the two edge samples, chains joined by a tree and two
adds) over the c kept-tap products that reach it: (c + 3) 2^-24 sum |k| |dy|, which holds for any
summation order of c terms."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import resample_ref as ref
import vrvq_amd
from conftest import rel_err
from vrvq_amd import _lib, ops

pytestmark = pytest.mark.gpu

TILE = _lib.RESAMPLE_TILE
# nine ratios between audio rates, and 24:1, whose tile window (511 * 24 + K = 13.5k samples) takes two of the
# kernel's 8192-sample LDS segments -- every other ratio here takes one
RATIOS = [(48000, 44100), (44100, 48000), (16000, 44100), (44100, 16000), (44100, 22050),
          (44100, 11025), (22050, 44100), (48000, 16000), (44100, 8000), (48000, 2000)]
IDS = [f"{o}-{n}" for o, n in RATIOS]
U = 2.0 ** -24


def _cases(old_sr, new_sr):
    """(L, n_out): the edge lengths at their default output length (the largest where that is
    0), and the lengths whose output count sits at the tile boundaries."""
    old, new, _sr, W, _K = ref.plan(old_sr, new_sr)
    out = []
    for L in sorted({1, 2, W - 1, W, W + 1, old - 1, old, old + 1} - {0, -1}):
        n = ref.out_length(L, old_sr, new_sr)
        out.append((L, n if n > 0 else ref.out_length_max(L, old_sr, new_sr)))
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        L = -(-n * old // new)
        L += 1 - L % 2  # odd: the three rows start at three different 4-byte phases of 16
        assert ref.out_length(L, old_sr, new_sr) >= n or ref.out_length_max(L, old_sr, new_sr) >= n
        out.append((L, n))
    return out


@lru_cache(maxsize=None)
def _data(old_sr, new_sr):
    """Per case: inputs (3 rows, 0.3 N(0, 1) + 0.05) and the float64 references, computed once."""
    g = np.random.default_rng(old_sr * 7 + new_sr)
    data = []
    for L, n in _cases(old_sr, new_sr):
        x = (0.3 * g.standard_normal((3, L)) + 0.05).astype(np.float32)
        dy = (0.3 * g.standard_normal((3, n)) + 0.05).astype(np.float32)
        d = dict(L=L, n=n, x=x, dy=dy,
                 y=ref.resample(x, old_sr, new_sr, output_length=n),
                 yabs=ref.resample(x, old_sr, new_sr, output_length=n, absolute=True),
                 dx=ref.adjoint(dy, L, old_sr, new_sr),
                 dxabs=ref.adjoint(dy, L, old_sr, new_sr, absolute=True),
                 cnt=ref.adjoint_counts(n, L, old_sr, new_sr))
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        data.append(d)
    return data


def _gpu(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared references stay read-only


def _table(old_sr, new_sr):
    plan = _lib.resample_plan(old_sr, new_sr)
    taps, first = _lib.resample_taps(old_sr, new_sr)
    return plan, _gpu(taps), _gpu(first)


@pytest.mark.parametrize("old_sr,new_sr", RATIOS, ids=IDS)
def test_forward_per_element(old_sr, new_sr):
    ntaps = _lib.resample_plan(old_sr, new_sr)["ntaps"]
    worst = 0.0
    for d in _data(old_sr, new_sr):
        x = _gpu(d["x"])
        y = vrvq_amd.resample(x, old_sr, new_sr, output_length=d["n"])
        assert y.shape == (3, d["n"]) and y.dtype == torch.float32
        bound = (ntaps + 3) * U * d["yabs"]
        err = np.abs(y.cpu().numpy().astype(np.float64) - d["y"])
        assert (bound > 0).all()
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"L={d['L']} n={d['n']}: error {ratio:.3f} of the bound"
        # a row alone is the row in the batch, bit for bit; a second call is the first
        for r in range(3):
            alone = vrvq_amd.resample(x[r:r + 1].clone(), old_sr, new_sr, output_length=d["n"])
            assert torch.equal(alone[0], y[r]), f"L={d['L']}: row {r} alone differs"
        assert torch.equal(vrvq_amd.resample(x, old_sr, new_sr, output_length=d["n"]), y)
        # the default length is the integer floor
        if ref.out_length(d["L"], old_sr, new_sr) > 0:
            y0 = vrvq_amd.resample(x, old_sr, new_sr)
            n0 = ref.out_length(d["L"], old_sr, new_sr)
            assert y0.shape[-1] == n0
            m = min(n0, d["n"])
            assert torch.equal(y0[:, :m], y[:, :m])
    print(f"{old_sr}->{new_sr}: worst forward error {worst:.3f} of (ntaps + 3) 2^-24 sum|k||x|")


@pytest.mark.parametrize("old_sr,new_sr", RATIOS, ids=IDS)
def test_adjoint_per_element(old_sr, new_sr):
    plan, taps, first = _table(old_sr, new_sr)
    worst = 0.0
    for d in _data(old_sr, new_sr):
        dy = _gpu(d["dy"])
        dx = ops.resample_adjoint(dy, taps, first, plan["old"], plan["W"], d["L"])
        assert dx.shape == (3, d["L"])
        bound = (d["cnt"][None, :] + 3) * U * d["dxabs"]
        err = np.abs(dx.cpu().numpy().astype(np.float64) - d["dx"])
        ok = err <= bound
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())
        worst = max(worst, ratio)
        assert ok.all(), f"L={d['L']} n={d['n']}: error {ratio:.3f} of the bound"
        for r in range(3):
            alone = ops.resample_adjoint(dy[r:r + 1].clone(), taps, first, plan["old"], plan["W"],
                                         d["L"])
            assert torch.equal(alone[0], dx[r]), f"L={d['L']}: row {r} alone differs"
        assert torch.equal(ops.resample_adjoint(dy, taps, first, plan["old"], plan["W"], d["L"]),
                           dx)
        # autograd through the public function returns that adjoint
        x = _gpu(d["x"]).requires_grad_(True)
        vrvq_amd.resample(x, old_sr, new_sr, output_length=d["n"]).backward(dy)
        assert torch.equal(x.grad, dx)
    print(f"{old_sr}->{new_sr}: worst adjoint error {worst:.3f} of (c + 3) 2^-24 sum|k||dy|")


def test_leading_dimensions_and_double_backward():
    x = _gpu(_data(44100, 22050)[-1]["x"]).reshape(3, 1, -1)
    y = vrvq_amd.resample(x, 44100, 22050)
    assert y.shape == (3, 1, x.shape[-1] // 2)
    assert torch.equal(y.reshape(3, -1), vrvq_amd.resample(x.reshape(3, -1), 44100, 22050))
    # the adjoint's gradient is the operation itself
    x = x.detach().requires_grad_(True)
    d = torch.ones_like(y, requires_grad=True)
    (gx,) = torch.autograd.grad(vrvq_amd.resample(x, 44100, 22050), x, d, create_graph=True)
    (gd,) = torch.autograd.grad(gx, d, x.detach())
    assert torch.equal(gd, y)


def test_graph_capture_replays_eager_bits():
    old_sr, new_sr = 48000, 44100
    d = _data(old_sr, new_sr)[-1]
    a0 = _gpu(d["x"])
    a1 = _gpu((d["x"][::-1] * 0.5).copy())
    eager0, eager1 = (vrvq_amd.resample(a, old_sr, new_sr) for a in (a0, a1))  # warms the table
    static = a0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vrvq_amd.resample(static, old_sr, new_sr)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = vrvq_amd.resample(static, old_sr, new_sr)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    static.copy_(a1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager1)


def test_unsupported_ratio_names_it():
    x = torch.zeros(1, 100, device="cuda")
    with pytest.raises(RuntimeError, match="44100:44101"):
        vrvq_amd.resample(x, 44100, 44101)
    with pytest.raises(ValueError, match="output_length"):
        vrvq_amd.resample(x, 48000, 44100, output_length=93)


# ------------------------------------------------------------------------------ codec
@lru_cache(maxsize=None)
def _codec():
    from oracle.torch_ref import TorchRef
    from test_codec import KW
    from vrvq_amd.recipe import load_recipe, recipe_state_dict, shapes_of
    model = vrvq_amd.DAC_VRVQ(**KW)
    load_recipe(model, 0)
    model = model.to("cuda:0").eval()
    return model, TorchRef(recipe_state_dict(shapes_of(model.state_dict()), 0), **KW)


def _signal48(n, seed):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 48000
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.05 * g.standard_normal((1, n))
    return torch.tensor(x, dtype=torch.float32)[None]


@pytest.mark.parametrize("seconds", [1.3, 0.7])
def test_codec_at_48k(seconds):
    from test_codec import SR, _ref_compress, _ref_decompress
    from vrvq_amd.codec import AudioSignal, loudness
    model, tr = _codec()
    audio = _signal48(int(seconds * 48000), 11)
    L = audio.shape[-1]
    x441 = vrvq_amd.resample(audio.cuda(), 48000, SR)
    assert x441.shape[-1] == SR * L // 48000
    dac = model.compress(AudioSignal(audio, 48000), win_duration=1.0, max_batch=2)
    assert int(dac.sample_rate) == 48000 and int(dac.original_length) == L
    assert abs(float(dac.input_db[0]) - float(loudness(x441, SR)[0])) < 1e-6
    same = model.compress(x441.cpu(), win_duration=1.0, max_batch=2)
    assert torch.equal(dac.codes, same.codes)
    ref_codes, _ = _ref_compress(tr, model, x441.cpu(), 1.0)
    np.testing.assert_array_equal(dac.codes.numpy(), ref_codes.numpy())
    # the tensor at 48 kHz with its rate named is the same call
    named = model.compress(audio, win_duration=1.0, max_batch=2, sample_rate=48000)
    assert torch.equal(named.codes, dac.codes) and int(named.sample_rate) == 48000

    sig = model.decompress(dac)
    assert sig.sample_rate == 48000 and sig.audio_data.shape == audio.shape
    full = _ref_decompress(tr, model, ref_codes, dac.chunk_length, not dac.padding, dac.input_db,
                           10 ** 9)                       # the whole decoded length
    want = vrvq_amd.resample(full.cuda(), SR, 48000)[..., :L]
    assert want.shape == audio.shape
    assert rel_err(sig.audio_data.cpu().numpy(), want.cpu().numpy()) < 1e-4


def test_codec_at_model_rate_is_unchanged():
    """A 44.1 kHz signal through the same calls: the bits of the path without a rate."""
    from test_codec import SR, _signal
    from vrvq_amd.codec import AudioSignal
    model, _tr = _codec()
    audio = _signal(int(1.3 * SR), 7)
    plain = model.compress(audio, win_duration=1.0, max_batch=2)
    rated = model.compress(AudioSignal(audio, SR), win_duration=1.0, max_batch=2)
    assert torch.equal(plain.codes, rated.codes)
    assert np.array_equal(np.asarray(plain.input_db), np.asarray(rated.input_db))
    assert int(rated.sample_rate) == SR and rated.original_length == plain.original_length
    a, b = model.decompress(plain), model.decompress(rated)
    assert a.sample_rate == b.sample_rate == SR
    assert torch.equal(a.audio_data, b.audio_data)


# ------------------------------------------------------------------------------ MSD
@pytest.mark.parametrize("rate", [2, 4])
def test_msd_rates(rate):
    from vrvq_amd.discriminator import MSD
    torch.manual_seed(rate)
    msd = MSD(rate).cuda()
    x = (0.3 * torch.randn(2, 1, 8192, device="cuda") + 0.05).requires_grad_(True)
    seen, grads = [], []

    def pre(_m, args):
        seen.append(args[0])
        args[0].register_hook(grads.append)   # the conv stack's input gradient, as it flows

    hook = msd.convs[0].register_forward_pre_hook(pre)
    fmap = msd(x)
    hook.remove()
    xr = vrvq_amd.resample(x.detach(), 44100, 44100 // rate)
    assert xr.shape == (2, 1, 8192 // rate)
    assert torch.equal(seen[0].detach(), xr)
    fmap[-1].sum().backward()
    # ... is the conv stack's own input gradient (recomputed apart: the library convolutions'
    # backward may order its sums differently from call to call) ...
    xin = xr.clone().requires_grad_(True)
    h = xin
    for layer in msd.convs:
        h = layer(h)
    msd.conv_post(h).sum().backward()
    assert grads[0].shape == xin.grad.shape
    assert rel_err(grads[0].cpu().numpy(), xin.grad.cpu().numpy()) < 1e-4
    # ... and x receives the resampler's adjoint of it, bit for bit
    plan, taps, first = _table(44100, 44100 // rate)
    want = ops.resample_adjoint(grads[0].reshape(2, -1).contiguous(), taps, first, plan["old"],
                                plan["W"], 8192).reshape(2, 1, 8192)
    assert torch.equal(x.grad, want)
    assert float(x.grad.abs().max()) > 0
