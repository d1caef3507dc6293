"""Integrated loudness on the GPU (vrvq_amd/csrc/loudness.hip) against the long-double
restatement of tests/loudness_ref.py, on the inputs of tests/loudness_cases.py.

Bounds. The fp64 output of the op is within 1e-10 LU of the reference: a cap, about 14 times the
worst error of a float64 emulation of the chunked scan with float64-powered transition matrices
(5-7e-12 LU) and four orders below the 1e-6 the codec tests hold input_db to. The float32 value
equals codec.loudness (the host yardstick) bit for bit; the reference values are at least 1e-9 LU
from a float32 rounding midpoint and every block at least 1e-3 LU from a gate (asserted, not
assumed), so neither side can round or gate the other way within its error.

Measured on an MI355X: worst |op - reference| over all cases 1.7e-12 LU (test_error_bound prints
it)."""
import numpy as np
import pytest
import torch

import loudness_cases as cases
import vrvq_amd
from vrvq_amd import codec, ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = list(cases.cases())
LD = np.longdouble


@pytest.fixture(scope="module")
def measured():
    """{name: (fp64 op output, vrvq_amd.loudness float32, codec.loudness float32)} as NumPy."""
    out = {}
    for name in NAMES:
        x, sr = cases.tensor(name)
        xd = x.to(DEV)
        out[name] = (ops.loudness(xd, sr).cpu().numpy(), vrvq_amd.loudness(xd, sr).cpu().numpy(),
                     codec.loudness(x, sr).numpy())
    return out


def test_preconditions():
    ref = cases.reference()
    for name in NAMES:
        lufs, margin = ref[name]
        assert np.all(margin >= 1e-3), (name, margin)
        assert all(cases.float32_midpoint_distance(v) >= 1e-9 for v in lufs), name


def test_error_bound(measured):
    ref = cases.reference()
    worst = {}
    for name in NAMES:
        got = measured[name][0]
        assert got.dtype == np.float64 and got.shape == (2,)
        worst[name] = float(np.abs(got.astype(LD) - ref[name][0]).max())
    for name, e in worst.items():
        print(f"{name}: |op - long double| = {e:.3g} LU")
    print(f"worst over all cases: {max(worst.values()):.3g} LU")
    assert max(worst.values()) <= 1e-10, worst
    assert measured["44k1_zeros"][0][1] == -70.0  # an all-zero item reads exactly -70


@pytest.mark.parametrize("name", NAMES)
def test_float32_equals_the_host_yardstick(measured, name):
    _, got, host = measured[name]
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), (got, host)
    assert np.array_equal(got, measured[name][0].astype(np.float32))  # rounded once from the fp64


@pytest.mark.parametrize("name", ["44k1_3s17_stereo", "11k025_2s_stereo", "16k_3000_padded"])
def test_bits_do_not_depend_on_the_batch(measured, name):
    x, sr = cases.tensor(name)
    xd = x.to(DEV)
    both = measured[name][0]
    alone = ops.loudness(xd[1:2].contiguous(), sr).cpu().numpy()
    three = ops.loudness(torch.cat([xd[0:1], xd[1:2], xd[0:1]]).contiguous(), sr).cpu().numpy()
    again = ops.loudness(xd, sr).cpu().numpy()
    bits = lambda a: a.view(np.uint64)  # noqa: E731
    assert bits(alone)[0] == bits(both)[1] == bits(three)[1]
    assert bits(three)[0] == bits(three)[2] == bits(both)[0]
    assert np.array_equal(bits(again), bits(both))


def test_shapes():
    x, sr = cases.tensor("44k1_5000_padded")
    xd = x.to(DEV)
    a = vrvq_amd.loudness(xd, sr)
    b = vrvq_amd.loudness(xd[:, 0], sr)
    assert a.shape == b.shape == (2,) and a.device == xd.device and torch.equal(a, b)
    # a view is measured as its contents
    wide = torch.zeros(2, 1, 6000, device=DEV)
    wide[..., :5000] = xd
    assert torch.equal(vrvq_amd.loudness(wide[..., :5000], sr), a)


def test_normalize_loudness():
    x, sr = cases.tensor("44k1_3s17_stereo")
    xd = x.to(DEV)
    y, before = vrvq_amd.normalize_loudness(xd, sr, return_loudness=True)
    assert torch.equal(before, vrvq_amd.loudness(xd, sr))
    after = codec.loudness(y.cpu(), sr)
    assert float((after + 16.0).abs().max()) < 1e-3
    db = torch.tensor([-20.0, -27.5])
    got = vrvq_amd.normalize_loudness(xd, sr, db.to(DEV)).cpu()
    want = codec.normalize(x, sr, db)  # host: measured by codec.loudness, gain on the CPU
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
    assert bool(((got - want).abs() <= ulp).all())
    assert torch.equal(codec.normalize(xd, sr, db).cpu(), got)  # codec's device route is this one
    mono = xd[:, :1].contiguous()  # (nb, nt) is (nb, 1, nt)
    assert torch.equal(vrvq_amd.normalize_loudness(mono[:, 0], sr, -16.0),
                       vrvq_amd.normalize_loudness(mono, sr, -16.0)[:, 0])


def test_graph_capture():
    x, sr = cases.tensor("44k1_chunk_edge_plus_1")
    x2, _ = cases.tensor("44k1_chunk_edge")
    x2 = torch.nn.functional.pad(x2, (0, 1)).to(DEV)
    static = x.to(DEV).clone()
    eager = vrvq_amd.normalize_loudness(x2, sr, -16.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vrvq_amd.normalize_loudness(static, sr, -16.0)  # warm the allocator off the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = vrvq_amd.normalize_loudness(static, sr, -16.0)
    static.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_compress_decompress_round_trip():
    """input_db is the host value in float32 bits, through one window and through several.
    decompress normalises the decoded windows to input_db and then crops them to the file's
    length, as the reference does (models/dac_base.py:295-301), so the file it returns reads
    input_db exactly when the crop removes nothing: a 1.3 s clip of a whole number of hops
    (112 x 512 samples), decoded as one window."""
    from test_codec import KW, SR, _signal
    from vrvq_amd.recipe import load_recipe

    model = vrvq_amd.DAC_VRVQ(**KW)
    load_recipe(model, 0)
    model = model.to(DEV).eval()
    n = 112 * model.hop_length
    assert abs(n / SR - 1.3) < 1e-3
    audio = _signal(n, 12)
    want = codec.loudness(audio, SR)
    for win in (1.0, 2.0):  # two windows with padding=False; one with padding=True
        dac = model.compress(audio, win_duration=win, max_batch=2)
        assert dac.padding == (win == 2.0)
        assert dac.input_db.device.type == "cpu" and dac.input_db.dtype == torch.float32
        assert np.array_equal(dac.input_db.numpy().view(np.uint32), want.numpy().view(np.uint32))
    sig = model.decompress(dac)
    assert sig.audio_data.is_cuda and sig.audio_data.shape == audio.shape
    back = codec.loudness(sig.audio_data.cpu(), SR)
    print(f"decompressed loudness {float(back[0]):.6f}, input_db {float(dac.input_db[0]):.6f}")
    assert float((back - dac.input_db).abs().max()) < 1e-3


def test_errors():
    with pytest.raises(ValueError, match="channels"):
        vrvq_amd.loudness(torch.zeros(1, 6, 30000, device=DEV), 44100)
    with pytest.raises(ValueError, match="sample rate"):
        vrvq_amd.loudness(torch.zeros(1, 1, 30000, device=DEV), 0)
    with pytest.raises(ValueError, match="sample rate"):
        vrvq_amd.loudness(torch.zeros(1, 1, 30000, device=DEV), -16000)
    with pytest.raises(ValueError, match="channels"):
        ops.loudness(torch.zeros(1, 6, 30000, device=DEV), 44100)
    with pytest.raises(ValueError, match="sample rate"):
        ops.loudness(torch.zeros(1, 1, 30000, device=DEV), 0)
