"""The layers' one packed-weight record (layers._WNConv.packed: fp32 pack, padded rows and bf16x3
planes under one key) follows its parameters and the ops.X3 switch: after an in-place update, and
after the switch is flipped on a live module, a forward equals a fresh module's bit for bit.

The in-place update is `weight_v.mul_(1.5)` under no_grad, the form an optimizer step takes. The
same write through `weight_v.data` leaves the parameter's version counter alone (torch hands out
a new counter with every `.data`), so no key built on `_version` -- this one or the two it
replaces -- can see it; whoever writes through `.data` clears `module._cache` themselves."""
import pytest
import torch

from vrvq_amd import ops
from vrvq_amd.layers import WNConv1d, WNConvTranspose1d

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, T = 2, 40


def _fresh(m):
    """A new module of m's geometry holding m's parameters: nothing cached."""
    if isinstance(m, WNConvTranspose1d):
        f = WNConvTranspose1d(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0],
                              m.padding[0])
    else:
        f = WNConv1d(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0],
                     m.dilation[0])
    f.load_state_dict(m.state_dict())
    return f.to(DEV)


def _module(make):
    torch.manual_seed(7)
    m = make().to(DEV)
    with torch.no_grad():
        m.bias.uniform_(-0.1, 0.1)
    x = torch.randn(B, m.in_channels, T, device=DEV)
    return m, x


@pytest.mark.parametrize("make", [
    lambda: WNConv1d(16, 16, 3, padding=1),
    lambda: WNConv1d(16, 32, 4, stride=2, padding=1),       # planes of the phase-split weight
    lambda: WNConvTranspose1d(16, 8, 4, stride=2, padding=1),
], ids=["conv_k3", "conv_k4_s2", "convt_k4_s2"])
def test_in_place_update_repacks(make):
    m, x = _module(make)
    assert m.prepared_x3() is not None
    with torch.no_grad():
        y0 = m(x)
        m.weight_v.mul_(1.5)
        y1 = m(x)
        want = _fresh(m)(x)
    assert torch.equal(y1, want)
    assert not torch.equal(y1, y0)


def test_switch_flip_on_a_live_module():
    m, x = _module(lambda: WNConv1d(16, 16, 7, padding=3))
    prev = ops.X3
    try:
        with torch.no_grad():
            for x3 in (True, False, True):
                ops.X3 = x3
                y = m(x)
                # the record in use is this setting's, not the one cached under the other
                assert (m.prepared_x3() is not None) == x3
                assert torch.equal(y, _fresh(m)(x)), x3
    finally:
        ops.X3 = prev
