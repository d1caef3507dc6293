"""Integrated loudness on the device: `loudness(x, sample_rate)` and `normalize_loudness`.

audiotools' `AudioSignal.loudness` is the ITU-R BS.1770-4 integrated loudness of its `Meter`, and
`AudioSignal.normalize(db)` / the `VolumeNorm` transform of the training recipe
(conf/vrvq/vrvq_a2_lufs.yml, `VolumeNorm.db: [const, -16]`) scale a batch by
exp((db - loudness) ln10 / 20). The reference measures on the host with scipy's lfilter (or, on a
GPU batch, with an FIR stand-in for the K-weighting). Here a GPU tensor is measured by the HIP
scan of include/vrvq.h "Integrated loudness": the exact fourth-order recurrence in fp64, no copy
to the host and no sync, so both functions run under graph capture. A CPU tensor takes
`codec.loudness`, the host restatement the device path is tested against.
"""
from __future__ import annotations

import torch

from . import ops
from .codec import GAIN_FACTOR
from .codec import loudness as _host_loudness


def _items(x: torch.Tensor) -> torch.Tensor:
    if x.dim() == 2:
        x = x[:, None]
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError("loudness: x must be (nb, nac, nt) or (nb, nt), none of them empty "
                         f"(got {tuple(x.shape)})")
    if x.shape[1] > 5:
        raise ValueError(f"loudness: 1 to 5 channels have a BS.1770 gain (got {x.shape[1]})")
    return x


def loudness(x: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """Integrated loudness (LUFS) per item of x (nb, nac, nt) or (nb, nt), floored at -70:
    float32 (nb,) on x's device, rounded once from the fp64 measurement as audiotools rounds its
    own. Input shorter than 0.5 s is measured as if zero-padded to 0.5 s. No host sync on the
    GPU."""
    sample_rate = int(sample_rate)
    if sample_rate <= 0:
        raise ValueError(f"loudness: the sample rate must be positive (got {sample_rate})")
    x = _items(x)
    if not x.is_cuda:
        return _host_loudness(x, sample_rate)
    x = x.detach().to(torch.float32).contiguous()
    return ops.loudness(x, sample_rate).to(torch.float32)


def loudness_gain(ref: torch.Tensor, db) -> torch.Tensor:
    """exp((db - ref) ln10 / 20) in float32 on ref's device: the gain that takes loudness `ref`
    (per item) to `db` (a number or a per-item tensor)."""
    # a number stays a number: no host-to-device copy, which a graph capture would refuse
    db = db.to(ref.device, torch.float32) if isinstance(db, torch.Tensor) else float(db)
    return torch.exp((db - ref) * GAIN_FACTOR)


def normalize_loudness(x: torch.Tensor, sample_rate: int, db=-16.0, return_loudness: bool = False):
    """x scaled per item to `db` LUFS (a number or a per-item tensor): audiotools'
    AudioSignal.normalize and the VolumeNorm transform, gain = exp((db - loudness) ln10 / 20) in
    float32. With return_loudness, (scaled, loudness before scaling). No host sync on the GPU."""
    ref = loudness(x, sample_rate)
    gain = loudness_gain(ref, db)
    y = x * gain.reshape((-1,) + (1,) * (x.dim() - 1))
    return (y, ref) if return_loudness else y
