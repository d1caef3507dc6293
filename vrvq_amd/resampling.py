"""Sample-rate conversion on the device: `resample(x, old_sr, new_sr)`.

audiotools' `AudioSignal.resample` is `julius.resample_frac(x, old_sr, new_sr)` with julius'
defaults zeros = 24, rolloff = 0.945: a polyphase windowed-sinc FIR with replicate padding. The
reference calls it before every encode (scripts/inference.py:187, models/dac_base.py:182), after
every decode (:296) and inside the scale discriminator (models/discriminator.py:87). Neither
package is available to this project, so include/vrvq.h "Sample-rate conversion" is the
specification and parity with julius itself is unpinned.

The tap table of a ratio is built on the host in fp64 (vrvq_resample_taps), rounded once to fp32
and cached per (device, reduced ratio, zeros, rolloff). After one warm call per ratio the op
allocates through the caching allocator only and runs under graph capture.
"""
from __future__ import annotations

import threading
from typing import Optional

import torch

from . import _lib, ops

_tables: dict = {}
_tables_lock = threading.Lock()


def _table(device: torch.device, old_sr: int, new_sr: int, zeros: int, rolloff: float):
    """(plan, taps, first) on `device` for the ratio, from the cache or built now."""
    plan = _lib.resample_plan(old_sr, new_sr, zeros, rolloff)
    key = (device.type, device.index, plan["old"], plan["new"], int(zeros), float(rolloff))
    hit = _tables.get(key)
    if hit is None:
        with _tables_lock:
            hit = _tables.get(key)
            if hit is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(
                        f"resample: the tap table of {plan['old']}:{plan['new']} is not cached "
                        "yet; call resample once at this ratio before capturing a graph")
                taps, first = _lib.resample_taps(old_sr, new_sr, zeros, rolloff)
                hit = (torch.from_numpy(taps).to(device), torch.from_numpy(first).to(device))
                _tables[key] = hit
    return plan, hit[0], hit[1]


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, taps, first, old, width, out_length):
        ctx.table = (taps, first, old, width, x.shape[-1])
        return ops.resample(x, taps, first, old, width, out_length)

    @staticmethod
    def backward(ctx, dy):
        taps, first, old, width, length = ctx.table
        dx = _ResampleAdjoint.apply(dy.contiguous(), taps, first, old, width, length)
        return dx, None, None, None, None, None


class _ResampleAdjoint(torch.autograd.Function):
    """The operation is linear: the gradient of its adjoint is the operation."""

    @staticmethod
    def forward(ctx, dy, taps, first, old, width, length):
        ctx.table = (taps, first, old, width, dy.shape[-1])
        return ops.resample_adjoint(dy, taps, first, old, width, length)

    @staticmethod
    def backward(ctx, ddx):
        taps, first, old, width, out_length = ctx.table
        ddy = _Resample.apply(ddx.contiguous(), taps, first, old, width, out_length)
        return ddy, None, None, None, None, None


def resample_length(length: int, old_sr: int, new_sr: int) -> int:
    """Default output length of `length` samples: floor(new * length / old) in integers."""
    return int(new_sr) * int(length) // int(old_sr)


def resample(x: torch.Tensor, old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945,
             output_length: Optional[int] = None) -> torch.Tensor:
    """x (..., T) float32 on the GPU at old_sr -> (..., T') at new_sr, differentiable in x.

    T' = floor(new_sr * T / old_sr) unless output_length (at most ceil(new_sr * T / old_sr)) is
    given. Equal rates return x itself. Ratios whose reduced form exceeds 1024:1024 raise
    RuntimeError naming the reduced ratio."""
    old_sr, new_sr = int(old_sr), int(new_sr)
    if old_sr == new_sr:
        return x
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("resample: x must be a float32 tensor on the GPU (there is no CPU path)")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise RuntimeError("resample: x must be (..., T) with T >= 1")
    length = x.shape[-1]
    plan, taps, first = _table(x.device, old_sr, new_sr, zeros, rolloff)
    out_max = (plan["new"] * length + plan["old"] - 1) // plan["old"]
    out_length = plan["new"] * length // plan["old"] if output_length is None else int(output_length)
    if output_length is not None and not 0 <= out_length <= out_max:
        raise ValueError(f"resample: output_length {out_length} is outside [0, {out_max}]")
    if out_length == 0 or x.numel() == 0:
        return x.new_zeros(x.shape[:-1] + (out_length,))
    rows = x.reshape(-1, length).contiguous()
    y = _Resample.apply(rows, taps, first, plan["old"], plan["W"], out_length)
    return y.reshape(x.shape[:-1] + (out_length,))
