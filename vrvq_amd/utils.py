"""Importance-map gating and rate helpers (reference: models/utils.py:45-73,
scripts/inference.py:88-112) on gfx950 kernels."""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import ops


def _as_scaled(x: torch.Tensor) -> torch.Tensor:
    if x.dtype != torch.float32:
        raise RuntimeError("importance map must be float32")
    return x.contiguous()


def generate_mask_hard(x: torch.Tensor, nq: int) -> torch.Tensor:
    """mask[b, n, t] = 1.0 if x[b, 0, t] - n >= 0 else 0.0   (models/utils.py:55-61)."""
    return ops.mask_hard(_as_scaled(x), nq)


def generate_mask_ste(x: torch.Tensor, nq: int, alpha: float = 1) -> torch.Tensor:
    """Straight-through mask (models/utils.py:45-53): x (B, 1, T) the scaled importance map.

    Forward: mask_smooth + (mask_quant - mask_smooth).detach(), which equals the hard mask
    exactly in fp32 (for q = 0 it is s + (-s) = 0; for q = 1, s >= 0.5 and 1 - s is exact by
    Sterbenz). Backward (when x requires grad): d/dx of the log-cosh smooth step
    logcosh(alpha, x - n) (models/utils.py:11-32), summed over the nq rows. Both run in the
    mask STE kernels (include/vrvq.h vrvq_mask_ste with levels = NULL)."""
    from . import train
    x = _as_scaled(x)
    if x.requires_grad and torch.is_grad_enabled():
        return train.mask_ste(x, nq, float(alpha))
    return ops.mask_hard(x, nq)


def scale_importance(imp_map: torch.Tensor, a: float, c: float = 1.0) -> torch.Tensor:
    """(imp_map * a) * c with fp32 roundings (see include/vrvq.h vrvq_scale_imp)."""
    return ops.scale_imp(_as_scaled(imp_map), a, c)


def cal_bpf_from_mask(mask: torch.Tensor, bits_per_codebook: Sequence[float]) -> float:
    """Bits per frame: sum(mask * bits[n]) / (B * T), returned as a Python float like the
    reference's `.item()` (models/utils.py:64-73)."""
    return float(cal_bpf_tensor(mask, bits_per_codebook).item())


def cal_bpf_tensor(mask: torch.Tensor, bits_per_codebook: Sequence[float]) -> torch.Tensor:
    """Same as cal_bpf_from_mask but returns a 0-d device tensor (no host sync)."""
    bits = torch.as_tensor(list(bits_per_codebook), dtype=torch.float32).to(mask.device)
    return ops.bpf(mask.contiguous(), bits)


def _device_const(values, dtype, device) -> torch.Tensor:
    """A small 1-d device tensor of Python numbers. Equal values are one fill; under stream
    capture (where a host-to-device copy of pageable memory is not allowed) unequal ones are one
    fill each."""
    values = list(values)
    if all(v == values[0] for v in values):
        return torch.full((len(values),), values[0], dtype=dtype, device=device)
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return torch.cat([torch.full((1,), v, dtype=dtype, device=device) for v in values])
    return torch.tensor(values, dtype=dtype, device=device)


def _bits_table(bits_per_codebook, nq: int, device) -> torch.Tensor:
    if isinstance(bits_per_codebook, (int, float)):
        bits_per_codebook = [bits_per_codebook] * nq
    bits = [int(b) for b in bits_per_codebook]
    if len(bits) != nq or any(b != v for b, v in zip(bits, bits_per_codebook)):
        raise ValueError(f"bits_per_codebook: {nq} integer bit counts expected")
    return _device_const(bits, torch.int32, device)


def _imp_rows(imp_map: torch.Tensor) -> torch.Tensor:
    imp = _as_scaled(imp_map)
    if imp.dim() < 2 or imp.numel() != imp.shape[0] * imp.shape[-1]:
        raise RuntimeError("importance map must be (B, T) or (B, 1, T)")
    return imp.reshape(imp.shape[0], imp.shape[-1])


def rate_curve(imp_map: torch.Tensor, levels, nq: int, bits_per_codebook=10) -> torch.Tensor:
    """Bits per frame of every clip at every level, (B, L) float32, in one launch and without
    building a mask: the frame count of the RVQ kernels (include/vrvq.h "Rate control") summed
    per clip as integers, divided by T."""
    imp = _imp_rows(imp_map)
    if torch.is_tensor(levels):
        lv = levels.to(imp.device, torch.float32).reshape(-1).contiguous()
    else:
        lv = _device_const([float(v) for v in levels], torch.float32, imp.device)
    total = ops.rate_curve(imp, lv, _bits_table(bits_per_codebook, nq, imp.device))
    return (total.to(torch.float64) / imp.shape[1]).to(torch.float32)


def kbps_to_budget(kbps: float, frames: int, sample_rate: int, hop_length: int) -> int:
    """Whole bits that `frames` frames may take at `kbps`, at the frame rate
    floor(sample_rate / hop_length) of scripts/inference.py:112."""
    return int(math.floor(float(kbps) * 1000 / math.floor(sample_rate / hop_length) * frames))


def solve_levels(imp_map: torch.Tensor, target_kbps, *, nq: int, sample_rate: int,
                 hop_length: int, level_min: float, level_max: float, bits_per_codebook=10,
                 pooled: bool = False):
    """The largest level in [level_min, level_max] at which each clip (or, pooled, the whole
    batch as one group) stays within `target_kbps`, solved on the device in one launch
    (include/vrvq.h vrvq_rate_solve). target_kbps: a number, or one per clip (not pooled).
    Returns device tensors (levels (G,) float32, bpf (G,) float32, status (G,) int32; 0 solved,
    1 infeasible even at level_min, 2 level_max fits), G = B, or 1 when pooled. No host sync for
    a number or a host sequence."""
    imp = _imp_rows(imp_map)
    B, T = imp.shape
    if level_min is None or level_max is None:
        raise ValueError("solve_levels: level_min and level_max are required")
    if torch.is_tensor(target_kbps) or isinstance(target_kbps, np.ndarray):
        target_kbps = target_kbps.tolist()
    scalar = not isinstance(target_kbps, (list, tuple))
    if pooled:
        if not scalar:
            raise ValueError("solve_levels: a pooled solve takes one target_kbps")
        budgets, frames = [kbps_to_budget(target_kbps, B * T, sample_rate, hop_length)], B * T
        off = _device_const([0, B], torch.int32, imp.device)
    else:
        ks = [target_kbps] * B if scalar else list(target_kbps)
        if len(ks) != B:
            raise ValueError(f"solve_levels: {len(ks)} targets for {B} clips")
        budgets, frames = [kbps_to_budget(k, T, sample_rate, hop_length) for k in ks], T
        off = torch.arange(B + 1, dtype=torch.int32, device=imp.device)
    budget = _device_const(budgets, torch.int64, imp.device)
    levels, total, status = ops.rate_solve(imp, _bits_table(bits_per_codebook, nq, imp.device),
                                           off, budget, level_min, level_max)
    return levels, (total.to(torch.float64) / frames).to(torch.float32), status


def masked_sum(z_q_is: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """z_q = sum_i z_q_is[:, i] * mask[:, i, None, :]   (scripts/inference.py:99-100)."""
    return ops.masked_sum(z_q_is.contiguous(), mask.contiguous())


def check_errors(device=None) -> None:
    """End-of-work check for the fused RVQ launches' bounded in-kernel waits (include/vrvq.h
    vrvq_rvq_pending_error): synchronises the device, then raises RuntimeError if any launch
    completed by now timed out (its outputs were poisoned: codes -1, NaN z_q). The RVQ ops also
    raise on such a code at their next call; a one-shot caller (a single encode, the last call of
    a sweep) calls this after its own work instead. Clears the code it reports."""
    from . import _lib
    torch.cuda.synchronize(device)
    code = _lib.rvq_pending_error()
    if code:
        raise RuntimeError(
            f"vrvq: a fused RVQ launch timed out in an in-kernel hand-off (code {code}: "
            f"{'projection partials' if code == 1 else 'stage rows'}); its outputs are invalid "
            "(codes -1, NaN)")


def sweep_latents(imp_map: torch.Tensor, z_q_is: torch.Tensor, levels: Sequence[float],
                  n_q: int):
    """Per level: hard mask of imp_map * (level * Nq) and the masked sum of z_q_is
    (scripts/inference.py:95-100). Returns (masks, z_q stacked level-major as (L*B, D, T))."""
    masks = [generate_mask_hard(scale_importance(imp_map, level * n_q, 1.0), n_q)
             for level in levels]
    return masks, torch.cat([masked_sum(z_q_is, m) for m in masks])


def level_sweep(model, audio: torch.Tensor, levels: Sequence[float], bits_per_codebook: int = 10,
                decode: bool = True, max_decode_clips: int | None = None):
    """The reference's VBR level sweep (scripts/inference.py:88-112) without file I/O.

    Encodes once (level 1), then for each level: hard mask of imp_map * (level * Nq),
    masked sum of z_q_is, bpf and kbps. The levels' z_q are decoded as batches of up to
    `max_decode_clips` clips (default: all L*B at once, the fastest; the reference decodes level
    by level, so a cap of B keeps its peak decoder memory). Clips are independent, but a conv's
    tile choice can depend on the batch size, so the per-level recon agrees with a per-level
    decode within fp32 rounding, not bit for bit (tests/test_gpu_parity.py checks the batched
    recon against the reference's per-level fixtures). Returns a list of dicts."""
    n_q = model.n_codebooks
    with torch.no_grad():
        x = model.preprocess(audio, model.sample_rate)
        enc = model.encode(x, n_quantizers=None, level=1)
        masks, z_all = sweep_latents(enc["imp_map"], enc["z_q_is"], levels, n_q)
        recon_all = None
        if decode:
            cap = max_decode_clips or z_all.shape[0]
            if cap < 1:
                raise ValueError("max_decode_clips must be >= 1")
            recon_all = torch.cat([model.decode(z_all[i:i + cap])
                                   for i in range(0, z_all.shape[0], cap)])
    check_errors(audio.device)  # the sweep's one encode: a timed-out hand-off raises here
    B = audio.shape[0]
    out = []
    for li, level in enumerate(levels):
        mask = masks[li]
        bpf = cal_bpf_from_mask(mask, [bits_per_codebook] * n_q)
        kbps = bpf * math.floor(model.sample_rate / model.hop_length) / 1000
        recon = recon_all[li * B:(li + 1) * B] if decode else None
        out.append({"level": level, "level_scaled": level * n_q, "mask": mask,
                    "z_q": z_all[li * B:(li + 1) * B], "recon": recon, "bpf": bpf, "kbps": kbps})
    return out
