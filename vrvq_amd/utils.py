"""Importance-map gating and rate helpers (reference: models/utils.py:45-73,
scripts/inference.py:88-112) on gfx950 kernels."""
from __future__ import annotations

import functools
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


def net_budgets(budgets, frames: int, side_bits_per_frame: int = 0):
    """Bit budgets of groups of `frames` frames after frames * side_bits_per_frame bits of side
    information. May be negative: no level fits (solve_levels status 1)."""
    side = int(side_bits_per_frame)
    if side < 0 or side != side_bits_per_frame:
        raise ValueError("side_bits_per_frame must be a non-negative integer")
    return [int(b) - int(frames) * side for b in budgets]


def solve_levels(imp_map: torch.Tensor, target_kbps, *, nq: int, sample_rate: int,
                 hop_length: int, level_min: float, level_max: float, bits_per_codebook=10,
                 pooled: bool = False, side_bits_per_frame: int = 0):
    """The largest level in [level_min, level_max] at which each clip (or, pooled, the whole
    batch as one group) stays within `target_kbps`, solved on the device in one launch
    (include/vrvq.h vrvq_rate_solve). target_kbps: a number, or one per clip (not pooled).
    Returns device tensors (levels (G,) float32, bpf (G,) float32, status (G,) int32; 0 solved,
    1 infeasible even at level_min, 2 level_max fits), G = B, or 1 when pooled. No host sync for
    a number or a host sequence.

    side_bits_per_frame: bits every frame spends outside its codes (the count field of the
    bitstream container, codes_io.count_bits_of(nq)); frames * side_bits_per_frame are taken off
    each group's budget on the host before the solve, so codes + side information fit
    target_kbps. A budget that goes negative gives status 1. The returned bpf counts codes only."""
    imp = _imp_rows(imp_map)
    if level_min is None or level_max is None:
        raise ValueError("solve_levels: level_min and level_max are required")
    off, budget, frames = _rate_groups(imp, target_kbps, pooled, sample_rate, hop_length,
                                       side_bits_per_frame, "solve_levels")
    levels, total, status = ops.rate_solve(imp, _bits_table(bits_per_codebook, nq, imp.device),
                                           off, budget, level_min, level_max)
    return levels, (total.to(torch.float64) / frames).to(torch.float32), status


def _rate_groups(imp, target_kbps, pooled, sample_rate, hop_length, side_bits_per_frame, fn):
    """(group_off (G + 1,) int32, budget (G,) int64, frames per group) of a solve over the rows
    of imp (B, T): one group per row, or all rows pooled."""
    B, T = imp.shape
    if torch.is_tensor(target_kbps) or isinstance(target_kbps, np.ndarray):
        target_kbps = target_kbps.tolist()
    scalar = not isinstance(target_kbps, (list, tuple))
    if pooled:
        if not scalar:
            raise ValueError(f"{fn}: a pooled solve takes one target_kbps")
        budgets, frames = [kbps_to_budget(target_kbps, B * T, sample_rate, hop_length)], B * T
        off = _device_const([0, B], torch.int32, imp.device)
    else:
        ks = [target_kbps] * B if scalar else list(target_kbps)
        if len(ks) != B:
            raise ValueError(f"{fn}: {len(ks)} targets for {B} clips")
        budgets, frames = [kbps_to_budget(k, T, sample_rate, hop_length) for k in ks], T
        off = torch.arange(B + 1, dtype=torch.int32, device=imp.device)
    budget = _device_const(net_budgets(budgets, frames, side_bits_per_frame), torch.int64,
                           imp.device)
    return off, budget, frames


def packets_of(frames: int, packet_frames: int) -> int:
    """Packets of packet_frames frames in a row of `frames` frames (the last may be short)."""
    return (int(frames) - 1) // int(packet_frames) + 1


def solve_levels_capped(imp_map: torch.Tensor, target_kbps, max_kbps: float, packet_frames: int,
                        *, nq: int, sample_rate: int, hop_length: int, level_min: float,
                        level_max: float, bits_per_codebook=10, pooled: bool = False,
                        side_bits_per_frame: int = 0):
    """solve_levels with a cap on the short-term rate: no packet of `packet_frames` consecutive
    frames of a clip (the last packet of a clip may be shorter) exceeds `max_kbps`, and each clip
    (or, pooled, the batch) stays within `target_kbps`. A packet that its cap binds runs at the
    largest level that fits the cap; all other packets of a group share the largest level at which
    the group still meets its budget, so the bits the capped packets give up go to the others
    (include/vrvq.h vrvq_rate_solve_capped; two launches, no host sync for a number or a host
    sequence of targets).

    Budgets are kbps_to_budget's over each group's and each packet's own frame count (the short
    last packet gets a pro-rata budget), both less side_bits_per_frame per frame. Returns a dict
    of device tensors: "level" (G,) float32, the level of the group's uncapped packets, "bpf" (G,)
    float32 (codes only), "status" (G,) int32 as solve_levels; "packet_level" (B, NP) float32,
    "packet_bits" (B, NP) int64, "packet_status" (B, NP) int32 (0 at the group's level, 1
    infeasible: over max_kbps even at level_min, where it runs; 2 held by its cap)."""
    imp = _imp_rows(imp_map)
    T = imp.shape[1]
    if level_min is None or level_max is None:
        raise ValueError("solve_levels_capped: level_min and level_max are required")
    P = int(packet_frames)
    if P < 1 or P != packet_frames:
        raise ValueError("solve_levels_capped: packet_frames must be an integer >= 1")
    off, budget, frames = _rate_groups(imp, target_kbps, pooled, sample_rate, hop_length,
                                       side_bits_per_frame, "solve_levels_capped")
    NP = packets_of(T, P)
    sizes = (min(P, T), T - (NP - 1) * P)                     # a full packet, the last one
    full, tail = (net_budgets([kbps_to_budget(max_kbps, n, sample_rate, hop_length)], n,
                              side_bits_per_frame)[0] for n in sizes)
    packet_budget = torch.full((NP,), full, dtype=torch.int64, device=imp.device)
    if tail != full:
        packet_budget[NP - 1:].fill_(tail)                    # fills only: capturable
    level, total, status, p_level, p_total, p_status = ops.rate_solve_capped(
        imp, _bits_table(bits_per_codebook, nq, imp.device), off, budget, packet_budget, P,
        level_min, level_max)
    return {"level": level, "bpf": (total.to(torch.float64) / frames).to(torch.float32),
            "status": status, "packet_level": p_level, "packet_bits": p_total,
            "packet_status": p_status}


def masked_sum(z_q_is: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """z_q = sum_i z_q_is[:, i] * mask[:, i, None, :]   (scripts/inference.py:99-100)."""
    return ops.masked_sum(z_q_is.contiguous(), mask.contiguous())


def check_errors(device=None) -> None:
    """End-of-work check for the fused RVQ launches' bounded in-kernel waits (include/vrvq.h
    vrvq_rvq_pending_error): synchronises the device, then raises RuntimeError if any launch
    completed by now timed out (its outputs were poisoned: NaN z_q / z_q_is). The RVQ ops also
    raise on such a code at their next call; a one-shot caller (a single encode, the last call of
    a sweep) calls this after its own work instead. Clears the code it reports."""
    from . import _lib
    torch.cuda.synchronize(device)
    code = _lib.rvq_pending_error()
    if code:
        raise RuntimeError(
            f"vrvq: a fused RVQ launch timed out in an in-kernel hand-off (code {code}: an "
            "expansion's wait for the chain's stage rows); its outputs are invalid (NaN)")


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
    by level, so a cap of B keeps its peak decoder memory). Clips are independent and a clip's
    sums do not depend on the batch it runs in (DESIGN.md "Batch invariance": where a conv's
    tile width follows the batch, both widths add K in the same order;
    tests/test_gpu_parity.py test_batch_invariance_*), so the batched recon is the per-level
    decode's (tests/test_gpu_parity.py checks it against the reference's per-level fixtures).
    Returns a list of dicts."""
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


# ------------------------------------------------------------------ distortion and quality
METRICS = ("si_sdr", "si_snr", "snr", "l1")       # the columns of ops.signal_metrics
QUALITY_METRICS = ("si_sdr", "si_snr", "snr")     # in dB, larger is better: solve_quality targets


def _clip_lengths(lengths, clips: int, device):
    if lengths is None:
        return None
    if torch.is_tensor(lengths):
        lengths = lengths.reshape(-1).to(device, torch.int64).contiguous()
    else:
        lengths = _device_const([int(v) for v in lengths], torch.int64, device)
    if lengths.numel() != clips:
        raise ValueError(f"lengths: {lengths.numel()} given for {clips} clips")
    return lengths


def signal_metrics(est: torch.Tensor, ref: torch.Tensor, lengths=None) -> dict:
    """SI-SDR, SI-SNR, SNR (dB) and L1 of reconstructions against their inputs on the device:
    what models/utils.py:91-129 cal_metrics gets from torchmetrics, for every row at once and
    without a host sync (include/vrvq.h "Distortion metrics": float32 eps, sums in fp64).

    est is (R, T) or (R, 1, T), ref (B, T) or (B, 1, T) with R = L * B level-major (row r against
    clip r % B, the layout of sweep_latents / level_sweep); `lengths`, one per clip, counts only
    each clip's first samples. Returns "si_sdr", "si_snr", "snr", "l1" as (L, B) float64 and
    "moments" (L, B, 8) = sum p, t, p t, p^2, t^2, |p - t|, (p - t)^2 and n: adding the moments
    of clips or windows gives the pooled sums exactly as far as fp64 adds them."""
    B = ref.shape[0]
    metrics, moments = ops.signal_metrics(est.contiguous(), ref.contiguous(),
                                          _clip_lengths(lengths, B, est.device))
    L = est.shape[0] // B
    out = {name: metrics[:, i].reshape(L, B) for i, name in enumerate(METRICS)}
    out["moments"] = moments.reshape(L, B, 8)
    return out


BSS_SDR = "bss_sdr"                    # rd_sweep's column and solve_quality's metric name
BSS_SDR_MAX_FILTER = 512
BSS_SDR_MAX_ROWS = 65535               # vrvq_bss_sdr's bound on rows (a grid dimension)


def bss_sdr(est: torch.Tensor, ref: torch.Tensor, lengths=None, filter_length: int = 512,
            zero_mean: bool = False, load_diag=None) -> torch.Tensor:
    """BSS-eval SDR (dB) of reconstructions against their inputs on the device: the "SDR" of
    models/utils.py:91-143 cal_metrics, torchmetrics.functional.signal_distortion_ratio (without
    use_cg_iter), for every row at once and without a host sync (include/vrvq.h "BSS SDR"). The
    estimate is projected onto the span of the `filter_length` delayed copies of the reference,
    so a short linear filter between input and output (a delay, a tilt) is forgiven; the ratio is
    the energy inside that span over the energy outside it, all of it in fp64.

    est is (R, T) or (R, 1, T), ref (B, T) or (B, 1, T) with R = L * B level-major and `lengths`
    one per clip, as in signal_metrics; `zero_mean` removes each row's mean first, `load_diag` is
    added to the autocorrelation's lag 0. Returns (L, B) float64. The autocorrelation of a clip
    is formed once for its L reconstructions, its Levinson recursion once per four of them, and
    at most 65535 rows go into one call. A silent or empty row, a NaN in its data or a singular
    system gives NaN; est == ref gives +inf or NaN. Argument errors are ValueErrors before any
    launch."""
    for x, what in ((est, "est"), (ref, "ref")):
        if not torch.is_tensor(x) or x.dim() < 2 or x.numel() == 0 \
                or x.numel() != x.shape[0] * x.shape[-1]:
            raise ValueError(f"bss_sdr: {what} must be (rows, T) or (rows, 1, T)")
    R, B = est.shape[0], ref.shape[0]
    if ref.shape[-1] != est.shape[-1] or R % B:
        raise ValueError(f"bss_sdr: est {tuple(est.shape)} against ref {tuple(ref.shape)}")
    if R > BSS_SDR_MAX_ROWS:
        raise ValueError(f"bss_sdr: {R} rows; at most {BSS_SDR_MAX_ROWS} in one call")
    if not 1 <= int(filter_length) <= BSS_SDR_MAX_FILTER:
        raise ValueError(f"bss_sdr: filter_length {filter_length} is outside "
                         f"[1, {BSS_SDR_MAX_FILTER}]")
    out = ops.bss_sdr(est.contiguous(), ref.contiguous(), _clip_lengths(lengths, B, est.device),
                      int(filter_length), bool(zero_mean), load_diag)
    return out.reshape(R // B, B)


_bss_sdr = bss_sdr                     # rd_sweep has a flag of the function's name


# ------------------------------------------------------------------ spectral distances
SPECTRAL_METRICS = ("mel", "stft")     # distances, smaller is better: rd_sweep columns, solve_quality
MEL_DISTANCE = dict(windows=(2048, 512), n_mels=(150, 80), clamp_eps=1e-5, pow=2.0,
                    log_weight=1.0, mag_weight=1.0)    # models/loss.py:257 MelSpectrogramLoss()
STFT_DISTANCE = dict(windows=(2048, 512), n_mels=None, clamp_eps=1e-5, pow=2.0,
                     log_weight=1.0, mag_weight=1.0)   # models/loss.py:168 MultiScaleSTFTLoss()
SPECTRAL_MIN_SAMPLES = 1025            # both defaults' largest window is 2048: T > 1024


@functools.lru_cache(maxsize=None)
def spectral_tables(window: int) -> np.ndarray:
    """(3 W,) float32 of include/vrvq.h "Spectral distance": exp(-2 pi i k / W) as (re, im) pairs,
    then the periodic Hann window, both formed in float64 and rounded once."""
    ang = 2.0 * np.pi * np.arange(window, dtype=np.float64) / window
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1).reshape(-1)
    return np.concatenate([tw, 0.5 - 0.5 * np.cos(ang)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mel_bands(sample_rate: int, window: int, n_mels: int, fmin: float = 0.0, fmax=None):
    """The banded form of losses.mel_filters: (bands (3, n_mels) int32 = start, len, offset into
    the weights; weights float32, the rows' non-zero runs packed, fp32 values as they are).
    ValueError if a row's non-zeros are not one contiguous run (then the banded sum would not be
    the dense one)."""
    from .losses import mel_filters
    fb = mel_filters(int(sample_rate), int(window), int(n_mels), float(fmin),
                     None if fmax is None else float(fmax))
    bands, weights, off = np.zeros((3, n_mels), np.int32), [], 0
    for m, row in enumerate(fb):
        nz = np.flatnonzero(row)
        start, ln = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        if nz.size != ln:
            raise ValueError(f"mel filter {m} of ({window}, {n_mels}) is not one contiguous run")
        bands[:, m] = (start, ln, off)
        weights.append(row[start:start + ln])
        off += ln
    weights = np.concatenate(weights + [np.zeros(1, np.float32)]).astype(np.float32)
    return bands, weights


_spectral_cache: dict = {}


def _spectral_device_tables(device, sample_rate, windows, n_mels, fmin, fmax):
    """Per scale the device buffers of ops.spectral_distance, built once per (device,
    configuration) and kept. The first call of a configuration copies from the host, so it cannot
    be inside a stream capture; later calls can."""
    tables, bands, weights = [], [], []
    for w, m, lo, hi in zip(windows, n_mels, fmin, fmax):
        key = (str(device), w)
        if key not in _spectral_cache:
            _spectral_cache[key] = torch.from_numpy(spectral_tables(w)).to(device)
        tables.append(_spectral_cache[key])
        key = (str(device), sample_rate, w, m, lo, hi)
        if key not in _spectral_cache:
            if m > 0:
                b, wt = mel_bands(sample_rate, w, m, lo, hi)
                _spectral_cache[key] = (torch.from_numpy(b).to(device),
                                        torch.from_numpy(wt).to(device))
            else:
                _spectral_cache[key] = (torch.empty(0, dtype=torch.int32, device=device),
                                        torch.empty(0, dtype=torch.float32, device=device))
        bands.append(_spectral_cache[key][0])
        weights.append(_spectral_cache[key][1])
    return tables, bands, weights


def _rows_2d(x: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(x) or x.dim() < 2 or x.numel() == 0 \
            or x.numel() != x.shape[0] * x.shape[-1]:
        raise ValueError(f"spectral_distance: {what} must be (rows, T) or (rows, 1, T)")
    return x.reshape(x.shape[0], x.shape[-1]).contiguous()


def _per_scale(value, default, scales: int, what: str) -> list:
    if value is None:
        return [default] * scales
    value = list(value) if isinstance(value, (list, tuple)) else [value] * scales
    if len(value) != scales:
        raise ValueError(f"spectral_distance: {len(value)} {what} for {scales} windows")
    return value


class _SpectralDistance(torch.autograd.Function):
    """ops.spectral_distance whose "distance" carries a gradient to est: the backward is
    ops.spectral_distance_grad on the saved inputs (the spectra are recomputed; no host sync).
    The terms are not differentiable and ref gets no gradient. The backward is differentiable
    once only (once_differentiable: a double backward raises instead of treating the gradient as
    a constant); lengths and the cached table tensors are constants of the call, kept on ctx."""

    @staticmethod
    def forward(ctx, e, r, lengths, windows, mels, tables, bands, weights, scalars):
        terms, dist = ops.spectral_distance(e, r, lengths, windows, mels, tables, bands, weights,
                                            *scalars)
        ctx.save_for_backward(e, r)
        ctx.args = (lengths, windows, mels, tables, bands, weights, scalars)
        ctx.mark_non_differentiable(terms)
        return terms, dist

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _grad_terms, grad_dist):
        e, r = ctx.saved_tensors
        lengths, windows, mels, tables, bands, weights, scalars = ctx.args
        grad = ops.spectral_distance_grad(e, r, lengths, windows, mels, tables, bands, weights,
                                          *scalars, grad_dist.to(torch.float64).contiguous())
        return (grad,) + (None,) * 8


def spectral_distance(est: torch.Tensor, ref: torch.Tensor, *, windows, n_mels=None,
                      clamp_eps: float = 1e-5, pow: float = 2.0, log_weight: float = 1.0,
                      mag_weight: float = 1.0, mel_fmin=None, mel_fmax=None,
                      sample_rate: int = 44100, lengths=None) -> dict:
    """Multi-scale STFT or mel distance of reconstructions against their inputs, per row, on the
    device and without a host sync: per clip what models/loss.py:168-401 (MultiScaleSTFTLoss;
    MelSpectrogramLoss with levels=None) averages over the batch (include/vrvq.h "Spectral
    distance": hop = window / 4, centred frames with reflection, periodic Hann, |rfft|, optional
    Slaney mel projection, L1 of pow * log10 of the clamped magnitudes and L1 of the magnitudes,
    every mean in fp64). With rows of equal length the batch mean of "distance" is the reference
    loss.

    est is (R, T) or (R, 1, T), ref (B, T) or (B, 1, T) with R = L * B level-major as in
    signal_metrics; `windows` powers of two in [32, 2048]; `n_mels` one per window (0 or None: the
    linear bins); `lengths`, one per clip, measures each clip as if it ended there (a clip no
    longer than window / 2 gets NaN at that scale and in its distance). Returns "distance" (L, B),
    "log" and "mag" (L, B, S), float64. Argument errors are ValueErrors before any launch.

    Where est requires a gradient (and grad mode is on), "distance" carries a grad_fn whose
    backward is a HIP kernel too (ops.spectral_distance_grad: the spectra are recomputed, no
    spectrogram is kept and there is no host sync); the forward's launch and bits are the same.
    "log" and "mag" stay detached, and ref never receives a gradient, whether or not it requires
    one. mel_distance and stft_distance inherit this."""
    windows = [int(w) for w in (windows if isinstance(windows, (list, tuple)) else [windows])]
    S = len(windows)
    if not 1 <= S <= 16:
        raise ValueError("spectral_distance: 1 to 16 windows")
    mels = [int(m or 0) for m in _per_scale(n_mels, 0, S, "n_mels")]
    fmin = [float(v) for v in _per_scale(mel_fmin, 0.0, S, "mel_fmin")]
    fmax = [None if v is None else float(v) for v in _per_scale(mel_fmax, None, S, "mel_fmax")]
    for w, m in zip(windows, mels):
        if not (32 <= w <= 2048 and w & (w - 1) == 0):
            raise ValueError(f"spectral_distance: window {w} is no power of two in [32, 2048]")
        if not 0 <= m <= w // 2 + 1:
            raise ValueError(f"spectral_distance: n_mels {m} for window {w}")
    if not float(clamp_eps) > 0:
        raise ValueError("spectral_distance: clamp_eps must be > 0")
    e, r = _rows_2d(est, "est"), _rows_2d(ref, "ref")
    (R, T), B = e.shape, r.shape[0]
    if r.shape[1] != T or R % B:
        raise ValueError(f"spectral_distance: est {tuple(est.shape)} against ref "
                         f"{tuple(ref.shape)}")
    if lengths is None and T <= max(windows) // 2:
        raise ValueError(f"spectral_distance: {T} samples; window {max(windows)} needs more than "
                         f"{max(windows) // 2}")
    lengths = _clip_lengths(lengths, B, e.device)
    tables, bands, weights = _spectral_device_tables(e.device, int(sample_rate), windows, mels,
                                                     fmin, fmax)
    if e.requires_grad and torch.is_grad_enabled():
        scalars = (float(clamp_eps), float(pow), float(log_weight), float(mag_weight))
        terms, dist = _SpectralDistance.apply(e, r.detach(), lengths, windows, mels, tables, bands,
                                              weights, scalars)
    else:
        terms, dist = ops.spectral_distance(e, r, lengths, windows, mels, tables, bands, weights,
                                            clamp_eps, pow, log_weight, mag_weight)
    L = R // B
    return {"distance": dist.reshape(L, B), "log": terms[:, :, 0].reshape(L, B, S),
            "mag": terms[:, :, 1].reshape(L, B, S)}


def mel_distance(est: torch.Tensor, ref: torch.Tensor, sample_rate: int = 44100,
                 lengths=None) -> torch.Tensor:
    """The "mel distance" of the DAC-family papers per clip, (L, B) float64: spectral_distance with
    the defaults of models/loss.py:257 MelSpectrogramLoss (MEL_DISTANCE: n_mels (150, 80), windows
    (2048, 512), pow 2, log and magnitude terms with weight 1). Needs more than 1024 samples."""
    return spectral_distance(est, ref, sample_rate=sample_rate, lengths=lengths,
                             **MEL_DISTANCE)["distance"]


def stft_distance(est: torch.Tensor, ref: torch.Tensor, lengths=None) -> torch.Tensor:
    """The multi-scale STFT distance per clip, (L, B) float64: spectral_distance with the defaults
    of models/loss.py:168 MultiScaleSTFTLoss (STFT_DISTANCE: windows (2048, 512), linear bins,
    pow 2, weights 1). Needs more than 1024 samples."""
    return spectral_distance(est, ref, lengths=lengths, **STFT_DISTANCE)["distance"]


def _spectral_columns(spectral) -> tuple:
    if spectral is None:
        return ()
    cols = (spectral,) if isinstance(spectral, str) else tuple(spectral)
    for c in cols:
        if c not in SPECTRAL_METRICS:
            raise ValueError(f"spectral column {c!r} is not one of {SPECTRAL_METRICS}")
    return cols


def _spectral_metric(name: str, recon, x, sample_rate: int, lengths) -> torch.Tensor:
    if name == "mel":
        return mel_distance(recon, x, sample_rate, lengths)
    return stft_distance(recon, x, lengths)


def _check_vbr_eval(model, what: str) -> None:
    if getattr(model, "model_type", None) != "VBR":
        raise ValueError(f"{what} needs a VBR model (this one is CBR)")
    if model.training:
        raise ValueError(f"{what} is an eval-mode feature (training draws its own levels)")


def _decoded(model, z_all: torch.Tensor, cap, samples: int, what: str) -> torch.Tensor:
    cap = z_all.shape[0] if cap is None else cap
    if cap < 1:
        raise ValueError("max_decode_clips must be >= 1")
    recon = torch.cat([model.decode(z_all[i:i + cap]) for i in range(0, z_all.shape[0], cap)])
    if recon.shape[-1] != samples:
        raise ValueError(f"{what}: decode returns {recon.shape[-1]} samples for an input of "
                         f"{samples}; the metrics compare sample by sample")
    return recon


def rd_sweep(model, audio: torch.Tensor, levels: Sequence[float], bits_per_codebook=10,
             lengths=None, max_decode_clips: int | None = None, spectral=None,
             bss_sdr: bool = False) -> dict:
    """Rate-distortion curves of every clip: the table scripts/inference.py:95-122 writes
    (metadata.json, {"sisdr", "kbps"} per level), per clip and with the distortion computed on
    the device.

    Encodes once (level 1), builds the levels' latents with sweep_latents, decodes them in
    batches of up to `max_decode_clips` (default all L * B, as level_sweep) and measures all L * B
    reconstructions against the preprocessed input in one signal_metrics call (`lengths`: each
    clip's samples before padding, if only those should count). The rate is rate_curve's: the
    bits encode(level=...) spends, the RVQ kernels' (imp * level) * Nq, which is the sweep masks'
    imp * (level * Nq) wherever the two products round alike (always for power-of-two level * Nq).

    Returns "levels" (L,) float32, "bpf" (L, B) float32, "kbps" (L, B) float64, "si_sdr",
    "si_snr", "snr", "l1" (L, B) float64 and "moments" (L, B, 8) on the device, "recon"
    (L * B, 1, T), and "summary", the reference's table: per level {"level", "level_scaled",
    "sisdr", "kbps"} with the batch means. One host sync, the check_errors at the end.

    `spectral` (default None: nothing added) names spectral distances to measure as well, "mel"
    (mel_distance, the paper's other distortion axis) and / or "stft" (stft_distance): each adds
    an (L, B) float64 entry of that name, computed from the same `recon`, input and `lengths`,
    and its batch mean under the same name in every summary row. They need clips of more than
    1024 samples.

    `bss_sdr` (default False: nothing added, nothing more runs) adds "bss_sdr", the BSS-eval SDR
    (L, B) float64 of the function of that name at its defaults, from the same `recon`, input and
    `lengths`, and its batch mean under "bss_sdr" in every summary row."""
    _check_vbr_eval(model, "rd_sweep")
    levels = [float(v) for v in levels]
    if not levels:
        raise ValueError("rd_sweep: no levels")
    spectral = _spectral_columns(spectral)
    if spectral and audio.shape[-1] < SPECTRAL_MIN_SAMPLES:
        raise ValueError(f"rd_sweep: spectral distances need clips of at least "
                         f"{SPECTRAL_MIN_SAMPLES} samples")
    n_q = model.n_codebooks
    with torch.no_grad():
        x = model.preprocess(audio, model.sample_rate)
        lengths = _clip_lengths(lengths, x.shape[0], x.device)
        enc = model.encode(x, n_quantizers=None, level=1)
        _masks, z_all = sweep_latents(enc["imp_map"], enc["z_q_is"], levels, n_q)
        recon = _decoded(model, z_all, max_decode_clips, x.shape[-1], "rd_sweep")
        out = signal_metrics(recon, x, lengths)
        for name in spectral:
            out[name] = _spectral_metric(name, recon, x, model.sample_rate, lengths)
        if bss_sdr:
            out[BSS_SDR] = _bss_sdr(recon, x, lengths)
        extra = spectral + ((BSS_SDR,) if bss_sdr else ())  # (L, B) columns with a summary mean
        bpf = rate_curve(enc["imp_map"], levels, n_q, bits_per_codebook).t().contiguous()
        kbps = bpf.to(torch.float64) * (math.floor(model.sample_rate / model.hop_length) / 1000)
        sisdr_mean, kbps_mean = out["si_sdr"].mean(1), kbps.mean(1)
        extra_means = [out[name].mean(1) for name in extra]
    check_errors(audio.device)  # the sweep's one encode: a timed-out hand-off raises here
    out.update(levels=_device_const(levels, torch.float32, x.device), bpf=bpf, kbps=kbps,
               recon=recon)
    out["summary"] = [{"level": lv, "level_scaled": lv * n_q, "sisdr": s, "kbps": k}
                      for lv, s, k in zip(levels, sisdr_mean.tolist(), kbps_mean.tolist())]
    for name, means in zip(extra, extra_means):
        for row, v in zip(out["summary"], means.tolist()):
            row[name] = v
    return out


def quality_bisect_init(level_min: torch.Tensor, level_max: torch.Tensor, value_min: torch.Tensor,
                        value_max: torch.Tensor, target: torch.Tensor):
    """The bracket of solve_quality from the two end probes, per clip: (lo, hi, value_lo,
    value_hi, status). status 1: even level_max misses the target (NaN counts as a miss), the
    bracket is level_max twice; 2: level_min already reaches it, level_min twice; 0: lo =
    level_min, hi = level_max. A closed bracket stays where it is under the rounds: the midpoint
    sqrt(l * l) is l. Pure tensor code, any device."""
    miss = ~(value_max >= target)
    easy = ~miss & (value_min >= target)
    status = torch.where(miss, 1, torch.where(easy, 2, 0)).to(torch.int32)
    lo = torch.where(miss, level_max, level_min)
    hi = torch.where(easy, level_min, level_max)
    value_lo = torch.where(miss, value_max, value_min)
    value_hi = torch.where(easy, value_min, value_max)
    return lo, hi, value_lo, value_hi, status


def quality_midpoint(lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """The geometric midpoint of fp32 brackets (levels act as factors): the fp32 nearest to
    sqrt(lo * hi), formed in fp64, where the product is exact, so that the level does not depend
    on how a device or a vector width rounds an fp32 sqrt. sqrt(l * l) is l."""
    return torch.sqrt(lo.to(torch.float64) * hi.to(torch.float64)).to(torch.float32)


def quality_bisect_update(lo, hi, value_lo, value_hi, mid, value_mid, target):
    """One round of solve_quality's bisection, per clip: a midpoint that reaches the target
    (value_mid >= target; NaN does not) becomes hi, any other becomes lo. Keeps value_hi >= target
    and not value_lo >= target. Pure tensor code, any device: (lo, hi, value_lo, value_hi)."""
    ok = value_mid >= target
    return (torch.where(ok, lo, mid), torch.where(ok, mid, hi),
            torch.where(ok, value_lo, value_mid), torch.where(ok, value_mid, value_hi))


def _latents_at(imp: torch.Tensor, z_q_is: torch.Tensor, levels: torch.Tensor, nq: int):
    """Each clip at its own level, as encode(level=levels) gates it: scaled rows
    fl(imp * level), the mask of fl(rows * Nq) and the masked sum."""
    B, T = imp.shape
    rows = ops.scale_imp_rows(imp, levels)
    mask = ops.mask_hard(ops.scale_imp(rows, 1.0, float(nq)).reshape(B, 1, T), nq)
    return rows, mask, ops.masked_sum(z_q_is, mask)


def _quality_args(model, audio, min_db, metric: str, iters: int) -> torch.Tensor:
    """solve_quality's checks, all before a kernel; returns the (B,) float64 targets."""
    _check_vbr_eval(model, "solve_quality")
    q = model.quantizer
    if q.level_min is None or q.level_max is None:
        raise ValueError("solve_quality: the model needs level_min and level_max")
    if metric not in QUALITY_METRICS + (BSS_SDR,) + SPECTRAL_METRICS:
        raise ValueError(f"solve_quality: metric {metric!r} is not one of "
                         f"{QUALITY_METRICS + (BSS_SDR,) + SPECTRAL_METRICS}")
    if int(iters) < 0:
        raise ValueError("solve_quality: iters must be >= 0")
    if metric in SPECTRAL_METRICS and audio.shape[-1] < SPECTRAL_MIN_SAMPLES:
        raise ValueError(f"solve_quality: metric {metric!r} needs clips of at least "
                         f"{SPECTRAL_MIN_SAMPLES} samples")
    B = audio.shape[0]
    if torch.is_tensor(min_db) and min_db.dim() > 0:
        n, target = min_db.numel(), min_db.reshape(-1).to(audio.device, torch.float64)
    elif isinstance(min_db, (list, tuple, np.ndarray)):
        vals = [float(v) for v in min_db]
        n, target = len(vals), vals
    else:
        n, target = B, [float(min_db)] * B
    if n != B:
        raise ValueError(f"solve_quality: {n} targets for {B} clips")
    return target if torch.is_tensor(target) else _device_const(target, torch.float64,
                                                                audio.device)


def solve_quality(model, audio: torch.Tensor, min_db, metric: str = "si_sdr", iters: int = 8,
                  lengths=None) -> dict:
    """Constant-quality encoding: per clip a level in [level_min, level_max] whose
    reconstruction reaches `min_db` (a number, or one per clip) in `metric` ("si_sdr", "si_snr",
    "snr" or "bss_sdr", the BSS-eval SDR of bss_sdr at its defaults), found by bisection with the
    decoder and the metric in the loop, all on the device.

    One encode (codes and the importance map do not depend on the level), one decode of 2 B clips
    for level_max and level_min, then `iters` rounds, each scale_imp_rows -> mask -> masked_sum
    -> one decode of B clips -> signal_metrics at the geometric midpoint of every clip's bracket
    (quality_bisect_update), and one more such pass at the levels returned. Nothing is read back
    to the host, so the call can be captured in a graph; a one-shot caller ends with
    check_errors.

    The metric need not be monotonic in the level, so the contract is the bracket, not "the
    smallest such level": for status 0, value >= target > value_lo (or value_lo is NaN) with
    level / level_lo <= (level_max / level_min) ^ (2 ^ -iters) up to fp32 rounding.

    Returns "level" (B,) float32 and "value" (B,) float64, the metric measured at it (in the
    final pass; a round measured the same clip at the same level and batch size); "level_lo" /
    "value_lo", the last level that failed and its value; "status" (B,) int32: 0 solved, 1 the
    target is not reached even at level_max (level = level_lo = level_max), 2 level_min already
    reaches it (level = level_lo = level_min); and "bpf" (B,) float32, "kbps" (B,) float64,
    "mask_imp", "z_q", "codes", "recon" at "level" (encode(level=out["level"]) gives the same
    mask).

    metric "mel" or "stft" (mel_distance / stft_distance, clips of more than 1024 samples): a
    distance, smaller is better, so `min_db` is then an upper bound on it and the contract is
    flipped: status 0 means value <= target < value_lo (or value_lo is NaN), status 1 that even
    level_max stays above the target, status 2 that level_min is already within it. The bisection
    is the same, run on the negated distance; "value" and "value_lo" are the distances
    themselves."""
    target = _quality_args(model, audio, min_db, metric, iters)
    flipped = metric in SPECTRAL_METRICS
    if flipped:
        target = -target
    elif metric != BSS_SDR:
        col = METRICS.index(metric)
    nq, q = model.n_codebooks, model.quantizer
    with torch.no_grad():
        x = model.preprocess(audio, model.sample_rate)
        B, dev = x.shape[0], x.device
        lengths = _clip_lengths(lengths, B, dev)
        enc = model.encode(x, n_quantizers=None, level=1)
        imp, z_q_is = _imp_rows(enc["imp_map"]), enc["z_q_is"]
        level_min = torch.full((B,), float(q.level_min), dtype=torch.float32, device=dev)
        level_max = torch.full((B,), float(q.level_max), dtype=torch.float32, device=dev)

        def measure(z_q):
            recon = _decoded(model, z_q, None, x.shape[-1], "solve_quality")
            if flipped:  # (L, B) level-major rows -> one value per row, negated: larger is better
                return recon, -_spectral_metric(metric, recon, x, model.sample_rate,
                                                lengths).reshape(-1)
            if metric == BSS_SDR:
                return recon, ops.bss_sdr(recon, x, lengths)
            return recon, ops.signal_metrics(recon, x, lengths)[0][:, col]

        ends = torch.cat([_latents_at(imp, z_q_is, lv, nq)[2] for lv in (level_max, level_min)])
        value = measure(ends)[1]
        lo, hi, value_lo, value_hi, status = quality_bisect_init(
            level_min, level_max, value[B:], value[:B], target)
        for _ in range(int(iters)):
            mid = quality_midpoint(lo, hi)
            value_mid = measure(_latents_at(imp, z_q_is, mid, nq)[2])[1]
            lo, hi, value_lo, value_hi = quality_bisect_update(lo, hi, value_lo, value_hi, mid,
                                                               value_mid, target)
        rows, mask, z_q = _latents_at(imp, z_q_is, hi, nq)
        recon, value_hi = measure(z_q)
        bpf = rate_curve(rows, [1.0], nq)[:, 0].contiguous()  # the rows carry their levels
        kbps = bpf.to(torch.float64) * (math.floor(model.sample_rate / model.hop_length) / 1000)
        if flipped:
            value_hi, value_lo = -value_hi, -value_lo
    return {"level": hi, "value": value_hi, "level_lo": lo, "value_lo": value_lo,
            "status": status, "bpf": bpf, "kbps": kbps, "mask_imp": mask, "z_q": z_q,
            "codes": enc["codes"], "recon": recon}
