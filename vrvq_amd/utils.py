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
             lengths=None, max_decode_clips: int | None = None) -> dict:
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
    "sisdr", "kbps"} with the batch means. One host sync, the check_errors at the end."""
    _check_vbr_eval(model, "rd_sweep")
    levels = [float(v) for v in levels]
    if not levels:
        raise ValueError("rd_sweep: no levels")
    n_q = model.n_codebooks
    with torch.no_grad():
        x = model.preprocess(audio, model.sample_rate)
        lengths = _clip_lengths(lengths, x.shape[0], x.device)
        enc = model.encode(x, n_quantizers=None, level=1)
        _masks, z_all = sweep_latents(enc["imp_map"], enc["z_q_is"], levels, n_q)
        recon = _decoded(model, z_all, max_decode_clips, x.shape[-1], "rd_sweep")
        out = signal_metrics(recon, x, lengths)
        bpf = rate_curve(enc["imp_map"], levels, n_q, bits_per_codebook).t().contiguous()
        kbps = bpf.to(torch.float64) * (math.floor(model.sample_rate / model.hop_length) / 1000)
        sisdr_mean, kbps_mean = out["si_sdr"].mean(1), kbps.mean(1)
    check_errors(audio.device)  # the sweep's one encode: a timed-out hand-off raises here
    out.update(levels=_device_const(levels, torch.float32, x.device), bpf=bpf, kbps=kbps,
               recon=recon)
    out["summary"] = [{"level": lv, "level_scaled": lv * n_q, "sisdr": s, "kbps": k}
                      for lv, s, k in zip(levels, sisdr_mean.tolist(), kbps_mean.tolist())]
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
    if metric not in QUALITY_METRICS:
        raise ValueError(f"solve_quality: metric {metric!r} is not one of {QUALITY_METRICS}")
    if int(iters) < 0:
        raise ValueError("solve_quality: iters must be >= 0")
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
    reconstruction reaches `min_db` (a number, or one per clip) in `metric` ("si_sdr", "si_snr"
    or "snr"), found by bisection with the decoder and the metric in the loop, all on the device.

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
    mask)."""
    target = _quality_args(model, audio, min_db, metric, iters)
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
    return {"level": hi, "value": value_hi, "level_lo": lo, "value_lo": value_lo,
            "status": status, "bpf": bpf, "kbps": kbps, "mask_imp": mask, "z_q": z_q,
            "codes": enc["codes"], "recon": recon}
