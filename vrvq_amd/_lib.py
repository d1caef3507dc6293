"""ctypes binding of the C-ABI in include/vrvq.h (libvrvq_hip.so, built in-tree for gfx950).

The library is the product: every arithmetic op of the hot path runs in it. There is no
fallback — if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes
import os
import threading

LIB_NAME = "libvrvq_hip.so"
LIB_PATH = os.environ.get("VRVQ_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float

# name -> argtypes (restype is int status unless noted). Mirrors include/vrvq.h exactly;
# tests/test_capi.py checks this table against the header and the exported symbols.
SIGNATURES = {
    "vrvq_weight_norm": [_P, _P, _I, _I, _P, _P],
    "vrvq_snake_inv_alpha": [_P, _I, _P, _P],
    "vrvq_snake": [_P, _I, _I, _I, _P, _P, _P, _P],
    "vrvq_phase_split": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P],
    "vrvq_codebook_prep": [_P, _I, _I, _P, _P, _P],
    "vrvq_conv1d": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _I,
                    _P, _P, _P, _P],
    "vrvq_conv1d_workspace": [_I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vrvq_conv1d_ws": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P,
                       _I, _P, _P, _P, _P, ctypes.c_longlong, _P],
    "vrvq_conv1d_proj": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _I,
                         _P, _P, ctypes.c_longlong, _P],
    "vrvq_x3_weight_size": [_I, _I, _I, _P],
    "vrvq_pack_x3_weight": [_P, _I, _I, _I, _P, _P],
    "vrvq_pack_conv1d_weight": [_P, _I, _I, _I, _I, _P, _P],
    "vrvq_residual_unit": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P,
                           _P, _P, _P],
    "vrvq_conv_transpose1d": [_P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "vrvq_conv_transpose1d_pad": [_P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P,
                                  _P, _P],
    "vrvq_pack_convt1d_weight": [_P, _I, _I, _I, _I, _P, _P],
    "vrvq_rvq_cross_prep": [_P, _P, _P, _I, _I, _I, _P, _P, _P],
    "vrvq_rvq_cross_prep_precise": [_P, _P, _P, _I, _I, _I, _P, _P, _P],
    "vrvq_rvq_frag": [_P, _I, _I, _I, _P, _P],
    "vrvq_rvq_workspace": [_I, _I, _I, _P],
    "vrvq_rvq_encode": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F,
                        _P, _P, _P, _P, _P, _P, _P, ctypes.c_longlong, _P],
    "vrvq_rvq_w_in_planes_size": [_I, _I, _I, _P],
    "vrvq_rvq_pack_w_in": [_P, _I, _I, _I, _P, _P],
    "vrvq_rvq_workspace_part": [_I, _I, _I, _I, _P],
    "vrvq_rvq_encode_part": [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F,
                             _P, _P, _P, _P, _P, _P, _P, ctypes.c_longlong, _P],
    "vrvq_rvq_fused_clips": [_I, _I, _I, _P],
    "vrvq_rvq_project": [_P, _I, _I, _I, _I, _I, _P, _P, _P],
    "vrvq_rvq_chain": [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P,
                       _P],
    "vrvq_rvq_expand": [_P, _I, _I, _I, _I, _I, _P, _P, _P, _F, _P, _P, _P, _P],
    "vrvq_rvq_gather": [_P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P],
    "vrvq_masked_loss": [_P, _P, _I, _I, _I, _P, _P],
    "vrvq_mask_hard": [_P, _I, _I, _I, _P, _P],
    "vrvq_scale_imp": [_P, _I, _F, _F, _P, _P],
    "vrvq_masked_sum": [_P, _P, _I, _I, _I, _I, _P, _P],
    "vrvq_bpf": [_P, _P, _I, _I, _I, _P, _P],
    "vrvq_rate_curve": [_P, _I, _I, _I, _P, _P, _I, _P, _P],
    "vrvq_rate_solve": [_P, _I, _I, _I, _P, _P, _I, _P, _F, _F, _P, _P, _P, _P],
    "vrvq_scale_imp_rows": [_P, _I, _I, _P, _P, _P],
    "vrvq_rate_solve_capped": [_P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _F, _F, _P, _P, _P, _P, _P,
                               _P, _P],
    "vrvq_scale_imp_packets": [_P, _I, _I, _P, _I, _P, _P],
    "vrvq_signal_metrics_workspace": [_I, ctypes.c_longlong, _P],
    "vrvq_signal_metrics": [_P, _P, _I, _I, ctypes.c_longlong, _P, _P, _P, _P, ctypes.c_longlong,
                            _P],
    "vrvq_bss_sdr_workspace": [_I, _I, ctypes.c_longlong, _I, _P],
    "vrvq_bss_sdr": [_P, _P, _I, _I, ctypes.c_longlong, _P, _I, _I, ctypes.c_double, _P, _P,
                     ctypes.c_longlong, _P],
    "vrvq_spectral_distance_workspace": [_I, ctypes.c_longlong, _I, _P, _P],
    "vrvq_spectral_distance": [_P, _P, _I, _I, ctypes.c_longlong, _P, _I, _P, _P, _P, _P, _P,
                               ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                               _P, _P, _P, ctypes.c_longlong, _P],
    "vrvq_spectral_distance_grad_workspace": [_I, ctypes.c_longlong, _I, _P, _P],
    "vrvq_spectral_distance_grad": [_P, _P, _I, _I, ctypes.c_longlong, _P, _I, _P, _P, _P, _P, _P,
                                    ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, _P, _P, _P, ctypes.c_longlong, _P],
    "vrvq_resample_plan": [_I, _I, _I, ctypes.c_double, ctypes.c_longlong, _P],
    "vrvq_resample_taps": [_I, _I, _I, ctypes.c_double, _P, ctypes.c_longlong, _P,
                           ctypes.c_longlong],
    "vrvq_resample": [_P, _I, ctypes.c_longlong, _I, _I, _I, _I, _P, _P, _P, ctypes.c_longlong,
                      _P],
    "vrvq_resample_adjoint": [_P, _I, ctypes.c_longlong, _I, _I, _I, _I, _P, _P, _P,
                              ctypes.c_longlong, _P],
    "vrvq_loudness_plan": [_I, _I, ctypes.c_longlong, _P],
    "vrvq_loudness": [_P, _I, _I, ctypes.c_longlong, _I, _P, _P, _P],
    "vrvq_pack_counts": [_P, _I, _I, _I, _P, _P, _P, _P, _P],
    "vrvq_pack_codes": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P],
    "vrvq_unpack_offsets": [_P, _I, _I, _P, _P, _P],
    "vrvq_unpack_codes": [_P, _P, _P, _I, _I, _I, _P, _P, _P],
    "vrvq_bitpack_plan": [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "vrvq_bitpack_write": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, ctypes.c_longlong, _P],
    "vrvq_bitunpack_plan": [_P, ctypes.c_longlong, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "vrvq_bitunpack_read": [_P, ctypes.c_longlong, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P,
                            _P],
    "vrvq_rvq_nearest": [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P],
    # training step
    "vrvq_wgrad_plan": [_I, _I, _I, _I, _I, _P, _P],
    "vrvq_conv1d_wgrad": [_P, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P,
                          ctypes.c_longlong, _P, _P],
    "vrvq_snake_backward_workspace": [_I, _I, _I, _P],
    "vrvq_snake_backward": [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, ctypes.c_longlong, _P],
    "vrvq_bias_grad_workspace": [_I, _I, _I, _P],
    "vrvq_bias_grad": [_P, _I, _I, _I, _P, _P, ctypes.c_longlong, _P],
    "vrvq_act_backward": [_P, _P, ctypes.c_longlong, _I, _P, _P],
    "vrvq_weight_norm_backward": [_P, _P, _P, _I, _I, _P, _P, _P],
    "vrvq_pack_conv1d_flip": [_P, _I, _I, _I, _I, _P, _P],
    "vrvq_mask_ste": [_P, _P, _P, _I, _I, _I, _F, _I, _I, _P, _P],
    "vrvq_mask_ste_backward": [_P, _P, _P, _I, _I, _I, _F, _I, _P, _P],
    "vrvq_rvq_expand_masked": [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "vrvq_rvq_backward_workspace": [_I, _I, _I, _P],
    "vrvq_rvq_backward": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P,
                          _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_longlong, _P],
}
EXTRA = {"vrvq_status_string": ([_I], ctypes.c_char_p), "vrvq_version": ([], _I),
         "vrvq_rvq_path": ([_I], _I), "vrvq_rvq_plan": ([_I] * 5 + [_P], _I),
         "vrvq_rvq_sync_error": ([_P, _P], _I), "vrvq_rvq_timing": ([_I], _I),
         "vrvq_rvq_timing_read": ([_P, _P], _I), "vrvq_rvq_pending_error": ([_P], _I),
         "vrvq_rvq_debug": ([ctypes.c_uint, ctypes.c_uint], _I),
         "vrvq_rvq_debug_capacity": ([_I], _I), "vrvq_conv_last_launch": ([_P], _I),
         "vrvq_conv_plan": ([_I] * 11 + [_P], _I),
         "vrvq_resample_error": ([], ctypes.c_char_p),
         "vrvq_loudness_error": ([], ctypes.c_char_p),
         "vrvq_bitstream_chunk_frames": ([], _I)}

METRICS_CHUNK = 16384  # VRVQ_METRICS_CHUNK of include/vrvq.h (tests/test_metrics.py compares)
SDR_CHUNK = 2048  # VRVQ_SDR_CHUNK (tests/test_sdr.py compares)
SDR_MAX_FILTER = 512  # filter_length's upper bound in vrvq_bss_sdr
SPECTRAL_TILE_SAMPLES = 8192  # VRVQ_SPECTRAL_TILE_SAMPLES (tests/test_spectral.py compares)
RESAMPLE_TILE = 512  # VRVQ_RESAMPLE_TILE (tests/test_resample.py compares)
LOUDNESS_CHUNK = 256  # VRVQ_LOUDNESS_CHUNK (tests/test_loudness.py compares)
LOUDNESS_PLAN_LEN = 30  # VRVQ_LOUDNESS_PLAN_LEN
BITSTREAM_CHUNK_FRAMES = 256  # VRVQ_BITSTREAM_CHUNK_FRAMES (tests/test_bitstream.py compares)


def spectral_tile_frames(window: int) -> int:
    """Frames of one workgroup's tile at this window: VRVQ_SPECTRAL_TILE_FRAMES of the header."""
    return SPECTRAL_TILE_SAMPLES // int(window)

_lock = threading.Lock()
_lib = None


def load() -> ctypes.CDLL:
    """Load libvrvq_hip.so (once). Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"vrvq_amd: HIP library {LIB_PATH} is missing; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = _I
        for name, (argtypes, restype) in EXTRA.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def call(name: str, *args) -> None:
    """Invoke a C-ABI entry point; raise RuntimeError with the library's message on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.vrvq_status_string(rc)
        raise RuntimeError(f"{name} failed ({rc}): {msg.decode() if msg else 'unknown'}")


def rvq_path(path: int = 0) -> int:
    """Select the RVQ launch structure (2: rvq_pt_kernel from the projection partials, default;
    1: chain and expansion as two launches; 0: query). Returns the previous path. Same outputs
    bit for bit."""
    prev = load().vrvq_rvq_path(path)
    if prev not in (1, 2):
        raise RuntimeError(f"vrvq_rvq_path({path}) failed ({prev})")
    return prev


def rvq_sync_error(stream: int) -> int:
    """Timeout code recorded by a fused RVQ launch on `stream` (0: none); clears it."""
    code = ctypes.c_int(0)
    call("vrvq_rvq_sync_error", ctypes.c_void_p(stream), ctypes.byref(code))
    return code.value


def rvq_pending_error() -> int:
    """Timeout code of any fused RVQ launch completed by now (0: none), no synchronisation;
    clears it."""
    code = ctypes.c_int(0)
    call("vrvq_rvq_pending_error", ctypes.byref(code))
    return code.value


def rvq_debug(spin_max: int = 0, stall: int = 0) -> None:
    """Test hook: bound every later fused launch's waits at spin_max polls (0: default) and delay
    its first chain part by stall x s_sleep(127)."""
    call("vrvq_rvq_debug", ctypes.c_uint(spin_max), ctypes.c_uint(stall))


def rvq_fused_clips(frames: int, nq: int, ncode: int = 1024) -> int:
    """Clips one fused launch from the conv's partials holds resident (0: the two-launch form
    runs; include/vrvq.h vrvq_rvq_fused_clips)."""
    n = ctypes.c_int(0)
    call("vrvq_rvq_fused_clips", frames, nq, ncode, ctypes.byref(n))
    return n.value


def rvq_debug_capacity(clips: int) -> int:
    """Test hook: cap the clips per fused launch from partials (0 forces the two launches, -1
    removes the cap). Returns the previous cap."""
    return int(load().vrvq_rvq_debug_capacity(int(clips)))


def conv_last_launch() -> dict:
    """Tile and path of the last conv launch on the MFMA tiles (include/vrvq.h
    vrvq_conv_last_launch): {BM, BN, KS, x3 (0 fp32-input, 1 chunk, 2 pair), S (split-K parts)}."""
    out = (ctypes.c_int * 5)()
    call("vrvq_conv_last_launch", out)
    return dict(zip(("BM", "BN", "KS", "x3", "S"), (int(v) for v in out)))


PLAN_KINDS = {"conv": 0, "proj": 1, "convt": 2}  # vrvq_plan_kind_t


def conv_plan(kind, batch: int, cin: int, tin: int, cout: int, k: int, stride: int = 1,
              pad: int = 0, dil: int = 1, x3: bool = True, workspace: bool = True) -> dict:
    """What a conv call of this shape would launch, decided on the host by the code that
    launches it (include/vrvq.h vrvq_conv_plan; no GPU needed). kind: "conv" (vrvq_conv1d /
    _ws), "proj" (vrvq_conv1d_proj) or "convt" (vrvq_conv_transpose1d_pad, k = 2 stride). Returns
    conv_last_launch()'s keys plus path (0: an MFMA tile, 1: small-Cout kernel, 2: Cin = 1
    stream kernel; the tile keys are 0 off the MFMA tiles) and WM; raises RuntimeError with the
    status the launch would return."""
    out = (ctypes.c_int * 7)()
    call("vrvq_conv_plan", PLAN_KINDS.get(kind, kind), batch, cin, tin, cout, k, stride, pad, dil,
         1 if x3 else 0, 1 if workspace else 0, out)
    return dict(zip(("BM", "BN", "KS", "x3", "S", "path", "WM"), (int(v) for v in out)))


def rvq_timing(on: bool) -> bool:
    """Attach HIP start / stop events to every rvq_pt_kernel launch (kernel duration on its
    stream) while on. Returns the previous setting."""
    return bool(load().vrvq_rvq_timing(1 if on else 0))


def rvq_timing_read():
    """(mean kernel ms, launches) of the launches recorded since the last read."""
    ms, n = ctypes.c_float(0.0), ctypes.c_int(0)
    call("vrvq_rvq_timing_read", ctypes.byref(ms), ctypes.byref(n))
    return float(ms.value), int(n.value)


RVQ_PLAN_KEYS = ("kind", "F", "P", "n_fb", "wg_per_clip", "lds", "resident", "clips", "launches",
                 "ws_bytes")
RVQ_PLAN_PT, RVQ_PLAN_CHAIN_EXPAND = 0, 1  # vrvq_rvq_plan_kind_t


def rvq_plan(batch: int, frames: int, nq: int, ncode: int = 1024, resident: int = 0) -> dict:
    """The launch plan of an rvq_encode_part call of this shape, and of rvq_encode after its
    projection launch (include/vrvq.h vrvq_rvq_plan),
    from the function that launches it. resident: workgroups of rvq_pt_kernel the device holds
    at once (given: no GPU needed; 0: ask the current device). Keys: RVQ_PLAN_KEYS."""
    out = (ctypes.c_longlong * 10)()
    call("vrvq_rvq_plan", batch, frames, nq, ncode, resident, out)
    return dict(zip(RVQ_PLAN_KEYS, (int(v) for v in out)))


RESAMPLE_PLAN_KEYS = ("old", "new", "W", "K", "ntaps", "out_length", "out_length_max",
                      "taps_len")


def _resample_call(name: str, *args) -> None:
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        why = lib.vrvq_resample_error() or lib.vrvq_status_string(rc)
        raise RuntimeError(f"{name} failed ({rc}): {why.decode() if why else 'unknown'}")


def resample_plan(old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945,
                  length: int = 0) -> dict:
    """The reduced ratio, the filter's half-width W and length K, the kept taps per phase and the
    output lengths of `length` input samples (include/vrvq.h vrvq_resample_plan; no GPU needed).
    Raises RuntimeError naming the reduced ratio where it is unsupported. Keys:
    RESAMPLE_PLAN_KEYS."""
    out = (ctypes.c_longlong * 8)()
    _resample_call("vrvq_resample_plan", int(old_sr), int(new_sr), int(zeros), float(rolloff),
                   int(length), out)
    return dict(zip(RESAMPLE_PLAN_KEYS, (int(v) for v in out)))


def resample_taps(old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945):
    """(taps float32 (new, ntaps), first int32 (new,)) as NumPy arrays: the tap table of
    include/vrvq.h vrvq_resample_taps, built on the host in fp64 and rounded once."""
    import numpy as np

    plan = resample_plan(old_sr, new_sr, zeros, rolloff)
    taps = np.empty((plan["new"], plan["ntaps"]), np.float32)
    first = np.empty((plan["new"],), np.int32)
    _resample_call("vrvq_resample_taps", int(old_sr), int(new_sr), int(zeros), float(rolloff),
                   taps.ctypes.data_as(ctypes.c_void_p), taps.size,
                   first.ctypes.data_as(ctypes.c_void_p), first.size)
    return taps, first


LOUDNESS_PLAN_INTS = ("eff_length", "win", "step", "blocks", "chunk", "chunks", "ws_bytes",
                      "pieces")


def loudness_plan(sample_rate: int, channels: int, length: int) -> dict:
    """How vrvq_loudness measures `length` samples of `channels` channels at `sample_rate`
    (include/vrvq.h vrvq_loudness_plan; no GPU needed): the integers LOUDNESS_PLAN_INTS (eff_length
    counts the zeros a signal under 0.5 s is measured with, ws_bytes is per item), "shelf" and
    "highpass" = (b0, b1, b2, a1, a2) with a0 = 1, and the chunk transition "M1", "M2", "K" as
    2 x 2 NumPy float64 arrays (s' = M1 s, t' = M2 t + K s over one chunk of zero input). Raises
    RuntimeError with the library's reason where the arguments are unsupported."""
    import numpy as np

    out = (ctypes.c_double * LOUDNESS_PLAN_LEN)()
    lib = load()
    rc = lib.vrvq_loudness_plan(int(sample_rate), int(channels), int(length), out)
    if rc != 0:
        why = lib.vrvq_loudness_error() or lib.vrvq_status_string(rc)
        raise RuntimeError(f"vrvq_loudness_plan failed ({rc}): "
                           f"{why.decode() if why else 'unknown'}")
    v = [float(d) for d in out]
    plan = {k: int(v[i]) for i, k in enumerate(LOUDNESS_PLAN_INTS)}
    plan["shelf"] = tuple(v[8:13])
    plan["highpass"] = tuple(v[13:18])
    for i, k in enumerate(("M1", "M2", "K")):
        plan[k] = np.array(v[18 + 4 * i:22 + 4 * i]).reshape(2, 2)
    return plan
