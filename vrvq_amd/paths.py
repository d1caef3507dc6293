"""Path policy: which of two kernel forms a layer runs, decided here and nowhere else. Pure
functions of the layer's shape; no environment variable picks a path (DESIGN.md "Path policy").

Three rules: x3_planes and ru_fused below, and the eval encode handing z to the quantizer as its
stage projections (the one line in DAC_VRVQ.encode). Three module attributes switch a rule off for
a test: ops.X3, model.RVQ_PROJ, discriminator.MPD_1D.
"""
from __future__ import annotations

X3_TAPS = (1, 2, 3, 7)  # tap counts the bf16x3 chunk kernels exist for (csrc/conv_k*_x3.hip)


def x3_planes(kind: str, cin: int, k: int, stride: int) -> bool:
    """Does this conv get bf16x3 split planes of its weight (the x3 MFMA path, csrc/conv_x3.h)?
    kind "conv" (Conv1d: forwards, and the adjoints that run as one) or "convt" (the polyphase
    ConvTranspose1d, k = 2 stride: two taps per phase). Below 8 input channels the planner takes
    the Cin = 1 stream kernel or the small-Cout kernel whether or not it is given planes
    (tests/test_launch_table.py), so none are packed. A strided conv takes planes as the
    stride-1 k = 2 conv over the phase-split view of x: k = 2 stride, stride a power of two."""
    if cin < 8:
        return False
    if kind == "convt":
        return True
    if stride == 1:
        return k in X3_TAPS
    return k == 2 * stride and stride & (stride - 1) == 0


def ru_fused(channels: int, x3: bool) -> bool:
    """Does a ResidualUnit of this width run as one launch (vrvq_residual_unit)? C = 64 / 96 /
    128, and C = 256 only without planes: with them the two launches (k7 on the x3 path at 128-row
    tiles, then k1 + skip) beat the fused kernel, whose 256-row x3 weight stage does not fit
    twice per CU (profiles/r02zi_bench_ab.txt). C = 192 runs as two launches since the 192-row
    x3 k1 tiles (+2.8 % end to end, profiles/r04z_ru_fusion_ab.txt)."""
    return channels in (64, 96, 128) or (channels == 256 and not x3)
