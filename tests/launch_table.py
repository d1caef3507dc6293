"""The conv launches of a model, in launch order, found without a GPU: the model runs on the CPU
with the tensor ops of vrvq_amd.ops replaced by shape-only stand-ins that note every conv call
(its shape, whether it was handed bf16x3 planes, one launch or two for a residual unit), and each
noted call is put to the host planner (vrvq_conv_plan) at B = 1.

tests/golden/launch_table_parent.json was written by `python tests/launch_table.py --record` with
this file placed in a checkout of the commit named in the fixture's header, so it holds what that
commit's own layers and training step launched; tests/test_launch_table.py recomputes the table
from the code under test. Nothing here states a path rule: a row says what was called.

Rows, per model: the eval chained path (encoder, importance subnet, decoder) as `eval/<weight>`,
then the training step's convs as `train/<weight>` (forwards) and `train/<weight>/adjoint` (input
gradients, in the backward's order). A row is
    [role, kind, cin, cout, k, stride, pad, dil, planes, ru, tin8, plan8, tin87, plan87]
kind "conv" / "proj" / "convt", or "ru" for a residual unit in one launch (planes then "k7,k1" as
two 0 / 1 digits, no plan: the planner covers conv entry points); ru is "fused", "two" (a conv
of a unit run as two launches) or "" (no unit); tinN the input length and planN the planner's
[BM, BN, KS, x3, S, path, WM] for the clip that gives N latent frames (8 and 87: the smallest that
reach the narrow and the 96-wide tiles).
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from vrvq_amd import _lib, ops  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "launch_table_parent.json")
FRAMES = (8, 87)
PLAN_KEYS = ("BM", "BN", "KS", "x3", "S", "path", "WM")
# one width off the default: channel counts outside the fused set and no multiple of 16
OFF_DEFAULT = dict(encoder_dim=48, decoder_dim=768, n_codebooks=8, level_min=0.125, level_max=6)


def model_configs():
    """name -> DAC_VRVQ kwargs: every distinct configuration tests/golden/manifest.json names
    (under the first name that has it), plus the off-default width."""
    with open(os.path.join(HERE, "golden", "manifest.json")) as f:
        man = json.load(f)
    named = list(man["yml_kwargs"].items())
    named += [(k, v["kwargs"]) for k, v in man.items() if isinstance(v, dict) and "kwargs" in v]
    out, seen = {}, set()
    for name, kw in named:
        key = json.dumps(kw, sort_keys=True)
        if key not in seen:
            seen.add(key)
            out[name] = kw
    out["off_default_48_768"] = OFF_DEFAULT
    return out


# ---------------------------------------------------------------------------- stand-ins
def _stand_ins(calls):
    """{name: function} for vrvq_amd.ops: packers hand the weight through (so a call's weight
    names its layer by address), convs note themselves in `calls` and return empty outputs."""
    E = torch.empty

    def pair(y, out_snake, want_raw):
        if out_snake is None:
            return y
        return (y if want_raw else None), torch.empty_like(y)

    def note(kind, x, w, cout, k, stride, pad, dil, planes, fused=False):
        calls.append(dict(w=w.data_ptr(), kind=kind, cin=x.shape[1], cout=cout, k=k, stride=stride,
                          pad=pad, dil=dil, planes=planes, fused=fused, tin=x.shape[2]))

    def conv1d(x, w_packed, cout, cout_pad, k, stride=1, pad=0, dil=1, bias=None, alpha=None,
               inv_alpha=None, residual=None, epilogue=0, out_snake=None, want_raw=True,
               w_x3=None):
        note("conv", x, w_packed, cout, k, stride, pad, dil, int(w_x3 is not None))
        y = E(x.shape[0], cout, ops.conv_out_len(x.shape[2], k, stride, pad, dil))
        return pair(y, out_snake, want_raw)

    def conv1d_proj(x, w_packed, cout, k, w3in, nq, pad=0, dil=1, bias=None, alpha=None,
                    inv_alpha=None, w_x3=None, want_z=False):
        note("proj", x, w_packed, cout, k, 1, pad, dil, int(w_x3 is not None))
        T = ops.conv_out_len(x.shape[2], k, 1, pad, dil)
        return E(8, x.shape[0] * T, 8 * nq), (E(x.shape[0], cout, T) if want_z else None)

    def conv_transpose1d(x, w_packed, cout, cout_pad, stride, bias=None, alpha=None,
                         inv_alpha=None, out_snake=None, want_raw=True, pad=-1, w_x3=None):
        p = (stride + 1) // 2 if pad < 0 else pad
        note("convt", x, w_packed, cout, 2 * stride, stride, p, 1, int(w_x3 is not None))
        y = E(x.shape[0], cout, ops.convt_out_len(x.shape[2], stride, pad))
        return pair(y, out_snake, want_raw)

    def residual_unit(x, x_snk, dil, w7, b7, alpha2, inv_alpha2, w1, b1, cout_pad, out_snake=None,
                      want_raw=True, w7_x3=None, w1_x3=None):
        C = x.shape[1]
        note("ru", x, w7, C, 7, 1, 3 * dil, dil,
             f"{int(w7_x3 is not None)},{int(w1_x3 is not None)}", fused=True)
        return pair(torch.empty_like(x), out_snake, want_raw)

    def rvq(B, T, cb, w_out, want_z_q_is, want_mask):
        nq, D = cb.shape[0], w_out.shape[1]
        return (torch.zeros(B, nq, T, dtype=torch.long), E(B, nq * 8, T), E(B, nq, T),
                E(B, nq, D, T) if want_z_q_is else None, E(B, D, T),
                E(B, nq, T) if want_mask else None)

    def rvq_encode(z, w_in_t, b_in, cb, cbf, c2, w_out, b_out, mcol, qb, imp=None, level=1.0,
                   want_z_q_is=True, want_mask=True):
        return rvq(z.shape[0], z.shape[2], cb, w_out, want_z_q_is, want_mask)

    def rvq_encode_part(part, frames, b_in, cb, cbf, c2, w_out, b_out, mcol, qb, imp=None,
                        level=1.0, want_z_q_is=True, want_mask=True):
        return rvq(part.shape[1] // frames, frames, cb, w_out, want_z_q_is, want_mask)

    def snake_backward(x, alpha, inv_alpha, grad, want_dx=True):
        return (torch.empty_like(x) if want_dx else None), E(x.shape[1])

    planes = torch.zeros(1, dtype=torch.int16)
    return dict(
        conv1d=conv1d, conv1d_proj=conv1d_proj, conv_transpose1d=conv_transpose1d,
        residual_unit=residual_unit, rvq_encode=rvq_encode, rvq_encode_part=rvq_encode_part,
        weight_norm=lambda g, v: v, snake_inv_alpha=lambda a: a,
        pack_conv1d_weight=lambda w: (w, ops.round_up(w.shape[0], 128)),
        pack_convt1d_weight=lambda w, s: (w, ops.round_up(w.shape[1] * s, 128)),
        pack_conv1d_flip=lambda w: (w, ops.round_up(w.shape[1], 128)),
        pack_x3_weight=lambda wp, k: planes, pack_x3_strided_weight=lambda w, s: planes,
        codebook_prep=lambda cb: (cb, cb[..., 0]), rvq_frag=lambda cbn: cbn,
        rvq_pack_w_in=lambda w: w,
        rvq_cross_prep=lambda wi, wo, bo: (E(wi.shape[0], wi.shape[0], 8, 8), E(wi.shape[0], 8)),
        masked_loss=lambda loss_pf, mask: torch.zeros(()),
        act_backward=lambda y, grad, epi: torch.empty_like(y),
        bias_grad=lambda grad: E(grad.shape[1]),
        conv1d_wgrad=lambda a, x, k, *r, **kw: E(a.shape[1], x.shape[1], k),
        weight_norm_backward=lambda g, v, dw: (torch.empty_like(g), torch.empty_like(v)),
        snake_backward=snake_backward)


class _Patched:
    """vrvq_amd.ops with the stand-ins in place, put back on exit."""

    def __init__(self, calls):
        self.new = _stand_ins(calls)

    def __enter__(self):
        self.old = {k: getattr(ops, k) for k in self.new}
        for k, f in self.new.items():
            setattr(ops, k, f)

    def __exit__(self, *exc):
        for k, f in self.old.items():
            setattr(ops, k, f)


# ---------------------------------------------------------------------------- the walk
def _walk(model, frames):
    """(role, call) of every conv launch of one eval forward and one training step's convs on a
    B = 1 clip of `frames` latent frames."""
    from vrvq_amd import train
    from vrvq_amd.layers import ResidualUnit
    names = {p.data_ptr(): n[:-len(".weight_v")] for n, p in model.named_parameters()
             if n.endswith(".weight_v")}
    in_unit = {f"{n}.block.{i}" for n, m in model.named_modules() if isinstance(m, ResidualUnit)
               for i in (1, 3)}
    x = torch.zeros(1, 1, frames * model.hop_length)
    out = []

    def take(calls, stage, adjoint_from=None):
        for i, c in enumerate(calls):
            name = names[c.pop("w")]
            role = f"{stage}/{name}" + ("/adjoint" if adjoint_from is not None and
                                        i >= adjoint_from else "")
            c["ru"] = "fused" if c.pop("fused") else "two" if name in in_unit else ""
            out.append((role, c))

    calls = []
    with _Patched(calls):
        model.eval()
        with torch.no_grad():
            enc = model.encode(x) if model.model_type == "CBR" else model.encode(x, None, 1.0)
            model.decode(enc["z_q"])
        take(calls, "eval")
        del calls[:]
        # the training step's convs: encoder, importance subnet, decoder (the quantizer between
        # them launches no conv), then their backward
        model.train()
        z, feat = train.encoder_forward(model.encoder, x)
        loss = train.decoder_forward(model.decoder, z).sum()
        if model.model_type == "VBR":
            loss = loss + train.imp_subnet_forward(model.quantizer.imp_subnet, feat).sum()
        n_fwd = len(calls)
        loss.backward()
        take(calls, "train", adjoint_from=n_fwd)
    return out


def _plan(c):
    planes = c["planes"] if isinstance(c["planes"], int) else None
    if planes is None:
        return None
    try:
        p = _lib.conv_plan(c["kind"], 1, c["cin"], c["tin"], c["cout"], c["k"], c["stride"],
                           c["pad"], c["dil"], bool(planes), c["kind"] != "convt")
    except RuntimeError as e:
        return str(e)
    return [p[k] for k in PLAN_KEYS]


SHAPE = ("kind", "cin", "cout", "k", "stride", "pad", "dil", "planes", "ru")


def table(kwargs):
    """The rows of one model (module docstring)."""
    import vrvq_amd
    torch.manual_seed(0)
    model = vrvq_amd.DAC_VRVQ(**kwargs)
    walks = [_walk(model, f) for f in FRAMES]
    rows = []
    for per_len in zip(*walks):
        role, c0 = per_len[0]
        assert all(r == role and [c[k] for k in SHAPE] == [c0[k] for k in SHAPE]
                   for r, c in per_len), role
        row = [role] + [c0[k] for k in SHAPE]
        for _r, c in per_len:
            row += [c["tin"], _plan(c)]
        rows.append(row)
    assert len({len(w) for w in walks}) == 1
    return rows


def tables():
    return {name: table(kw) for name, kw in model_configs().items()}


def record(commit):
    doc = {"header": {
        "commit": commit,
        "method": "python tests/launch_table.py --record <commit>, run in a checkout of that "
                  "commit: its own WNConv1d / WNConvTranspose1d.prepared_x3, "
                  "ResidualUnit.runs_fused and train._x3 / _x3s decided every row (the ops are "
                  "shape-only stand-ins, the plans come from vrvq_conv_plan at B = 1)",
        "row": ["role"] + list(SHAPE) + [f"{n}{f}" for f in FRAMES for n in ("tin", "plan")],
        "plan": list(PLAN_KEYS)},
        "models": tables()}
    with open(GOLDEN, "w") as f:
        f.write('{"header": ' + json.dumps(doc["header"], indent=1) + ',\n"models": {\n')
        blocks = []
        for name, rows in doc["models"].items():
            body = ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows)
            blocks.append(json.dumps(name) + ": [\n" + body + "\n]")
        f.write(",\n".join(blocks) + "\n}}\n")
    return doc


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        d = record(sys.argv[2])
        print({k: len(v) for k, v in d["models"].items()})
    else:
        sys.exit("usage: python tests/launch_table.py --record <commit>")
