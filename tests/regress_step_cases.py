"""The cases the fused regression-step tests share (engine/regress_step.py, csrc/cdx_regress_step.hip): small on purpose -- the largest
case has 33 rows.  Every case builds its tower (a stock ``nn.Sequential``, tests/tower_cases.py) and its batch from seeds; the strided
cases hand the step views of one (B, H, D) batch as the Decision Diffuser and Decision Veteran pipelines do.  ``autograd_reference`` is
the float64 reference: ``((net(cat([x0, x1])) - y) ** 2).mean()`` differentiated by autograd (reference invdynamic/mlp.py:54-60).
``rel_err`` is the error measure: max |a - b| / max |b|."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_cases as tc  # noqa: E402


def _c(rows, a0, a1, widths, acts, norm=False, view=None, batch=None, fancy=False):
    """`a0`, `a1`: the rows are [x0 | x1] (a1 == 0: x0 alone); `norm`: as tests/tower_cases.py; `view`: None (contiguous matrices),
    "dd" (x0, x1, y = obs[:, :-1], obs[:, 1:], act[:, :-1] of a `batch` = (B, H) batch) or "dv" (obs[:, 0], obs[:, 1], act[:, 0]);
    `fancy`: the ensemble's Linear-LayerNorm-Mish-Dropout stack in eval mode."""
    return SimpleNamespace(rows=rows, a0=a0, a1=a1, widths=list(widths), acts=list(acts), norm=norm, view=view, batch=batch, fancy=fancy)


_INV = ["relu", "relu", "tanh"]
CASES = {
    # rows 1 / 16 / 17 / 33 on the shape of MlpInvDynamic (ReLU, ReLU, tanh); hidden 16 and 32
    "invdyn_r1_k22_h32": _c(1, 11, 11, [32, 32, 3], _INV),
    "invdyn_r16_k22_h16": _c(16, 11, 11, [16, 16, 3], _INV),
    "invdyn_r17_k22_h32": _c(17, 11, 11, [32, 32, 3], _INV),             # K0 = 22: no multiple of 16 (nor of 4: scalar weight loads)
    "invdyn_r33_k22_h32": _c(33, 11, 11, [32, 32, 3], _INV),
    # the smallest input (o_dim 1); x0 alone; last widths 1 and 64
    "k2_r17": _c(17, 1, 1, [16, 3], ["relu", "tanh"]),
    "x0_alone_r17_w1": _c(17, 14, 0, [32, 32, 1], ["mish", "mish", None]),       # SfBC's critic: a scalar regression
    "last64_r17": _c(17, 11, 11, [32, 64], ["silu", "tanh"]),
    # one layer (no H buffer); LayerNorm layers (the ensemble's "fancy" stack in eval mode: its last Linear is hidden x hidden)
    "depth1_r17": _c(17, 11, 11, [3], ["tanh"]),
    "fancy_eval_r17_h32": _c(17, 11, 11, [32, 32, 32], ["mish", "mish", None], norm=[True, True, False], fancy=True),
    # the last activation: none / relu / silu / mish (tanh: above)
    "last_none_r17": _c(17, 11, 11, [32, 3], ["relu", None]),
    "last_relu_r17": _c(17, 11, 11, [32, 3], ["relu", "relu"]),
    "last_silu_r17": _c(17, 11, 11, [32, 3], ["relu", "silu"]),
    "last_mish_r17": _c(17, 11, 11, [32, 3], ["relu", "mish"]),
    # views of one (B, H, D) batch: 7 x 3 = 21 rows (the tile boundary at row 16 falls inside the sixth block); inner 1
    "dd_view_7x4x11": _c(21, 11, 11, [32, 32, 3], _INV, view="dd", batch=(7, 4)),
    "dv_view_5x3x11": _c(5, 11, 11, [32, 32, 3], _INV, view="dv", batch=(5, 3)),
}
# the edge of what regress_plan admits: K0 512, two 512-wide layers, a last width of 64 -- 136.7 KiB of LDS
ENVELOPE = {"envelope_r17_k512": _c(17, 448, 64, [512, 512, 64], _INV)}
CASES.update(ENVELOPE)
TABLE = list(CASES)


def build(case, dtype=torch.float32, device="cpu"):
    """The tower as a stock ``nn.Sequential``."""
    seq = tc.build(tc._c(case.rows, case.a0 + case.a1, case.widths, case.acts, norm=case.norm), seed=3, dtype=dtype, device=device)[0]
    if case.fancy:                                          # Linear-LN-Mish-Dropout-Linear-LN-Mish-Linear-Identity, as EnsembleMlpInvDynamic
        mods = list(seq)
        seq = nn.Sequential(*mods[:3], nn.Dropout(0.1), *mods[3:], nn.Identity()).eval()
    return seq


def make_inputs(case, seed=13, dtype=torch.float32, device="cpu") -> SimpleNamespace:
    """x0 (.., a0), x1 (.., a1) or None, y (.., W): contiguous matrices, or the pipelines' views of one batch."""
    g = torch.Generator().manual_seed(seed)
    W = case.widths[-1]
    if case.view is None:
        n = case.rows
        x0 = torch.randn(n, case.a0, generator=g) * (0.2 + 1.8 * torch.rand(n, 1, generator=g))
        x1 = torch.randn(n, case.a1, generator=g) if case.a1 else None
        y = torch.randn(n, W, generator=g).tanh()
        move = lambda t: None if t is None else t.to(device=device, dtype=dtype)      # noqa: E731
        return SimpleNamespace(x0=move(x0), x1=move(x1), y=move(y))
    B, H = case.batch
    assert case.a0 == case.a1
    obs = (torch.randn(B, H, case.a0, generator=g) * (0.2 + 1.8 * torch.rand(B, H, 1, generator=g))).to(device=device, dtype=dtype)
    act = torch.randn(B, H, W, generator=g).tanh().to(device=device, dtype=dtype)
    if case.view == "dd":                                   # pipelines/dd_d4rl_*.py:89-90
        inp = SimpleNamespace(x0=obs[:, :-1], x1=obs[:, 1:], y=act[:, :-1])
    else:                                                   # pipelines/veteran_d4rl_*.py:253
        inp = SimpleNamespace(x0=obs[:, 0, :], x1=obs[:, 1, :], y=act[:, 0, :])
    assert inp.x0.numel() == case.rows * case.a0 and not inp.x0.is_contiguous()
    return inp


def request(rs, case, net, inp):
    """The request object of engine/regress_step.py for this tower and this batch."""
    from cleandiffuser_amd.engine import tower
    d = rs.describe(net)
    assert d is not None
    q = rs.make_request(d, [p.detach() for p in tower.params_of(d)], inp.x0, inp.x1, inp.y)
    assert rs.shapes_ok(q)
    return q


def autograd_reference(case, dtype=torch.float64) -> dict:
    """The step in `dtype` on the CPU by plain autograd -> the loss, out (R, W) and the gradient of every parameter in the order of
    ``tower.params_of`` (= ``net.parameters()``)."""
    net = build(case, dtype=dtype)
    inp = make_inputs(case, dtype=dtype)
    x = inp.x0 if inp.x1 is None else torch.cat([inp.x0, inp.x1], -1)
    out = net(x)
    loss = ((out - inp.y) ** 2).mean()
    loss.backward()
    return {"loss": loss.detach(), "out": out.detach().reshape(-1, case.widths[-1]), "grads": [p.grad.detach() for p in net.parameters()]}


def rel_err(got, ref) -> float:
    """max |got - ref| / max |ref| (0 / 0 = 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    return err / top if top > 0 else err


def buffers(q) -> dict:
    """name -> tensor of everything the launch writes; the gradient buffers times R W (d_out carries 1 / (R W))."""
    lv, n = q.live, q.R * q.W
    out = {"x_cat": q.x_cat, "out": lv.out[0], "loss_part": q.loss_part}
    for l, norm in enumerate(lv.norm):
        if l < len(lv.width) - 1:
            out[f"H[{l}]"] = lv.H[0][l]
        out[f"G[{l}]"] = lv.G[0][l] * n
        if norm:
            out[f"Sb[{l}]"], out[f"Sg[{l}]"] = lv.Sb[0][l] * n, lv.Sg[0][l] * n
    return out


def sizes_request(rs, k0, widths, a0=None, rows=40):
    """A ``CdxRegressStep`` of sizes alone (every pointer null): what the C side's size checks and LDS plan read."""
    import ctypes
    a0 = k0 if a0 is None else a0
    net = rs.CdxCriticNet(K0=k0, n_towers=1, n_layers=len(widths), width=(ctypes.c_int32 * 6)(*widths), act=(ctypes.c_int32 * 6)(),
                          norm=(ctypes.c_int32 * 6)())
    op = lambda w: rs.CdxRegressRows(width=w, ld=max(w, 1), inner=1, period=1)      # noqa: E731
    return rs.CdxRegressStep(R=rows, net=net, x0=op(a0), x1=op(k0 - a0), y=op(widths[-1]))


# ------------------------------------------------------------------------------------------------------------------- #
# Three ``update`` steps of MlpInvDynamic, written once for the fixture generator (tools/gen_regress_step_golden.py: the real          #
# reference on the CPU) and the tests (this package)                                                                          #
# ------------------------------------------------------------------------------------------------------------------- #
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "invdyn_steps.npz")
STEPS, LR = 3, 1e-3
GOLDEN_CASES = {"r33": CASES["invdyn_r33_k22_h32"], "dd_view_7x4x11": CASES["dd_view_7x4x11"]}


def invdyn_of(kind: str):
    """``MlpInvDynamic`` of this repository ("amd") or of the real reference ("reference")."""
    import importlib
    if kind == "amd":
        return importlib.import_module("cleandiffuser_amd.invdynamic").MlpInvDynamic
    from oracle.ref_import import import_reference
    import_reference()
    return importlib.import_module("cleandiffuser.invdynamic").MlpInvDynamic


def run_invdyn(cls, case, device="cpu") -> dict:
    """STEPS ``update`` steps (Adam, lr 1e-3) from ``load_synth`` weights -> the loss of every step, the first step's gradients, the
    parameter checksums (mean, mean |.|) after the last."""
    from cleandiffuser_amd.utils.synth import synth_state_dict
    head = cls(case.a0, case.widths[-1], hidden_dim=case.widths[0], out_activation=nn.Tanh(), optim_params={"lr": LR}, device=device)
    head.mlp.load_state_dict({k: v.to(device) for k, v in synth_state_dict(head.mlp.state_dict(), 41).items()})
    out, losses = {}, []
    for i in range(STEPS):
        inp = make_inputs(case, seed=13 + i, device=device)
        losses.append(float(head.update(inp.x0, inp.y, inp.x1)["loss"]))
        if i == 0:
            out.update({f"grad/{n}": p.grad.detach().cpu().numpy().copy() for n, p in head.mlp.named_parameters()})
    out["loss"] = np.array(losses, dtype=np.float64)
    out["sums"] = np.array([[float(p.detach().double().mean()), float(p.detach().double().abs().mean())] for p in head.mlp.parameters()])
    return out


def golden(name: str) -> dict:
    with np.load(GOLDEN) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
