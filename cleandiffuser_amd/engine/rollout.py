"""Differentiable rollout of the row-MLP denoisers: ``sample(..., requires_grad=True)`` in two launches.

Diffusion-QL's policy update differentiates THROUGH the sampler (reference pipelines/dql_d4rl_mujoco.py:98-101: 5 DDPM steps of DQLMlp,
``actor_loss.backward()``).  Stepped on the host (``BaseDiffusionSDE._run_plan_torch`` over ``train.dql_forward``) that is ~25 launches
forward and 50-75 backward per denoising step.  Here the whole loop is ONE ``torch.autograd.Function``:

* forward  = ``cdx_rollout_fwd_f32`` (csrc/cdx_rollout.hip): all S steps for a 16-row tile per workgroup, saving X, P_raw, feat, Z, H;
* backward = ``cdx_rollout_bwd_f32``: the steps in reverse, d loss / d Z written over Z, then ONE ``cdx_conv_wgrad_f32`` product per layer
  over the S*B rows (``train._weight_grads``: in place / queued inside ``grads_in_place()``, handed to autograd outside) and one
  ``cdx_colsum_f32`` for the (S, E) gradient of the time-embedding table.

The time embedding ``time_mlp(map_noise(t_s))`` is per step, not per row: it is computed once per call on an (S, E) tensor under
autograd on the ordinary ``_LinearAct`` nodes, so ``time_mlp``'s parameter gradients flow as they always did.

``reference_forward`` / ``reference_backward`` restate the two kernels in plain torch on the same saved-tensor contract (explicit backward
formulas, no autograd): what the CPU tests run in place of the two C calls and what the GPU tests compare the buffers against.
``CDX_ROLLOUT=0`` keeps the host loop.
"""
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import blocks, train
from . import runtime as R
from .plan import KIND_DDIM, KIND_DDPM, V_XTHETA
from .rowtile import _bounds, declare, noise_index, reference_step, solver_env, step_admissible  # noqa: F401  (_bounds: tests/rollout_cases.py)

MAX_STEPS = 64             # CDX_ROLLOUT_MAX_STEPS: the step records travel in the kernel argument
MAX_WIDTH, MAX_FEATURES, MAX_X = 512, 512, 64


class CdxRollout(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("E", ctypes.c_int32), ("O", ctypes.c_int32), ("W", ctypes.c_int32),
                ("S", ctypes.c_int32), ("predict_noise", ctypes.c_int32), ("clip", ctypes.c_int32),
                ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("w3", ctypes.c_void_p), ("b3", ctypes.c_void_p), ("wh", ctypes.c_void_p), ("bh", ctypes.c_void_p),
                ("temb", ctypes.c_void_p), ("cond", ctypes.c_void_p), ("x_in", ctypes.c_void_p), ("prior", ctypes.c_void_p),
                ("fix_mask", ctypes.c_void_p), ("x_min", ctypes.c_void_p), ("x_max", ctypes.c_void_p), ("noise", ctypes.c_void_p),
                ("steps", ctypes.c_void_p),
                ("X", ctypes.c_void_p), ("P_raw", ctypes.c_void_p), ("feat", ctypes.c_void_p), ("Z", ctypes.c_void_p), ("H", ctypes.c_void_p),
                ("g_out", ctypes.c_void_p), ("G_head", ctypes.c_void_p), ("g_x", ctypes.c_void_p), ("g_cond", ctypes.c_void_p),
                ("g_temb", ctypes.c_void_p)]


def _lib():
    proto = ([ctypes.POINTER(CdxRollout), ctypes.c_void_p], ctypes.c_int)
    return declare(R.load_library(), {"cdx_rollout_fwd_f32": proto, "cdx_rollout_bwd_f32": proto})


def enabled() -> bool:
    return os.environ.get("CDX_ROLLOUT", "1") != "0"


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object both the kernels' binding and the torch restatement read and fill                                 #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(weights, temb, cond, x_in, prior, fix_mask, x_min, x_max, noise, steps, predict_noise: bool, clip: bool):
    """`weights` = (w1, b1, w2, b2, w3, b3, wh, bh); `steps` = the plan's Step records (kinds 0-2, vsel <= 1); bounds / mask (A,) or
    None; `noise` (n_noise, B, A) or None.  Allocates the saved-tensor buffers (the layout of include/cdx.h: cdx_rollout)."""
    b, a = x_in.shape
    w, f = weights[0].shape
    s, e = temb.shape
    o = f - a - e
    kw = dict(device=x_in.device, dtype=x_in.dtype)
    return SimpleNamespace(
        B=b, A=a, E=e, O=o, W=w, S=s, weights=tuple(weights), temb=temb, cond=cond, x_in=x_in, prior=prior, fix_mask=fix_mask,
        x_min=x_min if clip else None, x_max=x_max if clip else None, noise=noise, steps=list(steps), predict_noise=bool(predict_noise),
        clip=bool(clip),
        X=torch.empty(s + 1, b, a, **kw), P_raw=torch.empty(s, b, a, **kw), feat=torch.empty(s, b, f, **kw),
        Z=torch.empty(3, s, b, w, **kw), H=torch.empty(3, s, b, w, **kw),
        g_out=None, G_head=None, g_x=None, g_cond=None, g_temb=None)


def _c_request(q) -> "tuple":
    steps = R.pack_steps(q.steps)
    p = blocks._p
    w = q.weights
    c = CdxRollout(B=q.B, A=q.A, E=q.E, O=q.O, W=q.W, S=q.S, predict_noise=int(q.predict_noise), clip=int(q.clip),
                   w1=p(w[0]), b1=p(w[1]), w2=p(w[2]), b2=p(w[3]), w3=p(w[4]), b3=p(w[5]), wh=p(w[6]), bh=p(w[7]),
                   temb=p(q.temb), cond=p(q.cond), x_in=p(q.x_in), prior=p(q.prior), fix_mask=p(q.fix_mask), x_min=p(q.x_min),
                   x_max=p(q.x_max), noise=p(q.noise), steps=ctypes.cast(steps, ctypes.c_void_p),
                   X=p(q.X), P_raw=p(q.P_raw), feat=p(q.feat), Z=p(q.Z), H=p(q.H), g_out=p(q.g_out), G_head=p(q.G_head), g_x=p(q.g_x),
                   g_cond=p(q.g_cond), g_temb=p(q.g_temb))
    return c, steps


def native_forward(q) -> None:
    """``cdx_rollout_fwd_f32``: fills q.X, q.P_raw, q.feat, q.Z, q.H (one launch on the current stream)."""
    c, keep = _c_request(q)
    R._check(_lib().cdx_rollout_fwd_f32(ctypes.byref(c), R._stream_ptr(q.x_in.device)), "cdx_rollout_fwd_f32")
    del keep


def native_backward(q) -> None:
    """``cdx_rollout_bwd_f32``: q.Z <- d loss / d Z, fills q.G_head, q.g_temb and (when allocated) q.g_x, q.g_cond."""
    c, keep = _c_request(q)
    R._check(_lib().cdx_rollout_bwd_f32(ctypes.byref(c), R._stream_ptr(q.x_in.device)), "cdx_rollout_bwd_f32")
    del keep


# ------------------------------------------------------------------------------------------------------------------- #
# The same two passes in plain torch (any dtype, any device)                                                                  #
# ------------------------------------------------------------------------------------------------------------------- #
def _step_derivatives(st, predict_noise: bool):
    """(cx, cp): x' = cx * x + cp * P (+ noise) for the CLIPPED prediction P -- the affine update of ``_torch_step`` with eps and
    x_theta written out in (x, P)."""
    k0, k1, k2, k3, _ = st.k
    al, sg = st.alpha, st.sigma
    ex, ep = (0.0, 1.0) if predict_noise else (1.0 / sg, -al / sg)
    tx, tp = (1.0 / al, -sg / al) if predict_noise else (0.0, 1.0)
    ae = at = 0.0
    if st.kind == KIND_DDPM:
        ax, ae = k0, k2 - k0 * k1
    elif st.kind == KIND_DDIM:
        ax, ae = k0 / k2, k3 - k0 * k1 / k2
    else:
        ax = k0
        if st.vsel == V_XTHETA:
            at = -k1
        else:
            ae = -k1
    return ax + ae * ex + at * tx, ae * ep + at * tp


def reference_forward(q) -> None:
    """What ``cdx_rollout_fwd_f32`` computes, step by step, into the same buffers."""
    w1, b1, w2, b2, w3, b3, wh, bh = q.weights
    x = q.x_in
    q.X[0] = x
    for s, (st, ni) in enumerate(zip(q.steps, noise_index(q.steps))):
        cond = q.cond if q.cond is not None else x.new_zeros(q.B, q.O)
        feat = torch.cat([x, q.temb[s].expand(q.B, q.E), cond], -1)
        q.feat[s] = feat
        h = feat
        for l, (w, b) in enumerate(((w1, b1), (w2, b2), (w3, b3))):
            z = h @ w.t() + b
            h = z * torch.tanh(nn.functional.softplus(z))
            q.Z[l, s], q.H[l, s] = z, h
        p = h @ wh.t() + bh
        q.P_raw[s] = p
        x = reference_step(q, st, ni, x, p)
        q.X[s + 1] = x


def _mish_grad(z):
    t = torch.tanh(nn.functional.softplus(z))
    return t + z * (1. - t * t) * torch.sigmoid(z)


def reference_backward(q) -> None:
    """What ``cdx_rollout_bwd_f32`` computes from q.g_out and the saved buffers (explicit formulas, no autograd)."""
    w1, _, w2, _, w3, _, wh, _ = q.weights
    g = q.g_out
    if q.g_cond is not None:
        q.g_cond.zero_()
    for s in range(q.S - 1, -1, -1):
        st = q.steps[s]
        cx, cp = _step_derivatives(st, q.predict_noise)
        if q.fix_mask is not None:
            g = g * (1. - q.fix_mask)
        x, p = q.X[s], q.P_raw[s]
        lo, hi = _bounds(q, st, x)
        outside = torch.zeros_like(p, dtype=torch.bool)
        if lo is not None:
            outside = outside | (p < lo)
        if hi is not None:
            outside = outside | (p > hi)
        gp = g * cp
        gd = g * cx
        if q.predict_noise:
            gd = gd + torch.where(outside, gp / st.sigma, torch.zeros_like(gp))
        gp = torch.where(outside, torch.zeros_like(gp), gp)
        q.G_head[s] = gp
        gh = gp @ wh
        for l, w in ((2, w3), (1, w2), (0, None)):
            gz = gh * _mish_grad(q.Z[l, s])
            q.Z[l, s] = gz
            if w is not None:
                gh = gz @ w
        gf = q.Z[0, s] @ w1
        g = gd + gf[:, :q.A]
        q.g_temb[:, s * q.E:(s + 1) * q.E] = gf[:, q.A:q.A + q.E]
        if q.g_cond is not None:
            q.g_cond += gf[:, q.A + q.E:]
    if q.g_x is not None:
        q.g_x.copy_(g)


def reference_param_grads(q):
    """(dw1, db1, dw2, db2, dw3, db3, dwh, dbh) from the buffers a backward pass left: dW_l = sum_s G[l][s]^T H[l-1][s] (torch matmuls;
    the device path issues the same products through ``train._weight_grads``)."""
    out = []
    for p_rows, q_rows in _wgrad_operands(q):
        out += [p_rows.t() @ q_rows, p_rows.sum(0)]
    return tuple(out)


def _wgrad_operands(q):
    rows = q.S * q.B
    return ((q.Z[0].reshape(rows, q.W), q.feat.reshape(rows, -1)), (q.Z[1].reshape(rows, q.W), q.H[0].reshape(rows, q.W)),
            (q.Z[2].reshape(rows, q.W), q.H[1].reshape(rows, q.W)), (q.G_head.reshape(rows, q.A), q.H[2].reshape(rows, q.W)))


# ------------------------------------------------------------------------------------------------------------------- #
# The autograd node                                                                                                           #
# ------------------------------------------------------------------------------------------------------------------- #
class _Rollout(torch.autograd.Function):
    """x_S = rollout(x_T, cond, temb, noise; the eight parameters): forward and backward one launch each (+ the weight-gradient
    products).  `env` = (prior, fix_mask, x_min, x_max, steps, predict_noise, clip): no gradients."""

    @staticmethod
    def forward(ctx, x_t, cond, temb, noise, w1, b1, w2, b2, w3, b3, wh, bh, env):
        prior, fix_mask, x_min, x_max, steps, predict_noise, clip = env
        params = (w1, b1, w2, b2, w3, b3, wh, bh)
        q = make_request([p.detach() for p in params], temb.detach().contiguous(), None if cond is None else cond.detach().contiguous(),
                         x_t.detach().contiguous(), prior, fix_mask, x_min, x_max, noise, steps, predict_noise, clip)
        globals()["native_forward"](q)                       # (looked up per call: the CPU tests patch the two passes)
        ctx.q, ctx.params = q, params
        return q.X[q.S]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        q, params = ctx.q, ctx.params
        if q.G_head is not None:
            raise RuntimeError("the fused rollout keeps d loss / d Z in its saved buffers: it can be differentiated once")
        need = ctx.needs_input_grad
        kw = dict(device=g_out.device, dtype=g_out.dtype)
        q.g_out = g_out.contiguous()
        q.G_head = torch.empty(q.S, q.B, q.A, **kw)
        q.g_temb = torch.empty(q.B, q.S * q.E, **kw)
        q.g_x = torch.empty(q.B, q.A, **kw) if need[0] else None
        q.g_cond = torch.empty(q.B, q.O, **kw) if (q.cond is not None and need[1]) else None
        globals()["native_backward"](q)
        g_temb = blocks.colsum(q.g_temb).view(q.S, q.E) if need[2] else None
        grads = []
        rows = q.S * q.B
        for i, (p_rows, q_rows) in enumerate(_wgrad_operands(q)):
            w_param, b_param = params[2 * i], params[2 * i + 1]
            dw, db = train._weight_grads(p_rows, q_rows, rows, 1, 1, 1, 1, 0, w_param, b_param, need[4 + 2 * i], need[5 + 2 * i])
            grads += [dw, db]
        return (q.g_x, q.g_cond, g_temb, None, *grads, None)


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def _trunk(net):
    """(the three hidden Linears, the head) of a DQLMlp / DVInvMlp whose shape the kernels take, or None."""
    mid = list(getattr(net, "mid_layer", []))
    if len(mid) != 6 or not all(type(m) is nn.Linear and m.bias is not None for m in mid[0::2]) or \
            not all(type(m) is nn.Mish for m in mid[1::2]):
        return None
    l1, l2, l3 = mid[0::2]
    head = getattr(net, "final_layer", None)
    if type(head) is not nn.Linear or head.bias is None:
        return None
    w = l1.out_features
    if w % 16 or w > MAX_WIDTH or l1.in_features > MAX_FEATURES or head.out_features > MAX_X:
        return None
    if (l2.in_features, l2.out_features, l3.in_features, l3.out_features, head.in_features) != (w,) * 5:
        return None
    if not all(p.is_contiguous() for m in (l1, l2, l3, head) for p in (m.weight, m.bias)):
        return None
    return (l1, l2, l3), head


def time_table(net, plan, device) -> torch.Tensor:
    """``time_mlp(map_noise(t_s))`` for the S step records as an (S, E) tensor, under autograd on the library's Linear / Mish nodes:
    ``time_mlp``'s parameters get their gradients through it."""
    with train._weight_packs(net):
        return train._sequential(net.time_mlp, net.map_noise(R.device_times(plan, device)).contiguous())


def try_rollout(solver, model, plan, xt, prior, cond_vec, w_cfg, w_cg, feed) -> Optional[torch.Tensor]:
    """The state after the last step of `plan`, differentiable, or None: the host loop runs exactly as before (every None comes BEFORE
    the first draw from `feed`)."""
    if not (train.enabled() and enabled() and torch.is_grad_enabled()):
        return None
    if not (torch.is_tensor(xt) and xt.dim() == 2 and xt.is_cuda and xt.dtype == torch.float32 and xt.shape[0] > 0):
        return None
    net = model["diffusion"]
    use_cond = cond_vec is not None and w_cfg == 1.0
    if w_cfg not in (0.0, 1.0) or (w_cfg == 1.0 and cond_vec is None and type(net).__name__ != "DQLMlp"):
        return None                                       # (DVInvMlp without its condition: the host loop raises as the reference does)
    cond = torch.flatten(cond_vec, 1) if use_cond else None
    if not use_cond and type(net).__name__ == "DVInvMlp":
        return None
    fam = train.family_of(net, xt, cond)
    if fam is None or fam.name != "mlp":
        return None
    if not (w_cg == 0.0 or getattr(solver, "classifier", None) is None):
        return None
    steps = plan.steps
    if not step_admissible(steps, MAX_STEPS) or getattr(prior, "requires_grad", False):
        return None
    trunk = _trunk(net)
    b, a = xt.shape
    if trunk is None or trunk[1].out_features != a:
        return None
    (l1, l2, l3), head = trunk
    e = net.time_mlp[-1].out_features if isinstance(net.time_mlp, nn.Sequential) and isinstance(net.time_mlp[-1], nn.Linear) else -1
    o = l1.in_features - a - e
    if e <= 0 or o < 0 or (cond is not None and (cond.dtype != torch.float32 or not cond.is_cuda or tuple(cond.shape) != (b, o))):
        return None
    dev = xt.device
    env = solver_env(solver, plan, prior, b, a, dev, refuse_grad=True)
    if env is None:
        return None
    temb = time_table(net, plan, dev)
    noise = feed.many(xt, plan.n_noise)
    env = (*env[:4], steps, R._predicts_noise(plan, solver), env[4])
    return _Rollout.apply(xt, cond, temb, None if noise is None else R._f32c(noise.detach(), dev),
                          l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias, head.weight, head.bias, env)
