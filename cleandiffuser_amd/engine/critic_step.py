"""A critic's TD or expectile training step on ONE row-tile launch (``cdx_critic_step_f32``, csrc/cdx_critic_step.hip).

The dql / edp / idql / qgpo pipelines step a value critic on every gradient update: a frozen target evaluated without a gradient,
``y = rew + discount * (1 - done) * T``, an MSE or expectile loss of one tower or twin towers against y, backward.  With the towers on
one forward and one backward launch (engine/tower.py) that is still 80 to 150 device kernels, most of them the target's node chain, the
loss arithmetic and autograd's accumulations.  ``try_step`` runs the whole step as

1. the gradients zeroed in place (the optimiser's own ``zero_grad(set_to_none=False)``);
2. one ``cdx_critic_step_f32``: target, y, live forward, loss, backward-data (16 live rows of one live tower per workgroup);
3. one ``cdx_conv_wgrad_batch_f32`` for every weight and bias gradient, added into the ``.grad`` tensors;
4. one ``cdx_colsum_batch_f32`` for every gain and shift gradient, the loss and the mean of y.

The optimiser step stays the caller's: the gradients are where ``optim.step()`` reads them.  ``reference_step`` restates the launch in
plain torch on the same request object (any dtype, any device): what the CPU tests run in place of the C call and what the GPU tests
compare the buffers against in float64.  ``CDX_CRITIC_STEP=0`` keeps the eager sequence everywhere; which call sites take the fused step
without being asked (``CDX_CRITIC_STEP=1``) is DESIGN.md 3p."""
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn.functional as F

from . import blocks, tower, train
from . import runtime as R
from .energy import MAX_LDS
from .rowtile import ROWS, declare, r16

REDUCE = {"min": 0, "max": 1, "softmax": 2}            # CDX_CRITIC_MIN / MAX / SOFTMAX
LOSS = {"mse": 0, "expectile": 1}                      # CDX_CRITIC_MSE / EXPECTILE
MAX_K = 16                                             # CDX_CRITIC_MAX_K

_FP, _I, _F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
_PER_LAYER = _FP * tower.MAX_LAYERS * 2


class CdxCriticNet(ctypes.Structure):
    _fields_ = [("K0", _I), ("n_towers", _I), ("n_layers", _I), ("reserved", _I), ("width", _I * tower.MAX_LAYERS),
                ("norm", _I * tower.MAX_LAYERS), ("act", _I * tower.MAX_LAYERS), ("eps", _F * tower.MAX_LAYERS),
                ("w", _PER_LAYER), ("b", _PER_LAYER), ("gamma", _PER_LAYER), ("beta", _PER_LAYER)]


class CdxCriticStep(ctypes.Structure):
    _fields_ = [("R", _I), ("K", _I), ("A0", _I), ("A1", _I), ("B0", _I), ("B1", _I), ("reduce", _I), ("loss", _I),
                ("discount", _F), ("beta", _F), ("tau", _F), ("reserved", _I), ("live", CdxCriticNet), ("target", CdxCriticNet),
                ("x0", _FP), ("x1", _FP), ("z0", _FP), ("z1", _FP), ("rew", _FP), ("done", _FP), ("y_out", _FP), ("y_part", _FP),
                ("q_out", _FP * 2), ("loss_part", _FP * 2), ("x_cat", _FP), ("H", _FP * 2), ("G", _FP * 2), ("Sb", _FP * 2),
                ("Sg", _FP * 2)]


def _lib():
    return declare(R.load_library(), {"cdx_critic_step_lds_bytes": ([ctypes.POINTER(CdxCriticStep)], ctypes.c_longlong),
                                      "cdx_critic_step_f32": ([ctypes.POINTER(CdxCriticStep), ctypes.c_void_p], ctypes.c_int)})


def enabled(default: bool) -> bool:
    """``CDX_CRITIC_STEP=1``: every step the launch takes; ``CDX_CRITIC_STEP=0``: none; unset: the call sites that are fused by `default`
    (utils/critic_steps.py: where the measurement of DESIGN.md 3p decides it)."""
    asked = os.environ.get("CDX_CRITIC_STEP")
    return asked == "1" or (asked != "0" and default)


# ------------------------------------------------------------------------------------------------------------------- #
# Admission                                                                                                                   #
# ------------------------------------------------------------------------------------------------------------------- #
def describe(live_seqs, target_seqs):
    """(``tower.describe``'s answers of the live towers, of the target towers) for one or two Sequentials of one shape each whose last
    width is 1, or None."""
    out = []
    for seqs in (live_seqs, target_seqs):
        if len(seqs) not in (1, 2):
            return None
        descs = [tower.describe(s) for s in seqs]
        if any(d is None for d in descs) or any(tower.shape_of(d) != tower.shape_of(descs[0]) for d in descs[1:]):
            return None
        if descs[0].width[-1] != 1:
            return None
        out.append(descs)
    return tuple(out)


def lds_bytes(dl, dt) -> int:
    """The kernel's LDS plan (critic_plan of csrc/cdx_critic_step.hip; ``cdx_critic_step_lds_bytes``): two activation images
    [16][widest operand of both nets + 4], P_l [16][width[l]] and rstd_l [16] of every live layer, the target values [2][MAX_K][16],
    y / q / dq / l [4][16]."""
    ld = max(r16(w) for d in (dl, dt) for w in [d.K0] + list(d.width)) + 4
    return 4 * (2 * ROWS * ld + ROWS * sum(dl.width) + ROWS * len(dl.width) + 2 * MAX_K * ROWS + 4 * ROWS)


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object the kernel's binding and the torch restatement read and fill                                       #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(dl, live_weights, dt, target_weights, x0, x1, z0, z1, rew, done, *, group: int = 1, reduce: str = "min",
                 loss: str = "mse", discount: float = 1.0, beta: float = 0.0, tau: float = 0.5):
    """`dl` / `dt`: ``tower.describe``'s answer for the live / target towers' common shape; `live_weights` / `target_weights`: per tower
    ``tower.params_of`` as tensors; `x0` (R, A0), `x1` (R, A1) or None: the live rows ``[x0 | x1]``; `z0` (R, B0) or None, `z1`
    (R * group, B1) or None: the target rows ``[z0[r] | z1[r * group + j]]``; `rew`, `done` (R) or (R, 1), or both None (y = T).
    Allocates what the launch writes (the layout of include/cdx.h: cdx_critic_step): y (R), y_part (tiles), loss_part (towers, tiles),
    x_cat (R, K0) and, as ``q.live``, a ``tower`` request over x_cat whose out / H / G / Sb / Sg it fills (``q.live.P`` / ``.rstd`` are
    written by ``reference_step`` only: the kernel keeps them in LDS)."""
    rows = x0.shape[0]
    kw = dict(device=x0.device, dtype=x0.dtype)
    tiles = -(-rows // ROWS)
    q = SimpleNamespace(R=rows, K=int(group), reduce=reduce, loss=loss, discount=float(discount), beta=float(beta), tau=float(tau),
                        dl=dl, dt=dt, x0=x0, x1=x1, z0=z0, z1=z1, rew=rew, done=done, target_weights=target_weights, tiles=tiles,
                        A0=x0.shape[1], A1=0 if x1 is None else x1.shape[1], B0=0 if z0 is None else z0.shape[1],
                        B1=0 if z1 is None else z1.shape[1], y=torch.empty(rows, **kw), y_part=torch.empty(tiles, **kw),
                        loss_part=torch.empty(len(live_weights), tiles, **kw), x_cat=torch.empty(rows, dl.K0, **kw))
    q.live = tower.make_request(dl, live_weights, q.x_cat, save=True)
    tower.add_backward(q.live, [None] * len(live_weights), want_gx=False, want_params=True)
    return q


def shapes_ok(q) -> bool:
    """The sizes ``cdx_critic_step_f32`` refuses with CDX_EINVAL, and the operands' own shapes."""
    rows = q.R
    if not (1 <= q.K <= MAX_K and rows * q.K <= 0x7fffffff - ROWS and q.reduce in REDUCE and q.loss in LOSS):
        return False
    if (q.reduce == "min" and q.K != 1) or (q.K > 1 and q.B1 == 0) or q.A0 < 1:
        return False
    if q.A0 + q.A1 != q.dl.K0 or q.B0 + q.B1 != q.dt.K0 or (q.rew is None) != (q.done is None):
        return False
    for t, n, width in ((q.x0, rows, q.A0), (q.x1, rows, q.A1), (q.z0, rows, q.B0), (q.z1, rows * q.K, q.B1)):
        if t is not None and tuple(t.shape) != (n, width):
            return False
    if any(t is not None and t.numel() != rows for t in (q.rew, q.done)):
        return False
    return lds_bytes(q.dl, q.dt) <= MAX_LDS


def _c_net(d, weights) -> CdxCriticNet:
    p = blocks._p
    c = CdxCriticNet(K0=d.K0, n_towers=len(weights), n_layers=len(d.width))
    for l, w in enumerate(d.width):
        c.width[l], c.norm[l], c.act[l], c.eps[l] = w, int(d.norm[l]), d.act[l], d.eps[l]
    for t, ws in enumerate(weights):
        it = iter(ws)
        for l, has_norm in enumerate(d.norm):
            c.w[t][l], c.b[t][l] = p(next(it)), p(next(it))
            if has_norm:
                c.gamma[t][l], c.beta[t][l] = p(next(it)), p(next(it))
    return c


def _c_request(q) -> CdxCriticStep:
    p, lv = blocks._p, q.live
    live_weights = [[x for l in range(len(q.dl.width)) for x in ([lv.w[t][l], lv.b[t][l]] + ([lv.gamma[t][l], lv.beta[t][l]] if q.dl.norm[l] else []))]
                    for t in range(lv.n_towers)]
    c = CdxCriticStep(R=q.R, K=q.K, A0=q.A0, A1=q.A1, B0=q.B0, B1=q.B1, reduce=REDUCE[q.reduce], loss=LOSS[q.loss], discount=q.discount,
                      beta=q.beta, tau=q.tau, live=_c_net(q.dl, live_weights), target=_c_net(q.dt, q.target_weights), x0=p(q.x0), x1=p(q.x1),
                      z0=p(q.z0), z1=p(q.z1), rew=p(q.rew), done=p(q.done), y_out=p(q.y), y_part=p(q.y_part), x_cat=p(q.x_cat))
    for t in range(lv.n_towers):
        c.q_out[t], c.loss_part[t] = p(lv.out[t]), p(q.loss_part[t])
        c.H[t], c.G[t], c.Sb[t], c.Sg[t] = p(lv.H_buf[t]), p(lv.G_buf[t]), p(lv.S_buf[0][t]), p(lv.S_buf[1][t])
    return c


def native_step(q) -> None:
    """``cdx_critic_step_f32``: fills q.y, q.y_part, q.loss_part, q.x_cat and q.live.out / H / G / Sb / Sg (one launch on the current
    stream)."""
    c = _c_request(q)
    R._check(_lib().cdx_critic_step_f32(ctypes.byref(c), R._stream_ptr(q.x0.device)), "cdx_critic_step_f32")


# ------------------------------------------------------------------------------------------------------------------- #
# The same launch in plain torch (any dtype, any device)                                                                      #
# ------------------------------------------------------------------------------------------------------------------- #
def _tile_sums(q, v):
    """(tiles): the sums of the (R) vector `v` over the 16 rows of every tile."""
    return F.pad(v, (0, q.tiles * ROWS - q.R)).view(q.tiles, ROWS).sum(1)


def reference_target(q):
    """y (R) of the request: the target towers on ``[z0 | z1]``, the reduction over the towers and the group, the TD expression."""
    parts = ([q.z0.repeat_interleave(q.K, 0)] if q.z0 is not None else []) + ([q.z1] if q.z1 is not None else [])
    tq = tower.make_request(q.dt, q.target_weights, torch.cat(parts, 1), save=False)
    tower.reference_forward(tq)
    vals = [o.view(q.R, q.K) for o in tq.out]
    if q.reduce == "softmax":
        qm = vals[0] if len(vals) == 1 else torch.min(vals[0], vals[1])
        T = (torch.softmax(q.beta * qm, 1) * qm).sum(1)
    else:
        tops = [v.max(1)[0] for v in vals]
        T = tops[0] if len(tops) == 1 else torch.min(tops[0], tops[1])
    if q.rew is None:
        return T
    return q.rew.reshape(-1) + q.discount * (1 - q.done.reshape(-1)) * T


def reference_step(q) -> None:
    """What ``cdx_critic_step_f32`` computes, into the same buffers (and q.live.P / q.live.rstd, which the kernel keeps in LDS)."""
    lv = q.live
    y = reference_target(q)
    q.y.copy_(y)
    q.y_part.copy_(_tile_sums(q, y) / q.R)
    q.x_cat.copy_(q.x0 if q.x1 is None else torch.cat([q.x0, q.x1], 1))
    tower.reference_forward(lv)
    for t in range(lv.n_towers):
        out = lv.out[t][:, 0]
        if q.loss == "expectile":
            adv = y - out
            w = torch.abs(q.tau - (adv < 0).to(y.dtype))
            per_row, dq = w * adv ** 2, -2 * w * adv / q.R
        else:
            e = out - y
            per_row, dq = e ** 2, 2 * e / q.R
        q.loss_part[t].copy_(_tile_sums(q, per_row) / q.R)
        lv.g_out[t] = dq[:, None]
    tower.reference_backward(lv)


def loss_of(q):
    """The step's loss and the mean of y from the partial sums (0-d)."""
    return q.loss_part.sum(), q.y_part.sum()


def reference_param_grads(q, t: int) -> list:
    """The gradient of every parameter of live tower `t` from the launch's buffers, in the order of ``tower.params_of``."""
    return tower.reference_param_grads(q.live, t)


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def _on_device(x, params) -> bool:
    """A ROCm device and contiguous throughout?  (Looked up per call: the CPU tests patch it.)"""
    return x.is_cuda and all(p.device == x.device and p.is_contiguous() for p in params)


def _takes_in_place(p) -> bool:
    """May a kernel add p's gradient into ``p.grad`` (``train._grad_slot``'s conditions, asked before anything is written)?"""
    if not isinstance(p, torch.nn.Parameter) or not p.is_leaf or not p.requires_grad or p._backward_hooks or \
            getattr(p, "_post_accumulate_grad_hooks", None):
        return False
    g = p.grad
    return g is None or (g.dtype == torch.float32 and g.shape == p.shape and g.device == p.device and g.is_contiguous()
                         and not g.requires_grad)


def try_step(live_seqs, target_seqs, optim, x0, x1, z0, z1, rew, done, *, group: int = 1, reduce: str = "min", loss: str = "mse",
             discount: float = 1.0, beta: float = 0.0, tau: float = 0.5, default: bool = False) -> Optional[dict]:
    """One critic step up to, not including, ``optim.step()``: the gradients of `optim`'s parameters zeroed in place, then the loss's
    gradient of every parameter of the live towers in its ``.grad`` -> {"loss", "target_mean"} as 0-d device tensors (no host
    synchronisation), or None: the caller's eager sequence runs exactly as before (every None comes BEFORE anything is written).
    `optim`: any torch optimiser (or None: the live parameters' gradients alone are zeroed).  No clipping.  `default`: does this call
    site take the launch without being asked (``enabled``)?"""
    if not (enabled(default) and train.enabled()) or not torch.is_grad_enabled():
        return None
    if os.environ.get("CDX_TRAIN_INPLACE_GRADS", "1") == "0" or train._reducer_may_listen():
        return None
    inputs = [t for t in (x0, x1, z0, z1, rew, done) if t is not None]
    if x0 is None or not all(torch.is_tensor(t) and t.dtype == torch.float32 and not t.requires_grad for t in inputs):
        return None
    if x0.dim() != 2 or x0.shape[0] == 0 or any(t.dim() != 2 for t in (x1, z0, z1) if t is not None):
        return None
    descs = describe(live_seqs, target_seqs)
    if descs is None:
        return None
    dls, dts = descs
    live = [p for d in dls for p in tower.params_of(d)]
    frozen = [p for d in dts for p in tower.params_of(d)]
    if any(p.dtype != torch.float32 for p in live + frozen) or not all(globals()["_takes_in_place"](p) for p in live):
        return None
    if not globals()["_on_device"](x0, live + frozen) or any(t.device != x0.device for t in inputs):
        return None
    q = make_request(dls[0], [[p.detach() for p in tower.params_of(d)] for d in dls], dts[0],
                     [[p.detach() for p in tower.params_of(d)] for d in dts],
                     *[None if t is None else t.detach().contiguous() for t in (x0, x1, z0, z1, rew, done)],
                     group=group, reduce=reduce, loss=loss, discount=discount, beta=beta, tau=tau)
    if not shapes_ok(q):
        return None
    # -- from here on the step is taken --
    covered = set()
    if optim is not None:
        optim.zero_grad(set_to_none=False)
        covered = {id(p) for grp in optim.param_groups for p in grp["params"]}
    with torch.no_grad(), train.grads_in_place(live):
        for p in live:
            if id(p) not in covered and p.grad is not None:
                p.grad.zero_()
        slots = [train._grad_slot(p) for p in live]
        assert all(s is not None for s in slots), "a parameter admitted by _takes_in_place has no gradient slot"
        globals()["native_step"](q)
        lv, stats = q.live, torch.zeros(2, device=x0.device, dtype=torch.float32)
        wjobs, cjobs, i = [], [(q.loss_part.view(-1, 1), stats[0:1]), (q.y_part.view(-1, 1), stats[1:2])], 0
        for t in range(lv.n_towers):
            for l, (p_rows, q_rows, rows) in enumerate(tower.wgrad_operands(lv, t)):
                wjobs.append((p_rows, q_rows, rows, slots[i], slots[i + 1]))
                i += 2
                if lv.norm[l]:
                    cjobs += [(lv.Sg[t][l], slots[i]), (lv.Sb[t][l], slots[i + 1])]
                    i += 2
        globals()["weight_sums"](wjobs)
        globals()["column_sums"](cjobs)
        train._written(*slots)
    return {"loss": stats[0], "target_mean": stats[1]}


def weight_sums(jobs) -> None:
    tower.weight_sums(jobs)


def column_sums(jobs) -> int:
    return tower.column_sums(jobs)
