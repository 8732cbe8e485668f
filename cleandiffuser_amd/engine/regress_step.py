"""A supervised MSE training step of one tower against a GIVEN target on ONE row-tile launch (``cdx_regress_step_f32``,
csrc/cdx_regress_step.hip).

Decision Diffuser and Decision Veteran step an inverse-dynamics head on every gradient update (``MlpInvDynamic.update``), SfBC re-trains
a critic by the same step: rows ``[x0 | x1]`` through a Linear / activation tower, ``mean((out - y) ** 2)``, backward.  As library nodes
(``train.chain_forward``) that is a ``torch.cat``, one launch per Linear and activation forward, the loss arithmetic and about twice
that backward.  ``try_step`` runs the whole step as

1. the gradients zeroed in place (the optimiser's own ``zero_grad(set_to_none=False)``);
2. one ``cdx_regress_step_f32``: load, forward, loss, backward-data (16 rows per workgroup);
3. one ``cdx_conv_wgrad_batch_f32`` for every weight and bias gradient, added into the ``.grad`` tensors;
4. one ``cdx_colsum_batch_f32`` for every gain and shift gradient and the loss.

The optimiser step stays the caller's.  x0, x1 and y are read in place where they are rows of one stride or the ``[:, :-1]`` /
``[:, 1:]`` views of a (B, H, D) batch (``row_map``); anything else is copied.  ``reference_step`` restates the launch in plain torch on
the same request object (any dtype, any device): what the CPU tests run in place of the C call and what the GPU tests compare the buffers
against in float64.  ``CDX_REGRESS_STEP=0`` keeps the eager sequence everywhere; which call sites take the fused step without being asked
(``CDX_REGRESS_STEP=1``) is DESIGN.md 3r."""
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn.functional as F

from . import blocks, tower, train
from . import runtime as R
from .critic_step import CdxCriticNet, _c_net, _takes_in_place
from .energy import MAX_LDS, MAX_WIDTH, MAX_X
from .rowtile import ROWS, declare, r16

TILE_LD = 64                                           # RO_XLD: the row stride of the out / e^2 tile
_FP, _I = ctypes.c_void_p, ctypes.c_int32
_I32_MAX = 0x7fffffff


class CdxRegressRows(ctypes.Structure):
    _fields_ = [("ptr", _FP), ("width", _I), ("ld", _I), ("inner", _I), ("period", _I)]


class CdxRegressStep(ctypes.Structure):
    _fields_ = [("R", _I), ("reserved", _I), ("net", CdxCriticNet), ("x0", CdxRegressRows), ("x1", CdxRegressRows), ("y", CdxRegressRows),
                ("out", _FP), ("loss_part", _FP), ("x_cat", _FP), ("H", _FP), ("G", _FP), ("Sb", _FP), ("Sg", _FP)]


def _lib():
    return declare(R.load_library(), {"cdx_regress_step_lds_bytes": ([ctypes.POINTER(CdxRegressStep)], ctypes.c_longlong),
                                      "cdx_regress_step_f32": ([ctypes.POINTER(CdxRegressStep), ctypes.c_void_p], ctypes.c_int)})


def enabled(default: bool) -> bool:
    """``CDX_REGRESS_STEP=1``: every step the launch takes; ``CDX_REGRESS_STEP=0``: none; unset: the call sites that are fused by
    `default` (utils/regression_steps.py: where the measurement of DESIGN.md 3r decides it)."""
    asked = os.environ.get("CDX_REGRESS_STEP")
    return asked == "1" or (asked != "0" and default)


# ------------------------------------------------------------------------------------------------------------------- #
# Admission                                                                                                                   #
# ------------------------------------------------------------------------------------------------------------------- #
def describe(seq):
    """``tower.describe``'s answer for a Sequential of ``Linear -> [LayerNorm] -> [activation]`` layers whose last width is 1 .. 64, or
    None: a module the kernels do not know (GELU, an active ``nn.Dropout``), a hidden width off a multiple of 16, sizes over the limits."""
    return tower.describe(seq)


def lds_bytes(d) -> int:
    """The kernel's LDS plan (regress_plan of csrc/cdx_regress_step.hip; ``cdx_regress_step_lds_bytes``): two activation images
    [16][widest of K0 and the widths + 4], P_l [16][width[l]] and rstd_l [16] of every layer, the out / e^2 tile [16][64]."""
    ld = max(r16(w) for w in [d.K0] + list(d.width)) + 4
    return 4 * (2 * ROWS * ld + ROWS * sum(d.width) + ROWS * len(d.width) + ROWS * TILE_LD)


# ------------------------------------------------------------------------------------------------------------------- #
# The operands: rows read where they live                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def row_map(t):
    """(inner, period, ld) under which the kernel reads the rows of `t` in place -- row r of ``t.reshape(-1, t.shape[-1])`` starts at
    float ``((r // inner) * period + r % inner) * ld`` of ``t.data_ptr()`` -- or None: `t` has to be copied.  2-D (R, W) of strides
    (s, 1): (1, 1, s).  3-D (B, n, W) of strides (S, s, 1) with S a whole multiple of s and blocks that do not overlap: (n, S // s, s)
    (``obs[:, :-1]`` of a contiguous (B, H, D) batch: (H - 1, H, D))."""
    if t.dim() not in (2, 3) or t.numel() == 0:
        return None
    width = t.shape[-1]
    if width > 1 and t.stride(-1) != 1:
        return None
    s = t.stride(-2) if t.shape[-2] > 1 else width        # (the stride of a dimension of one element says nothing)
    if s < width or s > _I32_MAX:
        return None
    if t.dim() == 2:
        return 1, 1, s
    n = t.shape[1]
    if t.shape[0] == 1:
        return n, n, s
    S = t.stride(0)
    if S % s or S // s < n or S // s > _I32_MAX:
        return None
    return n, S // s, s


def _operand(t):
    """`t` as the kernel reads it: (the tensor -- itself or a contiguous copy --, (inner, period, ld))."""
    m = row_map(t)
    if m is None:
        t = t.contiguous()
        m = row_map(t)
    return t, m


def _rows(t):
    """The (R, W) matrix behind an operand (a copy where the view cannot be flattened): what the torch restatement reads."""
    return t.reshape(-1, t.shape[-1])


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object the kernel's binding and the torch restatement read and fill                                       #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(d, weights, x0, x1, y):
    """`d`: ``describe``'s answer; `weights`: ``tower.params_of`` as tensors; `x0` (.., A0), `x1` (.., A1) or None: the rows ``[x0 | x1]``;
    `y` (.., W): the target -- 2-D, or 3-D with the leading two dimensions being rows.  Allocates what the launch writes (the layout of
    include/cdx.h: cdx_regress_step): loss_part (tiles), x_cat (R, K0) and, as ``q.live``, a ``tower`` request over x_cat whose out / H /
    G / Sb / Sg it fills (``q.live.P`` / ``.rstd`` are written by ``reference_step`` only: the kernel keeps them in LDS)."""
    rows = x0.numel() // x0.shape[-1] if x0.shape[-1] else 0
    kw = dict(device=x0.device, dtype=x0.dtype)
    tiles = -(-rows // ROWS)
    q = SimpleNamespace(R=rows, d=d, tiles=tiles, A0=x0.shape[-1], A1=0 if x1 is None else x1.shape[-1], W=y.shape[-1],
                        x1=None, map1=None, loss_part=torch.empty(tiles, **kw), x_cat=torch.empty(rows, d.K0, **kw))
    q.x0, q.map0 = _operand(x0) if rows else (x0, None)
    q.y, q.map_y = _operand(y) if y.numel() else (y, None)
    if x1 is not None:
        q.x1, q.map1 = _operand(x1) if x1.numel() else (x1, None)
    q.live = tower.make_request(d, [weights], q.x_cat, save=True)
    tower.add_backward(q.live, [None], want_gx=False, want_params=True)
    return q


def shapes_ok(q) -> bool:
    """The sizes ``cdx_regress_step_f32`` refuses with CDX_EINVAL, and the operands' own shapes."""
    d = q.d
    if not (0 <= q.R <= _I32_MAX - ROWS and 1 <= d.K0 <= MAX_WIDTH and 1 <= d.width[-1] <= MAX_X):
        return False
    if q.A0 < 1 or q.A0 + q.A1 != d.K0 or q.W != d.width[-1]:
        return False
    for t, m in ((q.x0, q.map0), (q.x1, q.map1), (q.y, q.map_y)):
        if t is None:
            continue
        if t.numel() != q.R * t.shape[-1]:
            return False
        if q.R and t.shape[-1] and (m is None or m[0] < 1 or m[1] < m[0] or m[2] < 1):
            return False
    return lds_bytes(d) <= MAX_LDS


def _c_rows(t, m) -> CdxRegressRows:
    if t is None or m is None:
        return CdxRegressRows(width=0 if t is None else t.shape[-1])
    return CdxRegressRows(ptr=t.data_ptr(), width=t.shape[-1], ld=m[2], inner=m[0], period=m[1])


def _c_request(q) -> CdxRegressStep:
    p, lv, d = blocks._p, q.live, q.d
    ws = [x for l in range(len(d.width)) for x in ([lv.w[0][l], lv.b[0][l]] + ([lv.gamma[0][l], lv.beta[0][l]] if d.norm[l] else []))]
    return CdxRegressStep(R=q.R, net=_c_net(d, [ws]), x0=_c_rows(q.x0, q.map0), x1=_c_rows(q.x1, q.map1), y=_c_rows(q.y, q.map_y),
                          out=p(lv.out[0]), loss_part=p(q.loss_part), x_cat=p(q.x_cat), H=p(lv.H_buf[0]), G=p(lv.G_buf[0]),
                          Sb=p(lv.S_buf[0][0]), Sg=p(lv.S_buf[1][0]))


def native_step(q) -> None:
    """``cdx_regress_step_f32``: fills q.loss_part, q.x_cat and q.live.out / H / G / Sb / Sg (one launch on the current stream)."""
    c = _c_request(q)
    R._check(_lib().cdx_regress_step_f32(ctypes.byref(c), R._stream_ptr(q.x0.device)), "cdx_regress_step_f32")


# ------------------------------------------------------------------------------------------------------------------- #
# The same launch in plain torch (any dtype, any device)                                                                      #
# ------------------------------------------------------------------------------------------------------------------- #
def reference_step(q) -> None:
    """What ``cdx_regress_step_f32`` computes, into the same buffers (and q.live.P / q.live.rstd, which the kernel keeps in LDS)."""
    lv = q.live
    q.x_cat.copy_(_rows(q.x0) if q.x1 is None else torch.cat([_rows(q.x0), _rows(q.x1)], 1))
    tower.reference_forward(lv)
    e = lv.out[0] - _rows(q.y)
    n = q.R * q.W
    q.loss_part.copy_(F.pad((e ** 2).sum(1), (0, q.tiles * ROWS - q.R)).view(q.tiles, ROWS).sum(1) / n)
    lv.g_out[0] = 2 * e / n
    tower.reference_backward(lv)


def loss_of(q):
    """The step's loss from the partial sums (0-d)."""
    return q.loss_part.sum()


def reference_param_grads(q) -> list:
    """The gradient of every parameter from the launch's buffers, in the order of ``tower.params_of``."""
    return tower.reference_param_grads(q.live, 0)


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def _on_device(x, params) -> bool:
    """A ROCm device and contiguous throughout?  (Looked up per call: the CPU tests patch it.)"""
    return x.is_cuda and all(p.device == x.device and p.is_contiguous() for p in params)


def _capturing(x) -> bool:
    """Is a HIP graph being captured on x's device?  (The step allocates its buffers per call: not for a capture.)"""
    return x.is_cuda and torch.cuda.is_current_stream_capturing()


def try_step(seq, optim, x0, x1, y, *, default: bool = False) -> Optional[dict]:
    """One MSE step of `seq` on the rows ``[x0 | x1]`` against `y` up to, not including, ``optim.step()``: the gradients of `optim`'s
    parameters zeroed in place, then the gradient of ``mean((seq(cat) - y) ** 2)`` of every parameter of `seq` in its ``.grad`` ->
    {"loss"} as a 0-d device tensor (no host synchronisation), or None: the caller's eager sequence runs exactly as before (every None
    comes BEFORE anything is written).  `x0`, `x1` (or None), `y`: 2-D, or 3-D with the leading two dimensions being rows (views of a
    batch tensor are read in place, ``row_map``).  `optim`: any torch optimiser (or None: the parameters' gradients alone are zeroed).
    `default`: does this call site take the launch without being asked (``enabled``)?"""
    if not (enabled(default) and train.enabled()) or not torch.is_grad_enabled():
        return None
    if os.environ.get("CDX_TRAIN_INPLACE_GRADS", "1") == "0" or train._reducer_may_listen():
        return None
    inputs = [t for t in (x0, x1, y) if t is not None]
    if x0 is None or y is None or not all(torch.is_tensor(t) and t.dtype == torch.float32 and not t.requires_grad for t in inputs):
        return None
    if x0.dim() not in (2, 3) or x0.numel() == 0 or any(t.dim() != x0.dim() or t.shape[:-1] != x0.shape[:-1] for t in inputs):
        return None
    d = describe(seq)
    if d is None:
        return None
    params = tower.params_of(d)
    if any(p.dtype != torch.float32 for p in params) or not all(globals()["_takes_in_place"](p) for p in params):
        return None
    if not globals()["_on_device"](x0, params) or any(t.device != x0.device for t in inputs) or globals()["_capturing"](x0):
        return None
    q = make_request(d, [p.detach() for p in params], x0.detach(), None if x1 is None else x1.detach(), y.detach())
    if not shapes_ok(q):
        return None
    # -- from here on the step is taken --
    covered = set()
    if optim is not None:
        covered = {id(p) for grp in optim.param_groups for p in grp["params"]}
        # an optimiser that also holds parameters this step does not write (the other members of an ensemble) must see them without a
        # gradient, as the eager sequence's ``zero_grad()`` leaves them: it skips them.  (FusedAdam zeroes in place either way.)
        optim.zero_grad(set_to_none=not covered <= {id(p) for p in params})
    with torch.no_grad(), train.grads_in_place(params):
        for p in params:
            if id(p) not in covered and p.grad is not None:
                p.grad.zero_()
        slots = [train._grad_slot(p) for p in params]
        assert all(s is not None for s in slots), "a parameter admitted by _takes_in_place has no gradient slot"
        globals()["native_step"](q)
        lv, loss = q.live, torch.zeros(1, device=x0.device, dtype=torch.float32)
        wjobs, cjobs, i = [], [(q.loss_part.view(-1, 1), loss)], 0
        for l, (p_rows, q_rows, rows) in enumerate(tower.wgrad_operands(lv, 0)):
            wjobs.append((p_rows, q_rows, rows, slots[i], slots[i + 1]))
            i += 2
            if lv.norm[l]:
                cjobs += [(lv.Sg[0][l], slots[i]), (lv.Sb[0][l], slots[i + 1])]
                i += 2
        globals()["weight_sums"](wjobs)
        globals()["column_sums"](cjobs)
        train._written(*slots)
    return {"loss": loss[0]}


def weight_sums(jobs) -> None:
    tower.weight_sums(jobs)


def column_sums(jobs) -> int:
    return tower.column_sums(jobs)
