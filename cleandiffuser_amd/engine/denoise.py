"""The denoising loss of the row-MLP denoisers (DQLMlp / DVInvMlp) on one forward and one backward launch.

Diffusion-QL and EDP call ``bc_loss = actor.loss(act, obs)`` on every gradient step (reference pipelines/dql_d4rl_*.py,
edp_d4rl_mujoco.py:97) and EDP evaluates the net once more on a noised action (edp_d4rl_mujoco.py:100-108); both are combined with the Q
term and back-propagated by the pipeline, never through ``update()``.  On the library's per-layer nodes (``train.dql_forward``) that is
one launch per Linear / Mish of ``time_mlp``, the trunk and the head, ATen for the noise add, the concat and the weighted square, and
the mirror image in backward.  Here one evaluation is ONE ``torch.autograd.Function``:

* forward  = ``cdx_denoise_fwd_f32`` (csrc/cdx_denoise.hip): noise add, time MLP, features, trunk, head and, in loss mode, the tiles'
  shares of the loss, for a 16-row tile per workgroup; saves Zt, Ht, feat, Z, H, pred;
* backward = ``cdx_denoise_bwd_f32``: d loss / d pred, the head, the trunk and the time MLP transposed, d loss / d Z written over Z, then
  one ``cdx_conv_wgrad_f32`` product per layer (``train._weight_grads``: in place / queued inside ``grads_in_place()``, handed to
  autograd outside).

``try_loss`` serves ``BaseDiffusionSDE.loss``, ``try_predict`` the module call of ``utils.policy_steps.approx_action``.
``reference_forward`` / ``reference_backward`` restate the two kernels in plain torch on the same request (explicit backward formulas,
no autograd): what the CPU tests run in place of the two C calls and what the GPU tests compare the buffers against.  ``CDX_DENOISE=0``
keeps the per-layer nodes, ``CDX_DENOISE=1`` asks for the launches; which one an unset variable means is DESIGN.md 3q.
"""
import contextlib
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import blocks, train
from . import runtime as R
from .energy import MAX_LDS
from .rollout import MAX_FEATURES, MAX_X, _mish_grad, _trunk
from .rowtile import ALD, ROWS, declare, r16

MAX_TIME_HIDDEN = 512      # 2 E: the hidden layer of time_mlp is an MFMA A operand like a trunk layer
DEFAULT_ON = True          # what an unset CDX_DENOISE means: the fused node beat the per-layer route by the rule of DESIGN.md 3q

_FP, _I = ctypes.c_void_p, ctypes.c_int32
_WEIGHTS = ("tw1", "tb1", "tw2", "tb2", "w1", "b1", "w2", "b2", "w3", "b3", "wh", "bh")


class CdxDenoise(ctypes.Structure):
    _fields_ = [("R", _I), ("A", _I), ("E", _I), ("O", _I), ("W", _I), ("predict_noise", _I), ("loss_mode", _I), ("reserved", _I)] + \
               [(n, _FP) for n in _WEIGHTS] + \
               [(n, _FP) for n in ("xt", "x0", "eps", "a", "s", "emb0", "cond", "fix_mask", "lw", "wr", "Zt", "Ht", "feat", "Z", "H", "pred",
                                   "loss_part", "g_loss", "g_pred", "G_head", "G_t2", "g_xt", "g_cond", "g_emb0")]


def _lib():
    proto = ([ctypes.POINTER(CdxDenoise), ctypes.c_void_p], ctypes.c_int)
    return declare(R.load_library(), {"cdx_denoise_lds_bytes": ([ctypes.POINTER(CdxDenoise)], ctypes.c_longlong),
                                      "cdx_denoise_fwd_f32": proto, "cdx_denoise_bwd_f32": proto})


def enabled() -> bool:
    """``CDX_DENOISE=1``: every evaluation the launches take; ``CDX_DENOISE=0``: none; unset: ``DEFAULT_ON``."""
    asked = os.environ.get("CDX_DENOISE")
    return asked == "1" or (asked != "0" and DEFAULT_ON)


def lds_bytes(a: int, e: int, o: int, w: int) -> int:
    """The kernels' LDS plan (dn_lds of csrc/cdx_denoise.hip; ``cdx_denoise_lds_bytes``): two activation images [16][widest A operand +
    4] and one (16 x A) tile [16][68]."""
    ld = max(r16(a + e + o), w, r16(2 * e)) + 4
    return 4 * (2 * ROWS * ld + ROWS * ALD)


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object both the kernels' binding and the torch restatement read and fill                                 #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(weights, emb0, cond, *, xt=None, x0=None, eps=None, a=None, s=None, fix_mask=None, lw=None, wr=None,
                 predict_noise: bool = False, loss_mode: bool = True):
    """`weights` = (tw1, tb1, tw2, tb2, w1, b1, w2, b2, w3, b3, wh, bh); `emb0` (R, E); `cond` (R, O) or None; `xt` (R, A) (given-input
    mode) or `x0`, `eps` (R, A) and `a`, `s` (R); `fix_mask`, `lw` (A) or None; `wr` (R) or None.  Allocates the saved-tensor buffers (the
    layout of include/cdx.h: cdx_denoise)."""
    rows, e = emb0.shape
    w, f = weights[4].shape
    act = weights[10].shape[0]
    kw = dict(device=emb0.device, dtype=emb0.dtype)
    tiles = -(-rows // ROWS)
    return SimpleNamespace(
        R=rows, A=act, E=e, O=f - act - e, W=w, tiles=tiles, weights=tuple(weights), emb0=emb0, cond=cond, xt=xt, x0=x0, eps=eps, a=a, s=s,
        fix_mask=fix_mask, lw=lw, wr=wr, predict_noise=bool(predict_noise), loss_mode=bool(loss_mode),
        Zt=torch.empty(rows, 2 * e, **kw), Ht=torch.empty(rows, 2 * e, **kw), feat=torch.empty(rows, f, **kw),
        Z=torch.empty(3, rows, w, **kw), H=torch.empty(3, rows, w, **kw), pred=torch.empty(rows, act, **kw),
        loss_part=torch.empty(tiles, **kw) if loss_mode else None,
        g_loss=None, g_pred=None, G_head=None, G_t2=None, g_xt=None, g_cond=None, g_emb0=None)


def _c_request(q) -> CdxDenoise:
    p = blocks._p
    c = CdxDenoise(R=q.R, A=q.A, E=q.E, O=q.O, W=q.W, predict_noise=int(q.predict_noise), loss_mode=int(q.loss_mode))
    for n, t in zip(_WEIGHTS, q.weights):
        setattr(c, n, p(t))
    for n in ("xt", "x0", "eps", "a", "s", "emb0", "cond", "fix_mask", "lw", "wr", "Zt", "Ht", "feat", "Z", "H", "pred", "loss_part",
              "g_loss", "g_pred", "G_head", "G_t2", "g_xt", "g_cond", "g_emb0"):
        setattr(c, n, p(getattr(q, n)))
    return c


def native_forward(q) -> None:
    """``cdx_denoise_fwd_f32``: fills q.Zt, q.Ht, q.feat, q.Z, q.H, q.pred and q.loss_part (one launch on the current stream)."""
    c = _c_request(q)
    R._check(_lib().cdx_denoise_fwd_f32(ctypes.byref(c), R._stream_ptr(q.emb0.device)), "cdx_denoise_fwd_f32")


def native_backward(q) -> None:
    """``cdx_denoise_bwd_f32``: q.Z <- d loss / d Z, q.Zt <- d loss / d Zt, fills q.G_head, q.G_t2 and (when allocated) q.g_xt, q.g_cond,
    q.g_emb0."""
    c = _c_request(q)
    R._check(_lib().cdx_denoise_bwd_f32(ctypes.byref(c), R._stream_ptr(q.emb0.device)), "cdx_denoise_bwd_f32")


# ------------------------------------------------------------------------------------------------------------------- #
# The same two passes in plain torch (any dtype, any device)                                                                  #
# ------------------------------------------------------------------------------------------------------------------- #
def _mish(z):
    return z * torch.tanh(F.softplus(z))


def _target(q):
    return q.eps if q.predict_noise else q.x0


def _element_weight(q):
    """(R, A): lw (1 - m) wr."""
    w = q.pred.new_ones(q.R, q.A)
    if q.lw is not None:
        w = w * q.lw
    if q.fix_mask is not None:
        w = w * (1. - q.fix_mask)
    if q.wr is not None:
        w = w * q.wr[:, None]
    return w


def reference_forward(q) -> None:
    """What ``cdx_denoise_fwd_f32`` computes, into the same buffers."""
    tw1, tb1, tw2, tb2, w1, b1, w2, b2, w3, b3, wh, bh = q.weights
    if q.xt is not None:
        xt = q.xt
    else:
        xt = q.a[:, None] * q.x0 + q.s[:, None] * q.eps
        if q.fix_mask is not None:
            xt = (1. - q.fix_mask) * xt + q.fix_mask * q.x0
    zt = q.emb0 @ tw1.t() + tb1
    ht = _mish(zt)
    q.Zt.copy_(zt)
    q.Ht.copy_(ht)
    cond = q.cond if q.cond is not None else xt.new_zeros(q.R, q.O)
    h = torch.cat([xt, ht @ tw2.t() + tb2, cond], -1)
    q.feat.copy_(h)
    for l, (w, b) in enumerate(((w1, b1), (w2, b2), (w3, b3))):
        z = h @ w.t() + b
        h = _mish(z)
        q.Z[l], q.H[l] = z, h
    q.pred.copy_(h @ wh.t() + bh)
    if q.loss_mode:
        per = ((q.pred - _target(q)) ** 2 * _element_weight(q)).reshape(-1)
        per = F.pad(per, (0, (q.tiles * ROWS - q.R) * q.A))
        q.loss_part.copy_(per.view(q.tiles, ROWS * q.A).sum(1) / (q.R * q.A))


def reference_backward(q) -> None:
    """What ``cdx_denoise_bwd_f32`` computes from q.g_loss / q.g_pred and the saved buffers (explicit formulas, no autograd)."""
    tw1, _, tw2, _, w1, _, w2, _, w3, _, wh, _ = q.weights
    if q.loss_mode:
        gp = q.g_loss * 2. * (q.pred - _target(q)) * _element_weight(q) / (q.R * q.A)
    else:
        gp = q.g_pred
    q.G_head.copy_(gp)
    gh = gp @ wh
    for l, w in ((2, w3), (1, w2), (0, None)):
        gz = gh * _mish_grad(q.Z[l])
        q.Z[l] = gz
        if w is not None:
            gh = gz @ w
    gf = q.Z[0] @ w1
    q.G_t2.copy_(gf[:, q.A:q.A + q.E])
    if q.g_xt is not None:
        q.g_xt.copy_(gf[:, :q.A])
    if q.g_cond is not None:
        q.g_cond.copy_(gf[:, q.A + q.E:])
    gt = (q.G_t2 @ tw2) * _mish_grad(q.Zt)
    q.Zt.copy_(gt)
    if q.g_emb0 is not None:
        q.g_emb0.copy_(gt @ tw1)


def _wgrad_operands(q):
    return ((q.Zt, q.emb0), (q.G_t2, q.Ht), (q.Z[0], q.feat), (q.Z[1], q.H[0]), (q.Z[2], q.H[1]), (q.G_head, q.H[2]))


def reference_param_grads(q):
    """(dtw1, dtb1, dtw2, dtb2, dw1, db1, dw2, db2, dw3, db3, dwh, dbh) from the buffers a backward pass left (torch matmuls; the device
    path issues the same products through ``train._weight_grads``)."""
    out = []
    for p_rows, q_rows in _wgrad_operands(q):
        out += [p_rows.t() @ q_rows, p_rows.sum(0)]
    return tuple(out)


def loss_of(q):
    """The loss from the tiles' shares (0-d)."""
    return q.loss_part.sum()


# ------------------------------------------------------------------------------------------------------------------- #
# The autograd node                                                                                                           #
# ------------------------------------------------------------------------------------------------------------------- #
class _Denoise(torch.autograd.Function):
    """loss = denoise(x0, eps, a, s, emb0, cond; the twelve parameters) or, in prediction mode, pred = denoise(xt, ., ., ., emb0, cond;
    ...): forward and backward one launch each (+ the weight-gradient products).  `env` = (loss_mode, predict_noise, fix_mask, lw, wr):
    no gradients."""

    @staticmethod
    def forward(ctx, x, eps, a, s, emb0, cond, tw1, tb1, tw2, tb2, w1, b1, w2, b2, w3, b3, wh, bh, env):
        loss_mode, predict_noise, fix_mask, lw, wr = env
        params = (tw1, tb1, tw2, tb2, w1, b1, w2, b2, w3, b3, wh, bh)
        x = x.detach().contiguous()
        noise = dict(x0=x, eps=eps.detach().contiguous(), a=a.detach().contiguous(), s=s.detach().contiguous()) if loss_mode else dict(xt=x)
        q = make_request([p.detach() for p in params], emb0.detach().contiguous(), None if cond is None else cond.detach().contiguous(),
                         fix_mask=fix_mask, lw=lw, wr=wr, predict_noise=predict_noise, loss_mode=loss_mode, **noise)
        globals()["native_forward"](q)                       # (looked up per call: the CPU tests patch the two passes)
        ctx.q, ctx.params = q, params
        return loss_of(q) if loss_mode else q.pred

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        q, params = ctx.q, ctx.params
        if q.G_head is not None:
            raise RuntimeError("the fused denoising step keeps d loss / d Z in its saved buffers: it can be differentiated once")
        need = ctx.needs_input_grad
        kw = dict(device=g_out.device, dtype=g_out.dtype)
        if q.loss_mode:
            q.g_loss = g_out.reshape(1).contiguous()
        else:
            q.g_pred = g_out.contiguous()
        q.G_head, q.G_t2 = torch.empty(q.R, q.A, **kw), torch.empty(q.R, q.E, **kw)
        q.g_xt = torch.empty(q.R, q.A, **kw) if (need[0] and not q.loss_mode) else None
        q.g_emb0 = torch.empty(q.R, q.E, **kw) if need[4] else None
        q.g_cond = torch.empty(q.R, q.O, **kw) if (q.cond is not None and need[5]) else None
        globals()["native_backward"](q)
        grads = []
        for i, (p_rows, q_rows) in enumerate(_wgrad_operands(q)):
            w_param, b_param = params[2 * i], params[2 * i + 1]
            dw, db = train._weight_grads(p_rows, q_rows, q.R, 1, 1, 1, 1, 0, w_param, b_param, need[6 + 2 * i], need[7 + 2 * i])
            grads += [dw, db]
        return (q.g_xt, None, None, None, q.g_emb0, q.g_cond, *grads, None)


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
_inside_update = [0]


@contextlib.contextmanager
def inside_update():
    """The scope of ``DiffusionModel._loss_backward``: ``update()`` keeps its own route (the captured HIP graph or the eager pair over
    ``train.dql_forward``), so ``try_loss`` declines while it is open."""
    _inside_update[0] += 1
    try:
        yield
    finally:
        _inside_update[0] -= 1


def _net_spec(net, a: int):
    """(the twelve parameters, E, O) of a DQLMlp / DVInvMlp the kernels take for (., `a`) rows, or None."""
    trunk = _trunk(net)
    tm = getattr(net, "time_mlp", None)
    if trunk is None or not isinstance(tm, nn.Sequential) or len(tm) != 3 or not callable(getattr(net, "map_noise", None)):
        return None
    (l1, l2, l3), head = trunk
    t1, act, t2 = tm
    if type(t1) is not nn.Linear or type(act) is not nn.Mish or type(t2) is not nn.Linear or t1.bias is None or t2.bias is None:
        return None
    e = t1.in_features
    if (t1.out_features, t2.in_features, t2.out_features) != (2 * e, 2 * e, e) or 2 * e > MAX_TIME_HIDDEN:
        return None
    o = l1.in_features - a - e
    if head.out_features != a or a > MAX_X or o < 0 or l1.in_features > MAX_FEATURES or o != getattr(net, "obs_dim", o):
        return None
    params = tuple(p for m in (t1, t2, l1, l2, l3, head) for p in (m.weight, m.bias))
    if not all(p.is_contiguous() and p.dtype == torch.float32 and p.is_cuda for p in params):
        return None
    if lds_bytes(a, e, o, l1.out_features) > MAX_LDS:
        return None
    return params, e, o


def _rows_ok(x) -> bool:
    return torch.is_tensor(x) and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and x.shape[0] > 0


def _flat(v, a: int, dev):
    """A reference-style (1, A) / (A,) / scalar mask or weight as a dense (A,) table (None: absent); raises ValueError for what the
    kernels do not take (per-sample tables, one that takes a gradient)."""
    t = R._dense_hd(v, 1, a, dev)
    if t is not None and t.requires_grad:
        raise ValueError("a mask or weight that takes a gradient")
    return None if t is None else t.detach().reshape(-1).contiguous()


def _cond_fits(cond, b: int, o: int, net) -> bool:
    if cond is None:
        return type(net).__name__ == "DQLMlp"            # (DVInvMlp without its condition: the module raises as the reference does)
    return _rows_ok(cond) and tuple(cond.shape) == (b, o)


def try_loss(agent, x0, condition, kwargs) -> Optional[torch.Tensor]:
    """``agent.loss(x0, condition, **kwargs)`` (0-d, differentiable) on the two launches, or None: the caller's own sequence runs exactly
    as before (every None comes BEFORE anything is drawn or written)."""
    if not (enabled() and train.enabled() and torch.is_grad_enabled()) or _inside_update[0]:
        return None
    if not _rows_ok(x0) or x0.requires_grad:
        return None
    from ..diffusion import diffusionsde as sde
    if type(agent).add_noise not in (sde.DiscreteDiffusionSDE.add_noise, sde.ContinuousDiffusionSDE.add_noise):
        return None
    net = agent.model["diffusion"]
    b, a = x0.shape
    spec = _net_spec(net, a)
    if spec is None:
        return None
    params, e, o = spec
    if condition is None:
        if not _cond_fits(None, b, o, net):
            return None
    elif not (torch.is_tensor(condition) and condition.is_cuda and condition.dtype == torch.float32 and condition.shape[0] == b):
        return None
    wr = kwargs.get("weighted_regression_tensor", None)
    if wr is not None and not (torch.is_tensor(wr) and wr.is_cuda and wr.dtype == torch.float32 and tuple(wr.shape) == (b,)
                               and not wr.requires_grad):
        return None
    try:
        fix_mask, lw = _flat(agent.fix_mask, a, x0.device), _flat(agent.loss_weight, a, x0.device)
    except (ValueError, RuntimeError):
        return None
    if not (any(p.requires_grad for p in agent.model.parameters()) or (condition is not None and condition.requires_grad)):
        return None                                       # nothing to differentiate
    if torch.cuda.is_current_stream_capturing():
        return None
    # -- from here on the step is taken: the draws of add_noise, in its order, then the condition encoder as a module --
    t, eps = agent._noise_draws(x0)
    cond = agent.model["condition"](condition) if condition is not None else None
    emb0 = net.map_noise(t)
    if not (_cond_fits(cond, b, o, net) and _rows_ok(emb0) and tuple(emb0.shape) == (b, e) and _rows_ok(eps)):
        return agent._loss_of(x0, *agent.add_noise(x0, t, eps), cond, kwargs)      # (an encoder of another shape: the stock expression)
    alpha, sigma = agent._alpha_sigma_rows(t)
    env = (True, bool(agent.predict_noise), fix_mask, lw, None if wr is None else wr.detach().contiguous())
    return _Denoise.apply(x0, eps, R._f32c(alpha, x0.device), R._f32c(sigma, x0.device), emb0, cond, *params, env)


def try_predict(net, xt, t, cond) -> Optional[torch.Tensor]:
    """``net(xt, t, cond)`` (differentiable) on the two launches, or None: the module call runs exactly as before."""
    if not (enabled() and train.enabled() and torch.is_grad_enabled()) or _inside_update[0]:
        return None
    if not _rows_ok(xt) or not torch.is_tensor(t):
        return None
    b, a = xt.shape
    spec = _net_spec(net, a)
    if spec is None or not _cond_fits(cond, b, spec[2], net):
        return None
    params, e, _ = spec
    if not (xt.requires_grad or (cond is not None and cond.requires_grad) or any(p.requires_grad for p in net.parameters())):
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    emb0 = net.map_noise(t)
    if not (_rows_ok(emb0) and tuple(emb0.shape) == (b, e)):
        return None
    return _Denoise.apply(xt, None, None, None, emb0, cond, *params, (False, False, None, None, None))
