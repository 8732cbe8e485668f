"""QGPO's contrastive energy training step on one row-tile launch (``cdx_cep_step_f32``, csrc/cdx_cep.hip).

The energy model of QGPO is trained by ``clf.update(noisy_act, t, {"soft_label", "obs"})`` once per gradient step (reference
pipelines/qgpo_d4rl_mujoco.py:172-212): 256 states x K = 16 support actions through ``QGPONNClassifier`` (3 x 256 SiLU MLP), the loss a
cross entropy between the soft labels and the softmax of the energies over the K actions of a state.  As ATen autograd that is about a
hundred launches and five host synchronisations.  ``try_cep_update`` runs the same update as

1. ``map_noise(t)`` on the B states (ATen; the reference embeds the repeated (B, K) tensor),
2. ``optim.zero_grad()`` in place,
3. ONE ``cdx_cep_step_f32``: forward, loss and backward-data of the R = B K rows, 16 rows (16 / K whole softmax groups) per workgroup,
4. one ``cdx_colsum_f32`` over the (B, 4) per-state scalars -- read by ONE device-to-host copy at the end,
5. one ``cdx_conv_wgrad_batch_f32``: every weight gradient, the bias sums out of the same launch, added into the ``.grad`` tensors,
6. ``FusedAdam.step(max_norm=, ema=)``: clip, Adam and the EMA copy.

``reference_step`` restates the kernel in plain torch on the same request object (any dtype, any device): what the CPU tests run in place
of the C call and what the GPU tests compare the buffers against.  ``CDX_CEP=0`` keeps the autograd body of ``QGPOClassifier.update``.
"""
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import blocks, train
from . import runtime as R
from .energy import MAX_EMB, MAX_HIDDEN, MAX_LDS, MAX_OBS, MAX_WIDTH, MAX_X  # noqa: F401  (the limits of the one energy model)
from .energy import _silu_grad, classifier_lds, classifier_within_limits, describe_classifier as describe, energy_model
from .rowtile import ALD, ROWS, declare, on_device

GROUPS = (1, 2, 4, 8, 16)                              # K: a 16-row tile holds whole softmax groups
_SC = 64                                               # CEP_SC of the kernel

_FP, _I = ctypes.c_void_p, ctypes.c_int32


class CdxCepStep(ctypes.Structure):
    _fields_ = [("B", _I), ("K", _I), ("A", _I), ("O", _I), ("Ec", _I), ("n_hidden", _I), ("hidden", _I * MAX_HIDDEN),
                ("x", _FP), ("obs", _FP), ("temb", _FP), ("soft", _FP), ("obs_w", _FP), ("obs_b", _FP), ("act_w", _FP), ("act_b", _FP),
                ("w", _FP * MAX_HIDDEN), ("b", _FP * MAX_HIDDEN), ("wo", _FP), ("bo", _FP),
                ("feat", _FP), ("H", _FP), ("G", _FP), ("G_out", _FP), ("G_act", _FP), ("G_obs", _FP), ("stats", _FP)]


def _lib():
    return declare(R.load_library(), {"cdx_cep_lds_bytes": ([ctypes.POINTER(CdxCepStep)], ctypes.c_longlong),
                                      "cdx_cep_step_f32": ([ctypes.POINTER(CdxCepStep), ctypes.c_void_p], ctypes.c_int)})


def enabled() -> bool:
    return os.environ.get("CDX_CEP", "1") != "0"


# ------------------------------------------------------------------------------------------------------------------- #
# The net as the kernel reads it: ``describe`` = ``energy.describe_classifier``                                               #
# ------------------------------------------------------------------------------------------------------------------- #
def weights_of(desc):
    """[obs_w, obs_b, act_w, act_b, w_0, b_0, ..., w_o, b_o]: the parameters themselves."""
    return [p for lin in desc.lins for p in (lin.weight, lin.bias)]


def lds_bytes(desc) -> int:
    """The kernel's LDS plan (cep_plan of csrc/cdx_cep.hip; ``cdx_cep_lds_bytes``)."""
    maxw, pre = classifier_lds(desc)
    return 4 * (2 * ROWS * (maxw + 4) + pre + ROWS * ALD + _SC)


def within_limits(desc, k: int) -> bool:
    """The limits ``cdx_cep_step_f32`` refuses with CDX_EINVAL."""
    return k in GROUPS and classifier_within_limits(desc, desc.A) and lds_bytes(desc) <= MAX_LDS


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object the kernel's binding and the torch restatement read and fill                                       #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(weights, x, obs, temb, soft, k: int):
    """`weights` = [obs_w, obs_b, act_w, act_b, w_0, b_0, ..., w_o, b_o]; `x` (B K, A); `obs` (B, O); `temb` (B, Ec); `soft` (B K,).
    Allocates what the step writes (the layout of include/cdx.h: cdx_cep_step): feat, H / G (layer-major; ``q.H[l]`` / ``q.G[l]`` are
    the (R, hidden[l]) matrices), G_out, G_act, G_obs, stats."""
    b, o = obs.shape
    rows, a = x.shape
    ec = temb.shape[1]
    hidden = [w.shape[0] for w in weights[4:-2:2]]
    kw = dict(device=x.device, dtype=x.dtype)
    h_buf, g_buf = torch.empty(rows * sum(hidden), **kw), torch.empty(rows * sum(hidden), **kw)
    cuts = [rows * sum(hidden[:l]) for l in range(len(hidden) + 1)]
    layer = lambda buf: [buf[cuts[l]:cuts[l + 1]].view(rows, w) for l, w in enumerate(hidden)]        # noqa: E731
    return SimpleNamespace(B=b, K=k, A=a, O=o, Ec=ec, hidden=hidden, weights=list(weights), x=x, obs=obs, temb=temb, soft=soft,
                           feat=torch.empty(rows, 3 * ec, **kw), H_buf=h_buf, G_buf=g_buf, H=layer(h_buf), G=layer(g_buf),
                           G_out=torch.empty(rows, **kw), G_act=torch.empty(rows, ec, **kw), G_obs=torch.empty(b, ec, **kw),
                           stats=torch.empty(b, 4, **kw))


def _c_request(q) -> CdxCepStep:
    p = blocks._p
    w = q.weights
    c = CdxCepStep(B=q.B, K=q.K, A=q.A, O=q.O, Ec=q.Ec, n_hidden=len(q.hidden), x=p(q.x), obs=p(q.obs), temb=p(q.temb), soft=p(q.soft),
                   obs_w=p(w[0]), obs_b=p(w[1]), act_w=p(w[2]), act_b=p(w[3]), wo=p(w[-2]), bo=p(w[-1]), feat=p(q.feat), H=p(q.H_buf),
                   G=p(q.G_buf), G_out=p(q.G_out), G_act=p(q.G_act), G_obs=p(q.G_obs), stats=p(q.stats))
    for l, width in enumerate(q.hidden):
        c.hidden[l], c.w[l], c.b[l] = width, p(w[4 + 2 * l]), p(w[5 + 2 * l])
    return c


def native_step(q) -> None:
    """``cdx_cep_step_f32``: fills q.feat, q.H, q.G, q.G_out, q.G_act, q.G_obs and q.stats (one launch on the current stream)."""
    c = _c_request(q)
    R._check(_lib().cdx_cep_step_f32(ctypes.byref(c), R._stream_ptr(q.x.device)), "cdx_cep_step_f32")


def wgrad_operands(q):
    """(p, q, rows) of the weight-gradient product of every Linear, in the order of ``weights_of``: dW = p^T q, db = the column sums of p."""
    rows = q.B * q.K
    inputs = [q.feat] + q.H
    return ([(q.G_obs, q.obs, q.B), (q.G_act, q.x, rows)] + [(g, h, rows) for g, h in zip(q.G, inputs)]
            + [(q.G_out.view(rows, 1), q.H[-1], rows)])


def scalars(sums, b: int, k: int):
    """(loss, f_max, f_min, f_mean) from the column sums of q.stats."""
    return sums[0] / b, sums[1] / b, sums[2] / b, sums[3] / (b * k)


# ------------------------------------------------------------------------------------------------------------------- #
# The same step in plain torch (any dtype, any device)                                                                        #
# ------------------------------------------------------------------------------------------------------------------- #
def reference_step(q) -> SimpleNamespace:
    """What ``cdx_cep_step_f32`` computes, into the same buffers (explicit backward formulas, no autograd) -> the four scalars and the
    gradient of every parameter (the products the device path hands to ``cdx_conv_wgrad_batch_f32``), in the order of ``weights_of``."""
    w = q.weights
    b, k = q.B, q.K
    rep = lambda t: t.repeat_interleave(k, 0)                                             # noqa: E731   (row r = state r // K)
    q.feat.copy_(torch.cat([rep(q.obs @ w[0].t() + w[1]), q.x @ w[2].t() + w[3], rep(q.temb)], -1))
    f, dt, pres = energy_model(q.feat, w[4:-2:2], w[5:-2:2], w[-2], w[-1])
    for l, pre in enumerate(pres):
        q.H[l].copy_(nn.functional.silu(pre))
    f, y = f.view(b, k), q.soft.view(b, k)
    lse = torch.logsumexp(f, 1, keepdim=True)
    q.stats.copy_(torch.stack([-(y * (f - lse)).sum(1), f.max(1)[0], f.min(1)[0], f.sum(1)], 1))
    g_f = (torch.softmax(f, 1) * y.sum(1, keepdim=True) - y) / b
    q.G_out.copy_(g_f.reshape(-1) * dt[:, 0])
    g = q.G_out[:, None] * w[-2] * _silu_grad(pres[-1])
    for l in range(len(q.hidden) - 1, -1, -1):
        q.G[l].copy_(g)
        g = q.G[l] @ w[4 + 2 * l]
        if l:
            g = g * _silu_grad(pres[l - 1])
    q.G_obs.copy_(g[:, :q.Ec].reshape(b, k, q.Ec).sum(1))
    q.G_act.copy_(g[:, q.Ec:2 * q.Ec])
    loss, f_max, f_min, f_mean = scalars(q.stats.sum(0), b, k)
    grads = []
    for p_rows, q_rows, _ in wgrad_operands(q):
        grads += [p_rows.t() @ q_rows, p_rows.sum(0)]
    return SimpleNamespace(loss=loss, f_max=f_max, f_min=f_min, f_mean=f_mean, grads=grads)


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def _fused_optimiser(opt) -> bool:
    from .optim import FusedAdam
    return isinstance(opt, FusedAdam) and opt.native()


def _takes_grads_in_place(params) -> bool:
    """Would ``train._grad_slot`` hand out every parameter's ``.grad``?  (Asked BEFORE anything is written: the slot itself creates a
    missing gradient tensor.)"""
    if os.environ.get("CDX_TRAIN_INPLACE_GRADS", "1") == "0" or train._reducer_may_listen():
        return False
    for p in params:
        if not isinstance(p, nn.Parameter) or not p.is_leaf or not p.requires_grad or p.dtype != torch.float32 or not p.is_contiguous() \
                or p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
            return False
        g = p.grad
        if g is not None and (g.dtype != torch.float32 or g.shape != p.shape or g.device != p.device or not g.is_contiguous() or g.requires_grad):
            return False
    return True


def try_cep_update(clf, x, t, y, update_ema: bool = True) -> Optional[dict]:
    """The whole ``QGPOClassifier.update`` -> {"loss", "f_max", "f_mean", "f_min", "grad_norm"}, or None: the autograd body runs exactly
    as before (every None comes BEFORE anything is written)."""
    from ..classifier.qgpo_classifier import QGPOClassifier
    from ..nn_classifier.mlp import QGPONNClassifier
    from ..utils.embeddings import UntrainableFourierEmbedding
    if not (enabled() and train.enabled() and torch.is_grad_enabled()):
        return None
    if not (torch.is_tensor(x) and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32 and x.shape[0] > 0):
        return None
    b, k, a = x.shape
    if k not in GROUPS:
        return None
    if type(clf) is not QGPOClassifier or type(clf.model) is not QGPONNClassifier:
        return None
    net = clf.model
    emb = net.map_noise
    if type(emb) is not UntrainableFourierEmbedding:
        return None                                       # (the others carry parameters or do not take the (b, K) tensor of the reference)
    desc = describe(net)
    if desc is None or desc.A != a or 2 * emb.freqs.numel() != desc.Ec or not within_limits(desc, k):
        return None
    params = weights_of(desc)
    if not all(p.requires_grad and p.is_cuda for p in params) or not _takes_grads_in_place(params):
        return None
    if not _fused_optimiser(clf.optim):
        return None
    if not isinstance(y, dict) or not on_device(y.get("soft_label"), (b, k, 1)) or not on_device(y.get("obs"), (b, desc.O)):
        return None
    if not (torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == (b,)):
        return None
    if any(v.requires_grad for v in (x, t, y["soft_label"], y["obs"])):
        return None                                       # (the autograd body would hand these inputs their gradients too)
    dev, opt, rows = x.device, clf.optim, b * k
    with torch.no_grad():
        temb = R._f32c(emb(t), dev)
        opt.zero_grad()
        q = make_request([p.detach() for p in params], R._f32c(x.detach(), dev).view(rows, a), R._f32c(y["obs"].detach(), dev), temb,
                         R._f32c(y["soft_label"].detach(), dev).view(rows), k)
        globals()["native_step"](q)                          # (looked up per call: the CPU tests patch it)
        sums = blocks.colsum(q.stats)
        with train.grads_in_place(params):
            slots = [train._grad_slot(p) for p in params]
            assert all(s is not None for s in slots)
            blocks.conv_wgrad_batch([(p_rows, q_rows, n, 1, 1, 1, 1, 0, slots[2 * i], slots[2 * i + 1])
                                     for i, (p_rows, q_rows, n) in enumerate(wgrad_operands(q))])
            train._written(*slots)
        clip = clf.grad_clip_norm if isinstance(clf.grad_clip_norm, float) else None
        opt.step(max_norm=clip, ema=(clf.model, clf.model_ema, clf.ema_rate) if update_ema else None)
        loss, f_max, f_min, f_mean = (float(v) for v in scalars(sums.cpu(), b, k))
        grad_norm = float(opt.last_grad_norm) if clip else None
    return {"f_max": f_max, "f_mean": f_mean, "f_min": f_min, "loss": loss, "grad_norm": grad_norm}
