"""QGPO's energy-guided sampling loop in one launch (``cdx_energy_guided_run``, csrc/cdx_energy.hip).

QGPO's evaluation samples ``actor.sample(prior, solver, n_samples, sample_steps, condition_cfg=obs, w_cfg=1.0, condition_cg=obs, w_cg=w)``
once per environment step (reference pipelines/qgpo_d4rl_mujoco.py:244-249): an ``SfBCUNet`` denoiser under a diffusion SDE with a
``QGPOClassifier(QGPONNClassifier)`` energy model on 50-800 rows of actions.  Stepped on the host (``_run_plan_torch``) every denoising step is
the denoiser forward, the ~20 launches of ``mlp_grad.gradients`` and ATen's shift / clip / update / mask kernels.  Here the whole loop and
the final ``log_p`` are ONE kernel: one workgroup per 16 rows, both nets' activations in LDS.  What does not depend on the row is a table
made before the launch on the library's GEMM: ``den_c`` = ``t_layer(map_noise(t_s))`` (S, E) and ``clf_temb`` = the classifier's
``map_noise(t_s)`` with a last row for t = 0 (S + 1, Ec), kept in the plan's memo under the nets' weight signatures.

``reference_run`` restates the kernel in plain torch on the same request object (any dtype, any device): what the CPU tests run in place of
the C call and what the GPU tests compare the traces against.  ``CDX_ENERGY=0`` keeps the host loop.
"""
import ctypes
import functools
import os
import weakref
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import blocks, mlp_grad
from . import runtime as R
from .rowtile import ALD, ROWS, XLD, declare, noise_index, on_device, r16, reference_step, solver_env, step_admissible

MAX_STEPS, MAX_BLOCKS, MAX_HIDDEN = 64, 8, 4          # CDX_ENERGY_MAX_*
MAX_WIDTH, MAX_CONCAT, MAX_X, MAX_EMB, MAX_OBS = 512, 1024, 64, 128, 512
MAX_LDS = 160 * 1024

_FP, _I = ctypes.c_void_p, ctypes.c_int32


class CdxEnergyBlock(ctypes.Structure):
    _fields_ = [("in_", _I), ("in2", _I), ("out", _I), ("reserved", _I), ("w1", _FP), ("b1", _FP), ("w2", _FP), ("b2", _FP),
                ("wc", _FP), ("bc", _FP), ("ws", _FP), ("bs", _FP)]


class CdxEnergyGuided(ctypes.Structure):
    _fields_ = [("B", _I), ("A", _I), ("E", _I), ("O", _I), ("S", _I), ("Ec", _I), ("n_blocks", _I), ("n_down", _I), ("n_hidden", _I),
                ("predict_noise", _I), ("clip", _I), ("hidden", _I * MAX_HIDDEN),
                ("blocks", ctypes.POINTER(CdxEnergyBlock)), ("out_w", _FP), ("out_b", _FP), ("den_c", _FP), ("cond", _FP), ("obs", _FP),
                ("obs_w", _FP), ("obs_b", _FP), ("act_w", _FP), ("act_b", _FP), ("act_wt", _FP),
                ("clf_w", _FP * MAX_HIDDEN), ("clf_b", _FP * MAX_HIDDEN), ("clf_wt", _FP * MAX_HIDDEN), ("clf_wo", _FP), ("clf_bo", _FP),
                ("clf_temb", _FP), ("steps", ctypes.POINTER(R.CdxStep)), ("cg_scale", ctypes.POINTER(ctypes.c_float)),
                ("x_in", _FP), ("prior", _FP), ("fix_mask", _FP), ("x_min", _FP), ("x_max", _FP), ("noise", _FP),
                ("x_out", _FP), ("logp_out", _FP), ("trace_pred", _FP), ("trace_grad", _FP), ("trace_logp", _FP)]


def _lib():
    return declare(R.load_library(), {"cdx_energy_guided_lds_bytes": ([ctypes.POINTER(CdxEnergyGuided)], ctypes.c_longlong),
                                      "cdx_energy_guided_run": ([ctypes.POINTER(CdxEnergyGuided), ctypes.c_void_p], ctypes.c_int)})


def enabled() -> bool:
    return os.environ.get("CDX_ENERGY", "1") != "0"


# ------------------------------------------------------------------------------------------------------------------- #
# The two nets as the kernel reads them                                                                                       #
# ------------------------------------------------------------------------------------------------------------------- #
def describe_denoiser(net) -> Optional[SimpleNamespace]:
    """SfBCUNet -> the block table of ``cdx_energy_guided`` (detached parameters, no copies), or None for a tree that is not the
    reference's: rows {in_, in2, out, w1, b1, w2, b2, wc, bc, ws, bs}, n_down, out_w, out_b, A, E."""
    down, up = list(net.down_blocks), list(net.up_blocks)
    rows, kept, cur = [], [], net.out_layer.out_features
    for i, blk in enumerate(down + [net.mid_block] + up):
        lins = [getattr(blk, "linear1", [None])[0], getattr(blk, "linear2", [None])[0], getattr(blk, "linearc", None)]
        if not all(type(m) is nn.Linear and m.bias is not None for m in lins) or not (type(blk.linear1[1]) is nn.SiLU and type(blk.linear2[1]) is nn.SiLU):
            return None
        l1, l2, lc = lins
        in2 = kept.pop() if i > len(down) and kept else 0
        out = l1.out_features
        if l1.in_features != cur + in2 or (l2.in_features, l2.out_features, lc.out_features) != (out, out, out):
            return None
        if type(blk.skip) is nn.Linear and blk.skip.bias is not None and (blk.skip.in_features, blk.skip.out_features) == (cur + in2, out):
            ws, bs = blk.skip.weight.detach(), blk.skip.bias.detach()
        elif type(blk.skip) is nn.Identity and cur + in2 == out:
            ws = bs = None
        else:
            return None
        rows.append(SimpleNamespace(in_=cur, in2=in2, out=out, w1=l1.weight.detach(), b1=l1.bias.detach(), w2=l2.weight.detach(),
                                    b2=l2.bias.detach(), wc=lc.weight.detach(), bc=lc.bias.detach(), ws=ws, bs=bs))
        if i < len(down):
            kept.append(out)
        cur = out
    if type(net.out_layer) is not nn.Linear or net.out_layer.bias is None or net.out_layer.in_features != cur:
        return None
    emb = rows[0].wc.shape[1]
    if any(r.wc.shape[1] != emb for r in rows):
        return None
    return SimpleNamespace(rows=rows, n_down=len(down), out_w=net.out_layer.weight.detach(), out_b=net.out_layer.bias.detach(),
                           A=net.out_layer.out_features, E=emb)


class _Classifier(SimpleNamespace):
    """What ``describe_classifier`` returns.  The transposed operands of the guided kernel's backward are copies, made when first read
    (the guided route keeps the description per weight version, see ``_bound``; the training step never reads them): `wt[0]` = the
    act_proj columns [Ec, 2 Ec) of w[0] transposed (Ec, hidden[0]), `wt[l]` = w[l] transposed, `act_wt`."""

    @functools.cached_property
    def wt(self):
        return [self.w[0][:, self.Ec:2 * self.Ec].t().contiguous()] + [m.t().contiguous() for m in self.w[1:]]

    @functools.cached_property
    def act_wt(self):
        return self.act_w.t().contiguous()


def describe_classifier(net) -> Optional[_Classifier]:
    """QGPONNClassifier -> its sizes, its Linears in the order of the training request's weights (`lins`: obs_proj, act_proj, the hidden
    layers, the head) and their detached parameters as the guided request names them, or None unless the mlp is SiLU hidden layers and an
    identity output to one scalar, every layer a plain nn.Linear with a bias whose input is the width before it."""
    layers = mlp_grad._mlp_layers(net.mlp)
    if layers is None or len(layers) < 2 or any(act != "silu" for _, act in layers[:-1]) or layers[-1][1] != "none":
        return None
    lins = [net.obs_proj, net.act_proj] + [lin for lin, _ in layers]
    if any(type(m) is not nn.Linear or m.bias is None for m in lins):
        return None
    ec = net.act_proj.out_features
    hidden, last = lins[2:-1], lins[-1]
    widths = [ec * 3] + [lin.out_features for lin in hidden]
    if net.obs_proj.out_features != ec or last.out_features != 1 or [lin.in_features for lin in hidden + [last]] != widths:
        return None
    return _Classifier(Ec=ec, O=net.obs_proj.in_features, A=net.act_proj.in_features, hidden=widths[1:], lins=lins,
                       w=[lin.weight.detach() for lin in hidden], b=[lin.bias.detach() for lin in hidden], wo=last.weight.detach(),
                       bo=last.bias.detach(), obs_w=net.obs_proj.weight.detach(), obs_b=net.obs_proj.bias.detach(),
                       act_w=net.act_proj.weight.detach(), act_b=net.act_proj.bias.detach())


def _tensors(desc):
    """Every tensor of a description (the kernel reads them as dense fp32)."""
    out = []
    for v in vars(desc).values():
        for item in (v if isinstance(v, list) else [v]):
            out += _tensors(item) if isinstance(item, SimpleNamespace) else [item] if torch.is_tensor(item) else []
    return out


_cache = weakref.WeakKeyDictionary()


def _bound(net, make):
    """`make()` once per weight version of `net` (the transposes of the backward are copies) and per module tree (an activation swapped
    in place moves no weight)."""
    sig = (R._signature(net), tuple(type(m) for m in net.modules()))
    hit = _cache.get(net)
    if hit is None or hit[0] != sig:
        hit = (sig, make())
        _cache[net] = hit
    return hit[1]


def classifier_lds(clf):
    """(the widest MFMA operand, the floats of the saved pre-activations) of the energy model: em_plan of csrc/cdx_energy_mlp.h."""
    return max([r16(clf.O), r16(3 * clf.Ec)] + list(clf.hidden)), sum(ROWS * w for w in clf.hidden)


def classifier_within_limits(clf, a: int) -> bool:
    """The sizes of the energy model em_plan refuses, for states of width `a`."""
    return (1 <= len(clf.hidden) <= MAX_HIDDEN and all(w % 16 == 0 and 0 < w <= MAX_WIDTH for w in clf.hidden)
            and 0 < a <= MAX_X and 0 < clf.Ec <= MAX_EMB and 0 < clf.O <= MAX_OBS)


def lds_bytes(den, clf) -> int:
    """The kernel's LDS plan (en_plan of csrc/cdx_energy.hip; ``cdx_energy_guided_lds_bytes``)."""
    clf_w, pre = classifier_lds(clf)
    img = ROWS * (max([clf_w] + [r.out for r in den.rows]) + 4)
    pops = sum(r.in2 > 0 for r in den.rows)
    stack = sum(ROWS * (r.out + 4) for r in den.rows[den.n_down - pops:den.n_down])
    region = max(3 * img + stack, 2 * img + pre)
    return 4 * (region + ROWS * (r16(den.E) + 4) + ROWS * ALD + 2 * ROWS * XLD + ROWS * r16(clf.Ec) + 2 * ROWS)


def within_limits(den, clf, n_steps: int) -> bool:
    """The limits ``cdx_energy_guided_run`` refuses with CDX_EINVAL."""
    return (classifier_within_limits(clf, den.A) and all(r.out % 16 == 0 and r.out <= MAX_WIDTH for r in den.rows)
            and all(r.in_ + r.in2 <= MAX_CONCAT for r in den.rows) and den.E <= MAX_EMB and 1 <= n_steps <= MAX_STEPS
            and len(den.rows) <= MAX_BLOCKS and lds_bytes(den, clf) <= MAX_LDS)


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object the kernel's binding and the torch restatement read and fill                                       #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(den, clf, den_c, clf_temb, cond, obs, steps, cg_scale, predict_noise: bool, clip: bool, x_in, prior, fix_mask, x_min, x_max,
                 noise, trace: bool = False):
    """`den` / `clf` = ``describe_denoiser`` / ``describe_classifier``; `den_c` (S, E); `clf_temb` (S + 1, Ec); `cond` (B, E) or None;
    `obs` (B, O); `steps` = the plan's Step records; `cg_scale` = S Python floats; bounds / mask (A,) or None; `noise` (n_noise, B, A) or
    None.  Allocates x_out (B, A), logp_out (B, 1) and, with `trace`, trace_pred / trace_grad (S, B, A) and trace_logp (S, B)."""
    b, a = x_in.shape
    s = len(steps)
    kw = dict(device=x_in.device, dtype=x_in.dtype)
    return SimpleNamespace(
        B=b, A=a, E=den.E, O=clf.O, S=s, Ec=clf.Ec, den=den, clf=clf, den_c=den_c, clf_temb=clf_temb, cond=cond, obs=obs, steps=list(steps),
        cg_scale=[float(v) for v in cg_scale], predict_noise=bool(predict_noise), clip=bool(clip), x_in=x_in, prior=prior, fix_mask=fix_mask,
        x_min=x_min if clip else None, x_max=x_max if clip else None, noise=noise,
        x_out=torch.empty(b, a, **kw), logp_out=torch.empty(b, 1, **kw),
        trace_pred=torch.empty(s, b, a, **kw) if trace else None, trace_grad=torch.empty(s, b, a, **kw) if trace else None,
        trace_logp=torch.empty(s, b, **kw) if trace else None)


def _c_request(q):
    p = blocks._p
    den, clf = q.den, q.clf
    rows = (CdxEnergyBlock * len(den.rows))()
    for dst, r in zip(rows, den.rows):
        dst.in_, dst.in2, dst.out = r.in_, r.in2, r.out
        for name in ("w1", "b1", "w2", "b2", "wc", "bc", "ws", "bs"):
            setattr(dst, name, p(getattr(r, name)))
    steps = R.pack_steps(q.steps)
    cg = (ctypes.c_float * len(q.cg_scale))(*[float(np.float32(v)) for v in q.cg_scale])
    c = CdxEnergyGuided(B=q.B, A=q.A, E=q.E, O=q.O, S=q.S, Ec=q.Ec, n_blocks=len(den.rows), n_down=den.n_down, n_hidden=len(clf.hidden),
                        predict_noise=int(q.predict_noise), clip=int(q.clip), blocks=rows, out_w=p(den.out_w), out_b=p(den.out_b),
                        den_c=p(q.den_c), cond=p(q.cond), obs=p(q.obs), obs_w=p(clf.obs_w), obs_b=p(clf.obs_b), act_w=p(clf.act_w),
                        act_b=p(clf.act_b), act_wt=p(clf.act_wt), clf_wo=p(clf.wo), clf_bo=p(clf.bo), clf_temb=p(q.clf_temb), steps=steps,
                        cg_scale=cg, x_in=p(q.x_in), prior=p(q.prior), fix_mask=p(q.fix_mask), x_min=p(q.x_min), x_max=p(q.x_max),
                        noise=p(q.noise), x_out=p(q.x_out), logp_out=p(q.logp_out), trace_pred=p(q.trace_pred), trace_grad=p(q.trace_grad),
                        trace_logp=p(q.trace_logp))
    for l, w in enumerate(clf.hidden):
        c.hidden[l], c.clf_w[l], c.clf_b[l], c.clf_wt[l] = w, p(clf.w[l]), p(clf.b[l]), p(clf.wt[l])
    return c, (rows, steps, cg)


def native_run(q) -> None:
    """``cdx_energy_guided_run``: fills q.x_out, q.logp_out and the traces that are allocated (one launch on the current stream)."""
    c, keep = _c_request(q)
    R._check(_lib().cdx_energy_guided_run(ctypes.byref(c), R._stream_ptr(q.x_in.device)), "cdx_energy_guided_run")
    del keep


# ------------------------------------------------------------------------------------------------------------------- #
# The same loop in plain torch (any dtype, any device)                                                                        #
# ------------------------------------------------------------------------------------------------------------------- #
def _silu_grad(z):
    sg = torch.sigmoid(z)
    return sg * (1. + z * (1. - sg))


def energy_model(feat, ws, bs, wo, bo):
    """The mlp of QGPONNClassifier on the feature rows [obs_proj(obs) | act_proj(x) | temb] -> (f = 10 tanh(o / 10) (R,),
    1 - tanh^2(o / 10) (R, 1), the hidden pre-activations): the one torch restatement of csrc/cdx_energy_mlp.h's forward."""
    h, pres = feat, []
    for w, b in zip(ws, bs):
        pres.append(h @ w.t() + b)
        h = nn.functional.silu(pres[-1])
    t = torch.tanh((h @ wo.t() + bo) / 10)
    return (10 * t)[:, 0], 1. - t * t, pres


def _denoiser(den, x, c):
    """``SfBCUNet.forward`` on the block table: the raw prediction."""
    h, kept = x, []
    for i, r in enumerate(den.rows):
        if r.in2:
            h = torch.cat([h, kept.pop()], -1)
        t1 = nn.functional.silu(h @ r.w1.t() + r.b1) + (c @ r.wc.t() + r.bc)
        h = nn.functional.silu(t1 @ r.w2.t() + r.b2) + (h if r.ws is None else h @ r.ws.t() + r.bs)
        if i < den.n_down:
            kept.append(h)
    return h @ den.out_w.t() + den.out_b


def reference_run(q) -> None:
    """What ``cdx_energy_guided_run`` computes, step by step, into the same outputs and traces."""
    den, clf = q.den, q.clf
    x = q.x_in
    obs_feat = q.obs @ clf.obs_w.t() + clf.obs_b

    def energy_at(x, temb):                                            # (logp (B,), d logp / d f (B, 1), the hidden pre-activations)
        feat = torch.cat([obs_feat, x @ clf.act_w.t() + clf.act_b, temb.expand(x.shape[0], clf.Ec)], -1)
        return energy_model(feat, clf.w, clf.b, clf.wo, clf.bo)
    for s, (st, ni) in enumerate(zip(q.steps, noise_index(q.steps))):
        pred = _denoiser(den, x, q.den_c[s] if q.cond is None else q.den_c[s] + q.cond)
        logp, g, pres = energy_at(x, q.clf_temb[s])
        g = g * clf.wo * _silu_grad(pres[-1])                          # explicit backward: x SiLU'(pre), transposed weights
        for l in range(len(pres) - 1, 0, -1):
            g = (g @ clf.wt[l].t()) * _silu_grad(pres[l - 1])
        g = (g @ clf.wt[0].t()) @ clf.act_wt.t()                        # the act_proj columns of layer 0, then through act_proj
        if q.trace_pred is not None:
            q.trace_pred[s], q.trace_grad[s], q.trace_logp[s] = pred, g, logp
        x = reference_step(q, st, ni, x, pred + q.cg_scale[s] * g)
    q.x_out.copy_(x)
    if q.logp_out is not None:
        q.logp_out.copy_(energy_at(x, q.clf_temb[q.S])[0][:, None])


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def step_tables(net, clf_net, plan, device):
    """(den_c (S, E), clf_temb (S + 1, Ec)) of a plan: ``t_layer(map_noise(t_s))`` on ``cdx_gemm_f32`` as ``runtime2.mlp_table`` computes
    its time-feature rows, and the classifier's ``map_noise(t_s)`` with the row of t = 0 (a long, as the reference passes it for the
    final log_p).  Kept with the solver's cached plan under the two nets' weight signatures."""
    memo = plan.__dict__.setdefault("_memo", {})
    key = ("energy", str(device), id(net), id(clf_net))
    sig = (R._signature(net), R._signature(clf_net))
    hit = memo.get(key)
    if hit is not None and hit[0] == sig:
        return hit[1]
    with torch.no_grad():
        t_vec = R.device_times(plan, device)
        temb = R._f32c(net.map_noise(t_vec), device)
        seq = net.t_layer
        den_c = blocks.linear(blocks.linear(temb, seq[0].weight, seq[0].bias, act="silu"), seq[2].weight, seq[2].bias)
        t0 = torch.zeros((1,), dtype=torch.long, device=device)
        clf_temb = torch.cat([R._f32c(clf_net.map_noise(t_vec), device), R._f32c(clf_net.map_noise(t0), device)], 0).contiguous()
    memo[key] = (sig, (den_c, clf_temb))
    return memo[key][1]


def guidance_scale(plan, w_cg: float, predict_noise: bool):
    """The shift of the raw prediction per unit gradient, frozen per step (``classifier_guidance``: eps - w sigma g | x0 + w sigma^2 /
    alpha g): the expression of engine/guided.py."""
    return [(-(w_cg * st.sigma)) if predict_noise else (w_cg * ((st.sigma ** 2) / st.alpha)) for st in plan.steps]


def try_energy_guided(solver, model, plan, xt, prior, cond_vec, w_cfg, condition_cg, w_cg, feed) -> Optional[torch.Tensor]:
    """x_S (unclipped) of the energy-guided loop with ``_cdx_logp`` = the final log_p, or None: the host loop runs exactly as before
    (every None comes BEFORE the first draw from `feed`)."""
    from ..classifier.qgpo_classifier import QGPOClassifier
    from ..diffusion.diffusionsde import BaseDiffusionSDE
    from ..nn_classifier.mlp import QGPONNClassifier
    from ..nn_diffusion.sfbc_unet import SfBCUNet
    if not (enabled() and isinstance(solver, BaseDiffusionSDE)):
        return None
    if not (torch.is_tensor(xt) and xt.dim() == 2 and xt.is_cuda and xt.dtype == torch.float32 and xt.shape[0] > 0):
        return None
    net, clf = model["diffusion"], getattr(solver, "classifier", None)
    if type(net) is not SfBCUNet or type(clf) is not QGPOClassifier or type(clf.model_ema) is not QGPONNClassifier or clf.model_ema.training:
        return None
    clf_net = clf.model_ema
    b, a = xt.shape
    steps = plan.steps
    if w_cfg not in (0.0, 1.0) or not step_admissible(steps, MAX_STEPS):
        return None
    den, cl = _bound(net, lambda: describe_denoiser(net)), _bound(clf_net, lambda: describe_classifier(clf_net))
    if den is None or cl is None or den.A != a or cl.A != a or not within_limits(den, cl, len(steps)):
        return None
    if not on_device(condition_cg, (b, cl.O)) or (w_cfg == 1.0 and not on_device(cond_vec, (b, den.E))):
        return None
    if not all(t.is_contiguous() and t.dtype == torch.float32 for t in _tensors(den) + _tensors(cl)):
        return None
    dev = xt.device
    env = solver_env(solver, plan, prior, b, a, dev)
    if env is None:
        return None
    prior, fix_mask, x_min, x_max, clip = env
    with torch.no_grad():
        den_c, clf_temb = step_tables(net, clf_net, plan, dev)
        pn = R._predicts_noise(plan, solver)
        noise = feed.many(xt, plan.n_noise)
        q = make_request(den, cl, den_c, clf_temb, R._f32c(cond_vec.detach(), dev) if w_cfg == 1.0 else None,
                         R._f32c(condition_cg.detach(), dev), steps, guidance_scale(plan, w_cg, pn), pn, clip, R._f32c(xt.detach(), dev),
                         prior, fix_mask, x_min, x_max, None if noise is None else R._f32c(noise.detach(), dev))
        globals()["native_run"](q)                           # (looked up per call: the CPU tests patch it)
    out = q.x_out
    out._cdx_logp = q.logp_out
    return out
