"""The critics' Linear -> [LayerNorm] -> activation towers on one forward and one backward row-tile launch (``cdx_tower_fwd_f32`` /
``cdx_tower_bwd_f32``, csrc/cdx_tower.hip).

``DQLCritic``, ``TwinQ`` and ``V`` (utils/critics.py) are stepped on every gradient update of the dql / edp / idql / qgpo pipelines.  As
library nodes (``train.chain_forward``) a tower costs one launch per Linear, LayerNorm and activation forward and about twice that
backward.  ``try_tower`` runs one tower, or twin towers over the same input, as ONE ``torch.autograd.Function``:

* forward: one ``cdx_tower_fwd_f32`` (16 rows per workgroup, activations in LDS, the saved tensors H / P / rstd layer-major);
* backward: one ``cdx_tower_bwd_f32`` (G_l = d loss / d z_l, the per-tile partial sums of the LayerNorm gradients, g_x), one
  ``cdx_conv_wgrad_batch_f32`` for every weight and bias gradient of the call, one ``cdx_colsum_batch_f32`` for every gain and shift
  gradient.  Under ``train.grads_in_place()`` the sums are added into the ``.grad`` tensors; otherwise into one flat zeroed buffer whose
  views go back to autograd.

Without autograd it is the forward launch alone (``save == 0``), up to ``NOGRAD_MAX_ROWS`` rows -- asked for with ``CDX_TOWER=1``: the
default keeps ``heads.try_sequential`` there.  Which autograd calls take the launches without being asked is the call site's `default`
(``DQLCritic`` yes, ``TwinQ`` / ``V`` with ``CDX_TOWER=1``).  ``reference_forward`` / ``reference_backward`` restate the
kernels in plain torch on the same request object (any dtype, any device): what the CPU tests run in place of the C calls and what the
GPU tests compare the buffers against.  ``CDX_TOWER=0`` keeps the node route everywhere.
"""
import ctypes
import os
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import blocks, train
from . import runtime as R
from .consts import ACT_MISH, ACT_NONE, ACT_RELU, ACT_SILU, ACT_TANH
from .energy import MAX_LDS, MAX_WIDTH, MAX_X
from .rowtile import ROWS, declare, r16

MAX_LAYERS = 6                                         # CDX_TOWER_MAX_LAYERS
COLSUM_BATCH = 32                                      # CDX_COLSUM_BATCH
# the largest measured row count at which the no-grad forward launch still beats heads.run_chain by more than the two spreads
# (tools/bench_tower.py, profiles/tower_ab.txt)
NOGRAD_MAX_ROWS = 16384
_ACT_IDS = {None: ACT_NONE, "mish": ACT_MISH, "silu": ACT_SILU, "relu": ACT_RELU, "tanh": ACT_TANH}

_FP, _I = ctypes.c_void_p, ctypes.c_int32
_PER_LAYER = _FP * MAX_LAYERS * 2


class CdxTower(ctypes.Structure):
    _fields_ = [("R", _I), ("K0", _I), ("n_towers", _I), ("n_layers", _I), ("width", _I * MAX_LAYERS), ("norm", _I * MAX_LAYERS),
                ("act", _I * MAX_LAYERS), ("eps", ctypes.c_float * MAX_LAYERS), ("save", _I), ("want_gx", _I), ("want_params", _I),
                ("x", _FP), ("w", _PER_LAYER), ("b", _PER_LAYER), ("gamma", _PER_LAYER), ("beta", _PER_LAYER),
                ("out", _FP * 2), ("H", _FP * 2), ("P", _FP * 2), ("rstd", _FP * 2), ("g_out", _FP * 2), ("G", _FP * 2),
                ("Sb", _FP * 2), ("Sg", _FP * 2), ("g_x", _FP * 2)]


class CdxColsumJob(ctypes.Structure):
    _fields_ = [("src", _FP), ("out", _FP), ("rows", ctypes.c_longlong), ("cols", _I), ("ld", _I)]


class CdxColsumBatch(ctypes.Structure):
    _fields_ = [("n_jobs", _I), ("wg_start", _I * (COLSUM_BATCH + 1)), ("job", CdxColsumJob * COLSUM_BATCH)]


def _lib():
    tower = ([ctypes.POINTER(CdxTower), ctypes.c_void_p], ctypes.c_int)
    return declare(R.load_library(), {"cdx_tower_lds_bytes": ([ctypes.POINTER(CdxTower)], ctypes.c_longlong),
                                      "cdx_tower_fwd_f32": tower, "cdx_tower_bwd_f32": tower,
                                      "cdx_colsum_batch_f32": ([ctypes.POINTER(CdxColsumBatch), ctypes.c_void_p], ctypes.c_int)})


def enabled(default: bool) -> bool:
    """``CDX_TOWER=1``: every call the launches take; ``CDX_TOWER=0``: none; unset: the autograd calls of the call sites that are fused
    by `default` (utils/critics.py: where the measurement of DESIGN.md 3m decides it)."""
    asked = os.environ.get("CDX_TOWER")
    return asked == "1" or (asked != "0" and default)


def nograd_enabled() -> bool:
    """The no-grad forward launch is asked for (``CDX_TOWER=1``); unset, ``heads.try_sequential`` evaluates the critics as before."""
    return os.environ.get("CDX_TOWER") == "1"


# ------------------------------------------------------------------------------------------------------------------- #
# The tower as the kernels read it                                                                                            #
# ------------------------------------------------------------------------------------------------------------------- #
def describe(seq) -> Optional[SimpleNamespace]:
    """K0, and per layer width / norm / act (CDX_ACT_*) / eps and the Linear and LayerNorm modules, of a Sequential of
    ``Linear -> [LayerNorm] -> [activation]`` layers (``train._chain_plan``'s walk: nested Sequentials flattened, Identity and inactive
    Dropout dropped), or None: a module or an order the kernels do not know, or sizes outside their limits."""
    if not isinstance(seq, nn.Sequential):
        return None
    plan = train._chain_plan(seq)
    if not plan:
        return None
    d = SimpleNamespace(K0=0, width=[], norm=[], act=[], eps=[], lins=[], lns=[])
    i = 0
    while i < len(plan):
        kind, lin, act = plan[i]
        if kind != "linear":
            return None                                   # (a norm or an activation that no Linear of this layer precedes)
        ln = None
        if i + 1 < len(plan) and plan[i + 1][0] == "norm":
            if act is not None:
                return None                               # Linear -> activation -> LayerNorm
            ln, act = plan[i + 1][1], plan[i + 1][2]
            if ln.normalized_shape[0] != lin.out_features:
                return None
            i += 1
        if act not in _ACT_IDS:
            return None                                   # GELU
        if d.width and lin.in_features != d.width[-1]:
            return None
        d.K0 = d.K0 or lin.in_features
        d.width.append(lin.out_features)
        d.norm.append(ln is not None)
        d.act.append(_ACT_IDS[act])
        d.eps.append(float(ln.eps) if ln is not None else 0.0)
        d.lins.append(lin)
        d.lns.append(ln)
        i += 1
    return d if within_limits(d) else None


def shape_of(d) -> tuple:
    return d.K0, tuple(d.width), tuple(d.norm), tuple(d.act), tuple(d.eps)


def lds_bytes(d) -> int:
    """The kernels' LDS plan (tower_plan of csrc/cdx_tower.hip; ``cdx_tower_lds_bytes``): two activation images [16][widest + 4]."""
    return 4 * 2 * ROWS * (max(r16(w) for w in [d.K0] + list(d.width)) + 4)


def within_limits(d) -> bool:
    """The limits ``cdx_tower_fwd_f32`` / ``cdx_tower_bwd_f32`` refuse with CDX_EINVAL."""
    return (1 <= len(d.width) <= MAX_LAYERS and 0 < d.K0 <= MAX_WIDTH and all(0 < w <= MAX_WIDTH and w % 16 == 0 for w in d.width[:-1])
            and 0 < d.width[-1] <= MAX_X and all(e > 0 for e, n in zip(d.eps, d.norm) if n) and lds_bytes(d) <= MAX_LDS)


def params_of(d) -> list:
    """[w_0, b_0, (gamma_0, beta_0), w_1, ...]: the parameters themselves."""
    out = []
    for lin, ln in zip(d.lins, d.lns):
        out += [lin.weight, lin.bias] + ([ln.weight, ln.bias] if ln is not None else [])
    return out


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object the kernels' bindings and the torch restatements read and fill                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def _layers(buf, count: int, widths):
    """[tower][layer] (count, width) views of a (towers, stride) buffer, layer-major."""
    cuts = [count * sum(widths[:l]) for l in range(len(widths) + 1)]
    return [[row[cuts[l]:cuts[l + 1]].view(count, w) for l, w in enumerate(widths)] for row in buf]


def _r4(v: int) -> int:
    return (v + 3) & ~3                                   # (a tower's share of a buffer starts 16-byte aligned)


def make_request(d, weights, x, save: bool = True):
    """`d`: ``describe``'s answer for the towers' common shape; `weights`: per tower ``params_of`` as tensors; `x` (R, K0).  Allocates what
    the forward writes (the layout of include/cdx.h: cdx_tower): out, and with `save` H / P / rstd -- ``q.H[t][l]``, ``q.P[t][l]`` are the
    (R, width[l]) matrices, ``q.rstd[t][l]`` (R,)."""
    rows, towers, n = x.shape[0], len(weights), len(d.width)
    kw = dict(device=x.device, dtype=x.dtype)
    q = SimpleNamespace(R=rows, K0=d.K0, width=list(d.width), norm=list(d.norm), act=list(d.act), eps=list(d.eps), n_towers=towers, x=x,
                        save=save, w=[], b=[], gamma=[], beta=[], out=[torch.empty(rows, d.width[-1], **kw) for _ in range(towers)])
    for ws in weights:
        it = iter(ws)
        w, b, ga, be = [], [], [], []
        for has_norm in d.norm:
            w.append(next(it)), b.append(next(it))
            ga.append(next(it) if has_norm else None), be.append(next(it) if has_norm else None)
        q.w.append(w), q.b.append(b), q.gamma.append(ga), q.beta.append(be)
    if save:
        q.H_buf = torch.empty(towers, _r4(rows * sum(d.width[:-1])), **kw)
        q.P_buf = torch.empty(towers, _r4(rows * sum(d.width)), **kw)
        q.rstd_buf = torch.empty(towers, n * rows, **kw)
        q.H, q.P = _layers(q.H_buf, rows, d.width[:-1]), _layers(q.P_buf, rows, d.width)
        q.rstd = [[row[l * rows:(l + 1) * rows] for l in range(n)] for row in q.rstd_buf]
    return q


def add_backward(q, g_out, want_gx: bool, want_params: bool):
    """`g_out`: per tower (R, width[-1]).  Allocates what the backward writes: G (as P), Sb / Sg (``q.Sb[t][l]``: (tiles, width[l]), read
    for normed layers only), g_x per tower."""
    kw = dict(device=q.x.device, dtype=q.x.dtype)
    tiles = -(-q.R // ROWS)
    q.g_out, q.want_gx, q.want_params, q.tiles = list(g_out), want_gx, want_params, tiles
    q.G = q.Sb = q.Sg = q.g_x = None
    if want_params:
        q.G_buf = torch.empty(q.n_towers, _r4(q.R * sum(q.width)), **kw)
        q.S_buf = torch.empty(2, q.n_towers, tiles * sum(q.width), **kw)
        q.G = _layers(q.G_buf, q.R, q.width)
        q.Sb, q.Sg = _layers(q.S_buf[0], tiles, q.width), _layers(q.S_buf[1], tiles, q.width)
    if want_gx:
        q.g_x = [torch.empty(q.R, q.K0, **kw) for _ in range(q.n_towers)]
    return q


def _c_request(q, backward: bool) -> CdxTower:
    p = blocks._p
    c = CdxTower(R=q.R, K0=q.K0, n_towers=q.n_towers, n_layers=len(q.width), save=int(q.save), x=p(q.x))
    for l, w in enumerate(q.width):
        c.width[l], c.norm[l], c.act[l], c.eps[l] = w, int(q.norm[l]), q.act[l], q.eps[l]
    for t in range(q.n_towers):
        for l in range(len(q.width)):
            c.w[t][l], c.b[t][l], c.gamma[t][l], c.beta[t][l] = p(q.w[t][l]), p(q.b[t][l]), p(q.gamma[t][l]), p(q.beta[t][l])
        c.out[t] = p(q.out[t])
        if q.save:
            c.H[t], c.P[t], c.rstd[t] = p(q.H_buf[t]), p(q.P_buf[t]), p(q.rstd_buf[t])
        if backward:
            c.g_out[t] = p(q.g_out[t])
            if q.want_params:
                c.G[t], c.Sb[t], c.Sg[t] = p(q.G_buf[t]), p(q.S_buf[0][t]), p(q.S_buf[1][t])
            if q.want_gx:
                c.g_x[t] = p(q.g_x[t])
    if backward:
        c.want_gx, c.want_params = int(q.want_gx), int(q.want_params)
    return c


def native_forward(q) -> None:
    """``cdx_tower_fwd_f32``: fills q.out and, with q.save, q.H, q.P and q.rstd (one launch on the current stream)."""
    c = _c_request(q, False)
    R._check(_lib().cdx_tower_fwd_f32(ctypes.byref(c), R._stream_ptr(q.x.device)), "cdx_tower_fwd_f32")


def native_backward(q) -> None:
    """``cdx_tower_bwd_f32``: fills q.G, q.Sb, q.Sg (q.want_params) and q.g_x (q.want_gx) (one launch on the current stream)."""
    c = _c_request(q, True)
    R._check(_lib().cdx_tower_bwd_f32(ctypes.byref(c), R._stream_ptr(q.x.device)), "cdx_tower_bwd_f32")


def weight_sums(jobs) -> None:
    """`jobs` = [(p_rows, q_rows, rows, dw_out, db_out | None)]: dw_out += p^T q, db_out += the column sums of p, one launch."""
    blocks.conv_wgrad_batch([(p, q, n, 1, 1, 1, 1, 0, dw, db) for p, q, n, dw, db in jobs])


def column_sums(jobs) -> int:
    """`jobs` = [(src (rows, cols) fp32 device matrix, out (cols))]: out += the column sums of src, ceil(n / 32) launches of
    ``cdx_colsum_batch_f32``.  -> launches issued."""
    jobs = [j for j in jobs if j[0].shape[0] > 0]
    n_launch = 0
    for lo in range(0, len(jobs), COLSUM_BATCH):
        part = jobs[lo:lo + COLSUM_BATCH]
        b = CdxColsumBatch(n_jobs=len(part))
        start = 0
        for j, (src, out) in enumerate(part):
            rows, cols = src.shape
            assert out.is_contiguous() and out.numel() == cols and out.dtype == torch.float32
            b.wg_start[j] = start
            start += -(-cols // 64) * -(-rows // 64)
            b.job[j] = CdxColsumJob(src=src.data_ptr(), out=out.data_ptr(), rows=rows, cols=cols, ld=blocks._rows(src))
        b.wg_start[len(part)] = start
        R._check(_lib().cdx_colsum_batch_f32(ctypes.byref(b), R._stream_ptr(part[0][0].device)), "cdx_colsum_batch_f32")
        n_launch += 1
    return n_launch


def wgrad_operands(q, t: int):
    """(p, q, rows) of the weight-gradient product of every Linear of tower `t`: dW = p^T q, db = the column sums of p."""
    inputs = [q.x] + q.H[t]
    return [(q.G[t][l], inputs[l], q.R) for l in range(len(q.width))]


# ------------------------------------------------------------------------------------------------------------------- #
# The same two launches in plain torch (any dtype, any device)                                                                #
# ------------------------------------------------------------------------------------------------------------------- #
_ACT_FN = {ACT_NONE: lambda y: y, ACT_MISH: F.mish, ACT_SILU: F.silu, ACT_RELU: torch.relu, ACT_TANH: torch.tanh}


def _act_grad(act: int, y):
    if act == ACT_NONE:
        return torch.ones_like(y)
    if act == ACT_RELU:
        return (y > 0).to(y.dtype)
    if act == ACT_TANH:
        return 1 - torch.tanh(y) ** 2
    sg = torch.sigmoid(y)
    if act == ACT_SILU:
        return sg * (1 + y * (1 - sg))
    th = torch.tanh(F.softplus(y))                         # Mish
    return th + y * (1 - th * th) * sg


def reference_forward(q) -> None:
    """What ``cdx_tower_fwd_f32`` computes, into the same buffers."""
    n = len(q.width)
    for t in range(q.n_towers):
        h = q.x
        for l in range(n):
            y = z = h @ q.w[t][l].t() + q.b[t][l]
            if q.norm[l]:
                mean = z.mean(1, keepdim=True)
                rstd = 1 / torch.sqrt(((z - mean) ** 2).mean(1, keepdim=True) + q.eps[l])
                z = (z - mean) * rstd                      # xhat
                y = z * q.gamma[t][l] + q.beta[t][l]
                if q.save:
                    q.rstd[t][l].copy_(rstd[:, 0])
            h = _ACT_FN[q.act[l]](y)
            if l == n - 1:
                q.out[t].copy_(h)
            elif q.save:
                q.H[t][l].copy_(h)
            if q.save:
                q.P[t][l].copy_(z)


def reference_backward(q) -> None:
    """What ``cdx_tower_bwd_f32`` computes, into the same buffers (explicit formulas, no autograd)."""
    pad = q.tiles * ROWS - q.R
    tile_sums = lambda m: F.pad(m, (0, 0, 0, pad)).view(q.tiles, ROWS, -1).sum(1)      # noqa: E731
    for t in range(q.n_towers):
        dh = q.g_out[t]
        for l in range(len(q.width) - 1, -1, -1):
            p = q.P[t][l]
            if q.norm[l]:
                dy = dh * _act_grad(q.act[l], p * q.gamma[t][l] + q.beta[t][l])
                g = dy * q.gamma[t][l]
                dz = q.rstd[t][l][:, None] * (g - g.mean(1, keepdim=True) - p * (g * p).mean(1, keepdim=True))
                if q.want_params:
                    q.Sb[t][l].copy_(tile_sums(dy))
                    q.Sg[t][l].copy_(tile_sums(dy * p))
            else:
                dz = dh * _act_grad(q.act[l], p)
            if q.want_params:
                q.G[t][l].copy_(dz)
            if l or q.want_gx:
                dh = dz @ q.w[t][l]
        if q.want_gx:
            q.g_x[t].copy_(dh)


def reference_param_grads(q, t: int) -> list:
    """The gradient of every parameter of tower `t` from the backward's buffers, in the order of ``params_of``."""
    out = []
    for l, (p_rows, q_rows, _) in enumerate(wgrad_operands(q, t)):
        out += [p_rows.t() @ q_rows, p_rows.sum(0)] + ([q.Sg[t][l].sum(0), q.Sb[t][l].sum(0)] if q.norm[l] else [])
    return out


# ------------------------------------------------------------------------------------------------------------------- #
# Routing                                                                                                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def _on_device(x, params) -> bool:
    """A ROCm device, fp32 and contiguous throughout?  (Looked up per call: the CPU tests patch it.)"""
    return x.is_cuda and all(p.device == x.device and p.is_contiguous() for p in params)


class _Tower(torch.autograd.Function):
    """One or two towers over the same (R, K0) rows -> their (R, width[-1]) outputs.  Arguments: x, the common description, then every
    tower's ``params_of``."""

    @staticmethod
    def forward(ctx, x, d, *params):
        per = len(params_of(d))
        weights = [[p.detach() for p in params[i:i + per]] for i in range(0, len(params), per)]
        q = make_request(d, weights, x.detach(), save=True)
        globals()["native_forward"](q)
        ctx.q, ctx.params = q, params
        return tuple(q.out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_out):
        q, params = ctx.q, ctx.params
        needs = ctx.needs_input_grad[2:]
        g_out = [torch.zeros_like(o) if g is None else g.to(q.x.dtype).contiguous() for g, o in zip(g_out, q.out)]
        add_backward(q, g_out, want_gx=ctx.needs_input_grad[0], want_params=any(needs))
        globals()["native_backward"](q)
        g_x = None
        if q.want_gx:
            g_x = q.g_x[0] if q.n_towers == 1 else q.g_x[0] + q.g_x[1]
        grads = [None] * len(params)
        if q.want_params:
            # where the sums go: the .grad tensors under train.grads_in_place() (every wanted one or none), else one flat zeroed buffer
            wanted = [i for i, need in enumerate(needs) if need]
            slots = {i: train._grad_slot(params[i]) for i in wanted}
            in_place = all(s is not None for s in slots.values())
            if not in_place:
                flat = torch.zeros(sum(params[i].numel() for i in wanted), device=q.x.device, dtype=q.x.dtype)
                at = 0
                for i in wanted:
                    slots[i] = grads[i] = flat[at:at + params[i].numel()].view(params[i].shape)
                    at += params[i].numel()
            wjobs, cjobs, i = [], [], 0
            for t in range(q.n_towers):
                for l, (p_rows, q_rows, rows) in enumerate(wgrad_operands(q, t)):
                    if i in slots:
                        wjobs.append((p_rows, q_rows, rows, slots[i], slots.get(i + 1)))
                    elif i + 1 in slots:
                        cjobs.append((p_rows, slots[i + 1]))           # (a bias that trains under a frozen weight)
                    i += 2
                    if q.norm[l]:
                        cjobs += [(s, slots[j]) for s, j in ((q.Sg[t][l], i), (q.Sb[t][l], i + 1)) if j in slots]
                        i += 2
            if wjobs:
                globals()["weight_sums"](wjobs)
            if cjobs:
                globals()["column_sums"](cjobs)
            if in_place:
                train._written(*slots.values())
        ctx.q = None
        return (g_x, None, *grads)


def try_tower(seqs, x, default: bool = True) -> Optional[tuple]:
    """``tuple(seq(x) for seq in seqs)`` for one Sequential or two of the same shape on the fused launches, or None: the caller's other
    routes run exactly as before (every None comes BEFORE anything is written).  Leading dimensions of `x` are rows.  `default`: does
    this call site take the launches without being asked (``enabled``)?"""
    if not (enabled(default) and train.enabled()):
        return None
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() >= 1 and x.numel() > 0) or len(seqs) not in (1, 2):
        return None
    descs = [describe(s) for s in seqs]
    if any(d is None for d in descs) or any(shape_of(d) != shape_of(descs[0]) for d in descs[1:]):
        return None
    d = descs[0]
    params = [p for dd in descs for p in params_of(dd)]
    if x.shape[-1] != d.K0 or any(p.dtype != torch.float32 for p in params) or not globals()["_on_device"](x, params):
        return None
    rows = x.numel() // d.K0
    if rows > 0x7fffffff - ROWS:
        return None
    autograd = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    if not autograd and not (nograd_enabled() and rows <= NOGRAD_MAX_ROWS):
        return None
    lead = x.shape[:-1]
    x2 = x.reshape(rows, d.K0).contiguous()
    if autograd:
        outs = _Tower.apply(x2, d, *params)
    else:
        per = len(params) // len(seqs)
        q = make_request(d, [[p.detach() for p in params[i:i + per]] for i in range(0, len(params), per)], x2.detach(), save=False)
        globals()["native_forward"](q)
        outs = q.out
    return tuple(o.reshape(*lead, d.width[-1]) for o in outs)
