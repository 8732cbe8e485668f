"""Score K candidates per state and pick among them (``cdx_score_select_f32`` / ``cdx_select_f32``, csrc/cdx_select.hip).

Every value-guided pipeline ends its ``sample()`` call with the same tail: the observation repeated K times next to the K candidates, a
critic (twin towers and their minimum), ``softmax(T * q, 1)``, then ``multinomial`` / ``argmax`` / ``argsort`` and a gather, or the
weighted value -- 15 to 25 launches of a few microseconds.  Here it is

* ``native_score_select``: ONE launch for the critic on the UN-repeated observations (16 candidate rows of one state per workgroup, the
  layer body of the fused towers), the minimum of the twin towers and, with K <= 16, the reduction as well;
* ``native_select``: ONE launch for the reduction over given scores (K > 16 behind the first, or scores the caller already has).

``run`` issues what a request needs.  ``reference_scores`` / ``reference_select`` restate the two kernels in plain torch on the same
request object (any dtype, any device): what runs on the CPU, what ``CDX_SELECT=0`` keeps on the device for A/B runs, and what the GPU
tests compare the buffers against in float64.  Admission of a critic goes through ``tower.describe``: a tower it does not take (GELU, a
width outside the limits) runs as a module on the repeated rows and only the reduction goes native (utils/selection.py).  Nothing here
carries a gradient: inputs are detached."""
import ctypes
import math
import os
from types import SimpleNamespace
from typing import Optional

import torch

from . import blocks, tower
from . import runtime as R
from .energy import MAX_LDS, MAX_WIDTH, MAX_X
from .rowtile import ROWS, declare, r16

MODES = {"none": 0, "argmax": 1, "sample": 2, "topk_mean": 3}          # CDX_SELECT_*
MAX_K, MAX_TOPK = 1024, 16                                             # CDX_SELECT_MAX_K, CDX_SELECT_MAX_TOPK

_FP, _I = ctypes.c_void_p, ctypes.c_int32
_PER_LAYER = _FP * tower.MAX_LAYERS * 2


class CdxSelect(ctypes.Structure):
    _fields_ = [("S", _I), ("K", _I), ("P", _I), ("payload_ld", _I), ("mode", _I), ("top_k", _I), ("temperature", ctypes.c_float),
                ("reserved", _I), ("scores", _FP), ("payload", _FP), ("u", _FP), ("weights", _FP), ("value", _FP), ("index", _FP),
                ("picked", _FP)]


class CdxScoreSelect(ctypes.Structure):
    _fields_ = [("sel", CdxSelect), ("O", _I), ("A", _I), ("n_towers", _I), ("n_layers", _I), ("width", _I * tower.MAX_LAYERS),
                ("norm", _I * tower.MAX_LAYERS), ("act", _I * tower.MAX_LAYERS), ("eps", ctypes.c_float * tower.MAX_LAYERS),
                ("obs", _FP), ("cand", _FP), ("w", _PER_LAYER), ("b", _PER_LAYER), ("gamma", _PER_LAYER), ("beta", _PER_LAYER),
                ("scores", _FP)]


def _lib():
    return declare(R.load_library(), {"cdx_select_f32": ([ctypes.POINTER(CdxSelect), ctypes.c_void_p], ctypes.c_int),
                                      "cdx_score_select_lds_bytes": ([ctypes.POINTER(CdxScoreSelect)], ctypes.c_longlong),
                                      "cdx_score_select_f32": ([ctypes.POINTER(CdxScoreSelect), ctypes.c_void_p], ctypes.c_int)})


def enabled() -> bool:
    """``CDX_SELECT=0`` keeps the module-plus-torch route everywhere."""
    return os.environ.get("CDX_SELECT") != "0"


# ------------------------------------------------------------------------------------------------------------------- #
# Admission                                                                                                                   #
# ------------------------------------------------------------------------------------------------------------------- #
def lds_bytes(d) -> int:
    """The LDS plan of ``cdx_score_select_f32`` (score_plan of csrc/cdx_select.hip; ``cdx_score_select_lds_bytes``): the tile's scores
    and weights, the input image [16][K0 + 4], two activation images [16][widest layer + 4]."""
    return 4 * (2 * ROWS + ROWS * (r16(d.K0) + 4) + 2 * ROWS * (max(r16(w) for w in d.width) + 4))


def describe_critic(seqs, obs_dim: int, cand_dim: int):
    """``tower.describe``'s answer for one Sequential or two of the same shape that score rows ``[obs | cand]`` with one number each
    within the limits of ``cdx_score_select_f32``, or None."""
    if len(seqs) not in (1, 2):
        return None
    descs = [tower.describe(s) for s in seqs]
    if any(d is None for d in descs) or any(tower.shape_of(d) != tower.shape_of(descs[0]) for d in descs[1:]):
        return None
    d = descs[0]
    if d.K0 != obs_dim + cand_dim or d.width[-1] != 1 or not 1 <= cand_dim <= MAX_X or d.K0 > MAX_WIDTH or lds_bytes(d) > MAX_LDS:
        return None
    return descs


def within_limits(S: int, K: int, mode: str, top_k: int, temperature: float, P: int) -> bool:
    """The limits ``cdx_select_f32`` refuses with CDX_EINVAL."""
    return (S >= 0 and 1 <= K <= MAX_K and S * K <= 0x7fffffff - ROWS and mode in MODES and math.isfinite(temperature)
            and (mode != "topk_mean" or 1 <= top_k <= min(K, MAX_TOPK)) and 0 <= P <= MAX_X)


# ------------------------------------------------------------------------------------------------------------------- #
# The request: one object the kernels' bindings and the torch restatements read and fill                                     #
# ------------------------------------------------------------------------------------------------------------------- #
def make_request(S: int, K: int, mode: str = "argmax", temperature: float = 1.0, top_k: int = 1, u=None, scores=None, payload=None,
                 want_weights: bool = False, critic=None, obs=None, cand=None):
    """`scores` (S * K) given, or `critic` = (``tower.describe``'s answer, per tower ``tower.params_of`` as tensors) with `obs` (S, O) or
    None and `cand` (S * K, A).  `payload`: (S * K, P) rows with unit column stride (a row stride wider than P is passed on as it is) or
    None.  Allocates what the calls write (the layout of include/cdx.h: cdx_select): scores with a critic, value (S), weights (S, K) on
    request, and with a mode other than "none" index (S, n) int32 and, with a payload, picked (S, P); n = top_k in "topk_mean", else 1."""
    ref = scores if scores is not None else cand
    kw = dict(device=ref.device, dtype=ref.dtype)
    n = top_k if mode == "topk_mean" else 1
    q = SimpleNamespace(S=S, K=K, mode=mode, temperature=float(temperature), top_k=int(top_k), n=n, u=u, scores=scores, payload=payload,
                        P=0 if payload is None else payload.shape[1], critic=critic is not None, obs=obs, cand=cand,
                        weights=torch.empty(S, K, **kw) if want_weights else None, value=torch.empty(S, **kw), index=None, picked=None)
    if mode != "none":
        q.index = torch.empty(S, n, device=ref.device, dtype=torch.int32)
        if payload is not None:
            q.picked = torch.empty(S, q.P, **kw)
    if critic is not None:
        d, weights = critic
        q.O, q.A = d.K0 - cand.shape[1], cand.shape[1]
        q.d, q.tower_weights = d, weights
        q.scores = torch.empty(S * K, **kw)
    return q


def _c_select(q) -> CdxSelect:
    p = blocks._p
    c = CdxSelect(S=q.S, K=q.K, P=q.P, mode=MODES[q.mode], top_k=q.top_k, temperature=q.temperature, scores=p(q.scores), u=p(q.u),
                  weights=p(q.weights), value=p(q.value), index=p(q.index), picked=p(q.picked))
    if q.payload is not None:
        c.payload, c.payload_ld = p(q.payload), (q.payload.stride(0) if q.payload.shape[0] > 1 else q.P)
    return c


def _c_score_select(q) -> CdxScoreSelect:
    p, d = blocks._p, q.d
    c = CdxScoreSelect(sel=_c_select(q), O=q.O, A=q.A, n_towers=len(q.tower_weights), n_layers=len(d.width), obs=p(q.obs), cand=p(q.cand),
                       scores=p(q.scores))
    for l, w in enumerate(d.width):
        c.width[l], c.norm[l], c.act[l], c.eps[l] = w, int(d.norm[l]), d.act[l], d.eps[l]
    for t, ws in enumerate(q.tower_weights):
        it = iter(ws)
        for l, has_norm in enumerate(d.norm):
            c.w[t][l], c.b[t][l] = p(next(it)), p(next(it))
            if has_norm:
                c.gamma[t][l], c.beta[t][l] = p(next(it)), p(next(it))
    return c


def native_select(q) -> None:
    """``cdx_select_f32``: the reduction over q.scores -- fills q.value and what else the request holds of weights, index, picked (one
    launch on the current stream)."""
    c = _c_select(q)
    R._check(_lib().cdx_select_f32(ctypes.byref(c), R._stream_ptr(q.scores.device)), "cdx_select_f32")


def native_score_select(q) -> None:
    """``cdx_score_select_f32``: fills q.scores and, with K <= 16, everything ``native_select`` fills (one launch on the current
    stream)."""
    c = _c_score_select(q)
    R._check(_lib().cdx_score_select_f32(ctypes.byref(c), R._stream_ptr(q.cand.device)), "cdx_score_select_f32")


def run(q) -> int:
    """The launches a request needs on the device: critic and reduction in one for K <= 16, two for K > 16, the reduction alone over
    given scores.  -> launches issued."""
    if not q.critic:
        globals()["native_select"](q)
        return 1
    globals()["native_score_select"](q)
    if q.K <= ROWS:
        return 1
    globals()["native_select"](q)
    return 2


# ------------------------------------------------------------------------------------------------------------------- #
# The same two launches in plain torch (any dtype, any device)                                                                #
# ------------------------------------------------------------------------------------------------------------------- #
def reference_scores(q) -> None:
    """What ``cdx_score_select_f32`` writes to q.scores: the towers over ``[obs_s | cand_row]`` and their minimum."""
    x = q.cand
    if q.obs is not None:
        x = torch.cat([q.obs[:, None, :].expand(q.S, q.K, q.O).reshape(q.S * q.K, q.O), q.cand], 1)
    tq = tower.make_request(q.d, q.tower_weights, x, save=False)
    tower.reference_forward(tq)
    out = tq.out[0] if len(tq.out) == 1 else torch.min(tq.out[0], tq.out[1])
    q.scores.copy_(out[:, 0])


def reference_select(q) -> None:
    """What ``cdx_select_f32`` computes from q.scores, into the same buffers."""
    sc = q.scores.view(q.S, q.K)
    w = torch.softmax(q.temperature * sc, 1)
    q.value.copy_((w * sc).sum(1))
    if q.weights is not None:
        q.weights.copy_(w)
    if q.mode == "none":
        return
    ks = torch.arange(q.K, device=sc.device).expand(q.S, q.K)
    if q.mode == "sample":           # the smallest k whose running sum exceeds u, the last index for what is left
        beyond = torch.cumsum(w, 1) > q.u.to(w.dtype)[:, None]
        idx = torch.where(beyond, ks, torch.full_like(ks, q.K - 1)).min(1).values[:, None]
    elif q.mode == "argmax":         # the first maximum
        idx = torch.where(sc == sc.max(1, keepdim=True).values, ks, torch.full_like(ks, q.K - 1)).min(1).values[:, None]
    else:                            # rank order, the lowest index on ties
        idx = torch.sort(sc, dim=1, descending=True, stable=True).indices[:, :q.top_k]
    q.index.copy_(idx)
    if q.picked is not None:
        rows = q.payload[(torch.arange(q.S, device=sc.device)[:, None] * q.K + idx).reshape(-1)].view(q.S, q.n, q.P)
        acc = rows[:, 0]
        for r in range(1, q.n):
            acc = acc + rows[:, r]
        q.picked.copy_(acc / q.n if q.n > 1 else acc)


def reference_run(q) -> None:
    if q.critic:
        reference_scores(q)
    reference_select(q)


def on_device(*tensors) -> bool:
    """fp32 tensors on one ROCm device?  (Looked up per call: the CPU tests patch it.)"""
    ts = [t for t in tensors if t is not None]
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == ts[0].device for t in ts)


def rows_view(t: Optional[torch.Tensor], rows: int):
    """`t` as (rows, P) with unit column stride and one row stride, without a copy where its layout allows."""
    if t is None:
        return None
    t = t.detach()
    if t.dim() != 2:
        t = t.reshape(rows, t.shape[-1])
    if t.stride(1) != 1 or (rows > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t
