"""Host side of the horizon critic (``utils.critics.DVHorizonCritic``; C side: csrc/cdx_hcritic.hip, include/cdx.h).

Three routes, tried in this order by ``DVHorizonCritic.forward``:

* ``try_score``: scoring without autograd -- what the Decision Veteran pipelines do with ``num_envs x candidates`` freshly sampled plans at
  every environment step -- is ONE call of ``cdx_hcritic_run``: the checkpoint tensors in place, a cached workspace, every launch on the
  caller's stream.  Only token 0 of the last block reaches the output, so the last block runs its key / value projection over all rows
  and everything else on one row per trajectory.
* ``forward_nodes``: with autograd (the critic's MSE step) the whole forward on the library's autograd nodes, as ``train.dit_forward``.
* the stock modules: CPU, and anything the two refuse.

``reference_run`` restates the executor's pruned data flow in plain torch (any dtype): what the tests hold the executor against.
"""
import ctypes
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import bigbatch, train
from .bigbatch import CdxHcriticBlock, CdxHcriticWeights
from .rowtile import declare
from .runtime import _check, _stream_ptr, load_library

MAX_TOKENS, MAX_D_MODEL, MAX_HEAD_DIM = 64, 1024, 64
# Which routes serve without being asked: the measurement of DESIGN.md 3n (profiles/hcritic_ab.txt) against the stock modules on the device.
SCORE_DEFAULT = True      # 2.3-2.5 x the stock modules at both shipped scoring shapes
NODES_DEFAULT = True      # 1.4 x stock autograd on the batch-128 training step
CHUNK_OVERRIDE = int(os.environ.get("CDX_HCRITIC_CHUNK", 0)) or None      # tuning hook (tools/bench_hcritic.py, tests)


def _lib():
    w = ctypes.POINTER(CdxHcriticWeights)
    return declare(load_library(), {
        "cdx_hcritic_workspace_floats": ([w, ctypes.c_int32, ctypes.c_int32], ctypes.c_longlong),
        "cdx_hcritic_run": ([w, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_longlong,
                             ctypes.c_void_p], ctypes.c_int)})


def score_enabled() -> bool:
    """``CDX_HCRITIC=1``: the executor scores; ``CDX_HCRITIC=0``: the stock modules; unset: ``SCORE_DEFAULT``."""
    asked = os.environ.get("CDX_HCRITIC")
    return asked == "1" or (asked != "0" and SCORE_DEFAULT)


def nodes_enabled() -> bool:
    """``CDX_HCRITIC_NODES=1`` / ``0`` / unset (``NODES_DEFAULT``), under ``CDX_TRAIN_NATIVE`` like every node route."""
    asked = os.environ.get("CDX_HCRITIC_NODES")
    return train.enabled() and (asked == "1" or (asked != "0" and NODES_DEFAULT))


# ------------------------------------------------------------------------------------------------ #
# limits and the workspace plan (restated from csrc/cdx_hcritic.hip; tests/test_hcritic_cpu.py holds the two equal) #
# ------------------------------------------------------------------------------------------------ #
def within_limits(tokens: int, d_model: int, n_heads: int, depth: int) -> bool:
    return 1 <= tokens <= MAX_TOKENS and 1 <= d_model <= MAX_D_MODEL and n_heads >= 1 and d_model % n_heads == 0 and \
        d_model // n_heads <= MAX_HEAD_DIM and depth >= 1


def default_chunk(tokens: int, d_model: int) -> int:
    """Trajectories per pass where the caller does not say (``hc_default_chunk``)."""
    return max(max((320 << 20) // (16 * d_model), 2048) // tokens, 1)


def workspace_floats(tokens: int, d_model: int, depth: int, batch: int, chunk: int = 0) -> int:
    """Floats of workspace of ``cdx_hcritic_run`` (``hc_layout``): every buffer rounded up to 64 floats."""
    nb = min(chunk if chunk > 0 else default_chunk(tokens, d_model), batch)
    rows, d = nb * tokens, d_model
    r64 = lambda n: (n + 63) & ~63  # noqa: E731
    full = [rows * d, rows * d, rows * 3 * d] + ([rows * d, rows * d, rows * d, rows * 4 * d, rows * d] if depth > 1 else [])
    last = [nb * d, nb * d, nb * d, nb * d, nb * 4 * d, nb * d, nb * d]
    return sum(r64(n) for n in full + last)


def _shape_of(critic):
    """(d_model, n_heads, depth, pre_norm) of a critic whose blocks are what the executor computes, or None."""
    blocks_m = list(critic.blocks)
    if not blocks_m:
        return None
    heads, norm = blocks_m[0].attn.num_heads, blocks_m[0].norm_type
    if norm not in ("pre", "post"):
        return None
    for blk in blocks_m:
        a = blk.attn
        if a.in_proj_weight is None or a.in_proj_bias is None or a.bias_k is not None or a.add_zero_attn or not a.batch_first or \
                a.num_heads != heads or blk.norm_type != norm or blk.norm1.eps != blocks_m[0].norm1.eps or blk.norm2.eps != blk.norm1.eps:
            return None
    return critic.d_model, heads, len(blocks_m), norm == "pre"


def _dropout_active(critic) -> bool:
    return critic.training and critic.dropout > 0.0


def _wants_grad(critic, x) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in critic.parameters()))


def _on_device(x, params) -> bool:
    """A ROCm device, everything on it?  (Looked up per call: the CPU tests patch it.)"""
    return x.is_cuda and all(p.device == x.device for p in params)


def _fits(critic, x) -> bool:
    """fp32 (B, T, in_dim) with B > 0 on a ROCm device for exactly this class, within the limits."""
    from ..utils.critics import DVHorizonCritic
    if type(critic) is not DVHorizonCritic or not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] > 0):
        return False
    shape = _shape_of(critic)
    if shape is None or x.shape[2] != critic.in_dim or not within_limits(x.shape[1], shape[0], shape[1], shape[2]):
        return False
    params = list(critic.parameters())
    return all(p.dtype == torch.float32 and p.is_contiguous() for p in params) and globals()["_on_device"](x, params)


# ------------------------------------------------------------------------------------------------ #
# (a) the executor                                                                                     #
# ------------------------------------------------------------------------------------------------ #
def _bind(critic, tokens: int, device) -> bigbatch._Bound:
    d, heads, depth, pre = _shape_of(critic)
    keep = []
    p = lambda t: bigbatch._dev_f32(t, keep, device)  # noqa: E731
    arr = (CdxHcriticBlock * depth)()
    for i, blk in enumerate(critic.blocks):
        a, fc1, fc2 = blk.attn, blk.mlp[0], blk.mlp[3]
        arr[i] = CdxHcriticBlock(p(a.in_proj_weight), p(a.in_proj_bias), p(a.out_proj.weight), p(a.out_proj.bias), p(fc1.weight),
                                 p(fc1.bias), p(fc2.weight), p(fc2.bias))
    with torch.no_grad():
        pos = critic.pos_emb(torch.arange(tokens, device=device)).float().contiguous()
    w = CdxHcriticWeights(tokens=tokens, in_dim=critic.in_dim, d_model=d, n_heads=heads, depth=depth, pre_norm=int(pre),
                          eps=critic.blocks[0].norm1.eps, x_proj_w=p(critic.x_proj.weight), x_proj_b=p(critic.x_proj.bias), pos=p(pos),
                          blocks=arr, fin_w=p(critic.final_layer.weight), fin_b=p(critic.final_layer.bias))
    keep.append(arr)
    return bigbatch._Bound(w, keep, None)


def _score(critic, x: torch.Tensor, chunk: int = 0) -> torch.Tensor:
    """``cdx_hcritic_run`` on a request ``_fits`` admitted.  Weight pointers are bound once per weight version (``bigbatch._bound``:
    parameter storage, autograd versions and the epoch ``utils.invalidate_weights`` bumps)."""
    lib, batch, tokens = _lib(), x.shape[0], x.shape[1]
    bound = bigbatch._bound(critic, ("hcritic", tokens), lambda: _bind(critic, tokens, x.device))
    w = ctypes.byref(bound.struct)
    need = lib.cdx_hcritic_workspace_floats(w, batch, chunk)
    if need < 0:
        _check(int(need), "cdx_hcritic_workspace_floats")
    ws = bigbatch._workspace(x.device, need)
    out = torch.empty((batch, 1), device=x.device, dtype=torch.float32)
    _check(lib.cdx_hcritic_run(w, x.data_ptr(), out.data_ptr(), batch, chunk, ws.data_ptr(), ws.numel(), _stream_ptr(x.device)),
           "cdx_hcritic_run")
    return out


def try_score(critic, x, chunk: Optional[int] = None) -> Optional[torch.Tensor]:
    """``critic(x)`` as (B, 1) through the executor, or None (nothing has been written then): not asked for (``score_enabled``), a
    gradient is wanted, dropout is active, or not a request ``_fits`` admits (device, dtype, layout, class, limits)."""
    if not score_enabled():
        return None
    if not torch.is_tensor(x) or _wants_grad(critic, x) or _dropout_active(critic):
        return None
    if not (_fits(critic, x) and x.is_contiguous()):
        return None
    return globals()["_score"](critic, x.detach(), chunk if chunk is not None else (CHUNK_OVERRIDE or 0))


# ------------------------------------------------------------------------------------------------ #
# (b) the autograd nodes                                                                               #
# ------------------------------------------------------------------------------------------------ #
def supports_nodes(critic, x) -> bool:
    return nodes_enabled() and torch.is_tensor(x) and _wants_grad(critic, x) and _fits(critic, x)


@train._with_weight_packs
def forward_nodes(critic, x: torch.Tensor) -> torch.Tensor:
    """The critic's forward with autograd on the library's nodes: every Linear ``_LinearAct`` (fc1 with its GELU), every LayerNorm
    ``_LayerNormPlain``, the attention core ``_Attention`` (``_MHA`` with a drawn mask while the attention dropout is active); the MLP's
    nn.Dropout, the positional table and the residual adds stay ATen.  All tokens go through every block; the output Linear takes the
    token-0 rows."""
    L, LN = train._LinearAct.apply, train._LayerNormPlain.apply
    b, tokens, d_in = x.shape
    d = critic.d_model
    h = L(x.reshape(b * tokens, d_in), critic.x_proj.weight, critic.x_proj.bias, None)
    h = (h.view(b, tokens, d) + critic._positions(tokens, x.device)[None]).view(b * tokens, d)
    for blk in critic.blocks:
        pre, att = blk.norm_type == "pre", blk.attn
        u = LN(h, blk.norm1.eps) if pre else h
        qkv = L(u, att.in_proj_weight, att.in_proj_bias, None)
        keep = train.draw_keep(att.dropout, att.training, b, att.num_heads, tokens, tokens, x.device)
        core = train._Attention.apply(qkv, b, tokens, att.num_heads) if keep is None else \
            train._MHA.apply(qkv, None, b, att.num_heads, None, keep)
        a = u + L(core, att.out_proj.weight, att.out_proj.bias, None)
        v = LN(a, (blk.norm2 if pre else blk.norm1).eps)
        f = blk.mlp[2](L(v, blk.mlp[0].weight, blk.mlp[0].bias, "gelu_tanh"))            # (nn.Dropout: an ATen draw in train mode)
        o = (a if pre else v) + L(f, blk.mlp[3].weight, blk.mlp[3].bias, None)
        h = o if pre else LN(o, blk.norm2.eps)
    return L(h.view(b, tokens, d)[:, 0, :], critic.final_layer.weight, critic.final_layer.bias, None)


# ------------------------------------------------------------------------------------------------ #
# the executor's data flow in plain torch                                                              #
# ------------------------------------------------------------------------------------------------ #
def reference_run(critic, x: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """What ``cdx_hcritic_run`` computes, launch by launch, in `dtype` on the tensors of `critic` (eval semantics: no dropout): blocks
    0 .. depth - 2 over all rows; the last block with the sliced in_proj rows -- [d, 3d) for the keys and values of all tokens, [0, d) for
    the query of the token-0 rows taken in place -- and one row per trajectory behind its single-query attention."""
    c = lambda t: t.detach().to(dtype)  # noqa: E731
    b, T, _ = x.shape
    d, heads, depth, pre = _shape_of(critic)
    dh, eps = d // heads, critic.blocks[0].norm1.eps
    ln = lambda t: F.layer_norm(t, (d,), eps=eps)  # noqa: E731
    lin = lambda t, w, bias: t @ c(w).t() + c(bias)  # noqa: E731
    gelu = lambda t: F.gelu(t, approximate="tanh")  # noqa: E731
    with torch.no_grad():
        pos = critic.pos_emb(torch.arange(T, device=x.device)).to(dtype)
        h = (lin(c(x).reshape(b * T, -1), critic.x_proj.weight, critic.x_proj.bias).view(b, T, d) + pos[None]).reshape(b * T, d)
        for blk in list(critic.blocks)[:-1]:
            att = blk.attn
            u = ln(h) if pre else h
            q, k, v = (t.view(b, T, heads, dh).transpose(1, 2) for t in lin(u, att.in_proj_weight, att.in_proj_bias).chunk(3, dim=1))
            p = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
            a = lin((p @ v).transpose(1, 2).reshape(b * T, d), att.out_proj.weight, att.out_proj.bias) + u
            n = ln(a)
            o = lin(gelu(lin(n, blk.mlp[0].weight, blk.mlp[0].bias)), blk.mlp[3].weight, blk.mlp[3].bias) + (a if pre else n)
            h = o if pre else ln(o)
        blk = critic.blocks[-1]
        att = blk.attn
        u = ln(h) if pre else h
        u0 = u.view(b, T, d)[:, 0, :]                                           # the token-0 rows, in place
        kv = lin(u, att.in_proj_weight[d:], att.in_proj_bias[d:])                # (b T, 2d) = [k | v]
        q0 = lin(u0, att.in_proj_weight[:d], att.in_proj_bias[:d]).view(b, heads, 1, dh)
        k, v = (t.reshape(b, T, heads, dh).transpose(1, 2) for t in (kv[:, :d], kv[:, d:]))
        p = torch.softmax(q0 @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)         # (b, heads, 1, T)
        a0 = lin((p @ v).reshape(b, d), att.out_proj.weight, att.out_proj.bias) + u0
        n0 = ln(a0)
        o0 = lin(gelu(lin(n0, blk.mlp[0].weight, blk.mlp[0].bias)), blk.mlp[3].weight, blk.mlp[3].bias) + (a0 if pre else n0)
        return lin(o0 if pre else ln(o0), critic.final_layer.weight, critic.final_layer.bias)
