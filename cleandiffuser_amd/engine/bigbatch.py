"""Host side of the big-batch executors (``cdx_dit1d_run`` / ``cdx_pearcetf_run`` / ``cdx_chitf_run`` / ``cdx_resmlp_run`` /
``cdx_chiunet_run``, include/cdx.h, csrc/cdx_bigbatch.hip).

The backbones served here have layers that are plain GEMMs over M = batch x tokens rows, so the loop of ``sample()`` becomes a stream
of tiled-GEMM / LayerNorm / attention / solver-step launches issued by ONE C call.  This module only marshals pointers: the checkpoint
tensors are used in place (PyTorch layouts), the workspace is a cached device tensor, step records are the same ``plan.Step`` list the
fused kernel consumes.  What differs between the families -- which modules, how to bind them, the shapes they take, their chunk rule,
their C entries -- is one row each of ``FAMILIES``; ``forward()`` and ``sample()`` are written once against a row.
"""
import ctypes
import functools
import importlib
import os
import weakref
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import torch

from . import runtime
from .runtime import CdxStep, _check, _dense_hd, _f32c, _predicts_noise, _signature, _stream_ptr, host_steps, load_library

_FP = ctypes.c_void_p
_I = ctypes.c_int32


class CdxSampling(ctypes.Structure):
    _fields_ = [("batch", _I), ("hd", _I), ("emb_dim", _I), ("cond_dim", _I), ("temb", _FP),
                ("steps", ctypes.POINTER(CdxStep)), ("n_steps", _I), ("temb_per_sample", _I), ("predict_noise", _I),
                ("cfg_mode", _I), ("cfg_w", ctypes.c_float), ("cond", _FP), ("x_in", _FP), ("prior", _FP),
                ("fix_mask", _FP), ("noise", _FP), ("x_min", _FP), ("x_max", _FP), ("x_out", _FP), ("workspace", _FP),
                ("workspace_floats", ctypes.c_longlong), ("chunk", _I)]


class CdxDitBlock(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("ada_w", "ada_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w",
                                   "fc2_b")]


class CdxDitCross(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("in_w", "in_b", "out_w", "out_b")]


class CdxDitWeights(ctypes.Structure):
    _fields_ = [("tokens", _I), ("in_dim", _I), ("emb_dim", _I), ("d_model", _I), ("n_heads", _I), ("depth", _I),
                ("x_proj_w", _FP), ("x_proj_b", _FP), ("pos", _FP), ("map0_w", _FP), ("map0_b", _FP), ("map2_w", _FP),
                ("map2_b", _FP), ("blocks", ctypes.POINTER(CdxDitBlock)), ("fin_ada_w", _FP), ("fin_ada_b", _FP),
                ("fin_w", _FP), ("fin_b", _FP), ("cross", ctypes.POINTER(CdxDitCross))]


class CdxPearcetfBlock(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("qkv_w", "qkv_b", "o_w", "o_b", "r1", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "r2")]


class CdxPearcetfWeights(ctypes.Structure):
    _fields_ = [("act_dim", _I), ("To", _I), ("emb_dim", _I), ("te", _I), ("n_heads", _I), ("n_blocks", _I)] + \
               [(n, _FP) for n in ("ae0_w", "ae0_b", "ae2_w", "ae2_b", "a2i_w", "a2i_b", "t2i_w", "t2i_b", "c2i_w", "c2i_b", "cpos")] + \
               [("blocks", ctypes.POINTER(CdxPearcetfBlock)), ("fin_w", _FP), ("fin_b", _FP)]


class CdxResMlpBlock(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("ln_g", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class CdxResMlpWeights(ctypes.Structure):
    _fields_ = [("x_dim", _I), ("emb_dim", _I), ("obs_dim", _I), ("hidden", _I), ("n_blocks", _I), ("head_mish", _I),
                ("in_w", _FP), ("in_b", _FP), ("blocks", ctypes.POINTER(CdxResMlpBlock)), ("out_w", _FP), ("out_b", _FP)]


class CdxChitfLayer(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("ln1_g", "ln1_b", "sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ln2_g", "ln2_b", "ca_in_w",
                                   "ca_in_b", "ca_out_w", "ca_out_b", "ln3_g", "ln3_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")]


class CdxChitfEncLayer(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("ln1_g", "ln1_b", "sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ln2_g", "ln2_b", "ff1_w", "ff1_b",
                                   "ff2_w", "ff2_b")]


class CdxChitfWeights(ctypes.Structure):
    _fields_ = [("Ta", _I), ("To", _I), ("act_dim", _I), ("obs_dim", _I), ("d_model", _I), ("n_heads", _I), ("n_layers", _I),
                ("act_emb_w", _FP), ("act_emb_b", _FP), ("pos_emb", _FP), ("obs_emb_w", _FP), ("obs_emb_b", _FP),
                ("cond_pos_emb", _FP), ("enc0_w", _FP), ("enc0_b", _FP), ("enc2_w", _FP), ("enc2_b", _FP),
                ("layers", ctypes.POINTER(CdxChitfLayer)), ("lnf_g", _FP), ("lnf_b", _FP), ("head_w", _FP), ("head_b", _FP),
                ("self_mask", _FP), ("memory_mask", _FP), ("n_enc_layers", _I), ("enc_layers", ctypes.POINTER(CdxChitfEncLayer))]


class CdxChiUNetBlock(ctypes.Structure):
    _fields_ = [("cin_a", _I), ("cin_b", _I), ("cout", _I), ("groups", _I)] + \
               [(n, _FP) for n in ("w1a", "w1b", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "film_w", "film_b", "wra", "wrb", "br")]


class CdxUnetAttn(ctypes.Structure):
    _fields_ = [(n, _FP) for n in ("ln_g", "ln_b", "qkv_w", "out_w", "out_b")] + [("heads", _I), ("dim_head", _I)]


class CdxChiUNetWeights(ctypes.Structure):
    _fields_ = [(n, _I) for n in ("act_dim", "Ta", "cond_dim", "emb_dim", "kernel_size", "n_levels", "cond_predict_scale",
                                  "model_dim", "final_groups", "emb_hidden", "emb_out", "film_ld")] + \
               [(n, _FP) for n in ("map0_w", "map0_b", "map2_w", "map2_b", "gce_w", "gce_b")] + \
               [("blocks", ctypes.POINTER(CdxChiUNetBlock))] + \
               [(n, ctypes.POINTER(ctypes.c_void_p)) for n in ("down_w", "down_b", "up_w_even", "up_w_odd", "up_b")] + \
               [(n, _FP) for n in ("fin_w", "fin_b", "fin_g", "fin_be", "out_w", "out_b")] + \
               [("local_obs_dim", _I), ("lc_down_w", _FP), ("lc_down_b", _FP), ("attn", ctypes.POINTER(CdxUnetAttn))]


class CdxHcriticBlock(ctypes.Structure):                 # the horizon critic's executor: host path in engine/hcritic.py
    _fields_ = [(n, _FP) for n in ("qkv_w", "qkv_b", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class CdxHcriticWeights(ctypes.Structure):
    _fields_ = [("tokens", _I), ("in_dim", _I), ("d_model", _I), ("n_heads", _I), ("depth", _I), ("pre_norm", _I),
                ("eps", ctypes.c_float), ("x_proj_w", _FP), ("x_proj_b", _FP), ("pos", _FP),
                ("blocks", ctypes.POINTER(CdxHcriticBlock)), ("fin_w", _FP), ("fin_b", _FP)]


_declared = False


def _lib():
    global _declared
    lib = load_library()
    if not _declared:
        for fam in FAMILIES:                            # cdx_<entry>_workspace_floats(weights, request), cdx_<entry>_run(weights, request, stream)
            size, run = getattr(lib, f"cdx_{fam.entry}_workspace_floats"), getattr(lib, f"cdx_{fam.entry}_run")
            size.argtypes, size.restype = [ctypes.POINTER(fam.weights), ctypes.POINTER(CdxSampling)], ctypes.c_longlong
            run.argtypes, run.restype = [ctypes.POINTER(fam.weights), ctypes.POINTER(CdxSampling), ctypes.c_void_p], ctypes.c_int
        _declared = True
    return lib


# ------------------------------------------------------------------------------------------------ #
# weight marshalling (cached per module, invalidated when a parameter changes)                         #
# ------------------------------------------------------------------------------------------------ #
class _Bound:
    """ctypes weight struct + the tensors it points into (kept alive here)."""

    def __init__(self, struct, keep, sig):
        self.struct, self.keep, self.sig = struct, keep, sig


_cache = weakref.WeakKeyDictionary()


def _dev_f32(t: torch.Tensor, keep: list, device):
    """Pointer of an fp32 contiguous tensor on `device`; parameters that already are one are used in place."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
        t = t.detach().to(device=device, dtype=torch.float32).contiguous()
    keep.append(t)
    return t.data_ptr()


def _bind_dit(net, tokens: int, device) -> Optional[_Bound]:
    d = net.d_model
    heads = net.blocks[0].attn.num_heads if len(net.blocks) else 1
    if tokens > 1024 or d > 1024 or d % heads or d // heads > 64:          # CDX_ATTN_MAX_T
        return None
    cross_mods = list(getattr(net, "cross_attns", []))              # DiT1Ref only
    for a in [blk.attn for blk in net.blocks] + cross_mods:
        if a.in_proj_weight is None or a.in_proj_bias is None or a.bias_k is not None or a.add_zero_attn or \
                not a.batch_first or a.num_heads != heads:
            return None
    keep = []
    p = lambda t: _dev_f32(t, keep, device)  # noqa: E731
    cross = None
    if cross_mods:                                   # DiT1Ref (reference dit.py:135-180): one cross-attention in front of every block
        if len(cross_mods) != len(net.blocks):
            return None
        cross = (CdxDitCross * len(cross_mods))()
        for i, a in enumerate(cross_mods):
            cross[i] = CdxDitCross(p(a.in_proj_weight), p(a.in_proj_bias), p(a.out_proj.weight), p(a.out_proj.bias))
        keep.append(cross)
    blocks = (CdxDitBlock * max(len(net.blocks), 1))()
    for i, blk in enumerate(net.blocks):
        ada, fc1, fc2 = blk.adaLN_modulation[1], blk.mlp[0], blk.mlp[3]
        blocks[i] = CdxDitBlock(p(ada.weight), p(ada.bias), p(blk.attn.in_proj_weight), p(blk.attn.in_proj_bias),
                                p(blk.attn.out_proj.weight), p(blk.attn.out_proj.bias), p(fc1.weight), p(fc1.bias),
                                p(fc2.weight), p(fc2.bias))
    pos = net.pos_emb(torch.arange(tokens, device=device)).float().contiguous()     # dit.py:122-125
    fin = net.final_layer
    w = CdxDitWeights(tokens=tokens, in_dim=net.in_dim, emb_dim=net.emb_dim, d_model=d, n_heads=heads,
                      depth=len(net.blocks), x_proj_w=p(net.x_proj.weight), x_proj_b=p(net.x_proj.bias), pos=p(pos),
                      map0_w=p(net.map_emb[0].weight), map0_b=p(net.map_emb[0].bias), map2_w=p(net.map_emb[2].weight),
                      map2_b=p(net.map_emb[2].bias), blocks=blocks, fin_ada_w=p(fin.adaLN_modulation[1].weight),
                      fin_ada_b=p(fin.adaLN_modulation[1].bias), fin_w=p(fin.linear.weight), fin_b=p(fin.linear.bias), cross=cross)
    keep.append(blocks)
    return _Bound(w, keep, None)


def fold_pearcetf(net) -> Optional[dict]:
    """PearceTransformer weights with everything linear folded, in float64 then fp32 (include/cdx.h, cdx_pearcetf_weights):
    input_to_qkv1 into the attention's in_proj, out_proj into attn1_to_fcn, the 1/1.414 residual scaling and the eval-mode
    BatchNorm1d affine maps into the neighbouring Linear, the sine position codes into the token biases.  None: a variant the
    executor does not take (train mode -> BatchNorm1d batch statistics, non-default activations)."""
    import torch.nn as nn
    blocks_m = list(net.transformer_blocks)
    if net.training or not blocks_m:
        return None
    te, td, heads = blocks_m[0].trans_emb_dim, blocks_m[0].transformer_dim, blocks_m[0].nheads
    if te > 64 or td != te * heads or 2 + net.To > 64:
        return None
    if not isinstance(net.act_emb[1], nn.LeakyReLU) or net.act_emb[1].negative_slope != 0.01:
        return None
    f64 = lambda t: t.detach().to("cpu", torch.float64)  # noqa: E731
    out = {"te": te, "td": td, "heads": heads, "blocks": []}
    for blk in blocks_m:
        mha, bn_a, bn_b = blk.multihead_attn1, blk.norm1a, blk.norm1b
        if mha.in_proj_weight is None or mha.in_proj_bias is None or mha.bias_k is not None or mha.add_zero_attn or mha.batch_first or \
                not isinstance(blk.attn1_fcn[1], nn.GELU) or getattr(blk.attn1_fcn[1], "approximate", "none") != "none" or \
                not (bn_a.track_running_stats and bn_b.track_running_stats and bn_a.affine and bn_b.affine):
            return None
        wa, ba = f64(blk.input_to_qkv1.weight), f64(blk.input_to_qkv1.bias)
        wi, bi = f64(mha.in_proj_weight), f64(mha.in_proj_bias)
        sl = [slice(j * td, (j + 1) * td) for j in range(3)]
        s1 = f64(bn_a.weight) / torch.sqrt(f64(bn_a.running_var) + bn_a.eps)
        s2 = f64(bn_b.weight) / torch.sqrt(f64(bn_b.running_var) + bn_b.eps)
        wf, bfc = f64(blk.attn1_to_fcn.weight), f64(blk.attn1_to_fcn.bias)
        wo, bo = f64(mha.out_proj.weight), f64(mha.out_proj.bias)
        r1, r2 = s1 / 1.414, s2 / 1.414
        fc1, fc2 = blk.attn1_fcn[0], blk.attn1_fcn[2]
        out["blocks"].append({
            "qkv_w": torch.cat([wi[q] @ wa[q] for q in sl], 0), "qkv_b": torch.cat([wi[q] @ ba[q] + bi[q] for q in sl], 0),
            "o_w": r1[:, None] * (wf @ wo), "o_b": r1 * (wf @ bo + bfc) + f64(bn_a.bias) - f64(bn_a.running_mean) * s1, "r1": r1,
            "fc1_w": f64(fc1.weight), "fc1_b": f64(fc1.bias),
            "fc2_w": r2[:, None] * f64(fc2.weight), "fc2_b": r2 * f64(fc2.bias) + f64(bn_b.bias) - f64(bn_b.running_mean) * s2, "r2": r2})
    with torch.no_grad():
        dev0 = net.final.weight.device
        pos = lambda v: f64(net.pos_embed(torch.as_tensor(v, dtype=torch.float32, device=dev0).reshape(-1, 1)))  # noqa: E731
        pos12, cpos = pos([1.0, 2.0]), pos([float(3 + j) for j in range(net.To)])
    out.update(a2i_b=f64(net.act_to_input.bias) + pos12[0], t2i_b=f64(net.t_to_input.bias) + pos12[1], cpos=cpos)
    to32 = lambda v: v.to(torch.float32).contiguous() if isinstance(v, torch.Tensor) else v  # noqa: E731
    out["blocks"] = [{k: to32(v) for k, v in b.items()} for b in out["blocks"]]
    return {k: to32(v) for k, v in out.items()}


def _bind_pearcetf(net, _length, device) -> Optional[_Bound]:
    fold = fold_pearcetf(net)
    if fold is None:
        return None
    keep = []
    p = lambda t: _dev_f32(t, keep, device)  # noqa: E731
    arr = (CdxPearcetfBlock * len(fold["blocks"]))()
    for i, b in enumerate(fold["blocks"]):
        arr[i] = CdxPearcetfBlock(*[p(b[k]) for k in ("qkv_w", "qkv_b", "o_w", "o_b", "r1", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "r2")])
    ae0, ae2 = net.act_emb[0], net.act_emb[2]
    w = CdxPearcetfWeights(act_dim=ae0.in_features, To=net.To, emb_dim=net.emb_dim, te=fold["te"], n_heads=fold["heads"],
                           n_blocks=len(fold["blocks"]), ae0_w=p(ae0.weight), ae0_b=p(ae0.bias), ae2_w=p(ae2.weight), ae2_b=p(ae2.bias),
                           a2i_w=p(net.act_to_input.weight), a2i_b=p(fold["a2i_b"]), t2i_w=p(net.t_to_input.weight),
                           t2i_b=p(fold["t2i_b"]), c2i_w=p(net.cond_to_input.weight), c2i_b=p(net.cond_to_input.bias),
                           cpos=p(fold["cpos"]), blocks=arr, fin_w=p(net.final.weight), fin_b=p(net.final.bias))
    keep.append(arr)
    return _Bound(w, keep, None)


def _bind_resmlp(net, _length, device) -> Optional[_Bound]:
    hidden = net.affine_in.out_features
    if hidden > 4096:                                  # cdx_layernorm_f32 keeps a row in registers: C <= 4096
        return None
    keep = []
    p = lambda t: _dev_f32(t, keep, device)  # noqa: E731
    res = list(net.ln_resnet)
    blocks = (CdxResMlpBlock * max(len(res), 1))()
    for i, blk in enumerate(res):
        ln, fc1, fc2 = blk.net[1], blk.net[2], blk.net[4]
        blocks[i] = CdxResMlpBlock(p(ln.weight), p(ln.bias), p(fc1.weight), p(fc1.bias), p(fc2.weight), p(fc2.bias))
    head_mish = isinstance(net.affine_out, torch.nn.Sequential)
    head = net.affine_out[1] if head_mish else net.affine_out
    emb_dim = net.time_mlp[2].out_features
    x_dim = net.affine_in.in_features - emb_dim - net.obs_dim
    w = CdxResMlpWeights(x_dim=x_dim, emb_dim=emb_dim, obs_dim=net.obs_dim, hidden=hidden, n_blocks=len(res),
                         head_mish=int(head_mish), in_w=p(net.affine_in.weight), in_b=p(net.affine_in.bias),
                         blocks=blocks, out_w=p(head.weight), out_b=p(head.bias))
    keep.append(blocks)
    return _Bound(w, keep, None)


def _bind_chitf(net, _length, device) -> Optional[_Bound]:
    import torch.nn as nn
    d = net.act_emb.out_features
    layers = list(net.decoder.layers)
    if net.T > 64 or 1 + net.To > 16 or d > 1024 or net.decoder.norm is not None:
        return None
    enc_layers = []
    if not isinstance(net.encoder, nn.Sequential):    # n_cond_layers > 0: nn.TransformerEncoder (reference chitransformer.py:91-95)
        if not isinstance(net.encoder, nn.TransformerEncoder) or net.encoder.norm is not None:
            return None
        enc_layers = list(net.encoder.layers)
        for lyr in enc_layers:
            if not lyr.norm_first or getattr(lyr.activation, "__name__", "") != "gelu" or lyr.self_attn.in_proj_weight is None or \
                    not lyr.self_attn.batch_first or lyr.self_attn.num_heads != layers[0].self_attn.num_heads:
                return None
    heads = layers[0].self_attn.num_heads if layers else 1
    if d % heads or d // heads > 64:
        return None
    for lyr in layers:
        act = lyr.activation
        if not lyr.norm_first or getattr(act, "__name__", "") != "gelu" or lyr.self_attn.in_proj_weight is None or \
                lyr.multihead_attn.in_proj_weight is None or not lyr.self_attn.batch_first:
            return None
    keep = []
    p = lambda t: _dev_f32(t, keep, device)  # noqa: E731
    arr = (CdxChitfLayer * max(len(layers), 1))()
    for i, l in enumerate(layers):
        sa, ca = l.self_attn, l.multihead_attn
        arr[i] = CdxChitfLayer(p(l.norm1.weight), p(l.norm1.bias), p(sa.in_proj_weight), p(sa.in_proj_bias),
                               p(sa.out_proj.weight), p(sa.out_proj.bias), p(l.norm2.weight), p(l.norm2.bias),
                               p(ca.in_proj_weight), p(ca.in_proj_bias), p(ca.out_proj.weight), p(ca.out_proj.bias),
                               p(l.norm3.weight), p(l.norm3.bias), p(l.linear1.weight), p(l.linear1.bias), p(l.linear2.weight),
                               p(l.linear2.bias))
    enc = (CdxChitfEncLayer * max(len(enc_layers), 1))()
    for i, l in enumerate(enc_layers):
        sa = l.self_attn
        enc[i] = CdxChitfEncLayer(p(l.norm1.weight), p(l.norm1.bias), p(sa.in_proj_weight), p(sa.in_proj_bias), p(sa.out_proj.weight),
                                  p(sa.out_proj.bias), p(l.norm2.weight), p(l.norm2.bias), p(l.linear1.weight), p(l.linear1.bias),
                                  p(l.linear2.weight), p(l.linear2.bias))
    mlp_enc = not enc_layers
    neg = torch.finfo(torch.float32).min               # the kernels clamp scores at -3e38; -inf entries map onto that floor
    w = CdxChitfWeights(Ta=net.T, To=net.To, act_dim=net.act_emb.in_features, obs_dim=net.obs_dim, d_model=d, n_heads=heads,
                        n_layers=len(layers), act_emb_w=p(net.act_emb.weight), act_emb_b=p(net.act_emb.bias),
                        pos_emb=p(net.pos_emb[0]), obs_emb_w=p(net.obs_emb.weight), obs_emb_b=p(net.obs_emb.bias),
                        cond_pos_emb=p(net.cond_pos_emb[0]), enc0_w=p(net.encoder[0].weight) if mlp_enc else None,
                        enc0_b=p(net.encoder[0].bias) if mlp_enc else None, enc2_w=p(net.encoder[2].weight) if mlp_enc else None,
                        enc2_b=p(net.encoder[2].bias) if mlp_enc else None, n_enc_layers=len(enc_layers), enc_layers=enc,
                        layers=arr, lnf_g=p(net.ln_f.weight),
                        lnf_b=p(net.ln_f.bias), head_w=p(net.head.weight), head_b=p(net.head.bias),
                        self_mask=p(net.mask.detach().clamp_min(neg)), memory_mask=p(net.memory_mask.detach().clamp_min(neg)))
    keep += [arr, enc]
    return _Bound(w, keep, None)


class _Ptrs:
    """Device pointers of fp32 tensors; everything they point into is kept alive in ``keep``."""

    def __init__(self, device):
        self.keep, self.device = [], device

    def __call__(self, t):                              # parameters that already are fp32 contiguous on the device are used in place
        return _dev_f32(t, self.keep, self.device)

    def packed(self, t):                                # derived tensors are always fresh fp32 device copies
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def array(self, vals):
        a = (ctypes.c_void_p * max(len(vals), 1))(*vals)
        self.keep.append(a)
        return a


def _bind_unet(net, length: int, device) -> Optional[_Bound]:
    """ChiUNet1d / JannerUNet1d for the implicit-GEMM executor -- the walk both share: two residual blocks per level going down, the
    middle blocks, two per level going up (the first on the concatenated skip), the resampling convolutions and the head.  Conv
    weights are re-packed (c_out, k, c_in) once.  What differs between the two nets comes from _chiunet_adds / _janner_adds."""
    import torch.nn as nn
    from . import blocks as B
    from ..nn_diffusion.jannerunet import JannerUNet1d
    n_levels = len(net.downs)
    if length & (length - 1) or (length >> (n_levels - 1)) < 1 or n_levels > 8:
        return None
    adds = (_janner_adds if type(net) is JannerUNet1d else _chiunet_adds)(net)
    if adds is None:
        return None
    p = _Ptrs(device)

    def bind_block(blk, cin_b=0):
        c1, gn1, c2, gn2 = blk.conv1[0], blk.conv1[1], blk.conv2[0], blk.conv2[1]
        if adds.norm is not None and not (isinstance(gn1, adds.norm) and isinstance(gn2, adds.norm)):
            return None
        cin_a, film = c1.in_channels - cin_b, adds.film(blk)
        w1 = B.pack_conv(c1.weight)                     # (co, k, ci)
        has_res = isinstance(blk.residual_conv, nn.Conv1d)
        wr = blk.residual_conv.weight.detach()[:, :, 0] if has_res else None
        return CdxChiUNetBlock(
            cin_a=cin_a, cin_b=cin_b, cout=c1.out_channels, groups=gn1.num_groups,
            w1a=p.packed(w1[:, :, :cin_a]), w1b=p.packed(w1[:, :, cin_a:]) if cin_b else None, b1=p(c1.bias), g1=p(gn1.weight),
            be1=p(gn1.bias), w2=p.packed(B.pack_conv(c2.weight)), b2=p(c2.bias), g2=p(gn2.weight), be2=p(gn2.bias),
            film_w=p(film.weight), film_b=p(film.bias),
            wra=p.packed(wr[:, :cin_a]) if has_res else None, wrb=p.packed(wr[:, cin_a:]) if (has_res and cin_b) else None,
            br=p(blk.residual_conv.bias) if has_res else None)

    blocks = []                                         # (a level is (block, block, ..., resampler): Janner has its attention in between)
    for lvl in net.downs:
        blocks += [bind_block(lvl[0]), bind_block(lvl[1])]
    blocks += [bind_block(m) for m in adds.mids]
    for lvl in net.ups:
        blocks += [bind_block(lvl[0], lvl[0].conv1[0].in_channels // 2), bind_block(lvl[1])]
    blocks = adds.more_blocks(blocks, bind_block)
    if blocks is None or any(b is None for b in blocks):
        return None
    for b in blocks:                                    # identity skips need matching widths; the FAST GEMM path wants 16 | c_in
        if b.wra is None and (b.cin_b or b.cin_a != b.cout):
            return None
    arr = (CdxChiUNetBlock * len(blocks))(*blocks)
    downs = [lvl[-1].conv for lvl in net.downs if not isinstance(lvl[-1], nn.Identity)]
    ups = [lvl[-1].conv for lvl in net.ups if not isinstance(lvl[-1], nn.Identity)]
    if len(downs) != n_levels - 1 or len(ups) != n_levels - 1:
        return None
    up_packed = [B.pack_conv_transpose_k4s2p1(u.weight) for u in ups]
    fin = net.final_conv
    w = CdxChiUNetWeights(Ta=length, n_levels=n_levels, model_dim=net.model_dim, final_groups=fin[1].num_groups,
                          emb_hidden=net.map_emb[0].out_features, **adds.header)
    w.map0_w, w.map0_b, w.map2_w, w.map2_b = p(net.map_emb[0].weight), p(net.map_emb[0].bias), p(net.map_emb[2].weight), p(net.map_emb[2].bias)
    w.blocks = arr
    w.down_w, w.down_b = p.array([p.packed(B.pack_conv(d.weight)) for d in downs]), p.array([p(d.bias) for d in downs])
    w.up_w_even, w.up_w_odd = p.array([p.packed(e) for e, _ in up_packed]), p.array([p.packed(o) for _, o in up_packed])
    w.up_b = p.array([p(u.bias) for u in ups])
    w.fin_w, w.fin_b, w.fin_g, w.fin_be = p.packed(B.pack_conv(fin[0].weight)), p(fin[0].bias), p(fin[1].weight), p(fin[1].bias)
    w.out_w, w.out_b = p.packed(fin[3].weight.detach()[:, :, 0]), p(fin[3].bias)
    if not adds.finish(w, p):
        return None
    p.keep.append(arr)
    return _Bound(w, p.keep, None)


def _chiunet_adds(net) -> Optional[SimpleNamespace]:
    """ChiUNet1d: FiLM from cond_encoder (scale + bias unless cond_predict_scale is off), the observation either as one global
    vector through global_cond_encoder or -- local conditioning -- as a row per position through two extra residual blocks."""
    from . import blocks as B
    local = not net.obs_as_global_cond                  # local conditioning: one observation row per position (chiunet.py:78-82)
    if (local and net.local_cond_encoder is None) or (not local and net.global_cond_encoder is None) or (local and len(net.downs) < 2):
        return None
    E = net.emb_dim

    def more_blocks(blocks, bind_block):
        if not local:
            return blocks
        # the two places the local features join have a residual conv in every real net (act_dim != model_dim; concat input)
        if blocks[0] is None or blocks[0].wra is None or blocks[-2] is None or blocks[-2].wra is None:
            return None
        return blocks + [bind_block(net.local_cond_encoder[0]), bind_block(net.local_cond_encoder[1])]

    def finish(w, p):
        if local:
            down = net.local_cond_encoder[2].conv
            w.local_obs_dim = net.local_cond_encoder[0].conv1[0].in_channels
            w.lc_down_w, w.lc_down_b = p.packed(B.pack_conv(down.weight)), p(down.bias)
        else:
            w.gce_w, w.gce_b = p(net.global_cond_encoder.weight), p(net.global_cond_encoder.bias)
        return True

    header = dict(act_dim=net.downs[0][0].conv1[0].in_channels, emb_dim=E, cond_dim=0 if local else net.global_cond_encoder.in_features,
                  kernel_size=net.final_conv[0].kernel_size[0], cond_predict_scale=int(net.downs[0][0].cond_predict_scale),
                  emb_out=E, film_ld=E if local else 2 * E)
    return SimpleNamespace(film=lambda blk: blk.cond_encoder[1], mids=list(net.mids), norm=None, header=header,
                           more_blocks=more_blocks, finish=finish)


def _janner_adds(net) -> Optional[SimpleNamespace]:
    """JannerUNet1d: no observation input and bias-only FiLM from Linear(Mish(emb)); GroupNorm1d only; one kernel size for the blocks
    and the final conv; with ``attention=True`` a LinearAttention after every level's second block and between the middle blocks."""
    from ..utils import GroupNorm1d
    fin = net.final_conv
    if not isinstance(fin[1], GroupNorm1d) or fin[0].kernel_size[0] != net.kernel_size:
        return None

    def finish(w, p):
        if not getattr(net, "attention", False):
            return True
        # LinearAttention (reference jannerunet.py:72-95): channel LayerNorm -> to_qkv GEMM -> cdx_linattn_f32 -> to_out GEMM + the
        # normalised input
        from ..nn_diffusion.jannerunet import LinearAttention
        sites = [lvl[2] for lvl in net.downs] + [net.mid_attn] + [lvl[2] for lvl in net.ups]
        if len(sites) != 2 * w.n_levels or any(type(a) is not LinearAttention or a.to_qkv.bias is not None for a in sites):
            return False
        att = (CdxUnetAttn * len(sites))()
        for i, a in enumerate(sites):
            inner = a.to_out.in_channels
            if inner % a.heads or inner // a.heads > 64 or abs(a.scale - (inner // a.heads) ** -0.5) > 1e-12 or abs(a.norm.eps - 1e-5) > 1e-12:
                return False
            att[i] = CdxUnetAttn(p(a.norm.g.reshape(-1)), p(a.norm.b.reshape(-1)), p(a.to_qkv.weight.reshape(a.to_qkv.out_channels, -1)),
                                 p(a.to_out.weight.reshape(a.to_out.out_channels, -1)), p(a.to_out.bias), a.heads, inner // a.heads)
        w.attn = att
        p.keep.append(att)
        return True

    emb_out = net.map_emb[2].out_features
    header = dict(act_dim=net.in_dim, emb_dim=net.map_emb[0].in_features, cond_dim=0, kernel_size=net.kernel_size, cond_predict_scale=0,
                  emb_out=emb_out, film_ld=emb_out)
    return SimpleNamespace(film=lambda blk: blk.emb_mlp[1], mids=[net.mid_block1, net.mid_block2], norm=GroupNorm1d, header=header,
                           more_blocks=lambda blocks, bind_block: blocks, finish=finish)


def _bound(net, key, make) -> Optional[_Bound]:
    per_mod = _cache.setdefault(net, {})
    sig = _signature(net)
    hit = per_mod.get(key)
    if hit is not None and hit.sig == sig:
        return hit
    b = make()
    if b is not None:
        b.sig = sig
        per_mod[key] = b
    return b


_workspaces = {}


def _workspace(device, floats: int) -> torch.Tensor:
    """Scratch of the big-batch executors, one buffer per (device, stream): work is ordered by the stream it is enqueued on, so
    two solvers sampling on different torch streams must not share (or regrow) one buffer."""
    key = (device, _stream_ptr(device))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < floats:
        _workspaces[key] = ws = torch.empty(int(floats), dtype=torch.float32, device=device)
    return ws


# Chunk sizes (measured on MI355X, tools/bench_configs.py with CDX_DIT_CHUNK / CDX_MLP_CHUNK): the GEMMs are compute bound, so
# tall chunks win -- more 128 x 128 tiles per launch means fuller last waves of workgroups and fewer launches -- until the
# widest activation (rows x 4 width fp32) outgrows the 256 MiB Infinity Cache by much: DiT1d d=320 peaks at 64 k rows (335 MB),
# IDQLMlp hidden 1024 at 16 k rows (268 MB); twice that is 5-8 % slower, a quarter of it 15 % slower.
def _dit_chunk(batch: int, tokens: int, d_model: int, two: int) -> int:
    rows = max((320 << 20) // (4 * 4 * d_model), 2048)
    return max(min(batch, rows // (tokens * two)), 1)


def _mlp_chunk(batch: int, hidden: int, two: int) -> int:
    return max(min(batch, max((256 << 20) // (4 * 4 * hidden), 2048) // two), 1)


CHUNK_OVERRIDE = {"dit": int(os.environ.get("CDX_DIT_CHUNK", 0)) or None,      # tuning hooks (tools/bench_configs.py, tests)
                  "mlp": int(os.environ.get("CDX_MLP_CHUNK", 0)) or None,
                  "chitf": int(os.environ.get("CDX_CHITF_CHUNK", 0)) or None,
                  "chiunet": int(os.environ.get("CDX_CHIUNET_CHUNK", 0)) or None}
# ChiUNet1d has two native executors: the one-workgroup-per-trajectory program kernel (weights re-streamed by every CU) and the
# implicit-GEMM executor (weights shared by all rows).  The GEMM one wins once batch x length fills the 128 x 128 tiles.
UNET_GEMM_MIN_BATCH = int(os.environ.get("CDX_UNET_GEMM_MIN_BATCH", 96))   # measured: 1.45x at B=128, 1.18x at 256, 2.1x at 1024
# ... and, at ANY batch, once the net is large: the program kernel's step time is the weight stream of one CU (~13 us per MB: 3.7 ms
# per step for the 275 MB config-3 net, whatever the batch), the executor's is ~0.55 ms of dependent launches plus one pass over
# the weights for the whole batch.  Measured (round 3, profiles/r03_chiunet_small_batch.txt), 50-step DDPM at B = 8 / 32 / 64:
# model_dim 256 (68.9 M parameters) 190 / 181 / 178 ms on the program kernel vs 50 / 52 / 60 ms here; model_dim 64 (4.3 M) 16.5 vs
# 33 ms; model_dim 32 (1.1 M) 10 vs 28 ms -- the crossover sits near 10 M parameters.
UNET_GEMM_MIN_PARAMS = int(float(os.environ.get("CDX_UNET_GEMM_MIN_PARAMS", 10e6)))


# JannerUNet1d's channels are narrow (32..256): its GEMM tiles are mostly padding, so the program kernel keeps small and medium
# batches and the GEMM executor only takes over where weight re-streaming dominates (measured crossover, tools/bench_configs.py).
JANNER_GEMM_MIN_BATCH = int(os.environ.get("CDX_JANNER_GEMM_MIN_BATCH", 2048))   # config-2 net: 0.39x at 256, 0.89x at 1024, 1.16x at 3200


def _n_params(module) -> int:
    n = module.__dict__.get("_cdx_n_params")
    if n is None:
        n = module.__dict__["_cdx_n_params"] = sum(p.numel() for p in module.parameters())
    return n


def is_chiunet_gemm(module, batch: int, horizon: Optional[int] = None, edm: bool = False, forward: bool = False) -> bool:
    """Should this U-Net request go to the implicit-GEMM executor?  Yes from the measured crossover batch up, and -- when the
    horizon is given -- for configurations the one-workgroup program kernel cannot hold at all (wide / long nets whose
    activations exceed the LDS plan): those would otherwise drop to the PyTorch executor."""
    from ..nn_diffusion.chiunet import ChiUNet1d
    from ..nn_diffusion.jannerunet import JannerUNet1d
    if type(module) is JannerUNet1d:
        if horizon is not None and not edm and not forward:
            from . import runtime2
            # sampling loops: the program kernel keeps its lead at every batch size (two or three trajectories per workgroup), also for
            # nets that fit only as a compact one-trajectory program (antmaze Diffuser, H = 128 plans; measured at the antmaze size: 10.9 k
            # vs 6.0 k trajectories/s at B = 256, 13.3 k vs 11.5 k at B = 3200).  Stand-alone forwards (`forward`: per-sample timesteps)
            # and EDM plans keep the crossover rule below
            if runtime2.supported(module, horizon) is None:
                return False
        big = batch >= JANNER_GEMM_MIN_BATCH
    elif type(module) is ChiUNet1d and not module.obs_as_global_cond:
        return True                                     # local conditioning: the executor is its only native path
    elif type(module) is ChiUNet1d and module.obs_as_global_cond:
        big = batch >= UNET_GEMM_MIN_BATCH or _n_params(module) >= UNET_GEMM_MIN_PARAMS
    else:
        return False
    if big or horizon is None:
        return big
    from . import runtime2
    if runtime.supported_backbone(module, horizon, edm) is not None:
        return True                                    # no program holds it: the executor at any batch
    return forward and runtime2.compact_only(module, horizon)       # (compact programs serve sampling loops only)


def _chiunet_chunk(batch: int, Ta: int, model_dim: int, two: int) -> int:
    rows = max((256 << 20) // (4 * model_dim), 4096)       # widest live activation ~ rows x model_dim
    return max(min(batch, rows // (Ta * two)), 1)


def unet_chunk(net, batch: int, length: int, two: int = 1) -> int:
    """Trajectories per pass of the U-Net executor (CDX_CHIUNET_CHUNK / CHUNK_OVERRIDE["chiunet"] overrides the rule)."""
    return CHUNK_OVERRIDE["chiunet"] or _chiunet_chunk(batch, length, getattr(net, "model_dim", 32), two)


def unet_binding(net, length: int, device) -> Optional[_Bound]:
    """The U-Net executor's weights of `net` at this length: the binding sample() / forward() use, shared with the guided loop."""
    return _bound(net, ("chiunet", length), lambda: _bind_unet(net, length, device))


def _unet_cond_dim(w) -> int:
    """Width of a request's flattened condition: To * obs_dim (global conditioning) or Ta * obs_dim (local: a row per position)."""
    return w.Ta * w.local_obs_dim if w.local_obs_dim > 0 else w.cond_dim


def _time_features(net, t_vec, dev) -> torch.Tensor:
    """time_mlp(map_noise(t)) through the library's own GEMM (rows = number of distinct timesteps)."""
    from . import blocks
    e = _f32c(net.map_noise(t_vec), dev)
    l0, l2 = net.time_mlp[0], net.time_mlp[2]
    h = blocks.linear(e, _f32c(l0.weight, dev), _f32c(l0.bias, dev), act="mish")
    return blocks.linear(h, _f32c(l2.weight, dev), _f32c(l2.bias, dev))


# ------------------------------------------------------------------------------------------------ #
# the backbone families                                                                                #
# ------------------------------------------------------------------------------------------------ #
class Family(NamedTuple):
    """Everything the host path knows about one backbone family.  ``w`` below is the bound weight struct."""
    kind: str                        # name in _run and in the binding cache: `kind`, or (`kind`, length) where `per_length`
    entry: str                       # the C entries are cdx_<entry>_workspace_floats / cdx_<entry>_run ...
    weights: type                    # ... and take this struct
    modules: tuple                   # "file.Class" under nn_diffusion: the exact types served
    bind: Callable                   # (net, length, device) -> _Bound | None
    length: Optional[str]            # None: the state is (b, d).  Else it is (b, length, d) and this field of w holds the length
    width: Callable                  # w -> what the state's last dimension must equal
    cond_dim: Callable               # w -> width of a flattened condition row (0: the family takes no condition input)
    chunk: Callable                  # (net, w, batch, two) -> samples per pass; CHUNK_OVERRIDE[`override`] goes first
    override: str
    per_length: bool = False         # the binding depends on the length (position tables, level sizes)
    emb: str = "emb_dim"             # field of w with the width of a time-embedding row
    temb: Callable = lambda net, t, dev: _f32c(net.map_noise(t), dev)      # one embedding row per timestep
    # "optional"; "required" (the reference cannot run the net without one); "embedding": no condition input, forward() adds the
    # condition to map_noise(t) in front of map_emb (reference jannerunet.py:160-164) and sample() declines conditional requests
    cond: str = "optional"
    cond_shape: Optional[Callable] = None     # w -> shape[1:] the unflattened condition must have
    forward_checks_cond: bool = True          # forward() of DiT1d / IDQLMlp passes the condition on as it comes; sample() always checks
    refuses: Callable = lambda net: False     # asked before the binding cache is


FAMILIES = (
    Family("dit", "dit1d", CdxDitWeights, ("dit.DiT1d", "dit.DiT1Ref"), _bind_dit, "tokens", per_length=True,
           width=lambda w: w.in_dim * (2 if w.cross else 1),             # DiT1Ref rows are [reference | noisy]
           cond_dim=lambda w: w.emb_dim, forward_checks_cond=False,
           chunk=lambda net, w, b, two: _dit_chunk(b, w.tokens, w.d_model, two), override="dit"),
    # PearceTransformer runs 2 + To tokens of te * n_heads features per sample through the DiT kernels: DiT's chunk rule and override.
    # Train mode: BatchNorm1d uses batch statistics (reference pearcetransformer.py:38-39) -- the folded eval-mode weights a cached
    # binding holds do not describe that network (the cache key is the weight signature, not the mode)
    Family("pearcetf", "pearcetf", CdxPearcetfWeights, ("pearcetransformer.PearceTransformer",), _bind_pearcetf, None,
           width=lambda w: w.act_dim, cond_dim=lambda w: w.To * w.emb_dim, cond="required", cond_shape=lambda w: (w.To, w.emb_dim),
           chunk=lambda net, w, b, two: _dit_chunk(b, 2 + w.To, w.te * w.n_heads, two), override="dit",
           refuses=lambda net: net.training),
    Family("chitf", "chitf", CdxChitfWeights, ("chitransformer.ChiTransformer",), _bind_chitf, "Ta", emb="d_model",
           width=lambda w: w.act_dim, cond_dim=lambda w: w.To * w.obs_dim,
           chunk=lambda net, w, b, two: _dit_chunk(b, w.Ta, w.d_model, two), override="chitf"),
    Family("mlp", "resmlp", CdxResMlpWeights, ("mlp_backbones.IDQLMlp", "mlp_backbones.NewIDQLMlp"), _bind_resmlp, None,
           width=lambda w: w.x_dim, cond_dim=lambda w: w.obs_dim, forward_checks_cond=False,
           temb=lambda net, t, dev: _time_features(net, t, dev),         # its rows are time_mlp(map_noise(t))
           chunk=lambda net, w, b, two: _mlp_chunk(b, w.hidden, two), override="mlp"),
    # the two U-Nets share the executor, its struct and one binding cache; dispatch asks is_chiunet_gemm before it offers them a request
    _CHIUNET := Family("chiunet", "chiunet", CdxChiUNetWeights, ("chiunet.ChiUNet1d",), _bind_unet, "Ta", per_length=True,
                       width=lambda w: w.act_dim, cond_dim=_unet_cond_dim, cond="required",
                       chunk=lambda net, w, b, two: _chiunet_chunk(b, w.Ta, getattr(net, "model_dim", 32), two), override="chiunet"),
    _CHIUNET._replace(modules=("jannerunet.JannerUNet1d",), cond="embedding"),
)
_ENTRY = {fam.kind: fam.entry for fam in FAMILIES}


@functools.lru_cache(None)
def _served_types() -> dict:
    return {getattr(importlib.import_module("..nn_diffusion." + path.split(".")[0], __package__), path.split(".")[1]): fam
            for fam in FAMILIES for path in fam.modules}


def family_of(module) -> Optional[Family]:
    """The family serving exactly this module type (subclasses may compute something else), or None."""
    return _served_types().get(type(module))


def _run(kind, bound, *, batch, hd, emb_dim, cond_dim, temb, steps, n_steps, temb_per_sample, predict_noise, cfg_mode,
         cfg_w, cond, x_in, prior, fix_mask, noise, x_min, x_max, x_out, chunk):
    lib = _lib()
    pp = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    s = CdxSampling(batch=batch, hd=hd, emb_dim=emb_dim, cond_dim=cond_dim, temb=temb.data_ptr(), steps=steps,
                    n_steps=n_steps, temb_per_sample=int(temb_per_sample), predict_noise=int(predict_noise),
                    cfg_mode=cfg_mode, cfg_w=float(cfg_w), cond=pp(cond), x_in=x_in.data_ptr(), prior=pp(prior),
                    fix_mask=pp(fix_mask), noise=pp(noise), x_min=pp(x_min), x_max=pp(x_max), x_out=x_out.data_ptr(),
                    workspace=None, workspace_floats=0, chunk=chunk)
    size_fn, run_fn = getattr(lib, f"cdx_{_ENTRY[kind]}_workspace_floats"), getattr(lib, f"cdx_{_ENTRY[kind]}_run")
    need = size_fn(ctypes.byref(bound.struct), ctypes.byref(s))
    ws = _workspace(x_in.device, need)
    s.workspace, s.workspace_floats = ws.data_ptr(), ws.numel()
    if batch:
        _check(run_fn(ctypes.byref(bound.struct), ctypes.byref(s), _stream_ptr(x_in.device)), f"cdx_{kind}_run")


def _binding(fam, net, x) -> Optional[_Bound]:
    """The weights of `net` for a state shaped like `x`, or None when the family's executor does not take it."""
    if x.dim() != (3 if fam.length else 2) or fam.refuses(net):
        return None
    length = x.shape[1] if fam.length else None
    bound = _bound(net, (fam.kind, length) if fam.per_length else fam.kind, lambda: fam.bind(net, length, x.device))
    if bound is None or x.shape[-1] != fam.width(bound.struct) or (fam.length and length != getattr(bound.struct, fam.length)):
        return None
    return bound


def _condition_rows(fam, w, cond, dev, check_width=True) -> Optional[torch.Tensor]:
    """A condition flattened to fp32 rows, or None when its shape is not what the family takes."""
    if fam.cond_shape is not None and tuple(cond.shape[1:]) != fam.cond_shape(w):
        return None
    rows = _f32c(torch.flatten(cond, 1), dev)
    return rows if not check_width or rows.shape[1] == fam.cond_dim(w) else None


# ------------------------------------------------------------------------------------------------ #
# backbone.forward                                                                                     #
# ------------------------------------------------------------------------------------------------ #
def forward(net, x, noise, condition=None) -> Optional[torch.Tensor]:
    """``backbone.forward`` with a timestep per sample (what training-time evaluation, guided and custom loops call) as one executor
    call.  None -> the request is not one for this executor."""
    fam = family_of(net)
    if fam is None or (fam.cond == "required" and condition is None):
        return None
    bound = _binding(fam, net, x)
    if bound is None:
        return None
    w, b, dev = bound.struct, x.shape[0], x.device
    with torch.no_grad():
        temb, cond = fam.temb(net, noise, dev), None
        if fam.cond == "embedding":
            temb = temb.expand(b, -1)
            if condition is not None:
                if tuple(condition.shape) != tuple(temb.shape):
                    return None
                temb = temb + condition
            temb = _f32c(temb, dev)
        elif condition is not None and fam.cond_dim(w) > 0:
            cond = _condition_rows(fam, w, condition, dev, fam.forward_checks_cond)
            if cond is None:
                return None
        xin = _f32c(x, dev)
        out = torch.empty_like(xin)
        _run(fam.kind, bound, batch=b, hd=(x.shape[1] if fam.length else 1) * x.shape[-1], emb_dim=getattr(w, fam.emb),
             cond_dim=fam.cond_dim(w), temb=temb, steps=None, n_steps=0, temb_per_sample=1, predict_noise=0,
             cfg_mode=1 if cond is not None else 0, cfg_w=0.0 if fam.cond == "embedding" else 1.0, cond=cond, x_in=xin, prior=None,
             fix_mask=None, noise=None, x_min=None, x_max=None, x_out=out,
             chunk=CHUNK_OVERRIDE[fam.override] or fam.chunk(net, w, b, 1))
    return out


# ------------------------------------------------------------------------------------------------ #
# sample()                                                                                             #
# ------------------------------------------------------------------------------------------------ #
def sample(solver, net, plan, xt, prior, cond_vec, w_cfg, feed) -> Optional[torch.Tensor]:
    """Whole denoising loop as one executor call.  None -> caller uses another executor; no noise has been drawn from `feed` then."""
    fam = family_of(net)
    if fam is None:
        return None
    conditional = cond_vec is not None and w_cfg != 0.0
    if (fam.cond == "required" and not conditional) or (fam.cond == "embedding" and conditional):
        return None                                   # (the reference cannot run those backbones without a condition either)
    if fam.cond == "embedding":
        cond_vec = None
    bound = _binding(fam, net, xt)
    if bound is None:
        return None
    if cond_vec is None and w_cfg not in (0.0, 1.0):
        return None                                   # the reference raises here; let the torch executor do it
    w, dev, b, d = bound.struct, xt.device, xt.shape[0], xt.shape[-1]
    rows_h = xt.shape[1] if fam.length else 1
    try:
        fix_mask = _dense_hd(solver.fix_mask, rows_h, d, dev)
        clip = getattr(plan, "clip_each_step", True)
        x_min = _dense_hd(getattr(solver, "x_min", None), rows_h, d, dev) if clip else None
        x_max = _dense_hd(getattr(solver, "x_max", None), rows_h, d, dev) if clip else None
    except (ValueError, RuntimeError):
        return None
    with torch.no_grad():
        temb, cond_dim = fam.temb(net, runtime.device_times(plan, dev), dev), fam.cond_dim(w)
        if not conditional or cond_dim == 0:
            mode, cond = 0, None
        else:
            mode, cond = (1 if w_cfg == 1.0 else 2), _condition_rows(fam, w, cond_vec, dev)
            if cond is None or cond.shape[0] != b:
                return None
        noise = feed.many(xt, plan.n_noise)
        xin = _f32c(xt, dev)
        out = torch.empty_like(xin)
        _run(fam.kind, bound, batch=b, hd=rows_h * d, emb_dim=getattr(w, fam.emb), cond_dim=cond_dim, temb=temb, steps=host_steps(plan),
             n_steps=len(plan.steps), temb_per_sample=0, predict_noise=_predicts_noise(plan, solver),
             cfg_mode=mode, cfg_w=w_cfg, cond=cond, x_in=xin, prior=_f32c(prior, dev) if fix_mask is not None else None,
             fix_mask=fix_mask, noise=noise, x_min=x_min, x_max=x_max, x_out=out,
             chunk=CHUNK_OVERRIDE[fam.override] or fam.chunk(net, w, b, 2 if mode == 2 else 1))
    return out
