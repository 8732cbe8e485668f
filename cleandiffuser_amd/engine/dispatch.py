"""Dispatch rules between the fused gfx950 executors and the PyTorch executor.

Two native executors: the one-workgroup-per-trajectory program kernel (runtime2.py / program2.py: JannerUNet1d, ChiUNet1d below its
crossover, the HalfJannerUNet1d classifier, PearceMlp / DQLMlp / DVInvMlp / MlpNNDiffusion / SfBCUNet) and the big-batch GEMM executors
(bigbatch.py: DiT1d, DiT1Ref, ChiTransformer, PearceTransformer, IDQLMlp / NewIDQLMlp, the U-Nets at large batch or size).

HIP fast path  <=>  tensor lives on a ROCm device  AND  gradients are off  AND  dtype is fp32  AND
the backbone is one the program compiler understands.  Everything else (CPU tensors, autograd, exotic
variants such as ``attention=True``) runs the stock PyTorch modules.  On a ROCm device a *missing or
unloadable* ``libcdx.so`` is a hard error -- there is no silent eager fallback for supported backbones.
"""
from typing import Optional

import torch


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


def _gemm_executor(net, x, edm=False, forward=False, unet_only=False):
    """The big-batch GEMM executor (a bigbatch.Family) this request is to be offered to, or None.  DiT1d / DiT1Ref, PearceTransformer,
    ChiTransformer and IDQLMlp / NewIDQLMlp have no other native executor: what bigbatch answers is final, None (-> PyTorch) included.
    The U-Nets (kind "chiunet") also have the program kernel: they are offered from their crossover up (bigbatch.is_chiunet_gemm) and
    a None leaves the request to that kernel.  (The type sets are disjoint, so it does not matter which of the two is looked at first.)"""
    from . import bigbatch
    fam = bigbatch.family_of(net)
    if fam is None or fam.kind != "chiunet":
        return None if unet_only else fam
    return fam if bigbatch.is_chiunet_gemm(net, x.shape[0], x.shape[1] if x.dim() == 3 else None, edm, forward) else None


def _try_backbone_forward(module, x, noise, condition) -> Optional[torch.Tensor]:
    """Serve ``backbone.forward`` from the fused program kernel, or return None for the PyTorch path."""
    if not _on_gpu(x) or torch.is_grad_enabled() and _needs_grad(module, x, condition):
        return None
    if x.dtype != torch.float32:
        return None
    from . import bigbatch, runtime
    fam = _gemm_executor(module, x, forward=True)
    if fam is not None:
        y = bigbatch.forward(module, x, noise, condition)
        if y is not None or fam.kind != "chiunet":
            return y
    return runtime.backbone_forward(module, x, noise, condition)


def _needs_grad(module, x, condition) -> bool:
    if x.requires_grad or (condition is not None and condition.requires_grad):
        return True
    return any(p.requires_grad for p in module.parameters())


def _sample_unguided(solver, model, plan, xt, prior, cond_vec, w_cfg, feed, unet_only=False):
    """The whole loop on the GEMM executors (EDM / consistency kinds included), else in one launch of the program kernel."""
    from . import bigbatch, runtime
    net = model["diffusion"]
    fam = _gemm_executor(net, xt, edm=runtime.plan_is_edm(plan), unet_only=unet_only)
    if fam is not None:
        out = bigbatch.sample(solver, net, plan, xt, prior, cond_vec, w_cfg, feed)
        if out is not None or fam.kind != "chiunet":
            return out
    return runtime.fused_sample(solver, model, plan, xt, prior, cond_vec, w_cfg, feed)


def _try_fused_sample(solver, model, plan, xt, prior, cond_vec, w_cfg, w_cg, requires_grad, feed):
    """Run the whole denoising loop in one launch, or return None for the PyTorch executor."""
    if not _on_gpu(xt) or requires_grad or xt.dtype != torch.float32:
        return None
    if w_cg != 0.0 and solver.classifier is not None:
        from . import guided             # classifier guidance: fused backbone forward + explicit classifier backward per step
        return guided.guided_sample(solver, model, plan, xt, prior, cond_vec, w_cfg, w_cg, feed)
    return _sample_unguided(solver, model, plan, xt, prior, cond_vec, w_cfg, feed)


def _try_fused_raw(solver, model, plan, z, temperature, prior, feed):
    """The common unconditional request before x_T exists: `z` is the initial N(0, I) draw.  When the second-generation U-Net
    kernel takes the request it forms x_T = (z * temperature) * (1 - fix_mask) + prior * fix_mask itself (reference
    diffusionsde.py:509-510), so a steady-state sample() call launches that kernel and nothing else.
    None -> the caller forms x_T with ATen ops and goes through try_fused_sample as before (no draw consumed here)."""
    if not _on_gpu(z) or z.dtype != torch.float32 or z.dim() != 3:
        return None
    from . import runtime, runtime2
    net = model["diffusion"]
    if not runtime._is_janner(net) or runtime.plan_is_edm(plan) or runtime2.supported(net, z.shape[1]) is not None:
        return None
    if _gemm_executor(net, z) is not None:              # (a request the GEMM executor takes starts from x_T)
        return None
    return runtime.fused_sample(solver, model, plan, z, prior, None, 0.0, feed, x_scale=float(temperature))


def _try_fused_edm(solver, model, plan, xt, prior, cond_vec, w_cfg, w_cg, requires_grad, feed, condition_cg=None):
    """``ContinuousEDM.sample``: big-batch executors for the GEMM-shaped backbones, the program kernel for the rest.  Classifier
    guidance (reference newedm.py:217-234: only with a classifier, w_cg != 0 AND a condition_cg) goes through the per-step guided
    executor; without a condition_cg the reference applies no shift, so the request is an unguided one."""
    if not _on_gpu(xt) or requires_grad or xt.dtype != torch.float32:
        return None
    if w_cg != 0.0 and solver.classifier is not None and condition_cg is not None:
        from . import guided
        return guided.guided_sample(solver, model, plan, xt, prior, cond_vec, w_cfg, w_cg, feed)
    return _sample_unguided(solver, model, plan, xt, prior, cond_vec, w_cfg, feed)


def _try_fused_legacy_ddpm(solver, model, plan, xt, prior, cond_vec, w_cfg, w_cg, requires_grad, feed):
    """Legacy ``DDPM`` class: same fused executor, legacy step kinds.  Of the GEMM executors only the U-Net one is offered: a legacy
    DDPM over DiT1d or IDQLMlp runs on the PyTorch executor."""
    if not _on_gpu(xt) or requires_grad or xt.dtype != torch.float32:
        return None
    if solver.classifier is not None and w_cg != 0.0:
        return None
    return _sample_unguided(solver, model, plan, xt, prior, cond_vec, w_cfg, feed, unet_only=True)


def _scoped(fn):
    """One request = one signature scope (runtime.signature_scope): the weight signature of a module is computed once per request."""
    import functools

    @functools.wraps(fn)
    def entry(*a, **k):
        from .runtime import signature_scope
        with signature_scope():
            return fn(*a, **k)
    return entry


try_backbone_forward = _scoped(_try_backbone_forward)
try_fused_sample = _scoped(_try_fused_sample)
try_fused_raw = _scoped(_try_fused_raw)
try_fused_edm = _scoped(_try_fused_edm)
try_fused_legacy_ddpm = _scoped(_try_fused_legacy_ddpm)
