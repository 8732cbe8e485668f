"""The Python face of csrc/cdx_rowtile.h, shared by the bindings of the row-tile kernels (engine/rollout.py, energy.py, cep.py, tower.py, select.py): the tile
constants, ctypes prototypes, the solver step of the torch restatements and the admission checks that only look at solver and plan."""
from typing import Optional

import torch

from . import runtime as R
from .plan import KIND_DDIM, KIND_DDPM, KIND_LINEAR, V_XTHETA

ROWS, XLD, ALD = 16, 64, 68                            # RO_ROWS, RO_XLD, RO_ALD


def r16(v: int) -> int:
    return (v + 15) & ~15


def declare(lib, prototypes):
    """`lib` with {name: (argtypes, restype)} set on its functions (once: ctypes keeps one function object per name)."""
    for name, (argtypes, restype) in prototypes.items():
        f = getattr(lib, name)
        if f.argtypes is None:
            f.argtypes, f.restype = argtypes, restype
    return lib


def on_device(t, shape) -> bool:
    """An fp32 tensor of this shape on the GPU?"""
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)


def noise_index(steps):
    """Per step the number of its draw among the stochastic steps, or -1: ``noise_idx`` as ``runtime.pack_steps`` numbers it."""
    idx, k = [], 0
    for st in steps:
        idx.append(k if st.noise else -1)
        k += 1 if st.noise else 0
    return idx


def step_admissible(steps, max_steps: int) -> bool:
    """The records ``ro_check_steps`` admits: 1 .. max_steps one-step updates (the ...2M solvers carry x_theta from step to step, EDM
    plans carry flags: host loop)."""
    return 1 <= len(steps) <= max_steps and not any(st.kind not in (KIND_DDPM, KIND_DDIM, KIND_LINEAR) or st.vsel > 1 or st.flags
                                                     for st in steps)


def solver_env(solver, plan, prior, b: int, a: int, dev, refuse_grad: bool = False) -> Optional[tuple]:
    """(prior, fix_mask, x_min, x_max, clip) as a row-tile request carries them -- detached, mask and bounds flat (A,), the prior only
    with a mask, the bounds only when the plan clips -- or None for what the kernels do not take: per-sample masks or bounds, a mask
    without a (B, A) prior and, with `refuse_grad`, a mask or bound that takes a gradient."""
    try:
        fix_mask = R._dense_hd(solver.fix_mask, 1, a, dev)
        clip = bool(getattr(plan, "clip_each_step", True)) and solver.clip_pred
        x_min = R._dense_hd(getattr(solver, "x_min", None), 1, a, dev) if clip else None
        x_max = R._dense_hd(getattr(solver, "x_max", None), 1, a, dev) if clip else None
    except (ValueError, RuntimeError):
        return None
    if refuse_grad and any(t is not None and t.requires_grad for t in (fix_mask, x_min, x_max)):
        return None
    if fix_mask is not None and (not torch.is_tensor(prior) or tuple(prior.shape) != (b, a)):
        return None
    flat = lambda t: None if t is None else t.detach().reshape(-1).contiguous()      # noqa: E731
    return R._f32c(prior.detach(), dev) if fix_mask is not None else None, flat(fix_mask), flat(x_min), flat(x_max), clip


def _bounds(q, st, x):
    """(lower, upper) of the clamp at this step, each a tensor or None (``BaseDiffusionSDE.clip_prediction``)."""
    if not q.clip:
        return None, None
    if q.predict_noise:
        lo = (x - st.alpha * q.x_max) / st.sigma if q.x_max is not None else None
        hi = (x - st.alpha * q.x_min) / st.sigma if q.x_min is not None else None
        return lo, hi
    return q.x_min, q.x_max


def reference_step(q, st, ni: int, x, p):
    """x_{s+1} from x_s and the raw prediction `p`: clip, eps <-> x0, the affine update of the record, `+ k z` (draw `ni` of q.noise),
    fix-mask blend -- the solver step of the row-tile kernels (csrc/cdx_rollout.hip, csrc/cdx_energy.hip)."""
    lo, hi = _bounds(q, st, x)
    if lo is not None:
        p = torch.maximum(p, lo)
    if hi is not None:
        p = torch.minimum(p, hi)
    k0, k1, k2, k3, _ = st.k
    if q.predict_noise:
        eps, xth = p, (x - st.sigma * p) / st.alpha
    else:
        eps, xth = (x - st.alpha * p) / st.sigma, p
    if st.kind == KIND_DDPM:
        new = k0 * (x - k1 * eps) + k2 * eps
        if ni >= 0:
            new = new + k3 * q.noise[ni]
    elif st.kind == KIND_DDIM:
        new = k0 * ((x - k1 * eps) / k2) + k3 * eps
    else:
        assert st.kind == KIND_LINEAR and st.vsel <= 1
        new = k0 * x - k1 * (xth if st.vsel == V_XTHETA else eps)
        if ni >= 0:
            new = new + k2 * q.noise[ni]
    if q.fix_mask is not None:
        new = new * (1. - q.fix_mask) + q.prior * q.fix_mask
    return new
