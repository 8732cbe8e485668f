"""Pieces of the policy steps the pipelines write inline, as calls.

``approx_action`` is EDP's action approximation (reference pipelines/edp_d4rl_mujoco.py:100-108): one noised action, one evaluation of the
denoiser, the prediction fed to the critic for the Q term.

Execution: on a ROCm device, where the fused denoising node is switched on (``CDX_DENOISE``) and takes the net (DQLMlp /
DVInvMlp), the evaluation is one forward and one backward launch (engine/denoise.py); on the CPU, with ``CDX_DENOISE=0`` or on a refusal
the module call runs, so the result is the same everywhere.  Imported from this module: ``cleandiffuser_amd.utils`` does not re-export
it."""
from typing import Optional

import torch

from .misc import at_least_ndim


def approx_action(actor, act: torch.Tensor, obs: torch.Tensor, t: Optional[torch.Tensor] = None,
                  eps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``actor.model["diffusion"](alpha_t act + sigma_t eps, t, actor.model["condition"](obs, None))`` with `t` and `eps` drawn as the
    pipeline draws them (``randint`` over the diffusion steps -- the time distribution of the actor's own ``add_noise`` for a continuous
    SDE --, then ``randn_like``) unless given.  Differentiable; no fix mask, as in the pipeline."""
    from ..engine import denoise
    t, eps = actor._noise_draws(act, t, eps)
    alpha, sigma = actor._alpha_sigma_rows(t)
    noisy_act = at_least_ndim(alpha, act.dim()) * act + at_least_ndim(sigma, act.dim()) * eps
    cond = actor.model["condition"](obs, None)
    net = actor.model["diffusion"]
    pred = denoise.try_predict(net, noisy_act, t, cond)
    return net(noisy_act, t, cond) if pred is None else pred
