"""A supervised MSE training step as a call: ``mse_step(net, optim, x, y)`` is ``optim.zero_grad()``, ``((net(x) - y) ** 2).mean()``,
backward, ``optim.step()``.  Reference: the critic's inner loop of pipelines/sfbc_d4rl_mujoco.py:144-149 and ``update`` of the
inverse-dynamics heads (invdynamic/mlp.py:54-60; pipelines/dd_d4rl_*.py:89-90, veteran_d4rl_*.py:253/263/474).

Execution: on a ROCm device, where it is switched on (``CDX_REGRESS_STEP=1``, or unset at the call sites of ``FUSED_BY_DEFAULT``:
DESIGN.md 3r), the load of the rows, the forward, the loss and the backward-data pass are ONE launch and every parameter gradient comes
out of two more (engine/regress_step.py); on the CPU, with ``CDX_REGRESS_STEP=0`` or on a refusal (GELU, an active dropout, parameters
with hooks, an input that needs a gradient, ...) the eager sequence runs, so the result is the same everywhere.  Returns {"loss"} as a
0-d tensor on the inputs' device without a host synchronisation.  Imported from this module: ``cleandiffuser_amd.utils`` does not
re-export it."""
from typing import Optional

import torch
import torch.nn as nn

from .blocks import Mlp

# Which call sites take the fused launch without being asked (CDX_REGRESS_STEP unset): those where it beats the parent route by more
# than the sum of the two spreads in tools/bench_invdyn_step.py (profiles/invdyn_step_ab.txt).  Per call site: the
# largest row count up to which that was measured and holds (0: opt-in only).  ``MlpInvDynamic.update`` passes at 128 rows (Decision
# Veteran) and at 64 x 31 = 1984 rows (Decision Diffuser), obs 17 / act 6 and obs 60 / act 9 (a second run misses once, at 128 rows
# and obs 60, by 0.002 ms on one slow round of the parent: DESIGN.md 3r has both runs); nobody has measured beyond, where a CU
# runs several tiles one after the other.  ``update_idx`` (an optimiser over every member) and ``mse_step`` are not measured: opt-in.
FUSED_BY_DEFAULT = {"invdyn": 1984, "invdyn_ensemble": 0, "mse_step": 0}


def fused_by_default(site: str, rows: int) -> bool:
    return rows <= FUSED_BY_DEFAULT[site]


def sequential_of(net) -> Optional[nn.Sequential]:
    """The Sequential behind `net` (an ``nn.Sequential`` or the ``Mlp`` of ``utils``), or None."""
    if isinstance(net, Mlp):
        return net.mlp
    return net if isinstance(net, nn.Sequential) else None


def _rows_of(x) -> int:
    return x.numel() // x.shape[-1] if torch.is_tensor(x) and x.dim() >= 1 and x.shape[-1] else 0


def fused_step(net, optim, x0, x1, y, site: str, default: Optional[bool] = None) -> Optional[dict]:
    """``regress_step.try_step`` for `net` at call site `site` -> {"loss"} with the gradients in place (``optim.step()`` is the
    caller's), or None: nothing was written."""
    from ..engine import regress_step
    seq = sequential_of(net)
    if seq is None:
        return None
    if default is None:
        default = fused_by_default(site, _rows_of(x0))
    return regress_step.try_step(seq, optim, x0, x1, y, default=default)


def mse_step(net, optim, x, y, *, x1=None, default: Optional[bool] = None) -> dict:
    """One MSE step of `net` (an ``nn.Sequential`` or an ``Mlp``) on the rows `x` -- ``[x | x1]`` with `x1` -- against the target `y`,
    up to and including ``optim.step()``.  `default`: take the fused launch without being asked (None: ``FUSED_BY_DEFAULT``).
    -> {"loss"}."""
    if sequential_of(net) is None:
        raise TypeError("mse_step: `net` is an nn.Sequential or an Mlp")
    out = fused_step(net, optim, x, x1, y, "mse_step", default)
    if out is not None:
        optim.step()
        return out
    optim.zero_grad()
    loss = ((net(x if x1 is None else torch.cat([x, x1], dim=-1)) - y) ** 2).mean()
    loss.backward()
    optim.step()
    return {"loss": loss.detach()}
