"""The critics' training steps as calls: the TD step of a double-Q critic and IQL's expectile step of V, each up to and including
``optim.step()``.  Reference: the inline steps of pipelines/dql_d4rl_mujoco.py:80-94, dql_d4rl_antmaze.py:79-98,
idql_d4rl_mujoco.py:84-107 (utils/iql.py:62-84) and qgpo_d4rl_mujoco.py:141-152.

Execution: on a ROCm device, where it is switched on (by default the steps with one target row per transition, with
``CDX_CRITIC_STEP=1`` the grouped targets too: ``FUSED_BY_DEFAULT``), the target, the
TD expression, the live forward, the loss and the backward-data pass are ONE launch and every parameter gradient comes out of two more
(engine/critic_step.py); on the CPU, with ``CDX_CRITIC_STEP=0`` or on a refusal (a tower the kernel does not take, parameters with
hooks, an input that needs a gradient, ...) the eager sequence of the pipelines' inline steps runs, so the result is the same
everywhere.  Both calls return {"loss", "target_mean"} as 0-d tensors on the inputs' device without a host synchronisation.  Imported
from this module: ``cleandiffuser_amd.utils`` does not re-export them."""
from typing import Optional

import torch
import torch.nn.functional as F

from .critics import DQLCritic, TwinQ, V

REDUCTIONS = ("min", "max", "softmax")
# Which steps take the fused launch without being asked (CDX_CRITIC_STEP unset): those that beat the parent route by more than the sum
# of the two spreads in tools/bench_critic_step.py (profiles/critic_step_ab.txt).  The grouped targets do not: their K
# target passes run one after the other on the few workgroups a batch of 256 rows fills.
FUSED_BY_DEFAULT = {"td": True, "td_grouped": False, "expectile": True}


def _towers(net) -> Optional[tuple]:
    """The Sequentials of a critic this module knows, or None."""
    if isinstance(net, DQLCritic):
        return net.q1_model, net.q2_model
    if isinstance(net, TwinQ):
        return net.Q1, net.Q2
    if isinstance(net, V):
        return (net.V,)
    return None


def _both(net, obs, act):
    return net(obs, act) if isinstance(net, DQLCritic) else net.both(obs, act)


def _column(t: Optional[torch.Tensor], rows: int) -> Optional[torch.Tensor]:
    """rew / done as the kernel reads them: (R, 1) or (R) -> (R, 1); anything else is not taken."""
    if t is None or not torch.is_tensor(t) or t.numel() != rows or t.dim() not in (1, 2):
        return None
    return t.reshape(rows, 1)


def td_target(target, rew, next_obs, done, next_act=None, *, discount: float, group: int = 1, reduce: str = "min",
              beta: Optional[float] = None) -> torch.Tensor:
    """The eager TD target (R, 1), without a gradient: ``target`` a ``V`` on `next_obs` (`next_act` None), or a double-Q critic on
    ``[next_obs repeated group times | next_act]`` reduced over the towers and the group ("min": group == 1; "max": the minimum over the
    towers of the maximum over the group; "softmax": the ``softmax(beta q)``-weighted mean of the towers' minimum)."""
    with torch.no_grad():
        if next_act is None:
            T = target(next_obs)
        else:
            obs_rpt = next_obs if group == 1 else next_obs.unsqueeze(1).repeat(1, group, 1).view(-1, next_obs.shape[-1])
            t1, t2 = _both(target, obs_rpt, next_act)
            if reduce == "softmax":
                nq = torch.min(t1, t2).view(-1, group, 1)
                T = (nq * torch.softmax(beta * nq, 1)).sum(1)
            else:
                T = torch.min(t1.view(-1, group, 1).max(1)[0], t2.view(-1, group, 1).max(1)[0]) if group > 1 else torch.min(t1, t2)
        return (rew + (1 - done) * discount * T).detach()


def td_step(critic, target, optim, obs, act, rew, next_obs, done, next_act=None, *, discount: float, group: int = 1,
            reduce: str = "min", beta: Optional[float] = None, default: Optional[bool] = None) -> dict:
    """One TD step of the double-Q `critic` (``DQLCritic`` or ``TwinQ``): ``y = rew + discount (1 - done) T`` from the frozen `target`
    (``td_target``), ``loss = mse(q1, y) + mse(q2, y)``, ``optim.zero_grad()``, backward, ``optim.step()``.  `next_act`: (R * group,
    act_dim), row ``r * group + j`` the j-th candidate of transition r.  `default`: take the fused launch without being asked (None:
    ``FUSED_BY_DEFAULT``).  -> {"loss", "target_mean"}."""
    from ..engine import critic_step
    if reduce not in REDUCTIONS or (reduce == "min" and group != 1) or (reduce == "softmax" and beta is None):
        raise ValueError(f"td_step: reduce = {reduce!r} with group = {group}, beta = {beta}")
    if not isinstance(critic, (DQLCritic, TwinQ)):
        raise TypeError("td_step: `critic` is a DQLCritic or a TwinQ")
    if (next_act is None) != isinstance(target, V) or _towers(target) is None:
        raise TypeError("td_step: `target` is a V (without next_act) or a DQLCritic / TwinQ (with next_act)")
    if default is None:
        default = FUSED_BY_DEFAULT["td" if group == 1 else "td_grouped"]
    rows = obs.shape[0] if torch.is_tensor(obs) and obs.dim() == 2 else -1
    r, d = _column(rew, rows), _column(done, rows)
    if r is not None and d is not None:
        out = critic_step.try_step(_towers(critic), _towers(target), optim, obs, act, next_obs, next_act, r, d, group=group, reduce=reduce,
                                   loss="mse", discount=discount, beta=beta or 0.0, default=default)
        if out is not None:
            optim.step()
            return out
    y = td_target(target, rew, next_obs, done, next_act, discount=discount, group=group, reduce=reduce, beta=beta)
    q1, q2 = _both(critic, obs, act)
    loss = F.mse_loss(q1, y) + F.mse_loss(q2, y)
    optim.zero_grad()
    loss.backward()
    optim.step()
    return {"loss": loss.detach(), "target_mean": y.mean()}


def expectile_step(v, q_target, optim, obs, act, *, tau: float, default: Optional[bool] = None) -> dict:
    """IQL's expectile step of `v` (``V``) against the frozen double-Q `q_target`: ``adv = min(q_target(obs, act)) - v(obs)``,
    ``loss = mean(|tau - 1[adv < 0]| adv^2)``, ``optim.zero_grad()``, backward, ``optim.step()``.  -> {"loss", "target_mean"}."""
    from ..engine import critic_step
    if not isinstance(v, V) or not isinstance(q_target, (DQLCritic, TwinQ)):
        raise TypeError("expectile_step: `v` is a V, `q_target` a DQLCritic or a TwinQ")
    out = critic_step.try_step(_towers(v), _towers(q_target), optim, obs, None, obs, act, None, None, reduce="min", loss="expectile", tau=tau,
                               default=FUSED_BY_DEFAULT["expectile"] if default is None else default)
    if out is not None:
        optim.step()
        return out
    with torch.no_grad():
        qt = torch.min(*_both(q_target, obs, act))
    adv = qt - v(obs)
    loss = (torch.abs(tau - (adv < 0).float()) * adv ** 2).mean()
    optim.zero_grad()
    loss.backward()
    optim.step()
    return {"loss": loss.detach(), "target_mean": qt.mean()}
