"""The critic steps of the shipped training loops, written once for the fixture generator (tools/gen_critic_golden.py: the real reference on
the CPU), the GPU tests (this package on the device) and tools/bench_tower.py:

* the IDQL pipeline's inline IQL half-step (reference pipelines/idql_d4rl_mujoco.py:84-107): the expectile step of ``IDQLVNet`` against the
  frozen target ``IDQLQNet``, the TD step of ``IDQLQNet.both``, the Polyak update of the target;
* the Diffusion-QL critic step (reference pipelines/dql_d4rl_mujoco.py:80-94): two MSE terms of ``DQLCritic`` against the frozen target critic
  on the next action.

Weights are ``load_synth`` streams, batches are seeded: nothing but the recorded results is stored."""
import importlib
import os
from copy import deepcopy
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "critic_towers.npz")
STEPS, LR, TAU, DISCOUNT = 3, 3e-4, 0.7, 0.99
# (obs, act, hidden, batch): a ragged last tile of 16 rows in both, K0 = 14 (no multiple of 4) and 23 (the shipped 17 + 6)
CASES = {"o11_a3_h32_b24": SimpleNamespace(obs=11, act=3, hidden=32, batch=24),
         "o17_a6_h64_b40": SimpleNamespace(obs=17, act=6, hidden=64, batch=40)}
TABLE = list(CASES)


def utils_of(kind: str):
    """The ``utils`` package of this repository ("amd") or of the real reference ("reference")."""
    if kind == "amd":
        return importlib.import_module("cleandiffuser_amd.utils")
    from oracle.ref_import import import_reference
    import_reference()
    return importlib.import_module("cleandiffuser.utils")


def synth(module, seed):
    from cleandiffuser_amd.utils.synth import synth_state_dict
    module.load_state_dict(synth_state_dict(module.state_dict(), seed))
    return module


def batches(case, device="cpu", seed=7):
    """STEPS batches of (obs, act, rew, next_obs, done, next_act); about a third of the transitions are terminal."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(STEPS):
        b = [torch.randn(case.batch, case.obs, generator=g), torch.randn(case.batch, case.act, generator=g).tanh(),
             torch.randn(case.batch, 1, generator=g), torch.randn(case.batch, case.obs, generator=g),
             (torch.rand(case.batch, 1, generator=g) < 0.3).float(), torch.randn(case.batch, case.act, generator=g).tanh()]
        out.append([t.to(device) for t in b])
    return out


def checksums(module) -> np.ndarray:
    """(n_parameters, 2): mean and mean |.| of every parameter."""
    return np.array([[float(p.detach().double().mean()), float(p.detach().double().abs().mean())] for p in module.parameters()])


def _grads(module, prefix):
    return {f"{prefix}{n}": p.grad.detach().cpu().numpy().copy() for n, p in module.named_parameters()}


def iql_nets(U, case, device="cpu"):
    q = synth(U.IDQLQNet(case.obs, case.act, hidden_dim=case.hidden), 31).to(device)
    v = synth(U.IDQLVNet(case.obs, hidden_dim=case.hidden), 32).to(device)
    q_targ = deepcopy(q).requires_grad_(False).eval()
    return q.train(), q_targ, v.train()


def iql_half_step(q, q_targ, v, q_optim, v_optim, batch, polyak, on_grads=None):
    """One IQL half-step of the IDQL pipeline -> (v_loss, q_loss) as tensors; `on_grads(name)` is called after each backward pass."""
    obs, act, rew, next_obs, tml, _ = batch
    qt, val = q_targ(obs, act), v(obs)
    v_loss = (torch.abs(TAU - ((qt - val) < 0).float()) * (qt - val) ** 2).mean()
    v_optim.zero_grad()
    v_loss.backward()
    if on_grads:
        on_grads("V")
    v_optim.step()
    with torch.no_grad():
        td_target = rew + DISCOUNT * (1 - tml) * v(next_obs)
    q1, q2 = q.both(obs, act)
    q_loss = ((q1 - td_target) ** 2 + (q2 - td_target) ** 2).mean()
    q_optim.zero_grad()
    q_loss.backward()
    if on_grads:
        on_grads("Q")
    q_optim.step()
    polyak(q, q_targ)
    return v_loss.detach(), q_loss.detach()


def stock_polyak(q, q_targ):
    for param, target_param in zip(q.parameters(), q_targ.parameters()):
        target_param.data.copy_(0.995 * param.data + (1 - 0.995) * target_param.data)


def run_iql(U, case, device="cpu", adam=torch.optim.Adam, polyak=stock_polyak) -> dict:
    q, q_targ, v = iql_nets(U, case, device)
    q_optim, v_optim = adam(q.parameters(), lr=LR), adam(v.parameters(), lr=LR)
    out, losses, seen = {}, [], set()

    def first_grads(which):
        if which not in seen:
            seen.add(which)
            out.update(_grads(v if which == "V" else q, f"iql/grad/{which}."))
    for batch in batches(case, device):
        losses.append([float(l) for l in iql_half_step(q, q_targ, v, q_optim, v_optim, batch, polyak, first_grads)])
    out["iql/loss"] = np.array(losses, dtype=np.float64)
    for name, m in (("Q", q), ("V", v), ("Q_targ", q_targ)):
        out[f"iql/sums/{name}"] = checksums(m)
    return out


def dql_nets(U, case, device="cpu"):
    critic = synth(U.DQLCritic(case.obs, case.act, hidden_dim=case.hidden), 33).to(device)
    return critic.train(), deepcopy(critic).requires_grad_(False).eval()


def dql_critic_step(critic, critic_target, optim, batch, on_grads=None):
    obs, act, rew, next_obs, tml, next_act = batch
    current_q1, current_q2 = critic(obs, act)
    target_q = torch.min(*critic_target(next_obs, next_act))
    target_q = (rew + (1 - tml) * DISCOUNT * target_q).detach()
    critic_loss = F.mse_loss(current_q1, target_q) + F.mse_loss(current_q2, target_q)
    optim.zero_grad()
    critic_loss.backward()
    if on_grads:
        on_grads()
    optim.step()
    return critic_loss.detach()


def run_dql(U, case, device="cpu", adam=torch.optim.Adam) -> dict:
    critic, critic_target = dql_nets(U, case, device)
    optim = adam(critic.parameters(), lr=LR)
    out, losses = {}, []

    def first_grads():
        if not out:
            out.update(_grads(critic, "dql/grad/"))
    for batch in batches(case, device):
        losses.append(float(dql_critic_step(critic, critic_target, optim, batch, first_grads)))
    out["dql/loss"] = np.array(losses, dtype=np.float64)
    out["dql/sums"] = checksums(critic)
    return out


def golden(name: str) -> dict:
    with np.load(GOLDEN) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
