"""The cases the fused critic-step tests share (engine/critic_step.py, csrc/cdx_critic_step.hip): small on purpose -- the largest case
has 33 live rows, the grouped ones at most 272 target rows.  Every case builds its live and target towers (stock ``nn.Sequential``
modules, tests/tower_cases.py) and its batch from seeds.  ``autograd_reference`` is the float64 reference: the pipelines' inline step
written with torch ops on those modules (reference pipelines/dql_d4rl_mujoco.py:80-94, dql_d4rl_antmaze.py:88-94, qgpo_d4rl_mujoco.py:141-148,
utils/iql.py:62-84) and differentiated by autograd.  ``rel_err`` is the error measure: max |a - b| / max |b|."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_cases as tc  # noqa: E402

DISCOUNT = 0.99


def _c(rows, a0, a1, live, live_acts, live_towers, b0, b1, target, target_acts, target_towers, group=1, reduce="min", loss="mse", tau=0.5,
       beta=0.0, done="mixed", q_scale=1.0):
    """`a0`, `a1`: the live rows are [x0 | x1]; `b0`, `b1`: the target rows [z0 | z1], `group` rows of z1 per live row; `done`: "zeros",
    "ones", "mixed", or None (no reward: y = T, IQL's V step); `q_scale`: what the target's last Linear is multiplied by."""
    return SimpleNamespace(rows=rows, a0=a0, a1=a1, live=list(live), live_acts=list(live_acts), live_towers=live_towers, b0=b0, b1=b1,
                           target=list(target), target_acts=list(target_acts), target_towers=target_towers, group=group, reduce=reduce,
                           loss=loss, tau=tau, beta=beta, done=done, q_scale=q_scale)


_DQL, _IQL = ["tanh", "mish", "mish", None], ["mish", "mish", None]
CASES = {
    # rows 1 / 16 / 17 / 33; K0 14 and 23 (no multiples of 4); hidden 32 and 64; twin and single live towers
    "dql_r17_k23_h32": _c(17, 17, 6, [32, 32, 32, 1], _DQL, 2, 17, 6, [32, 32, 32, 1], _DQL, 2),
    "iql_q_r16_k14_h32_done0": _c(16, 11, 3, [32, 32, 1], _IQL, 2, 11, 0, [32, 32, 1], _IQL, 1, done="zeros"),       # a V target: K0 11, not 14
    "iql_q_r33_k23_h64": _c(33, 17, 6, [64, 64, 1], _IQL, 2, 17, 0, [64, 64, 1], _IQL, 1),
    "single_r1_k14_done1": _c(1, 11, 3, [32, 32, 1], _IQL, 1, 11, 3, [32, 32, 1], _IQL, 2, done="ones"),
    "iql_v_r33_tau07_h64": _c(33, 17, 0, [64, 64, 1], _IQL, 1, 17, 6, [64, 64, 1], _IQL, 2, loss="expectile", tau=0.7, done=None),
    "iql_v_r17_tau05_h32": _c(17, 11, 0, [32, 32, 1], _IQL, 1, 11, 3, [32, 32, 1], _IQL, 2, loss="expectile", tau=0.5, done=None),
    # the grouped targets: K = 10 with target rows crossing tiles (R = 5: 50 rows) and with two live tiles, K = 16, the softmax uneven
    "antmaze_k10_r5": _c(5, 11, 3, [32, 32, 32, 1], _DQL, 2, 11, 3, [32, 32, 32, 1], _DQL, 2, group=10, reduce="max"),
    "antmaze_k10_r17": _c(17, 17, 6, [32, 32, 32, 1], _DQL, 2, 17, 6, [32, 32, 32, 1], _DQL, 2, group=10, reduce="max"),
    "qgpo_k16_r3_beta3": _c(3, 11, 3, [32, 32, 1], _IQL, 2, 11, 3, [32, 32, 1], _IQL, 2, group=16, reduce="softmax", beta=3.0, q_scale=3.0),
    "qgpo_k16_r17_beta3": _c(17, 17, 6, [64, 64, 1], _IQL, 2, 17, 6, [64, 64, 1], _IQL, 2, group=16, reduce="softmax", beta=3.0, q_scale=3.0),
    # unequal widths; one 512-wide layer
    "unequal_r33": _c(33, 17, 6, [32, 48, 16, 1], ["silu", "relu", "mish", None], 2, 17, 6, [48, 32, 1], _IQL, 2),
    "wide512_r17": _c(17, 11, 3, [512, 1], ["tanh", None], 2, 11, 3, [32, 32, 1], _IQL, 2),
}
# the edges of what critic_plan admits (K0 <= 512, widths <= 512, K <= 16, LDS <= 160 KiB)
_W512 = ["tanh", None]
ENVELOPE = {
    # the kitchen DQLCritic (obs 60 + act 9), live and target: five K blocks with a ragged end, scalar weight loads, 83 KiB of LDS
    "kitchen_r17_k69": _c(17, 60, 9, [256, 256, 256, 1], _DQL, 2, 60, 9, [256, 256, 256, 1], _DQL, 2),
    # the widest input and the widest layer, A1 = 64: 32 K blocks, both sweeps of the product, 98 KiB of LDS
    "widest_r17_k512": _c(17, 448, 64, [512, 1], _W512, 2, 448, 64, [512, 1], _W512, 2),
    # the grouped target at the kitchen sizes
    "kitchen_antmaze_k10_r17": _c(17, 60, 9, [256, 256, 256, 1], _DQL, 2, 60, 9, [256, 256, 256, 1], _DQL, 2, group=10, reduce="max"),
    # a partial second sweep (272 = 17 column tiles) over K0 = 85, a single live tower on a V-like target
    "sweep272_r33_k85": _c(33, 76, 9, [272, 272, 1], _IQL, 1, 76, 0, [272, 1], ["mish", None], 1),
}
CASES.update(ENVELOPE)
TABLE = list(CASES)
ALL_ZERO_GRADS: dict = {}          # case -> names of gradients that are identically zero by construction (none in this table)


def build(case, dtype=torch.float32, device="cpu"):
    """(live towers, target towers) as stock ``nn.Sequential`` modules; the target is frozen."""
    live = tc.build(tc._c(case.rows, case.a0 + case.a1, case.live, case.live_acts, towers=case.live_towers), seed=3, dtype=dtype, device=device)
    target = tc.build(tc._c(case.rows, case.b0 + case.b1, case.target, case.target_acts, towers=case.target_towers, frozen=True), seed=5,
                      dtype=dtype, device=device)
    with torch.no_grad():
        for seq in target:
            seq[-1].weight.mul_(case.q_scale)
    return live, target


def make_inputs(case, seed=13, dtype=torch.float32, device="cpu") -> SimpleNamespace:
    """x0 (R, a0), x1 (R, a1) or None, z0 (R, b0), z1 (R * group, b1) or None, rew / done (R, 1) or None."""
    g = torch.Generator().manual_seed(seed)
    n = case.rows
    rand = lambda *s: torch.randn(*s, generator=g)                # noqa: E731
    scale = lambda r: 0.2 + 1.8 * torch.rand(r, 1, generator=g)   # noqa: E731
    inp = SimpleNamespace(x0=rand(n, case.a0) * scale(n), x1=rand(n, case.a1).tanh() if case.a1 else None, z0=rand(n, case.b0) * scale(n),
                          z1=rand(n * case.group, case.b1).tanh() if case.b1 else None, rew=None, done=None)
    if case.done is not None:
        inp.rew = rand(n, 1)
        inp.done = {"zeros": torch.zeros(n, 1), "ones": torch.ones(n, 1), "mixed": (torch.arange(n)[:, None] % 3 == 1).float()}[case.done]
    for k, v in vars(inp).items():
        if v is not None:
            setattr(inp, k, v.to(device=device, dtype=dtype))
    return inp


def request(cs, case, live, target, inp):
    """The request object of engine/critic_step.py for these towers and this batch."""
    from cleandiffuser_amd.engine import tower
    descs = cs.describe(live, target)
    assert descs is not None
    dls, dts = descs
    weights = lambda ds: [[p.detach() for p in tower.params_of(d)] for d in ds]      # noqa: E731
    q = cs.make_request(dls[0], weights(dls), dts[0], weights(dts), inp.x0, inp.x1, inp.z0, inp.z1, inp.rew, inp.done, group=case.group,
                        reduce=case.reduce, loss=case.loss, discount=DISCOUNT, beta=case.beta, tau=case.tau)
    assert cs.shapes_ok(q)
    return q


def inline_target(case, target, inp):
    """The pipelines' own target expressions -> (y (R, 1), the towers' minimum or per-tower values (R, group))."""
    with torch.no_grad():
        z0 = inp.z0.unsqueeze(1).repeat(1, case.group, 1).view(-1, case.b0)
        rows = z0 if inp.z1 is None else torch.cat([z0, inp.z1], -1)
        outs = [seq(rows) for seq in target]
        if case.reduce == "softmax":           # qgpo_d4rl_mujoco.py:141-144
            next_q = torch.min(*outs).view(-1, case.group, 1) if len(outs) == 2 else outs[0].view(-1, case.group, 1)
            T = (next_q * torch.softmax(case.beta * next_q, 1)).sum(1)
            picks = next_q[:, :, 0].argmax(1)
        else:                                  # dql_d4rl_antmaze.py:88-91; group == 1: dql_d4rl_mujoco.py:84, utils/iql.py:63, :72
            tops = [o.view(-1, case.group, 1).max(1) for o in outs]
            T = torch.min(tops[0][0], tops[1][0]) if len(outs) == 2 else tops[0][0]
            picks = tops[0][1][:, 0]
        y = T if inp.rew is None else inp.rew + (1 - inp.done) * DISCOUNT * T
    return y, picks


def autograd_reference(case, dtype=torch.float64) -> dict:
    """The inline step in `dtype` on the CPU -> y (R), loss, q per tower (R), advantage signs, the group's picks, and the gradient of
    every live parameter per tower in the order of ``tower.params_of``."""
    live, target = build(case, dtype=dtype)
    inp = make_inputs(case, dtype=dtype)
    y, picks = inline_target(case, target, inp)
    x = inp.x0 if inp.x1 is None else torch.cat([inp.x0, inp.x1], -1)
    qs = [seq(x) for seq in live]
    if case.loss == "expectile":               # utils/iql.py:63-64
        adv = y - qs[0]
        loss = (torch.abs(case.tau - (adv < 0).to(dtype)) * adv ** 2).mean()
    else:
        loss = sum(F.mse_loss(q, y) for q in qs)
    loss.backward()
    return {"y": y[:, 0].detach(), "loss": loss.detach(), "q": [q[:, 0].detach() for q in qs], "picks": picks,
            "adv": (y - qs[0]).detach()[:, 0], "grads": [[p.grad.detach() for p in seq.parameters()] for seq in live]}


def rel_err(got, ref) -> float:
    """max |got - ref| / max |ref| (0 / 0 = 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    return err / top if top > 0 else err


def buffers(q) -> dict:
    """name -> tensor of everything the launch writes; the gradient buffers times R (dq carries 1 / R)."""
    lv, out = q.live, {"y": q.y, "y_part": q.y_part, "loss_part": q.loss_part, "x_cat": q.x_cat}
    for t in range(lv.n_towers):
        out[f"q[{t}]"] = lv.out[t]
        for l, norm in enumerate(lv.norm):
            if l < len(lv.width) - 1:
                out[f"H[{t}][{l}]"] = lv.H[t][l]
            out[f"G[{t}][{l}]"] = lv.G[t][l] * q.R
            if norm:
                out[f"Sb[{t}][{l}]"], out[f"Sg[{t}][{l}]"] = lv.Sb[t][l] * q.R, lv.Sg[t][l] * q.R
    return out


# ------------------------------------------------------------------------------------------------------------------- #
# The grouped critic steps of the shipped loops, written once for the fixture generator (tools/gen_critic_step_golden.py: the real    #
# reference on the CPU) and the GPU tests (this package on the device)                                                        #
# ------------------------------------------------------------------------------------------------------------------- #
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "critic_steps_grouped.npz")
GROUPED = {"antmaze_k10": SimpleNamespace(kind="antmaze", obs=11, act=3, hidden=32, batch=24, group=10, beta=None),
           "qgpo_k16_beta3": SimpleNamespace(kind="qgpo", obs=17, act=6, hidden=64, batch=40, group=16, beta=3.0)}


def grouped_batches(case, device="cpu"):
    """``critic_steps.batches`` with next_act (batch * group, act): row r * group + j is candidate j of transition r."""
    import critic_steps as cs
    g = torch.Generator().manual_seed(19)
    out = []
    for b in cs.batches(case, "cpu"):
        b[5] = torch.randn(case.batch * case.group, case.act, generator=g).tanh()
        out.append([t.to(device) for t in b])
    return out


def grouped_nets(U, case, device="cpu"):
    import critic_steps as cs
    from copy import deepcopy
    cls = U.DQLCritic if case.kind == "antmaze" else U.IDQLQNet
    critic = cs.synth(cls(case.obs, case.act, hidden_dim=case.hidden), 35).to(device)
    target = deepcopy(critic).requires_grad_(False).eval()
    with torch.no_grad():                                    # (a target that has drifted from the critic, and whose values spread)
        for p in target.parameters():
            p.mul_(1.5 if p.dim() == 2 and p.shape[0] == 1 else 1.02)
    return critic.train(), target


def grouped_inline_step(case, critic, target, optim, batch):
    """The pipelines' inline step (reference pipelines/dql_d4rl_antmaze.py:79-98, qgpo_d4rl_mujoco.py:141-152) -> (loss, mean of y)."""
    import critic_steps as cs
    obs, act, rew, next_obs, tml, next_act = batch
    K = case.group
    if case.kind == "antmaze":
        current_q1, current_q2 = critic(obs, act)
        next_obs_rpt = next_obs.unsqueeze(1).repeat(1, K, 1).view(-1, case.obs)
        target_q1, target_q2 = target(next_obs_rpt, next_act)
        target_q1 = target_q1.view(-1, K, 1).max(1)[0]
        target_q2 = target_q2.view(-1, K, 1).max(1)[0]
        target_q = torch.min(target_q1, target_q2)
        target_q = (rew + (1 - tml) * cs.DISCOUNT * target_q).detach()
        loss = F.mse_loss(current_q1, target_q) + F.mse_loss(current_q2, target_q)
    else:
        with torch.no_grad():
            next_q = target(next_obs.unsqueeze(1).repeat(1, K, 1), next_act.view(-1, K, case.act))
            weight = torch.softmax(case.beta * next_q, 1)
            target_q = rew + cs.DISCOUNT * (1 - tml) * (next_q * weight).sum(1)
        q1, q2 = critic.both(obs, act)
        loss = ((q1 - target_q) ** 2 + (q2 - target_q) ** 2).mean()
    optim.zero_grad()
    loss.backward()
    optim.step()
    return loss.detach(), target_q.mean()


def grouped_call_step(case, critic, target, optim, batch):
    """The same step through ``utils.critic_steps.td_step``."""
    import critic_steps as cs
    from cleandiffuser_amd.utils.critic_steps import td_step
    obs, act, rew, next_obs, tml, next_act = batch
    kw = dict(reduce="max") if case.kind == "antmaze" else dict(reduce="softmax", beta=case.beta)
    out = td_step(critic, target, optim, obs, act, rew, next_obs, tml, next_act, discount=cs.DISCOUNT, group=case.group, **kw)
    return out["loss"], out["target_mean"]


def run_grouped(U, case, device="cpu", adam=torch.optim.Adam, step=grouped_inline_step) -> dict:
    """STEPS steps -> the losses and means of y of every step, the first step's gradients, the parameter checksums after the last."""
    import critic_steps as cs
    critic, target = grouped_nets(U, case, device)
    optim = adam(critic.parameters(), lr=cs.LR)
    out, rows = {}, []
    for i, batch in enumerate(grouped_batches(case, device)):
        rows.append([float(v) for v in step(case, critic, target, optim, batch)])
        if i == 0:
            out.update(cs._grads(critic, "grad/"))
    out["loss"] = np.array(rows, dtype=np.float64)
    out["sums"] = cs.checksums(critic)
    return out


def grouped_golden(name: str) -> dict:
    with np.load(GOLDEN) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


# the steps of tests/critic_steps.py made through the calls of utils/critic_steps.py
def run_iql_calls(U, case, device="cpu", adam=torch.optim.Adam, polyak=None) -> dict:
    """``critic_steps.run_iql`` with the two half-steps made through ``expectile_step`` / ``td_step``."""
    import critic_steps as cs
    from cleandiffuser_amd.utils import critic_steps
    q, q_targ, v = cs.iql_nets(U, case, device)
    q_optim, v_optim = adam(q.parameters(), lr=cs.LR), adam(v.parameters(), lr=cs.LR)
    out, losses = {}, []
    for i, (obs, act, rew, next_obs, tml, _) in enumerate(cs.batches(case, device)):
        lv = critic_steps.expectile_step(v, q_targ, v_optim, obs, act, tau=cs.TAU)["loss"]
        if i == 0:
            out.update(cs._grads(v, "iql/grad/V."))
        lq = critic_steps.td_step(q, v, q_optim, obs, act, rew, next_obs, tml, discount=cs.DISCOUNT)["loss"]
        if i == 0:
            out.update(cs._grads(q, "iql/grad/Q."))
        (polyak or cs.stock_polyak)(q, q_targ)
        losses.append([float(lv), float(lq)])
    out["iql/loss"] = np.array(losses, dtype=np.float64)
    for name, m in (("Q", q), ("V", v), ("Q_targ", q_targ)):
        out[f"iql/sums/{name}"] = cs.checksums(m)
    return out


def run_dql_calls(U, case, device="cpu", adam=torch.optim.Adam) -> dict:
    """``critic_steps.run_dql`` with the step made through ``td_step``."""
    import critic_steps as cs
    from cleandiffuser_amd.utils import critic_steps
    critic, critic_target = cs.dql_nets(U, case, device)
    optim = adam(critic.parameters(), lr=cs.LR)
    out, losses = {}, []
    for i, (obs, act, rew, next_obs, tml, next_act) in enumerate(cs.batches(case, device)):
        losses.append(float(critic_steps.td_step(critic, critic_target, optim, obs, act, rew, next_obs, tml, next_act, discount=cs.DISCOUNT)["loss"]))
        if i == 0:
            out.update(cs._grads(critic, "dql/grad/"))
    out["dql/loss"] = np.array(losses, dtype=np.float64)
    out["dql/sums"] = cs.checksums(critic)
    return out


def sizes_request(critic_step, live, target, K=1):
    """A ``CdxCriticStep`` of sizes alone (every pointer null) for `live` / `target` = (K0, widths): what the C side's size checks and
    LDS plan read."""
    import ctypes
    mk = lambda k0, widths: critic_step.CdxCriticNet(K0=k0, n_towers=2, n_layers=len(widths), width=(ctypes.c_int32 * 6)(*widths),   # noqa: E731
                                                     act=(ctypes.c_int32 * 6)(), norm=(ctypes.c_int32 * 6)())
    return critic_step.CdxCriticStep(R=40, K=K, A0=live[0], A1=0, B0=target[0] - 1, B1=1, reduce=1, loss=0, live=mk(*live), target=mk(*target))
