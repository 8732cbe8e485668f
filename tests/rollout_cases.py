"""TEST HELPER for the differentiable rollout (engine/rollout.py): the cases, and for each ONE float64 CPU run of the package's own host
loop (``BaseDiffusionSDE._run_plan_torch``) under torch.autograd -- the reference both tests/test_rollout_cpu.py and
tests/test_gpu_rollout.py compare with.  Computed once per process and never modified."""
import contextlib
import functools
from types import SimpleNamespace

import torch

from oracle import cases as _cases

TIE = 1e-4          # |P_raw - bound| < TIE * (1 + |bound|): the clamp decision may flip between two fp32 evaluations


def _c(net, seed, b, s, solver, predict_noise, bound, mask=True):
    return SimpleNamespace(net=net, seed=seed, B=b, S=s, solver=solver, predict_noise=predict_noise, bound=bound, mask=mask)


DQL, DV16, DV48 = ("DQLMlp", 11, 6, 16, None), ("DVInvMlp", 5, 3, 16, 16), ("DVInvMlp", 5, 3, 16, 48)

# (the bounds of the deterministic eps solvers and of x0-prediction are the ones at which the clamp takes between 5 % and 95 % of the
#  elements in some step: +-1 clamps 96-99 % / nothing there)
CASES = {
    # every solver the rollout takes x both prediction types, one action column fixed by the mask
    "dql_ddpm_eps": _c(DQL, 65, 256, 5, "ddpm", True, 1.0),
    "dql_sde1_eps": _c(DQL, 65, 256, 5, "sde_dpmsolver_1", True, 1.0),
    "dql_ddim_eps": _c(DQL, 65, 256, 5, "ddim", True, 2.5),
    "dql_ode1_eps": _c(DQL, 65, 256, 5, "ode_dpmsolver_1", True, 2.5),
    "dql_odepp1_eps": _c(DQL, 65, 256, 5, "ode_dpmsolver++_1", True, 2.5),
    "dql_sdepp1_eps": _c(DQL, 65, 256, 5, "sde_dpmsolver++_1", True, 1.0),
    "dql_ddpm_x0": _c(DQL, 65, 256, 5, "ddpm", False, 0.25),
    "dql_ddim_x0": _c(DQL, 65, 256, 5, "ddim", False, 0.25),
    "dql_sdepp1_x0": _c(DQL, 65, 256, 5, "sde_dpmsolver++_1", False, 0.25),
    "dql_sde1_x0": _c(DQL, 65, 256, 5, "sde_dpmsolver_1", False, 1.0),
    "dql_ode1_x0": _c(DQL, 65, 256, 5, "ode_dpmsolver_1", False, 0.25),
    "dql_odepp1_x0": _c(DQL, 65, 256, 5, "ode_dpmsolver++_1", False, 0.25),
    # the inverse-dynamics net at two widths, no mask
    "dv16_ddpm_eps": _c(DV16, 66, 50, 3, "ddpm", True, 1.0, mask=False),
    "dv48_ddpm_eps": _c(DV48, 66, 50, 3, "ddpm", True, 1.0, mask=False),
    "dv48_ddpm_x0": _c(DV48, 66, 50, 3, "ddpm", False, 0.25, mask=False),
}
TABLE = list(CASES)

# ragged and degenerate shapes (GPU): one row, a ragged second tile, one action, one step, widths of 1 / 3 / 16 column tiles
SHAPES = {
    "b1_a1_w16_s1": _c(("DVInvMlp", 4, 1, 16, 16), 67, 1, 1, "ddpm", False, 0.25, mask=False),
    "b17_a3_w48_s3": _c(("DVInvMlp", 5, 3, 16, 48), 66, 17, 3, "ddpm", True, 1.0),
    "b50_a6_w256_s3": _c(("DVInvMlp", 7, 6, 16, 256), 68, 50, 3, "sde_dpmsolver_1", True, 1.0),
    "b17_a1_w256_s1": _c(("DVInvMlp", 3, 1, 16, 256), 69, 17, 1, "ddim", False, 0.25, mask=False),
    "b1_a6_w48_s3": _c(("DVInvMlp", 5, 6, 16, 48), 70, 1, 3, "sde_dpmsolver++_1", True, 1.0),
    # (not an eps-type one-step solver here: from t = T the cosine schedule has alpha_T = 0.0084, and x <- 118.83 x - 118.81 eps cancels
    #  seven bits -- the fp32 host loop on the CPU is 5e-4 away from float64 in that case, whoever evaluates it)
    "b50_a3_w16_s1": _c(("DVInvMlp", 5, 3, 16, 16), 66, 50, 1, "sde_dpmsolver++_1", False, 0.25, mask=False),
}
CASES.update(SHAPES)

# the edges of what ro_check admits (A <= 64, A + E + O <= 512, W <= 512): more than one trip of the (16 x A) element loops, more than
# one column tile in the head, both sweeps of the product, many K blocks with a ragged end.  Held to float64 on the CPU too (TABLE).
ENVELOPE = {
    # every limit at once: A = 64, E = 128, O = 320 (F = 512), W = 512
    "limits_b17_a64_f512_w512_s2": _c(("DVInvMlp", 160, 64, 128, 512), 81, 17, 2, "ddpm", True, 1.0),
    # a partial second sweep (272 = 17 column tiles), A = 17 (two head tiles), F = 153: ten K blocks through the scalar weight loads
    "b33_a17_w272_s3_ddim": _c(("DVInvMlp", 60, 17, 16, 272), 82, 33, 3, "ddim", True, 2.5),
    # A = 33 under a mask: three trips of the element loops, a ragged third head tile, three K blocks in the transposed head product
    "b17_a33_w48_s3_x0": _c(("DVInvMlp", 5, 33, 16, 48), 84, 17, 3, "ddpm", False, 0.25),
    # the kitchen policy (obs 60, act 9): F = 85, W = 256
    "kitchen_dql_b17_s3": _c(("DQLMlp", 60, 9, 16, None), 85, 17, 3, "ddpm", True, 1.0),
}
CASES.update(ENVELOPE)
TABLE += list(ENVELOPE)


def build(case, lib, device="cpu", dtype=torch.float32):
    """(agent, inputs) of a case on `device`: synthetic weights, IdentityCondition, randn observations, recorded noise."""
    from cleandiffuser_amd.utils import load_synth
    cls, obs, act, emb, hidden = case.net
    net = load_synth(lib.DQLMlp(obs, act, emb_dim=emb) if cls == "DQLMlp" else lib.DVInvMlp(obs, act, emb_dim=emb, hidden_dim=hidden), case.seed)
    net = net.to(device=device, dtype=dtype)
    fm = None
    if case.mask:
        fm = torch.zeros(act, dtype=dtype)
        fm[act - 1] = 1.0
    agent = lib.DiscreteDiffusionSDE(net, lib.IdentityCondition(dropout=0.0), fix_mask=fm, predict_noise=case.predict_noise,
                                     x_max=case.bound * torch.ones(1, act, dtype=dtype), x_min=-case.bound * torch.ones(1, act, dtype=dtype),
                                     diffusion_steps=5, device=device)
    g = torch.Generator().manual_seed(9)
    o = obs if cls == "DQLMlp" else 2 * obs
    inp = SimpleNamespace(
        obs=torch.randn(case.B, o, generator=g, dtype=torch.float64).to(device=device, dtype=dtype),
        noise=[torch.randn(case.B, act, generator=g, dtype=torch.float64).to(device=device, dtype=dtype) for _ in range(case.S + 1)],
        q_w=torch.randn(act, generator=g, dtype=torch.float64).to(device=device, dtype=dtype),
        prior=(0.3 * torch.randn(case.B, act, generator=g, dtype=torch.float64)).to(device=device, dtype=dtype))
    return agent, inp


def sample(agent, case, inp, obs):
    return agent.sample(inp.prior, solver=case.solver, n_samples=case.B, sample_steps=case.S, use_ema=False, temperature=1.0,
                        condition_cfg=obs, w_cfg=1.0, requires_grad=True, noise=list(inp.noise))[0]


def objective(act, inp, weight):
    return -((act * inp.q_w).sum(-1) * weight).sum()


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 CPU run of case `name`: the host loop under torch.autograd.  -> namespace with the actions, d / d obs, d / d temb (S, E),
    every parameter gradient, the request the loop ran (plan, x_T, prior, condition: what ``reference_forward`` needs), the clamped share
    per step, the rows whose clamp decision is a tie and the row weights of the objective (0 for those rows, 1 otherwise)."""
    from cleandiffuser_amd.engine import rollout
    case = CASES[name]
    lib = _cases.lib_namespace("amd")
    with float64_default():
        agent, inp = build(case, lib, "cpu", torch.float64)
        net = agent.model["diffusion"]
        seen = SimpleNamespace(plan=None, xt=None, share=[], temb=[])
        run_plan, clip = agent._run_plan_torch, agent.clip_prediction

        def spy_plan(plan, xt, *a, **k):
            seen.plan, seen.xt = plan, xt.detach().clone()
            return run_plan(plan, xt, *a, **k)

        def spy_clip(pred, xt, alpha, sigma):
            out = clip(pred, xt, alpha, sigma)
            seen.share.append(float((out != pred).double().mean()))
            return out

        def keep_temb(mod, args, out):
            if out.requires_grad:
                out.retain_grad()
                seen.temb.append(out)
        agent._run_plan_torch, agent.clip_prediction = spy_plan, spy_clip
        hook = net.time_mlp.register_forward_hook(keep_temb)

        def run(weight):
            seen.share, seen.temb = [], []
            agent.model.zero_grad(set_to_none=True)
            obs = inp.obs.clone().requires_grad_(True)
            act = sample(agent, case, inp, obs)
            objective(act, inp, weight).backward()
            return act.detach(), obs.grad.clone()
        try:
            # the ties come from the rollout's own saved P_raw / X in float64 (compared with this loop's autograd by the CPU test)
            run(torch.ones(case.B))
            q = request(agent, seen.plan, seen.xt, inp, inp.obs)
            rollout.reference_forward(q)
            ties = tie_rows(q)
            weight = torch.where(ties, torch.zeros(case.B), torch.ones(case.B))
            act, g_obs = run(weight)
        finally:
            hook.remove()
            agent._run_plan_torch, agent.clip_prediction = run_plan, clip
        g_temb = torch.stack([t.grad.sum(0) for t in seen.temb])
        grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    return SimpleNamespace(case=case, act=act, g_obs=g_obs, g_temb=g_temb, grads=grads, plan=seen.plan, xt=seen.xt, share=list(seen.share),
                           ties=ties, weight=weight, q0=q)


def request(agent, plan, xt, inp, obs):
    """The rollout request of the loop the agent runs for these inputs (any dtype / device)."""
    from cleandiffuser_amd.engine import rollout
    net = agent.model["diffusion"]
    t = torch.tensor([st.t for st in plan.steps], dtype=torch.long, device=xt.device)
    with torch.no_grad():
        temb = net.time_mlp(net.map_noise(t))
    mid, head = net.mid_layer, net.final_layer
    weights = [p.detach() for m in (mid[0], mid[2], mid[4], head) for p in (m.weight, m.bias)]
    a = xt.shape[1]
    fm = agent.fix_mask.reshape(-1) if torch.is_tensor(agent.fix_mask) else None
    return rollout.make_request(weights, temb, obs.detach(), xt, inp.prior if fm is not None else None, fm, agent.x_min.reshape(a),
                                agent.x_max.reshape(a), torch.stack(inp.noise[1:1 + plan.n_noise]) if plan.n_noise else None, plan.steps,
                                agent.predict_noise, True)


def tie_rows(q):
    """Rows with an element of P_raw closer than TIE * (1 + |bound|) to a clamp bound at some step."""
    from cleandiffuser_amd.engine import rollout
    ties = torch.zeros(q.B, dtype=torch.bool)
    for s, st in enumerate(q.steps):
        for bound in rollout._bounds(q, st, q.X[s]):
            if bound is not None:
                bound = bound.expand_as(q.P_raw[s])
                ties |= ((q.P_raw[s] - bound).abs() < TIE * (1 + bound.abs())).any(-1).cpu()
    return ties
