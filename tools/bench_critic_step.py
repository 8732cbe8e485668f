"""A/B of the critics' training steps on one device: the fused step (engine/critic_step.py, ``CDX_CRITIC_STEP=1``) against the parent
routes (``CDX_CRITIC_STEP=0``: the eager sequence over the fused towers or the library nodes), alternating in one process.

    python tools/bench_critic_step.py [--batch 256] [--iters 400] [--rounds 5] [--out profiles/critic_step_ab.txt]

The shipped sizes (obs 17, act 6, hidden 256, B = 256), synthetic weights, FusedAdam, the steps through ``utils.critic_steps``:

1. the IDQL pipeline's IQL half-step (expectile step of V against the frozen twin Q, TD step of the twin Q against V, Polyak update);
2. the Diffusion-QL critic step plus the Q term of the policy step through the frozen critic (a gradient to the action only);
3. the Diffusion-QL antmaze critic step: the max-Q backup over K = 10 sampled next actions;
4. the QGPO critic step: the softmax-weighted target over K = 16 support actions.

Routes: "fused" (CDX_CRITIC_STEP=1), "parent" (CDX_CRITIC_STEP=0, CDX_TOWER unset: what the pipelines ran before) and "towers"
(CDX_CRITIC_STEP=0, CDX_TOWER=1: the parent route with every tower call on the fused tower launches).  Wall time of one step with a
device synchronise before and after it; a round times `--iters` steps per route, and every workload first runs `--settle` untimed steps
of every route.  Prints per round the median of every route, then their means, the spread over the rounds, the device kernels of one
steady-state step of each, and the verdict of the default rule against each parent route: the fused step must beat it by more than
the sum of the two spreads."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUTES = {"fused": ("1", None), "parent": ("0", None), "towers": ("0", "1")}        # CDX_CRITIC_STEP, CDX_TOWER


def set_route(route):
    for name, value in zip(("CDX_CRITIC_STEP", "CDX_TOWER"), ROUTES[route]):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=300, help="untimed steps of every route before a workload's first round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import critic_step_cases as cc
    import critic_steps as cs
    from types import SimpleNamespace
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.utils.critic_steps import expectile_step, td_step
    dev = "cuda:0"
    case = SimpleNamespace(obs=17, act=6, hidden=256, batch=a.batch)
    U = cs.utils_of("amd")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def iql_step():
        q, q_targ, v = cs.iql_nets(U, case, dev)
        q_optim, v_optim = FusedAdam(q.parameters(), lr=cs.LR), FusedAdam(v.parameters(), lr=cs.LR)
        obs, act, rew, next_obs, tml, _ = cs.batches(case, dev)[0]

        def step():
            expectile_step(v, q_targ, v_optim, obs, act, tau=cs.TAU)
            td_step(q, v, q_optim, obs, act, rew, next_obs, tml, discount=cs.DISCOUNT)
            cs.stock_polyak(q, q_targ)
        return step

    def dql_step():
        critic, critic_target = cs.dql_nets(U, case, dev)
        optim = FusedAdam(critic.parameters(), lr=cs.LR)
        obs, act, rew, next_obs, tml, next_act = cs.batches(case, dev)[0]
        new_act = act.clone().requires_grad_(True)

        def step():
            td_step(critic, critic_target, optim, obs, act, rew, next_obs, tml, next_act, discount=cs.DISCOUNT)
            critic.requires_grad_(False)                       # (FreezeModules of the pipeline)
            q1, q2 = critic(obs, new_act)
            (-q1.mean() / q2.abs().mean().detach()).backward()
            critic.requires_grad_(True)
            new_act.grad = None
        return step

    def grouped_step(kind, group, beta):
        g = SimpleNamespace(kind=kind, obs=case.obs, act=case.act, hidden=case.hidden, batch=a.batch, group=group, beta=beta)

        def make():
            critic, target = cc.grouped_nets(U, g, dev)
            optim = FusedAdam(critic.parameters(), lr=cs.LR)
            batch = cc.grouped_batches(g, dev)[0]
            return lambda: cc.grouped_call_step(g, critic, target, optim, batch)
        return make

    def timed(step, route):
        set_route(route)
        for _ in range(a.warmup):
            step()
        times = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(times)

    def kernels(step, route):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        set_route(route)
        step()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

    def ab(title, make, routes=("fused", "parent", "towers")):
        steps = {r: make() for r in routes}                      # one set of nets per route: each keeps training on its own weights
        say(title)
        for r in routes:                                         # (clocks, allocator and optimiser state settle: untimed)
            set_route(r)
            for _ in range(a.settle):
                steps[r]()
        ms = {r: [] for r in routes}
        for i in range(a.rounds):
            for r in routes:
                ms[r].append(timed(steps[r], r))
            say(f"  round {i}: " + "   ".join(f"{r} {ms[r][-1]:.3f}" for r in routes))
        spread = {r: max(v) - min(v) for r, v in ms.items()}
        mean = {r: statistics.mean(v) for r, v in ms.items()}
        for r in routes:
            say(f"  {r:7s} mean {mean[r]:.3f}  spread {spread[r]:.3f}  device kernels per step {kernels(steps[r], r)}")
        wins = {}
        for r in routes:
            if r != "fused":
                wins[r] = mean[r] - mean["fused"] > spread["fused"] + spread[r]
                say(f"  fused beats {r} by more than the sum of the spreads: {wins[r]}")
        return wins

    say(f"critic steps, obs 17, act 6, hidden 256, B = {a.batch}, FusedAdam lr 3e-4, {torch.cuda.get_device_name(0)}; median of {a.iters} "
        f"steps after {a.warmup} warm-up steps, {a.settle} untimed steps of every route before a workload's first round, ms (wall time, "
        f"synchronised around the step)")
    ab("1. IQL half-step of the IDQL pipeline", iql_step)
    ab("2. Diffusion-QL critic step + the Q term of the policy step through the frozen critic", dql_step)
    ab("3. Diffusion-QL antmaze critic step, max-Q backup over K = 10 sampled actions", grouped_step("antmaze", 10, None))
    ab("4. QGPO critic step, softmax-weighted target over K = 16 support actions, beta = 3", grouped_step("qgpo", 16, 3.0))
    for name in ("CDX_CRITIC_STEP", "CDX_TOWER"):
        os.environ.pop(name, None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
