"""A/B of the critic steps on one device: the fused towers (engine/tower.py) against the node route as it stood before (CDX_TOWER=0),
alternating in one process.

    python tools/bench_tower.py [--batch 256] [--iters 400] [--rounds 5] [--out profiles/tower_ab.txt]

The shipped sizes (obs 17, act 6, hidden 256, B = 256), synthetic weights, the steps of tests/critic_steps.py:

1. the IDQL pipeline's inline IQL half-step (V step against the frozen target, twin-Q step, Polyak update; FusedAdam);
2. the Diffusion-QL critic step plus the Q term of the policy step through the frozen critic (a gradient to the action only);
3. no-grad ``TwinQ`` evaluation at 256, 4096 and 16 384 rows.

Routes: "default" (CDX_TOWER unset: the fused launches where autograd is on), "all" (CDX_TOWER=1: the no-grad evaluations too) and
"nodes" (CDX_TOWER=0).  Wall time of one step with a device synchronise before and after it; a round times about a second of work per
route (400 steps of ~2 ms: the steps are bound by the host's launches, and shorter windows follow the host's other load), and every
workload first runs `--settle` untimed steps of every route.  Prints per round the median of every route, then their means, the spread
over the rounds, the verdict of the default rule (a fused route must beat the node route by more than the sum of the two spreads) and
the device kernels of one steady-state step of each."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUTES = {"default": None, "all": "1", "nodes": "0"}


def set_route(route):
    if ROUTES[route] is None:
        os.environ.pop("CDX_TOWER", None)
    else:
        os.environ["CDX_TOWER"] = ROUTES[route]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=300, help="untimed steps of every route before a workload's first round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import critic_steps as cs
    from types import SimpleNamespace
    from cleandiffuser_amd.engine.optim import FusedAdam
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
        batch = cs.batches(case, dev)[0]
        return lambda: cs.iql_half_step(q, q_targ, v, q_optim, v_optim, batch, cs.stock_polyak)

    def dql_step():
        critic, critic_target = cs.dql_nets(U, case, dev)
        optim = FusedAdam(critic.parameters(), lr=cs.LR)
        batch = cs.batches(case, dev)[0]
        new_act = batch[1].clone().requires_grad_(True)

        def step():
            cs.dql_critic_step(critic, critic_target, optim, batch)
            critic.requires_grad_(False)                       # (FreezeModules of the pipeline)
            q1, q2 = critic(batch[0], new_act)
            (-q1.mean() / q2.abs().mean().detach()).backward()
            critic.requires_grad_(True)
            new_act.grad = None
        return step

    def eval_step(rows):
        q = cs.synth(U.IDQLQNet(case.obs, case.act, hidden_dim=case.hidden), 31).to(dev).eval()
        g = torch.Generator().manual_seed(3)
        obs, act = torch.randn(rows, case.obs, generator=g).to(dev), torch.randn(rows, case.act, generator=g).to(dev)

        def step():
            with torch.no_grad():
                q(obs, act)
        return step

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

    def ab(title, make, routes):
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
        for r in routes:
            say(f"  {r:8s} mean {statistics.mean(ms[r]):.3f}  spread {spread[r]:.3f}  device kernels per step {kernels(steps[r], r)}")
        wins = {}
        for r in routes:
            if r != "nodes":
                wins[r] = statistics.mean(ms["nodes"]) - statistics.mean(ms[r]) > spread[r] + spread["nodes"]
                say(f"  {r} beats the node route by more than the sum of the spreads: {wins[r]}")
        return wins

    say(f"critic steps, obs 17, act 6, hidden 256, B = {a.batch}, FusedAdam lr 3e-4, {torch.cuda.get_device_name(0)}; median of {a.iters} "
        f"steps after {a.warmup} warm-up steps, {a.settle} untimed steps of every route before a workload's first round, ms (wall time, "
        f"synchronised around the step)")
    ab("1. IQL half-step of the IDQL pipeline", iql_step, ("default", "all", "nodes"))
    ab("2. Diffusion-QL critic step + the Q term of the policy step through the frozen critic", dql_step, ("default", "all", "nodes"))
    from cleandiffuser_amd.engine import tower
    say(f"(NOGRAD_MAX_ROWS as shipped: {tower.NOGRAD_MAX_ROWS}; lifted for the measurement below)")
    tower.NOGRAD_MAX_ROWS = 1 << 30
    for rows in (256, 4096, 16384):
        ab(f"3. no-grad TwinQ evaluation, {rows} rows", lambda rows=rows: eval_step(rows), ("all", "nodes"))
    os.environ.pop("CDX_TOWER", None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
