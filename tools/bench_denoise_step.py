"""A/B of the row-MLP denoising loss outside ``update()`` on one device: the fused node (engine/denoise.py, ``CDX_DENOISE=1``) against the
parent route (``CDX_DENOISE=0``: the per-layer library nodes of ``train.dql_forward`` and ATen around them), alternating in one process.

    python tools/bench_denoise_step.py [--batch 256] [--iters 400] [--rounds 5] [--out profiles/denoise_step_ab.txt]

The shipped EDP / Diffusion-QL sizes: ``DQLMlp(17, 6, emb_dim=64)``, B = 256, ``predict_noise=False``, bounds +-1, synthetic weights.

a. ``actor.loss(act, obs)`` + ``backward()``, with T = 5 and T = 50 diffusion steps;
b. the EDP policy step as the pipeline writes it, optimiser step excluded: ``loss`` + ``approx_action`` + the Q term through a frozen
   ``DQLCritic`` + ``backward()`` (reference pipelines/edp_d4rl_mujoco.py:97-120);
c. workload (b) with its backward pass inside ``train.grads_in_place(actor.model.parameters())``.

Wall time of one step with a device synchronise before and after it; every workload first runs `--settle` untimed steps of both routes,
then a round times `--iters` steps per route.  Prints per round the median of both routes, then their means, the spread over the rounds,
the device kernels of one steady-state step of each, and the verdict of the default rule: the fused route must beat the parent route by
more than the sum of the two spreads."""
import argparse
import contextlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = {"fused": "1", "parent": "0"}        # CDX_DENOISE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=300, help="untimed steps of every route before a workload's first round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cleandiffuser_amd.diffusion import DiscreteDiffusionSDE
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.nn_condition import IdentityCondition
    from cleandiffuser_amd.nn_diffusion import DQLMlp
    from cleandiffuser_amd.utils import load_synth
    from cleandiffuser_amd.utils.critics import DQLCritic
    from cleandiffuser_amd.utils.policy_steps import approx_action
    dev = "cuda:0"
    obs_dim, act_dim, eta = 17, 6, 1.0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def actor_of(steps):
        net = load_synth(DQLMlp(obs_dim, act_dim, emb_dim=64), 65).to(dev)
        return DiscreteDiffusionSDE(net, IdentityCondition(dropout=0.0), predict_noise=False, x_max=torch.ones(1, act_dim),
                                    x_min=-torch.ones(1, act_dim), diffusion_steps=steps, device=dev)

    g = torch.Generator().manual_seed(7)
    obs, act = torch.randn(a.batch, obs_dim, generator=g).to(dev), torch.randn(a.batch, act_dim, generator=g).clamp(-1, 1).to(dev)

    def loss_step(steps):
        def make():
            actor = actor_of(steps)

            def step():
                actor.model.zero_grad(set_to_none=False)
                actor.loss(act, obs).backward()
            return step
        return make

    def edp_step(in_place):
        def make():
            actor = actor_of(50)
            critic = load_synth(DQLCritic(obs_dim, act_dim), 66).to(dev)
            params = list(actor.model.parameters())
            flip = [0]

            def step():
                actor.model.zero_grad(set_to_none=False)
                bc_loss = actor.loss(act, obs)
                pred_act = approx_action(actor, act, obs)
                critic.requires_grad_(False)                       # (FreezeModules of the pipeline)
                q1, q2 = critic(obs, pred_act)
                flip[0] ^= 1                                       # (the pipeline's coin, without its host-side draw)
                q_loss = -q1.mean() / q2.abs().mean().detach() if flip[0] else -q2.mean() / q1.abs().mean().detach()
                with (train.grads_in_place(params) if in_place else contextlib.nullcontext()):
                    (bc_loss + eta * q_loss).backward()
                critic.requires_grad_(True)
            return step
        return make

    def timed(step, route):
        os.environ["CDX_DENOISE"] = ROUTES[route]
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
        os.environ["CDX_DENOISE"] = ROUTES[route]
        step()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

    def ab(title, make):
        steps = {r: make() for r in ROUTES}                      # one actor per route
        say(title)
        for r in ROUTES:                                         # (clocks, allocator and weight layouts settle: untimed)
            os.environ["CDX_DENOISE"] = ROUTES[r]
            for _ in range(a.settle):
                steps[r]()
        ms = {r: [] for r in ROUTES}
        for i in range(a.rounds):
            for r in ROUTES:
                ms[r].append(timed(steps[r], r))
            say(f"  round {i}: " + "   ".join(f"{r} {ms[r][-1]:.3f}" for r in ROUTES))
        spread = {r: max(v) - min(v) for r, v in ms.items()}
        mean = {r: statistics.mean(v) for r, v in ms.items()}
        for r in ROUTES:
            say(f"  {r:7s} mean {mean[r]:.3f}  spread {spread[r]:.3f}  device kernels per step {kernels(steps[r], r)}")
        win = mean["parent"] - mean["fused"] > spread["fused"] + spread["parent"]
        say(f"  fused beats parent by more than the sum of the spreads: {win}")
        return win

    say(f"denoising loss of DQLMlp({obs_dim}, {act_dim}, emb_dim=64), B = {a.batch}, predict_noise=False, bounds +-1, "
        f"{torch.cuda.get_device_name(0)}; median of {a.iters} steps after {a.warmup} warm-up steps, {a.settle} untimed steps of every route "
        f"before a workload's first round, ms (wall time, synchronised around the step)")
    wins = [ab("a. loss + backward, T = 5", loss_step(5)), ab("a. loss + backward, T = 50", loss_step(50)),
            ab("b. EDP policy step: loss + approx_action + DQLCritic Q term + backward", edp_step(False))]
    ab("c. workload (b) inside train.grads_in_place(actor.model.parameters())", edp_step(True))
    say(f"the default rule (a and b): {all(wins)}")
    os.environ.pop("CDX_DENOISE", None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
