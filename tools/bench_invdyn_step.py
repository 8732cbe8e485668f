"""A/B of the inverse-dynamics training step on one device: the fused step (engine/regress_step.py, ``CDX_REGRESS_STEP=1``) against the
parent route (``CDX_REGRESS_STEP=0``: the concatenation, the library nodes of ``train.chain_forward`` or the eager modules, the ATen loss
and autograd), alternating in one process.

    python tools/bench_invdyn_step.py [--iters 400] [--rounds 5] [--out profiles/invdyn_step_ab.txt]

``MlpInvDynamic(obs_dim, act_dim, 512, nn.Tanh())`` with synthetic weights, FusedAdam, one ``update(obs, act, next_obs)`` per step
including ``optim.step()`` and the ``loss.item()`` it returns, at the sizes the pipelines run:

1. Decision Veteran, 128 rows: ``obs[:, 0]`` / ``act[:, 0]`` / ``obs[:, 1]`` of a (128, 4, D) batch; obs 17 / act 6 and obs 60 / act 9;
2. Decision Diffuser, 64 x 31 = 1984 rows: ``obs[:, :-1]`` / ``act[:, :-1]`` / ``obs[:, 1:]`` of a (64, 32, D) batch; the same two sizes.

Wall time of one step with a device synchronise before and after it; a round times `--iters` steps per route, and every workload first
runs `--settle` untimed steps of every route.  Prints per round the median of every route, then their means, the spread over the
rounds, the device kernels of one steady-state step of each, and the verdict of the default rule: the fused step must beat the parent
by more than the sum of the two spreads."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = {"fused": "1", "parent": "0"}                   # CDX_REGRESS_STEP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=300, help="untimed steps of every route before a workload's first round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cleandiffuser_amd.invdynamic import MlpInvDynamic
    from cleandiffuser_amd.utils import load_synth
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def make(kind, obs_dim, act_dim):
        def build():
            head = MlpInvDynamic(obs_dim, act_dim, 512, nn.Tanh(), optim_params={"lr": 3e-4}, device=dev)
            load_synth(head.mlp, 11)
            g = torch.Generator().manual_seed(7)
            B, H = (128, 4) if kind == "dv" else (64, 32)
            obs, act = torch.randn(B, H, obs_dim, generator=g).to(dev), torch.randn(B, H, act_dim, generator=g).tanh().to(dev)
            if kind == "dv":
                return lambda: head.update(obs[:, 0, :], act[:, 0, :], obs[:, 1, :])
            return lambda: head.update(obs[:, :-1], act[:, :-1], obs[:, 1:])
        return build

    def timed(step, route):
        os.environ["CDX_REGRESS_STEP"] = ROUTES[route]
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
        os.environ["CDX_REGRESS_STEP"] = ROUTES[route]
        step()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

    def ab(title, build):
        steps = {r: build() for r in ROUTES}                     # one head per route: each keeps training on its own weights
        say(title)
        for r in ROUTES:                                         # (clocks, allocator and optimiser state settle: untimed)
            os.environ["CDX_REGRESS_STEP"] = ROUTES[r]
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

    say(f"MlpInvDynamic.update, hidden 512, tanh head, FusedAdam lr 3e-4, {torch.cuda.get_device_name(0)}; median of {a.iters} steps after "
        f"{a.warmup} warm-up steps, {a.settle} untimed steps of every route before a workload's first round, ms (wall time, synchronised "
        f"around the step, optim.step() and loss.item() included)")
    ab("1. Decision Veteran, 128 rows (obs[:, 0] / obs[:, 1] of a (128, 4, 17) batch), obs 17, act 6", make("dv", 17, 6))
    ab("2. Decision Veteran, 128 rows, obs 60, act 9 (kitchen)", make("dv", 60, 9))
    ab("3. Decision Diffuser, 64 x 31 = 1984 rows (obs[:, :-1] / obs[:, 1:] of a (64, 32, 17) batch), obs 17, act 6", make("dd", 17, 6))
    ab("4. Decision Diffuser, 1984 rows, obs 60, act 9 (kitchen)", make("dd", 60, 9))
    os.environ.pop("CDX_REGRESS_STEP", None)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
