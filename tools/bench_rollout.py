"""A/B of Diffusion-QL's policy step on one device: ``sample(requires_grad=True)`` + ``backward()`` of ``-(act * q).sum(-1).mean()`` on
the fused rollout (engine/rollout.py) and on the host loop (CDX_ROLLOUT=0), alternating in one process.

    python tools/bench_rollout.py [--batch 256] [--steps 5] [--iters 50] [--rounds 3]

DQLMlp(17, 6, emb_dim=64), 5-step DDPM, x_max / x_min = +-1, HIP events after warm-up.  Prints per round the median time of both routes,
then their means, the spread over the rounds and the device-kernel counts of one step (torch.profiler)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import cleandiffuser_amd as lib
    from cleandiffuser_amd.nn_condition import IdentityCondition
    from cleandiffuser_amd.nn_diffusion import DQLMlp
    from cleandiffuser_amd.diffusion import DiscreteDiffusionSDE
    from cleandiffuser_amd.utils import load_synth
    dev = "cuda:0"
    net = load_synth(DQLMlp(17, 6, emb_dim=64), 65).to(dev)
    agent = DiscreteDiffusionSDE(net, IdentityCondition(dropout=0.0), x_max=torch.ones(1, 6), x_min=-torch.ones(1, 6),
                                 diffusion_steps=a.steps, device=dev)
    g = torch.Generator().manual_seed(9)
    obs = torch.randn(a.batch, 17, generator=g).to(dev)
    q = torch.randn(6, generator=g).to(dev)
    prior = torch.zeros(a.batch, 6, device=dev)

    def step():
        agent.model.zero_grad(set_to_none=True)
        act, _ = agent.sample(prior, solver="ddpm", n_samples=a.batch, sample_steps=a.steps, use_ema=False, condition_cfg=obs, w_cfg=1.0,
                              requires_grad=True)
        (-(act * q).sum(-1).mean()).backward()

    def timed(route):
        os.environ["CDX_ROLLOUT"] = route
        for _ in range(a.warmup):
            step()
        times = []
        for _ in range(a.iters):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            step()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        return statistics.median(times)

    def kernels(route):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        os.environ["CDX_ROLLOUT"] = route
        step()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

    print(f"DQL policy step: DQLMlp(17, 6, emb_dim=64), B = {a.batch}, {a.steps}-step DDPM, {torch.cuda.get_device_name(0)}; "
          f"median of {a.iters} steps after {a.warmup} warm-up steps, ms (HIP events)")
    fused, host = [], []
    for r in range(a.rounds):
        fused.append(timed("1"))
        host.append(timed("0"))
        print(f"round {r}: fused {fused[-1]:.3f}   host loop {host[-1]:.3f}")
    print(f"fused      mean {statistics.mean(fused):.3f}  spread {max(fused) - min(fused):.3f}")
    print(f"host loop  mean {statistics.mean(host):.3f}  spread {max(host) - min(host):.3f}")
    print(f"device kernels per step: fused {kernels('1')}, host loop {kernels('0')}")


if __name__ == "__main__":
    main()
