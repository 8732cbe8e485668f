"""A/B of QGPO's evaluation call on one device: ``actor.sample(prior, "ddpm", sample_step_schedule="quad_continuous", condition_cfg=obs,
w_cfg=1, condition_cg=obs, w_cg=w)`` (reference pipelines/qgpo_d4rl_mujoco.py:244-249) on the fused energy-guided launch
(engine/energy.py) and on the host loop (CDX_ENERGY=0), alternating in one process.

    python tools/bench_energy.py [--batch 50 800] [--steps 15] [--iters 50] [--rounds 3]

The shipped widths: SfBCUNet(6) (emb 64, hidden 512 / 256 / 128) under ContinuousDiffusionSDE with MLPCondition(17, 64, [64]) and
QGPOClassifier(QGPONNClassifier(17, 6, 64, [256, 256, 256], "untrainable_fourier")), x_max / x_min = +-1, synthetic weights, HIP events
after warm-up.  Prints per batch and round the median time of both routes, then their means, the spread over the rounds, the verdict of the
default rule (the fused route must beat the host loop by more than the sum of the two spreads) and the device kernels of one call."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[50, 800])
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--w_cg", type=float, default=1.0)
    a = ap.parse_args()
    from cleandiffuser_amd.classifier import QGPOClassifier
    from cleandiffuser_amd.diffusion import ContinuousDiffusionSDE
    from cleandiffuser_amd.nn_classifier import QGPONNClassifier
    from cleandiffuser_amd.nn_condition import MLPCondition
    from cleandiffuser_amd.nn_diffusion import SfBCUNet
    from cleandiffuser_amd.utils import load_synth
    dev, obs_dim, act_dim = "cuda:0", 17, 6
    net = load_synth(SfBCUNet(act_dim), 71).to(dev)
    cond = load_synth(MLPCondition(obs_dim, 64, [64], torch.nn.SiLU(), dropout=0.0), 72).to(dev)
    clf = QGPOClassifier(load_synth(QGPONNClassifier(obs_dim, act_dim, 64, [256, 256, 256], "untrainable_fourier"), 73).to(dev), device=dev)
    actor = ContinuousDiffusionSDE(net, cond, classifier=clf, x_max=torch.ones(act_dim), x_min=-torch.ones(act_dim), device=dev)
    actor.eval()
    clf.eval()
    print(f"QGPO evaluation call: SfBCUNet({act_dim}) + QGPONNClassifier(64, [256, 256, 256]), {a.steps}-step ddpm, quad_continuous, "
          f"{torch.cuda.get_device_name(0)}; median of {a.iters} calls after {a.warmup} warm-up calls, ms (HIP events)")

    for batch in a.batch:
        g = torch.Generator().manual_seed(9)
        obs = torch.randn(batch, obs_dim, generator=g).to(dev)
        prior = torch.zeros(batch, act_dim, device=dev)

        def call():
            return actor.sample(prior, "ddpm", n_samples=batch, sample_steps=a.steps, sample_step_schedule="quad_continuous",
                                condition_cfg=obs, w_cfg=1.0, condition_cg=obs, w_cg=a.w_cg)

        def timed(route):
            os.environ["CDX_ENERGY"] = route
            for _ in range(a.warmup):
                call()
            times = []
            for _ in range(a.iters):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                t1.synchronize()
                times.append(t0.elapsed_time(t1))
            return statistics.median(times)

        def kernels(route):
            from torch.autograd import DeviceType
            from torch.profiler import ProfilerActivity, profile
            os.environ["CDX_ENERGY"] = route
            call()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                call()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

        fused, host = [], []
        for r in range(a.rounds):
            fused.append(timed("1"))
            host.append(timed("0"))
            print(f"B = {batch} round {r}: fused {fused[-1]:.3f}   host loop {host[-1]:.3f}")
        spread_f, spread_h = max(fused) - min(fused), max(host) - min(host)
        print(f"B = {batch} fused      mean {statistics.mean(fused):.3f}  spread {spread_f:.3f}")
        print(f"B = {batch} host loop  mean {statistics.mean(host):.3f}  spread {spread_h:.3f}")
        wins = statistics.mean(host) - statistics.mean(fused) > spread_f + spread_h
        print(f"B = {batch} the fused route beats the host loop by more than the sum of the spreads: {wins}")
        print(f"B = {batch} device kernels per call: fused {kernels('1')}, host loop {kernels('0')}")


if __name__ == "__main__":
    main()
