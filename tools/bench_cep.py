"""A/B of QGPO's energy training step on one device: ``clf.update(noisy_act, t, {"soft_label", "obs"})`` (reference
pipelines/qgpo_d4rl_mujoco.py:172-212) on the fused row-tile route (engine/cep.py) and on the autograd body as it stood before
(CDX_CEP=0), alternating in one process.

    python tools/bench_cep.py [--batch 256] [--k 16] [--iters 50] [--rounds 5] [--out profiles/cep_ab.txt]

The shipped sizes: QGPOClassifier(QGPONNClassifier(17, 6, 64, [256, 256, 256], "untrainable_fourier"), optim_params={"lr": 1e-3}), 256
states x 16 support actions, synthetic weights.  Wall time of one call with a device synchronise before and after it (the call itself
ends in a device-to-host copy of its scalars on either route).  Prints per round the median of both routes, then their means, the spread
over the rounds, the verdict of the default rule (the fused route must beat the autograd body by more than the sum of the two spreads) and
the device kernels of one steady-state call of each."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cleandiffuser_amd.classifier import QGPOClassifier
    from cleandiffuser_amd.nn_classifier import QGPONNClassifier
    from cleandiffuser_amd.utils import load_synth
    dev, obs_dim, act_dim = "cuda:0", 17, 6
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def make():
        net = load_synth(QGPONNClassifier(obs_dim, act_dim, 64, [256, 256, 256], "untrainable_fourier"), 73).to(dev)
        return QGPOClassifier(net, optim_params={"lr": 1e-3}, device=dev)
    clfs = {"1": make(), "0": make()}                        # one classifier per route: each keeps training on its own weights
    g = torch.Generator().manual_seed(9)
    x = torch.randn(a.batch, a.k, act_dim, generator=g).to(dev)
    t = (1e-3 + 0.999 * torch.rand(a.batch, generator=g)).to(dev)
    y = {"soft_label": torch.softmax(torch.randn(a.batch, a.k, 1, generator=g), 1).to(dev), "obs": torch.randn(a.batch, obs_dim, generator=g).to(dev)}
    say(f"QGPO energy training step: QGPONNClassifier(17, 6, 64, [256, 256, 256]), B = {a.batch} states x K = {a.k} support actions, Adam "
        f"lr 1e-3 + EMA, {torch.cuda.get_device_name(0)}; median of {a.iters} update() calls after {a.warmup} warm-up calls, ms (wall time, "
        f"synchronised around the call)")

    def timed(route):
        os.environ["CDX_CEP"] = route
        clf = clfs[route]
        for _ in range(a.warmup):
            clf.update(x, t, y)
        times = []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            clf.update(x, t, y)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(times)

    def kernels(route):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        os.environ["CDX_CEP"] = route
        clfs[route].update(x, t, y)
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            clfs[route].update(x, t, y)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

    fused, aten = [], []
    for r in range(a.rounds):
        fused.append(timed("1"))
        aten.append(timed("0"))
        say(f"round {r}: fused {fused[-1]:.3f}   autograd body {aten[-1]:.3f}")
    spread_f, spread_a = max(fused) - min(fused), max(aten) - min(aten)
    say(f"fused          mean {statistics.mean(fused):.3f}  spread {spread_f:.3f}")
    say(f"autograd body  mean {statistics.mean(aten):.3f}  spread {spread_a:.3f}")
    wins = statistics.mean(aten) - statistics.mean(fused) > spread_f + spread_a
    say(f"the fused route beats the autograd body by more than the sum of the spreads: {wins}")
    say(f"device kernels per call: fused {kernels('1')}, autograd body {kernels('0')}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
