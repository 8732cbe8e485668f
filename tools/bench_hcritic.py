"""A/B of the horizon critic on one device: the executor (``cdx_hcritic_run``), the stock modules and the library's autograd nodes,
alternating in one process.

    python tools/bench_hcritic.py [--iters 50] [--rounds 5] [--out profiles/hcritic_ab.txt]

Synthetic weights at the shipped configuration (d_model 256, 8 heads, depth 2, pre-norm):

1. scoring the candidates of one environment step under ``no_grad``: 2500 plans x 40 tokens with in_dim 29 (antmaze; maze2d has the
   same count) and 7500 x 32 with in_dim 60 (kitchen).  Routes: "executor" (``CDX_HCRITIC=1``; also with its passes forced to 256, 512
   and 1024 trajectories -- the chunk rule of csrc/cdx_hcritic.hip is chosen from these), "stock" (``CDX_HCRITIC=0``: what the
   reference's class does on the device) and "nodes" (``forward_nodes`` under no_grad: the unpruned forward on library kernels);
2. the critic's training step at batch 128 x 32 tokens (zero_grad, MSE loss, backward, torch.optim.Adam): "nodes"
   (``CDX_HCRITIC_NODES=1``) against "stock".

HIP events around every call; a round is the median of `--iters` calls per route, the routes taking turns; every route first runs
`--warmup` untimed calls.  Prints per round the median of every route, then the means, the spread over the rounds, the device kernels of
one steady-state call and the verdict of the default rule of DESIGN.md 3m: a native route is the default only where it beats the stock
route by more than the sum of the two spreads."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from cleandiffuser_amd.engine import hcritic
    from cleandiffuser_amd.utils.critics import DVHorizonCritic
    from cleandiffuser_amd.utils.synth import load_synth, synth_array
    dev = "cuda:0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def critic(in_dim):
        return load_synth(DVHorizonCritic(in_dim, 16, d_model=256, n_heads=8, depth=2, norm_type="pre"), 5).to(dev)

    def env(**kw):
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def scoring(batch, tokens, in_dim):
        net = critic(in_dim).eval()
        x = torch.from_numpy(synth_array("bench/hcritic/x", (batch, tokens, in_dim))).to(dev)

        def executor(chunk):
            def call():
                env(CDX_HCRITIC="1")
                hcritic.CHUNK_OVERRIDE = chunk
                with torch.no_grad():
                    return net(x)
            return call

        def stock():
            env(CDX_HCRITIC="0")
            with torch.no_grad():
                return net(x)

        def nodes():
            with torch.no_grad():
                return hcritic.forward_nodes(net, x)
        routes = {"executor": executor(None), "executor/256": executor(256), "executor/512": executor(512), "executor/1024": executor(1024),
                  "stock": stock, "nodes": nodes}
        ref = routes["stock"]()
        for r, call in routes.items():
            err = float((call() - ref).abs().max())
            assert err < 1e-3, (r, err)
        return routes

    def training(batch, tokens, in_dim):
        x = torch.from_numpy(synth_array("bench/hcritic/xt", (batch, tokens, in_dim))).to(dev)
        target = torch.from_numpy(synth_array("bench/hcritic/target", (batch, 1))).to(dev)

        def make(flag):
            net = critic(in_dim).train()
            optim = torch.optim.Adam(net.parameters(), lr=3e-4)

            def step():
                env(CDX_HCRITIC_NODES=flag)
                optim.zero_grad()
                F.mse_loss(net(x), target).backward()
                optim.step()
            return step
        return {"nodes": make("1"), "stock": make("0")}

    def timed(call):
        times = []
        for _ in range(a.iters):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        return statistics.median(times)

    def kernels(call):
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        call()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)

    def ab(title, routes, native):
        say(title)
        for call in routes.values():
            for _ in range(a.warmup):
                call()
        torch.cuda.synchronize()
        ms = {r: [] for r in routes}
        for i in range(a.rounds):
            for r, call in routes.items():
                ms[r].append(timed(call))
            say(f"  round {i}: " + "   ".join(f"{r} {ms[r][-1]:.3f}" for r in routes))
        spread = {r: max(v) - min(v) for r, v in ms.items()}
        for r, call in routes.items():
            say(f"  {r:14s} mean {statistics.mean(ms[r]):.3f}  spread {spread[r]:.3f}  device kernels per call {kernels(call)}")
        for r in native:
            gain = statistics.mean(ms["stock"]) - statistics.mean(ms[r])
            say(f"  {r} beats the stock route by more than the sum of the spreads: {gain > spread[r] + spread['stock']} "
                f"(stock / {r} = {statistics.mean(ms['stock']) / statistics.mean(ms[r]):.2f})")

    say(f"DVHorizonCritic, d_model 256, 8 heads, depth 2, pre-norm, {torch.cuda.get_device_name(0)}; HIP events around a call, median of "
        f"{a.iters} calls per round after {a.warmup} untimed calls of every route, ms")
    for batch, tokens, in_dim in ((2500, 40, 29), (7500, 32, 60)):
        ab(f"1. scoring {batch} plans x {tokens} tokens, in_dim {in_dim}, no_grad", scoring(batch, tokens, in_dim),
           ("executor", "executor/256", "executor/512", "executor/1024", "nodes"))
    hcritic.CHUNK_OVERRIDE = None
    ab("2. training step, 128 plans x 32 tokens, in_dim 60 (MSE, torch.optim.Adam)", training(128, 32, 60), ("nodes",))
    env(CDX_HCRITIC=None, CDX_HCRITIC_NODES=None)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
