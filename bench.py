#!/usr/bin/env python
"""bench.py -- denoised trajectories/sec on BASELINE config 2 (the north-star metric).

One "step" = one complete ``DiscreteDiffusionSDE.sample()`` call: JannerUNet1d (in 23, model 32, dim_mult [1,2,2,2],
k=5), horizon 32, B=256 trajectories per GPU, 20-step DDIM, x-prediction, fix-mask on the first observation,
temperature 0.5 -- synthetic random-init weights and synthetic inputs already resident in HBM.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (driver, N > 1)

A plain run sets up, warms up, times exactly K steps and prints the headline; everything else it measures or checks (the
blocks marked [--full] below) runs only with ``--full``.  ``--dump-outputs DIR`` writes what the last timed step returned
(``DIR/x.npy``, float32, rank 0); the global RNG is seeded right before the timed loop, so with the same arguments the last
step's inputs -- its initial draw included -- are the same from run to run and two builds can be compared output for output.

The ONE JSON line (rank 0):

* ``value`` -- trajectories/s of the metric's GLOBAL B = 256 call exactly as a pipeline makes it (no ``noise=``: the initial draw is
  inside the call).  N > 1: STRONG scaling -- the 256 trajectories are cut into 256 / N per rank through
  ``cleandiffuser_amd.distributed.sharded_sample`` (shard, sample, ONE RCCL all-gather of the result inside the timed region: north
  star "RCCL over xGMI used only to gather sampled trajectories"); ``scaling`` says "strong" (north star: ">= 6x strong scaling").
  ``ms_per_step`` -- milliseconds of one timed step (one such call).
* [--full] ``sustained`` -- the timed loop once more over >= 1 s.
* [--full] ``replayed_noise`` -- the same call with the recorded ``noise=[z0]`` (rounds 1-2's headline), for comparison.
* [--full] ``weak_scaling`` (N > 1) -- every rank its own 256 trajectories + the all-gather of N x 256;  ``strong_scaling.global_batch_3200``
  -- the batch the shipped Diffuser pipelines really sample (50 environments x 64 candidate plans) sharded the same way.
* [--full] ``roofline`` prices the single fused kernel against the fp32-MFMA peak using the algorithmic FLOPs of the reference modules
  (786.6 MFLOP per trajectory = 39.33 MFLOP x 20 forwards) and the kernel's mean duration from HIP events on the
  launch stream.
* [--full] ``predicted_scaling``, ``other_configs`` (N = 1) -- the other BASELINE configs and the guided / large-batch variants of config 2, measured by the same
  process right after the headline (short runs; builder-independent numbers for configs 1, 3, 4, 5).
* [--full] ``cpu_baseline`` (N = 1) -- the imported reference classes when the reference tree is importable (``kind: "reference"``; build
  container), else the CPU oracle port (oracle/torch_port.py, the same ATen ops the reference runs; ``kind: "port"``; GPU boxes) on
  this host: at the fastest thread count of a probe and at ONE thread, with the CPU model and torch build; plus the recorded figure
  of the real reference measured in the build container (profiles/r04_reference_cpu.json, re-measured per round by tools/measure_reference_cpu.py).  Reported baseline only.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BATCH, HORIZON, DIM, SAMPLE_STEPS = int(os.environ.get("BENCH_BATCH", "256")), 32, 23, 20
PEAK_FP32_MFMA_TFLOPS = 157.3            # MI355X_MICROARCH.md: v_mfma_f32_*_f32 dense peak
FLOPS_PER_TRAJ = 2.0 * 19.67e6 * SAMPLE_STEPS   # SURVEY 8d (the program compilers re-derive 19.67 M MAC, asserted in tests/)


def build_agent(device):
    from cleandiffuser_amd.diffusion import DiscreteDiffusionSDE
    from cleandiffuser_amd.nn_diffusion import JannerUNet1d
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(JannerUNet1d(DIM, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), seed=0)
    fix_mask = torch.zeros(HORIZON, DIM)
    fix_mask[0, :17] = 1.0
    agent = DiscreteDiffusionSDE(net, None, fix_mask=fix_mask, diffusion_steps=SAMPLE_STEPS, predict_noise=False,
                                 device=device)
    agent.eval()
    return agent, net


def make_inputs(device, seed, batch=None):
    batch = BATCH if batch is None else batch
    g = torch.Generator().manual_seed(1000 + seed)
    prior = torch.zeros(batch, HORIZON, DIM)
    prior[:, 0, :17] = torch.randn(batch, 17, generator=g)
    z0 = torch.randn(batch, HORIZON, DIM, generator=g)
    return prior.to(device), z0.to(device)


# ------------------------------------------------------------------------------------------------------------------- #
# CPU baseline leg (child process)                                                                                      #
# ------------------------------------------------------------------------------------------------------------------- #
def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _reference_call(net):
    """The REAL reference's sample() (imported from the read-only mount through oracle/ref_import.py) on the bench's weights, or None
    where the mount does not exist (the GPU boxes: SURVEY 8d's "imported reference classes" are only reachable in the build
    container)."""
    try:
        from oracle import cases, ref_import
        if not ref_import.available():
            return None
        ref = cases.lib_namespace("reference")
        rnet = ref.JannerUNet1d(DIM, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5)
        rnet.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
        fix = torch.zeros(HORIZON, DIM)
        fix[0, :17] = 1.0
        agent = ref.DiscreteDiffusionSDE(rnet, None, fix_mask=fix, diffusion_steps=SAMPLE_STEPS, predict_noise=False, device="cpu")
        agent.eval()
        prior, _ = make_inputs("cpu", 0, 256)
        return lambda: agent.sample(prior, solver="ddim", n_samples=256, sample_steps=SAMPLE_STEPS, temperature=0.5)[0]
    except Exception:  # noqa: BLE001 -- any import problem: fall back to the port, which is pinned to the same fixtures
        return None


def cpu_baseline(net, budget_s=10.0):
    """Time the CPU path on a bounded sample of the same workload: whole sample() calls at B=256 until ~budget_s of CPU work
    has been done (>= 2 calls) at the fastest thread count of a probe, then >= 1 call at one thread.  The imported reference
    classes when /root/reference is mounted (``kind: "reference"``), else the oracle port (``kind: "port"``)."""
    from oracle import torch_port
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    fwd = torch_port.make_forward(sd, dict(emb_dim=32, kernel_size=5, dim_mult=[1, 2, 2, 2]))
    prior, z0 = make_inputs("cpu", 0, 256)
    fm = torch.zeros(1, HORIZON, DIM)
    fm[0, 0, :17] = 1.0
    avail = torch.get_num_threads()           # torch's own default = the cores this process may use
    ref_call = _reference_call(net)
    kind = "reference" if ref_call is not None else "port"

    def call():
        with torch.no_grad():
            if ref_call is not None:
                return ref_call()
            return torch_port.vp_sample(fwd, prior, [z0], solver="ddim", sample_steps=SAMPLE_STEPS, discrete=True,
                                        diffusion_steps=SAMPLE_STEPS, temperature=0.5, predict_noise=False,
                                        fix_mask=fm)
    # the reference path is small-op bound: all cores of a big host oversubscribe it, so probe a few thread counts
    # (one timed call each) and run the bounded sample at the fastest -- `cores` reports what was actually used
    probe = {}
    for th in sorted({t for t in (8, 16, 32, 64, avail) if t <= avail}):
        torch.set_num_threads(th)
        call()                                 # warm-up (thread pool, oneDNN primitives)
        t0 = time.perf_counter()
        call()
        probe[th] = time.perf_counter() - t0
    cores = min(probe, key=probe.get)
    torch.set_num_threads(cores)
    call()
    t0, n = time.perf_counter(), 0
    while n < 2 or time.perf_counter() - t0 < budget_s:
        call()
        n += 1
    dt = time.perf_counter() - t0
    torch.set_num_threads(1)
    call()
    t1, n1 = time.perf_counter(), 0
    while n1 < 1 or time.perf_counter() - t1 < budget_s / 2:
        call()
        n1 += 1
    dt1 = time.perf_counter() - t1
    ref = None
    for name in ("r05_reference_cpu.json", "r04_reference_cpu.json", "r02_reference_cpu.json"):      # the newest record of the REAL reference (build container)
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                ref = json.load(f)
            ref["record"] = f"profiles/{name} -- a RECORDED figure (round {ref.get('round', 2)}, {ref.get('measured_on', 'date not recorded')}), " \
                            "not measured by this run: /root/reference does not exist on the GPU box"
            break
        except (OSError, ValueError):
            continue
    # port <-> reference: the two were timed back to back in the build container (tools/measure_reference_cpu.py: same weights, inputs,
    # threads, interleaved calls); the recorded ratio makes this box's `port` figure traceable to the reference (VERDICT r4 weak #9a)
    ratio = (ref or {}).get("port_over_reference")
    blas = [ln.strip() for ln in torch.__config__.show().splitlines() if "BLAS" in ln or "MKL" in ln or "OpenMP" in ln][:4]
    how = "the imported reference classes (/root/reference)" if kind == "reference" else "oracle/torch_port.py (no /root/reference on this box)"
    return {"value": 256 * n / dt, "unit": "trajectories/s", "cores": cores, "kind": kind,
            "sample": f"{n} full sample() calls of B=256 (20-step DDIM) through {how}, {dt:.1f}s wall, "
                      f"{cores} of {avail} threads (fastest of a probe over {sorted(probe)})",
            "all_cores": {"value": 256 / probe[avail], "cores": avail, "sample": "one call after a warm-up"},
            "one_thread": {"value": 256 * n1 / dt1, "cores": 1, "sample": f"{n1} calls, {dt1:.1f}s wall"},
            "cpu_model": _cpu_model(), "torch": torch.__version__, "torch_build": blas,
            "port_over_reference": 1.0 if kind == "reference" else ratio,
            "reference_equivalent": {"value": (256 * n / dt) / ratio, "unit": "trajectories/s",
                                     "how": "this box's port figure / the recorded port_over_reference (build container, "
                                            "profiles/r05_reference_cpu.json; asserted by tests/test_bench_contract.py)"}
            if (kind == "port" and ratio) else None,
            "reference_in_build_container_recorded": ref}


def cpu_baseline_subprocess(timeout_s=240):
    """Run the CPU leg in a child with a hard wall-clock bound so the GPU line is never held hostage."""
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only"], capture_output=True,
                           text=True, timeout=timeout_s)
        return json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:  # noqa: BLE001 -- report, never fail the bench on the baseline leg
        return {"value": None, "unit": "trajectories/s", "cores": None, "kind": "port",
                "sample": f"cpu baseline leg failed or exceeded {timeout_s}s: {type(e).__name__}"}


def recorded_traffic():
    """HBM-side bytes per launch of the fused kernel from the committed PMC pass (rocprofv3 --pmc cannot run inside this
    process); null when the record is absent."""
    for name in ("r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "r01_pmc_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                rec = json.load(f)
            out = {"traffic": rec["fetch_bytes_per_launch"] + rec["write_bytes_per_launch"], "traffic_unit": "bytes/launch",
                   "traffic_kernel": rec.get("kernel"),
                   "traffic_source": f"profiles/{name} (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950-corrected)"}
            # (round 4: the matrix-pipe and L2 counters of the same kernel, each from its own --pmc pass, next to the HBM-side bytes)
            for key in ("mfma_busy_frac", "l2_bytes_per_launch", "l2_hit_frac"):
                if key in rec:
                    out[key] = rec[key]
            return out
        except (OSError, KeyError, ValueError):
            continue
    return {"traffic": None}


def live_traffic(timeout_s=150):
    """HBM-side bytes per launch of the fused kernel, MEASURED by this run (VERDICT r4 weak #9b: rounds 1-4 re-printed a committed
    record): two child runs of this very script under ``rocprofv3 --kernel-trace --pmc`` -- FETCH_SIZE and WRITE_SIZE in separate
    passes (they do not fit one pass; MI355X_MICROARCH.md, PMC slots), no tracing domain besides the kernel trace -- a handful of
    launches each, mean per dispatch of the kernel that dominates.  FETCH_SIZE is doubled (the guide's gfx950 correction for 16 B / lane
    streams); WRITE_SIZE as reported (uncalibrated per the guide).  Returns None when rocprofv3 is missing or a pass fails / times out
    (the caller then quotes the committed record and says so)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    got = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            with tempfile.TemporaryDirectory(dir="/tmp") as d:
                env = dict(os.environ, TMPDIR="/tmp")
                cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                       "--steps", "8", "--warmup", "3", "--no-cpu-baseline", "--no-other-configs", "--no-pmc"]
                subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s, check=True)
                per = {}
                for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                    for row in csv.DictReader(open(path)):
                        if "cdx_unet2_kernel" in row.get("Kernel_Name", "") and row.get("Counter_Name") == counter:
                            per.setdefault(row["Kernel_Name"], []).append(float(row["Counter_Value"]))
                if not per:
                    return None
                # the kernel that does the work: by counter VOLUME, not by dispatch count (the idle repair launches behind the grouped
                # launches are as many dispatches of the ordinary program's instantiation)
                name = max(per, key=lambda k: sum(per[k]))
                got[counter] = (sum(per[name]) / len(per[name]), len(per[name]), name)
    except Exception:  # noqa: BLE001 -- never fail the bench on the counter leg
        return None
    fetch = got["FETCH_SIZE"][0] * 1024.0 * 2.0
    write = got["WRITE_SIZE"][0] * 1024.0
    return {"traffic": fetch + write, "traffic_unit": "bytes/launch", "fetch_bytes_per_launch": fetch, "write_bytes_per_launch": write,
            "traffic_kernel": got["FETCH_SIZE"][2][:96], "dispatches": got["FETCH_SIZE"][1],
            "traffic_source": "MEASURED by this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (one child run of this script per "
                              "counter, mean over its dispatches of the kernel; FETCH_SIZE x 1024 B x 2 = the guide's gfx950 correction, "
                              "WRITE_SIZE x 1024 B as reported)"}


# ------------------------------------------------------------------------------------------------------------------- #
# other configs (N = 1)                                                                                                 #
# ------------------------------------------------------------------------------------------------------------------- #
def other_configs(device):
    """Short measurements of the other BASELINE configs / config-2 variants (tools/bench_configs.py workloads): each entry has
    the whole-call rate, ms per sample() call, the fp32-MFMA fraction of the whole call and the kernel family that dominates."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_configs as bc
    from cleandiffuser_amd.engine import runtime
    out = []

    def timed(call, reps):
        x = call()
        torch.cuda.synchronize(device)
        assert torch.isfinite(x).all()
        runtime.enable_launch_timing(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        torch.cuda.synchronize(device)
        dt = (time.perf_counter() - t0) / reps
        k_ms = runtime.drain_launch_timing()
        runtime.enable_launch_timing(False)
        return dt, k_ms

    def big(tag, fn, kernel, reps=3, **kw):
        try:
            label, call, b, flops = fn(**kw)
            dt, k_ms = timed(call, reps)
            out.append({"name": tag, "workload": label, "value": b / dt, "unit": "samples/s", "ms_per_call": 1e3 * dt,
                        "roofline_frac": flops / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS, "dominant_kernel": kernel,
                        # program-kernel time per CALL (a call whose batch is cut into rounds is several launches)
                        "fused_kernel_ms": (sum(k_ms) / reps) if k_ms else None, "launches_per_call": len(k_ms) / reps})
        except Exception as e:  # noqa: BLE001 -- one broken side measurement must not take the headline down
            out.append({"name": tag, "error": f"{type(e).__name__}: {e}"})

    big("config2_B3200", bc.cfg2big, "cdx_unet2_kernel<3, 8> / <2, 8> (rounds of 256 workgroups: three rounds at three trajectories per workgroup + two at two, runtime2.plan_parts)", B=3200)
    # what one rank of an 8- / 2-GPU run of the metric's batch gets (and the real-time-control case): the small-batch mode
    big("config2_B32", bc.cfg2big, "cdx_unet2_kernel<1, 8, ..., split>: one trajectory over 4 workgroups of an XCD, all-gather of the cut "
        "ops through L2 (latency is the figure of merit: ms_per_call)", reps=10, B=32)
    big("config2_B128", bc.cfg2big, "cdx_unet2_kernel<1, 8, ..., split>: one trajectory over 2 workgroups of an XCD", reps=10, B=128)
    big("config2_guided_B256", bc.cfg2g, "cdx_unet2_kernel<1, 8, true, ..., split> as a GROUPED guided program (round 6): denoiser forward with its ten "
        "stream-bound layers grouped over 4 workgroups + classifier forward/backward on each member's own trajectory + shifted solver step "
        "+ final log_p, one launch per guided sample() call (and its idle repair launch)", reps=10, B=256)
    big("config2_guided_B3200", bc.cfg2g, "cdx_unet2_kernel<3, 8, true>: three trajectories per workgroup (compact guided program, saved "
        "normalised tensors in a global workspace), three rounds of 768 + two rounds of two per workgroup; the batch the shipped Diffuser pipelines "
        "sample (50 environments x 64 plans, all with w_cg > 0)", reps=2, B=3200)
    big("kitchen_guided_B256", bc.cfgKg, "cdx_unet2_kernel<1, 8, true>: guided program of the shipped kitchen Diffuser size (model_dim 64, "
        "H=32, D=69), saved tensors in the global workspace", B=256)
    big("antmaze_guided_B256", bc.cfgAg, "cdx_unet2_kernel<1, 8, true>: compact guided program of the shipped antmaze Diffuser size "
        "(model_dim 64, H=64, D=37)", B=256)
    big("antmaze_unguided_B3200", bc.cfgAu, "cdx_unet2_kernel<1, 8>: compact one-trajectory program (model_dim 64, H=64, D=37)", reps=2, B=3200)
    try:
        label, call, b, steps, net, horizon = bc.cfg1()
        dt, k_ms = timed(call, 5)
        from cleandiffuser_amd.engine import runtime2
        tile = runtime.mlp_tile(b)
        prog = runtime2.compiled_mlp2(net, "pearce", tile).prog
        flops = 2.0 * prog.macs_per_forward / tile * steps * b
        out.append({"name": "config1", "workload": label, "value": b / dt, "unit": "samples/s", "ms_per_call": 1e3 * dt,
                    "roofline_frac": flops / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                    "dominant_kernel": f"cdx_unet2_kernel<1, 8, false, false, true, true> (batch-tiled MLP program, {tile} samples per workgroup)",
                    "fused_kernel_ms": (sum(k_ms) / len(k_ms)) if k_ms else None})
    except Exception as e:  # noqa: BLE001
        out.append({"name": "config1", "error": f"{type(e).__name__}: {e}"})
    try:
        label, call, b, steps, net, horizon = bc.cfg3()
        dt, _ = timed(call, 2)
        flops = 2.0 * 298.4e6 * steps * b
        out.append({"name": "config3", "workload": label, "value": b / dt, "unit": "samples/s", "ms_per_call": 1e3 * dt,
                    "roofline_frac": flops / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS, "dominant_kernel": "cdx_gemm_kernel (implicit-GEMM conv)"})
    except Exception as e:  # noqa: BLE001
        out.append({"name": "config3", "error": f"{type(e).__name__}: {e}"})
    big("config4_shard512", bc.cfg4, "cdx_gemm_kernel", B=512)
    big("config5_chunk16384", bc.cfg5, "cdx_gemm_kernel", reps=1, B=16384)
    # config 5 as one rank of the 8-GPU run sees it: 1 M samples / 8 = 125 000 rows in ONE sample() call (cdx_resmlp_run cuts it into
    # 16 384-row chunks itself), and at the real hopper transition width D = 27 (report both)
    big("config5_shard125000", bc.cfg5, "cdx_gemm_kernel (8 chunks of <= 16 384 rows inside one cdx_resmlp_run call)", reps=1, B=125000)
    big("config5_D27_chunk16384", bc.cfg5, "cdx_gemm_kernel", reps=1, B=16384, D=27)
    # row a16: Diffusion Policy's transformer at the dp_pusht size and step count
    big("chitransformer_pusht_B1024", bc.cfgT, "cdx_gemm_kernel + cdx_attention_mfma_kernel + cross-attention (cdx_chitf_run)", reps=2, B=1024)
    # row f4: one training step of config 2 -- which side of it is native is in the entry
    try:
        from cleandiffuser_amd.engine import train as native_train
        has_native = True
    except ImportError:
        has_native = False
    for native, graph in ([(True, True), (True, False), (False, False)] if has_native else [(None, False)]):
        tag = "config2_update_B256" + ("_hipgraph" if graph else "" if native in (True, None) else "_autograd")
        try:
            label, call, b = bc.cfgU(256, native_backward=native, graph=graph)
            for _ in range(3):
                call()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(20):
                call()
            torch.cuda.synchronize(device)
            dt = (time.perf_counter() - t0) / 20
            how = ("forward / backward in the library's kernels (engine/train.py)" if native else
                   "forward / backward on PyTorch autograd (ATen / MIOpen kernels)")
            if graph:
                how += ", captured once and replayed as ONE HIP graph per step (the default since round 5 where the capturability probe passes)"
            # (roofline of a training step: forward + backward-data + backward-weights = 3 x the forward's FLOPs, VERDICT r5 missing #8)
            out.append({"name": tag, "workload": label, "value": 1.0 / dt, "unit": "update_steps/s", "ms_per_call": 1e3 * dt,
                        "roofline_frac": 3.0 * (FLOPS_PER_TRAJ / SAMPLE_STEPS) * b / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                        "what": how + "; gradient-norm clip + AdamW + EMA: cdx_optim_f32 (3 launches)"})
        except Exception as e:  # noqa: BLE001
            out.append({"name": tag, "error": f"{type(e).__name__}: {e}"})
    # ... and one whole Diffuser training iteration: update() + update_classifier() (round 6: the classifier's step on the library too)
    for native, graph in ([(True, True), (False, False)] if has_native else []):
        tag = "diffuser_train_iteration_B256" + ("_hipgraph" if graph else "_autograd")
        try:
            label, call, b, macs = bc.cfgUC(256, native_backward=native, graph=graph)
            for _ in range(3):
                call()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for _ in range(20):
                call()
            torch.cuda.synchronize(device)
            dt = (time.perf_counter() - t0) / 20
            out.append({"name": tag, "workload": label, "value": 1.0 / dt, "unit": "iterations/s", "ms_per_call": 1e3 * dt,
                        "roofline_frac": 3.0 * 2.0 * macs * b / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                        "what": ("denoiser and classifier: forward / backward on the library's kernels, one HIP-graph replay each; AdamW / Adam + "
                                 "EMA on cdx_optim_f32" if native else "PyTorch autograd over ATen / MIOpen kernels, torch.optim.Adam for the classifier")})
        except Exception as e:  # noqa: BLE001
            out.append({"name": tag, "error": f"{type(e).__name__}: {e}"})
    os.environ.pop("CDX_TRAIN_GRAPH", None)
    os.environ.pop("CDX_TRAIN_NATIVE", None)
    # row f4, third slice: where the training batch comes from -- HBM-resident dataset buffers against the reference's host-side loader
    for resident in (True, False):
        tag = "d4rl_batches_B64_" + ("resident" if resident else "dataloader")
        try:
            label, nxt, b, nbytes = bc.cfgD(64, resident=resident)
            for _ in range(5):
                nxt()
            torch.cuda.synchronize(device)
            reps = 400 if resident else 40
            t0 = time.perf_counter()
            for _ in range(reps):
                batch = nxt()
            torch.cuda.synchronize(device)
            dt = (time.perf_counter() - t0) / reps
            assert batch["act"].is_cuda and batch["obs"]["state"].shape[:2] == (b, 32)
            out.append({"name": tag, "workload": label, "value": 1.0 / dt, "unit": "batches/s", "ms_per_call": 1e3 * dt,
                        "batch_bytes": b * (32 * (11 + 3 + 1) + 1) * 4, "resident_bytes": nbytes})
        except Exception as e:  # noqa: BLE001
            out.append({"name": tag, "error": f"{type(e).__name__}: {e}"})
    return out


def predicted_scaling(agent, device):
    """What `bench.py --gpus N` should report on an N-GPU node, predicted on ONE GPU (VERDICT r3 'next' #7; the driver measures the
    real curve when it has an 8-GPU node): the data path of N ranks is `sample()` on ceil(B / N) trajectories per rank plus ONE RCCL
    all-gather of the result (cleandiffuser_amd/distributed.py), so value(N) = B / (latency(B / N) + all-gather(N, B)).  The
    latencies are MEASURED here (the same call, this GPU, the batch a rank would get); the all-gather is a MODEL: 30 us of RCCL
    launch latency + the bytes a rank receives at 60 GB/s (a conservative ring rate over one 153 GB/s xGMI link) -- under 2 % of the
    call at either batch, the prediction hangs on the measured latencies."""
    out = {"model": "value(N) = B / (measured sample() latency at ceil(B / N) trajectories on this GPU + 0.03 ms + received bytes / 60 GB/s)"}
    for gb in (256, 3200):
        rows = []
        for n in (1, 2, 4, 8):
            b = -(-gb // n)
            prior, _ = make_inputs(device, 777, b)
            kw = dict(solver="ddim", n_samples=b, sample_steps=SAMPLE_STEPS, temperature=0.5)
            for _ in range(3):
                agent.sample(prior, **kw)
            torch.cuda.synchronize(device)
            reps = 12 if b <= 800 else 4
            t0 = time.perf_counter()
            for _ in range(reps):
                agent.sample(prior, **kw)
            torch.cuda.synchronize(device)
            lat = 1e3 * (time.perf_counter() - t0) / reps
            gather = 0.0 if n == 1 else 0.03 + (gb - b) * HORIZON * DIM * 4 / 60e9 * 1e3
            rows.append({"n_gpus": n, "trajectories_per_gpu": b, "sample_ms": lat, "allgather_ms_model": gather,
                         "value": gb / (lat + gather) * 1e3})
        for r in rows:
            r["speedup"] = r["value"] / rows[0]["value"]
            r["efficiency"] = r["speedup"] / r["n_gpus"]
        out[f"global_batch_{gb}"] = rows
    return out


# ------------------------------------------------------------------------------------------------------------------- #
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)      # ~5.6 ms per call: a >= 2 s timed region
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline: sustained / replayed-noise loops, scaling legs, roofline, "
                         "other configs, CPU baseline (the --no-* options below trim it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the live rocprofv3 --pmc passes (roofline.traffic then quotes the committed record)")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    if args.cpu_baseline_only:               # child process of the N=1 run: CPU oracle timing only
        _, net = build_agent("cpu")
        print(json.dumps(cpu_baseline(net)), flush=True)
        return

    import faulthandler
    faulthandler.dump_traceback_later(600, exit=False)     # if anything wedges, say where (stderr)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the product path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or os.environ.get("BENCH_FORCE_DIST"):      # (BENCH_FORCE_DIST=1: exercise the RCCL path on a single-GPU box)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        assert dist.get_world_size() == world == args.gpus, (dist.get_world_size(), world, args.gpus)

    from cleandiffuser_amd import distributed as cdist
    from cleandiffuser_amd.engine import runtime
    runtime.load_library()
    agent, net = build_agent(device)
    prior, z0 = make_inputs(device, rank)
    kw = dict(solver="ddim", n_samples=BATCH, sample_steps=SAMPLE_STEPS, temperature=0.5)
    gathered = torch.empty((BATCH * world, HORIZON, DIM), device=device) if dist is not None else None

    gprior, gz = make_inputs(device, 12345, BATCH)        # the GLOBAL batch of the metric, identical on every rank
    skw = dict(solver="ddim", sample_steps=SAMPLE_STEPS, temperature=0.5)

    def step():
        # exactly what a pipeline calls (reference pipelines/diffuser_d4rl_mujoco.py:144): no `noise=`, the initial N(0, I) draw
        # (reference diffusionsde.py:493) happens inside sample() and inside the timed region.
        # N > 1: STRONG scaling of the metric's own batch -- the global B = 256 request is cut into 256 / N trajectories per rank,
        # sampled, and exchanged with the one RCCL all-gather of the data path, all inside the timed region
        if dist is not None:
            return cdist.sharded_sample(agent, gprior, gather=True, **skw)
        x, _ = agent.sample(prior, **kw)
        return x

    def step_replayed():
        x, _ = agent.sample(prior, noise=[z0], **kw)
        return x

    def step_weak():                          # every rank denoises its own 256 trajectories, then the all-gather of N x 256
        x, _ = agent.sample(prior, **kw)
        dist.all_gather_into_tensor(gathered, x)
        return x

    def fence():
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize(device)

    def timed_loop(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            x = fn()
        fence()
        elapsed = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([elapsed], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, x

    for _ in range(args.warmup):
        step()
    if args.full:
        runtime.enable_launch_timing(True)
    # the initial draws of the timed steps come from the global RNG: seeded here, after the warm-up, so that the last step's inputs
    # depend on the arguments alone (--dump-outputs compares builds output for output)
    torch.manual_seed(20240 + rank)
    elapsed, x = timed_loop(step, args.steps, 0)
    if args.full:
        kernel_ms = runtime.drain_launch_timing()
        repair_ms = runtime.drain_repair_timing()
        runtime.enable_launch_timing(False)
    assert torch.isfinite(x).all() and x.shape[0] == BATCH
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "x.npy"), x.detach().float().cpu().numpy())

    line = None
    if rank == 0:
        out = {
            "metric": "denoised trajectories/sec @ (B=256,H=32,D=23) 20-step DDIM",
            "value": BATCH * args.steps / elapsed,
            "unit": "trajectories/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,     # (the global batch of the metric is fixed: 256 at every N)
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: JannerUNet1d Diffuser H=32 D=23, 20-step DDIM, "
                                   f"global B={BATCH}, whole DiscreteDiffusionSDE.sample() call as a pipeline makes it (initial draw inside)"
                                   + (f", sharded {BATCH}/{world} per GPU, then one RCCL all-gather of the result" if dist is not None else ""),
                       "batch_per_gpu": BATCH // world, "global_batch": BATCH, "horizon": HORIZON, "dim": DIM,
                       "sample_steps": SAMPLE_STEPS, "world_size": world,
                       "parallelism": f"batch-sharded x{world}; the only data-path collective is the all-gather of the result"},
        }
        line = json.dumps(out)
    if args.full:
        line = full_measurements(args, out if rank == 0 else None, step=step, step_replayed=step_replayed, step_weak=step_weak,
                                 timed_loop=timed_loop, agent=agent, device=device, dist=dist, world=world, rank=rank,
                                 elapsed=elapsed, kernel_ms=kernel_ms, repair_ms=repair_ms, skw=skw)
    faulthandler.cancel_dump_traceback_later()

    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    # The JSON line is the LAST thing this process writes to stdout: RCCL prints a version banner through C stdio, which is
    # block-buffered on a pipe and would otherwise surface after the line when the process exits.
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except (OSError, AttributeError):
        pass
    sys.stdout.flush()
    if rank == 0:
        print(line, flush=True)


def full_measurements(args, out, *, step, step_replayed, step_weak, timed_loop, agent, device, dist, world, rank, elapsed, kernel_ms,
                      repair_ms, skw):
    """--full: everything besides the headline, measured by the same process right after the timed steps.  `out` is rank 0's headline
    record (None on the other ranks); returns rank 0's whole JSON line."""
    from cleandiffuser_amd import distributed as cdist
    # `value` times EXACTLY --steps calls (the contract); with the driver's --steps 20 that is a 74 ms region (VERDICT r4 weak #9c), so
    # the same loop is timed once more over at least one second and reported next to it (`sustained`)
    sus_steps = max(args.steps, int(1.05 / max(elapsed / args.steps, 1e-6)) + 1)
    el_sus, _ = timed_loop(step, sus_steps, 0)
    replay_reps = max(args.steps // 4, 5)
    el_replay, _ = timed_loop(step_replayed, replay_reps, 2)

    strong, weak = None, None
    if dist is not None:
        reps = max(args.steps // 4, 3)
        el, xw = timed_loop(step_weak, reps, 2)
        weak = {"value": BATCH * world * reps / el, "unit": "trajectories/s", "ms_per_call": 1e3 * el / reps, "calls_timed": reps,
                "what": f"every rank samples its own {BATCH} trajectories, then one RCCL all-gather of the {world} x {BATCH} result"}
        # the batch the shipped Diffuser pipelines really sample (50 environments x 64 candidate plans), sharded the same way
        strong = {}
        for gb in (3200,):
            gp, _ = make_inputs(device, 12345, gb)
            reps = max(args.steps // 16, 3)
            el, xs = timed_loop(lambda: cdist.sharded_sample(agent, gp, gather=True, **skw), reps, 2)
            assert xs.shape[0] == gb and torch.isfinite(xs).all()
            strong[f"global_batch_{gb}"] = {"value": gb * reps / el, "unit": "trajectories/s", "ms_per_call": 1e3 * el / reps,
                                            "trajectories_per_gpu": [cdist.shard_bounds(gb, r, world)[1] - cdist.shard_bounds(gb, r, world)[0]
                                                                     for r in range(world)], "calls_timed": reps,
                                            "includes": "shard, sample(), RCCL all-gather of the result"}

    if rank == 0:
        rec = recorded_traffic()
        live = live_traffic() if (world == 1 and dist is None and not args.no_pmc) else None
        traffic = dict(rec)
        if live is not None:
            traffic.update(live)
            traffic["recorded"] = {k: rec.get(k) for k in ("traffic", "traffic_source")}       # the committed record, for comparison
        k_ms = sum(kernel_ms) / max(len(kernel_ms), 1)
        launch_b = BATCH if dist is None else cdist.shard_bounds(BATCH, 0, world)[1]      # trajectories one launch of rank 0 processes
        achieved = FLOPS_PER_TRAJ * launch_b / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0
        from cleandiffuser_amd.engine import runtime2
        route = runtime2.route_info(agent.model_ema["diffusion"], HORIZON, launch_b, device)
        comp, n_wg = route["comp"], route["workgroups"]
        if route["mode"] == "grouped":
            kname = (f"cdx_unet2_kernel<1, 8, ..., split> as a GROUPED program: {route['k']} trajectories over the {route['k']} workgroups of a "
                     f"group on one XCD, the {comp.prog.meta['n_gops']} stream-bound layers computed per member for 1/{route['k']} of the output "
                     "channels of all the group's trajectories (16 tile columns), all-gathered through L2")
        elif route["mode"] == "split":
            kname = f"cdx_unet2_kernel<1, 8, ..., split>: one trajectory over {route['k']} workgroups of an XCD"
        else:
            tpw = route["parts"][0][2]
            kname = f"cdx_unet2_kernel<{tpw}, {comp.prog.nw}> ({tpw} trajectories, {comp.prog.nw} wave64 per workgroup)"
        # second roofline of the same launch: what the workgroups stream from L2 (activations never leave LDS).  One trajectory per
        # workgroup re-streams the whole packed weight set per forward and CU -- at B = 256 THAT was the binding limit through round 3
        # (56 % of the 34.5 TB/s aggregate L2 bandwidth of MI355X_MICROARCH.md); the grouped program streams 1/k of the large layers
        wbytes = float(route["stream_bytes_per_workgroup_forward"])
        l2_bytes = wbytes * n_wg * SAMPLE_STEPS
        l2 = {"bound": "l2", "bytes_per_launch": l2_bytes, "achieved": l2_bytes / (k_ms * 1e-3) / 1e12 if k_ms > 0 else 0.0,
              "peak": 34.5, "unit": "TB/s", "weight_bytes_per_workgroup_forward": wbytes,
              "packed_weight_bytes": 4.0 * comp.prog.meta["blob_floats"], "workgroups": n_wg, "mode": route["mode"], "group": route["k"]}
        l2["frac"] = l2["achieved"] / l2["peak"]
        out["roofline"] = {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                           "frac": achieved / PEAK_FP32_MFMA_TFLOPS, **traffic,
                           "kernel": kname, "kernel_ms": k_ms,
                           "launches_timed": len(kernel_ms), "flops_per_launch": FLOPS_PER_TRAJ * launch_b, "trajectories_per_launch": launch_b,
                           "l2_stream": l2}
        out["sustained"] = {"value": BATCH * sus_steps / el_sus, "unit": "trajectories/s", "ms_per_step": 1e3 * el_sus / sus_steps,
                            "steps": sus_steps, "seconds": el_sus, "what": "the timed loop of `value` once more over >= 1 s"}
        out["roofline"]["repair_launch"] = {
            "launches_timed": len(repair_ms), "mean_us": 1e3 * sum(repair_ms) / max(len(repair_ms), 1),
            "what": "the gated launch of the ordinary program enqueued behind every split / grouped launch (cdx.h: run_if): an empty grid "
                    "unless a member lost a granule, then it recomputes the request before the caller can see it (VERDICT r4 weak #8); "
                    "inside `value`, outside roofline.kernel_ms"}
        # the grouped / split routes need the WHOLE device (256 co-resident workgroups): a lost granule switches them off for the process with
        # one warning and the ordinary program -- ~15 % slower at this batch -- serves every later call.  Say so in the line
        from cleandiffuser_amd.engine import runtime2 as _rt2
        _dev = torch.device(device) if not isinstance(device, torch.device) else device
        out["roofline"]["launch_mode"] = {
            "grouped_ok": _rt2._group_ok.get(_dev), "split_ok": _rt2._split_ok.get(_dev),
            "exchange_failure": _rt2.last_exchange_error.get(_dev),
            "repaired_launches": sum(1 for r in repair_ms if r > 0.1),
            "what": "True: the mode passed its first-use check on this device and no exchange has failed since; False: it was switched off "
                    "(whole_chip() refused the device, or a member lost a granule -- `exchange_failure` has the first report) and the timed "
                    "launches ran the ordinary program; repaired_launches: repair launches of the timed region that did real work (> 0.1 ms)"}
        out["replayed_noise"] = {"value": BATCH * replay_reps / el_replay, "unit": "trajectories/s", "ms_per_call": 1e3 * el_replay / replay_reps,
                                 "calls_timed": replay_reps, "what": "the same call on this rank's own 256 trajectories with noise=[z0] "
                                 "(the initial draw outside the timed region): what rounds 1-2 reported as the headline"}
        if strong is not None:
            out["strong_scaling"], out["weak_scaling"] = strong, weak
        if world == 1 and not args.no_other_configs:
            out["predicted_scaling"] = predicted_scaling(agent, device)
            out["other_configs"] = other_configs(device)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_subprocess()
        return json.dumps(out)
    return None


if __name__ == "__main__":
    main()
