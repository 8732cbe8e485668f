"""Writes tests/golden/qgpo_guided.npz: the REAL reference (``oracle.ref_import.import_reference()``) on the cases of tests/energy_cases.py.

    python tools/gen_qgpo_golden.py

Per case the file records the inputs (obs, prior), the Gaussian draws the reference consumed (fed through ``torch.randn_like``, the way
oracle/extra_cases.py feeds them) and what ``sample()`` returned: x and log["log_p"].  Weights are ``load_synth`` streams and are not stored.

A fixture can only catch a wrong step if the reference's own run exercises it, so three conditions are asserted per case on the reference's
output before anything is written:
  * at most half of the final, unclipped elements lie outside the bounds (the result is not just the bounds);
  * median |x(w_cg) - x(w_cg = 0)| >= 1e-3 (the guidance moves the result);
  * in at least one step the clamp changes between 5 % and 95 % of the elements (both branches of the clip run).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import energy_cases as ec  # noqa: E402
from oracle import cases  # noqa: E402


def run_reference(name, lib):
    case, inp = ec.CASES[name], ec.make_inputs(name)
    agent = ec.build(case, lib)
    seen = {"share": [], "final": None}
    clip, logp = agent.clip_prediction, agent.classifier.logp

    def spy_clip(pred, xt, alpha, sigma):
        out = clip(pred, xt, alpha, sigma)
        seen["share"].append(float((out != pred).float().mean()))
        return out

    def spy_logp(x, t, c):
        seen["final"] = x.detach().clone()
        return logp(x, t, c)
    agent.clip_prediction, agent.classifier.logp = spy_clip, spy_logp
    t = torch.from_numpy

    def sample(w_cg):
        with cases.replay_randn(list(t(inp["noise"]))):
            return agent.sample(t(inp["prior"]), **ec.sample_kwargs(case, t(inp["obs"]), w_cg=w_cg))
    x, log = sample(None)
    share, final = list(seen["share"]), seen["final"]
    x_unguided, _ = sample(0.0)
    outside = float(((final > case.bound) | (final < -case.bound)).float().mean())
    shift = float((x - x_unguided).abs().median())
    print(f"{name:18s} outside the bounds {outside:.2f}  median shift {shift:.4f}  clamped per step {[round(s, 2) for s in share]}")
    assert outside <= 0.5, (name, outside)
    assert shift >= 1e-3, (name, shift)
    assert any(0.05 < s < 0.95 for s in share), (name, share)
    return {**inp, "x": x.detach().numpy(), "log_p": log["log_p"].detach().numpy()}


def main():
    lib = cases.lib_namespace("reference")
    torch.manual_seed(0)
    out = {}
    for name in ec.TABLE:
        for k, v in run_reference(name, lib).items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v, dtype=np.float32)
    np.savez_compressed(ec.GOLDEN, **out)
    print(f"wrote {ec.GOLDEN}: {os.path.getsize(ec.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
