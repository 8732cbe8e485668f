"""Writes tests/golden/denoise_steps.npz: the REAL reference (``oracle.ref_import.import_reference()``) on the loss cases of
tests/denoise_cases.py.

    python tools/gen_denoise_step_golden.py

Per case the reference's ``DiscreteDiffusionSDE.loss`` runs in float64 over its own ``DQLMlp`` / ``DVInvMlp`` with ``load_synth`` weights
on the case's seeded inputs; ``add_noise`` is wrapped to record the t and eps it draws.  The file records results only: t, eps, the loss
(float64) and gradients (float32): every parameter's for one hidden-32 and one hidden-64 case (``FULL``), the head's for the others --
the 256-wide net among them -- which keeps the file under 100 KB.  The inputs are the case's own seeded ones (``denoise_cases.inputs``)
and are not stored.

Before anything is written the generator asserts per case that the recorded t takes more than one value (a single row aside), that the
loss is finite and positive and that no recorded gradient is identically zero.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import denoise_cases as dc  # noqa: E402
from oracle import cases as _cases  # noqa: E402

FULL = ("dv32_r16_eps_mask_lw_wr", "dv64_r17_x0_mask_wr")


def run_reference(name, lib):
    case = dc.CASES[name]
    with dc.float64_default():
        agent, inp = dc.build(case, lib, "cpu", torch.float64)
        seen = {}
        add_noise = agent.add_noise

        def recording(x0, t=None, eps=None):
            xt, t, eps = add_noise(x0, t, eps)
            seen.update(t=t.clone(), eps=eps.clone())
            return xt, t, eps
        agent.add_noise = recording
        torch.manual_seed(case.seed)
        loss = agent.loss(inp.x0, inp.obs, **dc.loss_kwargs(inp))
        loss.backward()
    net = agent.model["diffusion"]
    out = {"t": seen["t"].numpy().astype(np.int64), "eps": seen["eps"].numpy().astype(np.float64), "loss": np.float64(loss.item())}
    keep = dc.PARAMS if name in FULL else dc.PARAMS[-2:]
    grads = dict(net.named_parameters())
    for n in keep:
        out["grad/" + n] = grads[n].grad.numpy().astype(np.float32)
        assert float(np.abs(out["grad/" + n]).max()) > 0.0, (name, n)
    assert case.R == 1 or len(set(out["t"].tolist())) > 1, (name, out["t"])
    assert np.isfinite(out["loss"]) and out["loss"] > 0.0, (name, out["loss"])
    print(f"{name}: loss {out['loss']:.8f}  t {out['t'].tolist()[:8]}")
    return out


def main():
    lib = _cases.lib_namespace("reference")
    out = {}
    for name in dc.LOSS_CASES:
        for k, v in run_reference(name, lib).items():
            out[f"{name}/{k}"] = v
    np.savez_compressed(dc.GOLDEN, **out)
    size = os.path.getsize(dc.GOLDEN)
    print(f"wrote {dc.GOLDEN}: {size} bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
