"""Writes tests/golden/invdyn_steps.npz: the REAL reference (``oracle.ref_import.import_reference()``) on the inverse-dynamics steps of
tests/regress_step_cases.py.

    python tools/gen_regress_step_golden.py

Per case the file records, for three ``MlpInvDynamic.update`` steps (reference invdynamic/mlp.py:63-69; Adam at lr 1e-3) from seeded
weights (``load_synth`` streams) and batches -- 33 contiguous rows, and the Decision Diffuser slicing ``obs[:, :-1]`` / ``act[:, :-1]`` /
``obs[:, 1:]`` of a (7, 4, 11) batch: the loss of every step, the gradient of every parameter after the first backward pass and, after
the third step, the mean and mean |.| of every parameter.  Weights and batches are not stored: the file holds recorded results only.

Before anything is written the generator asserts per case that the losses differ from step to step and that no first-step gradient is
identically zero.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import regress_step_cases as rc  # noqa: E402


def run_reference(name, cls):
    out = rc.run_invdyn(cls, rc.GOLDEN_CASES[name])
    assert (np.abs(np.diff(out["loss"])) > 1e-5).all(), (name, out["loss"])
    for k, v in out.items():
        if k.startswith("grad/"):
            assert float(np.abs(v).max()) > 0.0, (name, k)
    print(f"{name}: losses {out['loss'].round(6).tolist()}")
    return out


def main():
    cls = rc.invdyn_of("reference")
    torch.manual_seed(0)
    out = {}
    for name in rc.GOLDEN_CASES:
        for k, v in run_reference(name, cls).items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v, dtype=np.float32 if k.startswith("grad/") else np.float64)
    np.savez_compressed(rc.GOLDEN, **out)
    print(f"wrote {rc.GOLDEN}: {os.path.getsize(rc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
