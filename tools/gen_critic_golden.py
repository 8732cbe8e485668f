"""Writes tests/golden/critic_towers.npz: the REAL reference (``oracle.ref_import.import_reference()``) on the cases of tests/critic_steps.py.

    python tools/gen_critic_golden.py

Per case the file records, for three IQL half-steps of the IDQL pipeline (``IDQLVNet`` / ``IDQLQNet`` with its frozen target) and for three
Diffusion-QL critic steps (``DQLCritic`` with its frozen target) from seeded weights and batches: the losses of every step, the gradient
of every parameter after the first backward pass and, after the third step, the mean and mean |.| of every parameter.  Weights and
batches are seeded streams and are not stored: the file holds recorded results only.

A fixture only catches what the reference's own run exercises, so before anything is written the generator asserts per case that the
done mask of every batch is neither all 0 nor all 1, that the reference's own losses differ from step to step, and that no first-step
gradient is identically zero.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import critic_steps as cs  # noqa: E402


def run_reference(name, U):
    case = cs.CASES[name]
    for batch in cs.batches(case):
        done = float(batch[4].mean())
        assert 0.0 < done < 1.0, (name, done)
    out = {**cs.run_iql(U, case), **cs.run_dql(U, case)}
    for key in ("iql/loss", "dql/loss"):
        losses = out[key].reshape(cs.STEPS, -1)
        assert (np.abs(np.diff(losses, axis=0)) > 1e-4).all(), (name, key, losses)
    for k, v in out.items():
        if "/grad/" in k:
            assert float(np.abs(v).max()) > 0.0, (name, k)
    print(f"{name}: iql losses {out['iql/loss'].round(5).tolist()}  dql losses {out['dql/loss'].round(5).tolist()}")
    return out


def main():
    U = cs.utils_of("reference")
    torch.manual_seed(0)
    out = {}
    for name in cs.TABLE:
        for k, v in run_reference(name, U).items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v, dtype=np.float32 if "/grad/" in k else np.float64)
    np.savez_compressed(cs.GOLDEN, **out)
    print(f"wrote {cs.GOLDEN}: {os.path.getsize(cs.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
