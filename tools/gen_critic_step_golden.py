"""Writes tests/golden/critic_steps_grouped.npz: the REAL reference (``oracle.ref_import.import_reference()``) on the grouped critic steps
of tests/critic_step_cases.py.

    python tools/gen_critic_step_golden.py

Per case the file records, for three critic steps from seeded weights (``load_synth`` streams) and batches -- the Diffusion-QL antmaze
step with its max-Q backup over 10 sampled actions (reference pipelines/dql_d4rl_antmaze.py:79-98, ``DQLCritic``) and the QGPO step with
its softmax-weighted target over 16 support actions (qgpo_d4rl_mujoco.py:141-152, ``TwinQ``): the loss and the mean TD target of every
step, the gradient of every parameter after the first backward pass and, after the third step, the mean and mean |.| of every
parameter.  Weights and batches are not stored: the file holds recorded results only.

Before anything is written the generator asserts per case that the done mask of every batch is neither all 0 nor all 1, that the
losses differ from step to step, that no first-step gradient is identically zero, and that the group's best candidate is not always
candidate 0.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import critic_step_cases as cc  # noqa: E402
import critic_steps as cs  # noqa: E402


def run_reference(name, U):
    case = cc.GROUPED[name]
    critic, target = cc.grouped_nets(U, case)
    for batch in cc.grouped_batches(case):
        assert 0.0 < float(batch[4].mean()) < 1.0, name
        with torch.no_grad():
            rows = batch[3].unsqueeze(1).repeat(1, case.group, 1).view(-1, case.obs)
            q1 = (target(rows, batch[5])[0] if case.kind == "antmaze" else target(rows, batch[5])).view(-1, case.group)
        assert len(set(q1.argmax(1).tolist())) > 2, (name, q1.argmax(1))
    out = cc.run_grouped(U, case)
    assert (np.abs(np.diff(out["loss"][:, 0])) > 1e-4).all(), (name, out["loss"])
    for k, v in out.items():
        if k.startswith("grad/"):
            assert float(np.abs(v).max()) > 0.0, (name, k)
    print(f"{name}: losses {out['loss'][:, 0].round(5).tolist()}  mean targets {out['loss'][:, 1].round(5).tolist()}")
    return out


def main():
    U = cs.utils_of("reference")
    torch.manual_seed(0)
    out = {}
    for name in cc.GROUPED:
        for k, v in run_reference(name, U).items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v, dtype=np.float32 if k.startswith("grad/") else np.float64)
    np.savez_compressed(cc.GOLDEN, **out)
    print(f"wrote {cc.GOLDEN}: {os.path.getsize(cc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
