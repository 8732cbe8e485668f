"""Writes tests/golden/qgpo_cep.npz: the REAL reference (``oracle.ref_import.import_reference()``) on the cases of tests/cep_cases.py.

    python tools/gen_qgpo_cep_golden.py

Per case the file records the inputs (x, t, obs, soft_label), what three consecutive ``clf.update(x, t, {"soft_label", "obs"}, update_ema)``
calls returned, the gradient of every parameter after the first backward pass (read before ``optim.step`` through a spy on the optimiser;
small cases only) and, after the third call, the mean and mean |.| of every parameter and of every EMA parameter.  Weights are
``load_synth`` streams and are not stored.

A fixture only catches what the reference's own run exercises, so four conditions are asserted per case before anything is written:
  * at most 20 % of the energies have |f| > 9 (the tanh is not saturated);
  * K > 1: max minus min label >= 0.05 in at least half of the groups (the labels are not uniform);
  * K > 1: max_k f and min_k f differ by >= 1e-3 in at least half of the groups (the two statistics are distinct);
  * K > 1: the loss of call 3 differs from call 1 by more than 1e-4 (the optimiser moved something the loss sees).
With K = 1 a group is one row: log-softmax is 0, the loss is 0 in every call and max = min by construction -- the last two conditions
cannot hold there, and what that case pins is that the step runs and leaves the parameters where the reference leaves them.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cep_cases as cc  # noqa: E402
from oracle import cases  # noqa: E402


def run_reference(name, lib):
    case, inp = cc.CASES[name], cc.make_inputs(name)
    clf = cc.build(case, lib)
    x, t, y = cc.tensors(inp)
    with torch.no_grad():
        f = clf.model(x, t.unsqueeze(1).repeat(1, case.K), y["obs"].unsqueeze(1).repeat(1, case.K, 1))[..., 0]
    saturated = float((f.abs() > 9).float().mean())
    spread = float(((f.max(1)[0] - f.min(1)[0]) >= 1e-3).float().mean())
    lab = y["soft_label"][..., 0]
    uneven = float(((lab.max(1)[0] - lab.min(1)[0]) >= 0.05).float().mean())
    grads, step = {}, clf.optim.step

    def spy_step(*a, **k):
        if not grads:
            grads.update({n: p.grad.detach().clone() for n, p in cc.trainable(clf.model)})
        return step(*a, **k)
    clf.optim.step = spy_step
    logs = [clf.update(x, t, y, update_ema=case.update_ema) for _ in range(cc.CALLS)]
    moved = abs(logs[-1]["loss"] - logs[0]["loss"])
    print(f"{name:12s} |f| > 9: {saturated:.2f}  groups with uneven labels {uneven:.2f}  with distinct extremes {spread:.2f}  "
          f"loss {[round(l['loss'], 5) for l in logs]}  max|f| {float(f.abs().max()):.2f}")
    assert saturated <= 0.2, (name, saturated)
    if case.K > 1:
        assert uneven >= 0.5, (name, uneven)
        assert spread >= 0.5, (name, spread)
        assert moved > 1e-4, (name, moved)
    out = dict(inp)
    out["log"] = np.array([[np.nan if l[k] is None else l[k] for k in cc.LOG_KEYS] for l in logs], dtype=np.float64)
    out["sums"], out["sums_ema"] = cc.checksums(clf.model), cc.checksums(clf.model_ema)
    if case.grads:
        out.update({f"grad/{n}": g.numpy() for n, g in grads.items()})
    return out


def main():
    lib = cases.lib_namespace("reference")
    torch.manual_seed(0)
    out = {}
    for name in cc.TABLE:
        for k, v in run_reference(name, lib).items():
            out[f"{name}/{k}"] = np.ascontiguousarray(v, dtype=np.float64 if k in ("log", "sums", "sums_ema") else np.float32)
    np.savez_compressed(cc.GOLDEN, **out)
    print(f"wrote {cc.GOLDEN}: {os.path.getsize(cc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
