"""Writes tests/golden/horizon_critic.npz: the REAL reference's ``DVHorizonCritic`` (``oracle.ref_import.import_reference()``) on the cases of
tests/hcritic_cases.py.

    python tools/gen_hcritic_golden.py

Per case the file records the forward values, the names and shapes of the ``state_dict`` entries, for the cases with environments the
argmax index per environment, and for the training cases three consecutive MSE / Adam steps: every step's loss, every parameter's
gradient after the first backward pass and, after the third step, the mean and mean |.| of every parameter.  Weights, inputs and targets
are seeded streams and are not stored.

A fixture only catches what the reference's own run exercises, so before anything is written the generator asserts per case that the
reference's fp32 output is within 2e-5 of its own float64 run, that query 0 of the last block attends unevenly (mean largest
probability >= 2 / T), that the last token reaches the output (shifting it by 0.5 moves the output by more than 1e-3 on average), that the
top two values of every environment are more than 1e-3 apart, that the three losses differ and that no first-step gradient is
identically zero.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hcritic_cases as hc  # noqa: E402


def last_block_peak(net, x) -> float:
    """Mean over trajectories and heads of the largest attention probability of query 0 in the last block."""
    seen = []
    att = net.blocks[-1].attn
    handle = att.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach()))
    with torch.no_grad():
        net(x)
        handle.remove()
        u = seen[-1]
        _, p = att(u, u, u, need_weights=True, average_attn_weights=False)          # (b, heads, T, T)
    return float(p[:, :, 0, :].max(dim=-1).values.mean())


def run_reference(name, cls):
    c = hc.CASES[name]
    net, x = hc.build(cls, c), hc.inputs(name)
    with torch.no_grad():
        y = net(x)
        y64 = hc.build(cls, c, dtype=torch.float64)(x.double())
    err = float((y.double() - y64).abs().max())
    assert y.shape == (c.batch, 1) and err < 2e-5, (name, err)
    report = f"{name}: |y| <= {float(y.abs().max()):.3f}, fp32 error {err:.2e}"
    if c.tokens > 2:
        peak = last_block_peak(net, x)
        assert peak >= 2.0 / c.tokens, (name, peak, 2.0 / c.tokens)
        report += f", peak probability {peak:.3f} (uniform {1.0 / c.tokens:.3f})"
    if c.tokens > 1:
        moved = x.clone()
        moved[:, -1] += 0.5
        with torch.no_grad():
            shift = float((net(moved) - y).abs().mean())
        assert shift > 1e-3, (name, shift)
        report += f", last-token shift {shift:.3f}"
    sd = net.state_dict()
    shapes = np.full((len(sd), 2), -1, dtype=np.int64)
    for i, t in enumerate(sd.values()):
        shapes[i, :t.dim()] = t.shape
    out = {"y": y.numpy().astype(np.float32), "keys": np.array(list(sd)), "shapes": shapes}
    if c.envs:
        vals = np.sort(y.numpy().reshape(c.envs, -1), axis=1)
        assert ((vals[:, -1] - vals[:, -2]) > 1e-3).all(), (name, vals[:, -2:])
        out["argmax"] = hc.argmax_per_env(y.numpy(), c).astype(np.int64)
    if c.train:
        steps = hc.run_training(cls, name)
        assert (np.abs(np.diff(steps["loss"])) > 1e-5).all(), (name, steps["loss"])
        for k, v in steps.items():
            if k.startswith("grad/"):
                assert float(np.abs(v).max()) > 0.0, (name, k)
        out.update(steps)
        report += f", losses {steps['loss'].round(5).tolist()}"
    print(report)
    return out


def main():
    cls = hc.critic_class("reference")
    torch.manual_seed(0)
    torch.set_num_threads(8)                    # the thread count the tests run with (tests/conftest.py): ATen's CPU sums follow it
    out = {}
    for name in hc.TABLE:
        for k, v in run_reference(name, cls).items():
            out[f"{name}/{k}"] = v if k in ("keys", "shapes", "argmax") else \
                np.ascontiguousarray(v, dtype=np.float32 if (k.startswith("grad/") or k == "y") else np.float64)
    np.savez_compressed(hc.GOLDEN, **out)
    print(f"wrote {hc.GOLDEN}: {os.path.getsize(hc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
