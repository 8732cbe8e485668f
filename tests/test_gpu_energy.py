"""The energy-guided loop on the MI355X (csrc/cdx_energy.hip behind engine/energy.py): ``sample()`` against the fixture of the real
reference, the kernel's per-step traces against the float64 restatement, the launch structure, seeded draws, reproducibility."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_cases as ec  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.delenv("CDX_ENERGY", raising=False)


def _spy_run(monkeypatch):
    """The requests the kernel served."""
    from cleandiffuser_amd.engine import energy
    seen, real = [], energy.native_run

    def spy(q):
        real(q)
        seen.append(q)
    monkeypatch.setattr(energy, "native_run", spy)
    return seen


@pytest.mark.parametrize("name", ec.GOLDEN_TABLE)
def test_sample_matches_the_reference_fixture(name, amd_lib, monkeypatch):
    """x and log_p of ``agent.sample(...)`` on the device against what the real reference returned for the same inputs and draws
    (tests/golden/qgpo_guided.npz) at rtol = atol = 1e-4 -- served by ``try_energy_guided`` in one request."""
    case, gold = ec.CASES[name], ec.golden(name)
    seen = _spy_run(monkeypatch)
    agent = ec.build(case, amd_lib, DEV)
    x, log = ec.sample(agent, case, gold, device=DEV)
    torch.cuda.synchronize()
    assert len(seen) == 1, "the fused route did not take this request"
    print(name, "max|d x|", float(np.abs(x.cpu().numpy() - gold["x"]).max()), "max|d log_p|",
          float(np.abs(log["log_p"].cpu().numpy() - gold["log_p"]).max()))
    np.testing.assert_allclose(x.cpu().numpy(), gold["x"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(log["log_p"].cpu().numpy(), gold["log_p"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", ec.TABLE)
def test_every_step_matches_the_float64_restatement(name, amd_lib):
    """``native_run`` against ``reference_run`` in float64 on the CPU, step by step at rtol = atol = 1e-4: the unshifted prediction (the
    denoiser half of a step), the gradient and logp (the energy half), then x_S and log_p."""
    from cleandiffuser_amd.engine import energy
    ref = ec.reference(name)
    with ec.float64_default():
        agent64 = ec.build(ref.case, amd_lib, "cpu", torch.float64)
        want = ec.request(agent64, ref.plan, ref.xt, ref.inp, ref.case)
        energy.reference_run(want)
    agent = ec.build(ref.case, amd_lib, DEV)
    got = ec.request(agent, ref.plan, ref.xt.to(DEV, torch.float32), ref.inp, ref.case)
    energy.native_run(got)
    torch.cuda.synchronize()
    for what in ("trace_pred", "trace_grad", "trace_logp", "x_out", "logp_out"):
        g, w = getattr(got, what).cpu().double().numpy(), getattr(want, what).numpy()
        for s in range(g.shape[0]) if what.startswith("trace") else [slice(None)]:
            print(f"  {name} {what}[{s}]: max|d| {float(np.abs(g[s] - w[s]).max()):.3e}")
            np.testing.assert_allclose(g[s], w[s], rtol=1e-4, atol=1e-4, err_msg=f"{what}, step {s}")


def _qgpo_call(agent, case, steps, obs, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    prior = torch.zeros(case.B, case.A, device=DEV)
    return agent.sample(prior, **{**ec.sample_kwargs(case, obs), "sample_steps": steps})


def test_the_launch_count_does_not_grow_with_the_steps(amd_lib):
    """One ``sample()`` call contains cdx_energy_kernel exactly once and the same number of device kernels at 3 and at 6 sampling steps
    (the host loop grows by the denoiser's, the classifier gradient's and ATen's launches per step)."""
    from torch.autograd import DeviceType
    case = ec.CASES["c_ddpm_eps"]
    agent = ec.build(case, amd_lib, DEV)
    obs = torch.from_numpy(ec.make_inputs("c_ddpm_eps")["obs"]).to(DEV)
    counts = {}
    for steps in (3, 6):
        for _ in range(2):                                  # (plans, tables, transposes and the library are warm)
            _qgpo_call(agent, case, steps, obs)
        prof, _ = profiled(lambda: _qgpo_call(agent, case, steps, obs))
        kernels = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
        print(steps, "steps:", len(kernels), "device kernels")
        assert sum("cdx_energy_kernel" in k for k in kernels) == 1, kernels
        counts[steps] = len(kernels)
    assert counts[3] == counts[6], counts


@pytest.mark.parametrize("solver", ["ddpm", "sde_dpmsolver++_1"])
def test_seeded_draws_do_not_depend_on_the_route(solver, amd_lib, monkeypatch):
    """``torch.manual_seed`` and no ``noise=``: the fused route and the host loop (CDX_ENERGY=0) draw the same noise -- same actions and
    log_p at rtol = atol = 2e-4."""
    case = ec._c(solver=solver)
    agent = ec.build(case, amd_lib, DEV)
    obs = torch.from_numpy(ec.make_inputs("c_ddpm_eps")["obs"]).to(DEV)
    seen = _spy_run(monkeypatch)
    x, log = _qgpo_call(agent, case, case.S, obs, seed=123)
    assert len(seen) == 1
    monkeypatch.setenv("CDX_ENERGY", "0")
    x0, log0 = _qgpo_call(agent, case, case.S, obs, seed=123)
    assert len(seen) == 1
    np.testing.assert_allclose(x.cpu().numpy(), x0.cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(log["log_p"].cpu().numpy(), log0["log_p"].cpu().numpy(), rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("name", ["c_ddpm_eps", "shipped_b50"])
def test_two_calls_give_the_same_bits(name, amd_lib, monkeypatch):
    """No atomics, one fixed lane and order per element: two calls on the same inputs are ``torch.equal``."""
    case, gold = ec.CASES[name], ec.golden(name)
    seen = _spy_run(monkeypatch)
    agent = ec.build(case, amd_lib, DEV)
    (x1, log1), (x2, log2) = ec.sample(agent, case, gold, device=DEV), ec.sample(agent, case, gold, device=DEV)
    assert len(seen) == 2
    assert torch.equal(x1, x2) and torch.equal(log1["log_p"], log2["log_p"])
