"""The differentiable rollout on the MI355X (csrc/cdx_rollout.hip behind engine/rollout.py): the two kernels against the float64 CPU run of
the host loop, the launch structure, seeded draws, in-place parameter gradients."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_cases as rc  # noqa: E402
import tower_cases as tc  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.setenv("CDX_ROLLOUT", "1")
    monkeypatch.setenv("CDX_TRAIN_NATIVE", "1")


def _spy_forward(monkeypatch):
    """Requests the forward kernel served (with step 0 of what it saved, copied before backward writes over Z)."""
    from cleandiffuser_amd.engine import rollout
    seen, real = [], rollout.native_forward

    def spy(q):
        real(q)
        seen.append((q, q.P_raw[0].clone(), q.Z[:, 0].clone()))
    monkeypatch.setattr(rollout, "native_forward", spy)
    return seen


@pytest.mark.parametrize("name", list(rc.CASES))
def test_rollout_kernels_match_the_float64_host_loop(name, amd_lib, monkeypatch):
    """Actions (rtol = atol = 1e-4), d / d obs and every parameter gradient (max|d| <= 2e-4 max|g_ref|: the bars of the existing DQL
    test) of ``sample(requires_grad=True)`` + ``backward()`` on the fused route against the float64 CPU run of the host loop; the saved
    P_raw / Z of step 0 against ``reference_forward`` at 1e-4.  Rows whose clamp decision is a tie in float64 (|P_raw - bound| <
    1e-4 (1 + |bound|)) carry weight 0 in the objective on both sides; they are at most 5 % of the rows."""
    ref = rc.reference(name)
    case = ref.case
    assert int(ref.ties.sum()) <= 0.05 * case.B, (int(ref.ties.sum()), case.B)
    seen = _spy_forward(monkeypatch)
    agent, inp = rc.build(case, amd_lib, DEV)
    obs = inp.obs.clone().requires_grad_(True)
    act = rc.sample(agent, case, inp, obs)
    rc.objective(act, inp, ref.weight.to(DEV, torch.float32)).backward()
    torch.cuda.synchronize()
    assert len(seen) == 1, "the fused route did not take this request"
    q, p_raw0, z0 = seen[0]
    print(name, "max|d act|", float((act.detach().cpu().double() - ref.act).abs().max()), "tie rows", int(ref.ties.sum()))
    np.testing.assert_allclose(p_raw0.cpu().numpy(), ref.q0.P_raw[0].numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(z0.cpu().numpy(), ref.q0.Z[:, 0].numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(act.detach().cpu().numpy(), ref.act.numpy(), rtol=1e-4, atol=1e-4)
    got = {n: p.grad for n, p in agent.model["diffusion"].named_parameters() if p.grad is not None}
    assert set(got) == set(ref.grads) and len(got) == 12
    got["obs"], want = obs.grad, dict(ref.grads, obs=ref.g_obs)
    for n, g_ref in want.items():
        err, scale = float((got[n].cpu().double() - g_ref).abs().max()), float(g_ref.abs().max())
        print(f"  {n}: max|d| {err:.3e}, max|g_ref| {scale:.3e}")
        assert err <= 2e-4 * scale, (n, err, scale)


def _policy_step(agent, steps, b=64, seed=None):
    if seed is not None:
        torch.manual_seed(seed)
    obs = torch.ones(b, 11, device=DEV).requires_grad_(True)
    act, _ = agent.sample(torch.zeros(b, 6, device=DEV), solver="ddpm", n_samples=b, sample_steps=steps, use_ema=False,
                          condition_cfg=obs, w_cfg=1.0, requires_grad=True)
    (-act.sum(-1).mean()).backward()
    return act.detach()


def _dql_agent(amd_lib, **kw):
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.DQLMlp(11, 6, emb_dim=16), 65).to(DEV)
    return amd_lib.DiscreteDiffusionSDE(net, amd_lib.IdentityCondition(dropout=0.0), x_max=torch.ones(1, 6), x_min=-torch.ones(1, 6),
                                        diffusion_steps=12, device=DEV, **kw)


def test_the_launch_count_does_not_grow_with_the_steps(amd_lib):
    """``sample(requires_grad=True)`` + ``backward()``: the same number of device kernels at 3 and at 6 sampling steps, with
    cdx_rollout_fwd / cdx_rollout_bwd exactly once each (the host loop grows by ~25 + 50 launches per step)."""
    from torch.autograd import DeviceType
    agent = _dql_agent(amd_lib)
    counts = {}
    for steps in (3, 6):
        for _ in range(2):                                  # (plans, weight layouts and the library are warm)
            agent.model.zero_grad(set_to_none=True)
            _policy_step(agent, steps)
        agent.model.zero_grad(set_to_none=True)
        prof, _ = profiled(lambda: _policy_step(agent, steps))
        kernels = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
        print(steps, "steps:", len(kernels), "device kernels")
        assert sum("cdx_rollout_fwd" in k for k in kernels) == 1 and sum("cdx_rollout_bwd" in k for k in kernels) == 1, kernels
        counts[steps] = len(kernels)
    assert counts[3] == counts[6], counts


@pytest.mark.parametrize("solver", ["ddpm", "sde_dpmsolver++_1"])
def test_seeded_draws_do_not_depend_on_the_route(solver, amd_lib, monkeypatch):
    """``torch.manual_seed`` and no ``noise=``: the fused route and the host loop (CDX_ROLLOUT=0) draw the same noise -- same actions."""
    agent = _dql_agent(amd_lib)
    seen = _spy_forward(monkeypatch)

    def run():
        torch.manual_seed(123)
        obs = torch.linspace(-1, 1, 6 * 11, device=DEV).view(6, 11).requires_grad_(True)
        return agent.sample(torch.zeros(6, 6, device=DEV), solver=solver, n_samples=6, sample_steps=5, use_ema=False, condition_cfg=obs,
                            w_cfg=1.0, requires_grad=True)[0].detach()
    fused = run()
    assert len(seen) == 1
    monkeypatch.setenv("CDX_ROLLOUT", "0")
    host = run()
    assert len(seen) == 1
    np.testing.assert_allclose(fused.cpu().numpy(), host.cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_parameter_gradients_land_in_place_inside_a_scope(amd_lib, monkeypatch):
    """Inside ``train.grads_in_place(params)`` the rollout's weight-gradient products add straight into ``p.grad`` (queued, one batched
    launch when the pass ends) and equal what autograd accumulates outside a scope to 1e-6 relative."""
    from cleandiffuser_amd.engine import train
    case = rc.CASES["dv48_ddpm_eps"]
    agent, inp = rc.build(case, amd_lib, DEV)
    seen = _spy_forward(monkeypatch)
    params = list(agent.model.parameters())
    w = torch.ones(case.B, device=DEV)

    def run(in_place):
        agent.model.zero_grad(set_to_none=True)
        act = rc.sample(agent, case, inp, inp.obs.clone().requires_grad_(True))
        loss = rc.objective(act, inp, w)
        if in_place:
            handed = []
            real = train._weight_grads

            def spy(*a, **k):
                out = real(*a, **k)
                handed.append(out)
                return out
            monkeypatch.setattr(train, "_weight_grads", spy)
            with train.grads_in_place(params):
                loss.backward()
            monkeypatch.setattr(train, "_weight_grads", real)
            assert handed and all(dw is None and db is None for dw, db in handed), "gradients went through autograd inside the scope"
        else:
            loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in agent.model.named_parameters() if p.grad is not None}
    outside, inside = run(False), run(True)
    assert len(seen) == 2 and set(outside) == set(inside) and len(inside) == 12
    for n in outside:
        err, scale = float((inside[n] - outside[n]).abs().max()), float(outside[n].abs().max())
        print(f"  {n}: max|d| {err:.3e}, max|g| {scale:.3e}")
        assert err <= 1e-6 * scale, (n, err, scale)


def test_weights_off_16_byte_alignment_give_the_aligned_results(amd_lib, monkeypatch):
    """``_trunk`` admits a contiguous weight wherever it starts.  With every Linear weight at element offset 1 of a flat buffer (K a
    multiple of 4 in every layer: F = W = 512, so only the base address turns the float4 weight loads off) the fused route takes the
    request, and actions, d / d obs and every parameter gradient equal the aligned run to 1e-6 relative."""
    name = "limits_b17_a64_f512_w512_s2"
    case = rc.CASES[name]
    seen = _spy_forward(monkeypatch)
    weight = torch.ones(case.B, device=DEV)
    runs = []
    for unaligned in (False, True):
        agent, inp = rc.build(case, amd_lib, DEV)
        if unaligned:
            tc.repoint_off_alignment(agent.model["diffusion"])
        obs = inp.obs.clone().requires_grad_(True)
        act = rc.sample(agent, case, inp, obs)
        rc.objective(act, inp, weight).backward()
        torch.cuda.synchronize()
        got = {n: p.grad.clone() for n, p in agent.model["diffusion"].named_parameters() if p.grad is not None}
        got["obs"], got["act"] = obs.grad.clone(), act.detach().clone()
        runs.append(got)
    assert len(seen) == 2, "the fused route did not take both requests"
    assert set(runs[0]) == set(runs[1]) and len(runs[0]) == 14
    for n, want in runs[0].items():
        err, scale = float((runs[1][n] - want).abs().max()), float(want.abs().max())
        print(f"  {n}: max|d| {err:.3e}, max|aligned| {scale:.3e}")
        assert scale > 0 and err <= 1e-6 * scale, (n, err, scale)
