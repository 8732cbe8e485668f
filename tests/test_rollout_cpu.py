"""The differentiable rollout (engine/rollout.py) without a GPU: the torch restatement of the two kernels against torch.autograd through
the package's own host loop in float64, the routing decisions of ``try_rollout``, and the C layout of the ctypes mirror."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_cases as rc  # noqa: E402
import torch_blocks  # noqa: E402
from test_train_paths_cpu import _everything_is_on_the_device  # noqa: E402

RTOL = 1e-10


def _close(got, want, what):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= RTOL * max(scale, 1e-300), (what, float((got - want).abs().max()), scale)


@pytest.mark.parametrize("name", rc.TABLE)
def test_reference_restatement_equals_autograd_through_the_host_loop(name):
    """``reference_forward`` / ``reference_backward`` (explicit formulas, no autograd) against torch.autograd through
    ``_run_plan_torch`` in float64 on the CPU, to 1e-10 relative: actions, d / d obs, d / d temb and every parameter gradient -- for every
    solver the rollout takes, both prediction types, a fix-mask with one masked action column."""
    from cleandiffuser_amd.engine import rollout
    ref = rc.reference(name)
    case = ref.case
    # the case can discriminate: a real gradient reaches the observations and the clamp is neither idle nor everywhere
    print(name, "clamped share per step", ref.share, "max|d/d obs|", float(ref.g_obs.abs().max()), "tie rows", int(ref.ties.sum()))
    assert float(ref.g_obs.abs().max()) > 1e-3
    assert any(0.05 < s < 0.95 for s in ref.share), ref.share
    with rc.float64_default():
        agent, inp = rc.build(case, rc._cases.lib_namespace("amd"), "cpu", torch.float64)
        net = agent.model["diffusion"]
        q = rc.request(agent, ref.plan, ref.xt, inp, inp.obs)
        rollout.reference_forward(q)
        x_s = q.X[q.S].clone().requires_grad_(True)
        act = x_s.clip(agent.x_min, agent.x_max)                    # (the final clip of _sample_common stays an ATen op on the output)
        rc.objective(act, inp, ref.weight).backward()
        _close(act.detach(), ref.act, "actions")
        q.g_out = x_s.grad
        q.G_head, q.g_temb = torch.empty(q.S, q.B, q.A), torch.empty(q.B, q.S * q.E)
        q.g_x, q.g_cond = torch.empty(q.B, q.A), torch.empty(q.B, q.O)
        rollout.reference_backward(q)
        _close(q.g_cond, ref.g_obs, "d / d obs")
        g_temb = q.g_temb.sum(0).view(q.S, q.E)
        _close(g_temb, ref.g_temb, "d / d temb")
        names = ["mid_layer.0", "mid_layer.2", "mid_layer.4", "final_layer"]
        got = dict(zip([f"{n}.{leaf}" for n in names for leaf in ("weight", "bias")], rollout.reference_param_grads(q)))
        # time_mlp's parameters: d / d temb through the (S, E) table, as the device path does it
        net.zero_grad(set_to_none=True)
        t = torch.tensor([st.t for st in ref.plan.steps], dtype=torch.long)
        net.time_mlp(net.map_noise(t)).backward(g_temb)
        got.update({n: p.grad for n, p in net.named_parameters() if p.grad is not None})
        assert set(got) == set(ref.grads) and len(got) == 12
        for n in ref.grads:
            _close(got[n], ref.grads[n], n)


# ------------------------------------------------------------------------------------------------------------------- #
def _agent(lib, cls, sde, **kw):
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(lib.DQLMlp(11, 6, emb_dim=16) if cls == "DQLMlp" else lib.DVInvMlp(5, 6, emb_dim=16, hidden_dim=32), 65)
    return getattr(lib, sde)(net, lib.IdentityCondition(dropout=0.0), x_max=torch.ones(1, 6), x_min=-torch.ones(1, 6), device="cpu",
                             **({"diffusion_steps": 5} if sde == "DiscreteDiffusionSDE" else {}), **kw)


@pytest.fixture
def routed(monkeypatch, amd_lib):
    """``try_rollout`` as ``_sample_common`` calls it, recorded: the two C calls are the torch restatement, the kernel wrappers the
    torch stand-ins, and every tensor says it lives on the device."""
    from cleandiffuser_amd.engine import rollout
    monkeypatch.setattr(rollout, "native_forward", rollout.reference_forward)
    monkeypatch.setattr(rollout, "native_backward", rollout.reference_backward)
    monkeypatch.delenv("CDX_ROLLOUT", raising=False)
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)
    taken = []
    real = rollout.try_rollout

    def spy(*a, **k):
        out = real(*a, **k)
        taken.append(out is not None)
        return out
    monkeypatch.setattr(rollout, "try_rollout", spy)

    def run(agent, solver="ddpm", w_cfg=1.0, grad=True, obs_grad=True, dtype=torch.float32, steps=3, **kw):
        del taken[:]
        g = torch.Generator().manual_seed(3)
        net = agent.model["diffusion"]
        b, o = 20, getattr(net, "obs_dim", 11)
        obs = torch.randn(b, o, generator=g).to(dtype).requires_grad_(obs_grad)
        noise = [torch.randn(b, 6, generator=g).to(dtype) for _ in range(steps + 1)]
        with torch_blocks.emulated(), _everything_is_on_the_device(), torch.set_grad_enabled(grad):
            act, _ = agent.sample(torch.zeros(b, 6, dtype=dtype), solver=solver, n_samples=b, sample_steps=steps, use_ema=False,
                                  condition_cfg=obs, w_cfg=w_cfg, requires_grad=True, noise=noise, **kw)
            if act.requires_grad:
                act.sum().backward()
        return (taken[-1] if taken else False), act.detach(), obs.grad
    return run


@pytest.mark.parametrize("sde", ["DiscreteDiffusionSDE", "ContinuousDiffusionSDE"])
@pytest.mark.parametrize("cls", ["DQLMlp", "DVInvMlp"])
def test_the_rollout_takes_the_row_mlps(routed, amd_lib, monkeypatch, cls, sde):
    """DQLMlp and DVInvMlp under both SDE classes, w_cfg 1 (and 0 for DQLMlp: DVInvMlp needs its condition) -- and what it returns is
    what the host loop returns (CDX_ROLLOUT=0), gradient of the observations included."""
    agent = _agent(amd_lib, cls, sde)
    for solver in ("ddpm", "sde_dpmsolver++_1"):
        took, act, g_obs = routed(agent, solver=solver)
        assert took
        agent.model.zero_grad(set_to_none=True)
        monkeypatch.setenv("CDX_ROLLOUT", "0")
        took0, act0, g_obs0 = routed(agent, solver=solver)
        monkeypatch.delenv("CDX_ROLLOUT")
        assert not took0
        torch.testing.assert_close(act, act0, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(g_obs, g_obs0, rtol=1e-4, atol=1e-5)
    took, _, _ = routed(agent, w_cfg=0.0) if cls == "DQLMlp" else (True, None, None)
    assert took


def test_the_rollout_refuses_what_it_cannot_run(routed, amd_lib, monkeypatch):
    agent = _agent(amd_lib, "DQLMlp", "DiscreteDiffusionSDE")
    assert routed(agent)[0]
    for solver in ("ode_dpmsolver++_2M", "sde_dpmsolver++_2M"):
        assert not routed(agent, solver=solver)[0]                                   # multistep memory: host loop
    assert not routed(agent, w_cfg=0.5)[0]
    assert not routed(agent, grad=False)[0]                                          # no_grad
    monkeypatch.setenv("CDX_TRAIN_NATIVE", "0")
    assert not routed(agent)[0]
    monkeypatch.delenv("CDX_TRAIN_NATIVE")
    monkeypatch.setenv("CDX_ROLLOUT", "0")
    assert not routed(agent)[0]
    monkeypatch.delenv("CDX_ROLLOUT")
    # a frozen net on inputs that need no gradient
    for p in agent.model.parameters():
        p.requires_grad_(False)
    assert not routed(agent, obs_grad=False)[0]
    assert routed(agent, obs_grad=True)[0]                                           # (the observations still want theirs)
    for p in agent.model.parameters():
        p.requires_grad_(True)
    # float64
    with rc.float64_default():
        agent64 = _agent(amd_lib, "DQLMlp", "DiscreteDiffusionSDE")
        agent64.model.double()
        assert not routed(agent64, dtype=torch.float64)[0]

    # a classifier with w_cg > 0
    class _Clf:
        def gradients(self, x, t, c):
            return torch.zeros(x.shape[0], 1), torch.zeros_like(x)

        def logp(self, x, t, c):
            return torch.zeros(x.shape[0], 1)
    agent.classifier = _Clf()
    assert not routed(agent, w_cg=0.5, condition_cg=None)[0]
    assert routed(agent, w_cg=0.0)[0]
    agent.classifier = None


def test_the_rollout_leaves_the_unets_alone(amd_lib, monkeypatch):
    """JannerUNet1d (3-D trajectories): ``try_rollout`` answers None before it draws anything."""
    from cleandiffuser_amd.engine import plan as P, rollout
    from cleandiffuser_amd.diffusion.diffusionsde import _NoiseFeed
    net = amd_lib.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=3)
    agent = amd_lib.DiscreteDiffusionSDE(net, None, diffusion_steps=5, device="cpu")
    plan = P.build_vp_plan("ddpm", agent._alpha_host[[0, 2, 4]], agent._sigma_host[[0, 2, 4]], [0, 2, 4], 2)
    feed = _NoiseFeed([])
    with _everything_is_on_the_device():
        x = torch.zeros(4, 8, 6, requires_grad=True)
        assert rollout.try_rollout(agent, agent.model, plan, x, torch.zeros(4, 8, 6), None, 0.0, 0.0, feed) is None
        assert rollout.try_rollout(agent, agent.model, plan, x[:, 0], torch.zeros(4, 6), None, 0.0, 0.0, feed) is None


def test_rollout_mirror_has_the_c_layout(tmp_path):
    """``CdxRollout`` == ``cdx_rollout`` of include/cdx.h (gcc sizeof / offsetof), and the ABI number of header and binding is 19."""
    from cleandiffuser_amd.engine import rollout, runtime
    fields = [f[0] for f in rollout.CdxRollout._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(cdx_rollout));', 'printf("%d\\n", CDX_ABI_VERSION);', 'printf("%d\\n", CDX_ROLLOUT_MAX_STEPS);']
    src += [f'printf("%zu\\n", offsetof(cdx_rollout, {f}));' for f in fields] + ['return 0;}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert int(next(out)) == ctypes.sizeof(rollout.CdxRollout)
    assert int(next(out)) == runtime.ABI_VERSION == 19
    assert int(next(out)) == rollout.MAX_STEPS
    for f in fields:
        assert getattr(rollout.CdxRollout, f).offset == int(next(out)), f


def test_rollout_validation_fails_loudly():
    """The limits of csrc/cdx_rollout.hip are refused with CDX_EINVAL and a message before anything is launched (no GPU needed)."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import rollout, runtime
    lib = rollout._lib()
    steps = (runtime.CdxStep * 2)()
    steps[0].noise_idx = steps[1].noise_idx = -1
    ok = dict(B=4, A=6, E=16, O=11, W=32, S=2, w1=8, b1=8, w2=8, b2=8, w3=8, b3=8, wh=8, bh=8, temb=8, x_in=8, X=8, P_raw=8, feat=8, Z=8, H=8,
              steps=ctypes.cast(steps, ctypes.c_void_p))

    def refused(fn=lib.cdx_rollout_fwd_f32, **change):
        rc_ = fn(ctypes.byref(rollout.CdxRollout(**{**ok, **change})), None)
        return rc_ == -1 and lib.cdx_last_error()
    assert lib.cdx_rollout_fwd_f32(None, None) == -1 and b"null" in lib.cdx_last_error()
    assert b"multiple of 16" in refused(W=40) and b"multiple of 16" in refused(W=528)
    assert b"A + E + O" in refused(O=500)
    assert b"A must be" in refused(A=65, O=0)
    assert b"S must be" in refused(S=0) and b"S must be" in refused(S=65)
    assert b"weights" in refused(w2=None)
    assert b"saved-tensor" in refused(Z=None)
    assert b"steps" in refused(steps=None)
    assert b"backward buffers" in refused(lib.cdx_rollout_bwd_f32)
    steps[1].kind = 3
    assert b"kind" in refused()
    steps[1].kind, steps[1].vsel = 2, 2
    assert b"vsel" in refused()
    steps[1].vsel, steps[0].noise_idx = 1, 0
    assert b"noise" in refused()
    steps[0].noise_idx = -1
    assert lib.cdx_rollout_fwd_f32(ctypes.byref(rollout.CdxRollout(**{**ok, "B": 0})), None) == 0       # an empty batch is not an error
