"""The energy-guided loop (engine/energy.py) without a GPU: the torch restatement of the kernel against the package's own host loop in
float64 and against the fixture of the real reference, the routing decisions of ``try_energy_guided``, the C layout of the ctypes mirror
and the messages of the C side's validation."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_cases as ec  # noqa: E402
import torch_blocks  # noqa: E402
from test_train_paths_cpu import _everything_is_on_the_device  # noqa: E402

RTOL = 1e-10


def _close(got, want, what):
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= RTOL * max(scale, 1e-300), (what, float((got - want).abs().max()), scale)


@pytest.mark.parametrize("name", ec.TABLE)
def test_reference_restatement_equals_the_host_loop(name):
    """``reference_run`` in float64 against the host loop (CDX_ENERGY=0, the classifier gradient by autograd) to 1e-10 relative: x, log_p
    and, step by step, the unshifted prediction, the gradient and logp -- both SDE classes, every solver family the kernel takes, both
    prediction types, a fix-mask, w_cfg = 0, one row, one full tile, the shipped widths."""
    from cleandiffuser_amd.engine import energy
    ref = ec.reference(name)
    print(name, "clamped share per step", ref.share, "max|grad|", float(ref.grad.abs().max()))
    assert float(ref.grad.abs().max()) > 1e-3 and any(0.05 < s < 0.95 for s in ref.share)
    with ec.float64_default():
        agent = ec.build(ref.case, ec._cases.lib_namespace("amd"), "cpu", torch.float64)
        q = ec.request(agent, ref.plan, ref.xt, ref.inp, ref.case)
        energy.reference_run(q)
    _close(q.trace_pred, ref.pred, "prediction per step")
    _close(q.trace_grad, ref.grad, "gradient per step")
    _close(q.trace_logp, ref.logp, "logp per step")
    _close(q.x_out.clip(agent.x_min, agent.x_max), ref.x, "x")
    _close(q.logp_out, ref.log_p, "log_p")


@pytest.mark.parametrize("name", ec.GOLDEN_TABLE)
def test_reference_restatement_matches_the_fixture(name):
    """``reference_run`` in float32 on the CPU against what the real reference returned (tests/golden/qgpo_guided.npz) at the project's
    rtol = atol = 1e-4; the request is the one of the float64 run (plan, x_T) in float32."""
    from cleandiffuser_amd.engine import energy
    ref, gold = ec.reference(name), ec.golden(name)
    for k in ("obs", "prior", "noise"):
        np.testing.assert_array_equal(gold[k], ref.inp[k])
    agent = ec.build(ref.case, ec._cases.lib_namespace("amd"))
    q = ec.request(agent, ref.plan, ref.xt.float(), gold, ref.case, trace=False)
    energy.reference_run(q)
    np.testing.assert_allclose(q.x_out.clip(agent.x_min, agent.x_max).numpy(), gold["x"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(q.logp_out.numpy(), gold["log_p"], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------------- #
class _CountingFeed:
    """``_NoiseFeed`` that counts what is drawn from it."""

    def __init__(self, feed):
        self.feed, self.draws = feed, 0

    def many(self, ref, n):
        self.draws += n
        return self.feed.many(ref, n)

    def like(self, ref):
        self.draws += 1
        return self.feed.like(ref)

    def reserve(self, ref, n):
        return self.feed.reserve(ref, n)


class _HostLoop(Exception):
    pass


def _host_loop(*a, **k):
    raise _HostLoop


def _linear_silu(a, w, bias=None, act="none", **kw):
    y = torch_blocks.linear(a, w, bias, **kw)
    return torch.nn.functional.silu(y) if act == "silu" else y


@pytest.fixture
def routed(monkeypatch, amd_lib):
    """``try_energy_guided`` as ``_sample_common`` calls it, recorded: the C call is the torch restatement, the kernel wrappers the torch
    stand-ins, and every tensor says it lives on the device.  -> run(agent, case, ...) = (took?, draws the router made, x, log_p)."""
    from cleandiffuser_amd.engine import blocks, energy
    monkeypatch.setattr(energy, "native_run", energy.reference_run)
    monkeypatch.delenv("CDX_ENERGY", raising=False)
    calls = []
    real = energy.try_energy_guided

    def spy(solver, model, plan, xt, prior, cond_vec, w_cfg, condition_cg, w_cg, feed):
        counting = _CountingFeed(feed)
        out = real(solver, model, plan, xt, prior, cond_vec, w_cfg, condition_cg, w_cg, counting)
        calls.append((out is not None, counting.draws))
        return out
    monkeypatch.setattr(energy, "try_energy_guided", spy)

    def run(agent, case, dtype=torch.float32, **kw):
        """(a request the router refuses ends where the host loop would begin: `_HostLoop`)"""
        del calls[:]
        agent._run_plan_torch = _host_loop
        x = logp = None
        with torch_blocks.emulated(), _everything_is_on_the_device():
            blocks.linear = _linear_silu           # (the stand-in has no fused SiLU: t_layer, the condition MLP; emulated() restores it)
            try:
                x, log = ec.sample(agent, case, ec.make_inputs("c_ddpm_eps"), dtype=dtype, **kw)
                logp = log["log_p"]
            except _HostLoop:
                pass
            finally:
                del agent._run_plan_torch
        took, draws = calls[-1] if calls else (False, 0)
        return took, draws, x, logp
    return run


def _agent(amd_lib, **over):
    case = ec._c(**over)
    return ec.build(case, amd_lib), case


@pytest.mark.parametrize("sde", ["DiscreteDiffusionSDE", "ContinuousDiffusionSDE"])
def test_the_fused_route_takes_what_the_issue_lists(routed, amd_lib, monkeypatch, sde):
    """Both SDE classes, the one-step solvers, w_cfg 0 and 1 -- and what it returns is what the host loop returns on the CPU (where the
    classifier gradient is autograd's), log_p included."""
    for over in (dict(), dict(solver="ddim"), dict(solver="sde_dpmsolver++_1", predict_noise=False), dict(solver="ode_dpmsolver_1"),
                 dict(w_cfg=0.0), dict(mask=True)):
        agent, case = _agent(amd_lib, sde=sde, **over)
        took, draws, x, logp = routed(agent, case)
        assert took, over
        x0, log0 = ec.sample(agent, case, ec.make_inputs("c_ddpm_eps"))
        torch.testing.assert_close(x, x0, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(logp, log0["log_p"], rtol=1e-5, atol=1e-5)


def test_the_fused_route_refuses_before_it_draws(routed, amd_lib, monkeypatch):
    """Every refusal of the issue's list answers None with nothing drawn from the feed."""
    agent, case = _agent(amd_lib)
    assert routed(agent, case)[0]

    def refused(agent=agent, case=case, **kw):
        took, draws, _, _ = routed(agent, case, **kw)
        return not took and draws == 0
    # the switch
    monkeypatch.setenv("CDX_ENERGY", "0")
    assert refused()
    monkeypatch.delenv("CDX_ENERGY")
    # multistep memory, a classifier-free-guidance pair
    for solver in ("ode_dpmsolver++_2M", "sde_dpmsolver++_2M"):
        assert refused(solver=solver)
    assert refused(w_cfg=0.5)
    # w_cfg = 1 without a condition: the host loop's business
    assert refused(condition_cfg=None)
    # the observations of the classifier: missing, a wrong width, float64
    assert refused(condition_cg=None)
    assert refused(condition_cg=torch.zeros(case.B, case.O + 1))
    assert refused(condition_cg=torch.zeros(case.B, case.O, dtype=torch.float64))
    # float64 states
    with ec.float64_default():
        agent64 = ec.build(case, amd_lib, "cpu", torch.float64)
        assert refused(agent64, dtype=torch.float64)
    # a classifier in train mode; another classifier class; another network under it; a ReLU hidden layer
    agent.classifier.model_ema.train()
    assert refused()
    agent.classifier.model_ema.eval()
    keep = agent.classifier
    agent.classifier = amd_lib.MSEClassifier(amd_lib.MLPNNClassifier(case.A, case.O, 32, [48], timestep_emb_type="positional"), device="cpu")
    assert refused()
    agent.classifier = keep
    act = keep.model_ema.mlp.mlp[0][1]
    keep.model_ema.mlp.mlp[0][1] = torch.nn.ReLU()
    assert refused()
    keep.model_ema.mlp.mlp[0][1] = act
    assert routed(agent, case)[0]
    # another denoiser; a width that is no multiple of 16; a subclass of SfBCUNet
    other, _ = _agent(amd_lib, hidden=[64, 40, 32])
    assert refused(other)

    class Mine(amd_lib.SfBCUNet):
        pass
    sub, _ = _agent(amd_lib)
    sub.model_ema["diffusion"].__class__ = Mine
    assert refused(sub)
    # per-sample bounds
    agent.x_max = torch.ones(case.B, 1, case.A)
    assert refused()
    agent.x_max = case.bound * torch.ones(case.A)
    # history and autograd never reach the router
    took, draws, _, _ = routed(agent, case, preserve_history=True)
    assert not took and draws == 0
    took, draws, _, _ = routed(agent, case, requires_grad=True)
    assert not took and draws == 0
    # w_cg = 0: nothing to guide (the unguided one-launch route is not what this test is about: it answers None here)
    from cleandiffuser_amd.engine import dispatch
    monkeypatch.setattr(dispatch, "try_fused_sample", lambda *a, **k: None)
    took, draws, _, _ = routed(agent, case, w_cg=0.0)
    assert not took and draws == 0
    assert routed(agent, case)[0]


def test_the_lds_plan_is_a_limit_of_the_route(amd_lib):
    """``lds_bytes`` restates the kernel's plan (compared with the C side below); a classifier whose saved pre-activations do not fit
    beside the denoiser is outside the limits."""
    from cleandiffuser_amd.engine import energy
    agent = ec.build(ec.CASES["shipped_b50"], amd_lib)
    den = energy.describe_denoiser(agent.model_ema["diffusion"])
    clf = energy.describe_classifier(agent.classifier.model_ema)
    assert [(r.in_, r.in2, r.out) for r in den.rows] == [(6, 0, 512), (512, 0, 256), (256, 0, 128), (128, 0, 128), (128, 128, 256),
                                                          (256, 256, 512)] and den.n_down == 3
    assert [r.ws is None for r in den.rows] == [False, False, False, True, True, True]
    assert 100 * 1024 < energy.lds_bytes(den, clf) <= energy.MAX_LDS and energy.within_limits(den, clf, 15)
    assert not energy.within_limits(den, clf, 65) and not energy.within_limits(den, clf, 0)
    clf.hidden = [512, 512, 512, 512]
    assert energy.lds_bytes(den, clf) > energy.MAX_LDS and not energy.within_limits(den, clf, 15)


# ------------------------------------------------------------------------------------------------------------------- #
def test_energy_mirror_has_the_c_layout(tmp_path):
    """``CdxEnergyGuided`` / ``CdxEnergyBlock`` == the structs of include/cdx.h (gcc sizeof / offsetof); the addition is purely additive:
    the ABI number of header and binding is 19 (18 until cdx_optim_args gained the host-computed complements; this entry itself was additive)."""
    from cleandiffuser_amd.engine import energy, runtime
    c_name = lambda f: "in" if f == "in_" else f                                     # noqa: E731
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){',
           'printf("%d\\n", CDX_ABI_VERSION);',
           'printf("%d %d %d\\n", CDX_ENERGY_MAX_STEPS, CDX_ENERGY_MAX_BLOCKS, CDX_ENERGY_MAX_HIDDEN);']
    pairs = (("cdx_energy_block", energy.CdxEnergyBlock), ("cdx_energy_guided", energy.CdxEnergyGuided))
    for c_struct, mirror in pairs:
        src.append(f'printf("%zu\\n", sizeof({c_struct}));')
        src += [f'printf("%zu\\n", offsetof({c_struct}, {c_name(f[0])}));' for f in mirror._fields_]
    src.append('return 0;}')
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert int(next(out)) == runtime.ABI_VERSION == 19
    assert [int(next(out)) for _ in range(3)] == [energy.MAX_STEPS, energy.MAX_BLOCKS, energy.MAX_HIDDEN]
    for _, mirror in pairs:
        assert int(next(out)) == ctypes.sizeof(mirror)
        for f in mirror._fields_:
            assert getattr(mirror, f[0]).offset == int(next(out)), f[0]


def _c_side():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import energy, runtime
    return energy, runtime, energy._lib()


def test_energy_validation_fails_loudly():
    """The limits of csrc/cdx_energy.hip are refused with CDX_EINVAL and a message before anything is launched (no GPU needed)."""
    energy, runtime, lib = _c_side()
    steps = (runtime.CdxStep * 2)()
    steps[0].noise_idx = steps[1].noise_idx = -1
    cg = (ctypes.c_float * 2)()
    blk = dict(w1=8, b1=8, w2=8, b2=8, wc=8, bc=8)
    # a two-level U-Net on A = 6: down 6 -> 32 -> 16, mid 16, up [16 | 16] -> 32
    table = [dict(in_=6, in2=0, out=32, ws=8, bs=8, **blk), dict(in_=32, in2=0, out=16, ws=8, bs=8, **blk), dict(in_=16, in2=0, out=16, **blk),
             dict(in_=16, in2=16, out=32, ws=8, bs=8, **blk)]
    ok = dict(B=4, A=6, E=16, O=11, S=2, Ec=16, n_blocks=4, n_down=2, n_hidden=2, predict_noise=1, clip=1, out_w=8, out_b=8, den_c=8, obs=8,
              obs_w=8, obs_b=8, act_w=8, act_b=8, act_wt=8, clf_wo=8, clf_bo=8, clf_temb=8, x_in=8, x_out=8, steps=steps, cg_scale=cg)

    def refused(rows=None, hidden=(32, 32), clf_null=None, **change):
        rows = table if rows is None else rows
        arr = (energy.CdxEnergyBlock * len(rows))(*[energy.CdxEnergyBlock(**r) for r in rows])
        g = energy.CdxEnergyGuided(**{**ok, "blocks": arr, **change})
        for l, w in enumerate(hidden):
            g.hidden[l], g.clf_w[l], g.clf_b[l], g.clf_wt[l] = w, 8, 8, 8
        if clf_null is not None:
            g.clf_wt[clf_null] = None
        rc_ = lib.cdx_energy_guided_run(ctypes.byref(g), None)
        return rc_ == -1 and lib.cdx_last_error()

    def row(i, **change):
        return [dict(r, **change) if j == i else r for j, r in enumerate(table)]
    assert lib.cdx_energy_guided_run(None, None) == -1 and b"null request" in lib.cdx_last_error()
    assert b"bad size" in refused(A=0) and b"bad size" in refused(B=-1)
    assert b"A must be" in refused(A=65)
    assert b"E and Ec" in refused(E=129) and b"E and Ec" in refused(Ec=129)
    assert b"O must be" in refused(O=513)
    assert b"S must be" in refused(S=0) and b"S must be" in refused(S=65)
    assert b"n_blocks" in refused(n_blocks=0) and b"n_blocks" in refused(n_blocks=9) and b"n_blocks" in refused(n_down=5)
    assert b"n_hidden" in refused(n_hidden=0) and b"n_hidden" in refused(n_hidden=5)
    assert b"blocks" in refused(blocks=None)
    assert b"multiple of 16" in refused(hidden=(40, 32)) and b"multiple of 16" in refused(hidden=(32, 528))
    assert b"multiple of 16" in refused(rows=row(2, out=24)) and b"multiple of 16" in refused(rows=row(0, out=528))
    assert b"concat input" in refused(rows=row(3, in2=1040))
    assert b"chain" in refused(rows=row(1, in_=48))
    assert b"identity skip" in refused(rows=row(1, ws=None, bs=None))
    assert b"concat partner" in refused(rows=row(3, in2=32))
    assert b"more concat inputs" in refused(n_down=0)
    assert b"steps / cg_scale" in refused(steps=None) and b"steps / cg_scale" in refused(cg_scale=None)
    assert b"denoiser weights" in refused(rows=row(2, w2=None)) and b"denoiser weights" in refused(rows=row(0, bs=None))
    assert b"denoiser weights" in refused(out_w=None) and b"denoiser weights" in refused(den_c=None)
    assert b"classifier weights" in refused(act_wt=None) and b"classifier weights" in refused(clf_null=1)
    assert b"classifier weights" in refused(clf_temb=None)
    assert b"obs / x_in" in refused(obs=None) and b"obs / x_in" in refused(x_in=None)
    assert b"x_out" in refused(x_out=None)
    assert b"fix_mask" in refused(fix_mask=8)
    # an LDS plan over 160 KiB: 512-wide blocks with a 512 + 512 concat and four 512-wide classifier layers
    wide = [dict(in_=6, in2=0, out=512, ws=8, bs=8, **blk), dict(in_=512, in2=0, out=512, **blk), dict(in_=512, in2=0, out=512, **blk),
            dict(in_=512, in2=512, out=512, ws=8, bs=8, **blk), dict(in_=512, in2=512, out=512, ws=8, bs=8, **blk)]
    assert b"LDS plan" in refused(rows=wide, n_blocks=5, n_down=2, hidden=(512, 512, 512, 512), n_hidden=4)
    steps[1].kind = 3
    assert b"kind" in refused()
    steps[1].kind, steps[1].vsel = 2, 2
    assert b"vsel" in refused()
    steps[1].vsel, steps[1].flags = 1, 1
    assert b"flags" in refused()
    steps[1].flags, steps[0].noise_idx = 0, 0
    assert b"noise" in refused()
    steps[0].noise_idx = -1
    assert b"n_blocks" in refused(B=0, n_blocks=0)                                 # (sizes are checked for an empty batch too)
    arr = (energy.CdxEnergyBlock * 4)(*[energy.CdxEnergyBlock(**r) for r in table])
    g = energy.CdxEnergyGuided(**{**ok, "B": 0, "blocks": arr})
    g.hidden[0] = g.hidden[1] = 32
    assert lib.cdx_energy_guided_run(ctypes.byref(g), None) == 0                   # an empty batch is not an error


@pytest.mark.parametrize("name", ["c_ddpm_eps", "shipped_b50"])
def test_the_python_lds_plan_is_the_c_plan(name, amd_lib):
    """``energy.lds_bytes`` (what the router checks) == ``cdx_energy_guided_lds_bytes`` (what the launch uses)."""
    energy, _, lib = _c_side()
    agent = ec.build(ec.CASES[name], amd_lib)
    den = energy.describe_denoiser(agent.model_ema["diffusion"])
    clf = energy.describe_classifier(agent.classifier.model_ema)
    arr = (energy.CdxEnergyBlock * len(den.rows))(*[energy.CdxEnergyBlock(in_=r.in_, in2=r.in2, out=r.out, ws=None if r.ws is None else 8)
                                                     for r in den.rows])
    g = energy.CdxEnergyGuided(B=1, A=den.A, E=den.E, O=clf.O, S=1, Ec=clf.Ec, n_blocks=len(den.rows), n_down=den.n_down,
                               n_hidden=len(clf.hidden), blocks=arr)
    for l, w in enumerate(clf.hidden):
        g.hidden[l] = w
    assert lib.cdx_energy_guided_lds_bytes(ctypes.byref(g)) == energy.lds_bytes(den, clf)
