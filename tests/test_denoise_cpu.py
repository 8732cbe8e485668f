"""The fused denoising step (engine/denoise.py) without a GPU: the torch restatement of the two kernels against torch.autograd through the
stock module path in float64, the LDS plan and the C layout of the ctypes mirror, the validation of the C entries, the routing decisions
of ``try_loss`` / ``try_predict`` and the record of the real reference."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_cases as dc  # noqa: E402
import torch_blocks  # noqa: E402
from test_train_paths_cpu import _everything_is_on_the_device  # noqa: E402

RTOL = 1e-10


def _close(got, want, what, rtol=RTOL):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"  {what}: max|d| {err:.3e}, max|ref| {scale:.3e}")
    assert err <= rtol * max(scale, 1e-300), (what, err, scale)


@pytest.mark.parametrize("name", dc.TABLE)
def test_reference_restatement_equals_autograd_through_the_modules(name):
    """``reference_forward`` / ``reference_backward`` (explicit formulas, no autograd) against torch.autograd through ``loss()`` / the
    net's own forward in float64 on the CPU, to 1e-10 relative: the loss, pred, every parameter gradient, d / d cond and (prediction
    mode) d / d xt."""
    from cleandiffuser_amd.engine import denoise
    ref = dc.reference(name)
    case = ref.case
    with dc.float64_default():
        agent, inp = dc.build(case, dc._cases.lib_namespace("amd"), "cpu", torch.float64)
        q = dc.request(agent, case, inp)
        denoise.reference_forward(q)
        _close(q.pred, ref.pred, "pred")
        if case.mode == "loss":
            _close(denoise.loss_of(q), ref.value, "loss")
            assert float(ref.value) > 1e-3
        denoise.reference_backward(q)
        got = dict(zip(dc.PARAMS, denoise.reference_param_grads(q)))
        assert set(got) == set(ref.grads) and len(got) == 12
        for n in dc.PARAMS:
            assert float(ref.grads[n].abs().max()) > 0.0, n
            _close(got[n], ref.grads[n], n)
        if ref.g_obs is not None:
            _close(q.g_cond, ref.g_obs, "d / d cond")
        if ref.g_xt is not None:
            _close(q.g_xt, ref.g_xt, "d / d xt")


@pytest.mark.parametrize("name", dc.LOSS_CASES)
def test_loss_equals_the_record_of_the_real_reference(name):
    """``loss()`` in float64 on the CPU with the recorded t and eps against tests/golden/denoise_steps.npz: the loss to 1e-10 relative
    (stored as float64); the gradients the file holds to 2^-23 of their largest element (they are stored as float32: half an ulp of the
    largest element, doubled for the elements' own rounding)."""
    gold = dc.golden(name)
    ref = dc.reference(name, True)
    _close(ref.value, torch.tensor(float(gold["loss"]), dtype=torch.float64), "loss")
    kept = [k[5:] for k in gold if k.startswith("grad/")]
    assert kept and "final_layer.weight" in kept
    for n in kept:
        _close(ref.grads[n], torch.from_numpy(gold["grad/" + n]).double(), n, rtol=2.0 ** -23)


# ------------------------------------------------------------------------------------------------------------------- #
def _lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import denoise
    return denoise._lib()


def test_lds_plan_equals_the_c_side_across_the_bound():
    """``lds_bytes`` == ``cdx_denoise_lds_bytes`` over sizes on both sides of the 160 KiB bound (the entry points refuse the far side)."""
    from cleandiffuser_amd.engine import denoise
    lib = _lib()
    sides = set()
    for a in (1, 6, 64):
        for e in (8, 16, 100, 256):
            for o in (0, 11, 400):
                for w in (16, 256, 512, 1024, 1232, 1248, 2560):
                    want = denoise.lds_bytes(a, e, o, w)
                    assert lib.cdx_denoise_lds_bytes(ctypes.byref(denoise.CdxDenoise(A=a, E=e, O=o, W=w))) == want, (a, e, o, w)
                    sides.add(want <= denoise.MAX_LDS)
                    if want > denoise.MAX_LDS:
                        assert lib.cdx_denoise_fwd_f32(ctypes.byref(denoise.CdxDenoise(R=4, A=a, E=e, O=o, W=w)), None) == -1
    assert sides == {True, False}
    assert denoise.lds_bytes(6, 16, 11, 1232) <= denoise.MAX_LDS < denoise.lds_bytes(6, 16, 11, 1248)
    assert lib.cdx_denoise_lds_bytes(None) < 0 and lib.cdx_denoise_lds_bytes(ctypes.byref(denoise.CdxDenoise(A=0, E=16, W=16))) < 0


def test_denoise_mirror_has_the_c_layout(tmp_path):
    """``CdxDenoise`` == ``cdx_denoise`` of include/cdx.h (gcc sizeof / offsetof); the ABI number stays 19."""
    from cleandiffuser_amd.engine import denoise, runtime
    fields = [f[0] for f in denoise.CdxDenoise._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(cdx_denoise));', 'printf("%d\\n", CDX_ABI_VERSION);']
    src += [f'printf("%zu\\n", offsetof(cdx_denoise, {f}));' for f in fields] + ['return 0;}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert int(next(out)) == ctypes.sizeof(denoise.CdxDenoise)
    assert int(next(out)) == runtime.ABI_VERSION == 19
    for f in fields:
        assert getattr(denoise.CdxDenoise, f).offset == int(next(out)), f


def test_denoise_validation_fails_loudly():
    """The limits of csrc/cdx_denoise.hip are refused with CDX_EINVAL and a message before anything is launched (no GPU needed)."""
    from cleandiffuser_amd.engine import denoise
    lib = _lib()
    names = [f[0] for f in denoise.CdxDenoise._fields_[8:]]
    fwd = [n for n in names if not n.startswith(("g_", "G_"))]
    ok = dict(R=4, A=6, E=16, O=11, W=32, loss_mode=1, **{n: 8 for n in fwd})

    def refused(fn=lib.cdx_denoise_fwd_f32, **change):
        rc_ = fn(ctypes.byref(denoise.CdxDenoise(**{**ok, **change})), None)
        return rc_ == -1 and lib.cdx_last_error()
    assert lib.cdx_denoise_fwd_f32(None, None) == -1 and b"null" in lib.cdx_last_error()
    assert lib.cdx_denoise_bwd_f32(None, None) == -1 and b"null" in lib.cdx_last_error()
    assert b"multiple of 16" in refused(W=40) and b"multiple of 16" in refused(W=528)
    assert b"A + E + O" in refused(O=500)
    assert b"A must be" in refused(A=65, O=0)
    assert b"2 E" in refused(E=264, O=0)
    assert b"bad size" in refused(E=0)
    assert b"weights" in refused(tw2=None) and b"weights" in refused(bh=None)
    assert b"emb0" in refused(emb0=None)
    assert b"x0 / eps" in refused(xt=None, s=None)
    assert b"target" in refused(x0=None)                                             # (given-input mode, x0-prediction: no target)
    assert b"cond given" in refused(O=0)
    assert b"saved-tensor" in refused(Z=None) and b"saved-tensor" in refused(pred=None)
    assert b"loss_part" in refused(loss_part=None)
    assert b"backward buffers" in refused(lib.cdx_denoise_bwd_f32)
    assert b"g_loss" in refused(lib.cdx_denoise_bwd_f32, G_head=8, G_t2=8)
    assert b"g_loss" in refused(lib.cdx_denoise_bwd_f32, G_head=8, G_t2=8, g_loss=8, loss_mode=0)
    assert b"g_cond" in refused(lib.cdx_denoise_bwd_f32, G_head=8, G_t2=8, g_loss=8, g_cond=8, cond=None)
    for fn in (lib.cdx_denoise_fwd_f32, lib.cdx_denoise_bwd_f32):                   # an empty batch is not an error
        assert fn(ctypes.byref(denoise.CdxDenoise(R=0, A=6, E=16, O=11, W=32)), None) == 0


# ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture
def routed(monkeypatch):
    """The two routes as ``loss()`` / ``approx_action`` take them, recorded: the two C calls are the torch restatement, the kernel
    wrappers the torch stand-ins, and every tensor says it lives on the device."""
    from cleandiffuser_amd.engine import denoise
    calls = []

    def fwd(q):
        calls.append("fwd")
        denoise.reference_forward(q)

    def bwd(q):
        calls.append("bwd")
        denoise.reference_backward(q)
    monkeypatch.setattr(denoise, "native_forward", fwd)
    monkeypatch.setattr(denoise, "native_backward", bwd)
    monkeypatch.setenv("CDX_DENOISE", "1")
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)
    return calls


def _grads(agent):
    return {n: p.grad.clone() for n, p in agent.model["diffusion"].named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", ["dv32_r16_eps_mask_lw_wr", "dql_r17_eps_nocond", "dv64_r17_x0_mask_wr"])
def test_loss_takes_the_fused_node_and_equals_the_stock_route(name, routed, amd_lib, monkeypatch):
    """A seeded ``loss()`` + ``backward()``: one forward and one backward pass of the node, the value, every parameter gradient and
    d / d obs of the per-layer route (CDX_DENOISE=0), and the same state of the RNG afterwards."""
    case = dc.CASES[name]
    agent, inp = dc.build(case, amd_lib)
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("CDX_DENOISE", route)
        del routed[:]
        agent.model.zero_grad(set_to_none=True)
        obs = None if inp.obs is None else inp.obs.clone().requires_grad_(True)
        torch.manual_seed(5)
        with torch_blocks.emulated(), _everything_is_on_the_device():
            loss = agent.loss(inp.x0, obs, **dc.loss_kwargs(inp))
            loss.backward()
        assert routed == (["fwd", "bwd"] if route == "1" else []), routed
        out[route] = (loss.detach(), _grads(agent), None if obs is None else obs.grad, torch.get_rng_state())
    (l1, g1, o1, s1), (l0, g0, o0, s0) = out["1"], out["0"]
    assert torch.equal(s1, s0)
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-6)
    assert set(g1) == set(g0) and len(g1) == 12
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], rtol=1e-4, atol=1e-6)
    if o0 is not None:
        torch.testing.assert_close(o1, o0, rtol=1e-4, atol=1e-6)


def test_parameter_gradients_land_in_place_inside_a_scope(routed, amd_lib, monkeypatch):
    """Inside ``train.grads_in_place(params)`` the twelve weight-gradient products add straight into ``p.grad`` and autograd gets None."""
    from cleandiffuser_amd.engine import train
    case = dc.CASES["dv64_r33_eps_lw"]
    agent, inp = dc.build(case, amd_lib)
    handed, real = [], train._weight_grads

    def spy(*a, **k):
        out = real(*a, **k)
        handed.append(out)
        return out
    monkeypatch.setattr(train, "_weight_grads", spy)
    runs = []
    for in_place in (False, True):
        agent.model.zero_grad(set_to_none=True)
        del handed[:]
        with torch_blocks.emulated(), _everything_is_on_the_device(), dc.recorded_draws(agent, inp):
            loss = agent.loss(inp.x0, inp.obs)
            with (train.grads_in_place(agent.model.parameters()) if in_place else torch.enable_grad()):
                loss.backward()
        assert len(handed) == 6 and all((dw is None and db is None) == in_place for dw, db in handed), handed
        runs.append(_grads(agent))
    assert len(runs[0]) == 12
    for n in runs[0]:
        torch.testing.assert_close(runs[1][n], runs[0][n], rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("name", ["dv32_r17_pred", "dv64_r33_pred_nocondgrad", "dql_r16_pred_nocond"])
def test_approx_action_takes_the_prediction_node(name, routed, amd_lib, monkeypatch):
    """``approx_action`` + ``backward()`` on the fused node against the module call (CDX_DENOISE=0): pred, parameter gradients, d / d obs."""
    from cleandiffuser_amd.utils.policy_steps import approx_action
    case = dc.CASES[name]
    agent, inp = dc.build(case, amd_lib)
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("CDX_DENOISE", route)
        del routed[:]
        agent.model.zero_grad(set_to_none=True)
        obs = inp.obs.clone().requires_grad_(case.cond_grad) if inp.obs is not None else torch.zeros(case.R, 11)
        torch.manual_seed(6)
        with torch_blocks.emulated(), _everything_is_on_the_device():
            pred = approx_action(agent, inp.x0, obs) if inp.obs is not None else None
            if pred is None:                              # (condition=None: the node under the module's own rule, through try_predict)
                from cleandiffuser_amd.engine import denoise
                net = agent.model["diffusion"]
                pred = denoise.try_predict(net, dc.noised(agent, inp), inp.t, None) if route == "1" else net(dc.noised(agent, inp), inp.t, None)
            dc.objective(pred, inp).backward()
        assert routed == (["fwd", "bwd"] if route == "1" else []), routed
        out[route] = (pred.detach(), _grads(agent), obs.grad)
    torch.testing.assert_close(out["1"][0], out["0"][0], rtol=1e-5, atol=1e-6)
    for n in out["0"][1]:
        torch.testing.assert_close(out["1"][1][n], out["0"][1][n], rtol=1e-4, atol=1e-6)
    assert (out["1"][2] is None) == (out["0"][2] is None)
    if out["0"][2] is not None:
        torch.testing.assert_close(out["1"][2], out["0"][2], rtol=1e-4, atol=1e-6)


def test_every_refusal_returns_none_before_anything_is_drawn(routed, amd_lib, monkeypatch):
    from cleandiffuser_amd.engine import denoise
    from cleandiffuser_amd.utils import load_synth
    case = dc.CASES["dv32_r17_pred"]
    agent, inp = dc.build(case, amd_lib)
    net = agent.model["diffusion"]
    xt = dc.noised(agent, inp)

    def refused(agent=agent, x0=inp.x0, obs=inp.obs, grad=True, on_device=True):
        """(``try_loss`` answered None, ``try_predict`` answered None) for this request -- `x0` stands for xt in the second -- with the
        RNG stream untouched."""
        state = torch.get_rng_state()
        with torch_blocks.emulated(), (_everything_is_on_the_device() if on_device else torch.enable_grad()), torch.set_grad_enabled(grad):
            loss = denoise.try_loss(agent, x0, obs, {})
            pred = denoise.try_predict(agent.model["diffusion"], xt if x0 is inp.x0 else x0, inp.t, obs)
        assert torch.equal(torch.get_rng_state(), state), "a refusal drew from the RNG"
        return loss is None, pred is None

    with torch_blocks.emulated(), _everything_is_on_the_device():
        assert denoise.try_loss(agent, inp.x0, inp.obs, {}) is not None                   # (the request itself is one the node takes)
        assert denoise.try_predict(net, xt, inp.t, inp.obs) is not None
    for var in ("CDX_DENOISE", "CDX_TRAIN_NATIVE"):
        monkeypatch.setenv(var, "0")
        assert refused() == (True, True), var
        monkeypatch.setenv(var, "1")
    monkeypatch.delenv("CDX_DENOISE")                                                    # unset: the measured default
    with torch_blocks.emulated(), _everything_is_on_the_device():
        assert (denoise.try_loss(agent, inp.x0, inp.obs, {}) is not None) == denoise.DEFAULT_ON
        assert (denoise.try_predict(net, xt, inp.t, inp.obs) is not None) == denoise.DEFAULT_ON
    monkeypatch.setenv("CDX_DENOISE", "1")
    assert refused(on_device=False) == (True, True)                                      # not a ROCm device
    assert refused(grad=False) == (True, True)                                           # grad mode off
    assert refused(x0=inp.x0.double()) == (True, True)                                   # not fp32
    assert refused(x0=inp.x0[:, None]) == (True, True)                                   # not 2-D
    assert refused(x0=inp.x0.clone().requires_grad_(True))[0]                            # x0 itself needs a gradient (loss mode)
    assert refused(obs=None) == (True, True)                                             # DVInvMlp without its condition
    with torch_blocks.emulated(), _everything_is_on_the_device():                        # a condition of another width
        assert denoise.try_predict(net, xt, inp.t, inp.obs[:, :-1]) is None
    # a net _trunk does not take, a time_mlp of another shape
    other = amd_lib.DiscreteDiffusionSDE(load_synth(amd_lib.IDQLMlp(14, 3, emb_dim=16, hidden_dim=32), 3), amd_lib.IdentityCondition(dropout=0.0),
                                         diffusion_steps=dc.STEPS)
    assert refused(agent=other) == (True, True)
    tm = net.time_mlp
    net.time_mlp = nn.Sequential(nn.Linear(16, 48), nn.Mish(), nn.Linear(48, 16))
    assert refused() == (True, True)
    net.time_mlp = tm
    # nothing to differentiate
    agent.model.requires_grad_(False)
    assert refused() == (True, True)
    agent.model.requires_grad_(True)
    # inside update()'s scope
    with denoise.inside_update():
        assert refused() == (True, True)
    # an LDS plan over the bound
    monkeypatch.setattr(denoise, "MAX_LDS", 1024)
    assert refused() == (True, True)


def test_a_capturing_stream_is_refused(routed, amd_lib, monkeypatch):
    from cleandiffuser_amd.engine import denoise
    case = dc.CASES["dv32_r17_pred"]
    agent, inp = dc.build(case, amd_lib)
    with torch_blocks.emulated(), _everything_is_on_the_device():
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        state = torch.get_rng_state()
        assert denoise.try_loss(agent, inp.x0, inp.obs, {}) is None
        assert denoise.try_predict(agent.model["diffusion"], dc.noised(agent, inp), inp.t, inp.obs) is None
        assert torch.equal(torch.get_rng_state(), state)
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        assert denoise.try_loss(agent, inp.x0, inp.obs, {}) is not None


def test_update_keeps_its_own_route(routed, amd_lib, monkeypatch):
    """``update()`` with CDX_DENOISE=1: ``graphed_step`` is asked and the eager pair runs over ``train.dql_forward``; the fused node is
    not taken."""
    from cleandiffuser_amd.engine import train
    case = dc.CASES["dv32_r16_eps_mask_lw_wr"]
    agent, inp = dc.build(case, amd_lib)
    seen = []
    for fn in ("graphed_step", "dql_forward"):
        real = getattr(train, fn)
        monkeypatch.setattr(train, fn, (lambda real, fn: lambda *a, **k: (seen.append(fn), real(*a, **k))[1])(real, fn))
    monkeypatch.setattr(agent, "_apply_gradients", lambda *a, **k: None)               # (the optimiser's own launch needs the device)
    with torch_blocks.emulated(), _everything_is_on_the_device():
        log = agent.update(inp.x0, inp.obs, **dc.loss_kwargs(inp))
    assert np.isfinite(log["loss"])
    assert routed == [] and "graphed_step" in seen and "dql_forward" in seen, (routed, seen)
