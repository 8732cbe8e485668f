"""QGPO's contrastive energy training step (engine/cep.py) without a GPU: the torch restatement of the kernel against float64 autograd of
the package's own ``QGPOClassifier.loss`` and against the fixture of the real reference, the routing decisions of ``try_cep_update``, the
LDS plan, the C layout of the ctypes mirror and the messages of the C side's validation."""
import ctypes
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cep_cases as cc  # noqa: E402
import torch_blocks  # noqa: E402
from test_train_paths_cpu import _everything_is_on_the_device  # noqa: E402

RTOL64 = 1e-10
GRAD_BAR = 2e-4                # x max |g_ref| per parameter: the bar of tests/test_gpu_rollout.py


def _close64(got, want, what):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= RTOL64 * max(scale, 1e-300), (what, float((got - want).abs().max()), scale)


def clip_factor(case, gold):
    """What ``clip_grad_norm_`` multiplied the reference's first gradients by before the optimiser's spy read them (1 without a clip):
    the fused route clips inside the optimiser's step, so its ``.grad`` tensors are the unclipped ones."""
    return 1.0 if case.clip is None else min(1.0, case.clip / (float(gold["log"][0][4]) + 1e-6))


def assert_grads(got: dict, gold: dict, what, factor=1.0):
    """Every gradient of the fixture with max |d| <= 2e-4 x max |g_ref| (a reference gradient that is exactly zero is matched exactly);
    `factor`: ``clip_factor``."""
    names = [k[5:] for k in gold if k.startswith("grad/")]
    assert names and set(names) == set(got), (what, names, list(got))
    for n in names:
        ref = np.asarray(gold["grad/" + n], dtype=np.float64)
        err, bar = float(np.abs(factor * np.asarray(got[n], dtype=np.float64) - ref).max()), GRAD_BAR * float(np.abs(ref).max())
        print(f"  {what} {n}: max|d| {err:.3e}  bar {bar:.3e}")
        assert err <= bar, (what, n, err, bar)


def assert_log(log: dict, row, what):
    """A returned dict against a row of the fixture's ``log`` at rtol = atol = 1e-4 (grad_norm None <-> NaN)."""
    for k, want in zip(cc.LOG_KEYS, row):
        if np.isnan(want):
            assert log[k] is None, (what, k, log[k])
        else:
            print(f"  {what} {k}: {log[k]:.7f} (reference {want:.7f})")
            np.testing.assert_allclose(log[k], want, rtol=1e-4, atol=1e-4, err_msg=f"{what} {k}")


@pytest.mark.parametrize("name", cc.TABLE)
def test_reference_step_equals_float64_autograd(name, amd_lib):
    """``reference_step`` in float64 against autograd of ``QGPOClassifier.loss`` to 1e-10 relative: loss, the three statistics and every
    parameter gradient (K = 1: exactly zero on both sides)."""
    from cleandiffuser_amd.engine import cep
    ref = cc.reference(name)
    clf = cc.build(ref.case, amd_lib, "cpu", torch.float64)
    q = cc.request(clf, *cc.tensors(ref.inp, dtype=torch.float64))
    out = cep.reference_step(q)
    _close64(out.loss, ref.loss, "loss")
    for k in ("f_max", "f_mean", "f_min"):
        _close64(getattr(out, k), ref.stats[k], k)
    names = [n for n, _ in cc.trainable(clf.model)]
    assert len(names) == len(out.grads)
    for n, g in zip(names, out.grads):
        _close64(g.reshape(ref.grads[n].shape), ref.grads[n], n)
    if ref.case.K == 1:
        assert ref.loss == 0.0 and all(float(g.abs().max()) == 0.0 for g in out.grads)
    else:
        assert max(float(g.abs().max()) for g in out.grads) > 1e-3


@pytest.mark.parametrize("name", cc.GOLDEN_TABLE)
def test_reference_step_matches_the_fixture(name, amd_lib):
    """``reference_step`` in float32 on the CPU against the first ``update()`` of the real reference (tests/golden/qgpo_cep.npz): the
    scalars at rtol = atol = 1e-4, every recorded gradient at 2e-4 x max |g_ref|."""
    from cleandiffuser_amd.engine import cep
    case, gold = cc.CASES[name], cc.golden(name)
    inp = cc.make_inputs(name)
    for k in inp:
        np.testing.assert_array_equal(gold[k], inp[k])
    clf = cc.build(case, amd_lib)
    out = cep.reference_step(cc.request(clf, *cc.tensors(gold)))
    got = {k: float(getattr(out, k)) for k in cc.LOG_KEYS[:4]}
    assert_log({**got, "grad_norm": None}, list(gold["log"][0][:4]) + [np.nan], name)
    if case.grads:
        assert_grads({n: g.reshape(p.shape).numpy() for (n, p), g in zip(cc.trainable(clf.model), out.grads)}, gold, name,
                     clip_factor(case, gold))
    else:
        assert not any(k.startswith("grad/") for k in gold)


# ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture
def routed(monkeypatch):
    """``try_cep_update`` as ``QGPOClassifier.update`` calls it, recorded: the C call is the torch restatement, the kernel wrappers the
    torch stand-ins, every tensor says it lives on the device, and the optimiser -- a FusedAdam whose device kernels cannot run here --
    takes torch's own clip / Adam / EMA sequence.  -> run(clf, x, t, y, ...) = (took?, what update() returned)."""
    from cleandiffuser_amd.engine import cep, optim
    monkeypatch.setattr(cep, "native_step", cep.reference_step)
    monkeypatch.setattr(optim, "native_device", lambda t: False)
    monkeypatch.setattr(cep, "_fused_optimiser", lambda opt: isinstance(opt, optim.FusedAdam))
    monkeypatch.delenv("CDX_CEP", raising=False)
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)
    calls = []
    real = cep.try_cep_update

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(cep, "try_cep_update", spy)

    def run(clf, x, t, y, update_ema=True, on_device=True):
        del calls[:]
        with torch_blocks.emulated(), (_everything_is_on_the_device() if on_device else torch.enable_grad()):
            log = clf.update(x, t, y, update_ema=update_ema)
        return calls == [True], log
    return run


def _state(clf):
    return [(p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for p in clf.model.parameters()]


def _untouched(clf, before):
    return all(torch.equal(p.detach(), p0) and ((p.grad is None) if g0 is None else torch.equal(p.grad, g0))
               for p, (p0, g0) in zip(clf.model.parameters(), before))


@pytest.mark.parametrize("name", cc.GOLDEN_TABLE)
def test_three_updates_on_the_fused_route_reproduce_the_fixture(name, routed, amd_lib):
    """The accepted cases are taken, and with the native call replaced by ``reference_step`` three ``update()`` calls reproduce the real
    reference: each returned dict and, after the third call, the checksums of every parameter and every EMA parameter at rtol = atol =
    1e-4 -- zero_grad, the weight-gradient jobs, the clip, Adam and the EMA in the order the reference runs them."""
    case, gold = cc.CASES[name], cc.golden(name)
    clf = cc.build(case, amd_lib)
    x, t, y = cc.tensors(gold)
    for i in range(cc.CALLS):
        took, log = routed(clf, x, t, y, update_ema=case.update_ema)
        assert took, (name, i)
        assert_log(log, gold["log"][i], f"{name} call {i}")
    np.testing.assert_allclose(cc.checksums(clf.model), gold["sums"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(cc.checksums(clf.model_ema), gold["sums_ema"], rtol=1e-4, atol=1e-4)
    if not case.update_ema:
        assert not np.allclose(gold["sums"], gold["sums_ema"], rtol=1e-4, atol=1e-6)


def test_the_first_gradients_on_the_fused_route_are_the_fixtures(routed, amd_lib, monkeypatch):
    """The ``.grad`` tensors the route leaves for the optimiser (read through a spy on its step) against the reference's first backward."""
    name = "k4_ragged"
    case, gold = cc.CASES[name], cc.golden(name)
    clf = cc.build(case, amd_lib)
    seen, step = {}, clf.optim.step

    def spy_step(*a, **k):
        seen.update({n: p.grad.detach().clone().numpy() for n, p in cc.trainable(clf.model)})
        return step(*a, **k)
    clf.optim.step = spy_step
    took, _ = routed(clf, *cc.tensors(gold))
    assert took
    assert_grads(seen, gold, name, clip_factor(case, gold))


def test_the_fused_route_refuses_before_it_writes(routed, amd_lib, monkeypatch):
    """Every refusal of the issue's list: ``update()`` runs its autograd body (``try_cep_update`` answered None), and the refusal itself
    leaves the parameters and their ``.grad`` untouched."""
    from cleandiffuser_amd.engine import cep
    case = cc.CASES["k4_ragged"]
    x, t, y = cc.tensors(cc.make_inputs("k4_ragged"))

    def fresh(**over):
        return cc.build(SimpleNamespace(**{**vars(case), **over}), amd_lib)

    def refused(clf=None, x=x, t=t, y=y, on_device=True, body=True):
        clf = fresh() if clf is None else clf
        before = _state(clf)
        with torch_blocks.emulated(), (_everything_is_on_the_device() if on_device else torch.enable_grad()):
            assert cep.try_cep_update(clf, x, t, y, True) is None      # the refusal alone: nothing written
        assert _untouched(clf, before)
        if not body:
            return True
        took, log = routed(clf, x, t, y, on_device=on_device)   # and the autograd body still serves the call
        return not took and set(log) == set(cc.LOG_KEYS) and not _untouched(clf, before)

    assert routed(fresh(), x, t, y)[0]
    # the switches
    for var in ("CDX_CEP", "CDX_TRAIN_NATIVE"):
        monkeypatch.setenv(var, "0")
        assert refused(), var
        monkeypatch.delenv(var)
    # not on the device; float64; not (B, K, A); an empty batch; K that does not divide 16
    assert refused(on_device=False)
    clf64 = cc.build(case, amd_lib, "cpu", torch.float64)
    x64, t64, y64 = cc.tensors(cc.make_inputs("k4_ragged"), dtype=torch.float64)
    assert refused(clf64, x=x64, t=t64, y=y64)
    with torch_blocks.emulated(), _everything_is_on_the_device():
        for bad in (x[:, 0], x[:0], x[:, :3]):
            clf = fresh()
            before = _state(clf)
            assert cep.try_cep_update(clf, bad, t[:bad.shape[0]], y, True) is None and _untouched(clf, before)
    y3 = {"soft_label": y["soft_label"][:, :3].contiguous(), "obs": y["obs"]}
    assert refused(x=x[:, :3].contiguous(), y=y3)
    # subclasses of the classifier and of the network
    class MyClf(amd_lib.QGPOClassifier):
        pass

    class MyNet(amd_lib.QGPONNClassifier):
        pass
    clf = fresh()
    clf.__class__ = MyClf
    assert refused(clf)
    clf = fresh()
    clf.model.__class__ = MyNet
    assert refused(clf)
    # another time embedding (the positional ones do not take the (b, K) times of the autograd body either: the refusal alone)
    from cleandiffuser_amd.utils import load_synth
    for emb in ("positional", "fourier"):
        net = load_synth(amd_lib.QGPONNClassifier(case.O, case.A, case.Ec, list(case.hidden), emb), 73)
        assert refused(amd_lib.QGPOClassifier(net, optim_params={"lr": cc.LR}), body=False)
    # a ReLU hidden layer; an output activation
    clf = fresh()
    clf.model.mlp.mlp[0][1] = torch.nn.ReLU()
    assert refused(clf)
    clf = fresh()
    clf.model.mlp.mlp[-1] = torch.nn.Tanh()
    assert refused(clf)
    # a frozen parameter
    clf = fresh()
    clf.model.act_proj.bias.requires_grad_(False)
    assert refused(clf)
    # another optimiser
    clf = fresh()
    clf.optim = torch.optim.Adam(clf.model.parameters(), lr=cc.LR)
    assert refused(clf)
    # the labels and the observations: a wrong shape, float64, missing
    with torch_blocks.emulated(), _everything_is_on_the_device():
        for bad in ({"soft_label": y["soft_label"][..., 0], "obs": y["obs"]},
                    {"soft_label": y["soft_label"].double(), "obs": y["obs"]}, {"soft_label": y["soft_label"], "obs": y["obs"].double()},
                    {"soft_label": y["soft_label"], "obs": y["obs"][:, :-1]}, {"soft_label": y["soft_label"]}):
            clf = fresh()
            before = _state(clf)
            assert cep.try_cep_update(clf, x, t, bad, True) is None and _untouched(clf, before)
    # sizes outside the kernel's limits: a width that is no multiple of 16, a width over 512
    assert refused(fresh(hidden=[40]))
    assert refused(fresh(hidden=[528]))
    # an input that wants its own gradient
    assert refused(x=x.clone().requires_grad_())
    # autograd switched off
    clf = fresh()
    before = _state(clf)
    with torch.no_grad(), torch_blocks.emulated(), _everything_is_on_the_device():
        assert cep.try_cep_update(clf, x, t, y, True) is None
    assert _untouched(clf, before)
    assert routed(fresh(), x, t, y)[0]


# ------------------------------------------------------------------------------------------------------------------- #
def _c_side():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import cep
    return cep, cep._lib()


def test_the_python_lds_plan_is_the_c_plan():
    """``cep.lds_bytes`` (what the router checks) == ``cdx_cep_lds_bytes`` (what the launch uses) over a sweep of sizes, the shipped ones
    among them; four 512-wide layers are over the 160 KiB."""
    cep, lib = _c_side()
    seen = 0
    for o, ec, hidden in itertools.product((1, 7, 17, 100, 512), (2, 16, 22, 64, 128),
                                           ([16], [32, 48], [256, 256, 256], [512], [512, 512, 512], [512, 512, 512, 512])):
        desc = SimpleNamespace(O=o, Ec=ec, A=6, hidden=hidden)
        g = cep.CdxCepStep(B=1, K=16, A=6, O=o, Ec=ec, n_hidden=len(hidden))
        for l, w in enumerate(hidden):
            g.hidden[l] = w
        assert lib.cdx_cep_lds_bytes(ctypes.byref(g)) == cep.lds_bytes(desc), (o, ec, hidden)
        assert cep.within_limits(desc, 16) == (cep.lds_bytes(desc) <= cep.MAX_LDS)
        seen += 1
    assert seen == 150
    shipped = SimpleNamespace(O=17, Ec=64, A=6, hidden=[256, 256, 256])
    assert 64 * 1024 < cep.lds_bytes(shipped) <= cep.MAX_LDS and cep.within_limits(shipped, 16) and not cep.within_limits(shipped, 3)
    assert cep.lds_bytes(SimpleNamespace(O=17, Ec=64, A=6, hidden=[512] * 4)) > cep.MAX_LDS


def test_cep_validation_fails_loudly():
    """The limits of csrc/cdx_cep.hip are refused with CDX_EINVAL and a message before anything is launched (no GPU needed)."""
    cep, lib = _c_side()
    ok = dict(B=4, K=4, A=6, O=11, Ec=16, n_hidden=2, x=8, obs=8, temb=8, soft=8, obs_w=8, obs_b=8, act_w=8, act_b=8, wo=8, bo=8, feat=8,
              H=8, G=8, G_out=8, G_act=8, G_obs=8, stats=8)

    def refused(hidden=(32, 32), w_null=None, **change):
        g = cep.CdxCepStep(**{**ok, **change})
        for l, w in enumerate(hidden):
            g.hidden[l], g.w[l], g.b[l] = w, 8, 8
        if w_null is not None:
            g.w[w_null] = None
        rc = lib.cdx_cep_step_f32(ctypes.byref(g), None)
        return rc == -1 and lib.cdx_last_error()

    assert lib.cdx_cep_step_f32(None, None) == -1 and b"null request" in lib.cdx_last_error()
    assert lib.cdx_cep_lds_bytes(None) == -1 and b"null request" in lib.cdx_last_error()
    assert b"bad size" in refused(A=0) and b"bad size" in refused(B=-1) and b"bad size" in refused(Ec=0)
    for k in (0, 3, 5, 32):
        assert b"K must divide 16" in refused(K=k), k
    assert b"32 bits" in refused(B=2 ** 30, K=16)
    assert b"A must be" in refused(A=65)
    assert b"Ec must be" in refused(Ec=129)
    assert b"O must be" in refused(O=513)
    assert b"n_hidden" in refused(n_hidden=0) and b"n_hidden" in refused(n_hidden=5)
    assert b"multiple of 16" in refused(hidden=(40, 32)) and b"multiple of 16" in refused(hidden=(32, 528)) and b"multiple of 16" in refused(hidden=(32, 0))
    assert b"LDS plan" in refused(hidden=(512, 512, 512, 512), n_hidden=4)
    for name in ("x", "obs", "temb", "soft"):
        assert b"x / obs / temb / soft" in refused(**{name: None}), name
    for name in ("obs_w", "obs_b", "act_w", "act_b", "wo", "bo"):
        assert b"null pointer: weights" in refused(**{name: None}), name
    assert b"null pointer: weights" in refused(w_null=1)
    for name in ("feat", "H", "G", "G_out", "G_act", "G_obs", "stats"):
        assert b"null pointer: outputs" in refused(**{name: None}), name
    assert b"K must divide 16" in refused(B=0, K=3)                                  # (sizes are checked for an empty batch too)
    g = cep.CdxCepStep(B=0, K=16, A=6, O=11, Ec=16, n_hidden=1)
    g.hidden[0] = 32
    assert lib.cdx_cep_step_f32(ctypes.byref(g), None) == 0                          # an empty batch is not an error


def test_cep_mirror_has_the_c_layout(tmp_path):
    """``CdxCepStep`` == ``cdx_cep_step`` of include/cdx.h (gcc sizeof / offsetof); the addition is purely additive: the ABI number of
    header and binding did not move with it (19 now: cdx_optim_args carries the host-computed 1 - beta complements)."""
    from cleandiffuser_amd.engine import cep, runtime
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){', 'printf("%d\\n", CDX_ABI_VERSION);',
           'printf("%d\\n", CDX_ENERGY_MAX_HIDDEN);', 'printf("%zu\\n", sizeof(cdx_cep_step));']
    src += [f'printf("%zu\\n", offsetof(cdx_cep_step, {f[0]}));' for f in cep.CdxCepStep._fields_]
    src.append('return 0;}')
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert int(next(out)) == runtime.ABI_VERSION == 19
    assert int(next(out)) == cep.MAX_HIDDEN
    assert int(next(out)) == ctypes.sizeof(cep.CdxCepStep)
    for f in cep.CdxCepStep._fields_:
        assert getattr(cep.CdxCepStep, f[0]).offset == int(next(out)), f[0]
