"""CPU checks of the fused critic step (engine/critic_step.py, utils/critic_steps.py): the case table's own claims, the torch restatement
of the launch against float64 autograd of the pipelines' inline steps, the LDS plan against the library's, every refusal, the eager
fallback against the fixture of the real reference, the ctypes mirrors against the header."""
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
import critic_step_cases as cc  # noqa: E402
import critic_steps as cs  # noqa: E402


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for k in ("CDX_CRITIC_STEP", "CDX_TRAIN_NATIVE", "CDX_TRAIN_INPLACE_GRADS", "CDX_TOWER"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def refs():
    """The float64 autograd reference of every case: computed once, read only."""
    return {name: cc.autograd_reference(cc.CASES[name]) for name in cc.TABLE}


def test_the_case_table_covers_what_it_claims(refs):
    """On the reference alone: the group's maximum is not always candidate 0, expectile cases see advantages of both signs, no gradient
    is identically zero, the losses differ between cases, and the table has the shapes the kernel's paths depend on."""
    losses = [float(refs[n]["loss"]) for n in cc.TABLE]
    assert len({round(v, 9) for v in losses}) == len(losses), losses
    for name in cc.TABLE:
        case, ref = cc.CASES[name], refs[name]
        if case.group > 1:
            assert len(set(ref["picks"].tolist())) > 1, (name, ref["picks"])
        if case.loss == "expectile":
            assert bool((ref["adv"] < 0).any()) and bool((ref["adv"] > 0).any()), name
        for t, grads in enumerate(ref["grads"]):
            for i, g in enumerate(grads):
                assert (float(g.abs().max()) > 0) != ((t, i) in cc.ALL_ZERO_GRADS.get(name, ())), (name, t, i)
    C = cc.CASES.values()
    assert {c.rows for c in C} >= {1, 16, 17, 33} and {c.a0 + c.a1 for c in C} >= {14, 23}
    assert {c.live_towers for c in C} == {1, 2} and any(c.b0 + c.b1 != c.a0 + c.a1 and c.target_towers == 1 for c in C)
    assert {(c.group, c.rows) for c in C} >= {(10, 5), (10, 17), (16, 3)} and any(512 in c.live for c in C)
    assert {c.done for c in C} >= {"zeros", "ones", "mixed"} and {c.tau for c in C if c.loss == "expectile"} == {0.7, 0.5}
    assert any(len(set(c.live[:-1])) > 1 for c in C)
    q = cc.CASES["qgpo_k16_r3_beta3"]                      # the softmax weights are uneven: the largest holds more than twice 1 / K
    live, target = cc.build(q, dtype=torch.float64)
    inp = cc.make_inputs(q, dtype=torch.float64)
    rows = torch.cat([inp.z0.repeat_interleave(q.group, 0), inp.z1], 1)
    nq = torch.min(*[s(rows) for s in target]).view(-1, q.group)
    assert float(torch.softmax(q.beta * nq, 1).max(1)[0].min()) > 2.0 / q.group


@pytest.mark.parametrize("name", cc.TABLE)
def test_the_restatement_is_the_inline_step_in_float64(name, refs):
    """``reference_step`` in float64 against float64 autograd of the inline step to 1e-10 (relative to each quantity's largest
    magnitude): y, the loss, the mean of y, the towers' outputs and every parameter gradient."""
    from cleandiffuser_amd.engine import critic_step
    case, ref = cc.CASES[name], refs[name]
    live, target = cc.build(case, dtype=torch.float64)
    q = cc.request(critic_step, case, live, target, cc.make_inputs(case, dtype=torch.float64))
    critic_step.reference_step(q)
    loss, y_mean = critic_step.loss_of(q)
    assert cc.rel_err(q.y, ref["y"]) <= 1e-10 and cc.rel_err(loss, ref["loss"]) <= 1e-10 and cc.rel_err(y_mean, ref["y"].mean()) <= 1e-10
    for t in range(case.live_towers):
        assert cc.rel_err(q.live.out[t][:, 0], ref["q"][t]) <= 1e-10
        got = critic_step.reference_param_grads(q, t)
        assert len(got) == len(ref["grads"][t])
        for i, (a, b) in enumerate(zip(got, ref["grads"][t])):
            assert cc.rel_err(a, b) <= 1e-10, (name, t, i, cc.rel_err(a, b))


_sizes_request = cc.sizes_request


def test_the_lds_plan_is_the_librarys():
    """``lds_bytes`` against ``cdx_critic_step_lds_bytes`` over a sweep of live and target shapes; sizes the kernel does not take come back
    negative."""
    from types import SimpleNamespace
    from cleandiffuser_amd.engine import critic_step
    lib = critic_step._lib()
    seen = set()
    for k0 in (1, 14, 23, 64, 300, 512):
        for widths in ([1], [16, 1], [32, 32, 1], [256, 256, 256, 1], [512, 16, 1], [512, 512, 512, 512, 512, 1]):
            for tk0, twidths in ((k0, widths), (17, [64, 64, 1]), (512, [512, 1])):
                c = _sizes_request(critic_step, (k0, widths), (tk0, twidths))
                want = critic_step.lds_bytes(SimpleNamespace(K0=k0, width=widths), SimpleNamespace(K0=tk0, width=twidths))
                assert lib.cdx_critic_step_lds_bytes(ctypes.byref(c)) == want, (k0, widths, tk0, twidths)
                seen.add(want > critic_step.MAX_LDS)
    assert seen == {True, False}, "the sweep crosses the 160 KiB bound"
    for bad in (_sizes_request(critic_step, (14, [32, 3]), (14, [32, 1])), _sizes_request(critic_step, (14, [32, 1]), (14, [24, 1])),
                _sizes_request(critic_step, (14, [32, 1]), (14, [32, 1]), K=17), _sizes_request(critic_step, (14, [32, 1]), (14, [32, 1]), K=0)):
        assert lib.cdx_critic_step_lds_bytes(ctypes.byref(bad)) < 0


def test_the_entry_validates_before_touching_the_device():
    """``cdx_critic_step_f32``: CDX_EINVAL with a message on null pointers and on an LDS plan over the bound; R == 0 is CDX_OK."""
    from cleandiffuser_amd.engine import critic_step
    lib, einval = critic_step._lib(), -1                      # CDX_EINVAL
    c = _sizes_request(critic_step, (14, [32, 1]), (14, [32, 1]))
    assert lib.cdx_critic_step_f32(ctypes.byref(c), None) == einval and b"null pointer" in lib.cdx_last_error()
    big = _sizes_request(critic_step, (14, [512, 512, 512, 512, 512, 1]), (14, [32, 1]))
    assert lib.cdx_critic_step_f32(ctypes.byref(big), None) == einval and b"160 KiB" in lib.cdx_last_error()
    c.R = 0
    assert lib.cdx_critic_step_f32(ctypes.byref(c), None) == 0


def test_ctypes_mirrors_have_c_layout(tmp_path):
    from cleandiffuser_amd.engine import critic_step
    mirrors = {"cdx_critic_net": critic_step.CdxCriticNet, "cdx_critic_step": critic_step.CdxCriticStep}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){']
    for cname, mirror in mirrors.items():
        src.append(f'printf("%zu\\n", sizeof({cname}));')
        src += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src += ['printf("%d %d %d %d %d %d\\n", CDX_CRITIC_MIN, CDX_CRITIC_MAX, CDX_CRITIC_SOFTMAX, CDX_CRITIC_MSE, CDX_CRITIC_EXPECTILE, CDX_CRITIC_MAX_K);',
            'return 0;}']
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    for cname, mirror in mirrors.items():
        assert int(next(out)) == ctypes.sizeof(mirror), cname
        for f in mirror._fields_:
            assert getattr(mirror, f[0]).offset == int(next(out)), (cname, f[0])
    R, L = critic_step.REDUCE, critic_step.LOSS
    assert [int(v) for v in out] == [R["min"], R["max"], R["softmax"], L["mse"], L["expectile"], critic_step.MAX_K]


# ------------------------------------------------------------------------------------------------------------------- #
# Routing: the fused step with the C call replaced by its restatement, and every refusal                                      #
# ------------------------------------------------------------------------------------------------------------------- #
def _fake_device(monkeypatch):
    """The routing of ``try_step`` on the CPU: the device test says yes, the three launches are their torch restatements."""
    from cleandiffuser_amd.engine import critic_step
    calls = []
    monkeypatch.setattr(critic_step, "_on_device", lambda x, params: True)
    monkeypatch.setattr(critic_step, "native_step", lambda q: (calls.append("step"), critic_step.reference_step(q)))

    def weight_sums(jobs):
        calls.append("wgrad")
        for p, q, _, dw, db in jobs:
            dw.add_(p.t() @ q)
            db.add_(p.sum(0))

    def column_sums(jobs):
        calls.append("colsum")
        for src, out in jobs:
            out.add_(src.sum(0))
    monkeypatch.setattr(critic_step, "weight_sums", weight_sums)
    monkeypatch.setattr(critic_step, "column_sums", column_sums)
    return calls


def _nets(hidden=32):
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V, load_synth
    return (load_synth(TwinQ(11, 3, hidden_dim=hidden), 1), load_synth(V(11, hidden_dim=hidden), 2), load_synth(DQLCritic(11, 3, hidden_dim=hidden), 3))


def _batch(rows=24, group=1):
    g = torch.Generator().manual_seed(5)
    return dict(obs=torch.randn(rows, 11, generator=g), act=torch.randn(rows, 3, generator=g).tanh(), rew=torch.randn(rows, 1, generator=g),
                next_obs=torch.randn(rows, 11, generator=g), done=(torch.rand(rows, 1, generator=g) < 0.3).float(),
                next_act=torch.randn(rows * group, 3, generator=g).tanh())


@pytest.mark.parametrize("kind", ["iql_q", "iql_v", "dql", "antmaze", "qgpo"])
def test_the_fused_route_is_the_eager_step(kind, monkeypatch):
    """``td_step`` / ``expectile_step`` through ``try_step`` (the launches restated in torch) against the eager sequence from the same
    state: the loss, the mean of y, every gradient and the parameters after the optimiser step at rtol = atol = 1e-5; the route is one
    step launch, one weight-gradient launch, one column-sum launch."""
    from copy import deepcopy
    from cleandiffuser_amd.utils import critic_steps
    results = {}
    for route in ("eager", "fused"):
        monkeypatch.setenv("CDX_CRITIC_STEP", "1" if route == "fused" else "0")
        calls = _fake_device(monkeypatch)
        twin, v, dql = _nets()
        group = {"antmaze": 10, "qgpo": 16}.get(kind, 1)
        b = _batch(group=group)
        if kind == "iql_v":
            live, frozen = v, deepcopy(twin).requires_grad_(False)
        elif kind == "iql_q":
            live, frozen = twin, deepcopy(v).requires_grad_(False)
        else:
            live = dql if kind != "qgpo" else twin
            frozen = deepcopy(live).requires_grad_(False)
        optim = torch.optim.Adam(live.parameters(), lr=3e-4)
        if kind == "iql_v":
            out = critic_steps.expectile_step(live, frozen, optim, b["obs"], b["act"], tau=0.7)
        elif kind == "iql_q":
            out = critic_steps.td_step(live, frozen, optim, b["obs"], b["act"], b["rew"], b["next_obs"], b["done"], discount=0.99)
        else:
            kw = {"dql": {}, "antmaze": dict(group=10, reduce="max"), "qgpo": dict(group=16, reduce="softmax", beta=3.0)}[kind]
            out = critic_steps.td_step(live, frozen, optim, b["obs"], b["act"], b["rew"], b["next_obs"], b["done"], b["next_act"],
                                       discount=0.99, **kw)
        assert calls == (["step", "wgrad", "colsum"] if route == "fused" else []), (route, calls)
        assert out["loss"].dim() == 0 and out["target_mean"].dim() == 0
        results[route] = ([float(out["loss"]), float(out["target_mean"])], [p.grad.clone() for p in live.parameters()],
                          [p.detach().clone() for p in live.parameters()])
    (sa, ga, pa), (sb, gb, pb) = results["eager"], results["fused"]
    np.testing.assert_allclose(sb, sa, rtol=1e-5, atol=1e-5)
    for a, b_ in zip(ga + pa, gb + pb):
        np.testing.assert_allclose(b_.numpy(), a.numpy(), rtol=1e-5, atol=1e-5)


def _try(monkeypatch, mutate=None, env=None, grad=True, **kw):
    """``try_step`` of an IQL Q step on the faked device after `mutate(live, frozen, batch)` -> (answer, the launches made, the
    gradients before and after)."""
    from cleandiffuser_amd.engine import critic_step
    from cleandiffuser_amd.utils.critic_steps import _towers
    calls = _fake_device(monkeypatch)
    for k in ("CDX_CRITIC_STEP", "CDX_TRAIN_NATIVE", "CDX_TRAIN_INPLACE_GRADS"):
        monkeypatch.delenv(k, raising=False)
    for k, val in (env or {}).items():
        monkeypatch.setenv(k, val)
    twin, v, _ = _nets()
    v.requires_grad_(False)
    b = _batch()
    args = dict(live=_towers(twin), target=_towers(v), x0=b["obs"], x1=b["act"], z0=b["next_obs"], z1=None, rew=b["rew"], done=b["done"])
    for p in twin.parameters():
        p.grad = torch.full_like(p, 0.25)
    if mutate:
        mutate(twin, v, args)
    optim = torch.optim.SGD(twin.parameters(), lr=0.1)
    with torch.set_grad_enabled(grad):
        out = critic_step.try_step(args["live"], args["target"], optim, args["x0"], args["x1"], args["z0"], args["z1"], args["rew"],
                                   args["done"], discount=0.99, **kw)
    untouched = all(p.grad is not None and bool((p.grad == 0.25).all()) for p in twin.parameters())
    return out, calls, untouched


def test_every_refusal_comes_before_anything_is_written(monkeypatch):
    """The list of DESIGN.md 3p: each refusal answers None, launches nothing and leaves the gradients as they were; the plain call with
    ``CDX_CRITIC_STEP=1`` is taken."""
    from cleandiffuser_amd.engine import critic_step
    on = {"CDX_CRITIC_STEP": "1"}
    out, calls, untouched = _try(monkeypatch, env=on)
    assert out is not None and calls == ["step", "wgrad", "colsum"] and not untouched
    out, calls, untouched = _try(monkeypatch, env={})
    assert out is None and not calls and untouched, "unasked, this call site keeps the eager sequence (default=False)"
    out, calls, _ = _try(monkeypatch, env={}, default=True)
    assert out is not None and calls, "a call site that is fused by default is taken without the variable"

    def hook(twin, v, a):
        next(twin.parameters()).register_hook(lambda g: g)

    def post_hook(twin, v, a):
        next(twin.parameters()).register_post_accumulate_grad_hook(lambda p: None)

    def frozen(twin, v, a):
        twin.Q2[0].bias.requires_grad_(False)

    def gelu(twin, v, a):
        twin.Q1[2], twin.Q2[2] = nn.GELU(), nn.GELU()

    def odd_target(twin, v, a):
        v.V[2] = nn.GELU()

    def x_grad(twin, v, a):
        a["x1"] = a["x1"].clone().requires_grad_(True)

    def half(twin, v, a):
        a["x0"] = a["x0"].half()

    def double_net(twin, v, a):
        twin.double()
        for p in twin.parameters():
            p.grad = torch.full_like(p, 0.25)

    def rows(twin, v, a):
        a["z0"] = a["z0"][:-1]

    def width(twin, v, a):
        a["x1"] = a["x1"][:, :2]

    def rew_rows(twin, v, a):
        a["rew"] = a["rew"][:-1]

    def no_done(twin, v, a):
        a["done"] = None

    def three(twin, v, a):
        a["live"] = a["live"] + (twin.Q1,)

    def unequal(twin, v, a):
        from cleandiffuser_amd.utils.critics import _q_tower
        twin.Q2 = _q_tower(14, 64, nn.Mish(), 2)
        a["live"] = (twin.Q1, twin.Q2)
        for p in twin.Q2.parameters():
            p.grad = torch.full_like(p, 0.25)

    def grouped(k):
        def mutate(twin, v, a):                              # a twin target over [next_obs | k candidates]: only K differs between 16 and 17
            from copy import deepcopy
            from cleandiffuser_amd.utils.critic_steps import _towers
            a["target"] = _towers(deepcopy(twin).requires_grad_(False))
            a["z1"] = torch.randn(24 * k, 3, generator=torch.Generator().manual_seed(k)).tanh()
        return mutate

    def wide(twin, v, a):                                    # six 512-wide live layers: P_l alone is 160 KiB
        mods = []
        for i in range(5):
            mods += [nn.Linear(14 if i == 0 else 512, 512), nn.LayerNorm(512), nn.Mish()]
        a["live"] = (nn.Sequential(*mods, nn.Linear(512, 1)),)

    refusals = {"CDX_CRITIC_STEP=0": dict(env={"CDX_CRITIC_STEP": "0"}, default=True), "CDX_TRAIN_NATIVE=0": dict(env={**on, "CDX_TRAIN_NATIVE": "0"}),
                "in-place gradients off": dict(env={**on, "CDX_TRAIN_INPLACE_GRADS": "0"}), "grad mode off": dict(env=on, grad=False),
                "a hook": dict(env=on, mutate=hook), "a post-accumulate hook": dict(env=on, mutate=post_hook),
                "a frozen live parameter": dict(env=on, mutate=frozen), "GELU": dict(env=on, mutate=gelu), "a GELU target": dict(env=on, mutate=odd_target),
                "an input with a gradient": dict(env=on, mutate=x_grad), "fp16 input": dict(env=on, mutate=half), "fp64 towers": dict(env=on, mutate=double_net),
                "rows": dict(env=on, mutate=rows), "width": dict(env=on, mutate=width), "rew rows": dict(env=on, mutate=rew_rows),
                "rew without done": dict(env=on, mutate=no_done), "three towers": dict(env=on, mutate=three),
                "towers of two shapes": dict(env=on, mutate=unequal), "K > 16": dict(env=on, mutate=grouped(17), group=17, reduce="max"),
                "min with a group": dict(env=on, group=2, reduce="min"), "an LDS plan over the bound": dict(env=on, mutate=wide)}
    for what, kw in refusals.items():
        out, calls, untouched = _try(monkeypatch, **kw)
        assert out is None and not calls and untouched, what
    out, calls, _ = _try(monkeypatch, env=on, mutate=grouped(16), group=16, reduce="max")
    assert out is not None and calls == ["step", "wgrad", "colsum"], "K = 16 is taken"
    # not a ROCm device; a listening reducer
    monkeypatch.setenv("CDX_CRITIC_STEP", "1")
    out, calls, untouched = _try(monkeypatch, mutate=lambda *_: monkeypatch.setattr(critic_step, "_on_device", lambda x, p: x.is_cuda))
    assert out is None and not calls and untouched, "a CPU tensor"
    from cleandiffuser_amd.engine import train
    out, calls, untouched = _try(monkeypatch, mutate=lambda *_: monkeypatch.setattr(train, "_reducer_may_listen", lambda: True))
    assert out is None and not calls and untouched, "a listening reducer"


def test_a_missing_library_is_an_error_not_a_fallback(monkeypatch):
    """On a device the launch is the route: a library that does not load raises out of ``try_step``."""
    from cleandiffuser_amd.engine import critic_step
    monkeypatch.setenv("CDX_CRITIC_STEP", "1")
    monkeypatch.setattr(critic_step, "_on_device", lambda x, params: True)

    def missing():
        raise OSError("libcdx.so: cannot open shared object file")
    monkeypatch.setattr(critic_step, "_lib", missing)
    from cleandiffuser_amd.utils.critic_steps import _towers
    twin, v, _ = _nets()
    b = _batch()
    with pytest.raises(OSError):
        critic_step.try_step(_towers(twin), _towers(v.requires_grad_(False)), None, b["obs"], b["act"], b["next_obs"], None, b["rew"], b["done"],
                             discount=0.99)


# ------------------------------------------------------------------------------------------------------------------- #
# The eager fallback against the real reference                                                                               #
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", cs.TABLE)
def test_the_cpu_fallback_reproduces_the_reference_fixture(name):
    """Three IQL half-steps and three Diffusion-QL critic steps through ``expectile_step`` / ``td_step`` on the CPU against the real
    reference (tests/golden/critic_towers.npz) at that file's rtol = atol = 1e-4: losses, first-step gradients, parameter checksums."""
    case, gold, U = cs.CASES[name], cs.golden(name), cs.utils_of("amd")
    got = cc.run_iql_calls(U, case)
    got.update(cc.run_dql_calls(U, case))
    assert set(got) == set(gold)
    for k in gold:
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
