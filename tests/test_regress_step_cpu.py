"""CPU checks of the fused regression step (engine/regress_step.py, utils/regression_steps.py, invdynamic/mlp.py): the torch restatement
of the launch against float64 autograd, the LDS plan against the library's, the admission at every boundary, the ctypes mirrors against
the header, the routing with the C call replaced by its restatement, every refusal, the strided-view bookkeeping, the eager fallback
against the fixture of the real reference."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regress_step_cases as rc  # noqa: E402

ENV = ("CDX_REGRESS_STEP", "CDX_TRAIN_NATIVE", "CDX_TRAIN_INPLACE_GRADS", "CDX_TOWER")


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def refs():
    """The float64 autograd reference of every case: computed once, read only."""
    return {name: rc.autograd_reference(rc.CASES[name]) for name in rc.TABLE}


def test_the_case_table_covers_what_it_claims(refs):
    """On the reference alone: no gradient is identically zero, the losses differ between cases, and the table has the shapes the
    kernel's paths depend on."""
    losses = [float(refs[n]["loss"]) for n in rc.TABLE]
    assert len({round(v, 9) for v in losses}) == len(losses), losses
    for name in rc.TABLE:
        for i, g in enumerate(refs[name]["grads"]):
            assert float(g.abs().max()) > 0, (name, i)
    C = list(rc.CASES.values())
    assert {c.rows for c in C} >= {1, 16, 17, 33, 21, 5} and {c.a0 + c.a1 for c in C} >= {2, 22, 512}
    assert any(c.a1 == 0 for c in C) and {c.widths[-1] for c in C} >= {1, 3, 64} and {c.widths[0] for c in C} >= {16, 32, 512}
    assert any(len(c.widths) == 1 for c in C) and any(c.fancy for c in C) and {c.acts[-1] for c in C} == {None, "tanh", "relu", "silu", "mish"}
    assert {c.view for c in C} == {None, "dd", "dv"}


@pytest.mark.parametrize("name", rc.TABLE)
def test_the_restatement_is_the_autograd_step_in_float64(name, refs):
    """``reference_step`` in float64 against float64 autograd on the same modules and ``torch.cat`` inputs to 1e-10 (relative to each
    quantity's largest magnitude): the loss, the output and every parameter gradient."""
    from cleandiffuser_amd.engine import regress_step
    case, ref = rc.CASES[name], refs[name]
    q = rc.request(regress_step, case, rc.build(case, dtype=torch.float64), rc.make_inputs(case, dtype=torch.float64))
    regress_step.reference_step(q)
    assert rc.rel_err(regress_step.loss_of(q), ref["loss"]) <= 1e-10 and rc.rel_err(q.live.out[0], ref["out"]) <= 1e-10
    got = regress_step.reference_param_grads(q)
    assert len(got) == len(ref["grads"])
    for i, (a, b) in enumerate(zip(got, ref["grads"])):
        assert rc.rel_err(a, b) <= 1e-10, (name, i, rc.rel_err(a, b))


def _c_plan(k0, widths) -> int:
    """regress_plan of csrc/cdx_regress_step.hip, restated: two images [16][ld], P_l, rstd_l, the 16 x 64 tile, in bytes."""
    r16 = lambda v: (v + 15) // 16 * 16          # noqa: E731
    ld = max(r16(w) for w in [k0] + widths) + 4
    at_p = 2 * 16 * ld
    at_rstd = at_p + 16 * sum(widths)
    at_tile = at_rstd + 16 * len(widths)
    return 4 * (at_tile + 16 * 64)


def test_the_lds_plan_is_the_librarys():
    """``lds_bytes`` against the restated C plan and against ``cdx_regress_step_lds_bytes`` over a sweep of shapes that crosses the
    160 KiB bound; the shipped head at its widest is 136.7 KiB; sizes the kernel does not take come back negative."""
    from cleandiffuser_amd.engine import regress_step
    lib = regress_step._lib()
    seen = set()
    for k0 in (1, 2, 22, 64, 300, 512):
        for widths in ([1], [3], [16, 3], [32, 32, 64], [512, 512, 9], [512, 512, 64], [512, 512, 512, 64], [512, 512, 512, 512, 512, 1]):
            want = regress_step.lds_bytes(SimpleNamespace(K0=k0, width=widths))
            assert want == _c_plan(k0, widths), (k0, widths)
            assert lib.cdx_regress_step_lds_bytes(ctypes.byref(rc.sizes_request(regress_step, k0, widths))) == want, (k0, widths)
            seen.add(want > regress_step.MAX_LDS)
    assert seen == {True, False}, "the sweep crosses the 160 KiB bound"
    assert regress_step.lds_bytes(SimpleNamespace(K0=512, width=[512, 512, 64])) == 139968 <= regress_step.MAX_LDS == 160 * 1024
    bad = [rc.sizes_request(regress_step, 22, [32, 65]), rc.sizes_request(regress_step, 513, [32, 3]), rc.sizes_request(regress_step, 22, [24, 3]),
           rc.sizes_request(regress_step, 22, [32, 3], a0=0), rc.sizes_request(regress_step, 22, [32, 3], rows=-1)]
    two = rc.sizes_request(regress_step, 22, [32, 3])
    two.net.n_towers = 2
    wrong_y = rc.sizes_request(regress_step, 22, [32, 3])
    wrong_y.y.width = 4
    inner0 = rc.sizes_request(regress_step, 22, [32, 3])
    inner0.x0.inner = 0
    short = rc.sizes_request(regress_step, 22, [32, 3])
    short.y.inner, short.y.period = 3, 2
    for c in bad + [two, wrong_y, inner0, short]:
        assert lib.cdx_regress_step_lds_bytes(ctypes.byref(c)) < 0 and lib.cdx_last_error()
    for ok in (rc.sizes_request(regress_step, 22, [32, 64]), rc.sizes_request(regress_step, 512, [32, 3]),
               rc.sizes_request(regress_step, 22, [32, 3], rows=0x7fffffff - 16)):
        assert lib.cdx_regress_step_lds_bytes(ctypes.byref(ok)) > 0
    assert lib.cdx_regress_step_lds_bytes(ctypes.byref(rc.sizes_request(regress_step, 22, [32, 3], rows=0x7fffffff - 15))) < 0


def test_the_entry_validates_before_touching_the_device():
    """``cdx_regress_step_f32``: CDX_EINVAL with a message on null pointers and on an LDS plan over the bound; R == 0 is CDX_OK."""
    from cleandiffuser_amd.engine import regress_step
    lib, einval = regress_step._lib(), -1                     # CDX_EINVAL
    c = rc.sizes_request(regress_step, 22, [32, 3])
    assert lib.cdx_regress_step_f32(ctypes.byref(c), None) == einval and b"null pointer" in lib.cdx_last_error()
    assert lib.cdx_regress_step_f32(None, None) == einval and b"null request" in lib.cdx_last_error()
    big = rc.sizes_request(regress_step, 22, [512, 512, 512, 512, 512, 1])
    assert lib.cdx_regress_step_f32(ctypes.byref(big), None) == einval and b"160 KiB" in lib.cdx_last_error()
    c.R = 0
    assert lib.cdx_regress_step_f32(ctypes.byref(c), None) == 0


def _mlp(k0, widths, acts=None, extra=()):
    mods, k = [], k0
    for i, w in enumerate(widths):
        mods += [nn.Linear(k, w)] + ([acts[i]()] if acts and acts[i] else [])
        k = w
    return nn.Sequential(*mods, *extra)


def test_the_admission_at_every_boundary():
    """``describe`` and ``shapes_ok``: last widths 64 / 65, K0 512 / 513, hidden widths off a multiple of 16, GELU, an active and an
    inactive dropout."""
    from cleandiffuser_amd.engine import regress_step
    assert regress_step.describe(_mlp(22, [32, 64])) is not None and regress_step.describe(_mlp(22, [32, 65])) is None
    assert regress_step.describe(_mlp(512, [32, 3])) is not None and regress_step.describe(_mlp(513, [32, 3])) is None
    assert regress_step.describe(_mlp(22, [24, 3])) is None and regress_step.describe(_mlp(22, [32, 1])) is not None
    assert regress_step.describe(_mlp(22, [32, 3], [nn.GELU, nn.Tanh])) is None
    drop = nn.Sequential(nn.Linear(22, 32), nn.ReLU(), nn.Dropout(0.1), nn.Linear(32, 3))
    assert regress_step.describe(drop) is None, "an active dropout"
    assert regress_step.describe(drop.eval()) is not None and regress_step.describe(drop.train()) is None
    drop[2].p = 0.0
    assert regress_step.describe(drop) is not None, "p == 0"
    assert regress_step.describe(nn.Linear(22, 3)) is None, "not a Sequential"
    # shapes_ok: the operands against the tower
    net = _mlp(22, [32, 3])
    d = regress_step.describe(net)
    from cleandiffuser_amd.engine import tower
    ws = [p.detach() for p in tower.params_of(d)]
    x0, x1, y = torch.randn(5, 11), torch.randn(5, 11), torch.randn(5, 3)
    assert regress_step.shapes_ok(regress_step.make_request(d, ws, x0, x1, y))
    assert not regress_step.shapes_ok(regress_step.make_request(d, ws, x0, x1[:, :10], y)), "A0 + A1 != K0"
    assert not regress_step.shapes_ok(regress_step.make_request(d, ws, x0, x1, y[:, :2])), "the target's width"
    assert not regress_step.shapes_ok(regress_step.make_request(d, ws, x0, x1[:4], y)), "rows of x1"
    assert not regress_step.shapes_ok(regress_step.make_request(d, ws, x0, x1, y[:4])), "rows of y"
    wide = _mlp(22, [512, 512, 512, 512, 512, 1])
    dw = regress_step.describe(wide)
    assert dw is not None and not regress_step.shapes_ok(
        regress_step.make_request(dw, [p.detach() for p in tower.params_of(dw)], x0, x1, y[:, :1])), "an LDS plan over the bound"


def test_ctypes_mirrors_have_c_layout(tmp_path):
    from cleandiffuser_amd.engine import regress_step
    mirrors = {"cdx_regress_rows": regress_step.CdxRegressRows, "cdx_regress_step": regress_step.CdxRegressStep}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){']
    for cname, mirror in mirrors.items():
        src.append(f'printf("%zu\\n", sizeof({cname}));')
        src += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src += ['return 0;}']
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    for cname, mirror in mirrors.items():
        assert int(next(out)) == ctypes.sizeof(mirror), cname
        for f in mirror._fields_:
            assert getattr(mirror, f[0]).offset == int(next(out)), (cname, f[0])
    assert regress_step.TILE_LD == 64 and list(out) == []


# ------------------------------------------------------------------------------------------------------------------- #
# The strided views                                                                                                           #
# ------------------------------------------------------------------------------------------------------------------- #
def _gather(t, m):
    """The rows of `t` through the kernel's row map, from the flat storage behind ``t``'s first element."""
    inner, period, ld = m
    width, rows = t.shape[-1], t.numel() // t.shape[-1]
    flat = t.as_strided((t.untyped_storage().size() // t.element_size() - t.storage_offset(),), (1,))
    r = torch.arange(rows)
    at = ((r // inner) * period + r % inner) * ld
    return flat[at[:, None] + torch.arange(width)[None, :]]


def test_the_row_map_of_the_pipelines_views():
    """(inner, period, ld) of ``obs[:, :-1]`` / ``obs[:, 1:]`` (Decision Diffuser) and ``obs[:, 0]`` / ``obs[:, 1]`` (Decision Veteran)
    of a (B, H, D) batch, read in place; a view that fits neither is copied; the map gathers exactly the view's rows."""
    from cleandiffuser_amd.engine import regress_step
    obs = torch.randn(7, 4, 11)
    for view, want in ((obs[:, :-1], (3, 4, 11)), (obs[:, 1:], (3, 4, 11)), (obs[:, 0], (1, 1, 44)), (obs[:, 1, :], (1, 1, 44)),
                       (obs.view(28, 11), (1, 1, 11)), (obs, (4, 4, 11)), (obs[:, :, :5], (4, 4, 11)), (obs[:1, 1:], (3, 3, 11)),
                       (obs[:, ::2], (2, 2, 22)), (obs.view(28, 11)[:, 3:4], (1, 1, 11))):
        t, m = regress_step._operand(view)
        assert m == want and t.data_ptr() == view.data_ptr(), (view.shape, view.stride(), m)
        assert torch.equal(_gather(t, m), view.reshape(-1, view.shape[-1]))
    odd = torch.randn(350).as_strided((7, 3, 11), (50, 11, 1))           # an outer stride that is no whole multiple of the row stride
    for view in (obs.transpose(0, 1), obs[:, :, ::2], obs[:, 0:1].expand(7, 3, 11), torch.randn(11).expand(6, 11), odd,
                 obs.view(28, 11).t()):
        assert regress_step.row_map(view) is None, (view.shape, view.stride())
        t, m = regress_step._operand(view)
        assert t.is_contiguous() and t.data_ptr() != view.data_ptr() and torch.equal(_gather(t, m), view.reshape(-1, view.shape[-1]))
    # the request of the two pipeline slicings holds the views themselves
    for name in ("dd_view_7x4x11", "dv_view_5x3x11"):
        case = rc.CASES[name]
        inp = rc.make_inputs(case)
        q = rc.request(regress_step, case, rc.build(case), inp)
        assert q.x0.data_ptr() == inp.x0.data_ptr() and q.x1.data_ptr() == inp.x1.data_ptr() == inp.x0.data_ptr() + 4 * 11
        assert q.y.data_ptr() == inp.y.data_ptr()
        assert (q.map0, q.map1, q.map_y) == (((3, 4, 11),) * 2 + ((3, 4, 3),) if case.view == "dd" else ((1, 1, 33),) * 2 + ((1, 1, 9),))


# ------------------------------------------------------------------------------------------------------------------- #
# Routing: the fused step with the C call replaced by its restatement, and every refusal                                      #
# ------------------------------------------------------------------------------------------------------------------- #
def _fake_device(monkeypatch, capturing=False, on_device=None):
    """The routing of ``try_step`` on the CPU: the device test says yes (or is `on_device`), the three launches are their torch
    restatements."""
    from cleandiffuser_amd.engine import regress_step
    calls = []
    monkeypatch.setattr(regress_step, "_on_device", on_device or (lambda x, params: True))
    monkeypatch.setattr(regress_step, "_capturing", lambda x: capturing)
    monkeypatch.setattr(regress_step, "native_step", lambda q: (calls.append("step"), regress_step.reference_step(q)))

    def weight_sums(jobs):
        calls.append("wgrad")
        for p, q, _, dw, db in jobs:
            dw.add_(p.t() @ q)
            db.add_(p.sum(0))

    def column_sums(jobs):
        calls.append("colsum")
        for src, out in jobs:
            out.add_(src.sum(0))
    monkeypatch.setattr(regress_step, "weight_sums", weight_sums)
    monkeypatch.setattr(regress_step, "column_sums", column_sums)
    return calls


def _batch(kind, seed=5):
    g = torch.Generator().manual_seed(seed)
    obs, act = torch.randn(6, 4, 11, generator=g), torch.randn(6, 4, 3, generator=g).tanh()
    if kind == "dd":
        return obs[:, :-1], act[:, :-1], obs[:, 1:]
    if kind == "dv":
        return obs[:, 0], act[:, 0], obs[:, 1]
    return obs.reshape(24, 11), act.reshape(24, 3), obs.flip(0).reshape(24, 11)


def _params(module):
    return [p.detach().clone() for p in module.parameters()]


@pytest.mark.parametrize("kind", ["dd", "dv", "plain"])
def test_update_on_the_fused_route_is_the_parent_body(kind, monkeypatch):
    """``MlpInvDynamic.update`` through ``try_step`` (the launches restated in torch) against the parent body (``CDX_REGRESS_STEP=0``)
    over three steps from the same weights: every loss and the parameters after each step at rtol = atol = 1e-5; the route is one step
    launch, one weight-gradient launch, one column-sum launch per step."""
    from cleandiffuser_amd.invdynamic import MlpInvDynamic
    results = {}
    for route in ("0", "1"):
        monkeypatch.setenv("CDX_REGRESS_STEP", route)
        calls = _fake_device(monkeypatch)
        torch.manual_seed(3)
        head = MlpInvDynamic(11, 3, hidden_dim=32, optim_params={"lr": 1e-3})
        trace = []
        for i in range(3):
            o, a, o_next = _batch(kind, seed=5 + i)
            out = head.update(o, a, o_next)
            assert isinstance(out["loss"], float)
            trace.append(([out["loss"]], _params(head.mlp)))
        assert calls == (["step", "wgrad", "colsum"] * 3 if route == "1" else []), (route, calls)
        results[route] = trace
    for (la, pa), (lb, pb) in zip(results["0"], results["1"]):
        np.testing.assert_allclose(lb, la, rtol=1e-5, atol=1e-5)
        for a, b in zip(pa, pb):
            np.testing.assert_allclose(b.numpy(), a.numpy(), rtol=1e-5, atol=1e-5)


def test_update_idx_steps_one_member_and_skips_the_others(monkeypatch):
    """``EnsembleMlpInvDynamic.update_idx`` (standard members) on the fused route against the parent body over the members 0, 1, 0:
    losses and the parameters of EVERY member (the optimiser holds them all; the members not stepped must not move) at 1e-5."""
    from cleandiffuser_amd.invdynamic.mlp import EnsembleMlpInvDynamic
    results = {}
    for route in ("0", "1"):
        monkeypatch.setenv("CDX_REGRESS_STEP", route)
        calls = _fake_device(monkeypatch)
        torch.manual_seed(4)
        head = EnsembleMlpInvDynamic(11, 3, hidden_dim=32, n_models=2, optim_params={"lr": 1e-3})
        losses = [head.update_idx(idx, *_batch("dd", seed=7 + i)) for i, idx in enumerate((0, 1, 0))]
        assert all(isinstance(v, float) for v in losses) and len(calls) == (9 if route == "1" else 0)
        results[route] = (losses, _params(head.mlp))
    np.testing.assert_allclose(results["1"][0], results["0"][0], rtol=1e-5, atol=1e-5)
    for a, b in zip(results["0"][1], results["1"][1]):
        np.testing.assert_allclose(b.numpy(), a.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("net_kind", ["sequential", "mlp"])
def test_mse_step_on_the_fused_route_is_the_eager_sequence(net_kind, monkeypatch):
    """``mse_step`` (SfBC's critic loop: a scalar regression on the rows x alone, and on [x | x1]) over three steps on both routes."""
    from cleandiffuser_amd.utils import Mlp
    from cleandiffuser_amd.utils.regression_steps import mse_step
    results = {}
    for route in ("0", "1"):
        monkeypatch.setenv("CDX_REGRESS_STEP", route)
        calls = _fake_device(monkeypatch)
        torch.manual_seed(6)
        net = Mlp(11, [32, 32], 1, nn.Mish()) if net_kind == "mlp" else nn.Sequential(nn.Linear(22, 32), nn.LayerNorm(32), nn.SiLU(), nn.Linear(32, 3))
        optim = torch.optim.Adam(net.parameters(), lr=1e-3)
        trace = []
        for i in range(3):
            o, a, o_next = _batch("plain", seed=9 + i)
            out = mse_step(net, optim, o, a[:, :1]) if net_kind == "mlp" else mse_step(net, optim, o, a, x1=o_next)
            assert torch.is_tensor(out["loss"]) and out["loss"].dim() == 0 and not out["loss"].requires_grad
            trace.append(([float(out["loss"])], _params(net)))
        assert calls == (["step", "wgrad", "colsum"] * 3 if route == "1" else []), (route, calls)
        results[route] = trace
    for (la, pa), (lb, pb) in zip(results["0"], results["1"]):
        np.testing.assert_allclose(lb, la, rtol=1e-5, atol=1e-5)
        for a, b in zip(pa, pb):
            np.testing.assert_allclose(b.numpy(), a.numpy(), rtol=1e-5, atol=1e-5)
    with pytest.raises(TypeError):
        mse_step(nn.Linear(3, 3), None, torch.randn(2, 3), torch.randn(2, 3))


def _try(monkeypatch, mutate=None, env=None, grad=True, capturing=False, on_device=None, **kw):
    """``try_step`` of an inverse-dynamics step on the faked device after `mutate(args)` -> (answer, the launches made, whether the
    gradients are as they were)."""
    from cleandiffuser_amd.engine import regress_step
    calls = _fake_device(monkeypatch, capturing, on_device)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, val in (env or {}).items():
        monkeypatch.setenv(k, val)
    torch.manual_seed(1)
    net = _mlp(22, [32, 32, 3], [nn.ReLU, nn.ReLU, nn.Tanh])
    o, a, o_next = _batch("dd")
    args = dict(net=net, x0=o, x1=o_next, y=a)
    for p in net.parameters():
        p.grad = torch.full_like(p, 0.25)
    if mutate:
        mutate(args)
    optim = torch.optim.SGD(net.parameters(), lr=0.1)
    with torch.set_grad_enabled(grad):
        out = regress_step.try_step(args["net"], optim, args["x0"], args["x1"], args["y"], **kw)
    untouched = all(p.grad is not None and bool((p.grad == 0.25).all()) for p in net.parameters())
    return out, calls, untouched


def test_every_refusal_comes_before_anything_is_written(monkeypatch):
    """The list of DESIGN.md 3r: each refusal answers None, launches nothing and leaves the gradients as they were; the plain call with
    ``CDX_REGRESS_STEP=1`` is taken."""
    from cleandiffuser_amd.engine import train
    on = {"CDX_REGRESS_STEP": "1"}
    out, calls, untouched = _try(monkeypatch, env=on)
    assert out is not None and out["loss"].dim() == 0 and calls == ["step", "wgrad", "colsum"] and not untouched
    out, calls, untouched = _try(monkeypatch, env={})
    assert out is None and not calls and untouched, "unasked, a call site that is not fused by default keeps the eager sequence"
    out, calls, _ = _try(monkeypatch, env={}, default=True)
    assert out is not None and calls, "a call site that is fused by default is taken without the variable"

    def setter(key, fn):
        def mutate(a):
            a[key] = fn(a[key])
        return mutate

    def hook(a):
        next(a["net"].parameters()).register_hook(lambda g: g)

    def post_hook(a):
        next(a["net"].parameters()).register_post_accumulate_grad_hook(lambda p: None)

    def frozen(a):
        a["net"][0].bias.requires_grad_(False)

    def gelu(a):
        a["net"][1] = nn.GELU()

    def dropout(a):
        a["net"].insert(2, nn.Dropout(0.1))

    def width24(a):
        a["net"][0], a["net"][2] = nn.Linear(22, 24), nn.Linear(24, 32)
        for p in a["net"].parameters():
            p.grad = torch.full_like(p, 0.25)

    def double_net(a):
        a["net"].double()
        for p in a["net"].parameters():
            p.grad = torch.full_like(p, 0.25)

    def noncontiguous(a):
        lin = a["net"][2]
        lin.weight.data = lin.weight.data.t().contiguous().t()

    def empty(a):
        a["x0"], a["x1"], a["y"] = a["x0"][:0], a["x1"][:0], a["y"][:0]

    refusals = {"CDX_REGRESS_STEP=0": dict(env={"CDX_REGRESS_STEP": "0"}, default=True), "CDX_TRAIN_NATIVE=0": dict(env={**on, "CDX_TRAIN_NATIVE": "0"}),
                "in-place gradients off": dict(env={**on, "CDX_TRAIN_INPLACE_GRADS": "0"}), "grad mode off": dict(env=on, grad=False),
                "a capturing stream": dict(env=on, capturing=True),
                "a hook": dict(env=on, mutate=hook), "a post-accumulate hook": dict(env=on, mutate=post_hook),
                "a frozen parameter": dict(env=on, mutate=frozen), "GELU": dict(env=on, mutate=gelu), "an active dropout": dict(env=on, mutate=dropout),
                "a width off a multiple of 16": dict(env=on, mutate=width24),
                "an input with a gradient": dict(env=on, mutate=setter("x1", lambda t: t.clone().requires_grad_(True))),
                "a target with a gradient": dict(env=on, mutate=setter("y", lambda t: t.clone().requires_grad_(True))),
                "fp16 input": dict(env=on, mutate=setter("x0", lambda t: t.half())), "fp64 target": dict(env=on, mutate=setter("y", lambda t: t.double())),
                "an fp64 net": dict(env=on, mutate=double_net), "parameters that are not contiguous": dict(env=on, mutate=noncontiguous, on_device=lambda x, ps: all(p.is_contiguous() for p in ps)),
                "rows": dict(env=on, mutate=setter("y", lambda t: t[:-1])), "width": dict(env=on, mutate=setter("x1", lambda t: t[..., :10])),
                "the target's width": dict(env=on, mutate=setter("y", lambda t: t[..., :2])), "R == 0": dict(env=on, mutate=empty),
                "a 1-D input": dict(env=on, mutate=setter("x0", lambda t: t.reshape(-1))), "no target": dict(env=on, mutate=setter("y", lambda t: None))}
    for what, kw in refusals.items():
        out, calls, untouched = _try(monkeypatch, **kw)
        assert out is None and not calls and untouched, what
    # not a ROCm device; a listening reducer
    out, calls, untouched = _try(monkeypatch, env=on, on_device=lambda x, ps: x.is_cuda)
    assert out is None and not calls and untouched, "a CPU tensor"
    monkeypatch.setattr(train, "_reducer_may_listen", lambda: True)
    out, calls, untouched = _try(monkeypatch, env=on)
    assert out is None and not calls and untouched, "a listening reducer"


def test_the_gelu_heads_keep_the_nodes(monkeypatch):
    """``FancyMlpInvDynamic`` and ``ResInvDynamic`` are refused (GELU; a ModuleDict): their ``update`` never reaches the launch."""
    from cleandiffuser_amd.invdynamic.mlp import FancyMlpInvDynamic, ResInvDynamic
    monkeypatch.setenv("CDX_REGRESS_STEP", "1")
    calls = _fake_device(monkeypatch)
    for head in (FancyMlpInvDynamic(11, 3, hidden_dim=32), ResInvDynamic(11, 3, hidden_dim=32)):
        o, a, o_next = _batch("plain")
        assert isinstance(head.update(o, a, o_next)["loss"], float)
    assert not calls


def test_a_missing_library_is_an_error_not_a_fallback(monkeypatch):
    """On a device the launch is the route: a library that does not load raises out of ``try_step``."""
    from cleandiffuser_amd.engine import regress_step
    monkeypatch.setenv("CDX_REGRESS_STEP", "1")
    monkeypatch.setattr(regress_step, "_on_device", lambda x, params: True)

    def missing():
        raise OSError("libcdx.so: cannot open shared object file")
    monkeypatch.setattr(regress_step, "_lib", missing)
    o, a, o_next = _batch("plain")
    with pytest.raises(OSError):
        regress_step.try_step(_mlp(22, [32, 3], [nn.ReLU, nn.Tanh]), None, o, o_next, a)


def test_the_default_follows_the_measurement(monkeypatch):
    """``FUSED_BY_DEFAULT``: ``MlpInvDynamic.update`` takes the launch unasked up to the largest measured row count,
    1984; ``update_idx`` and ``mse_step`` only with ``CDX_REGRESS_STEP=1``."""
    from cleandiffuser_amd.invdynamic import MlpInvDynamic
    from cleandiffuser_amd.utils import regression_steps as rs
    assert rs.fused_by_default("invdyn", 128) and rs.fused_by_default("invdyn", 1984) and not rs.fused_by_default("invdyn", 1985)
    assert not rs.fused_by_default("invdyn_ensemble", 16) and not rs.fused_by_default("mse_step", 16)
    calls = _fake_device(monkeypatch)
    head = MlpInvDynamic(11, 3, hidden_dim=32)
    head.update(*_batch("dd"))
    assert calls == ["step", "wgrad", "colsum"]
    g = torch.Generator().manual_seed(1)
    head.update(torch.randn(1985, 11, generator=g), torch.randn(1985, 3, generator=g), torch.randn(1985, 11, generator=g))
    assert calls == ["step", "wgrad", "colsum"], "past the measured row count the parent body runs"
    net = nn.Sequential(nn.Linear(11, 16), nn.ReLU(), nn.Linear(16, 3))
    rs.mse_step(net, torch.optim.Adam(net.parameters()), *_batch("plain")[:2])
    assert calls == ["step", "wgrad", "colsum"], "mse_step is opt-in"


def test_the_namespace_of_utils_is_unchanged():
    import cleandiffuser_amd.utils as U
    assert not hasattr(U, "mse_step")


# ------------------------------------------------------------------------------------------------------------------- #
# The eager fallback against the real reference                                                                               #
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(rc.GOLDEN_CASES))
def test_the_cpu_fallback_reproduces_the_reference_fixture(name):
    """Three ``MlpInvDynamic.update`` steps on the CPU against the real reference (tests/golden/invdyn_steps.npz) at rtol = atol =
    1e-4: losses, first-step gradients, parameter checksums."""
    gold = rc.golden(name)
    got = rc.run_invdyn(rc.invdyn_of("amd"), rc.GOLDEN_CASES[name])
    assert set(got) == set(gold) and len(gold) == 8
    for k in gold:
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
