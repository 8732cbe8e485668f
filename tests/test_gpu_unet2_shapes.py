"""The denoiser forward of the program kernel (csrc/cdx_unet2.hip) against float64, over the rows of tests/unet2_shape_cases.py in every
program form each exists in: slots narrower than their 16-row tile (8 and 24 channels), model_dim 8 .. 64, a 3 and a 4 in dim_mult, one
and four levels, both kernel sizes, H 4 .. 64, D 1 .. 40, a part-empty last workgroup and a ragged last group (batch 7), the per-sample
condition, ChiUNet1d's FiLM with and without scale, the classifier-free pair; ordinary (4 / 8 waves, one / two trajectories per
workgroup), compact (one to three), split (2 / 4 workgroups per trajectory) and grouped (2 / 4) programs.  A wrong row period, partition
count or cut offset in the op interpreter gives plausible numbers, not a fault; the float64 run alone tells them apart
(tests/test_unet2_shape_cases_cpu.py), and every program ran on the NaN-poisoned CPU twin there before it came here.

Every (row, form) pair goes through the public route -- ``net(x, t, cond)`` or ``agent.sample`` -- with the form selected by the hooks
``runtime2`` reads (``unet2_shape_cases.ENV``), and is checked for

* route: exactly one ``cdx_unet2_run`` request (``runtime2.launch``, spied) of the form's program -- wave count, compact, trajectories
  per workgroup, split / group factor -- and no GEMM-executor request.  A split or grouped form also made its gated repair launch and
  nothing else, ``check_split_errors`` reports nothing and the mode's first-use flag is still on: otherwise the repair launch or the
  first-use fallback would have handed out the ordinary program's result.  (The mode's first use on the device runs its self-check on an
  unspied call first; where the device is no whole MI355X the form is skipped with the reason, and a mode that is off on a whole one
  fails the test.)  A
  refusal makes no program request and exactly one GEMM-executor request (none where the table says the stock module serves it);
* value: against the float64 CPU run (one per row and process) within 4 x YARDSTICK[family], relative to max(1, max |x64|), as rtol and
  as atol; the factor 4 is the margin of tests/test_gpu_solver_step.py for the device's summation order and FMA contraction.  Nothing
  here is derived from a device result;
* workspace: a launch that uses the per-stream workspace (compact programs, the pair) finds in ``runtime2._ws`` a view of a larger
  buffer, exactly the (batch + 1) * ws_floats it asks for, pre-filled with 1e30 -- finite, so a masked lane times an exact zero stays
  zero, but a stale read is a huge error -- and followed by 256 sentinel floats, untouched afterwards;
* determinism: a second identical call gives the same bits, and so does a third after a row of another shape ran in between (the
  narrow-slot argument of DESIGN.md 5 rests on what LDS holds at launch).

And: the number of trajectories per workgroup never changes a bit (the t1 / t2 / t3 forms of one program).

Measured on an MI355X, largest device error per family against its tolerance: Janner forward 3.07e-6 of 4e-6 (w64_m4 nw8_t1), Janner
sample 6.67e-6 of 2.2e-5 (n8_l4_s, nw8 and compact), conditional pair 3.03e-6 of 1.4e-5, ChiUNet forward 2.55e-6 of 4e-6 (chi_to1),
ChiUNet sample 6.08e-6 of 1.6e-5; split forms at most 6.21e-6, grouped 5.22e-6; the GEMM executor on refuse_gn48 1.13e-6.  The 118 tests
take 10 s.  `pytest -s` prints every pair's error."""
from types import SimpleNamespace

import pytest
import torch

import unet2_shape_cases as U
from test_gpu_solver_step import _spy_loops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON, SENTINEL, N_SENTINELS = 1e30, -12345.0, 256
_built = {}


def _get(name):
    """The net or agent of a row on the device: built once per process (its compiled programs stay in ``runtime2``'s cache)."""
    if name not in _built:
        _built[name] = U.device_build(name, DEV)
    return _built[name]


def _select(monkeypatch, form):
    for hook in U.HOOKS:
        monkeypatch.delenv(hook, raising=False)
    for hook, value in U.ENV[form].items():
        monkeypatch.setenv(hook, value)


def _spy_launches(monkeypatch):
    """Every ``runtime2.launch`` as a record of what decides the kernel it runs; the workspace it will use is seated first, poisoned and
    followed by sentinels.  -> (records, [(buffer, floats)])."""
    from cleandiffuser_amd.engine import runtime as R, runtime2
    seen, guards, orig = [], [], runtime2.launch

    def spy(comp, **kw):
        prog, parts = comp.prog, kw.get("parts")
        seen.append(SimpleNamespace(nw=prog.nw, compact=bool(prog.compact), t=parts[0][2] if parts else kw.get("t_per_wg"),
                                    n_parts=len(parts) if parts else 1, split=int(kw.get("split") or 0), group=bool(kw.get("group")),
                                    split_k=prog.meta.get("split_k", 0), group_k=prog.meta.get("group_k", 0),
                                    repair=kw.get("run_if") is not None, n_steps=kw.get("n_steps", 0),
                                    per_traj=bool(kw.get("emb_per_traj")), n_pass=2 if kw.get("emb_u") is not None else 1))
        need = prog.ws_floats                      # (runtime2.launch: the pair keeps [multistep memory | x_old | conditional prediction])
        if kw.get("emb_u") is not None:
            need = max(need, 3 * ((prog.horizon * prog.dim + 3) // 4 * 4))
        key = (kw["x_in"].device, R._stream_ptr(kw["x_in"].device))
        if need:
            floats = (kw["batch"] + 1) * need
            buf = torch.full((floats + N_SENTINELS,), POISON, dtype=torch.float32, device=kw["x_in"].device)
            buf[floats:] = SENTINEL
            monkeypatch.setitem(runtime2._ws, key, buf[:floats])
            guards.append((buf, floats))
        out = orig(comp, **kw)
        if need:
            assert runtime2._ws[key].data_ptr() == buf.data_ptr(), "the launch asked for more than (batch + 1) * ws_floats"
        return out
    monkeypatch.setattr(runtime2, "launch", spy)
    return seen, guards


def _mode_ready(name, form):
    """Split / grouped forms: the mode's flag after its first use on this device; skips where the mode cannot run here."""
    from cleandiffuser_amd.engine import runtime2
    dev = torch.device(DEV)
    if not runtime2.whole_chip(dev):
        pytest.skip("split / grouped programs need a whole MI355X (256 CUs behind 8 XCDs): runtime2.whole_chip is false here")
    ok = runtime2._MODE_FLAGS[form.startswith("group"), False]
    if dev not in ok:                              # first use: _launch_members checks the mode against the ordinary program, once
        U.device_run(name, DEV, _get(name))
        torch.cuda.synchronize()
    # (not a skip: on a whole MI355X a mode that is off has failed its first-use check against the ordinary program, or lost a granule,
    #  and every later request would silently take the ordinary program)
    assert ok.get(dev) is True, f"the {'grouped' if form.startswith('group') else 'small-batch'} mode is off on a whole MI355X: " \
                                f"{runtime2.last_exchange_error.get(dev, 'its first-use check against the ordinary program failed')}"
    return ok


def _run(name, form, monkeypatch):
    """One spied call of a row in a form -> x; route, workspace and error word checked."""
    from cleandiffuser_amd.engine import runtime2
    c = U.CASES[name]
    with monkeypatch.context() as m:
        seen, guards = _spy_launches(m)
        loops = _spy_loops(m)
        x = U.device_run(name, DEV, _get(name))
        torch.cuda.synchronize()
    for buf, floats in guards:
        assert bool((buf[floats:] == SENTINEL).all()), "the kernel wrote past the workspace it asked for"
    if c.refused is not None:
        assert seen == [], "the program kernel served a request its compiler refuses"
        assert [(k, n) for k, n, _ in loops] == ([("chiunet", 0)] if c.gemm else []), f"GEMM-executor requests of a refusal: {loops}"
        return x
    assert loops == [], "the GEMM executor served the request"
    first = [r for r in seen if not r.repair]
    assert len(first) == 1, f"exactly one cdx_unet2_run request must serve the case, got {[vars(r) for r in seen]}"
    r, key = first[0], U.program_key(form)
    assert (r.n_steps, r.n_pass) == ((2, 2 if c.cond_shape is not None else 1) if c.mode == "sample" else (0, 1))
    assert r.per_traj == (c.mode == "forward" or c.cond_shape is not None) and r.n_parts == 1
    if key[:5] in ("split", "group"):
        k = int(key[5:])
        assert (r.split, r.group, r.split_k, r.group_k, r.nw, r.compact, r.t) == \
            (k, key[:5] == "group", k if key[:5] == "split" else 0, k if key[:5] == "group" else 0, 8, False, 1), vars(r)
        assert [(s.repair, s.split, s.split_k, s.group_k, s.compact) for s in seen] == [(False, k, r.split_k, r.group_k, False),
                                                                                       (True, 0, 0, 0, False)], "member launch, then its repair launch"
        runtime2.check_split_errors(torch.device(DEV))
        assert runtime2._MODE_FLAGS[key[:5] == "group", False].get(torch.device(DEV)) is True, "the mode went off during the call"
    else:
        assert len(seen) == 1
        assert (r.split, r.split_k, r.group_k) == (0, 0, 0), vars(r)
        assert (r.nw, r.compact, r.t) == ({"nw4": 4}.get(key, 8), key == "compact", int(form[-1])), vars(r)
    return x


def _other(name):
    """A row of another shape and program to run in between."""
    return "w16_d1" if name != "w16_d1" else "n8_m4"


@pytest.mark.parametrize("name,form", U.PAIRS)
def test_program_kernel_matches_float64(name, form, monkeypatch):
    ref = U.reference(name)
    _select(monkeypatch, form)
    if U.program_key(form)[:5] in ("split", "group"):
        _mode_ready(name, form)
    x = _run(name, form, monkeypatch)
    tol, scale = U.tolerance(name), max(1.0, float(ref.x.abs().max()))
    if (name, form) in U.TWIN_BAR:                 # (the program's own fp32 summation order: 2 x the CPU twin's error, capped)
        tol = min(2.0 * U.TWIN_BAR[name, form][1], U.TWIN_BAR_MAX)
    assert x.dtype == torch.float32 and x.shape == ref.x.shape
    err = float((x.double().cpu() - ref.x).abs().max()) / scale
    print(f"\n{name} {form}: device error {err:.3e} of the scale {scale:.3f} (tolerance {tol:.1e})")
    assert torch.isfinite(x).all()
    torch.testing.assert_close(x.double().cpu(), ref.x, rtol=tol, atol=tol * scale)
    again = _run(name, form, monkeypatch)
    assert torch.equal(again, x), "a second identical call gives other bits"
    _select(monkeypatch, "nw8_t1")
    _run(_other(name), "nw8_t1", monkeypatch)
    _select(monkeypatch, form)
    assert torch.equal(_run(name, form, monkeypatch), x), "other bits after a row of another shape ran in between"


@pytest.mark.parametrize("name", U.REFUSALS)
def test_refused_rows_go_to_the_gemm_executor_at_the_same_bar(name, monkeypatch):
    ref = U.reference(name)
    for hook in U.HOOKS:
        monkeypatch.delenv(hook, raising=False)
    x = _run(name, None, monkeypatch)
    tol, scale = U.tolerance(name), max(1.0, float(ref.x.abs().max()))
    err = float((x.double().cpu() - ref.x).abs().max()) / scale
    print(f"\n{name}: {'GEMM-executor' if U.CASES[name].gemm else 'stock-module'} error {err:.3e} of the scale {scale:.3f} (tolerance {tol:.1e})")
    assert x.dtype == torch.float32 and torch.isfinite(x).all()
    torch.testing.assert_close(x.double().cpu(), ref.x, rtol=tol, atol=tol * scale)


_T_GROUPS = [(n, key, [f for f in U.CASES[n].forms if U.program_key(f) == key]) for n in U.SERVED
             for key in dict.fromkeys(U.program_key(f) for f in U.CASES[n].forms)]


@pytest.mark.parametrize("name,key,forms", [g for g in _T_GROUPS if len(g[2]) >= 2], ids=lambda v: v if isinstance(v, str) else "t")
def test_trajectories_per_workgroup_never_change_a_bit(name, key, forms, monkeypatch):
    outs = []
    for form in forms:
        _select(monkeypatch, form)
        outs.append(_run(name, form, monkeypatch))
    for form, x in zip(forms[1:], outs[1:]):
        assert torch.equal(x, outs[0]), f"{name}: {form} and {forms[0]} differ"
