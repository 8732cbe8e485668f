"""``solver_step_kernel`` (csrc/cdx_bigbatch.hip, behind run_step / launch_step) against float64, over every plan the solver classes
build: each case of tests/solver_step_cases.py runs ``sample()`` on the device with the recorded draws and is compared with the float64
CPU host loop of the same package (one run per case and process, ``solver_step_cases.reference``).

Tolerance: 4 x YARDSTICK, relative to max(1, max |x64|), as rtol and as atol.  YARDSTICK is the largest error of the fp32 CPU host loop
against the float64 one over all cases (tests/test_solver_step_cases_cpu.py); the factor 4 covers the other summation order and FMA
contraction of the device GEMMs.  Nothing here is derived from a device result.  (Measured on an MI355X, largest error per executor
against the 2.4e-5 tolerance: residual MLP 7.0e-6, DiT1d 6.3e-6, ChiTransformer 5.4e-6, PearceTransformer 6.9e-6, ChiUNet-GEMM 4.4e-6,
the large case 6.8e-6: the device is about as far from float64 as the fp32 host loop is, and most of the factor is slack.)

The fix-mask of every masked case has one element of 0.5 beside its ones (``solver_step_cases.build``).  Where m = 1 the blend with
prior that ends a step overwrites whatever the update made of that element, so a 0 / 1 mask cannot show a wrong mask on the
PREDICTION (kinds 3 / 4, CDX_STEP_MASK_PRED); the host loops blend with any m.  That element is how this sweep found that the legacy
EDM class masks its slope and the kernel did not.

Every case runs on the residual-MLP executor, whole and in chunks of 2 (batch 5: the last chunk holds one row, so the `b0` offsets
into noise, prior and the condition rows are exercised); a subset runs on the other four executors, whose prev / xold / pred buffers
are their own; one case is large enough for a second trip of launch_step's grid-stride loop.

The program kernel (csrc/cdx_unet2.hip) calls the same per-element step (csrc/cdx_step.h) on its LDS-resident state: the cases of
``PROGRAM_SUBSET`` run on the two U-Nets at their default route, against the same references at the same tolerance."""
import pytest
import torch

import solver_step_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 4.0 * S.YARDSTICK


def _spy_loops(monkeypatch):
    """Every ``bigbatch._run`` request as (kind, number of step records): a sampling loop has n_steps > 0, a stand-alone forward 0."""
    from cleandiffuser_amd.engine import bigbatch
    calls, orig = [], bigbatch._run

    def wrapped(kind, *a, **k):
        calls.append((kind, k["n_steps"], k["chunk"]))
        return orig(kind, *a, **k)
    monkeypatch.setattr(bigbatch, "_run", wrapped)
    return calls


def _check(x, ref_x, what):
    scale = max(1.0, float(ref_x.abs().max()))
    err = float((x.double().cpu() - ref_x).abs().max()) / scale
    print(f"\n{what}: device error {err:.3e} of the scale {scale:.3f} (tolerance {TOL:.1e})")
    assert torch.isfinite(x).all()
    torch.testing.assert_close(x.double().cpu(), ref_x, rtol=TOL, atol=TOL * scale)


def _run_case(name, executor, chunk, monkeypatch, ref, case=None):
    from cleandiffuser_amd.engine import bigbatch
    spec = S.EXECUTORS[executor]
    agent = S.build(name, executor, DEV, case=case)
    monkeypatch.setattr(bigbatch, "UNET_GEMM_MIN_BATCH", 1)
    monkeypatch.setitem(bigbatch.CHUNK_OVERRIDE, "dit" if spec.kind == "pearcetf" else spec.kind, chunk)
    calls = _spy_loops(monkeypatch)
    x = S.sample(agent, ref.case, ref.inp, device=DEV)
    torch.cuda.synchronize()
    loops = [c for c in calls if c[1] > 0]
    if (executor, name) in S.REFUSED:
        assert loops == [], "REFUSED lists this request, but the dispatcher served it natively"
    else:
        assert len(calls) == 1 and len(loops) == 1, \
            f"exactly one native call must serve the loop, got {calls}: the dispatcher refused the request and the torch loop ran"
        assert loops[0][:2] == (spec.kind, len(ref.plan.steps))
        if chunk is not None:
            assert loops[0][2] == chunk
        else:
            assert loops[0][2] >= x.shape[0], "the default chunk rule holds this batch in one chunk"
    return x


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("name", S.TABLE)
def test_step_matches_float64(name, chunk, monkeypatch):
    ref = S.reference(name, "mlp")
    x = _run_case(name, "mlp", chunk, monkeypatch, ref)
    _check(x, ref.x, f"mlp {name} chunk {chunk}")


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("name", S.EXECUTOR_SUBSET)
@pytest.mark.parametrize("executor", ["dit", "chitf", "pearcetf", "chiunet"])
def test_step_matches_float64_on_every_executor(executor, name, chunk, monkeypatch):
    ref = S.reference(name, executor)
    assert ref.env[1] == 1 and (ref.env[2] == 1 or ref.case.cls == "ContinuousConsistencyModel")
    x = _run_case(name, executor, chunk, monkeypatch, ref)
    _check(x, ref.x, f"{executor} {name} chunk {chunk}")


@pytest.mark.parametrize("name", S.PROGRAM_SUBSET)
@pytest.mark.parametrize("executor", S.PROGRAM_EXECUTORS)
def test_program_kernel_step_matches_float64(executor, name, monkeypatch):
    """The same step (csrc/cdx_step.h) as the program kernel runs it on its LDS-resident state: batch 5 is below the U-Nets' crossover, so
    with UNET_GEMM_MIN_BATCH left alone ``runtime2.fused_sample2`` serves the loop in one cdx_unet2_run launch.  The three masked ledm_*
    cases are the ones a step that ignores CDX_STEP_MASK_PRED on kinds 5 / 6 fails (tests/test_solver_step_cases_cpu.py: by 0.1 and more
    of the scale)."""
    from cleandiffuser_amd.engine import runtime2
    ref = S.reference(name, executor)
    served, orig = [], runtime2.fused_sample2

    def spy(*a, **k):
        out = orig(*a, **k)
        served.append(out is not None)
        return out
    monkeypatch.setattr(runtime2, "fused_sample2", spy)
    calls = _spy_loops(monkeypatch)
    x = S.sample(S.build(name, executor, DEV), ref.case, ref.inp, device=DEV)
    torch.cuda.synchronize()
    assert [c for c in calls if c[1] > 0] == [], "the GEMM executor ran the loop"
    if (executor, name) in S.PROGRAM_REFUSED:
        assert True not in served, "PROGRAM_REFUSED lists this request, but the program kernel served it"
    else:
        assert served == [True], f"exactly one program-kernel call must serve the loop, got {served}"
    _check(x, ref.x, f"program {executor} {name}")


def test_grid_stride_second_trip_matches_float64(monkeypatch):
    """300 000 rows x 4 in one chunk: more elements than the 4096 x 256 threads launch_step starts.  Compared on 4096 rows at a stride and
    the last 64 (the rows of a residual MLP are independent, so the float64 loop runs on those rows alone)."""
    L, case, rows = S.LARGE, S.large_case(), S.large_rows()
    assert L.batch * case.x_shape[0] > 4096 * 256
    inp = S.make_inputs(L.name, L.executor, batch=L.batch)
    ref = S.host_run(L.name, torch.float64, L.executor, inp={k: v[:, rows] if k == "noise" else v[rows] for k, v in inp.items()}, case=case)
    assert len(ref.plan.steps) == 2 and ref.env == (1, 1, 0) and ref.plan.n_noise == 1
    full = type(ref)(case=case, inp=inp, plan=ref.plan)
    x = _run_case(L.name, L.executor, None, monkeypatch, full, case=case)
    assert x.shape == (L.batch, 4)
    _check(x[rows.to(DEV)], ref.x, f"large {L.name}")
