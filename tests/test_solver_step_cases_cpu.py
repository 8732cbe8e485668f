"""The table of tests/solver_step_cases.py, kept honest without a GPU: every case runs the package's host loop on the CPU in float64 and
the test reads the request off it (the ``SamplePlan`` the solver object built, the clamp, the mask, the classifier-free halves).

* CASES produces exactly SIGNATURES -- the branches of ``solver_step_kernel`` (csrc/cdx_bigbatch.hip).
* Where a case has a per-step clamp, the float64 run changes between 2 % and 60 % of the elements at one step or more; a fix-mask
  leaves ``prior`` where it is 1 and nowhere else (one element is 0.5, see ``solver_step_cases.build``); cfg_mode 2 combines two predictions that differ; a multistep / Heun plan pushes at
  one step and reads at a later one.
* The yardstick: E32(case) = max |x32 - x64| / max(1, max |x64|) of the fp32 host loop against the float64 one on the same inputs and
  recorded draws.  No case exceeds the committed YARDSTICK, which tests/test_gpu_solver_step.py multiplies by 4.

Measured (8 CPU threads): E32 is 4.1e-8 .. 5.74e-6 over the 151 cases, and YARDSTICK is that maximum rounded up to 6e-6.  The ten
largest: lddpm_eps_full 5.74e-6, c_ddim_eps_full 5.02e-6, c_ode1_eps_full 4.76e-6, d_sdepp2M_x0_full 3.53e-6, c_odepp2M_eps_full
3.48e-6, c_odepp1_eps_full 2.88e-6, d_ddim_eps_full 2.77e-6, d_ode1_eps_full 2.70e-6, ldpm_odedpmpp2_eps_full 2.29e-6,
d_odepp2M_x0_full 2.28e-6.  `pytest -s` prints every case's E32 and its clamp share per step."""
import pytest
import torch

import solver_step_cases as S


@pytest.fixture(scope="module")
def runs():
    return {name: S.reference(name) for name in S.TABLE}


def test_cases_cover_exactly_the_kernels_branches(runs):
    produced = set().union(*(r.signatures for r in runs.values()))
    assert produced - S.SIGNATURES == set(), "a case reaches a branch SIGNATURES does not list"
    assert S.SIGNATURES - produced == set(), "a branch of solver_step_kernel has no case"
    for name, r in runs.items():                        # each case still is what its name says
        case = r.case
        per_step_clamp = case.clip is not None and "flow" not in name
        assert r.env == (int(per_step_clamp), int(case.mask), int(case.w_cfg not in (None, 1.0) and case.cls != "ContinuousConsistencyModel")), name
        assert len(r.plan.steps) <= 6 and r.plan.n_noise + 1 <= S.N_DRAWS, name


def test_every_solver_class_and_variant_is_in_the_table():
    from cleandiffuser_amd.engine.plan import LEGACY_DPM_SAMPLERS, SUPPORTED_SOLVERS
    by_cls = {}
    for case in S.CASES.values():
        by_cls.setdefault(case.cls, []).append(case)
    for cls in ("DiscreteDiffusionSDE", "ContinuousDiffusionSDE"):
        assert {(c.sample["solver"], c.ctor["predict_noise"]) for c in by_cls[cls]} == {(s, p) for s in SUPPORTED_SOLVERS for p in (True, False)}
    assert {c.ctor["predict_noise"] for c in by_cls["DDPM"]} == {True, False}
    assert {c.sample["sampler"] for c in by_cls["DPMSolver"]} == set(LEGACY_DPM_SAMPLERS)
    for cls in ("ContinuousEDM", "EDM"):
        assert {c.sample["solver"] for c in by_cls[cls]} == {"euler", "heun"}
        assert any(c.sample.get("diffusion_x_sampling_steps") or c.sample.get("extra_sample_steps") for c in by_cls[cls])
    for cls, cases in by_cls.items():                   # with and without bounds / mask, and every classifier-free mode the class has
        assert {c.mask for c in cases} == {True, False}, cls
        assert {c.clip is not None for c in cases} == ({False} if cls == "EDM" else {True, False}), cls
        assert {c.w_cfg for c in cases} == {None, 1.0, S.W2}, cls
    assert set(by_cls) == {"DiscreteDiffusionSDE", "ContinuousDiffusionSDE", "DDPM", "DPMSolver", "ContinuousEDM", "EDM",
                           "ContinuousRectifiedFlow", "DiscreteRectifiedFlow", "ContinuousConsistencyModel"}


def test_removing_a_branchs_only_case_is_noticed(runs):
    """The legacy x0 DDPM form (kind 4) comes from the two lddpm_x0 cases alone: without them the union misses its signatures."""
    rest = set().union(*(r.signatures for n, r in runs.items() if not n.startswith("lddpm_x0")))
    assert {s for s in S.SIGNATURES - rest} == {(4, 0, 0, 0, z, 0) + env for z in (0, 1) for env in ((0, 0, 0), (1, 1, 1))}


@pytest.mark.parametrize("name", S.TABLE)
def test_float64_run_meets_its_conditions(name, runs):
    r = runs[name]
    x, case = r.x, r.case
    assert x.dtype == torch.float64 and torch.isfinite(x).all()
    print(f"\n{name}: clamp share per step {[round(s, 3) for s in r.step_share]}, of the finished sample {[round(s, 3) for s in r.final_share]}")
    if r.env[0]:
        assert len(r.step_share) == len(r.plan.steps)
        assert any(0.02 <= s <= 0.60 for s in r.step_share), f"the clamp is idle or everywhere: {r.step_share}"
        free = 1.0 - (float(r.fix_mask.expand_as(x[0]).mean()) if case.mask else 0.0)
        assert all(s < free for s in r.final_share), "the finished sample sits at its bounds in every free element: nothing left to compare"
    elif case.clip is not None:                         # rectified flow: the one clip of the finished sample
        assert len(r.final_share) == 1 and 0.02 <= r.final_share[0] <= 0.60 + 0.2 * case.mask
    if case.mask:
        m = (r.fix_mask == 1.0).expand_as(x[0])             # (one more element has m = 0.5: neither prior nor free)
        assert ((r.fix_mask > 0) & (r.fix_mask < 1)).sum() == 1
        prior = torch.from_numpy(r.inp["prior"]).double()     # (inside every case's bounds: the clip of the finished sample keeps it)
        assert m.any() and not m.all() and float(prior.abs().max()) < 1.0
        assert torch.equal(x[:, m], prior[:, m]), "masked columns must hold prior"
        assert (x[:, ~m] != prior[:, ~m]).all(), "unmasked columns must not"
    if r.env[2]:
        c, u = r.halves[0]
        assert float((c - u).abs().max()) > 1e-2 * float(torch.maximum(c.abs().max(), u.abs().max()))
    else:
        assert not r.halves
    pushes = [i for i, st in enumerate(r.plan.steps) if st.push]
    reads = [i for i, st in enumerate(r.plan.steps) if st.kind == 6 or (st.kind == 2 and st.vsel >= 2)]
    if pushes or reads:
        assert pushes and reads and min(pushes) < max(reads), "a multistep / Heun plan pushes at one step and reads at a later one"
        assert all(any(p < i for p in pushes) for i in reads), "nothing reads the memory before it is written"
    multistep = any(k in name for k in ("2M", "dpm2", "dpmpp2", "heun"))
    assert bool(reads) == multistep, name


def test_program_subset_reaches_every_kind_the_memory_read_and_both_pushes():
    """What the program kernel's sweep (tests/test_gpu_solver_step.py) must reach of the shared step, on both of its executors."""
    for executor in S.PROGRAM_EXECUTORS:
        sigs = set().union(*(S.reference(name, executor).signatures for name in S.PROGRAM_SUBSET))
        assert sigs <= S.SIGNATURES
        assert {s[0] for s in sigs} == set(range(8)), executor
        assert any(s[0] == 2 and s[1] == 2 for s in sigs), "a multistep read (vsel 2)"
        assert any(s[0] == 2 and s[2] for s in sigs) and any(s[0] == 5 and s[2] for s in sigs), "the multistep push and the EDM push"
        assert any(s[0] in (5, 6) and s[3] and s[7] for s in sigs), "CDX_STEP_MASK_PRED on an EDM record, with a fix-mask"


@pytest.mark.parametrize("name", S.PROGRAM_LEDM)
@pytest.mark.parametrize("executor", S.PROGRAM_EXECUTORS)
def test_masked_legacy_edm_cases_show_a_step_that_ignores_the_flag(executor, name):
    """The legacy EDM class masks its slope (CDX_STEP_MASK_PRED on kinds 5 / 6).  A step that ignores the flag -- the record interpreter
    with the flags cleared -- must land far outside the GPU sweep's tolerance, or the sweep could not tell; with the flags it agrees with
    the host loop.  Both relative to max(1, max |x64|), float64 throughout.  Measured, without / with the flags -- chiunet: ledm_heun_full
    2.31e-1 / 2.0e-7, ledm_euler_full 2.31e-1 / 2.5e-8, ledm_heun_mask 1.05e-1 / 1.2e-7; janner: 3.52e-1 / 2.1e-7, 3.70e-1 / 1.7e-7,
    3.79e-1 / 4.5e-7 (the bound of the first is 2.4e-3)."""
    r = S.reference(name, executor)
    assert r.env[1] == 1 and all(st.flags & 1 for st in r.plan.steps if st.kind in (5, 6))
    scale = max(1.0, float(r.x.abs().max()))
    off = float((S.sim_run(name, executor, keep_flags=False) - r.x).abs().max()) / scale
    on = float((S.sim_run(name, executor) - r.x).abs().max()) / scale
    print(f"\n{executor} {name}: flags cleared {off:.3e}, flags kept {on:.3e} of the scale {scale:.3f}")
    assert off > 100 * 4.0 * S.YARDSTICK
    assert on <= 1e-5


@pytest.mark.parametrize("name", S.TABLE)
def test_fp32_host_loop_is_within_the_yardstick(name, runs):
    r = runs[name]
    x32 = S.host_run(name, torch.float32, inp=r.inp).x
    assert x32.dtype == torch.float32
    e32 = float((x32.double() - r.x).abs().max()) / max(1.0, float(r.x.abs().max()))
    print(f"\n{name}: E32 {e32:.3e}  max|x64| {float(r.x.abs().max()):.3f}")
    assert e32 <= S.YARDSTICK
