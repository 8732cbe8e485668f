"""TEST HELPER for the solver step of the GEMM executors (csrc/cdx_bigbatch.hip:solver_step_kernel behind run_step / launch_step): the
branches of that kernel as a table of signatures, named ``sample()`` requests that produce them, and for each request ONE float64 CPU
run of the package's own host loop -- the reference tests/test_gpu_solver_step.py compares the device with.

A signature is what decides which statements of the kernel execute for one step record of one request:

    (kind, vsel, push, CDX_STEP_MASK_PRED, draws noise, predict_noise, clamp present, fix-mask present, cfg_mode == 2)

normalised the way the kernel reads the record (``normalise``): `vsel` only for kind 2, the flag for kinds 2, 5 and 6, `predict_noise`
not for kinds >= 5 (None), `push` for kind 5 but not 6 / 7, the draw not for kinds 1, 5, 6.  ``SIGNATURES`` is written down from the
kernel and the plan builders' record forms (engine/plan.py); tests/test_solver_step_cases_cpu.py asserts that ``CASES`` produces exactly
that set, so a new branch needs a case and a case that stops reaching its branch fails.

Every case samples a tiny IDQLMlp (the residual-MLP executor, ``cdx_resmlp_run``); ``EXECUTORS`` has the smallest nets of the other
four executors for the subset of ``EXECUTOR_SUBSET``, and a JannerUNet1d: the two U-Nets also run ``PROGRAM_SUBSET`` on the program
kernel, which calls the same step function (csrc/cdx_step.h).  Weights are ``load_synth`` streams with the output layer scaled by `den_scale`;
bounds, `den_scale` and `temperature` are chosen per family so that the float64 run ALONE meets the conditions of the CPU test (a clamp
that changes between 2 % and 60 % of the elements at some step, a visible classifier-free difference)."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cases as _cases

B = 5                       # batch of every case: with a chunk of 2 the last chunk holds one row
OBS = 7                     # width of the observation of the conditional cases
N_DRAWS = 8                 # recorded draws per case: x_T and at most six stochastic steps

# ------------------------------------------------------------------------------------------------ #
# the kernel's branches                                                                                #
# ------------------------------------------------------------------------------------------------ #
_BARE, _FULL = (0, 0, 0), (1, 1, 1)
_PAIR = [_BARE, _FULL]
_EVERY = _PAIR + [(1, 0, 0), (0, 1, 0), (0, 0, 1)]          # (clamp, fix-mask, cfg_mode == 2): the three blocks are independent statements


def _signatures():
    out = set()
    add = lambda cores, envs: out.update(tuple(c) + tuple(e) for c in cores for e in envs)     # noqa: E731
    for pn in (1, 0):
        ddpm = [(0, 0, 0, 0, 1, pn), (0, 0, 0, 0, 0, pn)]                  # kind 0: the last step draws nothing
        add(ddpm, _EVERY if pn else _PAIR)
        add([(1, 0, 0, 0, 0, pn)], _PAIR)                                  # kind 1
        # kind 2 without the flag (the SDE classes): V = eps | xth, one-step; 2M: the first record pushes xth, the later ones read it
        add([(2, v, 0, 0, z, pn) for v in (0, 1) for z in (0, 1)], _PAIR)
        add([(2, v, 1, 0, z, pn) for v in (1, 2) for z in (0, 1)], _PAIR)
        # kind 2 with CDX_STEP_MASK_PRED (legacy DPMSolver): first order, and second order pushing eps (2) or xth (1)
        add([(2, v, 0, 1, z, pn) for v in (0, 1) for z in (0, 1)], _PAIR)
        add([(2, v, p, 1, z, pn) for v, p in ((0, 2), (3, 2), (1, 1), (2, 1)) for z in (0, 1)], _PAIR)
    add([(2, v, 1, 1, 1, 0) for v in (1, 2)], _EVERY)                      # (the DPMSolver lead: sde_dpmpp_2, x0-prediction)
    add([(2, 0, 0, 0, 0, 1)], [(0, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1)])    # rectified flow: linear records, never a per-step clamp
    add([(3, 0, 0, 0, z, 1) for z in (0, 1)], _EVERY)                      # legacy DDPM, eps: p (1 - m)
    add([(4, 0, 0, 0, z, 0) for z in (0, 1)], _PAIR)                       # legacy DDPM, x0: p (1 - m) + x m
    # EDM Euler, and Heun: the predictor pushes slope and state, the corrector reads them.  The legacy class sets the flag (its slope is
    # masked) and has no bounds
    add([(5, 0, 0, 0, 0, None), (5, 0, 1, 0, 0, None), (6, 0, 0, 0, 0, None)], _EVERY)
    add([(5, 0, 0, 1, 0, None), (5, 0, 1, 1, 0, None), (6, 0, 0, 1, 0, None)], [(0, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 1)])
    add([(7, 0, 0, 0, z, None) for z in (0, 1)], [(0, 0, 0), (1, 1, 0), (1, 0, 0), (0, 1, 0)])   # consistency: never cfg_mode 2
    return frozenset(out)


SIGNATURES = _signatures()


def normalise(st, predict_noise):
    """The part of a step record (plan.Step) the kernel's control flow reads."""
    k = st.kind
    if k >= 5:
        return (k, 0, int(st.push) if k == 5 else 0, (st.flags & 1) if k != 7 else 0, int(st.noise) if k == 7 else 0, None)
    pn = int(bool(predict_noise))
    if k == 2:
        return (2, st.vsel, int(st.push), st.flags & 1, int(st.noise), pn)
    return (k, 0, int(st.push), 0, int(st.noise) if k != 1 else 0, pn)


# ------------------------------------------------------------------------------------------------ #
# the requests                                                                                         #
# ------------------------------------------------------------------------------------------------ #
def _c(cls, ctor=None, sample=None, method="sample", clip=None, mask=False, w_cfg=None, den_scale=1.0, temperature=1.0):
    return SimpleNamespace(cls=cls, ctor=dict(ctor or {}), sample=dict(sample or {}), method=method, clip=clip, mask=mask, w_cfg=w_cfg,
                           den_scale=den_scale, temperature=temperature)


W2 = 1.3                    # the classifier-free weight that is neither 0 nor 1


def _envs(lead):
    """name suffix -> (clamp, mask, w_cfg): every variant runs bare and with everything on; a class's lead variant also one block at
    a time, the clamp one with w_cfg = 1.  A class without bounds, or whose bounds never reach the step (rectified flow clips the finished
    sample only), keeps the requests and gives the signatures without the clamp."""
    envs = {"bare": (False, False, None), "full": (True, True, W2)}
    if lead:
        envs.update(clamp_w1=(True, False, 1.0), mask=(False, True, None), cfg=(False, False, W2))
    return envs


# eps-prediction: a synthetic denoiser's eps is unrelated to x, so x0 = (x - sigma eps) / alpha is clamped nearly everywhere unless eps is
# small (den_scale) and the bounds leave room; x0-prediction clamps the output itself.  The deterministic solvers never leave a bound once
# clamped to it, so they start from a small x_T; the sde_dpm solvers (2 sigma expm1(h) eps, no contraction) overshoot at four steps and
# need wide bounds.  Without a clamp eps stays small, else x_T / alpha_T ~ 100 x_T hides every other term.  The values are the ones at
# which the float64 run meets the share condition and leaves the finished sample off its bounds somewhere
# (tests/test_solver_step_cases_cpu.py asserts both and prints the shares).
def _tune(pn, clamp, group=""):
    if not clamp:
        return dict(clip=None, den_scale=0.03, temperature=0.05) if pn else dict(clip=None, den_scale=1.0)
    if group in ("sde1", "sde2"):          # (sde_dpm_2 on an x0 net runs away fastest: three steps, a smaller output)
        return dict(clip=30.0, den_scale=0.1, temperature=0.5) if pn else dict(clip=30.0, den_scale=0.3 if group == "sde2" else 1.0)
    if pn:
        return dict(clip=5.0, den_scale=0.3, temperature=0.1) if group == "det" else dict(clip=2.5, den_scale=0.1)
    return dict(clip=1.0, den_scale=1.0)


def _group(solver):
    if solver in ("sde_dpmsolver_1", "sde_dpm_1", "sde_dpm_2"):
        return "sde2" if solver == "sde_dpm_2" else "sde1"
    return "det" if solver[:3] in ("ddi", "ode") else ""


def _table():
    t = {}

    def put(name, lead, make):
        for env, (clamp, mask, w) in _envs(lead).items():
            t[f"{name}_{env}"] = make(clamp, mask, w)

    short = lambda s: s.replace("dpmsolver", "").replace("++", "pp").replace("_", "")     # noqa: E731
    for tag, cls, ctor, sched in (("d", "DiscreteDiffusionSDE", dict(diffusion_steps=20), "uniform"),
                                  ("c", "ContinuousDiffusionSDE", {}, "quad_continuous")):
        for solver in ("ddpm", "ddim", "ode_dpmsolver_1", "ode_dpmsolver++_1", "ode_dpmsolver++_2M", "sde_dpmsolver_1", "sde_dpmsolver++_1",
                       "sde_dpmsolver++_2M"):
            for pn in (True, False):
                put(f"{tag}_{short(solver)}_{'eps' if pn else 'x0'}", solver == "ddpm" and pn,
                    lambda clamp, mask, w, cls=cls, ctor=ctor, solver=solver, pn=pn, sched=sched: _c(
                        cls, dict(ctor, predict_noise=pn), dict(solver=solver, sample_steps=4, sample_step_schedule=sched), mask=mask,
                        w_cfg=w, **_tune(pn, clamp, _group(solver))))
    for pn in (True, False):
        put(f"lddpm_{'eps' if pn else 'x0'}", pn, lambda clamp, mask, w, pn=pn: _c(
            "DDPM", dict(diffusion_steps=5, predict_noise=pn), dict(sample_steps=5), mask=mask, w_cfg=w, **_tune(pn, clamp)))
    for sampler in ("ode_dpm_1", "ddim", "sde_dpm_1", "ode_dpmpp_1", "sde_dpmpp_1", "ode_dpm_2", "sde_dpm_2", "ode_dpmpp_2", "sde_dpmpp_2"):
        for pn in (True, False):
            put(f"ldpm_{sampler.replace('_', '')}_{'eps' if pn else 'x0'}", sampler == "sde_dpmpp_2" and not pn,
                lambda clamp, mask, w, sampler=sampler, pn=pn: _c(
                    "DPMSolver", dict(predict_noise=pn), dict(sampler=sampler, sample_steps=3 if sampler == "sde_dpm_2" else 4),
                    mask=mask, w_cfg=w, **_tune(pn, clamp, _group(sampler))))
    put("ldpm_sdedpm1_x0_x", False, lambda clamp, mask, w: _c(          # sample_x: two more repeats of the last record
        "DPMSolver", dict(predict_noise=False), dict(sampler="sde_dpm_1", sample_steps=3, extra_sample_steps=2), method="sample_x",
        mask=mask, w_cfg=w, **_tune(False, clamp, "sde1")))
    edm = dict(sigma_max=10.0)
    for solver, extra, lead in (("euler", 0, False), ("heun", 0, True), ("heun", 1, False)):
        put(f"edm_{solver}{'_x' if extra else ''}", lead, lambda clamp, mask, w, solver=solver, extra=extra: _c(
            "ContinuousEDM", edm, dict(solver=solver, sample_steps=3, diffusion_x_sampling_steps=extra), mask=mask, w_cfg=w,
            clip=1.0 if clamp else None))
    for solver, method, extra, lead in (("euler", "sample", {}, False), ("heun", "sample", {}, True),
                                        ("euler", "sample_x", dict(extra_sample_steps=2), False)):
        for env, (_, mask, w) in _envs(lead).items():                       # (the legacy EDM class has no bounds)
            t[f"ledm_{solver}{'_x' if extra else ''}_{env.replace('clamp_', '')}"] = _c(
                "EDM", edm, dict(solver=solver, sample_steps=3, **extra), method=method, mask=mask, w_cfg=w)
    for tag, cls, ctor, sched in (("cflow", "ContinuousRectifiedFlow", {}, "uniform_continuous"),
                                  ("dflow", "DiscreteRectifiedFlow", dict(diffusion_steps=20), "uniform")):
        put(tag, True, lambda clamp, mask, w, cls=cls, ctor=ctor, sched=sched: _c(
            cls, ctor, dict(sample_steps=4, sample_step_schedule=sched, diffusion_x_sampling_steps=1), mask=mask, w_cfg=w,
            clip=1.5 if clamp else None))
    put("cm", True, lambda clamp, mask, w: _c(
        "ContinuousConsistencyModel", edm, dict(sample_steps=4, diffusion_x_sampling_steps=1), mask=mask, w_cfg=w,
        clip=1.0 if clamp else None))
    return t


CASES = _table()
TABLE = sorted(CASES)

# the largest E32 over CASES: max |x32 - x64| / max(1, max |x64|) of the fp32 CPU host loop against the float64 one on the same inputs
# and draws, as tests/test_solver_step_cases_cpu.py measures it (its docstring has the figures); the GPU tolerance is 4 x this
YARDSTICK = 6e-6


# ------------------------------------------------------------------------------------------------ #
# the executors: their smallest nets, and the subset of cases the four others run                      #
# ------------------------------------------------------------------------------------------------ #
def _e(net, x_shape, cond_shape, kind, needs_cond=False):
    return SimpleNamespace(net=net, x_shape=x_shape, cond_shape=cond_shape, kind=kind, needs_cond=needs_cond)


EXECUTORS = {       # name -> net, state shape, condition shape, the name bigbatch._run is called with, "the backbone cannot run without a condition"
    "mlp": _e(("IDQLMlp", dict(obs_dim=OBS, act_dim=5, emb_dim=16, hidden_dim=32, n_blocks=1)), (5,), (OBS,), "mlp"),
    "mlp4": _e(("IDQLMlp", dict(obs_dim=OBS, act_dim=4, emb_dim=16, hidden_dim=32, n_blocks=1)), (4,), (OBS,), "mlp"),      # (the large case)
    "dit": _e(("DiT1d", dict(in_dim=3, emb_dim=16, d_model=32, n_heads=2, depth=1, timestep_emb_type="positional")), (4, 3), (16,), "dit"),
    "chitf": _e(("ChiTransformer", dict(act_dim=3, obs_dim=OBS, Ta=4, To=2, d_model=32, nhead=2, num_layers=1)), (4, 3), (2, OBS), "chitf"),
    "pearcetf": _e(("PearceTransformer", dict(act_dim=5, To=2, emb_dim=16, trans_emb_dim=16, nhead=2)), (5,), (2, 16), "pearcetf", True),
    "chiunet": _e(("ChiUNet1d", dict(act_dim=3, obs_dim=OBS, To=2, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=3)), (4, 3),
                  (2, OBS), "chiunet", True),
    "janner": _e(("JannerUNet1d", dict(in_dim=3, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=3)), (4, 3), (16,), "chiunet"),
}
# `prev` / `xold` / `pred` are each executor's own buffers: a 2M multistep with cfg_mode 2, EDM Heun with clamp and mask, consistency with
# mask and noise, legacy DDPM with mask (both predictions: of the GEMM executors only the U-Net one is offered the legacy DDPM class, so
# kinds 3 / 4 reach this kernel through it alone), a CDX_STEP_MASK_PRED sampler, ddpm with a fix-mask
EXECUTOR_SUBSET = ("c_odepp2M_eps_full", "edm_heun_full", "cm_full", "lddpm_eps_full", "lddpm_x0_full", "ldpm_sdedpmpp2_x0_full",
                   "c_ddpm_eps_full")
_LEGACY_DDPM = ("dispatch.try_fused_legacy_ddpm offers the legacy DDPM class to the U-Net executor only (unet_only): over this backbone "
                "it runs the PyTorch loop")
# (executor, case) -> reason: requests the dispatcher does not hand to the executor; they run the PyTorch loop and must still match
REFUSED = {(ex, name): _LEGACY_DDPM for ex in ("mlp", "dit", "chitf", "pearcetf")
           for name in TABLE if CASES[name].cls == "DDPM" and (ex == "mlp" or name in EXECUTOR_SUBSET)}

# The program kernel (csrc/cdx_unet2.hip) runs the same per-element step (csrc/cdx_step.h) on its LDS-resident state: the two U-Nets at
# batch B, below their crossover to the GEMM executor, are served by runtime2.fused_sample2.  Beside EXECUTOR_SUBSET: the legacy EDM
# class with a fix-mask (CDX_STEP_MASK_PRED on kinds 5 / 6: the slope is masked, which only the mask element of 0.5 can show), and a ddim
# plan (kind 1, which no case of EXECUTOR_SUBSET has)
PROGRAM_EXECUTORS = ("chiunet", "janner")
PROGRAM_LEDM = ("ledm_heun_full", "ledm_euler_full", "ledm_heun_mask")
PROGRAM_SUBSET = EXECUTOR_SUBSET + PROGRAM_LEDM + ("c_ddim_eps_full",)
# (executor, case) -> reason: requests the dispatcher does not hand to the program kernel; they must still match on the route they take
PROGRAM_REFUSED = {}


def case_of(name, executor="mlp"):
    """Case `name` as `executor` runs it: its state shape, and w_cfg = 1 where the case has no condition but the backbone needs one."""
    case, spec = CASES[name], EXECUTORS[executor]
    w = 1.0 if (case.w_cfg is None and spec.needs_cond) else case.w_cfg
    return SimpleNamespace(**{**vars(case), "x_shape": spec.x_shape, "w_cfg": w})


def build(name, executor="mlp", device="cpu", dtype=torch.float32, case=None, spec=None):
    """The agent of a case on this package's classes, eval mode.  `spec`: a net outside ``EXECUTORS`` (tests/executor_shape_cases.py)."""
    from cleandiffuser_amd.utils import load_synth
    case, spec, lib = case or case_of(name, executor), spec or EXECUTORS[executor], _cases.lib_namespace("amd")
    net = load_synth(getattr(lib, spec.net[0])(**spec.net[1]), 81)
    head = [m for m in net.modules() if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d))][-1]      # the output layer, scaled
    with torch.no_grad():
        head.weight.mul_(case.den_scale)
        head.bias.mul_(case.den_scale)
    net = net.to(device=device, dtype=dtype)
    if dtype != torch.float32:           # (the embeddings are evaluated in the dtype of t, fp32 for continuous times: hand them on as `dtype`)
        net.map_noise.register_forward_hook(lambda mod, args, out: out.to(dtype))
        if hasattr(net, "pos_embed"):    # (PearceTransformer evaluates its token position codes on fp32 indices)
            net.pos_embed.register_forward_pre_hook(lambda mod, args: (args[0].to(dtype),))
    kw, xs = dict(case.ctor), case.x_shape
    if case.mask:
        # the last column (and, for a (T, D) state, the whole first position) is given; one more element is given by half.  A 0 / 1 mask
        # cannot show a wrong mask on the PREDICTION (kinds 3 / 4, CDX_STEP_MASK_PRED): where m = 1 the blend with prior that ends
        # every step overwrites whatever the update made of it.  Where m = 0.5 it does not, and the host loops blend the same way
        fm = torch.zeros(xs, dtype=dtype)
        fm[..., -1] = 1.0
        if len(xs) == 2:
            fm[0] = 1.0
        fm.reshape(-1)[-2] = 0.5
        kw["fix_mask"] = fm
    if case.clip is not None and case.cls != "EDM":
        kw["x_max"] = torch.full((1, *xs), float(case.clip), dtype=dtype, device=device)
        kw["x_min"] = torch.full((1, *xs), -float(case.clip), dtype=dtype, device=device)
    agent = getattr(lib, case.cls)(net, lib.IdentityCondition(dropout=0.0), device=device, **kw)
    agent.eval()
    return agent


def make_inputs(name, executor="mlp", batch=B):
    """prior (b, *x), noise (N_DRAWS, b, *x), cond (b, *cond) of a case as float32 numpy arrays: seeded draws."""
    spec = EXECUTORS[executor]
    g = torch.Generator().manual_seed(2000 + TABLE.index(name))
    prior = 0.9 * (2.0 * torch.rand(batch, *spec.x_shape, generator=g) - 1.0)       # (inside every case's bounds)
    noise = torch.randn(N_DRAWS, batch, *spec.x_shape, generator=g)
    cond = torch.randn(batch, *spec.cond_shape, generator=g)
    return {"prior": prior.numpy(), "noise": noise.numpy(), "cond": cond.numpy()}


def sample(agent, case, inp, device="cpu", dtype=torch.float32):
    """``agent.sample`` (or ``sample_x``) on the recorded inputs and draws -> x."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)          # noqa: E731
    kw = dict(case.sample, n_samples=inp["prior"].shape[0])
    if case.cls != "EDM":                # (the legacy EDM class has no temperature)
        kw["temperature"] = case.temperature
    if case.w_cfg is not None:
        kw.update(condition_cfg=t(inp["cond"]), w_cfg=case.w_cfg)
    x, _ = getattr(agent, case.method)(t(inp["prior"]), noise=list(t(inp["noise"])), **kw)
    return x.detach()


_ENTRIES = ("try_fused_sample", "try_fused_edm", "try_fused_legacy_ddpm")


@contextlib.contextmanager
def spied(net, seen):
    """What the CPU test reads off a host-loop run: the plan and request every solver class hands its plan consumer (the ``dispatch.try_*``
    entry in front of its own loop, which answers None on the CPU), the share of elements each ``clip`` of a state-shaped tensor changed,
    in call order, and the two halves of every doubled-batch denoiser call."""
    from cleandiffuser_amd.engine import dispatch
    orig = {n: getattr(dispatch, n) for n in _ENTRIES}
    clip = torch.Tensor.clip

    def entry(n):
        def spy(solver, model, plan, xt, prior, cond_vec, w_cfg, *a, **k):
            seen.plan, seen.xt = plan, xt.detach().clone()
            seen.cfg2 = cond_vec is not None and w_cfg not in (0.0, 1.0)
            seen.cond, seen.w_cfg = cond_vec, w_cfg
            return orig[n](solver, model, plan, xt, prior, cond_vec, w_cfg, *a, **k)
        return spy

    def spy_clip(self, *a, **k):
        out = clip(self, *a, **k)
        if self.shape == seen.shape:         # (the step schedules clip their grids too)
            seen.share.append(float((out != self).double().mean()))
        return out

    def hook(mod, args, out):
        if out.shape[0] == 2 * seen.shape[0]:
            seen.halves.append((out[:seen.shape[0]].detach().clone(), out[seen.shape[0]:].detach().clone()))
    for n in _ENTRIES:
        setattr(dispatch, n, entry(n))
    torch.Tensor.clip = spy_clip
    handle = net.register_forward_hook(hook)
    try:
        yield
    finally:
        handle.remove()
        torch.Tensor.clip = clip
        for n in _ENTRIES:
            setattr(dispatch, n, orig[n])


def host_run(name, dtype, executor="mlp", inp=None, case=None, spec=None):
    """One CPU run of case `name` on the package's host loop in `dtype` -> x, the plan, the signatures of its step records, the clamp
    shares (per step; then the clip of the finished sample where the class has one) and the classifier-free halves."""
    from cleandiffuser_amd.engine.runtime import _predicts_noise
    case = case or case_of(name, executor)
    inp = make_inputs(name, executor) if inp is None else inp
    agent = build(name, executor, "cpu", dtype, case, spec)
    seen = SimpleNamespace(plan=None, xt=None, cfg2=False, cond=None, w_cfg=0.0, share=[], halves=[], shape=inp["prior"].shape)
    with spied(agent.model_ema["diffusion"], seen):
        x = sample(agent, case, inp, dtype=dtype)
    clamp = bool(getattr(seen.plan, "clip_each_step", True)) and (getattr(agent, "x_min", None) is not None or
                                                                   getattr(agent, "x_max", None) is not None)
    pn = _predicts_noise(seen.plan, agent)
    env = (int(clamp), int(torch.is_tensor(agent.fix_mask)), int(seen.cfg2))
    n_step_clips = len(seen.plan.steps) if clamp else 0
    return SimpleNamespace(case=case, inp=inp, x=x, plan=seen.plan, xt=seen.xt, env=env, cond=seen.cond, w_cfg=seen.w_cfg, predict_noise=pn,
                           signatures={normalise(st, pn) + env for st in seen.plan.steps},
                           step_share=seen.share[:n_step_clips], final_share=seen.share[n_step_clips:], halves=seen.halves,
                           fix_mask=agent.fix_mask[0] if torch.is_tensor(agent.fix_mask) else None)


@functools.lru_cache(maxsize=None)
def reference(name, executor="mlp"):
    """The float64 CPU run of case `name` with the net of `executor`: computed once per process and never modified."""
    return host_run(name, torch.float64, executor)


def sim_run(name, executor, keep_flags=True):
    """The plan of ``reference(name, executor)`` through ``oracle.step_sim.run_plan`` -- the record interpreter -- in float64 on the same
    net, inputs and draws; `keep_flags` False clears every record's flags (CDX_STEP_MASK_PRED) first.  For cases without a clamp."""
    import dataclasses
    from oracle import step_sim
    r = reference(name, executor)
    assert r.env[0] == 0
    net = build(name, executor, "cpu", torch.float64, r.case).model_ema["diffusion"]
    plan = r.plan if keep_flags else dataclasses.replace(r.plan, steps=[dataclasses.replace(st, flags=0) for st in r.plan.steps])
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()          # noqa: E731
    return step_sim.run_plan(plan, net, r.xt, predict_noise=r.predict_noise, prior=t64(r.inp["prior"]),
                             fix_mask=r.fix_mask, noise=list(t64(r.inp["noise"])[1:]), cond=r.cond, w_cfg=r.w_cfg)


# ------------------------------------------------------------------------------------------------ #
# the one large case                                                                                   #
# ------------------------------------------------------------------------------------------------ #
# launch_step starts at most 4096 workgroups of 256 threads: past 4096 x 256 elements in a chunk the grid-stride loop takes a second
# trip.  300 000 rows of 4 are 1.2 M elements in one chunk (w_cfg = 1: a doubled batch would be split at 262 144 rows = exactly one trip).
LARGE = SimpleNamespace(name="c_ddpm_eps_full", executor="mlp4", batch=300_000)


def large_case():
    case = case_of(LARGE.name, LARGE.executor)
    return SimpleNamespace(**{**vars(case), "w_cfg": 1.0, "sample": dict(case.sample, sample_steps=2)})


def large_rows():
    """The rows the large case is compared on: 4096 at a stride, and the last 64."""
    return torch.cat([torch.arange(4096) * (LARGE.batch // 4096), torch.arange(LARGE.batch - 64, LARGE.batch)])
