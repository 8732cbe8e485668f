"""TEST HELPER for the energy-guided loop (engine/energy.py): the cases of tests/golden/qgpo_guided.npz, the agents they build from either
library (``oracle.cases.lib_namespace("reference" | "amd")``), and for each case ONE float64 CPU run of the package's own host loop -- the
reference the CPU tests compare ``reference_run`` with.  tools/gen_qgpo_golden.py runs the real reference on the same table.

Every case is ``agent.sample(prior, solver, n_samples=B, sample_steps=S, sample_step_schedule=..., condition_cfg=obs, w_cfg, condition_cg=obs,
w_cg)`` of an SfBCUNet under a diffusion SDE with a QGPOClassifier(QGPONNClassifier): the call of reference pipelines/qgpo_d4rl_mujoco.py:244-249.
Weights are ``load_synth`` streams; the denoiser's out layer is scaled by `den_scale`, the bounds are +-`bound` and x_T = `temperature` z,
chosen per solver so that the reference's own run meets the three conditions the generator asserts (not everything at a bound, a visible
guidance shift, a clamp that is neither idle nor everywhere)."""
import contextlib
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cases as _cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qgpo_guided.npz")

SMALL = dict(A=3, O=7, emb=32, hidden=[64, 48, 32], clf_emb=32, clf_hidden=[48, 48], clf_time="positional", S=5, B=21)
# the shipped widths: SfBCUNet(act_dim) default (emb 64, hidden 512 / 256 / 128), QGPONNClassifier(obs, act, 64, [256] * 3, fourier)
SHIPPED = dict(A=6, O=17, emb=64, hidden=[512, 256, 128], clf_emb=64, clf_hidden=[256, 256, 256], clf_time="untrainable_fourier", S=10, B=50)


def _c(sde="ContinuousDiffusionSDE", solver="ddpm", predict_noise=True, bound=2.5, den_scale=0.1, w_cfg=1.0, w_cg=5.0, mask=False,
       temperature=1.0, base=SMALL, **over):
    return SimpleNamespace(**{**base, **over}, sde=sde, solver=solver, predict_noise=predict_noise, bound=bound, den_scale=den_scale,
                           w_cfg=w_cfg, w_cg=w_cg, mask=mask, temperature=temperature)


# eps-prediction: a synthetic denoiser's eps is unrelated to x, so x0 = (x - sigma eps) / alpha is clamped in nearly every element unless
# eps is small (den_scale 0.1) and the bounds leave room (+-2.5); the deterministic solvers never leave a bound once clamped to it, so
# they start from a small x_T (temperature 0.02: x_T / alpha_T is of the bounds' size).  x0-prediction: the out layer as it is, +-1.
_DET = dict(temperature=0.02, w_cg=1.0)
_X0 = dict(predict_noise=False, bound=1.0, den_scale=1.0)


CASES = {
    # the continuous SDE x the four one-step solver families, eps-prediction
    "c_ddpm_eps": _c(),
    "c_ddim_eps": _c(solver="ddim", **_DET),
    "c_odepp1_eps": _c(solver="ode_dpmsolver++_1", **_DET),
    "c_sdepp1_eps": _c(solver="sde_dpmsolver++_1"),
    # the discrete SDE
    "d_ddpm_eps": _c(sde="DiscreteDiffusionSDE"),
    # x0-prediction
    "c_ddpm_x0": _c(**_X0),
    "c_odepp1_x0": _c(solver="ode_dpmsolver++_1", **_X0),
    # a fix-mask on the last action column, no classifier-free condition, one full tile, one row
    "c_ddpm_eps_mask": _c(mask=True),
    "c_ddpm_eps_nocfg": _c(w_cfg=0.0),
    "c_ddpm_eps_b16": _c(B=16),
    "c_ddpm_eps_b1": _c(B=1),
    # the shipped widths: the full-size LDS plan
    "shipped_b50": _c(base=SHIPPED),
}
GOLDEN_TABLE = list(CASES)         # the cases tests/golden/qgpo_guided.npz holds a record of

# the edges of what en_plan / em_plan admit (A <= 64, O <= 512, E, Ec <= 128, widths <= 512, a concat input <= 1024, LDS <= 160 KiB): no
# record of the real reference, held to the float64 host loop on the CPU and to the float64 restatement on the device
ENVELOPE = {
    # the kitchen pipeline (obs 60, act 9) at the shipped widths
    "kitchen_b17": _c(base=SHIPPED, O=60, A=9, S=3, B=17),
    # A = 33 under a mask: three trips of the element loops, three column tiles in the out layer and in act_proj's transpose
    "a33_b17_mask": _c(A=33, S=3, B=17, mask=True),
    # a concat input of 272 + 272 = 544 columns, a partial second sweep (272 = 17 column tiles), and O = 85: six K blocks with a ragged
    # end through the scalar weight loads of obs_proj
    "concat544_b33_o85": _c(hidden=[32, 272, 272], O=85, S=2, B=33),
    # the limits that fit 160 KiB together: A = 64, O = 512, E = Ec = 128, a 512-wide block in either net (139 KiB)
    "limits_b17": _c(A=64, O=512, emb=128, hidden=[512, 128], clf_emb=128, clf_hidden=[512], clf_time="untrainable_fourier", S=2, B=17),
}
CASES.update(ENVELOPE)
TABLE = list(CASES)
DISCRETE_STEPS = 20


def schedule(case):
    return "quad_continuous" if case.sde == "ContinuousDiffusionSDE" else "uniform"


def build(case, lib, device="cpu", dtype=torch.float32):
    """The agent of a case from `lib` (this package or the real reference), in eval mode, classifier attached."""
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(lib.SfBCUNet(case.A, emb_dim=case.emb, hidden_dims=list(case.hidden)), 71)
    with torch.no_grad():
        net.out_layer.weight.mul_(case.den_scale)
        net.out_layer.bias.mul_(case.den_scale)
    cond = load_synth(lib.MLPCondition(case.O, case.emb, [case.emb], torch.nn.SiLU(), dropout=0.0), 72)
    clf_net = load_synth(lib.QGPONNClassifier(case.O, case.A, case.clf_emb, list(case.clf_hidden), case.clf_time), 73)
    net, cond, clf_net = (m.to(device=device, dtype=dtype) for m in (net, cond, clf_net))
    if dtype != torch.float32:           # (the embeddings are evaluated in the dtype of t, fp32 for continuous times: hand them on as `dtype`)
        for m in (net, clf_net):
            m.map_noise.register_forward_hook(lambda mod, args, out: out.to(dtype))
    clf = lib.QGPOClassifier(clf_net, device=device)
    fm = None
    if case.mask:
        fm = torch.zeros(case.A, dtype=dtype)
        fm[case.A - 1] = 1.0
    extra = {"diffusion_steps": DISCRETE_STEPS} if case.sde == "DiscreteDiffusionSDE" else {}
    agent = getattr(lib, case.sde)(net, cond, fix_mask=fm, classifier=clf, predict_noise=case.predict_noise,
                                   x_max=case.bound * torch.ones(case.A, dtype=dtype), x_min=-case.bound * torch.ones(case.A, dtype=dtype),
                                   device=device, **extra)
    agent.eval()
    clf.eval()
    return agent


def make_inputs(name: str):
    """obs (B, O), prior (B, A), noise (S + 1, B, A) of a case as float32 numpy arrays: seeded draws (what the fixture records)."""
    case = CASES[name]
    g = torch.Generator().manual_seed(1000 + TABLE.index(name))
    obs = torch.randn(case.B, case.O, generator=g)
    prior = 0.3 * torch.randn(case.B, case.A, generator=g)
    noise = torch.randn(case.S + 1, case.B, case.A, generator=g)
    return {"obs": obs.numpy(), "prior": prior.numpy(), "noise": noise.numpy()}


def sample_kwargs(case, obs, w_cg=None):
    return dict(solver=case.solver, n_samples=case.B, sample_steps=case.S, sample_step_schedule=schedule(case),
                temperature=case.temperature, condition_cfg=obs, w_cfg=case.w_cfg, condition_cg=obs, w_cg=case.w_cg if w_cg is None else w_cg)


def golden(name: str):
    """The fixture's arrays of a case: obs, prior, noise (inputs), x, log_p (what the real reference returned)."""
    with np.load(GOLDEN) as z:
        return {k: z[f"{name}/{k}"] for k in ("obs", "prior", "noise", "x", "log_p")}


def sample(agent, case, inp, device="cpu", dtype=torch.float32, **kw):
    """``agent.sample`` of this package on the recorded inputs and draws -> (x, log)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)          # noqa: E731
    return agent.sample(t(inp["prior"]), noise=list(t(inp["noise"])), **{**sample_kwargs(case, t(inp["obs"])), **kw})


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def request(agent, plan, xt, inp, case, trace=True):
    """The kernel's request for the loop the agent runs on these inputs (any dtype / device; the tables by the modules themselves)."""
    from cleandiffuser_amd.engine import energy
    net, clf_net = agent.model_ema["diffusion"], agent.classifier.model_ema
    dev, dtype = xt.device, xt.dtype
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=dev, dtype=dtype)            # noqa: E731
    obs = t(inp["obs"])
    t_dtype = torch.long if plan.t_is_integer else torch.float32                          # (what the host loop feeds map_noise)
    with torch.no_grad():
        t_vec = torch.tensor([st.t for st in plan.steps], dtype=t_dtype, device=dev)
        den_c = net.t_layer(net.map_noise(t_vec))
        clf_temb = torch.cat([clf_net.map_noise(t_vec), clf_net.map_noise(torch.zeros(1, dtype=torch.long, device=dev))], 0).to(dtype)
        cond = agent.model_ema["condition"](obs, None) if case.w_cfg == 1.0 else None
    fm = agent.fix_mask.reshape(-1) if torch.is_tensor(agent.fix_mask) and case.mask else None
    noise = t(inp["noise"])[1:1 + plan.n_noise] if plan.n_noise else None
    return energy.make_request(energy.describe_denoiser(net), energy.describe_classifier(clf_net), den_c, clf_temb, cond, obs, plan.steps,
                               energy.guidance_scale(plan, case.w_cg, agent.predict_noise), agent.predict_noise, True, xt,
                               t(inp["prior"]) if fm is not None else None, fm, agent.x_min.reshape(-1), agent.x_max.reshape(-1), noise,
                               trace=trace)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 CPU run of case `name` on the package's host loop (CDX_ENERGY=0; ``mlp_grad`` leaves the CPU to autograd): x (clipped),
    log_p, the plan and x_T the loop ran on, per step the raw prediction before the shift, the gradient and logp, and the share of
    elements the clamp changed.  Computed once per process and never modified."""
    case = CASES[name]
    inp = make_inputs(name)
    with float64_default(), env(CDX_ENERGY="0"):
        agent = build(case, _cases.lib_namespace("amd"), "cpu", torch.float64)
        seen = SimpleNamespace(plan=None, xt=None, pred=[], grad=[], logp=[], share=[])
        run_plan, clip, cfg, grads = agent._run_plan_torch, agent.clip_prediction, agent.classifier_free_guidance, agent.classifier.gradients

        def spy_plan(plan, xt, *a, **k):
            seen.plan, seen.xt = plan, xt.detach().clone()
            return run_plan(plan, xt, *a, **k)

        def spy_clip(pred, xt, alpha, sigma):
            out = clip(pred, xt, alpha, sigma)
            seen.share.append(float((out != pred).double().mean()))
            return out

        def spy_cfg(*a, **k):
            seen.pred.append(cfg(*a, **k).detach().clone())
            return seen.pred[-1]

        def spy_grads(*a, **k):
            logp, grad = grads(*a, **k)
            seen.logp.append(logp.detach()[:, 0].clone())
            seen.grad.append(grad.detach().clone())
            return logp, grad
        agent._run_plan_torch, agent.clip_prediction, agent.classifier_free_guidance, agent.classifier.gradients = spy_plan, spy_clip, spy_cfg, spy_grads
        x, log = sample(agent, case, inp, dtype=torch.float64)
    return SimpleNamespace(case=case, inp=inp, x=x.detach(), log_p=log["log_p"].detach(), plan=seen.plan, xt=seen.xt,
                           pred=torch.stack(seen.pred), grad=torch.stack(seen.grad), logp=torch.stack(seen.logp), share=list(seen.share))
