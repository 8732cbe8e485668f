"""TEST HELPER for the fused denoising step (engine/denoise.py): the cases, their builders and for each ONE float64 CPU run of the stock
module path (``BaseDiffusionSDE.loss`` / the net's own ``forward``) under torch.autograd -- the reference both tests/test_denoise_cpu.py
and tests/test_gpu_denoise.py compare with.  Computed once per process and never modified."""
import contextlib
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cases as _cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_steps.npz")
STEPS = 5                   # diffusion steps of every case's DiscreteDiffusionSDE


def _c(net, rows, mode, predict_noise=False, mask=False, lw=False, wr=False, cond=True, cond_grad=True, seed=71):
    return SimpleNamespace(net=net, R=rows, mode=mode, predict_noise=predict_noise, mask=mask, lw=lw, wr=wr, cond=cond, cond_grad=cond_grad,
                           seed=seed)


# (class, obs, act, emb, hidden): DVInvMlp reads (obs, next_obs): O = 2 x 7 columns; DQLMlp O = 11, or none at all with condition=None
DV32, DV64, DQL = ("DVInvMlp", 7, 3, 16, 32), ("DVInvMlp", 7, 6, 16, 64), ("DQLMlp", 11, 6, 16, None)

CASES = {
    # loss mode: rows 1 / 16 / 17 / 33, both targets, mask x loss weight x weighted-regression rows
    "dv32_r1_x0": _c(DV32, 1, "loss"),
    "dv32_r16_eps_mask_lw_wr": _c(DV32, 16, "loss", predict_noise=True, mask=True, lw=True, wr=True, seed=72),
    "dv64_r17_x0_mask_wr": _c(DV64, 17, "loss", mask=True, wr=True, seed=73),
    "dv64_r33_eps_lw": _c(DV64, 33, "loss", predict_noise=True, lw=True, seed=74),
    "dql_r33_x0_mask_lw_wr": _c(DQL, 33, "loss", mask=True, lw=True, wr=True, seed=75),
    "dql_r17_eps_nocond": _c(DQL, 17, "loss", predict_noise=True, cond=False, seed=76),
    # prediction mode: with and without a gradient wanted for the condition
    "dv32_r17_pred": _c(DV32, 17, "pred", seed=77),
    "dv64_r33_pred_nocondgrad": _c(DV64, 33, "pred", cond_grad=False, seed=78),
    "dql_r16_pred_nocond": _c(DQL, 16, "pred", cond=False, seed=79),
}
LOSS_CASES = [n for n, c in CASES.items() if c.mode == "loss"]          # (the cases tests/golden/denoise_steps.npz holds a record of)

# the edges of what dn_check admits (A <= 64, 2 E <= 512, A + E + O <= 512, W <= 512), on the nets of rollout_cases.ENVELOPE and one at E = 256
DV512, DV272, DV48A33, KITCHEN = ("DVInvMlp", 160, 64, 128, 512), ("DVInvMlp", 60, 17, 16, 272), ("DVInvMlp", 5, 33, 16, 48), ("DQLMlp", 60, 9, 16, None)
ENVELOPE = {
    # every limit at once (F = 512, W = 512: 68 KiB of LDS), with everything the loss can carry
    "limits_r17_a64_f512_w512_eps_mask_lw_wr": _c(DV512, 17, "loss", predict_noise=True, mask=True, lw=True, wr=True, seed=91),
    # a partial second sweep (272 = 17 column tiles), A = 17, F = 153: ten K blocks through the scalar weight loads
    "dv272_r33_a17_x0": _c(DV272, 33, "loss", seed=92),
    # A = 33: three trips of the element loops, a ragged third head tile, with a gradient for the condition and for xt
    "dv48_r17_a33_pred": _c(DV48A33, 17, "pred", seed=93),
    # the kitchen policy (obs 60, act 9): F = 85, W = 256
    "kitchen_dql_r33_eps_lw": _c(KITCHEN, 33, "loss", predict_noise=True, lw=True, seed=94),
    "kitchen_dql_r17_pred": _c(KITCHEN, 17, "pred", seed=95),
    # the widest time MLP: 2 E = 512 (its hidden layer is an MFMA A operand of two sweeps), F = 267
    "dv32_r17_e256_x0_mask": _c(("DVInvMlp", 4, 3, 256, 32), 17, "loss", mask=True, seed=96),
}
CASES.update(ENVELOPE)
TABLE = list(CASES)
PARAMS = [f"{m}.{leaf}" for m in ("time_mlp.0", "time_mlp.2", "mid_layer.0", "mid_layer.2", "mid_layer.4", "final_layer") for leaf in ("weight", "bias")]


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def dims(case):
    cls, obs, act, emb, hidden = case.net
    return act, emb, (obs if cls == "DQLMlp" else 2 * obs), (256 if hidden is None else hidden)


def build(case, lib, device="cpu", dtype=torch.float32):
    """(agent, inputs) of a case on `device`: synthetic weights, IdentityCondition without dropout, seeded inputs and draws."""
    from cleandiffuser_amd.utils import load_synth
    cls, obs, act, emb, hidden = case.net
    net = load_synth(lib.DQLMlp(obs, act, emb_dim=emb) if cls == "DQLMlp" else lib.DVInvMlp(obs, act, emb_dim=emb, hidden_dim=hidden), case.seed)
    net = net.to(device=device, dtype=dtype)
    fm = lw = None
    if case.mask:
        fm = torch.zeros(act, dtype=dtype)
        fm[act - 1] = 1.0
    if case.lw:
        lw = torch.linspace(0.5, 2.0, act, dtype=torch.float64).to(dtype)
    agent = lib.DiscreteDiffusionSDE(net, lib.IdentityCondition(dropout=0.0), fix_mask=fm, loss_weight=lw, predict_noise=case.predict_noise,
                                     x_max=torch.ones(1, act, dtype=dtype), x_min=-torch.ones(1, act, dtype=dtype), diffusion_steps=STEPS,
                                     device=device)
    return agent, inputs(case, device, dtype)


def inputs(case, device="cpu", dtype=torch.float32, recorded=None):
    """The case's seeded inputs; `recorded`: {"t", "eps"} of a fixture in place of the case's own draws."""
    act, _, o, _ = dims(case)
    g = torch.Generator().manual_seed(1000 + case.seed)
    r64 = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    to = lambda v: v.to(device=device, dtype=dtype)                             # noqa: E731
    inp = SimpleNamespace(x0=to(r64(case.R, act)), obs=to(r64(case.R, o)) if case.cond else None,
                          t=torch.randint(STEPS, (case.R,), generator=g).to(device), eps=to(r64(case.R, act)),
                          wr=to(0.5 + torch.rand(case.R, generator=g, dtype=torch.float64)) if case.wr else None, q_w=to(r64(case.R, act)))
    if recorded is not None:
        inp.t, inp.eps = torch.as_tensor(recorded["t"]).to(device), to(torch.as_tensor(recorded["eps"]))
    return inp


@contextlib.contextmanager
def recorded_draws(agent, inp):
    """``agent.add_noise`` / ``agent.loss`` draw the case's recorded t and eps whatever route serves them."""
    draws = agent._noise_draws
    agent._noise_draws = lambda x0, t=None, eps=None: (inp.t if t is None else t, inp.eps if eps is None else eps)
    try:
        yield
    finally:
        agent._noise_draws = draws


def loss_kwargs(inp):
    return {} if inp.wr is None else {"weighted_regression_tensor": inp.wr}


def noised(agent, inp):
    """xt of prediction mode: the noised action without a mask, as EDP forms it."""
    return agent.alpha[inp.t][:, None] * inp.x0 + agent.sigma[inp.t][:, None] * inp.eps


def objective(pred, inp):
    return (pred * inp.q_w).sum()


def run(agent, case, inp, route=None):
    """One differentiated evaluation of the case on `agent`: -> (value, obs with its gradient or None, xt with its gradient or None).
    `route`: the callable that evaluates the net in prediction mode (default: the module call)."""
    obs = None if inp.obs is None else inp.obs.clone().requires_grad_(case.cond_grad)
    if case.mode == "loss":
        with recorded_draws(agent, inp):
            loss = agent.loss(inp.x0, obs, **loss_kwargs(inp))
        loss.backward()
        return loss.detach(), obs, None
    xt = noised(agent, inp).detach().requires_grad_(True)
    net = agent.model["diffusion"]
    cond = None if obs is None else agent.model["condition"](obs, None)
    pred = (route or (lambda n, x, t, c: n(x, t, c)))(net, xt, inp.t, cond)
    assert pred is not None, "the route did not take this request"
    objective(pred, inp).backward()
    return pred.detach(), obs, xt


@functools.lru_cache(maxsize=None)
def reference(name, recorded=False):
    """The float64 CPU run of case `name` through the stock module path under torch.autograd -> namespace with the value (the loss, or
    pred (R, A)), pred, every parameter gradient, d / d obs and d / d xt (each None where the case has none).  `recorded`: with the t and
    eps of the fixture."""
    case = CASES[name]
    lib = _cases.lib_namespace("amd")
    with float64_default():
        agent, inp = build(case, lib, "cpu", torch.float64)
        if recorded:
            inp = inputs(case, "cpu", torch.float64, golden(name))
        agent.model.zero_grad(set_to_none=True)
        value, obs, xt = run(agent, case, inp)
        net = agent.model["diffusion"]
        grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        with torch.no_grad():
            x_in = agent.add_noise(inp.x0, inp.t, inp.eps)[0] if case.mode == "loss" else noised(agent, inp)
            pred = net(x_in, inp.t, inp.obs)
    return SimpleNamespace(case=case, value=value, pred=pred, grads=grads, g_obs=None if obs is None else obs.grad,
                           g_xt=None if xt is None else xt.grad)


def request(agent, case, inp, want=("g_cond", "g_emb0", "g_xt")):
    """The kernels' request for this evaluation (any dtype / device), backward buffers allocated; the incoming gradient is the loss's 1
    or the objective's q_w."""
    from cleandiffuser_amd.engine import denoise
    net = agent.model["diffusion"]
    weights = [p.detach() for m in (net.time_mlp[0], net.time_mlp[2], net.mid_layer[0], net.mid_layer[2], net.mid_layer[4], net.final_layer)
               for p in (m.weight, m.bias)]
    with torch.no_grad():
        emb0 = net.map_noise(inp.t).to(inp.x0.dtype).contiguous()
    flat = lambda v: v.reshape(-1).contiguous() if torch.is_tensor(v) else None     # noqa: E731
    if case.mode == "loss":
        q = denoise.make_request(weights, emb0, inp.obs, x0=inp.x0, eps=inp.eps, a=agent.alpha[inp.t].to(inp.x0.dtype).contiguous(),
                                 s=agent.sigma[inp.t].to(inp.x0.dtype).contiguous(), fix_mask=flat(agent.fix_mask), lw=flat(agent.loss_weight),
                                 wr=inp.wr, predict_noise=case.predict_noise, loss_mode=True)
        q.g_loss = torch.ones(1, device=emb0.device, dtype=emb0.dtype)
    else:
        q = denoise.make_request(weights, emb0, inp.obs, xt=noised(agent, inp).contiguous(), loss_mode=False)
        q.g_pred = inp.q_w.contiguous()
    q.G_head, q.G_t2 = torch.empty_like(q.pred), torch.empty_like(emb0)
    q.g_cond = torch.empty_like(inp.obs) if (inp.obs is not None and "g_cond" in want) else None
    q.g_emb0 = torch.empty_like(emb0) if "g_emb0" in want else None
    q.g_xt = torch.empty_like(q.pred) if "g_xt" in want else None
    return q


@functools.lru_cache(maxsize=None)
def golden(name):
    """The record of the real reference for a loss case (tools/gen_denoise_step_golden.py): {"t", "eps", "loss", "grad/<parameter>"}."""
    with np.load(GOLDEN) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
