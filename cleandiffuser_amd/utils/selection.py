"""The tail of every value-guided ``sample()`` call -- score K candidates per state with a critic, re-weight, pick -- as one call
(engine/select.py, csrc/cdx_select.hip; DESIGN.md 3o, INTEGRATION.md for the pipelines' before / after lines).

Imported from this module: ``cleandiffuser_amd.utils`` does not re-export it (the arrangement of ``DVHorizonCritic``).

    sel = select_candidates(critic, obs, act, num_candidates, mode="sample", temperature=T)      # IDQL, DQL, EDP
    sel = select_candidates(critic, obs, act, num_candidates, mode="topk_mean", top_k=4)         # SfBC
    sel = select_candidates(q_targ, next_obs, supported_act, K, mode="none", temperature=betaQ, want_weights=True)   # QGPO
    sel = select_by_score(log_p, traj[:, 0, obs_dim:], num_candidates, mode="argmax")            # Diffuser, Decision Veteran

On a ROCm device the critic and the reduction are ONE launch for K <= 16 and two for K > 16, the reduction over given scores one;
``CDX_SELECT=0`` keeps the module-plus-torch route; on the CPU the torch restatement of the kernels runs.  Nothing here carries a
gradient."""
from collections import namedtuple

import torch
import torch.nn as nn

Selection = namedtuple("Selection", "picked index scores weights value")
Selection.__doc__ = """picked (S, P): the chosen payload row ("topk_mean": the mean of the top_k rows), None in mode "none" or without a
payload; index (S,) int32 ("topk_mean": (S, top_k) in rank order), None in mode "none"; scores (S, K); weights (S, K) =
softmax(temperature * scores, 1) with ``want_weights``, else None; value (S,) = (weights * scores).sum(1)."""


def _towers(critic):
    """The Sequentials whose minimum is the critic's score of ``cat([obs, cand], -1)``, or None for a callable the kernels do not
    know."""
    from .blocks import Mlp
    from .critics import DQLCritic, TwinQ
    if isinstance(critic, DQLCritic):
        return critic.q1_model, critic.q2_model
    if isinstance(critic, TwinQ):
        return critic.Q1, critic.Q2
    if isinstance(critic, Mlp):
        return (critic.mlp,)
    if isinstance(critic, nn.Sequential):
        return (critic,)
    return None


def _module_scores(critic, obs, cand, K: int):
    """The pipelines' own expression: the critic as a module on the repeated observation rows -> (S * K)."""
    from .blocks import Mlp
    from .critics import DQLCritic
    rows = None if obs is None else obs.unsqueeze(1).repeat(1, K, 1).reshape(-1, obs.shape[-1])
    if isinstance(critic, DQLCritic):
        out = critic.q_min(rows, cand)
    elif isinstance(critic, (nn.Sequential, Mlp)):          # one input: cat([obs, cand], -1)
        out = critic(cand if rows is None else torch.cat([rows, cand], -1))
    else:                                                   # a TwinQ (its forward is the minimum) or the caller's function
        out = critic(rows, cand)
    return out.detach().reshape(-1)


def _finish(q, S: int, K: int) -> Selection:
    index = None if q.index is None else (q.index if q.mode == "topk_mean" else q.index[:, 0])
    return Selection(q.picked, index, q.scores.view(S, K), q.weights, q.value)


def _uniforms(mode, u, S, generator, device):
    if mode != "sample":
        return None
    if u is None:
        u = torch.rand(S, generator=generator, device=device)
    return u.detach().to(device=device).reshape(S).contiguous()


def _check(S, K, mode, top_k, temperature, payload):
    from ..engine import select as E
    P = 0 if payload is None else payload.shape[-1]
    if not E.within_limits(S, K, mode, top_k, float(temperature), P):
        raise ValueError(f"selection outside the limits of cdx_select_f32: S = {S}, K = {K}, mode = {mode!r}, top_k = {top_k}, "
                         f"temperature = {temperature}, payload width = {P}")


@torch.no_grad()
def select_by_score(scores, payload, num_candidates: int, mode: str = "argmax", temperature: float = 1.0, top_k: int = 1, u=None,
                    generator=None, want_weights: bool = False) -> Selection:
    """The reduction over given scores: `scores` holds S * num_candidates numbers, candidate k of state s at s * num_candidates + k;
    `payload` (the same rows, width P <= 64; a slice such as ``traj[:, 0, obs_dim:]`` is read in place) or None.

    mode "argmax": the first maximum; "sample": the candidate drawn with probability softmax(temperature * scores, 1) by inverse CDF from
    one uniform per state -- `u` (S,) in [0, 1), or drawn here with ``torch.rand(S, generator=generator)`` on the scores' device (the
    distribution of ``torch.multinomial``, not its random stream); "topk_mean": the mean of the payload rows of the top_k <= 16
    scores; "none": weights and value only."""
    from ..engine import select as E
    K = int(num_candidates)
    scores = scores.detach().reshape(-1).contiguous()
    S = scores.numel() // K
    assert S * K == scores.numel(), "scores must hold num_candidates numbers per state"
    _check(S, K, mode, top_k, temperature, payload)
    payload = E.rows_view(payload, S * K)
    u = _uniforms(mode, u, S, generator, scores.device)
    q = E.make_request(S, K, mode, temperature, top_k, u, scores=scores, payload=payload, want_weights=want_weights)
    if S > 0:
        if E.enabled() and E.on_device(scores, payload, u):
            E.run(q)
        else:
            E.reference_run(q)
    return _finish(q, S, K)


@torch.no_grad()
def select_candidates(critic, obs, cand, num_candidates: int, mode: str = "sample", temperature: float = 1.0, top_k: int = 1, u=None,
                      generator=None, payload=None, want_weights: bool = False) -> Selection:
    """Score the num_candidates candidates of every state and pick among them.

    `critic`: a ``DQLCritic`` (its ``q_min``), a ``TwinQ`` (its minimum), an ``nn.Sequential`` or the ``Mlp`` of ``utils`` over
    ``cat([obs, cand], -1)`` (SfBC), or any callable ``(obs_rows, cand_rows) -> (R, 1)``.  `obs`: (S, O), NOT repeated, or None for a
    critic over the candidates alone; `cand`: S * num_candidates rows of width A, candidate k of state s at row s * num_candidates + k;
    `payload`: what to pick rows of (default: `cand`).  Modes, `u` and `generator` as ``select_by_score``.

    IDQL's advantage ``Q(obs, act) - V(obs)`` is not an input: the observation is the same for the K rows of a state, so ``V(obs)`` is
    one constant per softmax row and cancels; pass the ``TwinQ`` alone.  (``Selection.scores`` / ``value`` are then Q, not Q - V.)

    A critic whose towers ``tower.describe`` admits (Linear -> [LayerNorm] -> Mish / SiLU / ReLU / Tanh, A <= 64, O + A <= 512, one
    output) runs inside the call on the un-repeated observations; any other -- a GELU tower, a callable -- runs as a module on the
    repeated rows and only the reduction is the native call."""
    from ..engine import select as E
    K = int(num_candidates)
    cand = cand.detach()
    cand = cand.reshape(-1, cand.shape[-1]).contiguous()
    S = cand.shape[0] // K
    assert S * K == cand.shape[0], "cand must hold num_candidates rows per state"
    obs = None if obs is None else obs.detach().reshape(S, -1).contiguous()
    payload = cand if payload is None else payload
    _check(S, K, mode, top_k, temperature, payload)
    payload = E.rows_view(payload, S * K)
    u = _uniforms(mode, u, S, generator, cand.device)
    seqs = _towers(critic)
    descs = None if seqs is None else E.describe_critic(seqs, 0 if obs is None else obs.shape[1], cand.shape[1])
    native = E.enabled() and S > 0 and E.on_device(cand, obs, payload, u)
    if native and descs is not None:
        params = [[p.detach() for p in E.tower.params_of(d)] for d in descs]
        if E.on_device(cand, *[p for ps in params for p in ps]) and all(p.is_contiguous() for ps in params for p in ps):
            q = E.make_request(S, K, mode, temperature, top_k, u, payload=payload, want_weights=want_weights, critic=(descs[0], params),
                               obs=obs, cand=cand)
            E.run(q)
            return _finish(q, S, K)
    scores = _module_scores(critic, obs, cand, K) if S > 0 else cand.new_empty(0)
    q = E.make_request(S, K, mode, temperature, top_k, u, scores=scores.contiguous(), payload=payload, want_weights=want_weights)
    if S > 0:
        if native and E.on_device(scores):
            E.run(q)
        else:
            E.reference_run(q)
    return _finish(q, S, K)
