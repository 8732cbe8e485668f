"""The cases the candidate-selection tests share (engine/select.py, utils/selection.py, csrc/cdx_select.hip): the shipped critics at hidden
width 32 or 48, so a case takes milliseconds, and the ENVELOPE group at the edges of the sizes the kernels admit (up to K0 = 512, a
512-wide layer and K = 1024 candidates; still one to 128 tiles).  Every case builds its critic and inputs from its seed; the seeds were chosen on the CPU
(``decision_margin`` / ``sample_margin`` below) so that every decision of every state keeps the margin its test asserts."""
from types import SimpleNamespace

import torch
import torch.nn as nn

TEMPERATURES = (1.0, 20.0, 300.0)       # the range of the shipped weight_temperature / alpha / beta values
E2E_TEMPERATURE = 20.0


def _c(S, K, O, A, kind, hidden, seed):
    return SimpleNamespace(S=S, K=K, O=O, A=A, kind=kind, hidden=hidden, seed=seed)


CASES = {
    "dql_s3_k16": _c(3, 16, 7, 3, "dql", 32, 0),                 # the one-launch path
    "twinq_s2_k17": _c(2, 17, 11, 3, "twinq", 48, 0),            # a ragged last tile of 1 row, two launches
    "dql_s3_k50": _c(3, 50, 7, 3, "dql", 32, 1),                 # a ragged last tile of 2 rows
    "twinq_s1_k1": _c(1, 1, 11, 3, "twinq", 32, 0),              # one row
    "dql_s5_k5": _c(5, 5, 7, 3, "dql", 32, 0),                   # a tile that is mostly dead rows
    "mlp_s2_k256": _c(2, 256, 17, 6, "mlp", 48, 2),              # 16 tiles per state, a single tower without a norm (SfBC's Mlp, SiLU)
    "mlp_noobs_s2_k40": _c(2, 40, 0, 6, "mlp", 32, 0),           # no observation block
    "twinq_s2_k33_k021": _c(2, 33, 17, 4, "twinq", 32, 0),       # O + A = 21: scalar weight loads, zero padding of the image
}
# the edges of what score_plan / select_check admit (A <= 64, O + A <= 512, widths <= 512, K <= 1024, top_k <= 16, LDS <= 160 KiB); `hidden`
# as a list: the hidden widths of the Mlp
ENVELOPE = {
    "kitchen_dql_s2_k50": _c(2, 50, 60, 9, "dql", 256, 0),              # the kitchen DQLCritic: K0 = 69, five K blocks, scalar weight loads
    "twinq_s2_k17_o448_a64": _c(2, 17, 448, 64, "twinq", 32, 0),        # O + A = 512, A = 64: the widest image, 32 K blocks
    "mlp_s2_k1024": _c(2, 1024, 17, 6, "mlp", 48, 8),                   # 64 tiles per state; all 16 `taken` bits of a lane in the reduction
    "mlp_s2_k17_k0512_w512": _c(2, 17, 448, 64, "mlp", [512], 0),       # the widest critic: K0 = 512 into one 512-wide layer, 96 KiB of LDS
    "dql_s2_k16_w272_k085": _c(2, 16, 76, 9, "dql", 272, 0),            # a partial second sweep (272 = 17 column tiles) on the one-launch path
}
CASES.update(ENVELOPE)
TABLE = list(CASES)


def build_critic(case, dtype=torch.float32, device="cpu"):
    """The stock module of the case (``DQLCritic`` / ``TwinQ`` / ``Mlp``) with weights drawn from the case's seed: pre-norm rows differ
    in spread, gains and shifts are not trivial."""
    from cleandiffuser_amd.utils import DQLCritic, TwinQ
    from cleandiffuser_amd.utils.blocks import Mlp
    if case.kind == "dql":
        m = DQLCritic(case.O, case.A, hidden_dim=case.hidden)
    elif case.kind == "twinq":
        m = TwinQ(case.O, case.A, hidden_dim=case.hidden)
    else:
        m = Mlp(case.O + case.A, case.hidden if isinstance(case.hidden, list) else [case.hidden, case.hidden], 1, nn.SiLU())
    g = torch.Generator().manual_seed(1000 + case.seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Linear):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (1.5 / mod.in_features ** 0.5))
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.3)
            elif isinstance(mod, nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    return m.to(device=device, dtype=dtype).requires_grad_(False).eval()


def make_inputs(case):
    """(obs (S, O) | None, cand (S * K, A), u (S,)) in float32 on the CPU."""
    g = torch.Generator().manual_seed(2000 + case.seed)
    obs = torch.randn(case.S, case.O, generator=g) if case.O else None
    cand = torch.randn(case.S * case.K, case.A, generator=g).tanh()
    return obs, cand, torch.rand(case.S, generator=g)


def request(E, case, critic, obs, cand, mode, temperature, top_k=1, u=None, want_weights=True, scores=None):
    """The request of a case: with the critic inside, or over given `scores`."""
    from cleandiffuser_amd.utils.selection import _towers
    if scores is not None:
        return E.make_request(case.S, case.K, mode, temperature, top_k, u, scores=scores, payload=cand, want_weights=want_weights)
    descs = E.describe_critic(_towers(critic), case.O, case.A)
    assert descs is not None, "the case's critic is one the kernel takes"
    params = [[p.detach() for p in E.tower.params_of(d)] for d in descs]
    return E.make_request(case.S, case.K, mode, temperature, top_k, u, payload=cand, want_weights=want_weights,
                          critic=(descs[0], params), obs=obs, cand=cand)


def inverse_cdf(w, u):
    """The draw the call makes in place of ``torch.multinomial(w, 1)``: the smallest k whose running sum exceeds u, else the last."""
    K = w.shape[1]
    ks = torch.arange(K, device=w.device).expand_as(w)
    return torch.where(torch.cumsum(w, 1) > u.to(w.dtype)[:, None], ks, torch.full_like(ks, K - 1)).min(1).values


def pipeline_expression(critic, obs, cand, K, mode, temperature, top_k=1, u=None, v_net=None):
    """What the reference's pipelines write behind ``sample()``, with the repository's stock modules: the observation repeated K times,
    the critic on the rows, then (idql_d4rl_mujoco.py:181-194, dql_d4rl_mujoco.py:192-200) softmax and a draw -- by inverse CDF from `u`
    in place of ``torch.multinomial`` --, (sfbc_d4rl_mujoco.py:192-196) argsort, gather and the mean of the top rows,
    (veteran_d4rl_mujoco.py:440-446) argmax and an index, (qgpo_d4rl_mujoco.py:141-144) the softmax-weighted value.
    -> dict(scores (S, K), weights, value, index, picked)."""
    from cleandiffuser_amd.utils import DQLCritic, TwinQ
    A = cand.shape[-1]
    S = cand.shape[0] // K
    rows = None if obs is None else obs.unsqueeze(1).repeat(1, K, 1).view(-1, obs.shape[-1])
    if isinstance(critic, DQLCritic):
        q = critic.q_min(rows, cand)
    elif isinstance(critic, TwinQ):
        q = critic(rows, cand)
    else:
        q = critic(cand if rows is None else torch.cat([rows, cand], dim=-1))
    scores = q.view(-1, K, 1)
    adv = scores if v_net is None else (q - v_net(rows)).view(-1, K, 1)
    w = torch.softmax(adv * temperature, 1)
    out = dict(scores=scores[..., 0], weights=w[..., 0], value=(scores * w).sum(1)[:, 0], index=None, picked=None)
    act = cand.view(-1, K, A)
    if mode == "sample":
        p = w / w.sum(1, keepdim=True)
        out["index"] = inverse_cdf(p.squeeze(-1), u)
        out["picked"] = act[torch.arange(act.shape[0]), out["index"]]
    elif mode == "argmax":
        out["index"] = torch.argmax(scores[..., 0], -1)
        out["picked"] = act[torch.arange(S), out["index"]]
    elif mode == "topk_mean":
        sorted_indices = torch.argsort(scores[..., 0], dim=1, descending=True)
        out["index"] = sorted_indices[:, :top_k]
        out["picked"] = act.gather(1, sorted_indices.unsqueeze(-1).expand(-1, -1, act.size(-1)))[:, :top_k].mean(1)
    return out


def sample_margin(scores, temperature, u) -> float:
    """min over states and k of |running sum of softmax(temperature * scores) - u| in float64."""
    c = torch.cumsum(torch.softmax(temperature * scores.double(), 1), 1)
    return float((c - u.double()[:, None]).abs().min())


def decision_margin(scores, mode, temperature, top_k, u) -> float:
    """The smallest margin of a decision over every state in float64: first against second score ("argmax"), rank top_k against rank
    top_k + 1 ("topk_mean"), the running sum against u ("sample")."""
    s = torch.sort(scores.double(), dim=1, descending=True).values
    if mode == "sample":
        return sample_margin(scores, temperature, u)
    if mode == "argmax":
        return float((s[:, 0] - s[:, 1]).min()) if s.shape[1] > 1 else float("inf")
    n = min(top_k + 1, s.shape[1])                  # (the index is compared in rank order: every gap down to rank top_k + 1 counts)
    return float((s[:, :n - 1] - s[:, 1:n]).min()) if n > 1 else float("inf")


def tie_case():
    """Given scores with exact ties: S = 3, K = 20, top_k = 4, and a payload of P = 5 columns inside rows of 9 floats."""
    g = torch.Generator().manual_seed(5)
    S, K = 3, 20
    scores = torch.randint(0, 4, (S * K,), generator=g).float() / 2
    wide = torch.randn(S * K, 9, generator=g)
    return SimpleNamespace(S=S, K=K, top_k=4, scores=scores, wide=wide, cols=slice(2, 7))


def c_request(E, O=7, A=3, widths=(16, 1), S=4, K=5, **sel):
    """A ``CdxScoreSelect`` of sizes alone (every pointer null unless `sel` gives one): what the C side's size checks and LDS plan read."""
    g = E.CdxScoreSelect(O=O, A=A, n_towers=1, n_layers=len(widths))
    g.sel = E.CdxSelect(S=S, K=K, temperature=1.0, **sel)
    for l, w in enumerate(widths[:E.tower.MAX_LAYERS]):
        g.width[l], g.eps[l] = w, 1e-5
    return g
