"""Value heads the pipelines evaluate on freshly sampled tensors: the candidate re-weighting critics ``DQLCritic`` and
IQL's ``TwinQ`` / ``V``.  Interface / checkpoint contract: reference utils/building_blocks.py:79-147 and utils/iql.py:7-95 (same
attribute names, hence the same ``state_dict`` keys).  Decision Veteran's horizon critic ``DVHorizonCritic`` (building_blocks.py:149-229),
which the veteran_d4rl_* pipelines evaluate on every environment step's candidate plans, is mirrored with a native scoring call
(engine/hcritic.py); it is imported from this module -- ``cleandiffuser_amd.utils`` does not re-export it.
The reference's generic transformer toolkit (``Transformer`` / ``MultiHeadAttention``, building_blocks.py:231-373) is not mirrored.

Execution: every head here is a chain of ``Linear -> [LayerNorm] -> activation`` over rows, so on a ROCm device without
autograd the chain runs through ``engine/heads.py`` (fp32-MFMA GEMM with fused bias/activation epilogue + one fused
LayerNorm/activation launch per layer); with autograd ON (the critics' training steps) a whole tower, or the twin towers of a critic
together, is one forward and one backward row-tile launch (``engine/tower.py``: ``DQLCritic`` by default, ``TwinQ`` / ``V`` with
``CDX_TOWER=1`` -- the measurement of DESIGN.md 3m; ``CDX_TOWER=0`` or a tower it does not take: ``engine/train.py:chain_forward``, the
library nodes the denoisers train on), IQL's two Adam optimisers and its Polyak target update on ``cdx_optim_f32``; on CPU the stock
modules run.  A critic's whole training step -- target, TD expression, forward, loss, backward-data -- is one launch through
``utils/critic_steps.py`` (``td_step`` / ``expectile_step``), which ``IQL.update_V`` / ``update_Q`` call.
"""
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F


def _rows(seq: nn.Sequential, x: torch.Tensor, fused: bool = False) -> torch.Tensor:
    from ..engine import heads, tower, train
    y = tower.try_tower((seq,), x, fused)      # the whole tower on one forward and one backward launch (engine/tower.py)
    if y is not None:
        return y[0]
    if train.supports_chain(seq, x):           # autograd on, ROCm device (the critics' own training steps): library nodes forward and backward
        return train.chain_forward(seq, x)
    y = heads.try_sequential(seq, x)
    return seq(x) if y is None else y


def _twin(seq1: nn.Sequential, seq2: nn.Sequential, x: torch.Tensor, fused: bool = False):
    """(seq1(x), seq2(x)): twin towers over the same rows share their two launches.  `fused`: without being asked (CDX_TOWER=1)?"""
    from ..engine import tower
    y = tower.try_tower((seq1, seq2), x, fused)
    return y if y is not None else (_rows(seq1, x, fused), _rows(seq2, x, fused))


class SoftLowerBound(nn.Module):
    """x -> lb + softplus(x - lb): smooth clamp from below."""

    def __init__(self, lower_bound: float):
        super().__init__()
        self.lower_bound = lower_bound

    def forward(self, x):
        return self.lower_bound + F.softplus(x - self.lower_bound)


class SoftUpperBound(nn.Module):
    """x -> ub - softplus(ub - x): smooth clamp from above."""

    def __init__(self, upper_bound: float):
        super().__init__()
        self.upper_bound = upper_bound

    def forward(self, x):
        return self.upper_bound - F.softplus(self.upper_bound - x)


def _q_tower(in_dim: int, hidden: int, first_act: nn.Module, depth: int) -> nn.Sequential:
    layers, acts = [], [first_act] + [nn.Mish() for _ in range(depth - 1)]
    for i, act in enumerate(acts):
        layers += [nn.Linear(in_dim if i == 0 else hidden, hidden), nn.LayerNorm(hidden), act]
    return nn.Sequential(*layers, nn.Linear(hidden, 1))


class DQLCritic(nn.Module):
    """Double-Q critic of Diffusion-QL: two towers Linear-LN-Tanh, 2x(Linear-LN-Mish), Linear(1)."""

    def __init__(self, obs_dim: int, act_dim: int, hidden_dim: int = 256):
        super().__init__()
        self.q1_model = _q_tower(obs_dim + act_dim, hidden_dim, nn.Tanh(), 3)
        self.q2_model = _q_tower(obs_dim + act_dim, hidden_dim, nn.Tanh(), 3)

    def forward(self, obs, act):
        return _twin(self.q1_model, self.q2_model, torch.cat([obs, act], dim=-1), fused=True)

    def q1(self, obs, act):
        return _rows(self.q1_model, torch.cat([obs, act], dim=-1), fused=True)

    def q_min(self, obs, act):
        return torch.min(*self.forward(obs, act))


class TwinQ(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_dim: int = 256):
        super().__init__()
        self.Q1 = _q_tower(obs_dim + act_dim, hidden_dim, nn.Mish(), 2)
        self.Q2 = _q_tower(obs_dim + act_dim, hidden_dim, nn.Mish(), 2)

    def both(self, obs, act):
        return _twin(self.Q1, self.Q2, torch.cat([obs, act], -1))

    def forward(self, obs, act):
        return torch.min(*self.both(obs, act))


class V(nn.Module):
    def __init__(self, obs_dim, hidden_dim: int = 256):
        super().__init__()
        self.V = _q_tower(obs_dim, hidden_dim, nn.Mish(), 2)

    def forward(self, obs):
        return _rows(self.V, obs)


IDQLQNet = TwinQ
IDQLVNet = V


class DVTransformerBlock(nn.Module):
    """One block of the horizon critic: self-attention and a GELU(tanh) MLP around two LayerNorms without gain or shift.  "post":
    x = norm1(x + attn(x)); x = norm2(x + mlp(x)).  "pre": x = norm1(x); x = x + attn(x); x = x + mlp(norm2(x)) -- the residual stream
    continues from the normalised tensor."""

    def __init__(self, hidden_size: int, n_heads: int, dropout: float = 0.0, norm_type: str = "post"):
        super().__init__()
        self.norm_type = norm_type
        self.norm1 = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.attn = nn.MultiheadAttention(hidden_size, n_heads, dropout, batch_first=True)
        self.norm2 = nn.LayerNorm(hidden_size, elementwise_affine=False, eps=1e-6)
        self.mlp = nn.Sequential(nn.Linear(hidden_size, hidden_size * 4), nn.GELU(approximate="tanh"), nn.Dropout(dropout),
                                 nn.Linear(hidden_size * 4, hidden_size))

    def forward(self, x):
        if self.norm_type == "post":
            x = self.norm1(x + self.attn(x, x, x)[0])
            return self.norm2(x + self.mlp(x))
        if self.norm_type == "pre":
            x = self.norm1(x)
            x = x + self.attn(x, x, x)[0]
            return x + self.mlp(self.norm2(x))
        raise NotImplementedError(f"norm_type {self.norm_type!r}")


class DVHorizonCritic(nn.Module):
    """Decision Veteran's horizon critic: a transformer over the tokens of a plan (b, T, in_dim) whose value (b, 1) is read off token 0.
    ``emb_dim`` is part of the constructor's contract and otherwise unused.  Execution (engine/hcritic.py): without autograd on a ROCm
    device the executor ``cdx_hcritic_run`` where it is switched on, with autograd the library's nodes where they are, else the stock
    modules below (DESIGN.md 3n says which is the default and why)."""

    def __init__(self, in_dim: int, emb_dim: int, d_model: int = 384, n_heads: int = 6, depth: int = 12, dropout: float = 0.0,
                 norm_type: str = "post"):
        super().__init__()
        self.in_dim, self.emb_dim, self.d_model, self.dropout = in_dim, emb_dim, d_model, dropout
        from .embeddings import SinusoidalEmbedding
        self.x_proj = nn.Linear(in_dim, d_model)
        self.pos_emb = SinusoidalEmbedding(d_model)
        self.pos_emb_cache = None
        self.blocks = nn.ModuleList([DVTransformerBlock(d_model, n_heads, dropout, norm_type) for _ in range(depth)])
        self.final_layer = nn.Linear(d_model, 1)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _positions(self, tokens: int, device) -> torch.Tensor:
        if self.pos_emb_cache is None or self.pos_emb_cache.shape[0] != tokens or self.pos_emb_cache.device != device:
            self.pos_emb_cache = self.pos_emb(torch.arange(tokens, device=device))
        return self.pos_emb_cache

    def forward(self, x):
        from ..engine import hcritic
        y = hcritic.try_score(self, x)                 # scoring sampled plans: one executor call
        if y is not None:
            return y
        if hcritic.supports_nodes(self, x):            # the critic's own training step: library nodes forward and backward
            return hcritic.forward_nodes(self, x)
        x = self.x_proj(x) + self._positions(x.shape[1], x.device)[None]
        for block in self.blocks:
            x = block(x)
        return self.final_layer(x)[:, 0, :]


class IQL(nn.Module):
    """Implicit Q-Learning: expectile-regressed V, TD-regressed twin Q with a Polyak target (reference utils/iql.py:40-95)."""

    def __init__(self, obs_dim: int, act_dim: int, tau: float = 0.7, discount: float = 0.99, hidden_dim: int = 256):
        super().__init__()
        self.iql_tau, self.discount = tau, discount
        self.Q = TwinQ(obs_dim, act_dim, hidden_dim)
        self.Q_targ = deepcopy(self.Q).requires_grad_(False).eval()
        self.V = V(obs_dim, hidden_dim)
        # (torch.optim.Adam subclasses: one multi-tensor launch of cdx_optim_f32 per step on a ROCm device, torch's own step elsewhere)
        from ..engine.optim import FusedAdam
        self.optimV = FusedAdam(self.V.parameters(), lr=3e-4)
        self.optimQ = FusedAdam(self.Q.parameters(), lr=3e-4)

    def update_target(self, mu=0.995):
        from ..engine.optim import ema_update_native
        if ema_update_native(self.Q, self.Q_targ, mu):       # targ <- mu * targ + (1 - mu) * q over every pair, one launch
            return
        for p, p_targ in zip(self.Q.parameters(), self.Q_targ.parameters()):
            p_targ.data = mu * p_targ.data + (1 - mu) * p.data

    # (the two steps are utils/critic_steps.py's calls: on a ROCm device one launch each for target, forward, loss and backward-data
    # -- DESIGN.md 3p -- and the eager sequence on the CPU, with CDX_CRITIC_STEP=0 or on a refusal)
    def update_V(self, obs, act):
        from .critic_steps import expectile_step
        return expectile_step(self.V, self.Q_targ, self.optimV, obs, act, tau=self.iql_tau)["loss"].item()

    def update_Q(self, obs, act, rew, obs_next, done):
        from .critic_steps import td_step
        out = td_step(self.Q, self.V, self.optimQ, obs, act, rew, obs_next, done, discount=self.discount)
        self.update_target()
        return out["loss"].item()

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path, device):
        self.load_state_dict(torch.load(path, map_location=device))
