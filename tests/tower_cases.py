"""The towers the critic-tower tests share (engine/tower.py, csrc/cdx_tower.hip): small on purpose -- no case has more
than 33 rows, the ENVELOPE group at the edges of the admitted sizes (K0 and widths up to 512, a last width up to 64) included.  Every
case builds its ``nn.Sequential`` towers from a seed, scales the input so that tanh and the norm are not in a trivial regime, and says
which side takes a gradient."""
from types import SimpleNamespace

import torch
import torch.nn as nn

ACTS = {"tanh": nn.Tanh, "mish": nn.Mish, "silu": nn.SiLU, "relu": nn.ReLU, None: None}


def _c(rows, k0, widths, acts, norm=True, eps=1e-5, towers=1, frozen=False, x_grad=True, scale=2.0):
    """`acts`: one name per layer (None: no activation); `norm`: one flag per layer or one for all hidden layers (the last layer of a
    critic is a bare Linear: no norm there unless the list says so)."""
    n = len(widths)
    norms = list(norm) if isinstance(norm, (list, tuple)) else [bool(norm)] * (n - 1) + [False]
    return SimpleNamespace(rows=rows, k0=k0, widths=list(widths), acts=list(acts), norms=norms, eps=eps, towers=towers, frozen=frozen,
                           x_grad=x_grad, scale=scale)


CASES = {
    # rows 1 / 16 / 17 / 33; K0 7 (scalar weight loads) / 20 (a multiple of 4, not of 16) / 32
    "dql_like_r17_k7": _c(17, 7, [32, 32, 32, 1], ["tanh", "mish", "mish", None], towers=2),
    "twinq_like_r16_k20": _c(16, 20, [48, 48, 1], ["mish", "mish", None], towers=2),
    "v_like_r1_k32": _c(1, 32, [32, 32, 1], ["mish", "mish", None]),
    "unequal_r33": _c(33, 20, [32, 48, 16, 3], ["silu", "relu", None, None], norm=[True, False, True, False], eps=1e-3),
    "wide512_r33": _c(33, 7, [512, 1], ["tanh", None]),
    "depth1_r17": _c(17, 32, [3], [None], norm=[False]),
    "depth2_plain_r16": _c(16, 7, [16, 1], ["relu", None], norm=False),
    "depth6_r17": _c(17, 20, [16, 32, 16, 32, 16, 3], ["mish", "silu", "tanh", None, "relu", "tanh"], norm=[True, False, True, True, False, True]),
    "frozen_x_grad": _c(17, 7, [32, 32, 32, 1], ["tanh", "mish", "mish", None], towers=2, frozen=True, x_grad=True),
    "trainable_no_x_grad": _c(33, 20, [48, 48, 1], ["mish", "mish", None], towers=2, x_grad=False),
}
# the edges of what tower_plan / tw_check_layers admit (K0 <= 512, widths <= 512, last width <= 64, LDS <= 160 KiB)
ENVELOPE = {
    # every limit at once: 64.5 KiB of LDS, both sweeps of the product in every layer, a 4-tile last layer, 32 K blocks
    "limits_r17_k512": _c(17, 512, [512, 512, 64], ["mish", "tanh", None], towers=2),
    # the kitchen DQLCritic (obs 60 + act 9): five K blocks with a ragged end through the scalar weight loads
    "kitchen_r33_k69": _c(33, 69, [256, 256, 256, 1], ["tanh", "mish", "mish", None], towers=2),
    # a last layer of 33 columns (three column tiles, zero up to 48 for the transposed product) behind a normed first layer
    "wide_last_r17_k33": _c(17, 33, [48, 33], ["mish", None], norm=[True, False]),
    # the same with the norm and an activation on the wide last layer itself
    "wide_last_norm_r17_k33": _c(17, 33, [48, 33], ["mish", "tanh"], norm=[True, True]),
    # the smallest input
    "k1_r16": _c(16, 1, [16, 1], ["mish", None]),
    # a partial second sweep (272 = 17 column tiles) over K0 = 85 (F of the kitchen DQLMlp: six K blocks, ragged)
    "sweep272_r17_k85": _c(17, 85, [272, 272, 17], ["silu", "mish", None]),
}
CASES.update(ENVELOPE)
TABLE = list(CASES)


def build(case, seed=3, dtype=torch.float32, device="cpu"):
    """The towers of a case as stock ``nn.Sequential`` modules: weights, gains and shifts drawn so that pre-norm rows differ in spread
    and |y| exceeds 1."""
    g = torch.Generator().manual_seed(seed)
    towers = []
    for _ in range(case.towers):
        mods, k = [], case.k0
        for w, act, norm in zip(case.widths, case.acts, case.norms):
            lin = nn.Linear(k, w)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(w, k, generator=g) * (1.5 / k ** 0.5))
                lin.bias.copy_(torch.randn(w, generator=g) * 0.3)
            mods.append(lin)
            if norm:
                ln = nn.LayerNorm(w, eps=case.eps)
                with torch.no_grad():
                    ln.weight.copy_(1.0 + 0.5 * torch.randn(w, generator=g))
                    ln.bias.copy_(0.3 * torch.randn(w, generator=g))
                mods.append(ln)
            if ACTS[act] is not None:
                mods.append(ACTS[act]())
            k = w
        seq = nn.Sequential(*mods).to(device=device, dtype=dtype)
        seq.requires_grad_(not case.frozen)
        towers.append(seq)
    return towers


def make_inputs(case, seed=11):
    """x (rows, K0) with a per-row scale between 0.2 and `scale` (the rows' rstd spreads), g_out per tower (rows, width[-1]) / rows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case.rows, case.k0, generator=g) * (0.2 + (case.scale - 0.2) * torch.rand(case.rows, 1, generator=g))
    g_out = [torch.randn(case.rows, case.widths[-1], generator=g) / case.rows for _ in range(case.towers)]
    return x, g_out


def request(tower, towers, x):
    """The request object of engine/tower.py for these towers on `x`'s device and dtype."""
    descs = [tower.describe(s) for s in towers]
    assert all(d is not None for d in descs)
    q = tower.make_request(descs[0], [[p.detach() for p in tower.params_of(d)] for d in descs], x, save=True)
    q.descs = descs
    return q


def check_regime(tower, case):
    """The case table's own claim: across rows the rstd of the first norm spreads (max / min > 1.5 when it sees more than one row: the
    later norms read rows an earlier one has already scaled) and |y| exceeds 1 somewhere before an activation."""
    towers = build(case, dtype=torch.float64)
    x, _ = make_inputs(case)
    q = request(tower, towers, x.double())
    tower.reference_forward(q)
    big, first = False, True
    for l, norm in enumerate(case.norms):
        if norm:
            big = big or float((q.P[0][l] * q.gamma[0][l] + q.beta[0][l]).abs().max()) > 1.0
            if case.rows > 1 and first:
                assert float(q.rstd[0][l].max() / q.rstd[0][l].min()) > 1.5, (l, q.rstd[0][l])
            first = False
        else:
            big = big or float(q.P[0][l].abs().max()) > 1.0
    assert big


def c_request(tower, k0, widths, norms=None, acts=None, **kw):
    """A ``CdxTower`` of sizes alone (every pointer null): what the C side's size checks and LDS plan read."""
    g = tower.CdxTower(R=4, K0=k0, n_towers=1, n_layers=len(widths), **kw)
    for l, w in enumerate(widths):
        g.width[l], g.norm[l], g.act[l], g.eps[l] = w, int(norms[l]) if norms else 0, acts[l] if acts else 0, 1e-5
    return g


def repoint_off_alignment(module):
    """Every nn.Linear weight of `module` becomes a view at element offset 1 of a flat fp32 buffer of its own: contiguous, same values,
    and a base address that is 4 bytes past a 16-byte boundary."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            flat = torch.empty(m.weight.numel() + 1, device=m.weight.device, dtype=m.weight.dtype)
            view = flat[1:].view(m.weight.shape)
            view.copy_(m.weight.detach())
            m.weight.data = view
            assert m.weight.is_contiguous() and m.weight.data_ptr() % 16 == 4
