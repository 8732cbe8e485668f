"""The critics' fused towers (engine/tower.py) without a GPU: the torch restatements of the two kernels against float64 autograd of the
stock ``nn.Sequential``, the routing decisions of ``try_tower`` and what it hands to autograd, the descriptions of the shipped critics,
the LDS plan, the C layout of the ctypes mirrors and the messages of the C side's validation."""
import ctypes
import itertools
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_cases as tc  # noqa: E402

RTOL64 = 1e-10


def _close(got, want, what, rtol=RTOL64):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= rtol * scale, (what, err, scale)


def _autograd(towers, x, g_out, x_grad):
    """(outputs, g_x | None, per tower the gradients of ``tower.params_of``'s parameters | None) of the stock modules."""
    x = x.clone().requires_grad_(x_grad)
    outs = [s(x) for s in towers]
    leaves = ([x] if x_grad else []) + [p for s in towers for p in s.parameters() if p.requires_grad]
    grads = list(torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, g_out)), leaves))
    g_x = grads.pop(0) if x_grad else None
    return [o.detach() for o in outs], g_x, grads


@pytest.mark.parametrize("name", tc.TABLE)
def test_restatements_equal_float64_autograd(name):
    """``reference_forward`` / ``reference_backward`` in float64 against autograd through the stock ``nn.Sequential`` to 1e-10 relative:
    outputs, g_x and every parameter gradient; the case is in the regime its table claims."""
    from cleandiffuser_amd.engine import tower
    case = tc.CASES[name]
    tc.check_regime(tower, case)
    towers = tc.build(case, dtype=torch.float64)
    x, g_out = (t.double() if torch.is_tensor(t) else [g.double() for g in t] for t in tc.make_inputs(case))
    outs, g_x, grads = _autograd(towers, x, g_out, case.x_grad)
    q = tc.request(tower, towers, x)
    tower.reference_forward(q)
    tower.add_backward(q, g_out, want_gx=case.x_grad, want_params=not case.frozen)
    tower.reference_backward(q)
    for t in range(case.towers):
        _close(q.out[t], outs[t], f"out[{t}]")
    if case.x_grad:
        _close(sum(q.g_x), g_x, "g_x")
    if not case.frozen:
        got = [g for t in range(case.towers) for g in tower.reference_param_grads(q, t)]
        names = [n for s in towers for n, _ in s.named_parameters()]
        assert len(got) == len(grads) == len(names)
        for n, a, b in zip(names, got, grads):
            _close(a, b, n)


def _patch_to_cpu(monkeypatch, tower, served):
    """``try_tower`` as on the device, with the two C calls replaced by the restatements and the two sums by torch."""
    def fwd(q):
        served.append(q)
        tower.reference_forward(q)

    def wsums(jobs):
        for p, q_rows, _, dw, db in jobs:
            dw += p.t() @ q_rows
            if db is not None:
                db += p.sum(0)

    def csums(jobs):
        for src, out in jobs:
            out += src.sum(0)
    monkeypatch.setattr(tower, "_on_device", lambda x, params: True)
    monkeypatch.setattr(tower, "native_forward", fwd)
    monkeypatch.setattr(tower, "native_backward", tower.reference_backward)
    monkeypatch.setattr(tower, "weight_sums", wsums)
    monkeypatch.setattr(tower, "column_sums", csums)
    monkeypatch.delenv("CDX_TOWER", raising=False)
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("name", tc.TABLE)
def test_try_tower_hands_autograd_the_stock_gradients(name, in_place, monkeypatch):
    """The one autograd node (kernels replaced by their restatements) against the stock modules in float32: outputs, the input's
    gradient and every parameter gradient -- returned to autograd, or added into ``.grad`` under ``train.grads_in_place()`` on top of
    what was there."""
    from cleandiffuser_amd.engine import tower, train
    served = []
    _patch_to_cpu(monkeypatch, tower, served)
    case = tc.CASES[name]
    towers, stock = tc.build(case), tc.build(case)
    x, g_out = tc.make_inputs(case)
    x = x.view(1, case.rows, case.k0)                              # (leading dimensions are rows)
    outs0, g_x0, grads0 = _autograd(stock, x, [g.view(1, case.rows, -1) for g in g_out], case.x_grad)
    xa = x.clone().requires_grad_(case.x_grad)
    params = [p for s in towers for p in s.parameters()]
    if in_place:
        for p in params:
            p.grad = torch.ones_like(p)
    outs = tower.try_tower(towers, xa)
    assert outs is not None and len(served) == 1 and served[0].save
    loss = sum((o * g.view(1, case.rows, -1)).sum() for o, g in zip(outs, g_out))
    if in_place:
        with train.grads_in_place(params):
            loss.backward()
    else:
        loss.backward()
    for o, o0 in zip(outs, outs0):
        assert o.shape == o0.shape
        _close(o.detach(), o0, "out", 1e-5)
    if case.x_grad:
        _close(xa.grad, g_x0, "g_x", 1e-5)
    if not case.frozen:
        for p, g0 in zip(params, grads0):
            _close(p.grad - (1.0 if in_place else 0.0), g0, "parameter gradient", 2e-5)
    else:
        assert all(p.grad is None or in_place for p in params)


def _critic_like(k0=7, hidden=32):
    g = torch.Generator().manual_seed(0)
    seq = nn.Sequential(nn.Linear(k0, hidden), nn.LayerNorm(hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.LayerNorm(hidden), nn.Mish(),
                        nn.Linear(hidden, 1))
    return seq, torch.randn(5, k0, generator=g)


def test_every_refusal_returns_none_and_writes_nothing(monkeypatch):
    """Each refusal of the list: ``try_tower`` answers None before the (replaced) kernel is reached, and no ``.grad`` appears."""
    from cleandiffuser_amd.engine import tower
    served = []
    _patch_to_cpu(monkeypatch, tower, served)
    seq, x = _critic_like()
    twin, _ = _critic_like()
    xg = x.clone().requires_grad_(True)

    def refused(seqs, inp):
        before = len(served)
        assert tower.try_tower(seqs, inp) is None
        assert len(served) == before
        assert inp.grad is None and all(p.grad is None for s in seqs for p in s.parameters())
    assert tower.try_tower((seq,), xg) is not None and tower.try_tower((seq, twin), xg) is not None and len(served) == 2
    for var in ("CDX_TOWER", "CDX_TRAIN_NATIVE"):
        monkeypatch.setenv(var, "0")
        refused((seq,), xg)
        monkeypatch.delenv(var)
    before = len(served)                                                                  # a call site that is fused on request only
    assert tower.try_tower((seq,), xg, default=False) is None and len(served) == before
    monkeypatch.setenv("CDX_TOWER", "1")
    assert tower.try_tower((seq,), xg, default=False) is not None and len(served) == before + 1
    monkeypatch.delenv("CDX_TOWER")
    monkeypatch.setattr(tower, "_on_device", lambda x, params: x.is_cuda)
    refused((seq,), xg)                                                                   # not a ROCm device
    monkeypatch.setattr(tower, "_on_device", lambda x, params: True)
    refused((seq,), x.double().requires_grad_(True))                                      # not fp32
    refused((seq.double(),), xg)
    seq.float()
    refused((seq,), torch.zeros(0, 7, requires_grad=True))                                # empty input
    refused((seq,), torch.zeros(5, 8, requires_grad=True))                                # another input width
    for bad in (nn.Sequential(nn.Linear(7, 32), nn.GELU(), nn.Linear(32, 1)),
                nn.Sequential(nn.Linear(7, 32), nn.LayerNorm(32, elementwise_affine=False), nn.Linear(32, 1)),
                nn.Sequential(nn.Linear(7, 32), nn.LayerNorm((1, 32)), nn.Linear(32, 1)),
                nn.Sequential(nn.Linear(7, 32, bias=False), nn.Tanh(), nn.Linear(32, 1)),
                nn.Sequential(nn.Linear(7, 32), nn.Dropout(0.1), nn.Tanh(), nn.Linear(32, 1)).train(),
                nn.Sequential(nn.Linear(7, 32), nn.Tanh(), nn.LayerNorm(32), nn.Linear(32, 1)),      # activation before the norm
                nn.Sequential(nn.Tanh(), nn.Linear(7, 1)),
                nn.Sequential(nn.Linear(7, 24), nn.Tanh(), nn.Linear(24, 1)),                        # a hidden width that is no multiple of 16
                nn.Sequential(nn.Linear(7, 528), nn.Tanh(), nn.Linear(528, 1)),                      # > 512
                nn.Sequential(nn.Linear(7, 32), nn.Tanh(), nn.Linear(32, 65)),                       # last width > 64
                nn.Sequential(nn.Linear(513, 32), nn.Tanh(), nn.Linear(32, 1)),
                nn.Sequential(*[nn.Linear(16, 16) for _ in range(tower.MAX_LAYERS + 1)])):
        assert tower.describe(bad) is None
        k0 = next(m for m in bad.modules() if isinstance(m, nn.Linear)).in_features
        refused((bad,), torch.zeros(3, k0, requires_grad=True))
    other = nn.Sequential(nn.Linear(7, 32), nn.LayerNorm(32), nn.Tanh(), nn.Linear(32, 1))
    assert tower.try_tower((other,), xg) is not None
    refused((seq, other), xg)                                                             # twin towers of unequal shape
    refused((seq, twin, twin), xg)
    # no autograd: the node route's heads.try_sequential unless CDX_TOWER=1 asks for the forward launch, and then up to NOGRAD_MAX_ROWS
    frozen = _critic_like()[0].requires_grad_(False)
    refused((frozen,), x)
    with torch.no_grad():
        refused((seq,), x)
    monkeypatch.setenv("CDX_TOWER", "1")
    n = len(served)
    with torch.no_grad():
        y = tower.try_tower((seq,), x)
    assert y is not None and len(served) == n + 1 and not served[-1].save and not y[0].requires_grad
    torch.testing.assert_close(y[0], seq(x), rtol=1e-5, atol=1e-6)
    monkeypatch.setattr(tower, "NOGRAD_MAX_ROWS", 4)
    refused((frozen,), x)


def test_the_critics_pass_their_towers_in_one_call(monkeypatch):
    """``DQLCritic.forward`` / ``q_min`` pass both towers in one call and ``q1`` one, unasked; ``TwinQ.both`` / ``TwinQ.forward`` / ``V``
    do so with ``CDX_TOWER=1`` -- and land on the stock modules' values and gradients."""
    from cleandiffuser_amd.engine import tower
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V
    served = []
    _patch_to_cpu(monkeypatch, tower, served)
    g = torch.Generator().manual_seed(2)
    obs, act = torch.randn(5, 11, generator=g), torch.randn(5, 3, generator=g)
    c, q, v = DQLCritic(11, 3, hidden_dim=32), TwinQ(11, 3, hidden_dim=32), V(11, hidden_dim=32)
    x = torch.cat([obs, act], -1)
    for call, towers in ((lambda: c(obs, act), 2), (lambda: c.q_min(obs, act), 2), (lambda: c.q1(obs, act), 1)):
        del served[:]
        call()
        assert [s.n_towers for s in served] == [towers]
    torch.testing.assert_close(c.q_min(obs, act), torch.min(c.q1_model(x), c.q2_model(x)), rtol=1e-5, atol=1e-6)
    calls = ((lambda: q.both(obs, act), 2), (lambda: q(obs, act), 2), (lambda: v(obs), 1))
    del served[:]
    for call, _ in calls:
        call()
    assert not served
    monkeypatch.setenv("CDX_TOWER", "1")
    for call, towers in calls:
        del served[:]
        call()
        assert [s.n_towers for s in served] == [towers]
    q.zero_grad()
    q(obs, act).sum().backward()
    got = [p.grad.clone() for p in q.parameters()]
    monkeypatch.setenv("CDX_TOWER", "0")
    q.zero_grad()
    torch.min(q.Q1(x), q.Q2(x)).sum().backward()
    for a, b in zip(got, q.parameters()):
        _close(a, b.grad, "TwinQ gradient", 2e-5)


def test_hooked_parameters_get_returned_gradients(monkeypatch):
    """A parameter with a hook takes no in-place sum: under ``grads_in_place()`` the call is still served and autograd accumulates."""
    from cleandiffuser_amd.engine import tower, train
    served = []
    _patch_to_cpu(monkeypatch, tower, served)
    seq, x = _critic_like()
    stock, _ = _critic_like()
    stock.load_state_dict(seq.state_dict())
    fired = []
    seq[0].weight.register_hook(lambda g: fired.append(g.shape))
    with train.grads_in_place(list(seq.parameters())):
        tower.try_tower((seq,), x)[0].sum().backward()
    stock(x).sum().backward()
    assert len(served) == 1 and fired
    for p, p0 in zip(seq.parameters(), stock.parameters()):
        _close(p.grad, p0.grad, "gradient", 2e-5)


def test_descriptions_of_the_shipped_critics():
    """``describe`` of DQLCritic, TwinQ, V and a nested ``utils.Mlp`` is what the kernel expects."""
    from cleandiffuser_amd.engine import consts as P, tower
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V
    from cleandiffuser_amd.utils.blocks import Mlp
    c = DQLCritic(17, 6)
    for seq in (c.q1_model, c.q2_model):
        d = tower.describe(seq)
        assert tower.shape_of(d) == (23, (256, 256, 256, 1), (True, True, True, False), (P.ACT_TANH, P.ACT_MISH, P.ACT_MISH, P.ACT_NONE),
                                     (1e-5, 1e-5, 1e-5, 0.0))
        assert tower.params_of(d) == list(seq.parameters())
    q = TwinQ(17, 6)
    assert tower.shape_of(tower.describe(q.Q1)) == tower.shape_of(tower.describe(q.Q2)) == \
        (23, (256, 256, 1), (True, True, False), (P.ACT_MISH, P.ACT_MISH, P.ACT_NONE), (1e-5, 1e-5, 0.0))
    d = tower.describe(V(17, hidden_dim=64).V)
    assert (d.K0, d.width, d.norm) == (17, [64, 64, 1], [True, True, False]) and tower.lds_bytes(d) == 4 * 2 * 16 * 68
    m = Mlp(22, [64, 48], 3, nn.ReLU(), nn.Tanh())                # (one nested Sequential per hidden layer, an output activation)
    d = tower.describe(m.mlp)
    assert tower.shape_of(d) == (22, (64, 48, 3), (False,) * 3, (P.ACT_RELU, P.ACT_RELU, P.ACT_TANH), (0.0,) * 3)
    assert tower.params_of(d) == list(m.parameters())
    assert tower.describe(Mlp(22, [64], 3).mlp).act == [P.ACT_RELU, P.ACT_NONE]      # Identity dropped
    assert tower.describe(m) is None                                                  # (the module itself is no Sequential)


def _c_side():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import tower
    return tower, tower._lib()


_c_request = tc.c_request


def test_lds_plan_matches_the_c_side():
    """``tower.lds_bytes`` (what the router checks) == ``cdx_tower_lds_bytes`` (what the launch uses) over a sweep of input widths, widths
    and depths.  The plan is two activation images of the widest operand, so the widest admissible tower (512 throughout, six layers)
    needs 66 048 bytes: with these width limits no admissible size reaches the 160 KiB bound the entry points check."""
    tower, lib = _c_side()
    worst = 0
    for k0, w, last, depth in itertools.product((1, 7, 20, 32, 500, 512), (16, 48, 256, 512), (1, 3, 64), (1, 2, 4, 6)):
        widths = [w] * (depth - 1) + [last]
        d = SimpleNamespace(K0=k0, width=widths, norm=[False] * depth, eps=[0.0] * depth)
        got = lib.cdx_tower_lds_bytes(ctypes.byref(_c_request(tower, k0, widths)))
        assert got == tower.lds_bytes(d) and tower.within_limits(d), (k0, widths, got)
        worst = max(worst, got)
    assert worst == 4 * 2 * 16 * 516 <= tower.MAX_LDS
    # the first sizes past the limits are refused on both sides
    for k0, widths in ((513, [16, 1]), (7, [528, 1]), (7, [24, 1]), (7, [16, 65]), (7, [16] * 6 + [1])):
        d = SimpleNamespace(K0=k0, width=widths, norm=[False] * len(widths), eps=[0.0] * len(widths))
        assert not tower.within_limits(d)
        if len(widths) <= tower.MAX_LAYERS:
            assert lib.cdx_tower_lds_bytes(ctypes.byref(_c_request(tower, k0, widths))) == -1, (k0, widths)


def test_tower_validation_fails_loudly():
    """The limits of csrc/cdx_tower.hip are refused with CDX_EINVAL and a message before anything is launched (no GPU needed)."""
    tower, lib = _c_side()
    for fn in (lib.cdx_tower_fwd_f32, lib.cdx_tower_bwd_f32):
        assert fn(None, None) == -1 and b"null request" in lib.cdx_last_error()
        for change, word in ((dict(n_towers=3), b"n_towers"), (dict(n_layers=7), b"n_layers"), (dict(n_layers=0), b"n_layers"),
                             (dict(K0=513), b"K0"), (dict(K0=0), b"K0"), (dict(R=-1), b"R")):
            g = _c_request(tower, 7, [16, 1])
            for k, v in change.items():
                setattr(g, k, v)
            assert fn(ctypes.byref(g), None) == -1 and word in lib.cdx_last_error(), (change, lib.cdx_last_error())
        for widths, word in (([24, 1], b"multiple of 16"), ([528, 1], b"multiple of 16"), ([16, 65], b"last width"), ([16, 0], b"last width")):
            assert fn(ctypes.byref(_c_request(tower, 7, widths)), None) == -1 and word in lib.cdx_last_error(), widths
        assert fn(ctypes.byref(_c_request(tower, 7, [16, 1], acts=[2, 0])), None) == -1 and b"activation" in lib.cdx_last_error()   # GELU
        g = _c_request(tower, 7, [16, 1], norms=[1, 0])
        g.eps[0] = 0.0
        assert fn(ctypes.byref(g), None) == -1 and b"eps" in lib.cdx_last_error()
        assert fn(ctypes.byref(_c_request(tower, 7, [16, 1])), None) == -1 and b"null pointer" in lib.cdx_last_error()
        g = _c_request(tower, 7, [16, 1])
        g.R = 0
        assert fn(ctypes.byref(g), None) == 0                                            # an empty batch is not an error
    assert lib.cdx_tower_lds_bytes(None) == -1 and b"null request" in lib.cdx_last_error()
    assert lib.cdx_colsum_batch_f32(None, None) == -1 and b"null request" in lib.cdx_last_error()
    assert lib.cdx_colsum_batch_f32(ctypes.byref(tower.CdxColsumBatch()), None) == 0    # nothing to do
    b = tower.CdxColsumBatch(n_jobs=33)
    assert lib.cdx_colsum_batch_f32(ctypes.byref(b), None) == -1 and b"n_jobs" in lib.cdx_last_error()
    b = tower.CdxColsumBatch(n_jobs=1)
    b.job[0] = tower.CdxColsumJob(src=8, out=8, rows=65, cols=65, ld=64)
    assert lib.cdx_colsum_batch_f32(ctypes.byref(b), None) == -1 and b"bad shape" in lib.cdx_last_error()
    b.job[0].ld = 65
    b.wg_start[1] = 3                                                                     # 2 column tiles x 2 row slices
    assert lib.cdx_colsum_batch_f32(ctypes.byref(b), None) == -1 and b"wg_start" in lib.cdx_last_error()
    b.job[0].src = None
    b.wg_start[1] = 4
    assert lib.cdx_colsum_batch_f32(ctypes.byref(b), None) == -1 and b"null pointer" in lib.cdx_last_error()


def test_tower_mirrors_have_the_c_layout(tmp_path):
    """``CdxTower`` / ``CdxColsumJob`` / ``CdxColsumBatch`` == the structs of include/cdx.h (gcc sizeof / offsetof), and the header's ABI number
    is the one the package expects (19 since ``cdx_optim_args`` carries the host's 1 - beta complements; the tower's own entries were
    purely additive)."""
    from cleandiffuser_amd.engine import tower
    mirrors = {"cdx_tower": tower.CdxTower, "cdx_colsum_job": tower.CdxColsumJob, "cdx_colsum_batch": tower.CdxColsumBatch}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){',
           'printf("%d\\n%d\\n%d\\n", CDX_ABI_VERSION, CDX_TOWER_MAX_LAYERS, CDX_COLSUM_BATCH);']
    for cname, mirror in mirrors.items():
        src.append(f'printf("%zu\\n", sizeof({cname}));')
        src += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src += ['return 0;}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert [int(next(out)) for _ in range(3)] == [19, tower.MAX_LAYERS, tower.COLSUM_BATCH]
    for cname, mirror in mirrors.items():
        assert int(next(out)) == ctypes.sizeof(mirror), cname
        for f in mirror._fields_:
            assert getattr(mirror, f[0]).offset == int(next(out)), (cname, f[0])
