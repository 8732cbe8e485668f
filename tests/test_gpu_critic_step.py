"""The fused critic step on the MI355X (csrc/cdx_critic_step.hip behind engine/critic_step.py and utils/critic_steps.py): every buffer of
the launch against the float64 restatement, reproducibility, the margins around the outputs, the critic steps of the shipped loops
against the fixtures of the real reference, the fused route against the parent route, the launch structure."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_step_cases as cc  # noqa: E402
import critic_steps as cs  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUFFER_BAR = 1e-4              # x max |ref| per buffer: the bar of tests/test_gpu_tower.py for the same arithmetic
GRAD_BAR = 2e-4                # x max |g_ref| per parameter


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for k in ("CDX_CRITIC_STEP", "CDX_TOWER", "CDX_TRAIN_NATIVE", "CDX_TRAIN_INPLACE_GRADS"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def references():
    """The float64 restatement of every case on the CPU: computed once, read only."""
    from cleandiffuser_amd.engine import critic_step
    out = {}
    for name in cc.TABLE:
        case = cc.CASES[name]
        live, target = cc.build(case, dtype=torch.float64)
        q = cc.request(critic_step, case, live, target, cc.make_inputs(case, dtype=torch.float64))
        critic_step.reference_step(q)
        out[name] = {k: v.detach().clone().numpy() for k, v in cc.buffers(q).items()}
    return out


def _native(name):
    from cleandiffuser_amd.engine import critic_step
    case = cc.CASES[name]
    live, target = cc.build(case, device=DEV)
    q = cc.request(critic_step, case, live, target, cc.make_inputs(case, device=DEV))
    critic_step.native_step(q)
    return q


@pytest.mark.parametrize("name", cc.TABLE)
def test_the_launch_matches_the_float64_restatement(name, references):
    """Every buffer ``cdx_critic_step_f32`` writes -- y, y_part, loss_part, x_cat, q, H_l, R G_l, R Sb_l, R Sg_l of every live tower --
    against ``reference_step`` in float64 on the CPU within 1e-4 x max |ref| of the buffer."""
    got = {k: v.detach().cpu().double().numpy() for k, v in cc.buffers(_native(name)).items()}
    want = references[name]
    assert list(got) == list(want)
    worst = []
    for what in want:
        err, top = float(np.abs(got[what] - want[what]).max()), float(np.abs(want[what]).max())
        print(f"  {name} {what}: max|d| {err:.3e}  max|ref| {top:.3e}  ratio {err / top if top else 0.0:.2e}")
        if err > BUFFER_BAR * top:
            worst.append((what, err, top))
    assert not worst, worst


@pytest.mark.parametrize("name", ["dql_r17_k23_h32", "iql_v_r33_tau07_h64", "qgpo_k16_r17_beta3", "unequal_r33"])
def test_two_launches_give_the_same_bits(name):
    """No atomics, one fixed lane and order per element: two launches on the same inputs are ``torch.equal`` in everything they write."""
    a, b = cc.buffers(_native(name)), cc.buffers(_native(name))
    torch.cuda.synchronize()
    for what in a:
        assert torch.equal(a[what], b[what]), what


@pytest.mark.parametrize("name", ["dql_r17_k23_h32", "iql_q_r16_k14_h32_done0", "single_r1_k14_done1", "antmaze_k10_r5"])
def test_the_margins_around_the_outputs_stay_untouched(name):
    """Every output of the launch lives inside a sentinel-filled slab with 64 floats of margin on both sides (the per-tower buffers: around
    each tower's share); afterwards the margins still hold the sentinel and the insides equal an unpadded launch bit for bit."""
    from cleandiffuser_amd.engine import critic_step, tower
    plain = _native(name)
    case = cc.CASES[name]
    live, target = cc.build(case, device=DEV)
    q = cc.request(critic_step, case, live, target, cc.make_inputs(case, device=DEV))
    lv, M, SENT = q.live, 64, -777.25
    slabs = []

    def padded(t):
        """A fresh tensor of t's shape whose last dimension sits inside a sentinel slab."""
        slab = torch.full((*t.shape[:-1], t.shape[-1] + 2 * M), SENT, device=DEV)
        slabs.append((slab, t.shape[-1]))
        return slab[..., M:M + t.shape[-1]]
    q.y, q.y_part, q.loss_part = padded(q.y), padded(q.y_part), padded(q.loss_part)
    q.x_cat = padded(q.x_cat.view(-1)).view(q.x_cat.shape)
    lv.x = q.x_cat
    outs = padded(torch.empty(lv.n_towers, q.R))
    lv.out = [outs[t].view(q.R, 1) for t in range(lv.n_towers)]
    lv.H_buf, lv.G_buf, lv.S_buf = padded(lv.H_buf), padded(lv.G_buf), padded(lv.S_buf)
    lv.H, lv.G = tower._layers(lv.H_buf, q.R, lv.width[:-1]), tower._layers(lv.G_buf, q.R, lv.width)
    lv.Sb, lv.Sg = tower._layers(lv.S_buf[0], q.tiles, lv.width), tower._layers(lv.S_buf[1], q.tiles, lv.width)
    critic_step.native_step(q)
    torch.cuda.synchronize()
    for slab, n in slabs:
        assert bool((slab[..., :M] == SENT).all()) and bool((slab[..., M + n:] == SENT).all()), "a margin was written"
    a, b = cc.buffers(q), cc.buffers(plain)
    assert list(a) == list(b)
    for what in a:
        assert torch.equal(a[what], b[what]), what


def _assert_grads(got: dict, gold: dict, prefix, what):
    names = [k for k in gold if k.startswith(prefix)]
    assert names and set(names) == {k for k in got if k.startswith(prefix)}, (what, names, list(got))
    for n in names:
        ref = np.asarray(gold[n], dtype=np.float64)
        err, bar = float(np.abs(np.asarray(got[n], dtype=np.float64) - ref).max()), GRAD_BAR * float(np.abs(ref).max())
        print(f"  {what} {n}: max|d| {err:.3e}  bar {bar:.3e}")
        assert err <= bar, (what, n, err, bar)


def _spy(monkeypatch):
    """The requests the fused launch served."""
    from cleandiffuser_amd.engine import critic_step
    seen, real = [], critic_step.native_step

    def spy(q):
        real(q)
        seen.append(q)
    monkeypatch.setattr(critic_step, "native_step", spy)
    return seen


@pytest.mark.parametrize("name", cs.TABLE)
def test_the_calls_reproduce_the_reference_fixture(name, monkeypatch):
    """Three IQL half-steps and three Diffusion-QL critic steps through ``expectile_step`` / ``td_step`` on the device, every step on the
    fused launch (``CDX_CRITIC_STEP=1``), against the real reference (tests/golden/critic_towers.npz): losses and parameter checksums at
    rtol = atol = 1e-4, the first step's gradients at 2e-4 x max |g_ref| per parameter."""
    from cleandiffuser_amd.engine.optim import FusedAdam
    seen = _spy(monkeypatch)
    monkeypatch.setenv("CDX_CRITIC_STEP", "1")
    case, gold, U = cs.CASES[name], cs.golden(name), cs.utils_of("amd")
    got = cc.run_iql_calls(U, case, DEV, adam=FusedAdam)
    assert [(q.live.n_towers, q.loss) for q in seen] == [(1, "expectile"), (2, "mse")] * cs.STEPS, "a step fell back to the eager sequence"
    del seen[:]
    got.update(cc.run_dql_calls(U, case, DEV, adam=FusedAdam))
    assert [(q.live.n_towers, q.dt.K0) for q in seen] == [(2, case.obs + case.act)] * cs.STEPS
    assert set(got) == set(gold)
    for k in ("iql/loss", "dql/loss", "iql/sums/Q", "iql/sums/V", "iql/sums/Q_targ", "dql/sums"):
        print(f"  {name} {k}: max|d| {float(np.abs(got[k] - gold[k]).max()):.3e}")
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
    _assert_grads({k: v for k, v in got.items() if "/grad/" in k}, gold, ("iql/grad/", "dql/grad/"), name)


@pytest.mark.parametrize("name", list(cc.GROUPED))
def test_the_grouped_targets_reproduce_the_reference_fixture(name, monkeypatch):
    """Three antmaze (max over 10 sampled actions) / QGPO (softmax over 16 support actions) critic steps through ``td_step`` on the fused
    launch against the real reference (tests/golden/critic_steps_grouped.npz): losses, mean targets and parameter checksums at rtol =
    atol = 1e-4, the first step's gradients at 2e-4 x max |g_ref| per parameter."""
    from cleandiffuser_amd.engine.optim import FusedAdam
    seen = _spy(monkeypatch)
    monkeypatch.setenv("CDX_CRITIC_STEP", "1")
    case, gold = cc.GROUPED[name], cc.grouped_golden(name)
    got = cc.run_grouped(cs.utils_of("amd"), case, DEV, adam=FusedAdam, step=cc.grouped_call_step)
    assert [(q.K, q.reduce) for q in seen] == [(case.group, "max" if case.kind == "antmaze" else "softmax")] * cs.STEPS
    assert set(got) == set(gold)
    for k in ("loss", "sums"):
        print(f"  {name} {k}: max|d| {float(np.abs(got[k] - gold[k]).max()):.3e}")
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
    _assert_grads(got, gold, "grad/", name)


def _one_step(kind, route, monkeypatch):
    """(loss, mean target, gradients) of one step from fixed weights on `route` ("1": fused, "0": the parent route)."""
    from copy import deepcopy
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V, load_synth
    from cleandiffuser_amd.utils.critic_steps import expectile_step, td_step
    monkeypatch.setenv("CDX_CRITIC_STEP", route)
    g = torch.Generator().manual_seed(8)
    rows, group = 40, {"antmaze": 10, "qgpo": 16}.get(kind, 1)
    obs, act, rew, nxt = (torch.randn(rows, n, generator=g).to(DEV) for n in (17, 6, 1, 17))
    done, nact = (torch.rand(rows, 1, generator=g) < 0.3).float().to(DEV), torch.randn(rows * group, 6, generator=g).tanh().to(DEV)
    twin, v, dql = (load_synth(m, s).to(DEV) for m, s in ((TwinQ(17, 6, hidden_dim=64), 1), (V(17, hidden_dim=64), 2), (DQLCritic(17, 6, hidden_dim=64), 3)))
    if kind == "iql_v":
        live, out = v, None
        out = expectile_step(v, deepcopy(twin).requires_grad_(False), FusedAdam(v.parameters(), lr=0.0), obs, act, tau=0.7)
    elif kind == "iql_q":
        live = twin
        out = td_step(twin, deepcopy(v).requires_grad_(False), FusedAdam(twin.parameters(), lr=0.0), obs, act, rew, nxt, done, discount=0.99)
    else:
        live = twin if kind == "qgpo" else dql
        kw = {"dql": {}, "antmaze": dict(group=10, reduce="max"), "qgpo": dict(group=16, reduce="softmax", beta=3.0)}[kind]
        out = td_step(live, deepcopy(live).requires_grad_(False), FusedAdam(live.parameters(), lr=0.0), obs, act, rew, nxt, done, nact,
                      discount=0.99, **kw)
    return float(out["loss"]), float(out["target_mean"]), [p.grad.detach().cpu().numpy().copy() for p in live.parameters()]


@pytest.mark.parametrize("kind", ["iql_v", "iql_q", "dql", "antmaze", "qgpo"])
def test_the_two_routes_agree(kind, monkeypatch):
    """From the same weights and batch the fused step (``CDX_CRITIC_STEP=1``) and the parent route (``CDX_CRITIC_STEP=0``) give the
    loss, the mean target and every gradient within 2e-4 x the largest magnitude of each; a spy shows which route served."""
    seen = _spy(monkeypatch)
    la, ya, ga = _one_step(kind, "1", monkeypatch)
    assert len(seen) == 1, "the fused launch did not serve the step"
    lb, yb, gb = _one_step(kind, "0", monkeypatch)
    assert len(seen) == 1, "CDX_CRITIC_STEP=0 took the fused launch"
    print(f"  {kind}: loss {la:.7f} (fused) {lb:.7f} (parent); mean target {ya:.7f} {yb:.7f}; {len(ga)} gradients")
    assert abs(la - lb) <= GRAD_BAR * abs(lb) and abs(ya - yb) <= GRAD_BAR * max(abs(yb), 1e-3)
    assert len(ga) == len(gb) > 0
    for u, w in zip(ga, gb):
        top = float(np.abs(w).max())
        assert top > 0.0 and float(np.abs(u - w).max()) <= GRAD_BAR * top, (kind, float(np.abs(u - w).max()), top)


def _step_kernels(rows, route, monkeypatch):
    """The device kernels of a steady-state IQL Q step (``td_step`` of a TwinQ against a V target, FusedAdam) at the shipped widths."""
    from copy import deepcopy
    from torch.autograd import DeviceType
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.utils import TwinQ, V, load_synth
    from cleandiffuser_amd.utils.critic_steps import td_step
    monkeypatch.setenv("CDX_CRITIC_STEP", route)
    g = torch.Generator().manual_seed(2)
    twin, v = load_synth(TwinQ(17, 6), 5).to(DEV), load_synth(V(17), 6).to(DEV).requires_grad_(False)
    optim = FusedAdam(twin.parameters(), lr=3e-4)
    obs, act, rew, nxt = (torch.randn(rows, n, generator=g).to(DEV) for n in (17, 6, 1, 17))
    done = (torch.rand(rows, 1, generator=g) < 0.3).float().to(DEV)

    def step():
        td_step(twin, v, optim, obs, act, rew, nxt, done, discount=0.99)
    for _ in range(2):
        step()
    prof, _ = profiled(step)
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def test_the_launch_structure_of_a_step(monkeypatch):
    """A steady-state TD step contains the step kernel, the batched weight-gradient kernel and the batched column sum exactly once each
    and no tower, GEMM, LayerNorm or ATen GEMM kernel, the same number of device kernels at 16 and at 64 rows, and fewer than half of
    what the parent route (``CDX_CRITIC_STEP=0``) launches, measured here."""
    counts = {}
    for rows in (16, 64):
        kernels = _step_kernels(rows, "1", monkeypatch)
        print(f"rows = {rows}: {len(kernels)} device kernels on the fused step: {sorted(set(kernels))}")
        for k in ("cdx_critic_step_kernel", "cdx_conv_wgrad_batch_kernel", "cdx_colsum_batch_kernel"):
            assert sum(k in n for n in kernels) == 1, (k, kernels)
        low = [n.lower() for n in kernels]
        assert not any(k in n for n in low for k in ("cdx_tower_", "cdx_gemm_kernel", "cdx_layernorm", "cijk_", "addmm", "layer_norm", "gemm"))
        counts[rows] = len(kernels)
    assert counts[16] == counts[64], counts
    parent = _step_kernels(16, "0", monkeypatch)
    print(f"rows = 16: {len(parent)} device kernels on the parent route (CDX_CRITIC_STEP=0), {counts[16]} on the fused step")
    assert not any("cdx_critic_step" in n for n in parent)
    assert 2 * counts[16] < len(parent), (counts, len(parent))
