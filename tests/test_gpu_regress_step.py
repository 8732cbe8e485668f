"""The fused regression step on the MI355X (csrc/cdx_regress_step.hip behind engine/regress_step.py, utils/regression_steps.py and
invdynamic/mlp.py): every buffer of the launch against the float64 restatement, reproducibility, the margins around the outputs, the
fused route against the parent route, the inverse-dynamics steps against the fixture of the real reference, the launch structure."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regress_step_cases as rc  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUFFER_BAR = 1e-4              # x max |ref| per buffer: the bar of tests/test_gpu_critic_step.py for the same arithmetic
GRAD_BAR = 2e-4                # x max |g_ref| per parameter


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for k in ("CDX_REGRESS_STEP", "CDX_TOWER", "CDX_TRAIN_NATIVE", "CDX_TRAIN_INPLACE_GRADS"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def references():
    """The float64 restatement of every case on the CPU: computed once, read only."""
    from cleandiffuser_amd.engine import regress_step
    out = {}
    for name in rc.TABLE:
        case = rc.CASES[name]
        q = rc.request(regress_step, case, rc.build(case, dtype=torch.float64), rc.make_inputs(case, dtype=torch.float64))
        regress_step.reference_step(q)
        out[name] = {k: v.detach().clone().numpy() for k, v in rc.buffers(q).items()}
    return out


def _request(name):
    from cleandiffuser_amd.engine import regress_step
    case = rc.CASES[name]
    return rc.request(regress_step, case, rc.build(case, device=DEV), rc.make_inputs(case, device=DEV))


def _native(name):
    from cleandiffuser_amd.engine import regress_step
    q = _request(name)
    regress_step.native_step(q)
    return q


@pytest.mark.parametrize("name", rc.TABLE)
def test_the_launch_matches_the_float64_restatement(name, references):
    """Every buffer ``cdx_regress_step_f32`` writes -- x_cat, out, loss_part, H_l, R W G_l, R W Sb_l, R W Sg_l -- against
    ``reference_step`` in float64 on the CPU within 1e-4 x max |ref| of the buffer."""
    got = {k: v.detach().cpu().double().numpy() for k, v in rc.buffers(_native(name)).items()}
    want = references[name]
    assert list(got) == list(want)
    worst = []
    for what in want:
        err, top = float(np.abs(got[what] - want[what]).max()), float(np.abs(want[what]).max())
        print(f"  {name} {what}: max|d| {err:.3e}  max|ref| {top:.3e}  ratio {err / top if top else 0.0:.2e}")
        if err > BUFFER_BAR * top:
            worst.append((what, err, top))
    assert not worst, worst


@pytest.mark.parametrize("name", ["invdyn_r33_k22_h32", "fancy_eval_r17_h32", "last64_r17", "dd_view_7x4x11"])
def test_two_launches_give_the_same_bits(name):
    """No atomics, one fixed lane and order per element: two launches on the same inputs are ``torch.equal`` in everything they write."""
    a, b = rc.buffers(_native(name)), rc.buffers(_native(name))
    torch.cuda.synchronize()
    for what in a:
        assert torch.equal(a[what], b[what]), what


@pytest.mark.parametrize("name", ["invdyn_r1_k22_h32", "invdyn_r17_k22_h32", "fancy_eval_r17_h32", "depth1_r17", "dd_view_7x4x11"])
def test_the_margins_around_the_outputs_stay_untouched(name):
    """Every output of the launch lives inside a sentinel-filled slab with 64 floats of margin on both sides; afterwards the margins
    still hold the sentinel and the insides equal an unpadded launch bit for bit."""
    from cleandiffuser_amd.engine import regress_step, tower
    plain = _native(name)
    q = _request(name)
    lv, M, SENT = q.live, 64, -777.25
    slabs = []

    def padded(t):
        """A fresh tensor of t's shape whose last dimension sits inside a sentinel slab."""
        slab = torch.full((*t.shape[:-1], t.shape[-1] + 2 * M), SENT, device=DEV)
        slabs.append((slab, t.shape[-1]))
        return slab[..., M:M + t.shape[-1]]
    q.loss_part = padded(q.loss_part)
    q.x_cat = padded(q.x_cat.view(-1)).view(q.x_cat.shape)
    lv.x = q.x_cat
    lv.out = [padded(lv.out[0].view(-1)).view(lv.out[0].shape)]
    lv.H_buf, lv.G_buf, lv.S_buf = padded(lv.H_buf), padded(lv.G_buf), padded(lv.S_buf)
    lv.H, lv.G = tower._layers(lv.H_buf, q.R, lv.width[:-1]), tower._layers(lv.G_buf, q.R, lv.width)
    lv.Sb, lv.Sg = tower._layers(lv.S_buf[0], q.tiles, lv.width), tower._layers(lv.S_buf[1], q.tiles, lv.width)
    regress_step.native_step(q)
    torch.cuda.synchronize()
    unnormed = [l for l, n in enumerate(lv.norm) if not n]
    for slab, n in slabs:
        assert bool((slab[..., :M] == SENT).all()) and bool((slab[..., M + n:] == SENT).all()), "a margin was written"
    for l in unnormed:                                      # (Sb / Sg of a layer without a norm are nobody's to write)
        assert bool((lv.Sb[0][l] == SENT).all()) and bool((lv.Sg[0][l] == SENT).all()), l
    a, b = rc.buffers(q), rc.buffers(plain)
    assert list(a) == list(b)
    for what in a:
        assert torch.equal(a[what], b[what]), what


def _spy(monkeypatch):
    """The requests the fused launch served."""
    from cleandiffuser_amd.engine import regress_step
    seen, real = [], regress_step.native_step

    def spy(q):
        real(q)
        seen.append(q)
    monkeypatch.setattr(regress_step, "native_step", spy)
    return seen


def _batch(kind, rows=None):
    g = torch.Generator().manual_seed(8)
    B, H = (7, 4) if kind == "dd" else (40, 3)
    obs, act = torch.randn(B, H, 17, generator=g).to(DEV), torch.randn(B, H, 6, generator=g).tanh().to(DEV)
    if kind == "dd":
        return obs[:, :-1], act[:, :-1], obs[:, 1:]
    return obs[:, 0], act[:, 0], obs[:, 1]


def _one_step(kind, route, monkeypatch):
    """(loss, gradients) of one step from fixed weights on `route` ("1": fused, "0": the parent route)."""
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.invdynamic import MlpInvDynamic
    from cleandiffuser_amd.invdynamic.mlp import EnsembleMlpInvDynamic
    from cleandiffuser_amd.utils import Mlp, load_synth
    from cleandiffuser_amd.utils.regression_steps import mse_step
    monkeypatch.setenv("CDX_REGRESS_STEP", route)
    if kind in ("update_dd", "update_dv"):
        head = MlpInvDynamic(17, 6, hidden_dim=64, optim_params={"lr": 0.0}, device=DEV)
        net = load_synth(head.mlp, 1)
        o, a, o_next = _batch(kind[-2:])
        loss = head.update(o, a, o_next)["loss"]
    elif kind == "update_idx":
        head = EnsembleMlpInvDynamic(17, 6, hidden_dim=64, n_models=2, optim_params={"lr": 0.0}, device=DEV)
        net = load_synth(head.mlp, 2)[1]
        o, a, o_next = _batch("dd")
        loss = head.update_idx(1, o, a, o_next)
        assert all(p.grad is None or not bool(p.grad.any()) for p in head.mlp[0].parameters()), "member 0 took a gradient"
    else:                                                  # SfBC's critic: a scalar regression on [obs | act]
        net = load_synth(Mlp(23, [64, 64], 1, nn.Mish()), 3).to(DEV)
        o, a, _ = _batch("dv")
        g = torch.Generator().manual_seed(4)
        loss = float(mse_step(net, FusedAdam(net.parameters(), lr=0.0), o, torch.randn(o.shape[0], 1, generator=g).to(DEV), x1=a)["loss"])
    return float(loss), [p.grad.detach().cpu().numpy().copy() for p in net.parameters()]


@pytest.mark.parametrize("kind", ["update_dd", "update_dv", "update_idx", "mse_step"])
def test_the_two_routes_agree(kind, monkeypatch):
    """From the same weights and batch the fused step (``CDX_REGRESS_STEP=1``) and the parent route (``CDX_REGRESS_STEP=0``) give the loss
    and every gradient within 2e-4 x the largest magnitude of each; a spy shows which route served."""
    seen = _spy(monkeypatch)
    la, ga = _one_step(kind, "1", monkeypatch)
    assert len(seen) == 1, "the fused launch did not serve the step"
    if kind == "update_dd":
        assert (seen[0].map0, seen[0].map1, seen[0].map_y) == ((3, 4, 17), (3, 4, 17), (3, 4, 6)), "the views were copied"
    lb, gb = _one_step(kind, "0", monkeypatch)
    assert len(seen) == 1, "CDX_REGRESS_STEP=0 took the fused launch"
    print(f"  {kind}: loss {la:.7f} (fused) {lb:.7f} (parent); {len(ga)} gradients")
    assert abs(la - lb) <= GRAD_BAR * abs(lb)
    assert len(ga) == len(gb) > 0
    for u, w in zip(ga, gb):
        top = float(np.abs(w).max())
        assert top > 0.0 and float(np.abs(u - w).max()) <= GRAD_BAR * top, (kind, float(np.abs(u - w).max()), top)


@pytest.mark.parametrize("name", list(rc.GOLDEN_CASES))
def test_update_reproduces_the_reference_fixture(name, monkeypatch):
    """Three ``MlpInvDynamic.update`` steps on the device, every step on the fused launch (``CDX_REGRESS_STEP=1``), against the real
    reference (tests/golden/invdyn_steps.npz): losses and parameter checksums at rtol = atol = 1e-4, the first step's gradients at
    2e-4 x max |g_ref| per parameter."""
    seen = _spy(monkeypatch)
    monkeypatch.setenv("CDX_REGRESS_STEP", "1")
    gold = rc.golden(name)
    got = rc.run_invdyn(rc.invdyn_of("amd"), rc.GOLDEN_CASES[name], DEV)
    assert len(seen) == rc.STEPS, "a step fell back to the eager sequence"
    assert set(got) == set(gold)
    for k in ("loss", "sums"):
        print(f"  {name} {k}: max|d| {float(np.abs(got[k] - gold[k]).max()):.3e}")
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
    names = [k for k in gold if k.startswith("grad/")]
    assert len(names) == 6
    for n in names:
        ref = np.asarray(gold[n], dtype=np.float64)
        err, bar = float(np.abs(np.asarray(got[n], dtype=np.float64) - ref).max()), GRAD_BAR * float(np.abs(ref).max())
        print(f"  {name} {n}: max|d| {err:.3e}  bar {bar:.3e}")
        assert err <= bar, (name, n, err, bar)


def _step_kernels(rows, route, monkeypatch):
    """The device kernels of a steady-state ``MlpInvDynamic.update`` (FusedAdam) at the shipped widths."""
    from torch.autograd import DeviceType
    from cleandiffuser_amd.invdynamic import MlpInvDynamic
    from cleandiffuser_amd.utils import load_synth
    monkeypatch.setenv("CDX_REGRESS_STEP", route)
    g = torch.Generator().manual_seed(2)
    head = MlpInvDynamic(17, 6, optim_params={"lr": 3e-4}, device=DEV)
    load_synth(head.mlp, 5)
    o, a, o_next = (torch.randn(rows, n, generator=g).to(DEV) for n in (17, 6, 17))

    def step():
        head.update(o, a, o_next)
    for _ in range(2):
        step()
    prof, _ = profiled(step)
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def test_the_launch_structure_of_a_step(monkeypatch):
    """A steady-state ``update`` contains the step kernel, the batched weight-gradient kernel and the batched column sum exactly once
    each and no tower, GEMM, ATen GEMM, cat or copy kernel, the same number of device kernels at 16 and at 64 rows, and strictly fewer
    than the parent route (``CDX_REGRESS_STEP=0``) launches, measured here."""
    counts = {}
    for rows in (16, 64):
        kernels = _step_kernels(rows, "1", monkeypatch)
        print(f"rows = {rows}: {len(kernels)} device kernels on the fused step: {sorted(set(kernels))}")
        for k in ("cdx_regress_step_kernel", "cdx_conv_wgrad_batch_kernel", "cdx_colsum_batch_kernel"):
            assert sum(k in n for n in kernels) == 1, (k, kernels)
        low = [n.lower() for n in kernels]
        assert not any(k in n for n in low for k in ("cdx_tower_", "cdx_gemm_kernel", "cijk_", "addmm", "gemm", "catarray", "copy"))
        counts[rows] = len(kernels)
    assert counts[16] == counts[64], counts
    parent = _step_kernels(16, "0", monkeypatch)
    print(f"rows = 16: {len(parent)} device kernels on the parent route (CDX_REGRESS_STEP=0), {counts[16]} on the fused step")
    assert not any("cdx_regress_step" in n for n in parent)
    assert counts[16] < len(parent), (counts, len(parent))
