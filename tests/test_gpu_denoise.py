"""The fused denoising step on the MI355X (csrc/cdx_denoise.hip behind engine/denoise.py): every buffer of both launches against the
float64 restatement, ``loss()`` / ``approx_action`` + ``backward()`` against the float64 CPU run of the stock module path and the record of
the real reference, bit-reproducibility, seeded draws, and the launch structure."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_cases as dc  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN, SENTINEL = 64, -12345.0
FWD_BUFFERS = ("feat", "Zt", "Ht", "Z", "H", "pred", "loss_part")
BWD_BUFFERS = ("Z", "Zt", "G_head", "G_t2", "g_cond", "g_emb0", "g_xt")


@pytest.fixture(autouse=True)
def _fused_route(monkeypatch):
    monkeypatch.setenv("CDX_DENOISE", "1")
    monkeypatch.setenv("CDX_TRAIN_NATIVE", "1")


def _with_margins(q, names):
    """Every named buffer of the request re-homed in the middle of a sentinel-filled allocation -> {name: the whole allocation}."""
    homes = {}
    for n in names:
        t = getattr(q, n)
        if t is None:
            continue
        whole = torch.full((t.numel() + 2 * MARGIN,), SENTINEL, device=t.device, dtype=t.dtype)
        inner = whole[MARGIN:MARGIN + t.numel()].view(t.shape)
        inner.copy_(t)
        setattr(q, n, inner)
        homes[n] = whole
    return homes


def _margins_untouched(homes):
    for n, whole in homes.items():
        assert bool((whole[:MARGIN] == SENTINEL).all()) and bool((whole[-MARGIN:] == SENTINEL).all()), f"the margin of {n} was written"


def _buffers_close(got, want, what):
    for n, ref in want.items():
        err, scale = float((got[n].cpu().double() - ref).abs().max()), float(ref.abs().max())
        print(f"  {what} {n}: max|d| {err:.3e}, max|ref| {scale:.3e}")
        assert err <= 1e-4 * scale, (n, err, scale)


@pytest.mark.parametrize("name", dc.TABLE)
def test_every_buffer_of_both_launches_matches_the_float64_restatement(name, amd_lib):
    """feat, Zt, Ht, Z, H, pred, loss_part after the forward launch and G (over Z), Gt (over Zt), G_head, G_t2, g_cond, g_emb0, g_xt
    after the backward launch, each to 1e-4 max|ref|, with 64 sentinel floats on either side of every buffer untouched; a second pair
    of launches on the same inputs gives the same bits."""
    from cleandiffuser_amd.engine import denoise
    case = dc.CASES[name]
    with dc.float64_default():
        agent64, inp64 = dc.build(case, amd_lib, "cpu", torch.float64)
        q64 = dc.request(agent64, case, inp64)
        denoise.reference_forward(q64)
        fwd64 = {n: getattr(q64, n).clone() for n in FWD_BUFFERS if getattr(q64, n) is not None}
        denoise.reference_backward(q64)
    agent, inp = dc.build(case, amd_lib, DEV)
    runs = []
    for _ in range(2):
        q = dc.request(agent, case, inp)
        homes = _with_margins(q, FWD_BUFFERS + BWD_BUFFERS[2:])
        denoise.native_forward(q)
        torch.cuda.synchronize()
        fwd = {n: getattr(q, n).clone() for n in fwd64}
        denoise.native_backward(q)
        torch.cuda.synchronize()
        _margins_untouched(homes)
        runs.append((fwd, {n: getattr(q, n).clone() for n in BWD_BUFFERS if getattr(q, n) is not None}))
    fwd, bwd = runs[0]
    _buffers_close(fwd, fwd64, "forward")
    _buffers_close(bwd, {n: getattr(q64, n) for n in BWD_BUFFERS if getattr(q64, n) is not None}, "backward")
    for a, b in zip(runs[0], runs[1]):
        for n in a:
            assert torch.equal(a[n], b[n]), f"{n} differs between two identical launches"


def _check_against(ref, value, agent, obs, xt, with_xt=True):
    np.testing.assert_allclose(value.cpu().numpy(), ref.value.numpy(), rtol=1e-4, atol=1e-4)
    got = {n: p.grad for n, p in agent.model["diffusion"].named_parameters() if p.grad is not None}
    assert set(got) == set(ref.grads) and len(got) == 12
    want = dict(ref.grads)
    if ref.g_obs is not None:
        got["obs"], want["obs"] = obs.grad, ref.g_obs
    else:
        assert obs is None or obs.grad is None
    if ref.g_xt is not None and with_xt:
        got["xt"], want["xt"] = xt.grad, ref.g_xt
    for n, g_ref in want.items():
        err, scale = float((got[n].cpu().double() - g_ref).abs().max()), float(g_ref.abs().max())
        print(f"  {n}: max|d| {err:.3e}, max|g_ref| {scale:.3e}")
        assert err <= 2e-4 * scale, (n, err, scale)


def _spy(monkeypatch):
    from cleandiffuser_amd.engine import denoise
    seen, real = [], denoise.native_forward

    def spy(q):
        seen.append(q)
        real(q)
    monkeypatch.setattr(denoise, "native_forward", spy)
    return seen


@pytest.mark.parametrize("name", dc.TABLE)
def test_loss_and_approx_action_match_the_float64_module_path(name, amd_lib, monkeypatch):
    """``loss()`` + ``backward()`` (loss cases) and the prediction node behind ``approx_action`` + ``backward()`` (prediction cases) on
    the fused route against the float64 CPU run of the stock modules: the value at rtol = atol = 1e-4, every parameter gradient, d / d
    obs and d / d xt at max|d| <= 2e-4 max|g_ref|."""
    from cleandiffuser_amd.engine import denoise
    ref = dc.reference(name)
    case = ref.case
    seen = _spy(monkeypatch)
    agent, inp = dc.build(case, amd_lib, DEV)
    value, obs, xt = dc.run(agent, case, inp, route=denoise.try_predict)
    torch.cuda.synchronize()
    assert len(seen) == 1, "the fused route did not take this request"
    _check_against(ref, value, agent, obs, xt)
    if case.mode == "pred" and inp.obs is not None:       # the same evaluation through the public call, which noises the action itself
        from cleandiffuser_amd.utils.policy_steps import approx_action
        agent.model.zero_grad(set_to_none=True)
        obs = inp.obs.clone().requires_grad_(case.cond_grad)
        pred = approx_action(agent, inp.x0, obs, t=inp.t, eps=inp.eps)
        dc.objective(pred, inp).backward()
        torch.cuda.synchronize()
        assert len(seen) == 2, "approx_action did not take the fused node"
        _check_against(ref, pred.detach(), agent, obs, None, with_xt=False)


@pytest.mark.parametrize("name", dc.LOSS_CASES)
def test_loss_matches_the_record_of_the_real_reference(name, amd_lib, monkeypatch):
    """``loss()`` + ``backward()`` on the fused route with the recorded t and eps against tests/golden/denoise_steps.npz: the loss at
    rtol = atol = 1e-4, the gradients the file holds at max|d| <= 2e-4 max|g_ref|."""
    gold = dc.golden(name)
    case = dc.CASES[name]
    seen = _spy(monkeypatch)
    agent, _ = dc.build(case, amd_lib, DEV)
    inp = dc.inputs(case, DEV, torch.float32, gold)
    loss, _, _ = dc.run(agent, case, inp)
    torch.cuda.synchronize()
    assert len(seen) == 1, "the fused route did not take this request"
    np.testing.assert_allclose(float(loss), float(gold["loss"]), rtol=1e-4, atol=1e-4)
    grads = dict(agent.model["diffusion"].named_parameters())
    for k in [k for k in gold if k.startswith("grad/")]:
        g_ref = gold[k].astype(np.float64)
        err, scale = float(np.abs(grads[k[5:]].grad.cpu().double().numpy() - g_ref).max()), float(np.abs(g_ref).max())
        print(f"  {k}: max|d| {err:.3e}, max|g_ref| {scale:.3e}")
        assert err <= 2e-4 * scale, (k, err, scale)


def test_approx_action_draws_and_predicts_as_the_module_call(amd_lib, monkeypatch):
    """``approx_action`` under a seed: the fused prediction node and the module call (CDX_DENOISE=0) see the same draws and give the
    same prediction and d / d obs."""
    from cleandiffuser_amd.utils.policy_steps import approx_action
    case = dc.CASES["dv64_r33_pred_nocondgrad"]
    agent, inp = dc.build(case, amd_lib, DEV)
    seen = _spy(monkeypatch)
    out = []
    for route in ("1", "0"):
        monkeypatch.setenv("CDX_DENOISE", route)
        torch.manual_seed(11)
        obs = inp.obs.clone().requires_grad_(True)
        pred = approx_action(agent, inp.x0, obs)
        dc.objective(pred, inp).backward()
        out.append((pred.detach().cpu(), obs.grad.cpu()))
    assert len(seen) == 1
    np.testing.assert_allclose(out[0][0].numpy(), out[1][0].numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out[0][1].numpy(), out[1][1].numpy(), rtol=2e-4, atol=2e-4 * float(out[1][1].abs().max()))


@pytest.mark.parametrize("sde", ["DiscreteDiffusionSDE", "ContinuousDiffusionSDE"])
def test_a_seeded_loss_does_not_depend_on_the_route(sde, amd_lib, monkeypatch):
    """``torch.manual_seed`` and ``loss()``: the fused route and the per-layer route (CDX_DENOISE=0) draw the same t and eps -- the same
    value, under both SDE classes, with the condition encoder's dropout mask drawn after them on both."""
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.DQLMlp(11, 6, emb_dim=16), 65).to(DEV)
    agent = getattr(amd_lib, sde)(net, amd_lib.IdentityCondition(dropout=0.25), predict_noise=False, device=DEV,
                                  **({"diffusion_steps": 5} if sde == "DiscreteDiffusionSDE" else {}))
    seen = _spy(monkeypatch)
    g = torch.Generator().manual_seed(3)
    act, obs = torch.randn(40, 6, generator=g).to(DEV), torch.randn(40, 11, generator=g).to(DEV)
    values = []
    for route in ("1", "0"):
        monkeypatch.setenv("CDX_DENOISE", route)
        torch.manual_seed(123)
        values.append(float(agent.loss(act, obs)))
    assert len(seen) == 1
    np.testing.assert_allclose(values[0], values[1], rtol=1e-4, atol=1e-4)


def _kernels(prof):
    from torch.autograd import DeviceType
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def test_one_forward_and_one_backward_kernel_whatever_the_rows(amd_lib, monkeypatch):
    """``loss()`` + ``backward()``: cdx_denoise_fwd / cdx_denoise_bwd exactly once each, the same number of device kernels at 16 and at
    64 rows, and fewer than the per-layer route (CDX_DENOISE=0) launches for the same step."""
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.DQLMlp(11, 6, emb_dim=16), 65).to(DEV)
    agent = amd_lib.DiscreteDiffusionSDE(net, amd_lib.IdentityCondition(dropout=0.0), predict_noise=False, diffusion_steps=5, device=DEV)

    def step(rows):
        agent.model.zero_grad(set_to_none=True)
        act, obs = torch.ones(rows, 6, device=DEV), torch.ones(rows, 11, device=DEV)
        agent.loss(act, obs).backward()

    counts = {}
    for route, rows in (("1", 16), ("1", 64), ("0", 64)):
        monkeypatch.setenv("CDX_DENOISE", route)
        for _ in range(2):                                  # (weight layouts and the library are warm)
            step(rows)
        prof, _ = profiled(lambda: step(rows))
        kernels = _kernels(prof)
        print("CDX_DENOISE =", route, rows, "rows:", len(kernels), "device kernels")
        n_fwd, n_bwd = sum("cdx_denoise_fwd" in k for k in kernels), sum("cdx_denoise_bwd" in k for k in kernels)
        assert (n_fwd, n_bwd) == ((1, 1) if route == "1" else (0, 0)), kernels
        counts[route, rows] = len(kernels)
    assert counts["1", 16] == counts["1", 64], counts
    assert counts["1", 64] < counts["0", 64], counts
