"""QGPO's contrastive energy training step on the MI355X (csrc/cdx_cep.hip behind engine/cep.py): the kernel's buffers against the
float64 restatement, ``update()`` against the fixture of the real reference, the launch structure, the two routes, reproducibility."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cep_cases as cc  # noqa: E402
from gpu_profile import profiled  # noqa: E402
from test_cep_cpu import assert_grads, assert_log, clip_factor  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.delenv("CDX_CEP", raising=False)
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)


def _spy_step(monkeypatch):
    """The requests the kernel served."""
    from cleandiffuser_amd.engine import cep
    seen, real = [], cep.native_step

    def spy(q):
        real(q)
        seen.append(q)
    monkeypatch.setattr(cep, "native_step", spy)
    return seen


def _buffers(q, scale):
    """name -> tensor of everything the kernel writes; the gradients times `scale` (= B: dL/df carries 1 / B, which would hide them
    under the absolute tolerance)."""
    out = {"feat": q.feat, "stats": q.stats, "G_out": q.G_out * scale, "G_act": q.G_act * scale, "G_obs": q.G_obs * scale}
    for l in range(len(q.hidden)):
        out[f"H[{l}]"], out[f"G[{l}]"] = q.H[l], q.G[l] * scale
    return out


@pytest.mark.parametrize("name", cc.TABLE)
def test_the_kernel_matches_the_float64_restatement(name, amd_lib):
    """``native_step`` against ``reference_step`` in float64 on the CPU at rtol = atol = 1e-4: feat, H_l, B G_l, B G_out, B G_act,
    B G_obs and the (B, 4) per-state scalars."""
    from cleandiffuser_amd.engine import cep
    case, inp = cc.CASES[name], cc.make_inputs(name)
    want = cc.request(cc.build(case, amd_lib, "cpu", torch.float64), *cc.tensors(inp, dtype=torch.float64))
    cep.reference_step(want)
    got = cc.request(cc.build(case, amd_lib, DEV), *cc.tensors(inp, device=DEV))
    cep.native_step(got)
    torch.cuda.synchronize()
    g, w = _buffers(got, case.B), _buffers(want, case.B)
    for what in w:
        a, b = g[what].cpu().double().numpy(), w[what].numpy()
        print(f"  {name} {what}: max|d| {float(np.abs(a - b).max()):.3e}  max|ref| {float(np.abs(b).max()):.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=what)
    if case.K == 1:
        assert all(float(g[k].abs().max()) == 0.0 for k in g if k.startswith("G")) and float(got.stats[:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("name", cc.GOLDEN_TABLE)
def test_update_matches_the_reference_fixture(name, amd_lib, monkeypatch):
    """Three ``clf.update()`` calls on the device against the real reference (tests/golden/qgpo_cep.npz): each returned dict at rtol =
    atol = 1e-4, the first step's gradients at 2e-4 x max |g_ref| per parameter, the parameter and EMA checksums after the third call at
    rtol = atol = 1e-4 -- all three served by the fused route."""
    case, gold = cc.CASES[name], cc.golden(name)
    seen = _spy_step(monkeypatch)
    clf = cc.build(case, amd_lib, DEV)
    grads, step = {}, clf.optim.step

    def spy_optim(*a, **k):
        if not grads:
            grads.update({n: p.grad.detach().cpu().numpy().copy() for n, p in cc.trainable(clf.model)})
        return step(*a, **k)
    clf.optim.step = spy_optim
    x, t, y = cc.tensors(gold, device=DEV)
    for i in range(cc.CALLS):
        log = clf.update(x, t, y, update_ema=case.update_ema)
        assert len(seen) == i + 1, "the fused route did not take this call"
        assert_log(log, gold["log"][i], f"{name} call {i}")
    if case.grads:
        assert_grads(grads, gold, name, clip_factor(case, gold))
    for module, key in ((clf.model, "sums"), (clf.model_ema, "sums_ema")):
        got = cc.checksums(module)
        print(f"  {name} {key}: max|d| {float(np.abs(got - gold[key]).max()):.3e}")
        np.testing.assert_allclose(got, gold[key], rtol=1e-4, atol=1e-4, err_msg=key)


def _shipped(amd_lib, b, k=16, seed=5):
    """The shipped network (O 17, A 6, Ec 64, 3 x 256) with a seeded batch of `b` states x `k` support actions."""
    case = cc._c(b, k, 17, 6, 64, [256, 256, 256])
    clf = cc.build(case, amd_lib, DEV)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, k, 6, generator=g).to(DEV)
    t = (1e-3 + 0.999 * torch.rand(b, generator=g)).to(DEV)
    y = {"soft_label": torch.softmax(1.5 * torch.randn(b, k, 1, generator=g), 1).to(DEV), "obs": torch.randn(b, 17, generator=g).to(DEV)}
    return clf, x, t, y


def _kernels(clf, x, t, y):
    from torch.autograd import DeviceType
    for _ in range(2):                                      # (gradient tensors, optimiser state and pointer tables are warm)
        clf.update(x, t, y)
    prof, _ = profiled(lambda: clf.update(x, t, y))
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def test_the_launch_count_does_not_grow_with_the_batch(amd_lib, monkeypatch):
    """A steady-state ``update()`` contains cdx_cep_kernel exactly once and the batched weight-gradient kernel exactly once, the same
    number of device kernels at (B, K) = (8, 16) and (64, 16), and fewer than half of what the autograd body (CDX_CEP=0) launches."""
    counts = {}
    for b in (8, 64):
        kernels = _kernels(*_shipped(amd_lib, b))
        print(f"B = {b}: {len(kernels)} device kernels on the fused route")
        assert sum("cdx_cep_kernel" in k for k in kernels) == 1, kernels
        assert sum("cdx_conv_wgrad_batch_kernel" in k for k in kernels) == 1, kernels
        counts[b] = len(kernels)
    assert counts[8] == counts[64], counts
    monkeypatch.setenv("CDX_CEP", "0")
    aten = _kernels(*_shipped(amd_lib, 8))
    print(f"B = 8: {len(aten)} device kernels on the autograd body (CDX_CEP=0), {counts[8]} on the fused route")
    assert not any("cdx_cep_kernel" in k for k in aten)
    assert 2 * counts[8] < len(aten), (counts, len(aten))


@pytest.mark.parametrize("clip", [None, 0.5])
def test_the_two_routes_agree(clip, amd_lib, monkeypatch):
    """One ``update()`` from the same weights on seeded inputs: the fused route and the autograd body (CDX_CEP=0) return the same dict
    and leave the same parameters and EMA parameters at rtol = atol = 2e-4.  lr = 1e-3 as the pipeline sets it: Adam's first step
    moves every element by about lr, five times the bar, so a parameter one route left behind fails."""
    seen = _spy_step(monkeypatch)
    fused, x, t, y = _shipped(amd_lib, 8)
    aten, _, _, _ = _shipped(amd_lib, 8)
    fused.grad_clip_norm = aten.grad_clip_norm = clip
    log = fused.update(x, t, y)
    assert len(seen) == 1
    monkeypatch.setenv("CDX_CEP", "0")
    log0 = aten.update(x, t, y)
    assert len(seen) == 1
    print(log, log0)
    assert set(log) == set(log0) and (log["grad_norm"] is None) == (clip is None)
    for k in log0:
        if log0[k] is not None:
            np.testing.assert_allclose(log[k], log0[k], rtol=2e-4, atol=2e-4, err_msg=k)
    for a, b in ((fused.model, aten.model), (fused.model_ema, aten.model_ema)):
        for (n, p), p0 in zip(a.named_parameters(), b.parameters()):
            np.testing.assert_allclose(p.detach().cpu().numpy(), p0.detach().cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=n)


@pytest.mark.parametrize("name", ["k8_ragged", "shipped_b8"])
def test_two_launches_give_the_same_bits(name, amd_lib):
    """No atomics, one fixed lane and order per element: two ``native_step`` launches on the same inputs are ``torch.equal`` in
    everything the kernel writes."""
    from cleandiffuser_amd.engine import cep
    case, inp = cc.CASES[name], cc.make_inputs(name)
    clf = cc.build(case, amd_lib, DEV)
    one, two = (cc.request(clf, *cc.tensors(inp, device=DEV)) for _ in range(2))
    cep.native_step(one)
    cep.native_step(two)
    torch.cuda.synchronize()
    a, b = _buffers(one, 1.0), _buffers(two, 1.0)
    for what in a:
        assert torch.equal(a[what], b[what]), what
