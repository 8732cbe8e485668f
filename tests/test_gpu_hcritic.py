"""The horizon critic on the MI355X: the executor (csrc/cdx_hcritic.hip behind engine/hcritic.py) against the fixture of the real
reference and against the float64 restatement of its data flow, chunking, reproducibility, the launch structure; the node route's
forward values and training steps against the fixture; the switch back to the stock modules."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcritic_cases as hc  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_BAR = 2e-4                # x max |g_ref| per parameter: the bar of tests/test_gpu_cep.py


@pytest.fixture(autouse=True)
def _routes(monkeypatch):
    monkeypatch.setenv("CDX_HCRITIC", "1")
    monkeypatch.delenv("CDX_HCRITIC_NODES", raising=False)
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)


def _spy(monkeypatch, name):
    """The calls `engine.hcritic.<name>` served."""
    from cleandiffuser_amd.engine import hcritic
    seen, real = [], getattr(hcritic, name)

    def spy(*args, **kwargs):
        seen.append(args)
        return real(*args, **kwargs)
    monkeypatch.setattr(hcritic, name, spy)
    return seen


_scored = {}


def _executor(name):
    """(values of the executor on the case's inputs, computed once; the module)."""
    if name not in _scored:
        net = hc.build(hc.critic_class("amd"), hc.CASES[name], DEV)
        with torch.no_grad():
            y = net(hc.inputs(name, DEV))
        torch.cuda.synchronize()
        _scored[name] = (y.cpu().numpy(), net)
    return _scored[name]


@pytest.mark.parametrize("name", hc.TABLE)
def test_executor_matches_the_reference_fixture(name, monkeypatch):
    """``critic(x)`` under no_grad is one ``cdx_hcritic_run`` and equals the real reference's recorded values at rtol = atol = 1e-4; the
    argmax per environment is the recorded one."""
    seen = _spy(monkeypatch, "_score")
    _scored.pop(name, None)
    y, _ = _executor(name)
    assert len(seen) == 1, "the executor did not serve the call"
    gold = hc.golden(name)
    print(f"  {name}: max|d| {float(np.abs(y - gold['y']).max()):.3e}  max|ref| {float(np.abs(gold['y']).max()):.3e}")
    assert y.shape == gold["y"].shape
    np.testing.assert_allclose(y, gold["y"], rtol=1e-4, atol=1e-4)
    if hc.CASES[name].envs:
        assert hc.argmax_per_env(y, hc.CASES[name]).tolist() == gold["argmax"].tolist()


# (in_dim, T, d_model, heads, depth, norm, B): a head dimension of 3 -- the kernel's scalar loads -- next to the table
EXTRA = {"head_dim3_post": (3, 5, 12, 4, 2, "post", 7), "head_dim3_pre_depth1": (3, 5, 12, 4, 1, "pre", 7)}


@pytest.mark.parametrize("name", hc.TABLE + list(EXTRA))
def test_executor_matches_the_float64_restatement(name):
    """The executor against ``reference_run`` in float64 on the CPU at rtol = atol = 1e-4."""
    from cleandiffuser_amd.engine import hcritic
    if name in EXTRA:
        from types import SimpleNamespace
        i, T, d, h, depth, norm, B = EXTRA[name]
        case = SimpleNamespace(in_dim=i, tokens=T, d_model=d, heads=h, depth=depth, norm=norm, batch=B, in_proj_scale=1.0)
        x = hc.array(name, "x", (B, T, i))
        net = hc.build(hc.critic_class("amd"), case, DEV)
        with torch.no_grad():
            y = net(x.to(DEV)).cpu().numpy()
    else:
        case, x = hc.CASES[name], hc.inputs(name)
        y, _ = _executor(name)
    want = hcritic.reference_run(hc.build(hc.critic_class("amd"), case, dtype=torch.float64), x.double(), torch.float64).numpy()
    print(f"  {name}: max|d| {float(np.abs(y - want).max()):.3e}  max|ref| {float(np.abs(want).max()):.3e}")
    np.testing.assert_allclose(y, want, rtol=1e-4, atol=1e-4)


def test_chunked_passes_agree_with_one_pass(monkeypatch):
    """The 33-row case with `chunk` forced to 16 -- two full passes and a ragged one -- against the unchunked result at 1e-5."""
    from cleandiffuser_amd.engine import hcritic
    one, net = _executor("ragged_pre")
    with torch.no_grad():
        y = hcritic.try_score(net, hc.inputs("ragged_pre", DEV), chunk=16)
    assert y is not None
    print(f"  chunk 16 vs one pass: max|d| {float(np.abs(y.cpu().numpy() - one).max()):.3e}")
    np.testing.assert_allclose(y.cpu().numpy(), one, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", ["ragged_pre", "limits_post", "one_token"])
def test_two_calls_give_the_same_bits(name):
    _, net = _executor(name)
    x = hc.inputs(name, DEV)
    with torch.no_grad():
        a, b = net(x).clone(), net(x).clone()
    assert torch.equal(a, b)


def _assert_steps(got, gold, what):
    assert set(got) == {k for k in gold if k in ("loss", "sums") or k.startswith("grad/")}
    for k in ("loss", "sums"):
        print(f"  {what} {k}: max|d| {float(np.abs(got[k] - gold[k]).max()):.3e}")
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
    for k in gold:
        if k.startswith("grad/"):
            ref = np.asarray(gold[k], dtype=np.float64)
            err, bar = float(np.abs(np.asarray(got[k], dtype=np.float64) - ref).max()), GRAD_BAR * float(np.abs(ref).max())
            print(f"  {what} {k}: max|d| {err:.3e}  bar {bar:.3e}")
            assert err <= bar, (what, k, err, bar)


@pytest.mark.parametrize("name", hc.TRAIN_TABLE)
def test_node_route_matches_the_reference_fixture(name, monkeypatch):
    """With autograd on the library's nodes (``CDX_HCRITIC_NODES=1``): the forward values at rtol = atol = 1e-4, three MSE / Adam steps'
    losses and parameter checksums at 1e-4, the first step's gradients at 2e-4 x max |g_ref| per parameter."""
    monkeypatch.setenv("CDX_HCRITIC_NODES", "1")
    seen = _spy(monkeypatch, "forward_nodes")
    gold = hc.golden(name)
    net = hc.build(hc.critic_class("amd"), hc.CASES[name], DEV)
    y = net(hc.inputs(name, DEV))
    assert len(seen) == 1 and y.requires_grad, "the node route did not serve the call"
    np.testing.assert_allclose(y.detach().cpu().numpy(), gold["y"], rtol=1e-4, atol=1e-4)
    del seen[:]
    got = hc.run_training(hc.critic_class("amd"), name, DEV)
    assert len(seen) == hc.STEPS
    _assert_steps(got, gold, name)


def _score_kernels(batch):
    """The device kernels of a steady-state scoring call at the 33-row case's shape (three blocks, pre-norm)."""
    from torch.autograd import DeviceType
    c = hc.CASES["ragged_pre"]
    net = hc.build(hc.critic_class("amd"), c, DEV)
    x = hc.inputs("ragged_pre", DEV)[:batch].contiguous()

    def call():
        with torch.no_grad():
            return net(x)
    for _ in range(2):
        call()
    prof, _ = profiled(call)
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def test_the_launch_structure_of_a_scoring_call():
    """The same number of device kernels at B = 5 and B = 33, every one of them the library's (no ATen kernel), the single-query
    attention exactly once."""
    counts = {}
    for batch in (5, 33):
        kernels = _score_kernels(batch)
        print(f"B = {batch}: {len(kernels)} device kernels: {sorted(set(k.replace('(anonymous namespace)::', '').split('(')[0] for k in kernels))}")
        assert kernels and all("cdx_" in k for k in kernels), [k for k in kernels if "cdx_" not in k]
        assert sum("cdx_sqattn_kernel" in k for k in kernels) == 1
        counts[batch] = len(kernels)
    assert counts[5] == counts[33], counts


def test_unasked_the_measured_defaults_serve(monkeypatch):
    """With no switch set the routes DESIGN.md 3n made the default serve: a no_grad call the executor, a call with autograd the nodes."""
    from cleandiffuser_amd.engine import hcritic
    monkeypatch.delenv("CDX_HCRITIC")
    scored, nodes = _spy(monkeypatch, "_score"), _spy(monkeypatch, "forward_nodes")
    net = hc.build(hc.critic_class("amd"), hc.CASES["one_token"], DEV)
    x = hc.inputs("one_token", DEV)
    with torch.no_grad():
        net(x)
    net(x).sum().backward()
    assert (len(scored), len(nodes)) == (int(hcritic.SCORE_DEFAULT), int(hcritic.NODES_DEFAULT))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_switched_off_the_stock_modules_run(monkeypatch):
    """``CDX_HCRITIC=0``: neither the executor nor the nodes serve; the stock modules on the device give the fixture's values."""
    monkeypatch.setenv("CDX_HCRITIC", "0")
    scored, nodes = _spy(monkeypatch, "_score"), _spy(monkeypatch, "forward_nodes")
    net = hc.build(hc.critic_class("amd"), hc.CASES["ragged_pre"], DEV)
    with torch.no_grad():
        y = net(hc.inputs("ragged_pre", DEV)).cpu().numpy()
    assert not scored and not nodes
    np.testing.assert_allclose(y, hc.golden("ragged_pre")["y"], rtol=1e-4, atol=1e-4)
