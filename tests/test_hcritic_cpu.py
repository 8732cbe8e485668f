"""The horizon critic (utils/critics.py:DVHorizonCritic, engine/hcritic.py) without a GPU: the mirror against the real reference's recorded
outputs, names and training steps, the plain-torch restatement of the executor's pruned data flow against the module in float64, the
workspace plan against the C side, the refusals of the scoring route."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcritic_cases as hc  # noqa: E402

TOL = 2e-6


def _stock(critic, x, monkeypatch):
    with monkeypatch.context() as m:
        m.setenv("CDX_HCRITIC", "0")
        m.setenv("CDX_HCRITIC_NODES", "0")
        return critic(x)


@pytest.mark.parametrize("norm", ["post", "pre"])
def test_mirror_equals_the_module_fixture(norm):
    """``head/DVHorizonCritic/{post,pre}`` of tests/golden/modules.npz, recorded from the real reference, with the recipe of
    oracle/gen_module_golden.py:head_outputs."""
    from cleandiffuser_amd.utils.critics import DVHorizonCritic
    from cleandiffuser_amd.utils.synth import synth_array, synth_state_dict
    gold = np.load(os.path.join(ROOT, "tests", "golden", "modules.npz"))
    net = DVHorizonCritic(5, 16, d_model=32, n_heads=4, depth=2, norm_type=norm)
    net.load_state_dict(synth_state_dict(net.state_dict(), 5))
    traj = torch.from_numpy(synth_array("head/traj", (4, 6, 5)))
    with torch.no_grad():
        y = net.eval()(traj).numpy()
    assert y.shape == (4, 1)
    np.testing.assert_allclose(y, gold[f"head/DVHorizonCritic/{norm}"], rtol=TOL, atol=TOL)


def test_the_package_namespace_does_not_export_the_critic():
    """oracle/gen_module_golden.py:head_outputs probes ``hasattr(utils, "DVHorizonCritic")`` and tests/test_module_mirrors.py pins the names it
    yields: the import path is ``cleandiffuser_amd.utils.critics``."""
    import cleandiffuser_amd.utils as U
    from cleandiffuser_amd.utils import building_blocks, critics
    assert not hasattr(U, "DVHorizonCritic")
    assert building_blocks.DVHorizonCritic is critics.DVHorizonCritic


@pytest.mark.parametrize("name", hc.TABLE)
def test_mirror_equals_the_reference_over_the_table(name):
    gold = hc.golden(name)
    net = hc.build(hc.critic_class("amd"), hc.CASES[name])
    with torch.no_grad():
        y = net(hc.inputs(name)).numpy()
    np.testing.assert_allclose(y, gold["y"], rtol=TOL, atol=TOL)
    if hc.CASES[name].envs:
        assert hc.argmax_per_env(y, hc.CASES[name]).tolist() == gold["argmax"].tolist()


@pytest.mark.parametrize("name", hc.TABLE)
def test_state_dict_is_the_checkpoint_contract(name):
    """Key names, order and shapes as the reference's class reports them; a ``load_state_dict`` round trip reproduces the output."""
    cls, case = hc.critic_class("amd"), hc.CASES[name]
    net = hc.build(cls, case)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == hc.golden_keys()[name]
    fresh = cls(case.in_dim, 16, d_model=case.d_model, n_heads=case.heads, depth=case.depth, norm_type=case.norm).eval()
    assert all(float(m.bias.detach().abs().max()) == 0.0 for m in fresh.modules() if isinstance(m, torch.nn.Linear))
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(hc.inputs(name)), net(hc.inputs(name)))
    assert fresh.pos_emb_cache.shape == (case.tokens, case.d_model) and "pos_emb_cache" not in dict(fresh.named_buffers())
    with torch.no_grad():
        fresh(hc.inputs(name)[:, :max(case.tokens - 1, 1)])
    assert fresh.pos_emb_cache.shape[0] == max(case.tokens - 1, 1)               # rebuilt when the token count changes


def test_unknown_norm_type_raises():
    cls = hc.critic_class("amd")
    with pytest.raises(NotImplementedError):
        cls(5, 16, d_model=32, n_heads=4, depth=1, norm_type="sandwich")(torch.zeros(2, 3, 5))


@pytest.mark.parametrize("name", hc.TABLE)
def test_restatement_equals_the_module_in_float64(name):
    """``reference_run`` -- sliced in_proj rows, token-0 rows in place, one row per trajectory behind the last attention -- against the
    module's own forward, both in float64, at 1e-10; the table holds both norm orders."""
    from cleandiffuser_amd.engine import hcritic
    net = hc.build(hc.critic_class("amd"), hc.CASES[name], dtype=torch.float64)
    x = hc.inputs(name, dtype=torch.float64)
    with torch.no_grad():
        want = net(x)
    got = hcritic.reference_run(net, x, torch.float64)
    assert got.shape == want.shape == (hc.CASES[name].batch, 1)
    assert float((got - want).abs().max()) <= 1e-10
    assert {hc.CASES[n].norm for n in hc.TABLE} == {"pre", "post"}


def _assert_steps(got: dict, gold: dict, what, loss_tol=1e-5, grad_bar=2e-5, sums_tol=1e-5):
    assert set(got) == {k for k in gold if k == "loss" or k == "sums" or k.startswith("grad/")}
    for k in ("loss", "sums"):
        scale = float(np.abs(gold[k]).max())
        err = float(np.abs(got[k] - gold[k]).max())
        assert err <= (loss_tol if k == "loss" else sums_tol) * scale, (what, k, err, scale)
    for k in gold:
        if k.startswith("grad/"):
            ref = np.asarray(gold[k], dtype=np.float64)
            err, bar = float(np.abs(np.asarray(got[k], dtype=np.float64) - ref).max()), grad_bar * float(np.abs(ref).max())
            assert err <= bar, (what, k, err, bar)


@pytest.mark.parametrize("name", hc.TRAIN_TABLE)
def test_training_steps_on_the_stock_route_match_the_reference(name):
    """Three MSE / Adam steps: losses and parameter checksums at 1e-5 of their scale, first-step gradients at 2e-5 x max |g_ref| (the
    bars of tests/test_tower_cpu.py)."""
    _assert_steps(hc.run_training(hc.critic_class("amd"), name), hc.golden(name), name)


def _c_side():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import bigbatch, hcritic
    return hcritic, bigbatch, hcritic._lib()


def test_workspace_plan_matches_the_c_side():
    """``hcritic.workspace_floats`` == ``cdx_hcritic_workspace_floats`` over tokens, widths, depths, batches and chunks (0: the library's
    rule, a chunk beyond the batch, a ragged last pass); the first sizes past the limits are refused on both sides."""
    hcritic, bigbatch, lib = _c_side()
    seen = set()
    for T, (d, heads), depth, batch, chunk in itertools.product((1, 4, 17, 40, 64), ((32, 4), (36, 3), (256, 8), (1024, 16)), (1, 2, 5),
                                                                (0, 1, 33, 2500, 7500), (0, 1, 16, 4096)):
        w = bigbatch.CdxHcriticWeights(tokens=T, in_dim=7, d_model=d, n_heads=heads, depth=depth, pre_norm=1, eps=1e-6)
        got = lib.cdx_hcritic_workspace_floats(ctypes.byref(w), batch, chunk)
        assert hcritic.within_limits(T, d, heads, depth)
        assert got == hcritic.workspace_floats(T, d, depth, batch, chunk), (T, d, depth, batch, chunk, got)
        seen.add(got)
    assert len(seen) > 100 and 0 in seen
    for T, d, heads, depth, word in ((65, 32, 4, 2, b"tokens"), (0, 32, 4, 2, b"tokens"), (8, 1028, 257, 2, b"d_model"), (8, 130, 2, 2, b"head"),
                                     (8, 32, 5, 2, b"n_heads"), (8, 32, 4, 0, b"depth")):
        w = bigbatch.CdxHcriticWeights(tokens=T, in_dim=7, d_model=d, n_heads=heads, depth=depth, pre_norm=0, eps=1e-6)
        assert not hcritic.within_limits(T, d, heads, depth)
        assert lib.cdx_hcritic_workspace_floats(ctypes.byref(w), 8, 0) == -1 and word in lib.cdx_last_error(), (T, d, heads, depth)
        assert lib.cdx_hcritic_run(ctypes.byref(w), 8, 8, 8, 0, 8, 1 << 40, None) == -1 and word in lib.cdx_last_error()
    w = bigbatch.CdxHcriticWeights(tokens=8, in_dim=7, d_model=32, n_heads=4, depth=2, pre_norm=0, eps=1e-6)
    assert lib.cdx_hcritic_workspace_floats(None, 8, 0) == -1 and b"null" in lib.cdx_last_error()
    assert lib.cdx_hcritic_run(ctypes.byref(w), None, None, 0, 0, None, 0, None) == 0                     # an empty batch is not an error
    assert lib.cdx_hcritic_run(ctypes.byref(w), 8, 8, 4, 0, 8, 1 << 40, None) == -1 and b"null pointer" in lib.cdx_last_error()
    assert lib.cdx_hcritic_workspace_floats(ctypes.byref(w), 8, -1) == -1 and b"negative" in lib.cdx_last_error()
    big = bigbatch.CdxHcriticWeights(tokens=64, in_dim=7, d_model=1024, n_heads=16, depth=2, pre_norm=0, eps=1e-6)
    assert lib.cdx_hcritic_workspace_floats(ctypes.byref(big), 1 << 20, 1 << 20) == -1 and b"chunk too large" in lib.cdx_last_error()


def test_mirrors_have_the_c_layout(tmp_path):
    """``CdxHcriticBlock`` / ``CdxHcriticWeights`` == the structs of include/cdx.h (gcc sizeof / offsetof); the entries were additive: the
    header's ABI number is unchanged."""
    from cleandiffuser_amd.engine import bigbatch
    mirrors = {"cdx_hcritic_block": bigbatch.CdxHcriticBlock, "cdx_hcritic_weights": bigbatch.CdxHcriticWeights}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){', 'printf("%d\\n", CDX_ABI_VERSION);']
    for cname, mirror in mirrors.items():
        src.append(f'printf("%zu\\n", sizeof({cname}));')
        src += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src += ['return 0;}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert int(next(out)) == 19
    for cname, mirror in mirrors.items():
        assert int(next(out)) == ctypes.sizeof(mirror), cname
        for f in mirror._fields_:
            assert getattr(mirror, f[0]).offset == int(next(out)), (cname, f[0])


def _patch_to_cpu(monkeypatch, hcritic, served):
    """``try_score`` as on the device, with the C call replaced by its restatement."""
    def fake(critic, x, chunk):
        served.append((tuple(x.shape), chunk))
        return hcritic.reference_run(critic, x, torch.float32)
    monkeypatch.setattr(hcritic, "_on_device", lambda x, params: True)
    monkeypatch.setattr(hcritic, "_score", fake)
    monkeypatch.setenv("CDX_HCRITIC", "1")
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)
    monkeypatch.setenv("CDX_HCRITIC_NODES", "0")               # (no device here: a call with autograd goes on to the stock modules)


def test_every_refusal_returns_none_and_the_stock_modules_answer(monkeypatch):
    """Each refusal of the list: ``try_score`` answers None before the (replaced) executor is reached, and the module's forward then
    gives the stock result."""
    from cleandiffuser_amd.engine import hcritic
    from cleandiffuser_amd.utils.critics import DVHorizonCritic
    served = []
    _patch_to_cpu(monkeypatch, hcritic, served)
    case = hc.CASES["full_tile_post"]
    net, x = hc.build(DVHorizonCritic, case).requires_grad_(False), hc.inputs("full_tile_post")
    want = _stock(net, x, monkeypatch)
    y = net(x)                                                                   # the accepted request
    assert len(served) == 1 and served[0] == ((16, 6, 5), 0) and y.shape == (16, 1)
    torch.testing.assert_close(y, want, rtol=1e-5, atol=1e-5)
    assert hcritic.try_score(net, x, chunk=7) is not None and served[-1][1] == 7
    net.requires_grad_(True)
    with torch.no_grad():                                                        # grad mode off: parameters that train do not matter
        assert hcritic.try_score(net, x) is not None
    del served[:]

    def refused(critic, inp, check_forward=True):
        assert hcritic.try_score(critic, inp) is None and not served
        if check_forward:
            stock = _stock(critic, inp, monkeypatch)
            got = critic(inp)
            assert not served
            torch.testing.assert_close(got, stock, rtol=0, atol=0)
    refused(net, x)                                                              # a parameter wants a gradient
    net.requires_grad_(False)
    refused(net, x.clone().requires_grad_(True))                                 # the input wants one
    monkeypatch.setenv("CDX_HCRITIC", "0")
    refused(net, x)
    monkeypatch.delenv("CDX_HCRITIC")
    assert (hcritic.try_score(net, x) is not None) == hcritic.SCORE_DEFAULT      # unset: what DESIGN.md 3n decided
    del served[:]
    monkeypatch.setenv("CDX_HCRITIC", "1")
    monkeypatch.setattr(hcritic, "_on_device", lambda x, params: x.is_cuda)
    refused(net, x)                                                              # not a ROCm device
    monkeypatch.setattr(hcritic, "_on_device", lambda x, params: True)
    refused(net.double(), x.double())                                            # not fp32
    refused(net, x, check_forward=False)                                         # (float64 parameters)
    net.float()
    refused(net, x.double(), check_forward=False)
    refused(net, x.transpose(0, 1).contiguous().transpose(0, 1))                 # not contiguous
    refused(net, x[:0], check_forward=False)                                     # B == 0
    refused(net, x[:, :, :4], check_forward=False)                               # another input width
    refused(net, x[0], check_forward=False)                                      # no batch dimension
    refused(net, torch.zeros(2, 65, 5))                                          # T > 64
    wide = DVHorizonCritic(5, 16, d_model=130, n_heads=2, depth=1).requires_grad_(False).eval()
    refused(wide, x)                                                             # head dimension 65
    huge = DVHorizonCritic(5, 16, d_model=1040, n_heads=20, depth=1).requires_grad_(False).eval()
    refused(huge, x[:2])                                                         # d_model > 1024
    dropping = DVHorizonCritic(5, 16, d_model=32, n_heads=4, depth=1, dropout=0.1).requires_grad_(False)
    assert hcritic.try_score(dropping.train(), x) is None and not served         # active dropout
    assert hcritic.try_score(dropping.eval(), x) is not None and len(served) == 1
    assert hcritic.try_score(net.train(), x) is not None                         # train mode without dropout is fine
    del served[:]

    class Mine(DVHorizonCritic):
        pass
    refused(Mine(5, 16, d_model=32, n_heads=4, depth=1).requires_grad_(False).eval(), x)      # a subclass may compute something else
    mixed = DVHorizonCritic(5, 16, d_model=32, n_heads=4, depth=2).requires_grad_(False).eval()
    mixed.blocks[1].norm_type = "pre"
    refused(mixed, x)                                                            # blocks of two norm orders


def test_node_route_is_asked_only_with_autograd(monkeypatch):
    """``supports_nodes``: a ROCm device, a gradient wanted, ``CDX_TRAIN_NATIVE`` and ``CDX_HCRITIC_NODES``."""
    from cleandiffuser_amd.engine import hcritic
    from cleandiffuser_amd.utils.critics import DVHorizonCritic
    net, x = hc.build(DVHorizonCritic, hc.CASES["one_token"]), hc.inputs("one_token")
    monkeypatch.setenv("CDX_HCRITIC_NODES", "1")
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)
    assert not hcritic.supports_nodes(net, x)                                    # on the CPU
    monkeypatch.setattr(hcritic, "_on_device", lambda x, params: True)
    assert hcritic.supports_nodes(net, x)
    with torch.no_grad():
        assert not hcritic.supports_nodes(net, x)
    for var in ("CDX_HCRITIC_NODES", "CDX_TRAIN_NATIVE"):
        monkeypatch.setenv(var, "0")
        assert not hcritic.supports_nodes(net, x)
        monkeypatch.setenv(var, "1")
    monkeypatch.delenv("CDX_HCRITIC_NODES")
    assert hcritic.supports_nodes(net, x) == hcritic.NODES_DEFAULT
