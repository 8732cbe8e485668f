"""The host logic of the training path (cleandiffuser_amd/engine/train.py) on the CPU tier: with the kernel wrappers replaced by torch
expressions of their contracts (tests/torch_blocks.py), every native training forward -- JannerUNet1d, ChiUNet1d, DiT1d, IDQLMlp,
ChiTransformer, DQLMlp, PearceMlp, SfBCUNet -- must give torch.autograd's output and gradients of the module's own PyTorch forward; gradients routed
straight into ``.grad`` (grads_in_place) must equal autograd's accumulation; the weight-layout registry must stay current across
optimiser steps with one refresh per parameter change.  (The kernels themselves: tests/test_gpu_parity.py on the MI355X.)"""
import pytest
import torch

import cleandiffuser_amd.nn_diffusion as N
from cleandiffuser_amd.engine import train
from cleandiffuser_amd.utils import load_synth
from torch_blocks import emulated


def _case(name):
    g = torch.Generator().manual_seed(11)
    if name == "janner":
        net = load_synth(N.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2, 2], kernel_size=5), 3)
        return net, train.janner_forward, (torch.randn(4, 8, 6, generator=g), torch.randint(0, 20, (4,), generator=g), None)
    if name == "janner_cond":
        net = load_synth(N.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=3), 4)
        return net, train.janner_forward, (torch.randn(3, 8, 6, generator=g), torch.randint(0, 20, (3,), generator=g), torch.randn(3, 16, generator=g))
    if name == "chiunet":
        net = load_synth(N.ChiUNet1d(2, 5, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], obs_as_global_cond=True), 5)
        return net, train.chi_forward, (torch.randn(3, 16, 2, generator=g), torch.randint(0, 20, (3,), generator=g), torch.randn(3, 2, 5, generator=g))
    if name == "dit":
        net = load_synth(N.DiT1d(7, emb_dim=32, d_model=64, n_heads=4, depth=2, timestep_emb_type="fourier"), 6)
        return net, train.dit_forward, (torch.randn(3, 16, 7, generator=g), torch.rand(3, generator=g), torch.randn(3, 32, generator=g))
    if name == "idql":
        net = load_synth(N.IDQLMlp(11, 5, emb_dim=16, hidden_dim=64, n_blocks=2, dropout=0.0), 7)
        return net, train.idql_forward, (torch.randn(6, 5, generator=g), torch.rand(6, generator=g), torch.randn(6, 11, generator=g))
    if name == "chitf":
        net = load_synth(N.ChiTransformer(3, 5, 6, 3, d_model=64, nhead=4, num_layers=2, p_drop_attn=0.0, n_cond_layers=2), 8)
        return net, train.chitf_forward, (torch.randn(4, 6, 3, generator=g), torch.randint(0, 20, (4,), generator=g), torch.randn(4, 3, 5, generator=g))
    if name == "dql":
        net = load_synth(N.DQLMlp(11, 6, emb_dim=16), 9)
        return net, train.dql_forward, (torch.randn(5, 6, generator=g), torch.randint(0, 10, (5,), generator=g), torch.randn(5, 11, generator=g))
    if name == "pearce":
        net = load_synth(N.PearceMlp(6, To=2, emb_dim=32, hidden_dim=64), 10)
        return net, train.pearce_forward, (torch.randn(7, 6, generator=g), torch.randint(0, 20, (7,), generator=g), torch.randn(7, 2, 32, generator=g))
    if name == "sfbc":
        net = load_synth(N.SfBCUNet(5, emb_dim=16, hidden_dims=[64, 32, 16]), 11)
        return net, train.sfbc_forward, (torch.randn(6, 5, generator=g), torch.rand(6, generator=g), torch.randn(6, 16, generator=g))
    if name == "chain_critic":                                # Linear -> LayerNorm -> Tanh / Mish towers (DQLCritic, IQL's TwinQ / V)
        from cleandiffuser_amd.utils import DQLCritic
        net = load_synth(DQLCritic(7, 3, hidden_dim=32), 13).q1_model
        return net, train.chain_forward, (torch.randn(6, 10, generator=g),)
    if name == "chain_invdyn":                                # Linear -> GELU -> LayerNorm -> Identity -> ... -> Tanh (active Dropout: the stock modules)
        from cleandiffuser_amd.invdynamic import FancyMlpInvDynamic
        net = FancyMlpInvDynamic(5, 3, hidden_dim=32, add_norm=True, add_dropout=False).model
        return net, train.chain_forward, (torch.randn(6, 10, generator=g),)
    if name == "chain_mlp":                                   # utils.Mlp: nested Sequential(Linear, ReLU) per hidden layer, Tanh output
        from cleandiffuser_amd.utils import Mlp
        net = load_synth(Mlp(10, [32, 32], 3, torch.nn.ReLU(), torch.nn.Tanh()), 14).mlp
        return net, train.chain_forward, (torch.randn(6, 10, generator=g),)
    if name == "half_janner":
        from cleandiffuser_amd.nn_classifier import HalfJannerUNet1d
        net = load_synth(HalfJannerUNet1d(16, 6, out_dim=1, kernel_size=3, model_dim=16, emb_dim=16, dim_mult=(1, 2, 2)), 12)
        return net, train.half_janner_forward, (torch.randn(5, 16, 6, generator=g), torch.randint(0, 20, (5,), generator=g), None)
    raise KeyError(name)


def _wgt(net, args, seed):
    """Weights of the scalar the tests differentiate: one per OUTPUT element (the classifier maps (b, H, D) to (b, out_dim))."""
    with torch.no_grad():
        shape = (net._forward_torch(*args) if hasattr(net, "_forward_torch") else net(*args)).shape
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _grads(net):
    return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}


def _reference(net, args, wgt):
    net.zero_grad(set_to_none=True)
    x = args[0].clone().requires_grad_(True)
    y = net._forward_torch(x, *args[1:]) if hasattr(net, "_forward_torch") else None
    if y is None:                                           # (modules whose forward() is the torch code once no device path applies)
        y = net(x, *args[1:])
    (y * wgt).sum().backward()
    return y.detach(), x.grad.clone(), _grads(net)


def _close(got, want, what, tol=2e-5):
    if want is None:
        assert got is None or float(got.abs().max()) == 0.0, what
        return
    assert got is not None, what
    sc = float(want.abs().max()) + 1e-12
    assert float((got - want).abs().max()) <= tol * sc + 1e-7, (what, float((got - want).abs().max()), sc)


CASES = ["janner", "janner_cond", "chiunet", "dit", "idql", "chitf", "dql", "pearce", "sfbc", "half_janner", "chain_critic", "chain_invdyn", "chain_mlp"]


@pytest.mark.parametrize("name", CASES)
def test_native_training_forward_is_the_modules_autograd_graph(name):
    net, fwd, args = _case(name)
    net.train()
    wgt = _wgt(net, args, 1)
    y0, gx0, gp0 = _reference(net, args, wgt)
    with emulated():
        for in_place in (False, True):
            net.zero_grad(set_to_none=True)
            x = args[0].clone().requires_grad_(True)
            y = fwd(net, x, *args[1:])
            if in_place:
                with train.grads_in_place():
                    (y * wgt).sum().backward()
            else:
                (y * wgt).sum().backward()
            _close(y.detach(), y0, f"{name}: output")
            _close(x.grad, gx0, f"{name}: input gradient")
            for n, g in _grads(net).items():
                _close(g, gp0[n], f"{name} (in place {in_place}): {n}")


def test_in_place_gradient_scope_covers_the_named_parameters_only(monkeypatch):
    """``grads_in_place(params)`` is a process-wide switch (autograd's worker threads run the nodes), so it names the
    parameters it is for: while agent A's update() is inside its backward, a backward over ANOTHER net -- from another thread, or a
    nested one -- keeps autograd's own accumulation (its caller may be torch.autograd.grad(), which must see the gradients); and with a
    multi-rank process group up nothing is summed in place (a DDP reducer listens on the gradient accumulators)."""
    net_a, fwd, args = _case("janner")
    net_b, _, _ = _case("janner")
    net_a.train(), net_b.train()
    wgt = _wgt(net_a, args, 1)
    _, _, want = _reference(net_b, args, wgt)
    _, _, want_a = _reference(net_a, args, wgt)
    net_a.zero_grad(set_to_none=True), net_b.zero_grad(set_to_none=True)
    slots = []
    orig = train._grad_slot
    monkeypatch.setattr(train, "_grad_slot", lambda p: (slots.append((id(p), orig(p) is not None)), orig(p))[1])
    ids_a, ids_b = {id(p) for p in net_a.parameters()}, {id(p) for p in net_b.parameters()}
    with emulated():
        with train.grads_in_place(net_a.parameters()):
            (fwd(net_b, args[0], *args[1:]) * wgt).sum().backward()          # B's backward inside A's scope: autograd accumulates
            assert slots and all(not took for i, took in slots if i in ids_b)
            for n, g in _grads(net_b).items():
                _close(g, want[n], f"outside the scope: {n}")
            slots.clear()
            (fwd(net_a, args[0], *args[1:]) * wgt).sum().backward()          # A's own: in place
            assert any(took for i, took in slots if i in ids_a)
        slots.clear()
        import torch.distributed as dist
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        net_a.zero_grad(set_to_none=True)
        with train.grads_in_place(net_a.parameters()):
            (fwd(net_a, args[0], *args[1:]) * wgt).sum().backward()
        assert slots and not any(took for _, took in slots)
    for n, g in _grads(net_a).items():
        _close(g, want_a[n], f"under a process group: {n}")


@pytest.mark.parametrize("name", ["janner", "chiunet", "chitf", "pearce"])
def test_in_place_gradient_sums_accumulate_and_leave_hooked_or_frozen_parameters_to_autograd(name):
    net, fwd, args = _case(name)
    net.train()
    wgt = torch.randn(args[0].shape, generator=torch.Generator().manual_seed(2))
    _, _, gp0 = _reference(net, args, wgt)
    params = dict(net.named_parameters())
    trained = [n for n, g in gp0.items() if g is not None]
    frozen, hooked = trained[1], trained[-1]
    params[frozen].requires_grad_(False)
    fired = []
    params[hooked].register_hook(lambda g: fired.append(1))
    seeds = {n: torch.randn(p.shape, generator=torch.Generator().manual_seed(3)) for n, p in params.items()}
    with emulated():
        for n, p in params.items():
            p.grad = None if n == frozen else seeds[n].clone()
        versions = {n: p.grad._version for n, p in params.items() if p.grad is not None}
        with train.grads_in_place():
            (fwd(net, args[0], *args[1:]) * wgt).sum().backward()
    assert len(fired) == 1 and params[frozen].grad is None
    for n in trained:
        if n != frozen:
            _close(params[n].grad - seeds[n], gp0[n], f"{name}: {n}")
            assert params[n].grad._version > versions[n], n          # FusedAdamW tells a written gradient by its version
    # outside update(): nothing touches .grad, the functional API gets the tensors
    params[frozen].requires_grad_(True)
    net.zero_grad(set_to_none=True)
    with emulated():
        got = torch.autograd.grad((fwd(net, args[0], *args[1:]) * wgt).sum(), [params[n] for n in trained])
    assert all(p.grad is None for p in params.values())
    for n, g in zip(trained, got):
        _close(g, gp0[n], f"{name}: autograd.grad {n}")


@pytest.mark.parametrize("name", ["janner", "chiunet", "chitf", "dit"])
def test_weight_layouts_are_refreshed_once_per_parameter_change(name, monkeypatch):
    net, fwd, args = _case(name)
    net.train()
    wgt = torch.randn(args[0].shape, generator=torch.Generator().manual_seed(4))
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    with emulated() as counts:
        seen = []
        for step in range(4):
            _, _, gp0 = _reference(net, args, wgt)
            net.zero_grad(set_to_none=True)
            before = dict(counts)
            with train.grads_in_place():
                (fwd(net, args[0], *args[1:]) * wgt).sum().backward()
            seen.append((counts["aten_pack"] - before["aten_pack"], counts["relayout"] - before["relayout"]))
            for n, g in _grads(net).items():
                _close(g, gp0[n], f"{name} step {step}: {n}")
            if step != 2:
                opt.step()                                  # (no step between passes 2 and 3: nothing at all may be launched)
        assert seen[0][0] > 0 and seen[0][1] == 0 and seen[1] == (0, 1) and seen[2] == (0, 1) and seen[3] == (0, 0), seen
        # moved parameters (module.to / a re-created tensor): the table is rebuilt from scratch, never read through stale addresses
        for p in net.parameters():
            p.data = p.data.clone()
        _, _, gp0 = _reference(net, args, wgt)
        net.zero_grad(set_to_none=True)
        before = dict(counts)
        (fwd(net, args[0], *args[1:]) * wgt).sum().backward()
        assert counts["aten_pack"] - before["aten_pack"] == seen[0][0] and counts["relayout"] == before["relayout"]
        for n, g in _grads(net).items():
            _close(g, gp0[n], f"{name} after the move: {n}")
    monkeypatch.setenv("CDX_TRAIN_PACKS", "0")
    with emulated() as counts:
        net.zero_grad(set_to_none=True)
        (fwd(net, args[0], *args[1:]) * wgt).sum().backward()
        assert counts["relayout"] == 0 and counts["aten_pack"] == seen[0][0]


def test_a_copied_module_starts_with_an_empty_layout_registry():
    """``deepcopy(model)`` (how every agent builds its EMA twin) and pickling must not carry the registry over: it names addresses of the
    ORIGINAL module's parameters and buffers."""
    import copy
    import pickle
    net, fwd, args = _case("janner")
    net.train()
    with emulated():
        fwd(net, args[0], *args[1:]).sum().backward()
        assert net._cdx_weight_packs.entries
        twin = copy.deepcopy(net)
        assert not twin._cdx_weight_packs.entries and twin._cdx_weight_packs.sig is None
        thawed = pickle.loads(pickle.dumps(net))
        assert not thawed._cdx_weight_packs.entries
        y0, y1 = fwd(net, args[0], *args[1:]), fwd(twin, args[0], *args[1:])       # and the twin builds its own
        assert torch.equal(y0, y1) and twin._cdx_weight_packs.entries
        assert all(k not in net._cdx_weight_packs.entries for k in twin._cdx_weight_packs.entries)


def _chain(x, y_up):
    """net_down's input: the sample, moved by net_up's output (broadcast where that net maps a sequence to one number per sample)."""
    return x + 0.1 * y_up.reshape(y_up.shape + (1,) * (x.dim() - y_up.dim()))


def _nested_graph(nets, fwds, args, wgts, n_nested):
    """net_up -> a node whose backward() runs `n_nested` complete forward + backward passes of net_mid -> net_down, then .backward()."""
    up, mid, down = nets

    class Nested(torch.autograd.Function):
        @staticmethod
        def forward(ctx, h):
            return h.clone()

        @staticmethod
        def backward(ctx, g):
            with torch.enable_grad():
                for _ in range(n_nested):
                    (fwds[1](mid, args[0].clone().requires_grad_(True), *args[1:]) * wgts[1]).sum().backward()
            return g

    y_up = fwds[0](up, args[0].clone().requires_grad_(True), *args[1:])
    y = fwds[2](down, Nested.apply(_chain(args[0], y_up)), *args[1:])
    (y * wgts[2]).sum().backward()


@pytest.mark.parametrize("batched", ["1", "0"])
@pytest.mark.parametrize("n_nested", [0, 1, 5])
@pytest.mark.parametrize("name", ["janner", "janner_cond", "half_janner"])
def test_a_reentrant_backward_keeps_every_queued_weight_gradient(name, n_nested, batched, monkeypatch):
    """a backward pass that runs inside another one's node (a re-entrant pass: gradient penalties, a guidance term computed
    in backward()) opens weight-gradient queues of its own.  The outer pass's queue -- filled half by net_down before the nested passes,
    half by net_up after them -- must survive them and be flushed once, whatever ids autograd gives the passes."""
    monkeypatch.setenv("CDX_TRAIN_WGRAD_BATCH", batched)
    nets = [_case(name)[0].train() for _ in range(3)]
    for i, net in enumerate(nets):                          # (three different nets: same architecture, different weights)
        load_synth(net, 20 + i)
    _, fwd, args = _case(name)
    wgts = [_wgt(net, args, 30 + i) for i, net in enumerate(nets)]
    torch_fwd = lambda net, *a: net._forward_torch(*a) if hasattr(net, "_forward_torch") else net(*a)      # noqa: E731
    for net in nets:
        net.zero_grad(set_to_none=True)
    _nested_graph(nets, [torch_fwd] * 3, args, wgts, n_nested)
    want = [_grads(net) for net in nets]
    assert any(g is not None for g in want[0].values()) and any(g is not None for g in want[2].values())
    for net in nets:
        net.zero_grad(set_to_none=True)
    with emulated():
        with train.grads_in_place():
            _nested_graph(nets, [fwd] * 3, args, wgts, n_nested)
        assert not train._wgrad_queues
    for which, net, ref in zip(("net_up", "net_mid", "net_down"), nets, want):
        for n, g in _grads(net).items():
            _close(g, ref[n], f"{name}, {n_nested} nested passes: {which}.{n}")


def test_a_backward_pass_that_raises_leaves_no_weight_gradient_queue_behind():
    """The end-of-pass callback of a pass that raised never runs: what it had queued is dropped when its grads_in_place() scope closes,
    nothing of it reaches the next step's gradients."""
    net, fwd, args = _case("janner")
    net.train()
    wgt = _wgt(net, args, 1)
    _, _, want = _reference(net, args, wgt)

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, h):
            return h.clone()

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("boom")

    with emulated() as counts:
        net.zero_grad(set_to_none=True)
        before = counts.get("wgrad_batch", 0)
        with pytest.raises(RuntimeError, match="boom"):
            with train.grads_in_place():
                y = fwd(net, Boom.apply(fwd(net, args[0], *args[1:])), *args[1:])      # the second application queues, then Boom raises
                try:
                    (y * wgt).sum().backward()
                finally:
                    assert train._wgrad_queues             # (the failed pass had queued products: the case is not vacuous)
        assert not train._wgrad_queues and counts.get("wgrad_batch", 0) == before
        net.zero_grad(set_to_none=True)
        with train.grads_in_place():
            (fwd(net, args[0], *args[1:]) * wgt).sum().backward()
        assert not train._wgrad_queues
    for n, g in _grads(net).items():
        _close(g, want[n], f"the step after a failed pass: {n}")
