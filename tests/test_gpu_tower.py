"""The critics' fused towers on the MI355X (csrc/cdx_tower.hip behind engine/tower.py): the two kernels' buffers against the float64
restatements, the fused route against the node route, the critic steps of the shipped loops against the fixture of the real reference,
the launch structure, reproducibility."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_steps as cs  # noqa: E402
import tower_cases as tc  # noqa: E402
from gpu_profile import profiled  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_BAR = 2e-4                # x max |g_ref| per parameter: the bar of tests/test_gpu_cep.py


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    monkeypatch.delenv("CDX_TOWER", raising=False)
    monkeypatch.delenv("CDX_TRAIN_NATIVE", raising=False)


def _spy_forward(monkeypatch):
    """The requests the forward kernel served."""
    from cleandiffuser_amd.engine import tower
    seen, real = [], tower.native_forward

    def spy(q):
        real(q)
        seen.append(q)
    monkeypatch.setattr(tower, "native_forward", spy)
    return seen


def _run(tower, case, device, dtype, native):
    """Forward and backward of a case through the kernels (`native`) or their restatements -> the request with every buffer filled."""
    towers = tc.build(case, dtype=dtype, device=device)
    x, g_out = tc.make_inputs(case)
    q = tc.request(tower, towers, x.to(device=device, dtype=dtype))
    (tower.native_forward if native else tower.reference_forward)(q)
    tower.add_backward(q, [g.to(device=device, dtype=dtype) for g in g_out], want_gx=case.x_grad, want_params=not case.frozen)
    (tower.native_backward if native else tower.reference_backward)(q)
    return q


def _buffers(q, scale):
    """name -> tensor of everything the two kernels write; the gradients times `scale` (= R: g_out carries 1 / R, which would hide them
    under the absolute tolerance)."""
    out = {}
    for t in range(q.n_towers):
        out[f"out[{t}]"] = q.out[t]
        for l, norm in enumerate(q.norm):
            if l < len(q.width) - 1:
                out[f"H[{t}][{l}]"] = q.H[t][l]
            out[f"P[{t}][{l}]"] = q.P[t][l]
            if norm:
                out[f"rstd[{t}][{l}]"] = q.rstd[t][l]
            if q.want_params:
                out[f"G[{t}][{l}]"] = q.G[t][l] * scale
                if norm:
                    out[f"Sb[{t}][{l}]"], out[f"Sg[{t}][{l}]"] = q.Sb[t][l] * scale, q.Sg[t][l] * scale
        if q.want_gx:
            out[f"g_x[{t}]"] = q.g_x[t] * scale
    return out


def _assert_kernels_match_float64(name, case):
    from cleandiffuser_amd.engine import tower
    want = _run(tower, case, "cpu", torch.float64, native=False)
    got = _run(tower, case, DEV, torch.float32, native=True)
    torch.cuda.synchronize()
    g, w = _buffers(got, case.rows), _buffers(want, case.rows)
    assert list(g) == list(w)
    for what in w:
        a, b = g[what].cpu().double().numpy(), w[what].numpy()
        print(f"  {name} {what}: max|d| {float(np.abs(a - b).max()):.3e}  max|ref| {float(np.abs(b).max()):.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-4, err_msg=what)


@pytest.mark.parametrize("name", tc.TABLE)
def test_the_kernels_match_the_float64_restatements(name):
    """``native_forward`` / ``native_backward`` against ``reference_forward`` / ``reference_backward`` in float64 on the CPU at rtol = atol =
    1e-4: out, H_l, P_l, rstd_l, R G_l, R Sb_l, R Sg_l and R g_x of every tower."""
    _assert_kernels_match_float64(name, tc.CASES[name])


# below 48 KiB, 50.5 KiB, below 48 KiB again, 64.5 KiB (the largest plan two images [16][512 + 4] can make)
HIGH_WATER = [("twinq_like_r16_k20", None), ("w400_r17_k20", tc._c(17, 20, [400, 1], ["mish", None])), ("v_like_r1_k32", None),
              ("limits_r17_k512", None)]


def _high_water_sequence():
    """(run in a process of its own) the requests of HIGH_WATER in order, each against float64."""
    from cleandiffuser_amd.engine import tower
    for name, case in HIGH_WATER:
        case = tc.CASES[name] if case is None else case
        towers = tc.build(case)
        print(name, "LDS bytes", tower.lds_bytes(tower.describe(towers[0])))
        _assert_kernels_match_float64(name, case)


def test_the_lds_attribute_follows_the_largest_request_of_the_process():
    """``ro_launch_tiles`` raises the kernel's dynamic-LDS attribute only past its own high-water mark, which lives as long as the
    process: a fresh process runs, on both tower kernels, a request below 48 KiB, one of 50.5 KiB, one below 48 KiB again and then one of
    64.5 KiB -- each equal to its float64 reference at rtol = atol = 1e-4."""
    import subprocess
    from cleandiffuser_amd.engine import tower
    sizes = [tower.lds_bytes(tower.describe(tc.build(tc.CASES[n] if c is None else c)[0])) for n, c in HIGH_WATER]
    assert sizes[0] < 48 * 1024 < sizes[1] < sizes[3] and sizes[2] < 48 * 1024 and sizes[3] == 2 * 16 * 516 * 4, sizes
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_tower as t; t._high_water_sequence()"], cwd=here, env=env, capture_output=True,
                         text=True, timeout=300)
    print(out.stdout[-4000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert [line.split()[0] for line in out.stdout.splitlines() if "LDS bytes" in line] == [n for n, _ in HIGH_WATER]


@pytest.mark.parametrize("name", ["twinq_like_r16_k20", "limits_r17_k512"])
def test_weights_off_16_byte_alignment_give_the_aligned_results(name, monkeypatch):
    """K a multiple of 4 in every layer, so only the base address turns the float4 weight loads off: with every Linear weight at element
    offset 1 of a flat buffer ``try_tower`` takes the request, and outputs, g_x and every parameter gradient equal the aligned run to
    1e-6 relative."""
    from cleandiffuser_amd.engine import tower
    monkeypatch.setenv("CDX_TOWER", "1")
    seen = _spy_forward(monkeypatch)
    case = tc.CASES[name]
    assert case.k0 % 4 == 0 and all(w % 4 == 0 for w in case.widths[:-1])
    x0, g_out = tc.make_inputs(case)
    runs = []
    for unaligned in (False, True):
        towers = tc.build(case, device=DEV)
        for seq in towers if unaligned else []:
            tc.repoint_off_alignment(seq)
        x = x0.to(DEV).requires_grad_(True)
        outs = tower.try_tower(towers, x)
        assert outs is not None and len(seen) == 1 + unaligned, "the fused route did not take this request"
        sum((o * g.to(DEV)).sum() for o, g in zip(outs, g_out)).backward()
        torch.cuda.synchronize()
        got = {f"out[{t}]": o.detach().clone() for t, o in enumerate(outs)}
        got["g_x"] = x.grad.clone()
        got.update({f"{t}.{n}": p.grad.clone() for t, seq in enumerate(towers) for n, p in seq.named_parameters()})
        runs.append(got)
    assert set(runs[0]) == set(runs[1])
    for n, want in runs[0].items():
        err, scale = float((runs[1][n] - want).abs().max()), float(want.abs().max())
        print(f"  {name} {n}: max|d| {err:.3e}, max|aligned| {scale:.3e}")
        assert scale > 0 and err <= 1e-6 * scale, (n, err, scale)


@pytest.mark.parametrize("name", ["dql_like_r17_k7", "unequal_r33", "depth6_r17"])
def test_two_launch_pairs_give_the_same_bits(name):
    """No atomics, one fixed lane and order per element: two forward and backward launch pairs on the same inputs are ``torch.equal`` in
    everything the kernels write."""
    from cleandiffuser_amd.engine import tower
    case = tc.CASES[name]
    one, two = (_run(tower, case, DEV, torch.float32, native=True) for _ in range(2))
    torch.cuda.synchronize()
    a, b = _buffers(one, 1.0), _buffers(two, 1.0)
    for what in a:
        assert torch.equal(a[what], b[what]), what


def test_column_sums_in_one_launch():
    """``cdx_colsum_batch_f32`` against torch: jobs of different shapes (more than one 64-row slice, a ragged column tile, a strided
    source, an empty job), added on top of what `out` holds."""
    from cleandiffuser_amd.engine import tower
    g = torch.Generator().manual_seed(1)
    srcs = [torch.randn(r, c, generator=g).to(DEV) for r, c in ((1, 1), (3, 48), (130, 65), (64, 256), (0, 16))]
    srcs.append(torch.randn(70, 40, generator=g).to(DEV)[:, :33])
    outs = [torch.full((s.shape[1],), 0.5, device=DEV) for s in srcs]
    assert tower.column_sums(list(zip(srcs, outs))) == 1
    for s, o in zip(srcs, outs):
        np.testing.assert_allclose(o.cpu().numpy(), 0.5 + s.double().sum(0).cpu().numpy(), rtol=1e-5, atol=1e-5)


def _critic_call(kind, amd_lib, rows=24, seed=3):
    """(module, parameters that train, inputs that take a gradient, loss()) of the three critic calls the routes are compared on."""
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V, load_synth
    g = torch.Generator().manual_seed(seed)
    obs, act = torch.randn(rows, 17, generator=g).to(DEV), torch.randn(rows, 6, generator=g).tanh().to(DEV)
    target = torch.randn(rows, 1, generator=g).to(DEV)
    if kind == "twinq_mse":
        m = load_synth(TwinQ(17, 6, hidden_dim=64), 5).to(DEV)

        def loss():
            q1, q2 = m.both(obs, act)
            return ((q1 - target) ** 2 + (q2 - target) ** 2).mean()
        return m, list(m.parameters()), [], loss
    if kind == "v_expectile":
        m = load_synth(V(17, hidden_dim=64), 6).to(DEV)

        def loss():
            adv = target - m(obs)
            return (torch.abs(0.7 - (adv < 0).float()) * adv ** 2).mean()
        return m, list(m.parameters()), [], loss
    m = load_synth(DQLCritic(17, 6, hidden_dim=64), 7).to(DEV).requires_grad_(False)
    act.requires_grad_(True)

    def loss():
        q1, q2 = m(obs, act)
        return -q1.mean() / q2.abs().mean().detach()
    return m, [], [act], loss


@pytest.mark.parametrize("kind", ["twinq_mse", "v_expectile", "dql_frozen"])
def test_the_two_routes_agree(kind, amd_lib, monkeypatch):
    """From the same weights and inputs the fused route (CDX_TOWER=1) and the node route (CDX_TOWER=0) give the loss and every gradient
    within rtol = atol = 2e-4; a spy on the launch function shows which route served the call, and which one does unasked."""
    seen = _spy_forward(monkeypatch)
    results = []
    _critic_call(kind, amd_lib)[3]().backward()
    assert len(seen) == (1 if kind == "dql_frozen" else 0), "unasked, DQLCritic's calls take the fused route and TwinQ's / V's do not"
    del seen[:]
    for route in ("fused", "nodes"):
        monkeypatch.setenv("CDX_TOWER", "1" if route == "fused" else "0")
        _, params, inputs, loss = _critic_call(kind, amd_lib)
        value = loss()
        value.backward()
        assert len(seen) == 1, f"{route}: the forward kernel served {len(seen)} calls"
        assert seen[0].n_towers == (1 if kind == "v_expectile" else 2)
        results.append((float(value.detach()), [t.grad.detach().cpu().numpy() for t in params + inputs]))
    (a, ga), (b, gb) = results
    print(f"  {kind}: loss {a:.7f} (fused) {b:.7f} (nodes), {len(ga)} gradients")
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-4)
    assert len(ga) == len(gb) > 0
    for u, v in zip(ga, gb):
        assert float(np.abs(v).max()) > 0.0
        np.testing.assert_allclose(u, v, rtol=2e-4, atol=2e-4)


def _assert_grads(got: dict, gold: dict, prefix, what):
    names = [k for k in gold if k.startswith(prefix)]
    assert names and set(names) == set(got), (what, names, list(got))
    for n in names:
        ref = np.asarray(gold[n], dtype=np.float64)
        err, bar = float(np.abs(np.asarray(got[n], dtype=np.float64) - ref).max()), GRAD_BAR * float(np.abs(ref).max())
        print(f"  {what} {n}: max|d| {err:.3e}  bar {bar:.3e}")
        assert err <= bar, (what, n, err, bar)


@pytest.mark.parametrize("name", cs.TABLE)
def test_critic_steps_match_the_reference_fixture(name, monkeypatch):
    """Three IQL half-steps of the IDQL pipeline and three Diffusion-QL critic steps on the device against the real reference
    (tests/golden/critic_towers.npz): the losses and the parameter checksums after the third step at rtol = atol = 1e-4, the first step's
    gradients at 2e-4 x max |g_ref| per parameter -- every call with autograd served by the fused route."""
    from cleandiffuser_amd.engine.optim import FusedAdam
    seen = _spy_forward(monkeypatch)
    case, gold, U = cs.CASES[name], cs.golden(name), cs.utils_of("amd")
    monkeypatch.setenv("CDX_TOWER", "1")                      # (TwinQ / V take the fused route on request; their no-grad calls then too)
    got = cs.run_iql(U, case, DEV, adam=FusedAdam)
    assert [(q.n_towers, q.save) for q in seen] == [(2, False), (1, True), (1, False), (2, True)] * cs.STEPS, \
        "the fused route did not take the four critic calls of every half-step"
    del seen[:]
    monkeypatch.delenv("CDX_TOWER")
    got.update(cs.run_dql(U, case, DEV, adam=FusedAdam))
    assert [(q.n_towers, q.save) for q in seen] == [(2, True)] * cs.STEPS
    assert set(got) == set(gold)
    for k in ("iql/loss", "dql/loss", "iql/sums/Q", "iql/sums/V", "iql/sums/Q_targ", "dql/sums"):
        print(f"  {name} {k}: max|d| {float(np.abs(got[k] - gold[k]).max()):.3e}")
        np.testing.assert_allclose(got[k], gold[k], rtol=1e-4, atol=1e-4, err_msg=k)
    _assert_grads({k: v for k, v in got.items() if "/grad/" in k}, gold, ("iql/grad/", "dql/grad/"), name)


def _twinq_kernels(rows):
    """The device kernels of a steady-state ``TwinQ.both`` with its backward at the shipped sizes (obs 17, act 6, hidden 256)."""
    from torch.autograd import DeviceType
    from cleandiffuser_amd.utils import TwinQ, load_synth
    g = torch.Generator().manual_seed(2)
    m = load_synth(TwinQ(17, 6), 5).to(DEV)
    obs, act, target = (torch.randn(rows, n, generator=g).to(DEV) for n in (17, 6, 1))

    def step():
        m.zero_grad(set_to_none=True)
        q1, q2 = m.both(obs, act)
        ((q1 - target) ** 2 + (q2 - target) ** 2).mean().backward()
    for _ in range(2):
        step()
    prof, _ = profiled(step)
    return [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]


def test_the_launch_structure_of_a_twin_step(monkeypatch):
    """A steady-state ``TwinQ.both`` with its backward contains the forward kernel, the backward kernel, the batched weight-gradient
    kernel and the batched column sum exactly once each and none of the node route's kernels, the same number of device kernels at 16
    and at 64 rows, and fewer than half of what the node route (CDX_TOWER=0) launches."""
    counts = {}
    monkeypatch.setenv("CDX_TOWER", "1")
    for rows in (16, 64):
        kernels = _twinq_kernels(rows)
        print(f"rows = {rows}: {len(kernels)} device kernels on the fused route")
        for k in ("cdx_tower_fwd_kernel", "cdx_tower_bwd_kernel", "cdx_conv_wgrad_batch_kernel", "cdx_colsum_batch_kernel"):
            assert sum(k in n for n in kernels) == 1, (k, kernels)
        assert not any(k in n for n in kernels for k in ("cdx_gemm_kernel", "cdx_layernorm", "cdx_act_"))
        counts[rows] = len(kernels)
    assert counts[16] == counts[64], counts
    monkeypatch.setenv("CDX_TOWER", "0")
    nodes = _twinq_kernels(16)
    print(f"rows = 16: {len(nodes)} device kernels on the node route (CDX_TOWER=0), {counts[16]} on the fused route")
    assert not any("cdx_tower" in n for n in nodes)
    assert 2 * counts[16] < len(nodes), (counts, len(nodes))


def test_no_grad_evaluation_on_request(amd_lib, monkeypatch):
    """``CDX_TOWER=1``: a no-grad ``TwinQ`` / ``V`` / ``DQLCritic.q_min`` evaluation is the forward launch alone (nothing saved) and equals
    the default route (``heads.try_sequential``) at rtol = atol = 1e-4; above ``NOGRAD_MAX_ROWS`` the default route serves."""
    from cleandiffuser_amd.engine import tower
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V, load_synth
    seen = _spy_forward(monkeypatch)
    g = torch.Generator().manual_seed(4)
    obs, act = torch.randn(3, 11, 17, generator=g).to(DEV), torch.randn(3, 11, 6, generator=g).to(DEV)
    nets = [load_synth(TwinQ(17, 6, hidden_dim=64), 1), load_synth(V(17, hidden_dim=64), 2), load_synth(DQLCritic(17, 6, hidden_dim=64), 3)]
    calls = [lambda m: m(obs, act), lambda m: m(obs), lambda m: m.q_min(obs, act)]
    with torch.no_grad():
        want = [c(m.to(DEV).eval()) for c, m in zip(calls, nets)]
        assert not seen
        monkeypatch.setenv("CDX_TOWER", "1")
        got = [c(m) for c, m in zip(calls, nets)]
        assert [(q.n_towers, q.save, q.R) for q in seen] == [(2, False, 33), (1, False, 33), (2, False, 33)]
        for a, b in zip(got, want):
            assert a.shape == b.shape == (3, 11, 1)
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-4, atol=1e-4)
        monkeypatch.setattr(tower, "NOGRAD_MAX_ROWS", 32)
        calls[1](nets[1])
        assert len(seen) == 3
