"""GPU parity tests (run with ``pytest -m gpu`` on an MI355X).  Every call goes through the C ABI (libcdx.so):
``agent.sample`` on a ROCm device dispatches to ``cdx_unet2_run`` (whole loop, one launch) and
``backbone.forward`` to the same kernel in forward mode.  Bar: 1e-4 (fp32) against fixtures produced by the real
reference on CPU with identical injected noise (tests/golden/, oracle/gen_golden.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import cases
from conftest import golden_path
from gpu_profile import profiled as _profiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=1e-4, atol=1e-4)
CFG4_ELEMENTWISE_SHARE = 0.005    # (measured on MI355X, round 5: 3 of 5568 elements = 0.05 %)


def _extra(name):
    """Outputs of oracle/extra_cases.py scenario `name` built from THIS repo's classes on the device, and the committed
    fixture the real reference produced for the same scenario (tests/golden/extra_<name>.npz)."""
    from oracle import extra_cases
    return extra_cases.run(name, "amd", DEV), np.load(golden_path("extra_" + name))


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from cleandiffuser_amd.engine import runtime, runtime2
    runtime.load_library()          # hard failure if libcdx.so is missing -- never a silent eager fallback
    # the small-batch mode checks itself against the ordinary program on its first use per device (two launches instead of one):
    # get that over with before the tests that count launches
    name = "janner_cfg2_ddim"
    agent, _ = cases.build(cases.lib_namespace("amd"), name, device=DEV)
    inp = cases.make_inputs(name)
    agent.sample(torch.from_numpy(inp["prior"]).to(DEV), **cases.sample_kwargs(name, inp, device=DEV))
    torch.cuda.synchronize()
    # (a device on which it fails -- another partition mode -- runs everything on the ordinary program; the tests of the mode skip)
    # ... and the same for the full-batch grouped mode (k trajectories over the k workgroups of a group): first use at B = 256
    prior = torch.zeros(256, 32, 23, device=DEV)
    agent.sample(prior, n_samples=256, solver="ddim", sample_steps=2)
    torch.cuda.synchronize()
    # ... and for the two GUIDED modes (round 6): the small-batch one at B = 8, the grouped one at B = 200
    gagent, _ = cases.build(cases.lib_namespace("amd"), "janner_cfg2_guided_ddpm", device=DEV)
    for nb in (8, 200):
        gagent.sample(torch.zeros(nb, 32, 23, device=DEV), n_samples=nb, solver="ddpm", sample_steps=2, w_cg=0.1)
    torch.cuda.synchronize()


def _spy_launches(monkeypatch):
    """Counts launches of the program kernel (cdx_unet2_run via runtime2.launch): `n` and `v2` are the same number.  `repair`: the
    gated launches behind split / grouped launches (cdx.h: run_if) -- an empty grid unless a granule was lost -- counted apart."""
    from cleandiffuser_amd.engine import runtime2
    calls = {"n": 0, "v2": 0, "repair": 0}
    orig2 = runtime2.launch

    def wrapped2(*a, **k):
        if k.get("run_if") is not None:
            calls["repair"] += 1
            return orig2(*a, **k)
        calls["n"] += 1
        calls["v2"] += 1
        return orig2(*a, **k)
    monkeypatch.setattr(runtime2, "launch", wrapped2)
    return calls


def test_mfma_lane_maps_on_silicon():
    """The lane->element maps the kernels assume (guide section 3 + CK's 4x64 view of 4x4x1) hold on gfx950."""
    from cleandiffuser_amd.engine import runtime
    out = runtime.probe_mfma_layout(DEV).numpy()
    digits = 1 + 64 + 64 ** 2 + 64 ** 3
    for l in range(64):
        for r in range(4):
            i, j = 4 * (l >> 4) + r, l & 15
            assert out[0, l, r] == (i + 1) * digits, ("16x16x4 A/D map", l, r, out[0, l, r])
            assert out[1, l, r] == (j + 1) * digits, ("16x16x4 B/D map", l, r, out[1, l, r])
            blk, jj = l // 4, l % 4
            assert out[2, l, r] == 4 * blk + r + 1, ("4x4x1 A/D map", l, r, out[2, l, r])
            assert out[3, l, r] == 4 * blk + jj + 1, ("4x4x1 B/D map", l, r, out[3, l, r])


FWD_CASES = ["janner_cfg2_ddim", "janner_h4_ddpm", "janner_tiny_disc_ddim", "janner_tiny_cond_w1",
             "janner_tiny_cont_ddim", "janner_h64_single"]


@pytest.mark.parametrize("name", FWD_CASES)
def test_backbone_forward_matches_reference(name, amd_lib, monkeypatch):
    gold = np.load(golden_path(name))
    c = cases.CASES[name]
    agent, _ = cases.build(amd_lib, name, device=DEV)
    net = agent.model_ema["diffusion"]
    inp = cases.make_inputs(name)
    temp = c["sample"].get("temperature", 1.0)
    xt0 = inp["noise"][0] * np.float32(temp)
    if inp["fix_mask"] is not None:
        xt0 = xt0 * (1 - inp["fix_mask"][None]) + inp["prior"] * inp["fix_mask"][None]
    S = c["sample"]["sample_steps"]
    from cleandiffuser_amd.utils import SUPPORTED_SAMPLING_STEP_SCHEDULE as SS
    if c["solver"][0] == "DiscreteDiffusionSDE":
        sched = SS[c["sample"].get("sample_step_schedule", "uniform")](agent.diffusion_steps, S)
        t = torch.full((c["batch"],), int(sched[S]), dtype=torch.long, device=DEV)
    else:
        sched = SS[c["sample"].get("sample_step_schedule", "uniform_continuous")](agent.t_diffusion, S)
        t = torch.full((c["batch"],), float(sched[S]), dtype=torch.float32, device=DEV)
    cond = torch.from_numpy(inp["cond"]).to(DEV) if inp["cond"] is not None else None
    calls = _spy_launches(monkeypatch)
    with torch.no_grad():
        pred = net(torch.from_numpy(xt0.astype(np.float32)).to(DEV), t, cond)
    torch.cuda.synchronize()
    assert calls["n"] == 1, "forward must be served by exactly one fused launch"
    np.testing.assert_allclose(pred.cpu().numpy(), gold["pred0"], **TOL)


FUSED_CASES = [n for n, c in cases.CASES.items() if c["net"][0] in ("JannerUNet1d", "PearceMlp", "DQLMlp", "DVInvMlp", "ChiUNet1d", "SfBCUNet")
               and not c["sample"].get("w_cg")]
BIGBATCH_CASES = [n for n, c in cases.CASES.items() if c["net"][0] in cases.BIGBATCH_NETS]
TORCH_EXECUTOR_CASES = [n for n in cases.CASES if n not in FUSED_CASES and n not in BIGBATCH_CASES
                        and not cases.CASES[n]["sample"].get("w_cg")]


def _spy_bigbatch(monkeypatch):
    from cleandiffuser_amd.engine import bigbatch
    calls = []
    orig = bigbatch._run

    def wrapped(kind, *a, **k):
        calls.append((kind, k["chunk"], k["batch"]))
        return orig(kind, *a, **k)
    monkeypatch.setattr(bigbatch, "_run", wrapped)
    return calls


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("name", BIGBATCH_CASES)
def test_bigbatch_sample_matches_reference_fixture(name, chunk, amd_lib, monkeypatch):
    """DiT1d / IDQLMlp / NewIDQLMlp: the whole loop is ONE C call (cdx_dit1d_run / cdx_resmlp_run) that enqueues the
    GEMM / LayerNorm / attention / solver-step kernels; `chunk=2` forces several independent passes over the batch."""
    from cleandiffuser_amd.engine import bigbatch
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    calls = _spy_bigbatch(monkeypatch)
    kind = {"DiT1d": "dit", "ChiTransformer": "chitf"}.get(cases.CASES[name]["net"][0], "mlp")
    monkeypatch.setitem(bigbatch.CHUNK_OVERRIDE, kind, chunk)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == [kind], "exactly one native call for the whole loop"
    assert x.device.type == "cuda" and x.shape == gold["x_out"].shape
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


GUIDED_CASES = [n for n, c in cases.CASES.items() if c["sample"].get("w_cg")]


@pytest.mark.parametrize("name", ["janner_cfg2_guided_ddpm", "janner_h4_guided_eps", "janner_cfg2_diffuser_logp"])
def test_native_classifier_gradients_match_autograd(name, amd_lib, monkeypatch):
    """d logp / d x of HalfJannerUNet1d from the explicit forward+backward kernels vs torch.autograd on the same module."""
    from cleandiffuser_amd.engine import classifier_grad
    agent, _ = cases.build(amd_lib, name, device=DEV)
    c = cases.CASES[name]
    g = torch.Generator().manual_seed(11)
    b, H, D = 6, c["horizon"], c["net"][1]["in_dim"]
    x = torch.randn(b, H, D, generator=g).to(DEV)
    t = torch.randint(0, 20, (b,), generator=g).to(DEV)
    clf = agent.classifier
    logp_n, grad_n = clf.gradients(x.clone(), t, None)
    monkeypatch.setattr(classifier_grad, "ONE_CALL", False)                          # same schedule issued op by op from Python
    logp_p, grad_p = clf.gradients(x.clone(), t, None)
    np.testing.assert_allclose(logp_n.cpu().numpy(), logp_p.cpu().numpy(), rtol=1e-5, atol=1e-5)     # (C path may split K)
    np.testing.assert_allclose(grad_n.cpu().numpy(), grad_p.cpu().numpy(), rtol=1e-5, atol=1e-5 * max(float(grad_p.abs().max()), 1.0))
    monkeypatch.setattr(classifier_grad, "gradients", lambda *a, **k: None)          # force the autograd path
    logp_a, grad_a = clf.gradients(x.clone(), t, None)
    torch.cuda.synchronize()
    np.testing.assert_allclose(logp_n.cpu().numpy(), logp_a.cpu().numpy(), **TOL)
    scale = float(grad_a.abs().max())
    np.testing.assert_allclose(grad_n.cpu().numpy(), grad_a.cpu().numpy(), rtol=1e-4, atol=1e-4 * max(scale, 1.0))


def test_guided_program_gradient_matches_autograd(amd_lib):
    """The guided program's classifier part on the GPU (cdx_unet2_kernel<1, 8, true> in forward mode returns the gradient slot):
    d classifier(x, t).sum() / d x against torch.autograd on the same module, B = 70 (more workgroups than one XCD holds)."""
    from cleandiffuser_amd.engine import runtime2
    agent, _ = cases.build(amd_lib, "janner_cfg2_guided_ddpm", device=DEV)
    net, clf = agent.model_ema["diffusion"], agent.classifier.model_ema
    assert runtime2.guided_supported(net, clf, 32) is None
    g = torch.Generator().manual_seed(11)
    x = torch.randn(70, 32, 23, generator=g).to(DEV)
    t = torch.full((70,), 7, dtype=torch.long, device=DEV)
    grad = runtime2.classifier_gradient2(net, clf, x, t)
    xr = x.clone().requires_grad_()
    clf._forward_torch(xr, t, None).sum().backward()
    torch.cuda.synchronize()
    scale = float(xr.grad.abs().max())
    np.testing.assert_allclose(grad.cpu().numpy(), xr.grad.cpu().numpy(), rtol=1e-4, atol=1e-4 * max(scale, 1.0))


def test_guided_two_trajectories_per_workgroup(amd_lib, monkeypatch):
    """Guided program variant for two trajectories per workgroup (saved x_hat tensors in the launch's global workspace, capped staging
    area; taken above B = 256): B = 37 (half-empty last workgroup -> spare workspace block) forced through it must agree with the
    one-trajectory, all-in-LDS program to summation-order noise (the staging cap changes some K splits), and reproduce itself."""
    name = "janner_cfg2_guided_ddpm"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    g = torch.Generator().manual_seed(13)
    B = 37
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(6)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=5, temperature=0.5, w_cg=0.3)
    outs = {}
    for t in ("1", "2", "2", "3", "3"):
        monkeypatch.setenv("CDX_UNET2_T", t)
        calls = _spy_launches(monkeypatch)
        x, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        torch.cuda.synchronize()
        assert calls["v2"] == 1
        outs.setdefault(t, []).append(x)
    assert torch.equal(outs["2"][0], outs["2"][1])
    np.testing.assert_allclose(outs["2"][0].cpu().numpy(), outs["1"][0].cpu().numpy(), rtol=2e-4, atol=2e-4)
    # three per workgroup: the compact variant on top (state / multistep memory in global memory, the classifier's copy of x_t
    # re-read through a load op, in-place residual outputs): 49.6 KB of LDS per trajectory; 37 = 12 full workgroups + one with a
    # single real trajectory
    assert torch.equal(outs["3"][0], outs["3"][1])
    np.testing.assert_allclose(outs["3"][0].cpu().numpy(), outs["1"][0].cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_guided_batch_is_cut_into_rounds_of_three_per_workgroup(amd_lib, monkeypatch):
    """Above two rounds of workgroups a guided batch is cut like an unguided one (runtime2.plan_parts): rounds of 256 x 3 trajectories
    on the compact guided program plus the remaining rounds at two per workgroup on the same program; the result agrees with the
    one-trajectory program on the same draws."""
    from cleandiffuser_amd.engine import runtime2
    name = "janner_cfg2_guided_ddpm"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    g = torch.Generator().manual_seed(14)
    B = 1536 + 40
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(4)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=3, temperature=0.5, w_cg=0.3)
    assert runtime2.plan_parts(B, 3, runtime2.GUIDED_ROUND_COST) == [(0, 768, 3), (768, 808, 2)]
    calls = _spy_launches(monkeypatch)
    x3, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    assert calls["v2"] == 1, calls
    monkeypatch.setenv("CDX_UNET2_T", "1")
    x1, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    np.testing.assert_allclose(x3.cpu().numpy(), x1.cpu().numpy(), rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("one_call", ["v2", True, False])
@pytest.mark.parametrize("name", GUIDED_CASES)
def test_guided_sampling_matches_reference_fixture(name, one_call, amd_lib, monkeypatch):
    """w_cg > 0.  "v2": the whole guided loop is ONE cdx_unet2_run launch (denoiser forward, classifier forward + backward and the
    shifted solver step on LDS-resident state) whenever the guided program exists.  True: cdx_guided_run (fused backbone forward +
    native classifier forward/backward + solver step per record, ~105 launches per step from one C call).  False: the host steps
    the loop and every step's gradient still comes from the native kernels."""
    from cleandiffuser_amd.engine import classifier_grad, guided, runtime2
    gold = np.load(golden_path(name))
    if one_call != "v2":
        monkeypatch.setenv("CDX_UNET2_GUIDED", "0")
    launches = _spy_launches(monkeypatch)
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    used = {"grad": 0, "loop": 0}
    orig_g, orig_l = classifier_grad.gradients, guided.guided_sample

    def counted(*a, **k):
        out = orig_g(*a, **k)
        used["grad"] += out is not None
        return out

    def loop(*a, **k):
        out = orig_l(*a, **k) if one_call else None
        used["loop"] += out is not None
        return out
    monkeypatch.setattr(classifier_grad, "gradients", counted)
    monkeypatch.setattr(guided, "guided_sample", loop)
    x, _ = agent.sample(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    if one_call == "v2":
        assert used == {"grad": 0, "loop": 1}
        c = cases.CASES[name]
        if runtime2.guided_supported(agent.model_ema["diffusion"], agent.classifier.model_ema, c["horizon"]) is None:
            assert launches["v2"] == 1, "guided loop with a guided program must be one cdx_unet2_run launch"
    elif one_call:
        # (the only v2 launch left is the classifier's own program scoring the final trajectories: the log_p pass)
        assert used == {"grad": 0, "loop": 1} and launches["v2"] <= 1
    else:
        assert used["grad"] == kw["sample_steps"], "every step's classifier gradient must come from the native kernels"
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


CHIUNET_CASES = [n for n, c in cases.CASES.items() if c["net"][0] == "ChiUNet1d"]


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("name", CHIUNET_CASES)
def test_chiunet_gemm_executor_matches_reference_fixture(name, chunk, amd_lib, monkeypatch):
    """ChiUNet1d's second native executor (implicit-GEMM convolutions, cdx_chiunet_run) -- normally chosen for batch >= 96 --
    forced on for the small fixtures: same reference samples, one native call."""
    from cleandiffuser_amd.engine import bigbatch
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    monkeypatch.setattr(bigbatch, "UNET_GEMM_MIN_BATCH", 1)
    monkeypatch.setitem(bigbatch.CHUNK_OVERRIDE, "chiunet", chunk)
    calls = _spy_bigbatch(monkeypatch)
    fused = _spy_launches(monkeypatch)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["chiunet"] and fused["n"] == 0
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("name", ["janner_cfg2_ddim", "janner_h4_ddpm", "janner_cfg2_ddpm_clip", "janner_h64_single",
                                  "janner_legacy_dpm_sdepp2", "janner_rflow_discrete", "janner_legacy_edm_euler",
                                  "janner_legacy_edm_heun", "janner_legacy_edm_x", "janner_cm"])
def test_janner_gemm_executor_matches_reference_fixture(name, amd_lib, monkeypatch):
    """Unconditional JannerUNet1d through the implicit-GEMM U-Net executor (meant for batches in the thousands; forced here)."""
    from cleandiffuser_amd.engine import bigbatch
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    monkeypatch.setattr(bigbatch, "JANNER_GEMM_MIN_BATCH", 1)
    monkeypatch.setenv("CDX_UNET2", "0")              # (the program kernel would otherwise keep every batch size it supports)
    calls = _spy_bigbatch(monkeypatch)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["chiunet"]       # EDM / consistency records included (c_in-scaled input copy)
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


def test_chiunet_gemm_forward_matches_program_kernel(amd_lib, monkeypatch):
    """backbone.forward with per-sample timesteps: the two native ChiUNet1d executors agree (and the program kernel is pinned to
    the reference by the fixtures above)."""
    from cleandiffuser_amd.engine import bigbatch
    name = "chiunet_cfg3_legacy_ddpm"
    agent, net = cases.build(amd_lib, name, device=DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 16, 2, generator=g).to(DEV)
    t = torch.randint(0, 10, (37,), generator=g).to(DEV)
    cond = torch.randn(37, 2, 20, generator=g).to(DEV)
    with torch.no_grad():
        a = net(x, t, cond)
        monkeypatch.setattr(bigbatch, "UNET_GEMM_MIN_BATCH", 1)
        calls = _spy_bigbatch(monkeypatch)
        b = net(x, t, cond)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["chiunet"]
    np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), **TOL)


@pytest.mark.parametrize("name", BIGBATCH_CASES)
def test_bigbatch_forward_matches_reference_fixture(name, amd_lib, monkeypatch):
    """`backbone.forward` with a different timestep per sample (what training-time evaluation and custom loops call)."""
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    x, t, cond = cases.forward_probe(name, agent, inp, device=DEV)
    calls = _spy_bigbatch(monkeypatch)
    with torch.no_grad():
        pred = agent.model_ema["diffusion"](x, t, cond)
    torch.cuda.synchronize()
    assert len(calls) == 1
    np.testing.assert_allclose(pred.cpu().numpy(), gold["fwd_pred"], **TOL)


@pytest.mark.parametrize("name", TORCH_EXECUTOR_CASES)
def test_unfused_backbones_match_reference_on_device(name, amd_lib, monkeypatch):
    """Backbones/solvers that have no fused program yet (configs 1, 3, 4, 5 at fixture size) run the PyTorch executor
    on the ROCm device: API-complete and reference-exact, but NOT native code -- listed in DESIGN.md section 7."""
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    calls = _spy_launches(monkeypatch)
    x, log = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert calls["n"] == 0
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_sample_matches_reference_fixture(name, amd_lib, monkeypatch):
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    n_draws = int(gold["n_draws"])
    calls = _spy_launches(monkeypatch)
    x, log = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:n_draws]), **kw)
    torch.cuda.synchronize()
    has_clf = "log_p" in gold.files
    assert calls["n"] == (2 if has_clf else 1), "one launch for the whole loop (+ one for the classifier score)"
    assert x.device.type == "cuda" and x.shape == gold["x_out"].shape
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)
    if has_clf:
        np.testing.assert_allclose(log["log_p"].cpu().numpy(), gold["log_p"], **TOL)
        assert int(log["log_p"].argmax()) == int(gold["log_p"].argmax()), "candidate arg-max must be bit-exact"


V2_CASES = [n for n in FUSED_CASES if cases.CASES[n]["net"][0] == "JannerUNet1d" and not cases.CASES[n].get("cond")
            and not cases.CASES[n]["sample"].get("w_cfg")]


@pytest.mark.parametrize("n_waves", ["4", "8"])
@pytest.mark.parametrize("t_per_wg", ["1", "2"])
@pytest.mark.parametrize("name", V2_CASES)
def test_unet2_kernel_matches_reference_fixture(name, t_per_wg, n_waves, amd_lib, monkeypatch):
    """The second-generation kernel (cdx_unet2_run) in its four workgroup shapes -- 4 or 8 waves, one or two trajectories per
    workgroup (the fixtures' odd batch sizes exercise the half-empty last workgroup): every unconditional JannerUNet1d fixture
    whose plan has no EDM step kinds must be served by it -- one launch -- and reproduce the reference."""
    from cleandiffuser_amd.engine import runtime, runtime2
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    monkeypatch.setenv("CDX_UNET2_T", t_per_wg)
    monkeypatch.setenv("CDX_UNET2_NW", n_waves)
    calls = _spy_launches(monkeypatch)
    seen, orig = [], runtime2.fused_sample2

    def spy(solver, net, plan, *a, **k):
        seen.append(plan)
        return orig(solver, net, plan, *a, **k)
    monkeypatch.setattr(runtime2, "fused_sample2", spy)
    x, log = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    net = agent.model_ema["diffusion"]
    assert len(seen) == 1, "unconditional JannerUNet1d requests are offered to the v2 kernel first"
    if runtime2.supported(net, x.shape[1]) is None and not runtime.plan_is_edm(seen[0]):
        # (+ 1: a fixture with a classifier scores the final trajectories with the classifier's own v2 program)
        assert calls["v2"] == 1 + ("log_p" in gold.files), "supported unconditional U-Net loop must run on cdx_unet2_run"
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


def test_program_kernel_is_batch_invariant_across_workgroup_shapes(amd_lib, monkeypatch):
    """Same request through cdx_unet2_run with T = 1 and T = 2 in both wave shapes: T does not change a single bit (trajectories in a
    workgroup never interact); the 4- and 8-wave programs agree to fp32 summation-order noise."""
    name = "janner_cfg2_ddpm_clip"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    g = torch.Generator().manual_seed(7)
    B = 37
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g) for _ in range(11)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=10)
    outs = {}
    for tag, env in (("t1", {"CDX_UNET2_T": "1", "CDX_UNET2_NW": "4"}), ("t2", {"CDX_UNET2_T": "2"}),
                     ("t1w8", {"CDX_UNET2_T": "1", "CDX_UNET2_NW": "8"}), ("t2w8", {"CDX_UNET2_T": "2"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        calls = _spy_launches(monkeypatch)
        outs[tag], _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        torch.cuda.synchronize()
        assert calls["n"] == 1
    assert torch.equal(outs["t1"], outs["t2"]), "trajectories per workgroup must not change results"
    assert torch.equal(outs["t1w8"], outs["t2w8"]), "trajectories per workgroup must not change results (8-wave shape)"
    # (the 8-wave program cuts K into more slices: same math, another summation order; a 10-step clipped DDPM amplifies that noise
    #  near the clip boundary -- both shapes are pinned to the reference at 1e-4 by the fixtures)
    np.testing.assert_allclose(outs["t1w8"].cpu().numpy(), outs["t1"].cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_three_trajectories_per_workgroup(amd_lib, monkeypatch):
    """The compact program (state and multistep memory in global memory, in-place residual outputs) with 1, 2 and 3 trajectories per
    workgroup: bit-identical results (B = 40: a half-empty last workgroup in every shape; DPM-Solver++ 2M exercises the multistep
    memory in the workspace), and within summation-order noise of the standard program."""
    name = "janner_cfg2_ddim"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    g = torch.Generator().manual_seed(21)
    B = 40
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    z0 = torch.randn(B, 32, 23, generator=g).to(DEV)
    kw = dict(solver="ode_dpmsolver++_2M", n_samples=B, sample_steps=6, temperature=0.5)
    outs = {}
    for tag, env in (("std", {"CDX_UNET2_T": "1", "CDX_UNET2_COMPACT": "0"}), ("c1", {"CDX_UNET2_T": "1", "CDX_UNET2_COMPACT": "1"}),
                     ("c2", {"CDX_UNET2_T": "2", "CDX_UNET2_COMPACT": "1"}), ("c3", {"CDX_UNET2_T": "3", "CDX_UNET2_COMPACT": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        calls = _spy_launches(monkeypatch)
        outs[tag], _ = agent.sample(prior.to(DEV), noise=[z0], **kw)
        torch.cuda.synchronize()
        assert calls["v2"] == 1
    assert torch.equal(outs["c1"], outs["c2"]) and torch.equal(outs["c1"], outs["c3"])
    np.testing.assert_allclose(outs["c3"].cpu().numpy(), outs["std"].cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_split_tail_launch_does_not_change_results(amd_lib, monkeypatch):
    """B = 640: the bulk (512) runs two trajectories per workgroup, the remainder (128) one per workgroup through a second
    cdx_unet2_run over the trajectory range [512, 640) -- bit-identical to the single two-per-workgroup launch (DDPM: per-step noise
    is indexed with the full-batch stride in both)."""
    name = "janner_cfg2_ddpm_clip"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    g = torch.Generator().manual_seed(9)
    B = 640
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(4)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=3)
    outs = {}
    monkeypatch.setenv("CDX_UNET2_T3", "0")              # (with the compact program B = 640 would be one launch of three per workgroup)
    for split in ("1", "0"):
        monkeypatch.setenv("CDX_UNET2_SPLIT_TAIL", split)
        outs[split], _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    assert torch.equal(outs["1"], outs["0"])
    assert torch.isfinite(outs["1"]).all()


def test_steady_state_sample_call_is_one_kernel_launch(amd_lib, monkeypatch):
    """a steady-state sample() call of the north-star config dispatches no ATen compute -- the schedule grid
    (a CPU linspace) and the output allocation are all the host does besides the one cdx_unet2_run launch: x_T = z * temperature
    blended with the prior is formed inside the kernel, step table / FiLM table / dense masks come from the per-plan caches."""
    from torch.utils._python_dispatch import TorchDispatchMode
    name = "janner_cfg2_ddim"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    B, H, D = 64, 32, 23
    g = torch.Generator().manual_seed(5)
    prior = torch.zeros(B, H, D)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    z0 = torch.randn(B, H, D, generator=g).to(DEV)
    prior = prior.to(DEV)
    kw = dict(solver="ddim", n_samples=B, sample_steps=20, temperature=0.5)
    ref, _ = agent.sample(prior, noise=[z0], **kw)

    class Log(TorchDispatchMode):
        ops = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Log.ops.append(str(func))
            return func(*args, **(kwargs or {}))
    calls = _spy_launches(monkeypatch)
    with Log():
        x, _ = agent.sample(prior, noise=[z0], **kw)
    torch.cuda.synchronize()
    assert calls["v2"] == 1 and calls["n"] == 1
    assert set(Log.ops) <= {"aten.linspace.default", "aten.empty_like.default"}, Log.ops
    assert torch.equal(x, ref)
    # the in-kernel x_T is the ATen one bit for bit: same request with x_T formed on the host (conditioning kwargs absent, history on
    # would change the executor, so go through the internal entry the raw start falls back to)
    from cleandiffuser_amd.engine import dispatch
    monkeypatch.setattr(dispatch, "try_fused_raw", lambda *a, **k: None)
    x_host, _ = agent.sample(prior, noise=[z0], **kw)
    assert torch.equal(x_host, x), "x_T formed by the kernel must equal the ATen mul/blend sequence exactly"


def test_full_size_properties(amd_lib):
    """BASELINE config 2 at B=256: size-independent properties -- determinism, batch independence (a trajectory's
    result does not depend on its neighbours or its block index), fix-mask exactness, agreement with the CPU
    executor on a slice."""
    name = "janner_cfg2_ddim"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    cpu_agent, _ = cases.build(amd_lib, name, device="cpu")
    B, H, D = 256, 32, 23
    g = torch.Generator().manual_seed(3)
    prior = torch.zeros(B, H, D)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    z0 = torch.randn(B, H, D, generator=g)
    kw = dict(solver="ddim", n_samples=B, sample_steps=20, temperature=0.5)
    x1, _ = agent.sample(prior.to(DEV), noise=[z0], **kw)
    x2, _ = agent.sample(prior.to(DEV), noise=[z0], **kw)
    assert torch.equal(x1, x2), "not deterministic"
    assert torch.equal(x1[:, 0, :17].cpu(), prior[:, 0, :17]), "fix-mask must re-impose the prior exactly"
    sl = slice(100, 108)
    kw8 = dict(kw, n_samples=8)
    x_sub, _ = agent.sample(prior[sl].to(DEV), noise=[z0[sl]], **kw8)
    # (256 trajectories take the grouped program, 8 the small-batch mode -- other K orders in the layers they cut: equal to fp32 noise;
    #  on the SAME program a trajectory's bits depend on nothing but the trajectory: a slice of 8 through the grouped program -- other
    #  groups, other member indices -- and through the ordinary program against the full batch on each)
    np.testing.assert_allclose(x_sub.cpu().numpy(), x1[sl].cpu().numpy(), rtol=5e-5, atol=5e-5)
    from cleandiffuser_amd.engine import runtime2
    os.environ["CDX_UNET2_SPLIT"] = "0"
    try:
        os.environ["CDX_UNET2_GROUP"] = "0"
        x_same, _ = agent.sample(prior[sl].to(DEV), noise=[z0[sl]], **kw8)
        x1p, _ = agent.sample(prior.to(DEV), noise=[z0], **kw)
        assert torch.equal(x_same, x1p[sl]), "a trajectory must not depend on its batch neighbours"
        np.testing.assert_allclose(x1p.cpu().numpy(), x1.cpu().numpy(), rtol=5e-5, atol=5e-5)
        if runtime2._group_ok.get(torch.device(DEV)) is True:
            os.environ["CDX_UNET2_GROUP"] = "4"
            x_grp, _ = agent.sample(prior[sl.start + 1:sl.stop].to(DEV), noise=[z0[sl.start + 1:sl.stop]], **dict(kw, n_samples=7))
            runtime2.check_split_errors()
            assert torch.equal(x_grp, x1[sl.start + 1:sl.stop]), "grouped program: a trajectory must not depend on its group or member index"
    finally:
        del os.environ["CDX_UNET2_SPLIT"]
        os.environ.pop("CDX_UNET2_GROUP", None)
    x_cpu, _ = cpu_agent.sample(prior[sl], noise=[z0[sl]], **kw8)
    np.testing.assert_allclose(x_sub.cpu().numpy(), x_cpu.numpy(), **TOL)
    assert torch.isfinite(x1).all()


def test_rng_path_runs_on_device(amd_lib):
    """Without ``noise=`` the draws come from the device generator: shape/finite/mask checks only."""
    agent, _ = cases.build(amd_lib, "janner_cfg2_ddpm_clip", device=DEV)
    prior = torch.zeros(16, 32, 23, device=DEV)
    x, _ = agent.sample(prior, solver="ddpm", n_samples=16, sample_steps=10)
    assert x.shape == (16, 32, 23) and torch.isfinite(x).all() and x.abs().max() <= 2.0 + 1e-6


def test_weight_update_invalidates_program_cache(amd_lib):
    agent, _ = cases.build(amd_lib, "janner_tiny_disc_ddim", device=DEV)
    net = agent.model_ema["diffusion"]
    x = torch.randn(4, 8, 6, device=DEV)
    t = torch.full((4,), 7, dtype=torch.long, device=DEV)
    with torch.no_grad():
        y0 = net(x, t)
        net.final_conv[3].bias.add_(1.0)
        y1 = net(x, t)
    np.testing.assert_allclose((y1 - y0).cpu().numpy(), 1.0, rtol=0, atol=1e-5)


@pytest.mark.parametrize("name", ["janner_tiny_disc_ddim", "janner_tiny_cond_w2", "janner_cfg2_guided_ddpm"])
def test_ema_update_reaches_the_native_executors(name, amd_lib):
    """``sample(use_ema=True)`` between training steps (DQL target actions, periodic evaluation, consistency distillation,
    classifier guidance): after ``ema_update()`` the packed-weight caches of the native executors (v2 / v1 program, classifier
    gradient) must be rebuilt -- the round-1 caches keyed on ``Tensor._version`` alone, which writes through ``p.data`` do not
    bump.  Device result == CPU executor of an identically updated agent, and != the pre-update result."""
    agent, _ = cases.build(amd_lib, name, device=DEV)
    cpu_agent, _ = cases.build(amd_lib, name, device="cpu")
    inp = cases.make_inputs(name)
    kw, kw_cpu = cases.sample_kwargs(name, inp, device=DEV), cases.sample_kwargs(name, inp)
    prior = torch.from_numpy(inp["prior"])
    x0, _ = agent.sample(prior.to(DEV), noise=list(inp["noise"]), **kw)                  # fills every cache with the old weights
    for a in (agent, cpu_agent):
        gen = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for p in a.model.parameters():
                p.add_(0.05 * torch.randn(p.shape, generator=gen).to(p.device))
        a.ema_rate = 0.5
        a.ema_update()
        if a.classifier is not None:
            with torch.no_grad():
                for p in a.classifier.model.parameters():
                    p.add_(0.05 * torch.randn(p.shape, generator=gen).to(p.device))
            a.classifier.ema_rate = 0.5
            a.classifier.ema_update()
    x1, _ = agent.sample(prior.to(DEV), noise=list(inp["noise"]), **kw)
    want, _ = cpu_agent.sample(prior, noise=list(inp["noise"]), **kw_cpu)
    assert float((x1 - x0).abs().max()) > 1e-3, "EMA step must change the samples"
    np.testing.assert_allclose(x1.cpu().numpy(), want.numpy(), rtol=2e-4, atol=2e-4)
    # a caller that still writes through .data has to say so
    from cleandiffuser_amd.utils import invalidate_weights
    for a in (agent, cpu_agent):
        for p in a.model_ema.parameters():
            p.data.mul_(1.01)
        invalidate_weights(a.model_ema)
    x2, _ = agent.sample(prior.to(DEV), noise=list(inp["noise"]), **kw)
    want2, _ = cpu_agent.sample(prior, noise=list(inp["noise"]), **kw_cpu)
    np.testing.assert_allclose(x2.cpu().numpy(), want2.numpy(), rtol=2e-4, atol=2e-4)


def test_candidate_argmax_matches_cpu_at_diffuser_batch(amd_lib):
    """Diffuser's candidate selection (reference pipelines/diffuser_d4rl_mujoco.py:144-147): 64 candidates x 4 envs,
    arg-max of the classifier score per env must pick the same candidate as the CPU executor (index-exact)."""
    name = "janner_cfg2_diffuser_logp"
    agent, _ = cases.build(amd_lib, name, device=DEV)
    cpu_agent, _ = cases.build(amd_lib, name, device="cpu")
    n_cand, n_env, H, D = 64, 4, 32, 23
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(n_env, 17, generator=g)
    prior = torch.zeros(n_cand * n_env, H, D)
    prior[:, 0, :17] = obs.repeat(n_cand, 1)
    zs = [torch.randn(n_cand * n_env, H, D, generator=g) for _ in range(20)]
    kw = dict(solver="ddpm", n_samples=n_cand * n_env, sample_steps=20, temperature=0.5)
    x_g, log_g = agent.sample(prior.to(DEV), noise=zs, **kw)
    x_c, log_c = cpu_agent.sample(prior, noise=zs, **kw)
    lp_g = log_g["log_p"].cpu().view(n_cand, n_env)
    lp_c = log_c["log_p"].view(n_cand, n_env)
    np.testing.assert_allclose(lp_g.numpy(), lp_c.numpy(), **TOL)
    assert torch.equal(lp_g.argmax(0), lp_c.argmax(0))
    top2 = lp_c.topk(2, dim=0).values
    assert float((top2[0] - top2[1]).min()) > 1e-4, "test inputs must not contain near-ties"


def test_chiunet_forward_one_launch(amd_lib, monkeypatch):
    """ChiUNet1d.forward (FiLM blocks, global condition) served by the program kernel with per-sample timesteps."""
    agent, _ = cases.build(amd_lib, "chiunet_cfg3_legacy_ddpm", device=DEV)
    cpu_agent, _ = cases.build(amd_lib, "chiunet_cfg3_legacy_ddpm", device="cpu")
    g = torch.Generator().manual_seed(2)
    x, c = torch.randn(5, 16, 2, generator=g), torch.randn(5, 2, 20, generator=g)
    t = torch.tensor([0, 3, 9, 5, 1])
    calls = _spy_launches(monkeypatch)
    with torch.no_grad():
        y = agent.model_ema["diffusion"](x.to(DEV), t.to(DEV), c.to(DEV))
        y_ref = cpu_agent.model_ema["diffusion"](x, t, c)
    assert (calls["n"], calls["v2"]) == (1, 1)
    np.testing.assert_allclose(y.cpu().numpy(), y_ref.numpy(), **TOL)


def test_empty_and_ragged_batches(amd_lib, monkeypatch):
    """Edge cases of the boundary: an empty request returns an empty tensor without launching; batch sizes that do
    not fill the last wave of workgroups / the last MLP tile (1, 257, 17) give the same rows as a larger batch."""
    monkeypatch.setenv("CDX_UNET2_SPLIT", "0")           # (bit-equality between batch sizes holds on ONE program, not across the small-batch mode)
    agent, _ = cases.build(amd_lib, "janner_tiny_disc_ddim", device=DEV)
    kw = dict(solver="ddim", sample_steps=5, temperature=0.8)
    x, _ = agent.sample(torch.zeros(0, 8, 6, device=DEV), n_samples=0, **kw)
    assert x.shape == (0, 8, 6)
    g = torch.Generator().manual_seed(9)
    z = torch.randn(257, 8, 6, generator=g)
    prior = torch.zeros(257, 8, 6)
    prior[:, 0, :4] = torch.randn(257, 4, generator=g)
    big, _ = agent.sample(prior.to(DEV), n_samples=257, noise=[z], **kw)
    one, _ = agent.sample(prior[256:].to(DEV), n_samples=1, noise=[z[256:]], **kw)
    assert torch.equal(big[256:], one)
    magent, _ = cases.build(amd_lib, "dqlmlp_ddpm", device=DEV)
    obs = torch.randn(17, 17, generator=g)
    zs = [torch.randn(17, 6, generator=g) for _ in range(5)]
    mk = dict(solver="ddpm", sample_steps=5, w_cfg=1.0)
    m17, _ = magent.sample(torch.zeros(17, 6, device=DEV), n_samples=17, condition_cfg=obs.to(DEV), noise=zs, **mk)
    m3, _ = magent.sample(torch.zeros(3, 6, device=DEV), n_samples=3, condition_cfg=obs[14:].to(DEV),
                          noise=[q[14:] for q in zs], **mk)
    assert torch.equal(m17[14:], m3)


@pytest.mark.parametrize("name", ["janner_tiny_disc_ddpm", "chiunet_cfg3_legacy_ddpm", "dit_ddim_cfg", "idql_obs_ddim_cfg",
                                  "chitransformer_ddim", "pearce_cfg1_ddpm", "janner_cm", "janner_rflow_cont_cfg"])
def test_training_step_on_device_keeps_autograd(name, amd_lib, monkeypatch):
    """loss()/update() on the ROCm device must stay on PyTorch autograd: the native executors only serve
    gradient-free calls, so one optimiser step must change the weights and produce a finite loss."""
    from cleandiffuser_amd.engine import bigbatch, runtime, runtime2
    agent, net = cases.build(amd_lib, name, device=DEV)
    agent.train()
    native = {"n": 0}
    for mod, fn in ((runtime2, "launch"), (bigbatch, "_run")):
        orig = getattr(mod, fn)
        monkeypatch.setattr(mod, fn, lambda *a, _o=orig, **k: (native.__setitem__("n", native["n"] + 1), _o(*a, **k))[1])
    c = cases.CASES[name]
    inp = cases.make_inputs(name)
    x0 = torch.from_numpy(inp["noise"][0]).to(DEV)
    cond = torch.from_numpy(inp["cond"]).to(DEV) if inp["cond"] is not None else None
    before = [p.detach().clone() for p in net.parameters()]
    log = agent.update(x0, cond)
    torch.cuda.synchronize()
    assert np.isfinite(log["loss"])
    # the consistency loss evaluates its target under torch.no_grad(): that forward may (and does) take the native kernel
    assert native["n"] == (1 if c["solver"][0] == "ContinuousConsistencyModel" else 0)
    changed = sum(float((p.detach() - b).abs().sum()) for p, b in zip(net.parameters(), before))
    assert changed > 0.0


def _full_size(which, B):
    """The BASELINE config-3/4/5 solvers at their real network sizes (synthetic weights), with explicit inputs."""
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from cleandiffuser_amd import diffusion as DF, nn_condition as NC, nn_diffusion as ND
    from cleandiffuser_amd.diffusion.ddpm import DDPM
    from cleandiffuser_amd.utils import load_synth
    g = torch.Generator().manual_seed(17)

    def make(dev):
        if which == "cfg3":
            net = load_synth(ND.ChiUNet1d(2, 20, 2, model_dim=256, emb_dim=256, dim_mult=[1, 2, 2], obs_as_global_cond=True))
            one = torch.ones(1, 16, 2, device=dev)
            return DDPM(net, NC.IdentityCondition(dropout=0.0), diffusion_steps=50, x_max=one, x_min=-one, device=dev)
        if which == "cfg4":
            net = load_synth(ND.DiT1d(29, emb_dim=128, d_model=320, n_heads=10, depth=2, timestep_emb_type="fourier"))
            cond = load_synth(NC.MLPCondition(1, 128, [128], torch.nn.SiLU(), dropout=0.25), 2)
            fix = torch.zeros(64, 29)
            fix[0] = 1.0
            return DF.ContinuousDiffusionSDE(net, cond, fix_mask=fix, predict_noise=True, noise_schedule="linear",
                                             x_max=3 * torch.ones(1, 64, 29), x_min=-3 * torch.ones(1, 64, 29), device=dev)
        net = load_synth(ND.IDQLMlp(0, 15, emb_dim=128, hidden_dim=1024, n_blocks=6))
        return DF.ContinuousEDM(net, None, device=dev)

    def make_eval(dev):
        a = make(dev)
        a.eval()
        return a

    if which == "cfg3":
        prior, cond = torch.zeros(B, 16, 2), torch.randn(B, 2, 20, generator=g)
        zs = [torch.randn(B, 16, 2, generator=g) for _ in range(50)]
        kw = dict(sample_steps=50, w_cfg=1.0)
    elif which == "cfg4":
        prior, cond = torch.zeros(B, 64, 29), torch.rand(B, 1, generator=g)
        prior[:, 0] = torch.randn(B, 29, generator=g)
        zs = [torch.randn(B, 64, 29, generator=g)]
        kw = dict(solver="ode_dpmsolver++_2M", sample_steps=10, w_cfg=2.0, temperature=0.5)
    else:
        prior, cond = torch.zeros(B, 15), None
        zs = [torch.randn(B, 15, generator=g)]
        kw = dict(solver="euler", sample_steps=16)
    return make_eval, prior, cond, zs, kw


@pytest.mark.parametrize("which,B", [("cfg3", 1024), ("cfg4", 512), ("cfg5", 4096)])
def test_bigbatch_full_size_properties(which, B, amd_lib):
    """BASELINE configs 3, 4, 5 at their real network and batch sizes: determinism (split-K included), exact fix-mask, a
    sample's result independent of its batch neighbours / of the executor that serves a small batch (1e-4), and agreement with
    the CPU executor on two samples."""
    make, prior, cond, zs, kw = _full_size(which, B)
    agent = make(DEV)

    def run(a, sl, dev):
        p = prior[sl].to(dev)
        c = None if cond is None else cond[sl].to(dev)
        x, _ = a.sample(p, n_samples=p.shape[0], condition_cfg=c, noise=[z[sl] for z in zs], **kw)
        return x
    full = slice(0, B)
    x1, x2 = run(agent, full, DEV), run(agent, full, DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(x1).all() and torch.equal(x1, x2), "not deterministic"
    if which == "cfg4":
        assert torch.equal(x1[:, 0].cpu(), prior[:, 0].clip(-3, 3)), "fix-mask must re-impose the prior exactly (then the final clip)"
    sl = slice(B // 2 + 3, B // 2 + 11)
    scale = max(float(x1.abs().max()), 1.0)
    np.testing.assert_allclose(run(agent, sl, DEV).cpu().numpy(), x1[sl].cpu().numpy(), rtol=1e-4, atol=1e-4 * scale)
    two = slice(B // 2 + 3, B // 2 + 5)
    x_cpu = run(make("cpu"), two, "cpu")
    np.testing.assert_allclose(x1[two].cpu().numpy(), x_cpu.numpy(), rtol=1e-4, atol=1e-4 * scale)


@pytest.mark.gpu
def test_post_sampling_heads_run_native_and_match_reference(amd_lib, monkeypatch):
    """Critics / inverse-dynamics heads on the device: every Sequential goes through engine/heads.py (counted),
    results equal the reference's CPU outputs; tanh / LayerNorm-as-GroupNorm(L=1,G=1) paths included."""
    from cleandiffuser_amd.engine import heads
    from oracle import gen_module_golden as G
    calls = {"n": 0, "eager": 0}
    real = heads.try_sequential

    def counted(seq, x):
        y = real(seq, x)
        calls["n" if y is not None else "eager"] += 1
        return y
    monkeypatch.setattr(heads, "try_sequential", counted)
    gold = np.load(golden_path("modules"))
    out = G.head_outputs("cleandiffuser_amd", device="cuda")
    for k, v in out.items():
        np.testing.assert_allclose(v, gold[f"head/{k}"], rtol=1e-4, atol=2e-5, err_msg=k)
    assert calls["eager"] == 0 and calls["n"] >= 25, calls


@pytest.mark.gpu
def test_heads_at_candidate_batch(amd_lib):
    """IDQL-style re-weighting at pipeline scale: 256 states x 64 candidates through TwinQ/V and the inverse-dynamics head,
    against the same modules run by PyTorch on the device (fp32, 1e-4)."""
    from cleandiffuser_amd.invdynamic import MlpInvDynamic
    from cleandiffuser_amd.utils import DQLCritic, TwinQ, V, load_synth
    torch.manual_seed(0)
    n, o, a = 256 * 64, 17, 6
    obs, act, nxt = torch.randn(n, o, device="cuda"), torch.randn(n, a, device="cuda"), torch.randn(n, o, device="cuda")
    q, v, c = load_synth(TwinQ(o, a)).cuda().eval(), load_synth(V(o)).cuda().eval(), load_synth(DQLCritic(o, a)).cuda().eval()
    inv = MlpInvDynamic(o, a, device="cuda")
    inv.eval()
    with torch.no_grad():
        got = [q(obs, act), v(obs), c.q_min(obs, act), inv(obs, nxt)]
        x = torch.cat([obs, act], -1)
        want = [torch.min(q.Q1(x), q.Q2(x)), v.V(obs), torch.min(c.q1_model(x), c.q2_model(x)), inv.mlp.mlp(torch.cat([obs, nxt], -1))]
    for g, w in zip(got, want):
        assert g.shape == w.shape
        np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), rtol=1e-4, atol=1e-4)
    adv = got[0] - got[1]
    idx = torch.multinomial(torch.softmax(adv.view(256, 64) * 3.0, -1), 1)         # selection stays on the device
    assert idx.shape == (256, 1) and idx.is_cuda


@pytest.mark.gpu
def test_condition_encoders_run_native(amd_lib, monkeypatch):
    """The built-in low-dim condition encoders go through engine/heads.py while sampling (eval, no grad) -- including
    the K = 1 first layer of Decision Diffuser's return encoder -- and equal the same modules on CPU."""
    from cleandiffuser_amd import nn_condition as NC
    from cleandiffuser_amd.engine import heads
    from cleandiffuser_amd.utils import load_synth
    calls = {"n": 0, "eager": 0}
    real = heads.try_sequential

    def counted(seq, x):
        y = real(seq, x)
        if x.is_cuda:
            calls["n" if y is not None else "eager"] += 1
        return y
    monkeypatch.setattr(heads, "try_sequential", counted)
    torch.manual_seed(0)
    cases = [(NC.MLPCondition(1, 128, [128], torch.nn.SiLU(), 0.25), torch.rand(37, 1)),
             (NC.MLPCondition(11, 64, [96, 48]), torch.randn(300, 11)),
             (NC.LinearCondition(9, 32), torch.randn(5, 9)),
             (NC.MLPSieveObsCondition(7, emb_dim=16, hidden_dim=64), torch.randn(6, 3, 7)),
             (NC.PearceObsCondition(17, 64, flatten=True, dropout=0.0), torch.randn(256, 1, 17)),
             (NC.PearceObsCondition(5, 32, flatten=False), torch.randn(4, 2, 5)),
             (NC.FourierCondition(32, 64), torch.rand(8, 1)),
             (NC.PositionalCondition(32, 32), torch.rand(8))]
    for enc, c in cases:
        enc = load_synth(enc).eval()
        with torch.no_grad():
            want = enc(c)
            got = enc.cuda()(c.cuda())
        assert got.shape == want.shape
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=2e-5, err_msg=type(enc).__name__)
    assert calls == {"n": len(cases), "eager": 0}, calls
    enc = cases[0][0].train()                                  # training: label-dropout mask + autograd -> stock modules
    out = enc(cases[0][1].cuda())
    assert out.requires_grad and calls["eager"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [64, 192, 512])
def test_pearce_mlp_widths_match_reference_fixture(hidden, amd_lib, monkeypatch):
    """Batch-tiled MLP program at other widths than the config-1 fixture (group sizes 8 / 24 / 64 in the segmented GroupNorm
    epilogue, ragged last tile): one fused launch, reference fixture at the 1e-4 bar.  hidden_dim 192 has GroupNorm groups of 24
    channels -- not the 2^k float4 lanes per position the epilogue partitions: its hidden slots are laid out 8 x 32 with zero pad
    channels that stay out of the variance."""
    launches = _spy_launches(monkeypatch)
    out, gold = _extra(f"pearce_h{hidden}")
    torch.cuda.synchronize()
    assert launches["n"] == 1, "whole loop in one fused launch"
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("name,horizon,compact_t1", [("janner_h128", 128, True), ("janner_h128", 128, False), ("janner_h64_w48", 64, False)])
def test_janner_beyond_one_workgroup_takes_gemm_executor(name, horizon, compact_t1, amd_lib, monkeypatch):
    """Long-horizon / wide JannerUNet1d (maze2d-style plans) whose default LDS plan does not fit: H = 128 still fits as a compact
    one-trajectory program (144 KB: one fused launch); without that variant (CDX_UNET2_COMPACT_T1=0), and for the 48-channel net
    whose GroupNorm groups do not match the epilogue partition, small batches go to the implicit-GEMM U-Net executor instead of
    failing or dropping to eager.  Reference fixture, 1e-4."""
    from cleandiffuser_amd.engine import runtime, runtime2
    if not compact_t1:
        monkeypatch.setenv("CDX_UNET2_COMPACT_T1", "0")
    calls = _spy_bigbatch(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    net = out["_agent"].model_ema["diffusion"]
    if compact_t1:
        assert runtime2.supported(net, horizon) is None and runtime2.compiled2(net, horizon, 8).prog.compact and calls == []
    else:
        assert runtime2.supported(net, horizon) is not None
        assert [c[0] for c in calls] == ["chiunet"]
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["program", "executor"])
@pytest.mark.parametrize("size", ["kitchen", "antmaze"])
def test_shipped_large_diffuser_configs_stay_native(size, path, amd_lib, monkeypatch):
    """The two shipped Diffuser / AdaptDiffuser configurations with model_dim 64, against fixtures of the real reference
    (stand-alone forward, unguided loop, guided loop, classifier log_p) at 1e-4.
    path "program" (the default): every call is ONE program-kernel launch.  kitchen (H = 32, D = 69): 141 KB of LDS, the guided
    program keeps its saved tensors in the global workspace.  antmaze (H = 64, D = 37) fits only as a COMPACT program (state and
    multistep memory in global memory, in-place residual outputs; guided: the classifier re-reads x_t from global memory): 158 KB.
    path "executor" (CDX_UNET2_GUIDED=0, CDX_UNET2_COMPACT_T1=0 -- the round-1 route, kept for nets that fit no program): kitchen's
    guided loop is one cdx_guided_run call around the fused denoiser; antmaze's unguided sampling is one implicit-GEMM executor
    call and its guided loop one cdx_guided_run call that runs the same executor for its per-step denoiser forward."""
    from cleandiffuser_amd.engine import classifier_grad, guided, runtime, runtime2
    H = 32 if size == "kitchen" else 64
    steps, fits = 3, size == "kitchen"
    if path == "executor":
        monkeypatch.setenv("CDX_UNET2_GUIDED", "0")
        monkeypatch.setenv("CDX_UNET2_COMPACT_T1", "0")
    calls, fused = _spy_bigbatch(monkeypatch), _spy_launches(monkeypatch)
    grads, one_call = {"n": 0}, {"n": 0}
    real_grad, real_guided = classifier_grad.gradients, guided.guided_sample

    def counted(*a, **k):
        out = real_grad(*a, **k)
        grads["n"] += out is not None
        return out

    def counted_guided(*a, **k):
        out = real_guided(*a, **k)
        one_call["n"] += out is not None
        return out
    monkeypatch.setattr(classifier_grad, "gradients", counted)
    monkeypatch.setattr(guided, "guided_sample", counted_guided)
    out, gold = _extra("diffuser_" + size)
    torch.cuda.synchronize()
    net = out["_agent"].model_ema["diffusion"]
    if path == "program":
        assert runtime2.guided_supported(net, out["_agent"].classifier.model_ema, H) is None
        # sampling loops: no executor call at all; antmaze's stand-alone forward (per-sample timesteps) is one GEMM-executor call
        assert one_call["n"] == 1 and grads["n"] == 0 and [c[0] for c in calls] == ([] if fits else ["chiunet"]), calls
        assert (runtime2.compiled2(net, H, 8).prog.compact) == (not fits) and runtime2.compact_only(net, H) == (not fits)
    elif fits:
        assert one_call["n"] == 1 and calls == []                                    # cdx_guided_run: the whole guided loop
    else:
        # GEMM executor: the stand-alone forward and the unguided loop; the guided loop is ONE cdx_guided_run call whose per-step
        # denoiser forward is the same executor (cdx_guided_launch.denoiser_gemm) -- no per-step host round trips
        assert one_call["n"] == 1 and grads["n"] == 0 and len(calls) == 2, (calls, grads)
    for k in ("fwd", "x", "x_guided", "log_p"):
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=k, **TOL)
    assert int(out["log_p"].argmax()) == int(gold["log_p"].argmax())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["chitf_ta10", "chitf_enc2", "dit_h10_d384", "dit_h96", "dit_h40_depth8"])
def test_shipped_transformer_shapes_match_reference_fixture(which, amd_lib, monkeypatch):
    """Token counts / widths of the shipped dp_* and veteran configs that the small fixtures do not cover (Ta = 10, 10 and 40
    tokens, head_dim 64, depth 8; ChiTransformer with a transformer condition encoder, n_cond_layers = 2; DiT1d over 96 tokens --
    the streamed-key attention kernel, no shipped config is that long): whole loop native,
    reference fixture at 1e-4 (depth 8 included)."""
    calls = _spy_bigbatch(monkeypatch)
    out, gold = _extra(which)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["chitf" if which.startswith("chitf") else "dit"]
    got = out["x"].cpu().numpy()
    if which in ("chitf_ta10", "dit_h96"):
        # Round 5 FINDING (profiles/r05_dit_error_budget.txt): these two clipped, saturating scenarios sit AT the resolving power of an
        # fp32 fixture -- the reference's own fp32 result is 1.5e-4 / 1.7e-4 away from the same reference in float64
        # (extra_<name>_fp64.npz, oracle/gen_golden_extra.py:fp64_yardstick).  Rounds 1-4 passed them at 1e-4 because the GEMM kernel
        # summed K in ONE sequential fma chain, exactly as the MKL build that made the fixture does -- the same rounding errors, not
        # smaller ones.  The K-blocked accumulation (every GEMM now at or below ATen's error against float64) leaves 1-2 of 210 / 2016
        # elements 1.4-1.9e-4 from the fp32 fixture.  Asserted: no element further from the float64 truth than 1.25x the fp32 CPU path's
        # own worst error, the mean error within 1.25x of it, and at most 0.5 % of the elements beyond 1e-4 of the fp32 fixture.
        # (yardsticks computed on THIS box by the package's PyTorch executor, pinned to the reference's by tests/test_extra_fixtures.py:
        #  results at this level move with the host's exp / log rounding -- see test_config4_with_resolving_power...)
        from oracle import extra_cases
        x64 = extra_cases.run(which, "amd", "cpu", fp64=True)["x"].double().numpy()
        c32 = extra_cases.run(which, "amd", "cpu")["x"].double().numpy()
        ref_err, own_err = np.abs(c32 - x64), np.abs(got - x64)
        bad = np.abs(got - gold["x"]) > 1e-4 + 1e-4 * np.abs(gold["x"])
        print(f"{which}: native vs fp64 max {own_err.max():.3e} mean {own_err.mean():.3e}; CPU fp32 (this box) vs fp64 max {ref_err.max():.3e} "
              f"mean {ref_err.mean():.3e}; beyond 1e-4 of the Xeon fp32 fixture: {int(bad.sum())} of {bad.size}; float64 here vs the Xeon's "
              f"{np.abs(x64 - np.load(golden_path(f'extra_{which}_fp64'))['x']).max():.3e}")
        # the yardstick's link to the REFERENCE, checked on the box that uses it: the float64 run of this package here
        # equals the float64 run of the imported reference in the build container (committed, stored rounded to fp32) -- these two
        # clipped loops do not amplify the hosts' transcendental differences (measured 6e-8 in round 5)
        fix64 = np.load(golden_path(f"extra_{which}_fp64"))["x"].astype(np.float64)
        assert np.abs(x64 - fix64).max() <= 2e-6 * max(1.0, np.abs(fix64).max()), np.abs(x64 - fix64).max()
        assert bad.mean() <= 0.005, f"{int(bad.sum())} of {bad.size} elements beyond 1e-4 of the fp32 reference"
        assert own_err.max() <= 1.25 * ref_err.max(), (own_err.max(), ref_err.max())
        assert own_err.mean() <= 1.25 * ref_err.mean() + 1e-7, (own_err.mean(), ref_err.mean())
        return
    if which != "dit_h40_depth8":
        np.testing.assert_allclose(got, gold["x"], **TOL)
        return
    # FINDING: this one scenario cannot be held to 1e-4 against the fp32 reference, because the reference cannot
    # hold it against itself -- depth 8 on synthetic, saturating weights amplifies fp32 rounding ~300x and the reference's fp32
    # result is 1.7e-4 (7 of 3480 elements > 1e-4) away from the SAME reference evaluated in float64 (extra_dit_h40_depth8_fp64.npz,
    # oracle/gen_golden_extra.py).  Measured on MI355X: 4 of 3480 elements beyond 1e-4 of the fp32 fixture, worst 3.5e-4.
    # What is asserted: >= 99.5 % of the elements inside the 1e-4 bar, and no element further from the float64 truth than 3x the
    # fp32 reference's own worst error.
    x64 = np.load(golden_path("extra_dit_h40_depth8_fp64"))["x"]
    ref_err = np.abs(gold["x"] - x64).max()
    bad = np.abs(got - gold["x"]) > 1e-4 + 1e-4 * np.abs(gold["x"])
    assert bad.mean() <= 0.005, f"{int(bad.sum())} of {bad.size} elements beyond 1e-4 of the fp32 reference"
    assert np.abs(got - x64).max() <= 3.0 * ref_err, (np.abs(got - x64).max(), ref_err)


@pytest.mark.gpu
@pytest.mark.parametrize("executor", ["program", "gemm"])
def test_chiunet_config3_width_matches_reference_fixture(executor, amd_lib, monkeypatch):
    """ChiUNet1d at the BASELINE config-3 width (model_dim 256, 68.9 M parameters; split-K over 6 slices and K up to 10 240 only
    exist at this width) through both native executors, against a fixture of the real reference."""
    from cleandiffuser_amd.engine import bigbatch
    if executor == "gemm":
        monkeypatch.setattr(bigbatch, "UNET_GEMM_MIN_BATCH", 1)
    else:                                   # (a net of this size takes the GEMM executor at every batch by default)
        monkeypatch.setattr(bigbatch, "UNET_GEMM_MIN_PARAMS", 10 ** 12)
    calls, fused = _spy_bigbatch(monkeypatch), _spy_launches(monkeypatch)
    out, gold = _extra("chiunet_cfg3_width")
    torch.cuda.synchronize()
    assert ([c[0] for c in calls], fused["n"]) == ((["chiunet"], 0) if executor == "gemm" else ([], 1))
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)


def test_chiunet_local_conditioning_runs_on_the_gemm_executor(amd_lib, monkeypatch):
    """ChiUNet1d(obs_as_global_cond=False) -- one observation row per action position, local_cond_encoder's two blocks
    joining the first down level and the last up level (reference chiunet.py:78-82, 153-185) -- used to take the PyTorch modules;
    now the stand-alone forward and the whole legacy-DDPM loop are one cdx_chiunet_run call each.  Reference fixture, 1e-4."""
    calls = _spy_bigbatch(monkeypatch)
    out, gold = _extra("chiunet_local_cond")
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["chiunet", "chiunet"], calls
    for k in ("fwd", "x"):
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=k, **TOL)


@pytest.mark.parametrize("name", ["pearce_cfg_pair", "dql_cfg_pair", "mlpnn_cfg_pair"])
def test_tile_mlp_cfg_pair_is_fused(name, amd_lib, monkeypatch):
    """w_cfg not in {0, 1} on the batch-tiled MLP programs (PearceMlp, DQLMlp) used to fall back to the PyTorch
    executor; now the conditional / zero-condition pair of every step runs inside the one cdx_unet2_run launch (the context slot's
    condition channels are rewritten per branch).  Reference fixture, 1e-4."""
    calls = _spy_launches(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    assert calls["n"] == 1, "CFG pair on a tile-MLP denoiser must be one fused launch"
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)


def test_wide_idqlmlp_runs_on_the_resmlp_executor(amd_lib, monkeypatch):
    """IDQLMlp with hidden_dim 2048 (> 1024) -- cdx_layernorm_f32 now keeps rows of up to 4096 channels in registers, so
    cdx_resmlp_run takes the net instead of the PyTorch executor.  Reference fixture (EDM Euler), 1e-4."""
    calls = _spy_bigbatch(monkeypatch)
    out, gold = _extra("idql_h2048")
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["mlp"], calls                   # one cdx_resmlp_run call
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)


# ---- BASELINE.json's configurations at their exact (size x solver x steps x guidance) combination (VERDICT r2 "Next" #1) ----
@pytest.mark.parametrize("name", ["baseline_cfg1", "baseline_cfg2_b256", "baseline_cfg2_guided", "baseline_cfg3", "baseline_cfg4",
                                  "baseline_cfg5"])
def test_exact_baseline_configuration_matches_reference_fixture(name, amd_lib, monkeypatch):
    """PearceMlp 256 x 100-step DDPM; JannerUNet1d config 2 at B = 256 (the headline launch itself, straight against the reference)
    and its classifier-guided 20-step DDPM variant with log_p; ChiUNet1d model_dim 256 x 50-step legacy DDPM; DiT1d d 320 / 10 heads
    / 64 tokens x CFG 2.0 x 10-step DPM-Solver++ 2M; IDQLMlp 1024 x 6 x 128-step EDM Euler.  Fixtures: the real reference on the
    same weights and draws (oracle/extra_cases.py:baseline_config).  Bar 1e-4, relative to the fixture's largest magnitude where the
    un-clipped config 4 on synthetic weights leaves the unit range (|x| up to 589)."""
    fused, big = _spy_launches(monkeypatch), _spy_bigbatch(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    assert fused["n"] + len(big) >= 1, "the loop must run natively"
    for k in gold.files:
        got = out[k].cpu().numpy()
        if name == "baseline_cfg4":
            # un-clipped config 4 on plain synthetic weights (|x| up to 589): ELEMENTWISE |d| <= 1e-4 + 1e-4 |x| (round 5; rounds 3-4
            # divided both sides by 589 first, i.e. allowed 0.059 everywhere).  The sampler amplifies fp32 rounding so much here that
            # the reference's own fp32 run violates the elementwise bar against float64 on a share of the elements (the first step
            # divides by alpha(1) = 0.0066) -- test_config4_with_resolving_power... is the test with teeth; this one reports the
            # violating share and bounds it, and bounds the worst element relative to the tensor's scale.
            bad = np.abs(got - gold[k]) > 1e-4 + 1e-4 * np.abs(gold[k])
            print(f"baseline_cfg4/{k}: {int(bad.sum())} of {bad.size} elements beyond the elementwise 1e-4 bar, max |d| = "
                  f"{np.abs(got - gold[k]).max():.3e} at |x| max {np.abs(gold[k]).max():.1f}")
            # ... next to what the reference's own fp32 arithmetic does on THIS host (the package's PyTorch executor on the CPU, pinned to
            # the reference at 2e-6 by the CPU suite) against the same Xeon-made fixture: the allowance is visibly the reference's own
            from oracle import extra_cases
            c32 = extra_cases.run(name, "amd", "cpu")[k].cpu().numpy()
            bad_cpu = np.abs(c32 - gold[k]) > 1e-4 + 1e-4 * np.abs(gold[k])
            print(f"baseline_cfg4/{k}: CPU fp32 on this box vs the same fixture: {int(bad_cpu.sum())} of {bad_cpu.size} beyond the bar, max |d| = "
                  f"{np.abs(c32 - gold[k]).max():.3e}")
            assert bad.mean() <= bad_cpu.mean() + CFG4_ELEMENTWISE_SHARE, (bad.mean(), bad_cpu.mean())
            assert bad.mean() <= CFG4_ELEMENTWISE_SHARE, f"{name}/{k}: {bad.mean():.4f} of the elements beyond rtol = atol = 1e-4"
            assert np.abs(got - gold[k]).max() <= 1e-4 * max(1.0, float(np.abs(gold[k]).max()))
            continue
        np.testing.assert_allclose(got, gold[k], err_msg=f"{name}/{k}", **TOL)
    if name == "baseline_cfg2_guided":                               # candidate selection is index-exact
        assert int(out["log_p"].argmax()) == int(gold["log_p"].argmax())
        # ... and the classifier's final log_p forward ran INSIDE the guided launch (round 3): one kernel launch for the whole call
        assert (fused["n"], fused["v2"]) == (1, 1), fused


@pytest.mark.parametrize("name", ["baseline_cfg5_d27", "baseline_cfg3_b130", "baseline_cfg5_b300", "baseline_cfg5_d27_b300"])
def test_baseline_configurations_beyond_one_tile_match_reference_fixture(name, amd_lib, monkeypatch):
    """VERDICT r3 'weak' #3 / 'missing' #6: configs 3 and 5 at batches that cross the GEMM executors' tile and chunk boundaries (130 /
    300), against the REAL reference instead of this repo's CPU executor, and config 5 at the real hopper transition width D = 27.
    Fixtures: the imported reference on the same weights and draws (oracle/extra_cases.py:GPU_ONLY).  ABSOLUTE 1e-4."""
    big = _spy_bigbatch(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    assert len(big) >= 1, "the loop must run on the native executors"
    for k in gold.files:
        d = np.abs(out[k].cpu().numpy() - gold[k])
        assert float(d.max()) <= 1e-4, f"{name}/{k}: max |d| = {d.max():.3e} at |x| = {np.abs(gold[k]).max():.2f} (absolute bar 1e-4)"


def test_config5_across_the_executors_chunk_boundary_matches_reference_fixture(amd_lib, monkeypatch):
    """VERDICT r5 'weak' #1: config 5 in ONE sample() call of 16 384 + 300 rows -- cdx_resmlp_run cuts the call into 16 384-row chunks
    itself, the cut a rank of the 8-GPU run crosses seven times per call (`config5_shard125000` in bench.py) -- against what the REAL
    reference produced for the rows either side of the cut (samples are independent, reference newedm.py:286-438: the fixture generator
    sampled only those rows from the same draws; oracle/extra_cases.py:ROW_SUBSET).  ABSOLUTE 1e-4."""
    big = _spy_bigbatch(monkeypatch)
    out, gold = _extra("baseline_cfg5_b16684")
    torch.cuda.synchronize()
    assert len(big) >= 1, "the loop must run on the native executor"
    rows = gold["rows"].astype(np.int64)
    x = out["x"].cpu().numpy()
    assert x.shape == (16384 + 300, 15) and np.isfinite(x).all()
    d = np.abs(x[rows] - gold["x"])
    assert float(d.max()) <= 1e-4, f"max |d| = {d.max():.3e} at rows {rows[np.argwhere(d > 1e-4)[:, 0]]} (absolute bar 1e-4)"


@pytest.mark.parametrize("name", ["baseline_cfg4_tied", "baseline_cfg4_tied_b96", "baseline_cfg4_tied_b512"])
def test_config4_with_resolving_power_against_the_float64_yardstick(name, amd_lib, monkeypatch):
    """VERDICT r3 'weak' #1 / r4 'next' #1: config 4 with a DiT1d that behaves like a trained noise predictor (output layer tied to the
    input projection, oracle/extra_cases.py:baseline_config): same network size, solver, steps and guidance, but the un-clipped result
    stays |x| <= 7.7 instead of 589, so errors are visible in absolute terms -- at B = 3, at B = 96 (6144 token rows: several GEMM
    tiles) and at B = 512, the exact per-GPU shard of BASELINE config 4 (65 536 token rows with the CFG pair).

    What this configuration can be held to (tools/dit_error_budget.py, profiles/r04_ / r05_dit_error_budget.txt, r05_host_transcendentals.txt):
    eps-prediction without clipping divides by alpha(1) = 0.0066 in the first step and CFG w = 2 triples the network's contribution --
    whatever rounding enters is amplified ~1000x.  (i) An fp32 run of the reference is 1.8e-4 (B = 3) / 9.5e-4 (B = 96) away from the
    same reference in float64, so the yardstick is float64, not an fp32 fixture.  (ii) The reference's fp32 result is HOST-dependent at
    the same level: ATen's vectorised exp / log / tanh return different last bits on the Xeon of the build container and on the EPYC
    of the GPU box (same image, same draws -- tools/randn_host_check.py), the fp32 noise schedule the solver computes from them moves
    by an ulp, and the result by 3e-4.  A fixture made elsewhere therefore cannot resolve 1e-4 here either: the yardsticks are computed
    ON THIS BOX by this package's PyTorch executor -- pinned to the imported reference at 2e-6 in fp32 and 3e-7 in float64 by the CPU
    suite (tests/test_extra_fixtures.py) -- in float64 (the truth) and in fp32 (what the reference computes on this host).
    Asserted (round 5: the GEMMs sum K in blocks of 16, every one of them at or below ATen's error; rounds 3-4 allowed 3x): the native
    result is no further from the float64 truth than 1.25x the fp32 CPU path -- worst element and mean --, its share of elements
    beyond 1e-4 of the truth at most the CPU path's + 0.5 points.  The committed Xeon fixtures are reported next to it and bounded by
    the triangle inequality with the host term.  B = 512: the yardsticks cover every 16th trajectory of the batch the device sampled."""
    from oracle import extra_cases
    big = _spy_bigbatch(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    assert [c[0] for c in big] == ["dit"], big
    stride = int(gold["stride"][0]) if "stride" in gold.files else 1
    native = out["x"].cpu().numpy().astype(np.float64)
    rows = slice(0, None, 16) if native.shape[0] > 128 else None
    got = native[rows] if rows is not None else native
    x64 = extra_cases.run(name, "amd", "cpu", fp64=True, rows=rows)["x"].double().numpy()
    c32 = extra_cases.run(name, "amd", "cpu", rows=rows)["x"].double().numpy()
    ref_err, own_err = np.abs(c32 - x64), np.abs(got - x64)
    fix32 = gold["x"].astype(np.float64)
    fix64 = np.load(golden_path(f"extra_{name}_fp64"))["x"].astype(np.float64)
    host = np.abs(x64 - (fix64[::16 // stride] if rows is not None else fix64)).max()      # float64 here vs float64 in the build container
    print(f"{name}: native vs fp64 max {own_err.max():.3e} mean {own_err.mean():.3e} beyond 1e-4: {(own_err > 1e-4).mean():.4f}; "
          f"CPU fp32 (this box) vs fp64 max {ref_err.max():.3e} mean {ref_err.mean():.3e} beyond 1e-4: {(ref_err > 1e-4).mean():.4f}; "
          f"native vs the Xeon fp32 fixture max {np.abs(native[::stride] - fix32).max():.3e}; float64 on this box vs the Xeon's {host:.3e}")
    assert own_err.max() <= max(1e-4, 1.25 * ref_err.max()), (own_err.max(), ref_err.max())
    assert own_err.mean() <= max(2e-6, 1.25 * ref_err.mean()), (own_err.mean(), ref_err.mean())
    assert (own_err > 1e-4).mean() <= (ref_err > 1e-4).mean() + 0.005, ((own_err > 1e-4).mean(), (ref_err > 1e-4).mean())
    # the committed fixtures (build container): native is within (own error + the fixture's own error + what the host moves)
    assert np.abs(native[::stride] - fix32).max() <= own_err.max() + np.abs(fix32 - fix64).max() + host + 1e-6


@pytest.mark.parametrize("name", ["discrete_eps", "discrete_x0", "continuous_eps", "edm_conditional_nodrop", "legacy_ddpm",
                                  "weighted_regression", "chiunet_ddpm", "chiunet_cfg3", "dit_small", "dit_cfg4", "chitf_small", "chitf_pusht", "sfbc_continuous",
                                  "classifier_cumrew", "classifier_cfg2"])      # ("edm_conditional": nn.Dropout draws inside ATen, CPU-only)
def test_loss_and_update_match_reference_fixture(name):
    """loss() / update() on the ROCm device against what the REAL reference computed on CPU from the same seeded
    timestep / noise / label-dropout draws (oracle/train_cases.py; the CPU generator's draws are replayed on the device): loss value,
    three AdamW + EMA updates, clipped-gradient norms, parameter / EMA checksums.  Reference diffusionsde.py:94-141, newedm.py:152-190,
    ddpm.py:80-112, basic.py:66,83-86."""
    from oracle import train_cases
    gold = np.load(golden_path("train_" + name))
    out = train_cases.run(name, "amd", DEV)
    assert set(gold.files) == set(out)
    for k in gold.files:
        np.testing.assert_allclose(out[k], gold[k], err_msg=f"{name}/{k}", **TOL)


# ---- row f4, first slice: the optimiser side of update() on the library (csrc/cdx_optim.hip, engine/optim.py) ----
def test_fused_adamw_matches_torch_adamw_over_ten_steps():
    """FusedAdamW.step (one multi-tensor launch: clip -> decoupled decay -> moments -> bias-corrected step -> EMA -> zeroed gradients)
    against torch.optim.AdamW + clip_grad_norm_ + the reference's EMA loop (diffusion/basic.py:66,83-86) fed the SAME gradients for 10
    steps: parameters, both moments, EMA copies and the reported norms agree to 1e-6 (relative to the tensor's scale)."""
    from copy import deepcopy
    from cleandiffuser_amd.engine.optim import FusedAdamW
    from cleandiffuser_amd.nn_diffusion import JannerUNet1d
    from cleandiffuser_amd.utils import load_synth
    torch.manual_seed(0)
    net_a = load_synth(JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=5), 3).to(DEV)
    net_b, ema_a = deepcopy(net_a), deepcopy(net_a).requires_grad_(False)
    ema_b = deepcopy(ema_a)
    kw = dict(lr=3e-3, weight_decay=1e-2, betas=(0.9, 0.99))
    opt_a, opt_b = FusedAdamW(net_a.parameters(), **kw), torch.optim.AdamW(net_b.parameters(), **kw)
    assert opt_a.native()
    rate, max_norm = 0.9, 0.7
    for step in range(10):
        grads = [torch.randn_like(p) * (0.02 if step % 3 else 2.0) for p in net_a.parameters()]      # clipped on some steps only
        for p, q, g in zip(net_a.parameters(), net_b.parameters(), grads):
            if p.grad is None:
                p.grad = g.clone()
            else:
                assert float(p.grad.abs().max()) == 0.0, "step(zero_grad=True) must leave zeroed gradients in place"
                p.grad.add_(g)
            q.grad = g.clone()
        opt_a.step(max_norm=max_norm, ema=(net_a, ema_a, rate), zero_grad=True)
        norm_b = torch.nn.utils.clip_grad_norm_(net_b.parameters(), max_norm)
        opt_b.step()
        with torch.no_grad():
            for q, e in zip(net_b.parameters(), ema_b.parameters()):
                e.mul_(rate).add_(q.detach(), alpha=1 - rate)
        torch.testing.assert_close(opt_a.last_grad_norm, norm_b, rtol=2e-6, atol=0)
    sd_a = opt_a.state_dict()                       # (refreshes the per-parameter `step` tensors from the python-side counters)
    for (n, p), q, ea, eb in zip(net_a.named_parameters(), net_b.parameters(), ema_a.parameters(), ema_b.parameters()):
        scale = float(q.detach().abs().max()) + 1e-12
        assert float((p.detach() - q.detach()).abs().max()) <= 1e-6 * max(scale, 1.0), n
        assert float((ea - eb).abs().max()) <= 1e-6 * max(scale, 1.0), n
        sa, sb = opt_a.state[p], opt_b.state[q]
        assert float(sa["step"]) == float(sb["step"]) == 10.0
        torch.testing.assert_close(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-9)
        torch.testing.assert_close(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-12)
    # state_dict round trip through the stock optimiser class (pipelines checkpoint agent.optimizer)
    opt_c = torch.optim.AdamW(net_b.parameters(), **kw)
    opt_c.load_state_dict(sd_a)


def test_fused_adamw_skips_parameters_without_a_gradient_like_torch():
    """after step(zero_grad=True) / zero_grad() the gradients stay allocated (zeroed in place).  A parameter whose
    gradient nobody writes in a later iteration (update() without a condition: the condition encoder; an unused branch) must be
    treated as torch treats ``grad is None``: no weight decay, no momentum step, no step count -- while the EMA still covers EVERY
    parameter (reference basic.py:83-86).  Six steps against torch.optim.AdamW + the reference's EMA loop, with half of the
    parameters receiving gradients only on even steps."""
    from copy import deepcopy
    from cleandiffuser_amd.engine.optim import FusedAdamW
    torch.manual_seed(1)
    net_a = torch.nn.Sequential(torch.nn.Linear(12, 40), torch.nn.Mish(), torch.nn.Linear(40, 40), torch.nn.Mish(), torch.nn.Linear(40, 5)).to(DEV)
    net_b, ema_a = deepcopy(net_a), deepcopy(net_a).requires_grad_(False)
    ema_b = deepcopy(ema_a)
    kw = dict(lr=3e-3, weight_decay=5e-2, betas=(0.9, 0.99))
    opt_a, opt_b = FusedAdamW(net_a.parameters(), **kw), torch.optim.AdamW(net_b.parameters(), **kw)
    assert opt_a.native()
    rate = 0.8
    late = {id(p) for p in list(net_a.parameters())[2:4]}                      # the middle Linear: gradients on even steps only
    for step in range(6):
        for p, q in zip(net_a.parameters(), net_b.parameters()):
            if id(p) in late and step % 2:
                continue                                                     # (a: zeroed tensor left by the last step; b: None)
            g = torch.randn_like(p)
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.add_(g)                                               # what autograd's AccumulateGrad does
            q.grad = g.clone()
        if step == 3:
            opt_a.zero_grad()                                                # the explicit call must keep the same contract ...
            opt_b.zero_grad()
            for p, q in zip(net_a.parameters(), net_b.parameters()):         # ... and a backward pass after it counts again
                if id(p) not in late:
                    g = torch.randn_like(p)
                    p.grad.add_(g)
                    q.grad = g.clone()
        opt_a.step(ema=(net_a, ema_a, rate), zero_grad=True)
        opt_b.step()
        opt_b.zero_grad()
        with torch.no_grad():
            for q, e in zip(net_b.parameters(), ema_b.parameters()):
                e.mul_(rate).add_(q.detach(), alpha=1 - rate)
    opt_a.state_dict()
    for (n, p), q, ea, eb in zip(net_a.named_parameters(), net_b.parameters(), ema_a.parameters(), ema_b.parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=2e-6, atol=2e-7, msg=n)
        torch.testing.assert_close(ea, eb, rtol=2e-6, atol=2e-7, msg=n + " (ema)")
        assert float(opt_a.state[p]["step"]) == float(opt_b.state[q]["step"]) == (3.0 if id(p) in late else 6.0), n
    assert len(opt_a._tables) <= 8, "pointer tables must not accumulate per step count (ADVICE r3, low)"


# ---- row f4, second slice: forward / backward of update() on the library's kernels (engine/train.py, csrc/cdx_train.hip) ----
@pytest.mark.parametrize("shape", ["config2", "h4_dims_1_4_2", "conditional"])
def test_native_training_graph_matches_autograd(shape, amd_lib, monkeypatch):
    """JannerUNet1d with autograd ON on the device: the output and the gradient of EVERY parameter (conv weights / biases through the
    TN weight-gradient GEMM and the column sums, GroupNorm gains / shifts, the FiLM and embedding Linears that stay on ATen) and of the
    input, against torch.autograd of the module's own PyTorch forward on the same device.  config 2 (H = 32: stride-2 and transposed
    convs at three levels, a 23-channel first layer), the shipped H = 4 / dim_mult [1, 4, 2] net, a conditional call."""
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth
    if shape == "h4_dims_1_4_2":
        net, H, D = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 4, 2], kernel_size=5), 5), 4, 23
    else:
        net, H, D = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 5), 32, 23
    net = net.to(DEV)
    g = torch.Generator().manual_seed(2)
    B = 24
    x = torch.randn(B, H, D, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(0, 20, (B,), generator=g).to(DEV)
    cond = torch.randn(B, 32, generator=g).to(DEV) if shape == "conditional" else None
    wgt = torch.randn(B, H, D, generator=g).to(DEV)

    def run(native):
        monkeypatch.setenv("CDX_TRAIN_NATIVE", "1" if native else "0")
        net.zero_grad(set_to_none=True)
        x.grad = None
        fam = train.family_of(net, x)
        assert (fam is not None) == native and (fam is None or fam.name == "janner")
        y = net(x, t, cond)
        ((y * wgt).sum() / B).backward()
        return y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in net.named_parameters()}
    y1, gx1, gp1 = run(True)
    y0, gx0, gp0 = run(False)
    torch.cuda.synchronize()
    np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gx1.cpu().numpy(), gx0.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(gx0.abs().max()))
    assert set(gp1) == set(gp0)
    for n in gp0:
        scale = float(gp0[n].abs().max()) + 1e-12
        err = float((gp1[n] - gp0[n]).abs().max())
        assert err <= 2e-4 * scale, f"{n}: |d| = {err:.3e} at scale {scale:.3e}"
        assert gp1[n].is_contiguous() and gp1[n].shape == gp0[n].shape


@pytest.mark.parametrize("shape", ["dim32_scale", "dim64_bias", "cfg3_width"])
def test_native_chiunet_training_graph_matches_autograd(shape, amd_lib, monkeypatch):
    """Round 5 (VERDICT r4 missing #2 / next #8): ChiUNet1d with a global condition and autograd ON -- every Conv1d / ConvTranspose1d /
    GroupNorm -> Mish node and every block's FiLM Linear on the library's kernels (engine/train.py:chi_forward; reference
    nn_diffusion/chiunet.py:13-45,152-192).  Output, input gradient and the gradient of EVERY parameter against torch.autograd of the
    module's own PyTorch forward on the same device.  FiLM as (scale, bias) and as a bias; the config-3 width (GroupNorm groups of
    32 / 64 / 128 channels -- the 128-wide ones take the per-lane-pair path of cdx_groupnorm_bwd_f32 -- and K up to 10 240)."""
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth
    dim, scale, B = {"dim32_scale": (32, True, 12), "dim64_bias": (64, False, 12), "cfg3_width": (256, True, 6)}[shape]
    net = load_synth(amd_lib.ChiUNet1d(2, 5, 2, model_dim=dim, emb_dim=dim, dim_mult=[1, 2, 2], cond_predict_scale=scale,
                                       obs_as_global_cond=True), 9).to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 16, 2, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(0, 20, (B,), generator=g).to(DEV)
    cond = torch.randn(B, 2, 5, generator=g).to(DEV)
    wgt = torch.randn(B, 16, 2, generator=g).to(DEV)

    def run(native):
        monkeypatch.setenv("CDX_TRAIN_NATIVE", "1" if native else "0")
        net.zero_grad(set_to_none=True)
        x.grad = None
        fam = train.family_of(net, x, cond)
        assert (fam is not None) == native and (fam is None or fam.name == "chi")
        y = net(x, t, cond)
        ((y * wgt).sum() / B).backward()
        return y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in net.named_parameters()}
    y1, gx1, gp1 = run(True)
    y0, gx0, gp0 = run(False)
    torch.cuda.synchronize()
    ys = max(1.0, float(y0.abs().max()))
    np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), rtol=1e-4, atol=1e-4 * ys)
    np.testing.assert_allclose(gx1.cpu().numpy(), gx0.cpu().numpy(), rtol=1e-4, atol=2e-4 * float(gx0.abs().max()))
    assert set(gp1) == set(gp0)
    for n in gp0:
        sc = float(gp0[n].abs().max()) + 1e-12
        err = float((gp1[n] - gp0[n]).abs().max())
        assert err <= 3e-4 * sc, f"{n}: |d| = {err:.3e} at scale {sc:.3e}"
        assert gp1[n].is_contiguous() and gp1[n].shape == gp0[n].shape


@pytest.mark.parametrize("shape", ["dit_d64", "dit_cfg4", "idql_h64", "idql_cfg5", "newidql_cond"])
def test_native_transformer_and_resmlp_training_graphs_match_autograd(shape, amd_lib, monkeypatch):
    """Round 5 (VERDICT r4 missing #2 / next #8): DiT1d and IDQLMlp / NewIDQLMlp with autograd ON -- every Linear (cdx_gemm_f32, the
    transposed GEMM, cdx_conv_wgrad_f32), LayerNorm (+ adaLN modulate; cdx_layernorm_f32 / cdx_layernorm_bwd_f32), the attention core
    (cdx_attention_f32 / cdx_attention_bwd_f32) and the GELU(tanh) / Mish factors on the library's kernels (engine/train.py:dit_forward,
    idql_forward; reference nn_diffusion/dit.py:10-130, idqlmlp.py:9-49).  Output, input gradient and the gradient of EVERY parameter
    against torch.autograd of the module's own PyTorch forward on the same device: the config-4 net (d 320, 10 heads, 64 tokens), a
    small one (head_dim 16, 16 tokens), the config-5 net (hidden 1024 x 6 blocks) and conditional variants."""
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth
    g = torch.Generator().manual_seed(4)
    if shape.startswith("dit"):
        d, heads, T, B = (64, 4, 16, 6) if shape == "dit_d64" else (320, 10, 64, 4)
        net = load_synth(amd_lib.DiT1d(7, emb_dim=32, d_model=d, n_heads=heads, depth=2, timestep_emb_type="fourier"), 11).to(DEV)
        x = torch.randn(B, T, 7, generator=g).to(DEV).requires_grad_(True)
        t = torch.rand(B, generator=g).to(DEV)
        cond = torch.randn(B, 32, generator=g).to(DEV)
        sup = "dit"
    else:
        cls = amd_lib.NewIDQLMlp if shape == "newidql_cond" else amd_lib.IDQLMlp
        obs, h, nb, B = (0, 1024, 6, 24) if shape == "idql_cfg5" else (11, 64, 2, 9)
        net = load_synth(cls(obs, 15, emb_dim=32, hidden_dim=h, n_blocks=nb, dropout=0.0), 12).to(DEV)
        x = torch.randn(B, 15, generator=g).to(DEV).requires_grad_(True)
        t = torch.rand(B, generator=g).to(DEV)
        cond = torch.randn(B, obs, generator=g).to(DEV) if obs else None
        sup = "idql"
    wgt = torch.randn(*x.shape, generator=g).to(DEV)

    def run(native):
        monkeypatch.setenv("CDX_TRAIN_NATIVE", "1" if native else "0")
        net.zero_grad(set_to_none=True)
        x.grad = None
        fam = train.family_of(net, x, cond)
        assert (fam is not None) == native and (fam is None or fam.name == sup)
        y = net(x, t, cond)
        ((y * wgt).sum() / x.shape[0]).backward()
        return y.detach().clone(), x.grad.clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    y1, gx1, gp1 = run(True)
    y0, gx0, gp0 = run(False)
    torch.cuda.synchronize()
    ys = max(1.0, float(y0.abs().max()))
    np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), rtol=1e-4, atol=1e-4 * ys)
    np.testing.assert_allclose(gx1.cpu().numpy(), gx0.cpu().numpy(), rtol=1e-4, atol=2e-4 * float(gx0.abs().max()))
    assert set(gp1) == set(gp0)
    for n in gp0:
        if gp0[n] is None:                               # (the frozen frequencies of a Fourier timestep embedding)
            assert gp1[n] is None, n
            continue
        sc = float(gp0[n].abs().max()) + 1e-12
        err = float((gp1[n] - gp0[n]).abs().max())
        assert err <= 3e-4 * sc, f"{n}: |d| = {err:.3e} at scale {sc:.3e}"
        assert gp1[n].is_contiguous() and gp1[n].shape == gp0[n].shape


def test_halfdit_classifier_gradient_runs_on_the_library_nodes(amd_lib, monkeypatch):
    """VERDICT r4 missing #4: the guidance gradient of a HalfDiT1d classifier (reference nn_classifier/half_dit.py:9, classifier/base.py:
    74-79 differentiate logp with autograd) -- on the device the trunk's Linear / LayerNorm + modulate / attention nodes are library
    kernels forward AND backward (cdx_attention_bwd_f32 is called once per block), and logp / d logp / dx equal the CPU autograd of the
    same module at 1e-4."""
    from cleandiffuser_amd.engine import blocks
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.HalfDiT1d(7, 1, emb_dim=32, d_model=64, n_heads=4, depth=2), 13)
    with torch.no_grad():                                # (a fresh HalfDiT1d head is zero-initialised: give the gradient something to flow through)
        for lin in (net.final_layer.linear, net.final_layer.adaLN_modulation[-1]):
            lin.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(2)
    x, t, y = torch.randn(6, 16, 7, generator=g), torch.randint(0, 20, (6,), generator=g), torch.randn(6, 1, generator=g)
    clf_cpu = amd_lib.CumRewClassifier(net, device="cpu")
    clf_cpu.eval()
    lp0, g0 = clf_cpu.gradients(x.clone(), t, y)
    calls = {"n": 0}
    orig = blocks.attention_backward
    monkeypatch.setattr(blocks, "attention_backward", lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), orig(*a, **k))[1])
    from copy import deepcopy
    clf = amd_lib.CumRewClassifier(deepcopy(net), device=DEV)
    clf.eval()
    lp1, g1 = clf.gradients(x.clone().to(DEV), t.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    assert calls["n"] == 2, calls
    np.testing.assert_allclose(lp1.cpu().numpy(), lp0.numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g1.cpu().numpy(), g0.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(g0.abs().max())))
    assert float(g0.abs().max()) > 1e-3


def test_layernorm_and_attention_backward_kernels_match_autograd():
    """cdx_layernorm_bwd_f32 (affine, modulate, plain; C = 320 and the 4096-wide register variant) and cdx_attention_bwd_f32 (T = 64 /
    head_dim 32, T = 10 / head_dim 64, T = 33 / head_dim 24) against torch.autograd of the same op."""
    import torch.nn.functional as F
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(1)
    for M, C, T in ((192, 320, 64), (40, 4096, 10), (66, 72, 33)):
        x = torch.randn(M, C, generator=g).to(DEV).requires_grad_(True)
        dy = torch.randn(M, C, generator=g).to(DEV)
        gamma, beta = (torch.randn(C, generator=g).to(DEV).requires_grad_(True) for _ in range(2))
        mod = torch.randn(M // T, 2 * C, generator=g).to(DEV).requires_grad_(True)
        F.layer_norm(x, (C,), gamma, beta, 1e-5).backward(dy)
        dx, dyx = blocks.layernorm_backward(dy, x.detach(), gamma=gamma.detach(), eps=1e-5, want_dyxhat=True)
        torch.testing.assert_close(dx, x.grad, rtol=2e-4, atol=2e-5)
        torch.testing.assert_close(blocks.colsum(dyx), gamma.grad, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(blocks.colsum(dy), beta.grad, rtol=2e-4, atol=2e-4)
        x.grad = None
        scale, shift = mod[:, :C], mod[:, C:]
        y = (F.layer_norm(x, (C,), eps=1e-6).view(M // T, T, C) * (1 + scale[:, None]) + shift[:, None]).view(M, C)
        y.backward(dy)
        dx, dyx = blocks.layernorm_backward(dy, x.detach(), scale=scale.detach(), rows_per_mod=T, eps=1e-6, want_dyxhat=True)
        torch.testing.assert_close(dx, x.grad, rtol=2e-4, atol=2e-5)
        torch.testing.assert_close(torch.cat([dyx.view(M // T, T, C).sum(1), dy.view(M // T, T, C).sum(1)], 1), mod.grad, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(blocks.layernorm(x.detach(), scale=scale.detach(), shift=shift.detach(), rows_per_mod=T, eps=1e-6), y.detach(),
                                   rtol=1e-5, atol=1e-5)
    for B, T, H, dh in ((3, 64, 10, 32), (2, 10, 4, 64), (2, 33, 3, 24)):
        dm = H * dh
        qkv = torch.randn(B * T, 3 * dm, generator=g).to(DEV).requires_grad_(True)
        dout = torch.randn(B * T, dm, generator=g).to(DEV)
        q, k, v = (z.reshape(B, T, H, dh).transpose(1, 2) for z in qkv.chunk(3, dim=-1))
        o = (torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, dim=-1) @ v).transpose(1, 2).reshape(B * T, dm)
        torch.testing.assert_close(blocks.attention(qkv.detach().contiguous(), B, T, H), o.detach(), rtol=1e-4, atol=1e-5)
        o.backward(dout)
        got = blocks.attention_backward(qkv.detach().contiguous(), dout, B, T, H)
        torch.testing.assert_close(got, qkv.grad, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("M,C,T,blocks_of", [(66, 1500, 33, None), (66, 1500, 33, 1536), (40, 320, 10, 400), (24, 2050, 8, 2100), (35, 1023, 7, None),
                                             (6, 1, 3, None), (6, 1, 3, 9), (6, 63, 3, 70), (6, 65, 3, None), (6, 1024, 3, 1031),
                                             (6, 1025, 3, None), (6, 2048, 3, None), (6, 2049, 3, 2057)])
def test_layernorm_backward_against_float64_on_column_blocks(M, C, T, blocks_of):
    """cdx_layernorm_bwd_f32 against float64 autograd ON THE CPU: the <32> variant (1024 < C <= 2048), odd widths, and dy / x as column
    blocks of wider matrices (lddy != C, ldx != C, first column 3: no alignment to lean on).  M = 6: the widths at which the launcher
    changes instantiation (1024 | 1025, 2048 | 2049), one column short of / past a wave's 64 lanes, and a row of ONE column (xhat = 0,
    dx = 0), each on two rows more than a workgroup's four, contiguous or as a column block."""
    import torch.nn.functional as F
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(M + C)
    x, dy = torch.randn(M, C, generator=g) * 2 + 0.5, torch.randn(M, C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    mod = torch.randn(M // T, 2 * C, generator=g)
    if blocks_of:
        xd, dyd = (torch.randn(M, blocks_of, generator=g).to(DEV)[:, 3:3 + C].copy_(t) for t in (x, dy))
        assert xd.stride(0) == blocks_of
    else:
        xd, dyd = x.to(DEV), dy.to(DEV)
    x64, g64, m64 = (t.double().requires_grad_(True) for t in (x, gamma, mod))
    F.layer_norm(x64, (C,), g64, beta.double(), 1e-5).backward(dy.double())
    dx, dyx = blocks.layernorm_backward(dyd, xd, gamma=gamma.to(DEV), eps=1e-5, want_dyxhat=True)
    torch.testing.assert_close(dx.cpu().double(), x64.grad, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(dyx.cpu().double().sum(0), g64.grad, rtol=2e-4, atol=2e-4)
    x64.grad = None
    (F.layer_norm(x64, (C,), eps=1e-6).view(M // T, T, C) * (1 + m64[:, None, :C]) + m64[:, None, C:]).view(M, C).backward(dy.double())
    scale = mod.to(DEV)[:, :C]                               # (a column block itself: ldmod = 2 C)
    dx, dyx = blocks.layernorm_backward(dyd, xd, scale=scale, rows_per_mod=T, eps=1e-6, want_dyxhat=True)
    torch.testing.assert_close(dx.cpu().double(), x64.grad, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(dyx.cpu().double().view(M // T, T, C).sum(1), m64.grad[:, :C], rtol=2e-4, atol=2e-4)
    x64.grad = None
    F.layer_norm(x64, (C,), eps=1e-5).backward(dy.double())
    torch.testing.assert_close(blocks.layernorm_backward(dyd, xd, eps=1e-5).cpu().double(), x64.grad, rtol=2e-4, atol=2e-5)


def _mha_reference(q, k, v, B, H, mask, keep):
    """softmax(q k^T / sqrt(dh) + mask) o keep @ v in plain torch ops (what F.multi_head_attention_forward computes between the
    projections in train mode, with the dropout mask given instead of drawn)."""
    dm = q.shape[1]
    dh = dm // H
    qh, kh, vh = (z.reshape(B, -1, H, dh).transpose(1, 2) for z in (q, k, v))
    sc = qh @ kh.transpose(-1, -2) / dh ** 0.5
    p = torch.softmax(sc if mask is None else sc + mask, dim=-1)
    return ((p if keep is None else p * keep) @ vh).transpose(1, 2).reshape(-1, dm)


@pytest.mark.parametrize("B,Tq,Tk,H,dh,masked,drop", [(3, 10, 10, 4, 64, True, 0.3), (2, 16, 3, 4, 64, True, 0.3), (2, 64, 64, 10, 32, False, 0.1),
                                                      (5, 6, 4, 4, 16, True, 0.0), (1, 33, 17, 3, 24, False, 0.0)])
def test_mha_training_kernels_match_autograd_with_mask_and_dropout(B, Tq, Tk, H, dh, masked, drop):
    """cdx_mha_train_fwd_f32 / _bwd_f32 (ABI 15): the attention core of nn.MultiheadAttention in train mode -- additive mask (causal /
    staggered, -inf entries), dropout mask applied to the probabilities, q next to a packed [k | v] of another length (the memory
    cross-attention of nn.TransformerDecoderLayer) and packed [q | k | v] rows -- against torch.autograd of the same arithmetic with the
    SAME dropout mask (reference nn_diffusion/chitransformer.py:108-121,148-154)."""
    from cleandiffuser_amd.engine import train
    g = torch.Generator().manual_seed(B * 100 + Tq)
    dm = H * dh
    mask = None
    if masked:
        i, j = torch.meshgrid(torch.arange(Tq), torch.arange(Tk), indexing="ij")
        mask = torch.zeros(Tq, Tk).masked_fill(~(i >= j - 1), float("-inf")).to(DEV)
    keep = (torch.rand(B, H, Tq, Tk, generator=g) >= drop).float().div(1 - drop).to(DEV) if drop else None
    dout = torch.randn(B * Tq, dm, generator=g).to(DEV)
    # cross form: q (B * Tq, dm), kv packed (B * Tk, 2 dm)
    q = torch.randn(B * Tq, dm, generator=g).to(DEV).requires_grad_(True)
    kv = torch.randn(B * Tk, 2 * dm, generator=g).to(DEV).requires_grad_(True)
    ref = _mha_reference(q, kv[:, :dm], kv[:, dm:], B, H, mask, keep)
    ref.backward(dout)
    gq, gkv = q.grad.clone(), kv.grad.clone()
    q.grad = kv.grad = None
    out = train._MHA.apply(q, kv, B, H, mask, keep)
    out.backward(dout)
    torch.testing.assert_close(out.detach(), ref.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(q.grad, gq, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(kv.grad, gkv, rtol=2e-4, atol=2e-5)
    if Tq == Tk:                                          # packed self-attention form
        qkv = torch.randn(B * Tq, 3 * dm, generator=g).to(DEV).requires_grad_(True)
        ref = _mha_reference(qkv[:, :dm], qkv[:, dm:2 * dm], qkv[:, 2 * dm:], B, H, mask, keep)
        ref.backward(dout)
        want = qkv.grad.clone()
        qkv.grad = None
        out = train._MHA.apply(qkv, None, B, H, mask, keep)
        out.backward(dout)
        torch.testing.assert_close(out.detach(), ref.detach(), rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(qkv.grad, want, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("shape", ["pusht", "cond_encoder", "unconditional"])
def test_native_chitransformer_training_graph_matches_autograd(shape, amd_lib, monkeypatch):
    """VERDICT r4 missing #2, last backbone: ChiTransformer with autograd ON in TRAIN mode -- every Linear, LayerNorm and the three
    attention cores (memory self-attention, causal self-attention, staggered memory cross-attention) on the library's kernels
    (engine/train.py:chitf_forward; reference nn_diffusion/chitransformer.py:60-158): output, input gradient and the gradient of EVERY
    parameter against torch.autograd of nn.TransformerDecoder / nn.TransformerEncoder on the same device (dropout 0 on both sides)."""
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth
    g = torch.Generator().manual_seed(5)
    d, heads, layers, cl, ta, to, B = {"pusht": (256, 4, 8, 0, 10, 2, 8), "cond_encoder": (64, 4, 2, 2, 6, 3, 5), "unconditional": (128, 2, 2, 0, 16, 1, 4)}[shape]
    net = load_synth(amd_lib.ChiTransformer(3, 5, ta, to, d_model=d, nhead=heads, num_layers=layers, p_drop_attn=0.0, n_cond_layers=cl), 13).to(DEV)
    net.train()
    x = torch.randn(B, ta, 3, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(0, 20, (B,), generator=g).to(DEV)
    cond = None if shape == "unconditional" else torch.randn(B, to, 5, generator=g).to(DEV)
    wgt = torch.randn(*x.shape, generator=g).to(DEV)

    def run(native):
        monkeypatch.setenv("CDX_TRAIN_NATIVE", "1" if native else "0")
        net.zero_grad(set_to_none=True)
        x.grad = None
        fam = train.family_of(net, x, cond)
        assert (fam is not None) == native and (fam is None or fam.name == "chitf")
        y = net(x, t, cond)
        ((y * wgt).sum() / x.shape[0]).backward()
        return y.detach().clone(), x.grad.clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    y1, gx1, gp1 = run(True)
    y0, gx0, gp0 = run(False)
    torch.cuda.synchronize()
    np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(y0.abs().max())))
    np.testing.assert_allclose(gx1.cpu().numpy(), gx0.cpu().numpy(), rtol=1e-4, atol=2e-4 * float(gx0.abs().max()))
    assert set(gp1) == set(gp0)
    for n in gp0:
        if gp0[n] is None:                               # (cond_encoder: constructed by the reference, used by nothing; the frozen masks)
            assert gp1[n] is None, n
            continue
        sc = float(gp0[n].abs().max()) + 1e-12
        err = float((gp1[n] - gp0[n]).abs().max())
        assert err <= 3e-4 * sc, f"{n}: |d| = {err:.3e} at scale {sc:.3e}"
        assert gp1[n].shape == gp0[n].shape


@pytest.mark.parametrize("which", ["pearce_cfg1", "pearce_small", "sfbc"])
def test_native_pearce_and_sfbc_training_graphs_match_autograd(which, amd_lib, monkeypatch):
    """The last two denoisers the reference's pipelines train (dbc_*: PearceMlp = BASELINE config 1; sfbc_*: SfBCUNet) with autograd ON:
    Linear / GroupNorm1d / GELU / LeakyReLU / SiLU on the library's nodes (engine/train.py:pearce_forward, sfbc_forward; reference
    nn_diffusion/pearcemlp.py:10-77, sfbc_unet.py:9-82) -- output, input gradient and every parameter gradient against torch.autograd
    of the module's own forward on the same device; update() of either takes the HIP-graph step."""
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth
    g = torch.Generator().manual_seed(12)
    if which.startswith("pearce"):
        act, To, emb, hid, B = (6, 1, 128, 512, 64) if which == "pearce_cfg1" else (3, 2, 32, 64, 7)
        net = load_synth(amd_lib.PearceMlp(act, To=To, emb_dim=emb, hidden_dim=hid), 15).to(DEV)
        x, t, cond = torch.randn(B, act, generator=g), torch.randint(0, 100, (B,), generator=g), torch.randn(B, To, emb, generator=g)
        sup = "pearce"
    else:
        net = load_synth(amd_lib.SfBCUNet(6, emb_dim=64), 16).to(DEV)
        x, t, cond, sup = torch.randn(33, 6, generator=g), torch.rand(33, generator=g), torch.randn(33, 64, generator=g), "sfbc"
    net.train()
    x, t, cond = x.to(DEV).requires_grad_(True), t.to(DEV), cond.to(DEV)
    wgt = torch.randn(*x.shape, generator=g).to(DEV)

    def run(native):
        monkeypatch.setenv("CDX_TRAIN_NATIVE", "1" if native else "0")
        net.zero_grad(set_to_none=True)
        x.grad = None
        fam = train.family_of(net, x, cond)
        assert (fam is not None) == native and (fam is None or fam.name == sup)
        y = net(x, t, cond)
        ((y * wgt).sum() / x.shape[0]).backward()
        return y.detach().clone(), x.grad.clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    y1, gx1, gp1 = run(True)
    y0, gx0, gp0 = run(False)
    np.testing.assert_allclose(y1.cpu().numpy(), y0.cpu().numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(y0.abs().max())))
    np.testing.assert_allclose(gx1.cpu().numpy(), gx0.cpu().numpy(), rtol=1e-4, atol=2e-4 * float(gx0.abs().max()))
    for n in gp0:
        if gp0[n] is None:
            assert gp1[n] is None, n
            continue
        sc = float(gp0[n].abs().max()) + 1e-12
        assert float((gp1[n] - gp0[n]).abs().max()) <= 3e-4 * sc, n
    monkeypatch.setenv("CDX_TRAIN_NATIVE", "1")
    if which.startswith("pearce"):
        agent = amd_lib.DDPM(net, amd_lib.IdentityCondition(dropout=0.0), diffusion_steps=20, predict_noise=True, device=DEV)
    else:
        agent = amd_lib.ContinuousDiffusionSDE(net, amd_lib.IdentityCondition(dropout=0.0), predict_noise=True, noise_schedule="linear", device=DEV)
    agent.train()
    logs = [agent.update(x.detach(), cond)["loss"] for _ in range(3)]
    assert np.isfinite(logs).all() and any(isinstance(v, train.GraphedStep) for v in agent.__dict__.get("_cdx_graphed", {}).values())


def test_chitransformer_update_with_the_pipelines_dropout_runs_native_and_seeded(amd_lib, monkeypatch):
    """The dp_* pipelines train ChiTransformer with p_drop_attn = 0.3 (reference pipelines/dp_pusht.py:176-180): update() in train mode
    takes the native path (attention dropout masks drawn on the device and applied inside cdx_mha_train_*), is served by the HIP-graph
    step, reproduces under torch.manual_seed, and its dropout is REAL (train-mode losses differ from the eval-mode loss of the same
    draws; a module-level check pins the dropped attention against torch ops with the same mask)."""
    import torch.nn.functional as F
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth

    def make():
        net = load_synth(amd_lib.ChiTransformer(3, 5, 10, 2, d_model=64, nhead=4, num_layers=2, p_drop_attn=0.3), 14)
        return amd_lib.DDPM(net, amd_lib.IdentityCondition(dropout=0.0), diffusion_steps=20, predict_noise=True, grad_clip_norm=1.0, device=DEV)
    g = torch.Generator().manual_seed(6)
    x0, cond = torch.randn(16, 10, 3, generator=g).clamp(-1, 1).to(DEV), torch.randn(16, 2, 5, generator=g).to(DEV)
    calls = []
    orig = train.chitf_forward
    monkeypatch.setattr(train, "chitf_forward", lambda *a: (calls.append(1), orig(*a))[1])
    runs = []
    for _ in range(2):
        agent = make()
        agent.train()
        torch.manual_seed(77)
        runs.append([float(agent.update(x0, cond)["loss"]) for _ in range(4)])
    assert calls and np.isfinite(runs[0]).all()
    # seeded: same draws (timesteps, noise, every dropout mask), eager or replayed (weight-gradient sums use float atomics: ~1e-7)
    np.testing.assert_allclose(runs[0], runs[1], rtol=1e-3)
    assert any(isinstance(v, train.GraphedStep) for v in agent.__dict__.get("_cdx_graphed", {}).values())
    agent = make()
    torch.manual_seed(77)
    agent.train()
    l_train = float(agent.loss(x0, cond))
    torch.manual_seed(77)
    agent.eval()
    with torch.enable_grad():
        l_eval = float(agent.loss(x0, cond))
    assert abs(l_train - l_eval) > 1e-4 * abs(l_eval), (l_train, l_eval)
    # one attention module of that net, dropped with a known mask
    att = agent.model["diffusion"].decoder.layers[0].self_attn
    att.train()
    h2 = torch.randn(16 * 10, 64, generator=g).to(DEV).requires_grad_(True)
    keep = (torch.rand(16, 4, 10, 10, generator=g) >= 0.3).float().div(0.7).to(DEV)
    monkeypatch.setattr(train, "draw_keep", lambda *a: keep)
    mask = agent.model["diffusion"].mask.detach()
    out = train._self_attention(att, h2, 16, 10, mask)
    qkv = F.linear(h2, att.in_proj_weight, att.in_proj_bias)
    ref = F.linear(_mha_reference(qkv[:, :64], qkv[:, 64:128], qkv[:, 128:], 16, 4, mask, keep), att.out_proj.weight, att.out_proj.bias)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,L,C,G", [(5, 8, 32, 8), (7, 4, 1024, 8), (256, 32, 64, 8), (2, 16, 512, 8), (1, 8, 16, 8)])
def test_groupnorm_backward_adds_its_gain_and_shift_sums_onto_the_callers_buffers(B, L, C, G):
    """cdx_gn_args.dgamma_sum / dbeta_sum (ABI 15): the backward kernel's own float atomics -- four samples of a group per workgroup,
    combined in LDS first -- against the staged (B, C) partials + column sums of the same kernel and against torch.autograd; on top of
    what the buffers held; batches that are not a multiple of four; groups of 2 to 128 channels."""
    import torch.nn.functional as F
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(B * 7 + C)
    x = torch.randn(B * L, C, generator=g).to(DEV)
    dy = torch.randn(B * L, C, generator=g).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    dx0, dg0, db0 = blocks.groupnorm_backward(dy, x, gamma, beta, B, L, G, act="mish", param_grads=True)
    seed_g, seed_b = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    acc_g, acc_b = seed_g.clone(), seed_b.clone()
    dx1, none_g, none_b = blocks.groupnorm_backward(dy, x, gamma, beta, B, L, G, act="mish", param_grads=True, grads_out=(acc_g, acc_b))
    assert none_g is None and none_b is None and torch.equal(dx1, dx0)
    sc = float(dg0.abs().max()) + float(db0.abs().max())
    # (two orders of the same B * L terms per channel, and the difference acc - seed rounds at the accumulator's magnitude)
    torch.testing.assert_close(acc_g - seed_g, dg0, rtol=1e-4, atol=3e-5 * sc + 1e-6)
    torch.testing.assert_close(acc_b - seed_b, db0, rtol=1e-4, atol=3e-5 * sc + 1e-6)
    # autograd ON THE CPU: ATen's group_norm backward on this ROCm build returns wrong gain / shift gradients from batch 255 on
    # (tools/aten_groupnorm_backward_check.py, profiles/r04_aten_groupnorm_backward.txt)
    xr, gr, br = (t.cpu().clone().requires_grad_(True) for t in (x, gamma, beta))
    F.mish(F.group_norm(xr.view(B, L, C).permute(0, 2, 1), G, gr, br, 1e-5)).permute(0, 2, 1).reshape(B * L, C).backward(dy.cpu())
    torch.testing.assert_close((acc_g - seed_g).cpu(), gr.grad, rtol=2e-4, atol=5e-5 * sc + 1e-6)
    torch.testing.assert_close((acc_b - seed_b).cpu(), br.grad, rtol=2e-4, atol=5e-5 * sc + 1e-6)
    torch.testing.assert_close(dx1.cpu(), xr.grad, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("B,L,C,G", [(5, 8, 32, 8), (7, 4, 1024, 8), (256, 32, 64, 8), (3, 32, 512, 8), (3, 64, 512, 8), (1, 8, 16, 8),
                                     (6, 5, 2048, 8), (9, 3, 256, 8)])
@pytest.mark.parametrize("act", ["mish", "none"])
def test_groupnorm_backward_in_registers_and_its_position_sums(B, L, C, G, act):
    """Round 6: the group-in-registers backward kernel (x and dy read once as float4, float64 statistics) on the shapes it takes --
    power-of-two groups of 4..256 channels, L * cg <= 2048, odd lengths, batches that are not a multiple of four -- and the scalar
    kernel on the ones it refuses (2-channel groups, 4096 elements per group), both against torch.autograd on the CPU; and
    cdx_gn_args.dy_possum (ABI 17): dy summed over each sample's positions out of the same launch, written into a column block of a
    wider matrix, with each of the three parameter-gradient modes."""
    import torch.nn.functional as F
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(B * 11 + C + L)
    x = torch.randn(B * L, C, generator=g).to(DEV)
    dy = torch.randn(B * L, C, generator=g).to(DEV)
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    xr, gr, br = (t.cpu().clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.group_norm(xr.view(B, L, C).permute(0, 2, 1), G, gr, br, 1e-5)
    (F.mish(y) if act == "mish" else y).permute(0, 2, 1).reshape(B * L, C).backward(dy.cpu())
    want_sum = dy.view(B, L, C).sum(1).cpu()
    for mode in ("none", "parts", "sums"):
        wide = torch.full((B, C + 64), 7.0, device=DEV)
        possum = wide[:, 32:32 + C]
        acc = (torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
        out = blocks.groupnorm_backward(dy, x, gamma, beta, B, L, G, act=act, param_grads=mode != "none",
                                        grads_out=acc if mode == "sums" else None, possum_out=possum)
        dx = out if mode == "none" else out[0]
        torch.testing.assert_close(dx.cpu(), xr.grad, rtol=2e-4, atol=2e-5)
        torch.testing.assert_close(possum.cpu(), want_sum, rtol=1e-5, atol=1e-5)
        assert float(wide[:, :32].min()) == 7.0 and float(wide[:, 32 + C:].max()) == 7.0       # nothing outside the block
        if mode != "none":
            dg, db = (out[1], out[2]) if mode == "parts" else acc
            sc = float(gr.grad.abs().max()) + float(br.grad.abs().max())
            torch.testing.assert_close(dg.cpu(), gr.grad, rtol=2e-4, atol=5e-5 * sc + 1e-6)
            torch.testing.assert_close(db.cpu(), br.grad, rtol=2e-4, atol=5e-5 * sc + 1e-6)


@pytest.mark.parametrize("B,L,C,G", [(5, 8, 48, 4), (3, 200, 24, 2)])
@pytest.mark.parametrize("act", ["mish", "none"])
def test_groupnorm_backward_of_a_group_width_that_is_no_power_of_two(B, L, C, G, act):
    """Groups of 12 channels (96 and 2400 elements per group): dx out of the scalar kernel against float64 autograd on the CPU; the
    parameter gradients and position sums need a power-of-two width and are refused with CDX_EINVAL, nothing written."""
    import torch.nn.functional as F
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(B + L + C)
    x, dy = torch.randn(B * L, C, generator=g), torch.randn(B * L, C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = F.group_norm(xr.view(B, L, C).permute(0, 2, 1), G, gr, br, 1e-5)
    (F.mish(y) if act == "mish" else y).permute(0, 2, 1).reshape(B * L, C).backward(dy.double())
    args = (dy.to(DEV), x.to(DEV), gamma.to(DEV), beta.to(DEV), B, L, G)
    dx = blocks.groupnorm_backward(*args, act=act)
    torch.testing.assert_close(dx.cpu().double(), xr.grad, rtol=2e-4, atol=2e-5)
    acc = (torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
    for kw in (dict(param_grads=True), dict(param_grads=True, grads_out=acc), dict(possum_out=torch.zeros(B, C, device=DEV))):
        with pytest.raises(RuntimeError, match="failed with code -1"):
            blocks.groupnorm_backward(*args, act=act, **kw)
    assert float(acc[0].abs().max()) == 0.0 and float(acc[1].abs().max()) == 0.0


def test_relayout_kernel_builds_every_weight_layout_and_the_registry_keeps_them_current(amd_lib, monkeypatch):
    """cdx_relayout_f32 (ABI 15): every layout a training step needs of a conv / conv-transpose / linear weight -- whole parameters and a
    row slice of a packed one -- as ONE launch, bit-identical to the ATen permute / flip / stack expressions; and the registry around
    it (engine/train.py:_WeightPacks): ATen calls only in the first step, one launch after every parameter change, none without one,
    gradients equal to the CDX_TRAIN_PACKS=0 path throughout."""
    from cleandiffuser_amd.engine import blocks, train
    from cleandiffuser_amd.utils import load_synth
    g = torch.Generator().manual_seed(2)
    jobs, want = [], []
    for kind in ("conv", "convt_bwd", "conv_bwd", "conv_s2_mid", "conv_s2_outer", "convt_even", "convt_odd", "linear_t"):
        k = 3 if kind.startswith("conv_s2") else (4 if kind.startswith("convt") else 5)
        full = (torch.randn(40, 24, generator=g) if kind == "linear_t" else torch.randn(40, 24, k, generator=g)).to(DEV)
        for w in (full, full[8:32]):
            shape, n, st, off = train._geom(kind, w)
            dst = torch.full(shape, float("nan"), device=DEV)
            jobs.append((w, off, dst, n, st))
            want.append(train._aten_pack(kind, w))
    big = torch.randn(300, 70, 5, generator=g).to(DEV)         # several chunks, a ragged last one
    shape, n, st, off = train._geom("conv_bwd", big)
    jobs.append((big, off, torch.empty(shape, device=DEV), n, st))
    want.append(train._aten_pack("conv_bwd", big))
    blocks.relayout(blocks.relayout_table(jobs, DEV))
    for (_, _, dst, _, _), w in zip(jobs, want):
        assert torch.equal(dst, w)
    # the registry over three optimiser steps of a small U-Net
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "0")
    calls = {"aten": 0, "launch": 0}
    orig_pack, orig_launch = train._aten_pack, blocks.relayout
    def counted_pack(k, w):                               # (a 1-tap weight is its own layout: the "pack" is a view, no launch -- not counted)
        t = orig_pack(k, w)
        calls["aten"] += int(t.untyped_storage().data_ptr() != w.untyped_storage().data_ptr())
        return t
    monkeypatch.setattr(train, "_aten_pack", counted_pack)
    monkeypatch.setattr(blocks, "relayout", lambda t: (calls.__setitem__("launch", calls["launch"] + 1), orig_launch(t))[1])

    def make():
        net = load_synth(amd_lib.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=5), 3)
        return amd_lib.DiscreteDiffusionSDE(net, None, diffusion_steps=20, grad_clip_norm=1.0, device=DEV)
    x0 = torch.randn(12, 8, 6, generator=g).to(DEV)
    runs = {}
    for packs in ("1", "0"):
        monkeypatch.setenv("CDX_TRAIN_PACKS", packs)
        agent = make()
        agent.train()
        torch.manual_seed(3)
        per_step = []
        for step in range(3):
            before = dict(calls)
            log = agent.update(x0)
            per_step.append((calls["aten"] - before["aten"], calls["launch"] - before["launch"], float(log["loss"]), float(log["grad_norm"])))
        before = dict(calls)
        agent.loss(x0).backward()                          # no parameter change since the last forward... (the optimiser stepped: one launch)
        agent.loss(x0).backward()                          # ...and now really none
        per_step.append((calls["aten"] - before["aten"], calls["launch"] - before["launch"], 0.0, 0.0))
        runs[packs] = per_step
    on, off = runs["1"], runs["0"]
    assert on[0][0] > 0 and on[0][1] == 0 and on[1][:2] == (0, 1) and on[2][:2] == (0, 1) and on[3][:2] == (0, 1), on
    assert all(r[1] == 0 and r[0] > 0 for r in off[:3]), off
    np.testing.assert_allclose([r[2:] for r in on[:3]], [r[2:] for r in off[:3]], rtol=1e-5)


@pytest.mark.parametrize("kind", ["janner", "chiunet", "dit"])
def test_update_accumulates_parameter_gradients_in_place(kind, amd_lib, monkeypatch):
    """Inside update()'s backward (engine/train.py:grads_in_place) the weight / bias / gain sums are added straight into ``p.grad`` by the
    kernels that produce them (no zero-filled staging buffer, no AccumulateGrad add): same gradients as autograd's own accumulation
    (CDX_TRAIN_INPLACE_GRADS=0), on top of whatever ``.grad`` already held, with FEWER launches; a parameter with a hook keeps autograd's
    accumulation (the hook fires); outside update() -- torch.autograd.grad over loss() -- nothing touches ``.grad``."""
    from torch.profiler import profile, ProfilerActivity
    from cleandiffuser_amd.engine import train
    from cleandiffuser_amd.utils import load_synth
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "0")
    g = torch.Generator().manual_seed(8)
    if kind == "janner":
        net = load_synth(amd_lib.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=5), 3)
        agent = amd_lib.DiscreteDiffusionSDE(net, None, diffusion_steps=20, device=DEV)
        x0, cond = torch.randn(12, 8, 6, generator=g).to(DEV), None
    elif kind == "chiunet":
        net = load_synth(amd_lib.ChiUNet1d(2, 5, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], obs_as_global_cond=True), 4)
        agent = amd_lib.DDPM(net, amd_lib.IdentityCondition(dropout=0.0), diffusion_steps=20, device=DEV)
        x0, cond = torch.randn(12, 16, 2, generator=g).clamp(-1, 1).to(DEV), torch.randn(12, 2, 5, generator=g).to(DEV)
    else:
        net = load_synth(amd_lib.DiT1d(7, emb_dim=32, d_model=64, n_heads=4, depth=2, timestep_emb_type="fourier"), 5)
        agent = amd_lib.ContinuousDiffusionSDE(net, None, predict_noise=True, noise_schedule="linear", device=DEV)
        x0, cond = torch.randn(12, 16, 7, generator=g).to(DEV), None
    agent.train()
    params = dict(agent.model.named_parameters())
    fired = []
    hooked = [n for n, p in params.items() if p.dim() == 1][-1]
    params[hooked].register_hook(lambda gr: fired.append(1))

    def backward(in_place, seed_grads):
        monkeypatch.setenv("CDX_TRAIN_INPLACE_GRADS", "1" if in_place else "0")
        for n, p in params.items():
            p.grad = None if seed_grads is None else seed_grads[n].clone()
        torch.manual_seed(5)
        def region():
            loss = agent.loss(x0, cond)
            with train.grads_in_place():
                loss.backward()
        prof, _ = _profiled(region, [ProfilerActivity.CUDA], rerun=False)      # (a second pass would accumulate onto the gradients compared below)
        launches = sum(e.count for e in prof.key_averages() if e.device_time_total > 0)
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in params.items()}, launches
    g0, n0 = backward(False, None)
    g1, n1 = backward(True, None)
    assert len(fired) == 2
    fired.clear()
    seeds = {n: torch.randn(p.shape, generator=g).to(DEV) for n, p in params.items()}
    _, n0 = backward(False, seeds)                       # steady state: the gradients exist (zeroed in place by the optimiser)
    g2, n1 = backward(True, seeds)
    for n in params:
        if g0[n] is None:
            assert g1[n] is None or float(g1[n].abs().max()) == 0.0, n
            continue
        sc = float(g0[n].abs().max()) + 1e-12
        assert float((g1[n] - g0[n]).abs().max()) <= 1e-5 * sc + 1e-7, n
        assert float((g2[n] - seeds[n] - g0[n]).abs().max()) <= 1e-5 * (sc + float(seeds[n].abs().max())), n
    assert n1 < n0 - len(params) // 2, (n1, n0, len(params))            # a fill and an add per parameter pair and more are gone
    print(f"{kind}: {n0} launches with autograd's accumulation, {n1} with in-place sums ({len(params)} parameters)")
    # outside update(): the functional API gets real tensors and leaves .grad alone
    for p in params.values():
        p.grad = None
    torch.manual_seed(5)
    want = [p for p in params.values() if p.requires_grad]
    got = torch.autograd.grad(agent.loss(x0, cond), want, allow_unused=True)
    assert all(p.grad is None for p in params.values())
    for (n, p), gr in zip([(n, p) for n, p in params.items() if p.requires_grad], got):
        if g0[n] is not None:
            assert gr is not None and float((gr - g0[n]).abs().max()) <= 1e-5 * float(g0[n].abs().max()) + 1e-7, n
    # and update() itself still lands where the optimiser expects: every written gradient counts as written
    log = agent.update(x0, cond) if cond is not None else agent.update(x0)
    assert np.isfinite(log["loss"])


def test_chiunet_update_runs_without_aten_conv_or_groupnorm_kernels(amd_lib, monkeypatch):
    """update() of the dp_pusht configuration (ChiUNet1d under the legacy DDPM class) dispatches no ATen / MIOpen convolution and no
    group_norm kernel, forward or backward.  (Eager step: the profiler does not attribute the kernels of a HIP-graph replay by name.)"""
    from torch.profiler import profile, ProfilerActivity
    from cleandiffuser_amd.utils import load_synth
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "0")
    net = load_synth(amd_lib.ChiUNet1d(2, 5, 2, model_dim=64, emb_dim=64, dim_mult=[1, 2, 2], obs_as_global_cond=True), 7)
    agent = amd_lib.DDPM(net, amd_lib.IdentityCondition(dropout=0.0), diffusion_steps=20, predict_noise=True, grad_clip_norm=1.0, device=DEV)
    agent.train()
    g = torch.Generator().manual_seed(3)
    x0, cond = torch.randn(64, 16, 2, generator=g).clamp(-1, 1).to(DEV), torch.randn(64, 2, 5, generator=g).to(DEV)
    agent.update(x0, cond)
    prof, log = _profiled(lambda: agent.update(x0, cond))
    assert np.isfinite(log["loss"])
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if any(k in n.lower() for k in ("convolution", "miopen", "group_norm", "conv1d", "conv_transpose"))]
    assert not bad, bad
    assert any("cdx_gemm_kernel" in n for n in names) and any("cdx_groupnorm_bwd" in n for n in names), names


def test_update_runs_without_aten_conv_or_groupnorm_kernels(amd_lib):
    """VERDICT r3 'next' #5: update() of config 2 at B = 256 -- loss, backward, clip, AdamW, EMA -- dispatches NO ATen / MIOpen
    convolution and no group_norm kernel, forward or backward: the profiler sees the library's GEMM / weight-gradient / GroupNorm /
    column-sum / optimiser kernels plus ATen's elementwise glue; and three updates land on the same loss values, gradient norms and
    weights as the reference sequence on the CPU (autograd, clip_grad_norm_, AdamW, EMA) fed the same draws.
    (The twin runs on the CPU because ATen's own group_norm backward on THIS ROCm build returns gain / shift gradients that are off by
    100 % once the batch reaches 255 -- tools/aten_groupnorm_backward_check.py, profiles/r04_aten_groupnorm_backward.txt: float64 on the CPU agrees with
    the library's kernel to 5e-5 and with ATen-CPU, not with ATen-GPU.  Up to B = 128 the device twin agrees too:
    test_native_training_graph_matches_autograd.)"""
    from copy import deepcopy
    from torch.profiler import profile, ProfilerActivity
    from oracle.train_cases import cpu_rng
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 7)
    fm = torch.zeros(32, 23)
    fm[0, :17] = 1.0
    mk = lambda n, dev: amd_lib.DiscreteDiffusionSDE(n, None, fix_mask=fm, diffusion_steps=20, predict_noise=False, grad_clip_norm=1.0,  # noqa: E731
                                                     device=dev)
    a, b = mk(deepcopy(net), DEV), mk(deepcopy(net), "cpu")
    b.optimizer = torch.optim.AdamW(b.model.parameters(), lr=2e-4, weight_decay=1e-5)        # the stock sequence
    x0 = torch.randn(256, 32, 23, generator=torch.Generator().manual_seed(3))
    with cpu_rng(DEV):
        torch.manual_seed(11)
        la_all = [a.update(x0.to(DEV)) for _ in range(3)]
    torch.manual_seed(11)
    lb_all = [b.update(x0) for _ in range(3)]
    prof, _ = _profiled(lambda: a.update(x0.to(DEV)), rerun=False)       # (a fifth update would leave the state budget checked below)
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if any(w in n.lower() for w in ("convolution", "conv1d", "conv_transpose", "miopen", "group_norm", "native_batch_norm"))]
    assert not bad, f"ATen convolution / group_norm ops in a native update(): {bad}"
    assert any("cdx_conv_wgrad" in n for n in names) and any("cdx_groupnorm_bwd_" in n for n in names), names
    # round 6: the weight-gradient products of all 65 layers leave the step's backward pass as ceil(65 / 32) = 3 batched launches
    assert sum(int(e.count) for e in prof.key_averages() if "cdx_conv_wgrad_batch_kernel" in e.key) <= 3 or os.environ.get("CDX_TRAIN_WGRAD_BATCH") == "0"
    for la, lb in zip(la_all, lb_all):
        assert abs(la["loss"] - lb["loss"]) <= 1e-5 * max(1.0, abs(lb["loss"]))
        assert abs(float(la["grad_norm"]) - float(lb["grad_norm"])) <= 1e-4 * float(lb["grad_norm"])
    # (the profiled fourth update moved only `a`: compare the state after three through the EMA copies' distance budget instead --
    #  the EMA moves by (1 - 0.995) of one more AdamW step of lr 2e-4)
    for (n, p), q in zip(a.model_ema.named_parameters(), b.model_ema.parameters()):
        assert float((p.detach().cpu() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(q.detach().abs().max())) + 1.1e-6, n


def test_fused_adam_matches_torch_adam_over_ten_steps():
    """FusedAdam.step (cdx_optim_f32 mode CDX_OPT_ADAM, ABI 16: clip -> g += wd p -> moments -> bias-corrected step -> EMA) against
    torch.optim.Adam (L2 weight decay, the optimiser of the reference's classifiers, classifier/base.py:24) + clip_grad_norm_ + the EMA
    loop fed the SAME gradients for 10 steps; its state_dict loads into the stock class."""
    from copy import deepcopy
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.nn_classifier import HalfJannerUNet1d
    from cleandiffuser_amd.utils import load_synth
    torch.manual_seed(0)
    net_a = load_synth(HalfJannerUNet1d(16, 6, out_dim=1, kernel_size=3, model_dim=16, emb_dim=16, dim_mult=(1, 2, 2)), 3).to(DEV)
    net_b, ema_a = deepcopy(net_a), deepcopy(net_a).requires_grad_(False)
    ema_b = deepcopy(ema_a)
    kw = dict(lr=3e-3, weight_decay=5e-2, betas=(0.9, 0.99))
    opt_a, opt_b = FusedAdam(net_a.parameters(), **kw), torch.optim.Adam(net_b.parameters(), **kw)
    assert opt_a.native() and isinstance(opt_a, torch.optim.Adam) and not isinstance(opt_a, torch.optim.AdamW)
    rate, max_norm = 0.9, 0.7
    for step in range(10):
        grads = [torch.randn_like(p) * (0.02 if step % 3 else 2.0) for p in net_a.parameters()]
        for p, q, g in zip(net_a.parameters(), net_b.parameters(), grads):
            p.grad, q.grad = g.clone(), g.clone()
        opt_a.step(max_norm=max_norm, ema=(net_a, ema_a, rate))
        norm_b = torch.nn.utils.clip_grad_norm_(net_b.parameters(), max_norm)
        opt_b.step()
        with torch.no_grad():
            for q, e in zip(net_b.parameters(), ema_b.parameters()):
                e.mul_(rate).add_(q.detach(), alpha=1 - rate)
        torch.testing.assert_close(opt_a.last_grad_norm, norm_b, rtol=2e-6, atol=0)
    for (n, p), q, ea, eb in zip(net_a.named_parameters(), net_b.parameters(), ema_a.parameters(), ema_b.parameters()):
        scale = max(float(q.detach().abs().max()), 1.0)
        assert float((p.detach() - q.detach()).abs().max()) <= 1e-6 * scale, n
        assert float((ea - eb).abs().max()) <= 1e-6 * scale, n
        torch.testing.assert_close(opt_a.state[p]["exp_avg_sq"], opt_b.state[q]["exp_avg_sq"], rtol=1e-5, atol=1e-12)
    torch.optim.Adam(net_b.parameters(), **kw).load_state_dict(opt_a.state_dict())


@pytest.mark.parametrize("n_jobs", [1, 5, 37])
def test_batched_weight_gradients_equal_the_single_launches(n_jobs):
    """cdx_conv_wgrad_batch_f32 (ABI 16): the products of many layers in ceil(n / 32) launches, job table as the kernel argument --
    convolutions of 1-5 taps, the stride-2 downsample, a transposed conv's operand order, Linears, widths that are no tile multiple,
    with and without the bias sum -- ADDED onto what the gradient tensors hold, against cdx_conv_wgrad_f32 per product (same kernel body)
    and against a float64 einsum."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(n_jobs)
    shapes = [(5, 1, 1, 32, 64), (3, 2, 1, 64, 64), (1, 1, 0, 23, 32), (5, 1, 2, 128, 96), (1, 1, 0, 256, 40), (3, 1, 1, 16, 16), (4, 1, 1, 32, 32)]
    jobs, refs, singles = [], [], []
    for j in range(n_jobs):
        taps, stride, pad, ca, cb = shapes[j % len(shapes)]
        batch = int(torch.randint(2, 9, (1,), generator=g))
        l_q = 16 if stride == 1 else 32
        l_p = (l_q + 2 * pad - taps) // stride + 1
        p = torch.randn(batch * l_p, ca, generator=g).to(DEV)
        q = torch.randn(batch * l_q, cb, generator=g).to(DEV)
        seed_w, seed_b = torch.randn(ca, cb, taps, generator=g).to(DEV), torch.randn(ca, generator=g).to(DEV)
        want_db = j % 2 == 0
        dw, db = seed_w.clone(), (seed_b.clone() if want_db else None)
        jobs.append((p, q, batch, l_p, l_q, taps, stride, pad, dw, db))
        one = blocks.conv_wgrad(p, q, batch, l_p, l_q, taps, stride, pad, bias_grad=want_db)
        singles.append((one[0] if want_db else one, one[1] if want_db else None))
        p3, q3 = p.double().view(batch, l_p, ca).cpu(), q.double().view(batch, l_q, cb).cpu()
        ref = torch.zeros(ca, cb, taps, dtype=torch.float64)
        m = torch.arange(l_p)
        for t in range(taps):
            idx = m * stride + t - pad
            ok = (idx >= 0) & (idx < l_q)
            ref[:, :, t] = torch.einsum("nma,nmb->ab", p3[:, ok], q3[:, idx[ok]])
        refs.append((seed_w.double().cpu() + ref, seed_b.double().cpu() + p.double().cpu().sum(0)))
    # (a product over zero rows -- an empty batch -- rides along: left out like conv_wgrad leaves it out, no launch, nothing added)
    keep_w, keep_b = torch.randn(8, 8, 3, generator=g).to(DEV), torch.randn(8, generator=g).to(DEV)
    empty = (torch.zeros(0, 8, device=DEV), torch.zeros(0, 8, device=DEV), 0, 16, 16, 3, 1, 1, keep_w.clone(), keep_b.clone())
    assert blocks.conv_wgrad_batch([empty] + jobs) == -(-n_jobs // 32) and blocks.conv_wgrad_batch([empty]) == 0
    torch.cuda.synchronize()
    assert torch.equal(empty[8], keep_w) and torch.equal(empty[9], keep_b)
    for (p, q, batch, l_p, l_q, taps, stride, pad, dw, db), (rw, rb), (sw, sb) in zip(jobs, refs, singles):
        scale = max(1.0, float(rw.abs().max()))
        assert float((dw.double().cpu() - rw).abs().max()) <= 2e-5 * scale
        if db is not None:
            assert float((db.double().cpu() - rb).abs().max()) <= 2e-5 * max(1.0, float(rb.abs().max()))


def _wgrad_ref(p, q, batch, l_p, l_q, taps, stride, pad):
    p3, q3 = p.double().view(batch, l_p, -1), q.double().view(batch, l_q, -1)
    ref = torch.zeros(p3.shape[2], q3.shape[2], taps, dtype=torch.float64)
    m = torch.arange(l_p)
    for t in range(taps):
        idx = m * stride + t - pad
        ok = (idx >= 0) & (idx < l_q)
        ref[:, :, t] = torch.einsum("nma,nmb->ab", p3[:, ok], q3[:, idx[ok]])
    return ref


# (batch, l_p, l_q, taps, stride, pad, ca, cb): 256 x 32 = 512 whole 16-row chunks; 255 x 31 = 7905 rows = 494 chunks + 1 row
WGRAD_MANY_SLICES = [(256, 32, 32, 1, 1, 0, 64, 64), (255, 31, 31, 1, 1, 0, 23, 130), (255, 31, 31, 5, 1, 2, 65, 23), (256, 32, 32, 5, 1, 2, 130, 65),
                     (255, 31, 31, 16, 1, 8, 23, 64), (256, 16, 31, 3, 2, 1, 64, 130), (255, 31, 63, 3, 2, 1, 130, 23), (256, 32, 64, 4, 2, 1, 65, 64)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("batch,l_p,l_q,taps,stride,pad,ca,cb", WGRAD_MANY_SLICES)
def test_weight_gradients_over_many_row_slices_against_float64(batch, l_p, l_q, taps, stride, pad, ca, cb, bias):
    """The accumulation every real update() uses -- thousands of rows cut into up to 64 slices, each ending in float atomics onto the
    gradient -- against the float64 einsum: slice counts chosen by the library (0), one slice, 7 slices of unequal length, and 64
    (of 7905 rows = 495 chunks: 8 chunks per slice, the last two slices EMPTY and the one before ends in a one-row chunk); the same
    products through the batched launch; 1 / 3 / 4 / 5 / 16 taps, stride 2 over an odd length, widths 23 / 64 / 65 / 130; ADDED onto
    what the gradient holds; twice (float atomics: the two runs agree within the bar, not bit for bit)."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(batch + taps * 7 + ca)
    p, q = torch.randn(batch * l_p, ca, generator=g), torch.randn(batch * l_q, cb, generator=g)
    seed_w, seed_b = torch.randn(ca, cb, taps, generator=g), torch.randn(ca, generator=g)
    rw = seed_w.double() + _wgrad_ref(p, q, batch, l_p, l_q, taps, stride, pad)
    rb = seed_b.double() + p.double().sum(0)
    bar_w, bar_b = 2e-5 * max(1.0, float(rw.abs().max())), 2e-5 * max(1.0, float(rb.abs().max()))
    pd, qd = p.to(DEV), q.to(DEV)

    def run(k_split):
        dw, db = seed_w.clone().to(DEV), (seed_b.clone().to(DEV) if bias else None)
        if k_split == "batch":
            assert blocks.conv_wgrad_batch([(pd, qd, batch, l_p, l_q, taps, stride, pad, dw, db)]) == 1
        else:
            blocks.conv_wgrad(pd, qd, batch, l_p, l_q, taps, stride, pad, k_split=k_split, bias_grad=bias, dw_out=dw, db_out=db)
        return dw.cpu().double(), (db.cpu().double() if bias else None)
    for k_split in (0, 1, 7, 64, "batch"):
        (w1, b1), (w2, b2) = run(k_split), run(k_split)
        for w in (w1, w2):
            assert float((w - rw).abs().max()) <= bar_w, (k_split, float((w - rw).abs().max()), bar_w)
        assert float((w1 - w2).abs().max()) <= bar_w, k_split
        if bias:
            for b in (b1, b2):
                assert float((b - rb).abs().max()) <= bar_b, (k_split, float((b - rb).abs().max()), bar_b)
            assert float((b1 - b2).abs().max()) <= bar_b, k_split


def test_weight_gradients_of_operands_whose_first_element_is_not_16_byte_aligned():
    """wg_load4 takes its float4 load from the row stride and the column alone.  blocks.conv_wgrad / conv_wgrad_batch accept any strided
    view, so they copy an operand with a 4-float row stride whose base is not 16-byte aligned: a column block starting at an odd
    column, a contiguous matrix cut out of a flat buffer at an odd offset (``.contiguous()`` returns such a view unchanged)."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(9)
    batch, l, ca, cb = 6, 16, 64, 32
    p = torch.randn(batch * l, ca + 8, generator=g).to(DEV)[:, 1:1 + ca]
    q = torch.randn(1 + batch * l * cb, generator=g).to(DEV)[1:].view(batch * l, cb)
    assert p.stride(0) % 4 == 0 and p.data_ptr() % 16 != 0 and q.is_contiguous() and q.data_ptr() % 16 != 0
    assert all(blocks._wgrad_operand(t).data_ptr() % 16 == 0 and torch.equal(blocks._wgrad_operand(t), t) for t in (p, q))
    ref = _wgrad_ref(p.cpu(), q.cpu(), batch, l, l, 3, 1, 1)
    rb = p.double().cpu().sum(0)
    dw, db = blocks.conv_wgrad(p, q, batch, l, l, 3, 1, 1, bias_grad=True)
    jobs = [(p, q, batch, l, l, 3, 1, 1, torch.zeros(ca, cb, 3, device=DEV), torch.zeros(ca, device=DEV)),
            (q, p, batch, l, l, 3, 1, 1, torch.zeros(cb, ca, 3, device=DEV), None)]
    assert blocks.conv_wgrad_batch(jobs) == 1
    bar = 2e-5 * max(1.0, float(ref.abs().max()))
    assert float((dw.double().cpu() - ref).abs().max()) <= bar and float((jobs[0][8].double().cpu() - ref).abs().max()) <= bar
    assert float((db.double().cpu() - rb).abs().max()) <= bar and float((jobs[0][9].double().cpu() - rb).abs().max()) <= bar
    ref_t = _wgrad_ref(q.cpu(), p.cpu(), batch, l, l, 3, 1, 1)
    assert float((jobs[1][8].double().cpu() - ref_t).abs().max()) <= 2e-5 * max(1.0, float(ref_t.abs().max()))


def test_a_failed_capture_falls_back_to_the_eager_step_and_keeps_earlier_gradients(amd_lib, monkeypatch):
    """(i) a capture that fails -- here: user code that raises only while the stream is capturing, which the eager probe cannot
    see -- must not leave update() with an exception: the agent steps eagerly from then on, generators and gradients as before the
    attempt.  (An ILLEGAL CUDA call under capture -- a synchronisation -- invalidates the capture inside the driver; torch's
    capture_end then throws before it un-registers its generator and allocator pool, which no Python code can repair: that class of
    failure is what the eager probe in front of the capture exists for.)  (ii) gradients a caller accumulated BEFORE the first update() are part of that update (the reference's
    update() adds onto them), also when the step is captured."""
    from copy import deepcopy
    from cleandiffuser_amd.utils import load_synth
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "auto")
    net = load_synth(amd_lib.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=5), 5)
    mk = lambda: amd_lib.DiscreteDiffusionSDE(deepcopy(net), None, diffusion_steps=20, predict_noise=False, grad_clip_norm=1.0, device=DEV)  # noqa: E731
    x0 = torch.randn(8, 8, 6, generator=torch.Generator().manual_seed(1)).to(DEV)
    # (i)
    a = mk()
    real_loss = a.loss

    def loss(x, c=None, **kw):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("this loss() cannot be captured")
        return real_loss(x, c, **kw)
    a.loss = loss
    log = a.update(x0)
    assert np.isfinite(log["loss"]) and a.__dict__.get("_cdx_graph_off", "").startswith("capture failed"), a.__dict__.get("_cdx_graph_off")
    assert np.isfinite(a.update(x0)["loss"]) and not torch.cuda.is_current_stream_capturing()
    # (ii) the same seeded draws with and without earlier gradients: the parameter updates must differ by what the earlier gradients add
    b, c = mk(), mk()
    extra = [0.05 * torch.randn_like(p) for p in b.model.parameters()]
    for p, e in zip(b.model.parameters(), extra):
        p.grad = e.clone()
    for p in c.model.parameters():
        p.grad = None
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "0")
    for p, e in zip(c.model.parameters(), extra):
        p.grad = e.clone()
    torch.manual_seed(3)
    lc = c.update(x0)                                   # eager: loss.backward() accumulates onto the earlier gradients
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "auto")
    torch.manual_seed(3)
    lb = b.update(x0)                                   # first update(): builds the graph, must accumulate likewise
    assert b.__dict__.get("_cdx_graphed") and not b.__dict__.get("_cdx_graph_off")
    assert abs(float(lb["grad_norm"]) - float(lc["grad_norm"])) <= 2e-5 * float(lc["grad_norm"]), (lb, lc)
    for (n, p), q in zip(b.model.named_parameters(), c.model.parameters()):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(q.detach().abs().max())), n


def test_critic_and_inverse_dynamics_updates_run_on_library_kernels(amd_lib):
    """VERDICT r5 'missing' #6: the heads trained NEXT to a denoiser -- IQL's V / twin-Q steps with the Polyak target (reference
    utils/iql.py:40-95; pipelines/idql_d4rl_mujoco.py), the inverse-dynamics heads' ``update`` (invdynamic/mlp.py:63, :199) -- on the
    device: their Linear / LayerNorm / activation nodes are library launches forward and backward (no ATen addmm / layer_norm kernel in
    the profile), the Adam steps and the Polyak update are cdx_optim_f32 launches, and five steps land on the parameters of the same
    classes run on the CPU (stock torch modules, torch.optim.Adam)."""
    from copy import deepcopy
    from torch.profiler import profile, ProfilerActivity
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.invdynamic import FancyMlpInvDynamic, MlpInvDynamic
    from cleandiffuser_amd.utils import IQL, load_synth
    g = torch.Generator().manual_seed(9)
    obs, act, nxt = torch.randn(64, 11, generator=g), torch.randn(64, 3, generator=g).tanh(), torch.randn(64, 11, generator=g)
    rew, done = torch.randn(64, 1, generator=g), (torch.rand(64, 1, generator=g) < 0.1).float()
    iql_c = load_synth(IQL(11, 3, hidden_dim=64), 21)
    iql_c.Q_targ.load_state_dict(iql_c.Q.state_dict())
    iql_g = deepcopy(iql_c).to(DEV)
    iql_g.optimV, iql_g.optimQ = FusedAdam(iql_g.V.parameters(), lr=3e-4), FusedAdam(iql_g.Q.parameters(), lr=3e-4)
    iql_c.optimV, iql_c.optimQ = torch.optim.Adam(iql_c.V.parameters(), lr=3e-4), torch.optim.Adam(iql_c.Q.parameters(), lr=3e-4)
    assert iql_g.optimV.native()
    d = lambda t: t.to(DEV)  # noqa: E731
    for _ in range(5):
        lv_c, lq_c = iql_c.update_V(obs, act), iql_c.update_Q(obs, act, rew, nxt, done)
        lv_g, lq_g = iql_g.update_V(d(obs), d(act)), iql_g.update_Q(d(obs), d(act), d(rew), d(nxt), d(done))
        assert abs(lv_c - lv_g) <= 2e-5 * max(1.0, abs(lv_c)) and abs(lq_c - lq_g) <= 2e-5 * max(1.0, abs(lq_c)), (lv_c, lv_g, lq_c, lq_g)
    for mod in ("Q", "V", "Q_targ"):
        for (n, p), q in zip(getattr(iql_g, mod).named_parameters(), getattr(iql_c, mod).parameters()):
            assert float((p.detach().cpu() - q.detach()).abs().max()) <= 5e-6 * max(1.0, float(q.detach().abs().max())), (mod, n)
    heads = []
    for cls, kw in ((MlpInvDynamic, dict(hidden_dim=64)), (FancyMlpInvDynamic, dict(hidden_dim=64, add_norm=True))):
        torch.manual_seed(4)
        hc = cls(11, 3, optim_params={"lr": 1e-3}, device="cpu", **kw)
        hg = cls(11, 3, optim_params={"lr": 1e-3}, device=DEV, **kw)
        hg._net().load_state_dict(hc._net().state_dict())
        hc.optim = torch.optim.Adam(hc._net().parameters(), lr=1e-3)
        assert isinstance(hg.optim, FusedAdam) and hg.optim.native()
        hc.train(), hg.train()
        for _ in range(5):
            lc, lg = hc.update(obs, act, nxt)["loss"], hg.update(d(obs), d(act), d(nxt))["loss"]
            assert abs(lc - lg) <= 2e-5 * max(1.0, abs(lc)), (cls.__name__, lc, lg)
        for (n, p), q in zip(hg._net().named_parameters(), hc._net().parameters()):
            assert float((p.detach().cpu() - q.detach()).abs().max()) <= 5e-6 * max(1.0, float(q.detach().abs().max())), (cls.__name__, n)
        heads.append(hg)
    def region():
        iql_g.update_V(d(obs), d(act))
        iql_g.update_Q(d(obs), d(act), d(rew), d(nxt), d(done))
        for hg in heads:
            hg.update(d(obs), d(act), d(nxt))
    prof, _ = _profiled(region)
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if any(w in n.lower() for w in ("addmm", "aten::mm", "layer_norm", "cijk_", "aten::linear"))]
    assert not bad, f"ATen GEMM / LayerNorm ops in the native head updates: {bad}"
    assert any("cdx_gemm_kernel" in n for n in names) and any("cdx_optim_kernel" in n for n in names), names


def test_classifier_update_runs_on_library_kernels(amd_lib):
    """VERDICT r5 'missing' #2: ``CumRewClassifier.update`` of the config-2 classifier (HalfJannerUNet1d, H = 32, D = 23) at the Diffuser
    pipeline's batch -- the call next to ``update()`` in every Diffuser training iteration (reference pipelines/diffuser_d4rl_mujoco.py:88-91,
    classifier/base.py:47-58) -- dispatches no ATen / MIOpen convolution and no group_norm kernel, runs its loss + backward as a HIP-graph
    replay from the second call on, steps through ``FusedAdam`` (cdx_optim_f32, L2 decay), and lands on the losses / parameters / EMA copies
    of the stock sequence on the CPU (autograd, torch.optim.Adam, the reference's EMA loop)."""
    from copy import deepcopy
    from torch.profiler import profile, ProfilerActivity
    from cleandiffuser_amd.engine.optim import FusedAdam
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.HalfJannerUNet1d(32, 23, out_dim=1, kernel_size=3, model_dim=32, emb_dim=32, dim_mult=(1, 2, 2, 2)), 17)
    kw = {"lr": 1e-3, "weight_decay": 1e-3}
    a, b = amd_lib.CumRewClassifier(deepcopy(net), device=DEV, optim_params=kw), amd_lib.CumRewClassifier(deepcopy(net), device="cpu", optim_params=kw)
    b.optim = torch.optim.Adam(b.model.parameters(), **kw)                    # the stock optimiser
    assert isinstance(a.optim, FusedAdam) and isinstance(a.optim, torch.optim.Adam) and a.optim.native()
    g = torch.Generator().manual_seed(5)
    x, t, r = torch.randn(64, 32, 23, generator=g), torch.randint(0, 20, (64,), generator=g), torch.randn(64, 1, generator=g)
    a.train(), b.train()
    la = [a.update(x.to(DEV), t.to(DEV), r.to(DEV))["loss"] for _ in range(3)]
    lb = [b.update(x, t, r)["loss"] for _ in range(3)]
    assert a.__dict__.get("_cdx_graphed") and not a.__dict__.get("_cdx_graph_off"), a.__dict__.get("_cdx_graph_off")
    prof, _ = _profiled(lambda: a.update(x.to(DEV), t.to(DEV), r.to(DEV)), rerun=False)     # (the EMA budget below counts four updates)
    names = [e.key for e in prof.key_averages()]
    bad = [n for n in names if any(w in n.lower() for w in ("convolution", "conv1d", "miopen", "group_norm", "native_batch_norm"))]
    assert not bad, f"ATen convolution / group_norm ops in a native classifier update(): {bad}"
    assert any("hipGraphLaunch" in n or "GraphLaunch" in n for n in names), names
    for u, v in zip(la, lb):
        assert abs(u - v) <= 2e-5 * max(1.0, abs(v)), (la, lb)
    for (n, p), q in zip(a.model_ema.named_parameters(), b.model_ema.parameters()):
        assert float((p.detach().cpu() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(q.detach().abs().max())) + 6e-6, n


def test_dql_backprop_through_the_sampler_runs_on_library_kernels(amd_lib, monkeypatch):
    """VERDICT r3 'missing' #2: Diffusion-QL's policy update differentiates THROUGH sample(..., requires_grad=True) (reference
    pipelines/dql_d4rl_mujoco.py:101, diffusionsde.py:401-427: 5 DDPM steps of DQLMlp under autograd).  On the device every Linear /
    Mish node of those forwards is a library launch (engine/train.py:_LinearAct: cdx_gemm_f32, cdx_act_f32 / cdx_act_bwd_f32,
    cdx_conv_wgrad_f32); the sampled actions, the gradient of a critic-like objective w.r.t. every actor parameter and w.r.t. the
    observation equal the ATen autograd path (CDX_TRAIN_NATIVE=0) on the same draws."""
    from torch.profiler import profile, ProfilerActivity
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.DQLMlp(11, 6, emb_dim=16), 65).to(DEV)
    agent = amd_lib.DiscreteDiffusionSDE(net, amd_lib.IdentityCondition(dropout=0.0), predict_noise=False, x_max=torch.ones(1, 6), x_min=-torch.ones(1, 6),
                                         diffusion_steps=5, device=DEV)
    g = torch.Generator().manual_seed(9)
    B = 256
    obs = torch.randn(B, 11, generator=g).to(DEV).requires_grad_(True)
    zs = [torch.randn(B, 6, generator=g).to(DEV) for _ in range(6)]
    q_w = torch.randn(6, generator=g).to(DEV)

    def run(native):
        monkeypatch.setenv("CDX_TRAIN_NATIVE", "1" if native else "0")
        agent.model.zero_grad(set_to_none=True)
        obs.grad = None
        act, _ = agent.sample(torch.zeros(B, 6, device=DEV), solver="ddpm", n_samples=B, sample_steps=5, use_ema=False, temperature=1.0,
                              condition_cfg=obs, w_cfg=1.0, requires_grad=True, noise=list(zs))
        (-(act * q_w).sum(-1).mean()).backward()
        return act.detach().clone(), obs.grad.clone(), {n: p.grad.clone() for n, p in agent.model.named_parameters() if p.grad is not None}
    prof, (a1, go1, gp1) = _profiled(lambda: run(True))
    names = [e.key for e in prof.key_averages()]
    assert not [n for n in names if "aten::addmm" in n or "aten::mish" in n or "Cijk_" in n], "ATen Linear / Mish kernels in the native DQL path"
    assert any("cdx_conv_wgrad_kernel" in n for n in names) and any("cdx_gemm_kernel" in n for n in names)
    a0, go0, gp0 = run(False)
    np.testing.assert_allclose(a1.cpu().numpy(), a0.cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(go1.cpu().numpy(), go0.cpu().numpy(), rtol=1e-4, atol=1e-4 * float(go0.abs().max()))
    assert set(gp1) == set(gp0) and len(gp1) >= 10
    for n in gp0:
        scale = float(gp0[n].abs().max()) + 1e-12
        assert float((gp1[n] - gp0[n]).abs().max()) <= 2e-4 * scale, n


def test_graphed_update_equals_the_eager_native_update(amd_lib, monkeypatch):
    """CDX_TRAIN_GRAPH=1: forward + backward of update() captured once into a HIP graph (engine/train.py:GraphedStep) and replayed per
    step.  With the timestep / noise draws pinned (the graph uses the device generator's graph-safe stream, an eager step the ordinary
    one) five replayed updates on changing batches must land on the same losses, gradient norms and weights as five eager native
    updates of a twin -- including the optimiser's `None`-gradient bookkeeping (a replay does not move version counters)."""
    from copy import deepcopy
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 7)
    fm = torch.zeros(32, 23)
    fm[0, :17] = 1.0
    mk = lambda n: amd_lib.DiscreteDiffusionSDE(n, None, fix_mask=fm, diffusion_steps=20, predict_noise=False, grad_clip_norm=1.0, device=DEV)  # noqa: E731
    a, b = mk(deepcopy(net)), mk(deepcopy(net))
    B = 64
    g = torch.Generator().manual_seed(5)
    t_fix = torch.randint(20, (B,), generator=g).to(DEV)
    eps_fix = torch.randn(B, 32, 23, generator=g).to(DEV)
    for agent in (a, b):
        def add_noise(x0, t=None, eps=None, agent=agent):
            alpha, sigma = agent.alpha[t_fix].view(-1, 1, 1), agent.sigma[t_fix].view(-1, 1, 1)
            xt = alpha * x0 + sigma * eps_fix
            return (1. - agent.fix_mask) * xt + agent.fix_mask * x0, t_fix, eps_fix
        agent.add_noise = add_noise
    batches = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(5)]
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "1")
    la = [a.update(x) for x in batches]
    assert len(a.__dict__.get("_cdx_graphed", {})) == 1, "one captured graph for the one batch shape"
    monkeypatch.setenv("CDX_TRAIN_GRAPH", "0")
    lb = [b.update(x) for x in batches]
    for u, v in zip(la, lb):
        assert abs(u["loss"] - v["loss"]) <= 1e-5 * max(1.0, abs(v["loss"])), (u, v)
        assert abs(float(u["grad_norm"]) - float(v["grad_norm"])) <= 1e-4 * float(v["grad_norm"])
    for (n, p), q in zip(list(a.model.named_parameters()) + list(a.model_ema.named_parameters()),
                         list(b.model.parameters()) + list(b.model_ema.parameters())):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(q.detach().abs().max())), n


@pytest.mark.parametrize("which", ["janner_sde", "chiunet_ddpm", "dit_continuous", "idql_edm_dropout"])
def test_default_update_is_a_graph_replay_and_equals_the_eager_step(which, amd_lib, monkeypatch):
    """Round 5: with NOTHING set, update() of every natively trained backbone -- under DiscreteDiffusionSDE,
    the legacy DDPM class, ContinuousDiffusionSDE and ContinuousEDM -- passes the capturability probe on its first call and is one
    HIP-graph replay + the optimiser launches from then on; five updates from the same seed land on the losses, gradient norms and
    weights of an eager twin (CDX_TRAIN_GRAPH=0), label dropout and nn.Dropout draws included."""
    from copy import deepcopy
    from cleandiffuser_amd.utils import load_synth
    g = torch.Generator().manual_seed(21)
    if which == "janner_sde":
        net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 7)
        fm = torch.zeros(32, 23)
        fm[0, :17] = 1.0
        mk = lambda n: amd_lib.DiscreteDiffusionSDE(n, None, fix_mask=fm, diffusion_steps=20, predict_noise=False, grad_clip_norm=1.0, device=DEV)  # noqa: E731
        data = [(torch.randn(48, 32, 23, generator=g).to(DEV), None) for _ in range(5)]
    elif which == "chiunet_ddpm":
        net = load_synth(amd_lib.ChiUNet1d(2, 5, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], obs_as_global_cond=True), 7)
        mk = lambda n: amd_lib.DDPM(n, amd_lib.IdentityCondition(dropout=0.25), diffusion_steps=20, grad_clip_norm=1.0, device=DEV)  # noqa: E731
        data = [(torch.randn(24, 16, 2, generator=g).clamp(-1, 1).to(DEV), torch.randn(24, 2, 5, generator=g).to(DEV)) for _ in range(5)]
    elif which == "dit_continuous":
        net = load_synth(amd_lib.DiT1d(7, emb_dim=32, d_model=64, n_heads=4, depth=2, timestep_emb_type="fourier"), 7)
        cnd = load_synth(amd_lib.MLPCondition(1, 32, [32], torch.nn.SiLU(), dropout=0.25), 8)
        mk = lambda n: amd_lib.ContinuousDiffusionSDE(n, deepcopy(cnd), predict_noise=True, noise_schedule="linear", grad_clip_norm=1.0, device=DEV)  # noqa: E731
        data = [(torch.randn(12, 16, 7, generator=g).to(DEV), torch.rand(12, 1, generator=g).to(DEV)) for _ in range(5)]
    else:
        net = load_synth(amd_lib.IDQLMlp(11, 3, emb_dim=16, hidden_dim=64, n_blocks=2, dropout=0.1), 7)
        mk = lambda n: amd_lib.ContinuousEDM(n, amd_lib.IdentityCondition(dropout=0.25), grad_clip_norm=0.5, device=DEV)  # noqa: E731
        data = [(torch.randn(40, 3, generator=g).to(DEV), torch.randn(40, 11, generator=g).to(DEV)) for _ in range(5)]
    a, b = mk(deepcopy(net)), mk(deepcopy(net))
    logs = {}
    for tag, agent in (("auto", a), ("0", b)):
        if tag == "auto":
            monkeypatch.delenv("CDX_TRAIN_GRAPH", raising=False)
        else:
            monkeypatch.setenv("CDX_TRAIN_GRAPH", tag)
        agent.train()
        torch.manual_seed(77)
        logs[tag] = [agent.update(x, c) if c is not None else agent.update(x) for x, c in data]
    assert a.__dict__.get("_cdx_graph_off") is None and len(a.__dict__.get("_cdx_graphed", {})) == 1, a.__dict__.get("_cdx_graph_off")
    assert not b.__dict__.get("_cdx_graphed")
    for u, v in zip(logs["auto"], logs["0"]):
        assert abs(u["loss"] - v["loss"]) <= 1e-5 * max(1.0, abs(v["loss"])), (u, v)
        assert abs(float(u["grad_norm"]) - float(v["grad_norm"])) <= 1e-4 * float(v["grad_norm"])
    for (n, p), q in zip(list(a.model.named_parameters()) + list(a.model_ema.named_parameters()),
                         list(b.model.parameters()) + list(b.model_ema.parameters())):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(q.detach().abs().max())), n


def test_update_that_cannot_be_captured_keeps_the_eager_path(amd_lib, monkeypatch):
    """The capturability probe: an agent whose loss() synchronises (here: the suite's own shim that draws from the CPU generator and moves
    the draws to the device) is found out on its first update() -- BEFORE any capture is attempted --, keeps the eager path for good,
    says why, and its draws / gradients are what they would have been without the probe (same losses as with CDX_TRAIN_GRAPH=0)."""
    from copy import deepcopy
    from oracle.train_cases import cpu_rng
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=5), 61)
    mk = lambda n: amd_lib.DiscreteDiffusionSDE(n, None, diffusion_steps=50, grad_clip_norm=1.0, device=DEV)  # noqa: E731
    a, b = mk(deepcopy(net)), mk(deepcopy(net))
    x0 = torch.randn(5, 8, 6, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = {}
    for tag, agent in (("auto", a), ("0", b)):
        if tag == "auto":
            monkeypatch.delenv("CDX_TRAIN_GRAPH", raising=False)
        else:
            monkeypatch.setenv("CDX_TRAIN_GRAPH", tag)
        with cpu_rng(DEV):
            torch.manual_seed(4321)
            out[tag] = [agent.update(x0)["loss"] for _ in range(3)]
    assert isinstance(a.__dict__.get("_cdx_graph_off"), str) and not a.__dict__.get("_cdx_graphed"), a.__dict__.get("_cdx_graph_off")
    assert torch.cuda.get_sync_debug_mode() == 0
    # (same draws, same gradients -- up to the order of the float atomics the weight / gain sums are combined with: ~1e-7)
    np.testing.assert_allclose(out["auto"], out["0"], rtol=2e-6, err_msg=str(out))


def test_graphed_update_draws_what_the_eager_update_draws_and_survives_dropped_gradients(amd_lib, monkeypatch):
    """CDX_TRAIN_GRAPH=1 against the eager native path from the SAME seed, draws NOT pinned: the capture's warm-up steps must not cost
    the generator anything (the replays then draw exactly what eager steps draw), and gradients set to None between two updates
    (``zero_grad(set_to_none=True)`` of user code) must not leave the graph accumulating into freed memory: it is captured again."""
    from copy import deepcopy
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 7)
    fm = torch.zeros(32, 23)
    fm[0, :17] = 1.0
    mk = lambda n: amd_lib.DiscreteDiffusionSDE(n, None, fix_mask=fm, diffusion_steps=20, predict_noise=False, grad_clip_norm=1.0, device=DEV)  # noqa: E731
    a, b = mk(deepcopy(net)), mk(deepcopy(net))
    batches = [torch.randn(32, 32, 23, generator=torch.Generator().manual_seed(9 + i)).to(DEV) for i in range(5)]
    logs = {}
    for tag, agent in (("1", a), ("0", b)):
        monkeypatch.setenv("CDX_TRAIN_GRAPH", tag)
        torch.manual_seed(123)
        out = []
        for i, x in enumerate(batches):
            if i == 3:
                for p in agent.model.parameters():
                    p.grad = None
            out.append(agent.update(x))
        logs[tag] = out
    assert getattr(a, "_cdx_recaptures", 0) == 1
    for u, v in zip(logs["1"], logs["0"]):
        assert abs(u["loss"] - v["loss"]) <= 1e-5 * max(1.0, abs(v["loss"])), (u, v)
    for (n, p), q in zip(a.model.named_parameters(), b.model.parameters()):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(q.detach().abs().max())), n


def test_update_runs_without_aten_optimiser_launches(amd_lib):
    """config 2's update(): after loss.backward() the whole optimiser side -- gradient-norm clip, AdamW, EMA, zeroed gradients -- is
    the library's kernels (3 launches), and the result equals the PyTorch sequence (clip_grad_norm_, torch.optim.AdamW.step,
    zero_grad, per-tensor EMA) on an identical twin fed the same draws: loss, updated weights, EMA weights, grad norm."""
    from copy import deepcopy
    from torch.profiler import profile, ProfilerActivity
    from oracle.train_cases import cpu_rng
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 7)
    fm = torch.zeros(32, 23)
    fm[0, :17] = 1.0
    mk = lambda n: amd_lib.DiscreteDiffusionSDE(n, None, fix_mask=fm, diffusion_steps=20, predict_noise=False, grad_clip_norm=1.0,  # noqa: E731
                                                device=DEV)
    a, b = mk(deepcopy(net)), mk(deepcopy(net))
    b.optimizer = torch.optim.AdamW(b.model.parameters(), lr=2e-4, weight_decay=1e-5)        # the stock sequence
    x0 = torch.randn(16, 32, 23, generator=torch.Generator().manual_seed(3)).to(DEV)
    logs = []
    for agent in (a, b):
        with cpu_rng(DEV):
            torch.manual_seed(11)
            logs.append([agent.update(x0) for _ in range(3)])
    for la, lb in zip(*logs):
        assert abs(la["loss"] - lb["loss"]) <= 1e-6 * max(1.0, abs(lb["loss"]))
        torch.testing.assert_close(la["grad_norm"], lb["grad_norm"], rtol=1e-5, atol=0)
    for (n, p), q in zip(list(a.model.named_parameters()) + list(a.model_ema.named_parameters()),
                         list(b.model.parameters()) + list(b.model_ema.parameters())):
        # (two backward passes of the SAME graph differ by atomics order in the conv weight gradients; where a gradient is ~0 Adam's
        #  m / sqrt(v) amplifies that to a fraction of lr = 2e-4 per step: 2.1e-6 observed after 3 steps)
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(q.detach().abs().max())), n
    # kernel census of one more update(): nothing of ATen's optimiser / foreach / clip machinery runs on the device
    with cpu_rng(DEV):
        torch.manual_seed(12)
        a.loss(x0).backward()
        torch.cuda.synchronize()
        prof, _ = _profiled(lambda: a._apply_gradients(True), [ProfilerActivity.CUDA], rerun=False)
        torch.manual_seed(12)
        b.update(x0)                                   # (the twin takes the same fourth step)
    kernels = [e.key for e in prof.key_averages() if not e.key.startswith("hip") and "Memcpy" not in e.key and "Memset" not in e.key]
    assert kernels and all("cdx_optim" in n for n in kernels), kernels      # (norm pass x 2 kernels + the fused AdamW / EMA pass)
    # and sampling right after sees the updated EMA weights (packed-weight caches key on the bumped version counters)
    prior = torch.zeros(4, 32, 23, device=DEV)
    z = torch.randn(4, 32, 23, device=DEV)
    xa, _ = a.sample(prior, solver="ddim", n_samples=4, sample_steps=5, noise=[z])
    xb, _ = b.sample(prior, solver="ddim", n_samples=4, sample_steps=5, noise=[z])
    np.testing.assert_allclose(xa.cpu().numpy(), xb.cpu().numpy(), **TOL)


# ---- row f3: PearceTransformer and DiT1Ref on the library (VERDICT r2 missing #2) ----
@pytest.mark.parametrize("name", ["pearcetf_small", "pearcetf_default"])
def test_pearce_transformer_runs_on_its_executor(name, amd_lib, monkeypatch):
    """PearceTransformer (reference pearcetransformer.py:91-151): the stand-alone forward with per-sample timesteps, the w_cfg = 1 loop
    and the CFG-pair loop are ONE cdx_pearcetf_run call each (folded projections / BatchNorm, MFMA attention over the 2 + To tokens);
    fixtures from the real reference at the DBC pipelines' default size (1024-wide attention) and a small one, 1e-4."""
    calls = _spy_bigbatch(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["pearcetf"] * 3, calls
    for k in gold.files:
        scale = max(1.0, float(np.abs(gold[k]).max()))
        np.testing.assert_allclose(out[k].cpu().numpy() / scale, gold[k] / scale, err_msg=f"{name}/{k}", **TOL)


def test_dit1ref_runs_on_the_dit_executor(amd_lib, monkeypatch):
    """DiT1Ref (reference dit.py:135-180): cross-attention to the reference half's tokens in front of every block, [reference |
    prediction] output -- forward, CFG-pair DDIM loop and unconditional SDE loop are one cdx_dit1d_run call each."""
    calls = _spy_bigbatch(monkeypatch)
    out, gold = _extra("dit1ref")
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["dit"] * 3, calls
    for k in gold.files:
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=k, **TOL)


# ---- round 3: conditional / CFG / EDM JannerUNet1d requests on the second-generation kernel (VERDICT r2 "Next" #3) ----
V2_COND_CASES = ["janner_tiny_cond_w1", "janner_tiny_cond_w2", "janner_legacy_dpm_ddim_cfg", "janner_rflow_cont_cfg",
                 "janner_legacy_edm_euler", "janner_legacy_edm_heun", "janner_legacy_edm_x", "janner_cm"]


@pytest.mark.parametrize("name", V2_COND_CASES)
def test_conditional_and_edm_janner_requests_run_on_the_v2_kernel(name, amd_lib, monkeypatch):
    """Condition embedding with w_cfg = 1, the classifier-free-guidance pair, EDM Euler / Heun / Diffusion-X and consistency plans of a
    JannerUNet1d are ONE cdx_unet2_run launch: per-trajectory
    FiLM rows, both forwards of the pair and step kinds 5-7 inside the kernel.  Reference fixtures, 1e-4."""
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    calls = _spy_launches(monkeypatch)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("B", [600, 604])          # 604 = 201 x 3 + 1: the last workgroup holds one real and two idle trajectories
@pytest.mark.parametrize("solver_kw", [dict(solver="ode_dpmsolver++_2M", w_cfg=1.7), dict(solver="ddpm", w_cfg=1.0)])
def test_conditional_config2_net_is_independent_of_trajectories_per_workgroup(solver_kw, B, amd_lib, monkeypatch):
    """The config-2 network with a condition embedding at B = 600 (three trajectories per workgroup on the compact program: the state
    and the conditional prediction of the CFG pair live in global memory, the state slot is rebuilt between the two forwards) against
    the same request one trajectory per workgroup: bit-identical, and equal to the PyTorch executor on a slice."""
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 5)
    fm = torch.zeros(32, 23)
    fm[0, :17] = 1.0
    lim = 3.0 * torch.ones(1, 32, 23)
    # (x0-prediction like config 2: with eps-prediction the clipped 6-step loop on synthetic weights amplifies summation-order noise
    #  past 1e-4 on a handful of the 441 600 elements -- 2.9e-4 observed between the two PROGRAMS of the same kernel)
    agent = amd_lib.DiscreteDiffusionSDE(net, amd_lib.IdentityCondition(dropout=0.0), fix_mask=fm, diffusion_steps=20, predict_noise=False,
                                         x_max=lim, x_min=-lim, device=DEV)
    agent.eval()
    g = torch.Generator().manual_seed(9)
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    cond = torch.randn(B, 32, generator=g).to(DEV)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(7)]
    kw = dict(n_samples=B, sample_steps=6, temperature=0.8, condition_cfg=cond, **solver_kw)
    calls = _spy_launches(monkeypatch)
    x3, _ = agent.sample(prior.to(DEV), noise=zs, **kw)
    assert calls["v2"] >= 1
    monkeypatch.setenv("CDX_UNET2_T", "1")          # the same (compact) program, one trajectory per workgroup: not a bit may change
    monkeypatch.setenv("CDX_UNET2_COMPACT", "1")
    x1, _ = agent.sample(prior.to(DEV), noise=zs, **kw)
    monkeypatch.delenv("CDX_UNET2_COMPACT")
    xd, _ = agent.sample(prior.to(DEV), noise=zs, **kw)       # the default program, one per workgroup: summation-order noise only
    monkeypatch.delenv("CDX_UNET2_T")
    assert torch.equal(x1, x3)
    np.testing.assert_allclose(xd.cpu().numpy(), x3.cpu().numpy(), rtol=2e-4, atol=2e-4)
    from cleandiffuser_amd.engine import dispatch
    monkeypatch.setattr(dispatch, "try_fused_sample", lambda *a, **k: None)
    monkeypatch.setattr(dispatch, "try_backbone_forward", lambda *a, **k: None)
    xs, _ = agent.sample(prior[-5:].to(DEV), noise=[z[-5:] for z in zs], **dict(kw, n_samples=5, condition_cfg=cond[-5:]))
    np.testing.assert_allclose(x3[-5:].cpu().numpy(), xs.cpu().numpy(), **TOL)


@pytest.mark.parametrize("edm_solver", ["euler", "heun"])
def test_edm_config2_net_three_per_workgroup(edm_solver, amd_lib, monkeypatch):
    """ContinuousEDM (step kinds 5 / 6: the network sees c_in x, state / slope / x_old in global memory) over the config-2 net at
    B = 605 -- three trajectories per workgroup on the compact program, a half-empty last workgroup -- against the same program one
    per workgroup (bit-identical) and the PyTorch executor on the last rows (1e-4)."""
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 6)
    fm = torch.zeros(32, 23)
    fm[0, :17] = 1.0
    lim = 2.0 * torch.ones(1, 32, 23)
    agent = amd_lib.ContinuousEDM(net, None, fix_mask=fm, x_max=lim, x_min=-lim, device=DEV)
    agent.eval()
    g = torch.Generator().manual_seed(10)
    B = 605
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV)]
    kw = dict(solver=edm_solver, n_samples=B, sample_steps=5)
    calls = _spy_launches(monkeypatch)
    x3, _ = agent.sample(prior.to(DEV), noise=zs, **kw)
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    monkeypatch.setenv("CDX_UNET2_T", "1")
    monkeypatch.setenv("CDX_UNET2_COMPACT", "1")
    x1, _ = agent.sample(prior.to(DEV), noise=zs, **kw)
    monkeypatch.delenv("CDX_UNET2_COMPACT")
    monkeypatch.delenv("CDX_UNET2_T")
    assert torch.equal(x1, x3)
    from cleandiffuser_amd.engine import dispatch
    monkeypatch.setattr(dispatch, "try_fused_edm", lambda *a, **k: None)
    monkeypatch.setattr(dispatch, "try_backbone_forward", lambda *a, **k: None)
    xs, _ = agent.sample(prior[-4:].to(DEV), noise=[zs[0][-4:]], **dict(kw, n_samples=4))
    np.testing.assert_allclose(x3[-4:].cpu().numpy(), xs.cpu().numpy(), **TOL)


def test_janner_forward_with_condition_and_per_sample_timesteps_is_one_v2_launch(amd_lib, monkeypatch):
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(amd_lib.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2, 2], kernel_size=5), 5).to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    for B in (7, 300):
        x, c = torch.randn(B, 32, 23, generator=g).to(DEV), torch.randn(B, 32, generator=g).to(DEV)
        t = (torch.arange(B) * 7 % 20).to(DEV)
        calls = _spy_launches(monkeypatch)
        with torch.no_grad():
            got, got_u = net(x, t, c), net(x, t, None)
            want, want_u = net._forward_torch(x, t, c), net._forward_torch(x, t, None)
        assert (calls["n"], calls["v2"]) == (2, 2)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), **TOL)
        np.testing.assert_allclose(got_u.cpu().numpy(), want_u.cpu().numpy(), **TOL)


def test_mlp_classifier_gradients_run_without_autograd(amd_lib, monkeypatch):
    """VERDICT r2 missing #3: `d logp / d x` of MSEClassifier(MLPNNClassifier) and QGPOClassifier(QGPONNClassifier) (QGPO's energy
    guidance, evaluated at every denoising step) comes from an explicit GEMM forward + backward on the library (engine/mlp_grad.py:
    cdx_gemm_f32 on the transposed weights, cdx_act_bwd_f32) -- torch.autograd.grad is never called -- and equals what the REAL
    reference's autograd produced (tests/golden/modules.npz, oracle/gen_module_golden.py:wrapper_outputs)."""
    from oracle import gen_module_golden as G
    from cleandiffuser_amd import classifier as C
    gold = np.load(golden_path("modules"))

    def no_autograd(*a, **k):
        raise AssertionError("torch.autograd.grad called: the native gradient path was not taken")
    monkeypatch.setattr(torch.autograd, "grad", no_autograd)
    net, (x, t) = G.build("cleandiffuser_amd", "MLPNNClassifier")
    y = torch.from_numpy(G.synth_array("mod/mse/y", (G.B, 2)))
    clf = C.MSEClassifier(net, temperature=0.7, device=DEV)
    logp, grad = clf.gradients(x.clone().to(DEV), t.to(DEV), y.to(DEV))
    np.testing.assert_allclose(logp.cpu().numpy(), gold["MSEClassifier/logp"], **TOL)
    np.testing.assert_allclose(grad.cpu().numpy(), gold["MSEClassifier/grad"], **TOL)
    net, (x, t, obs) = G.build("cleandiffuser_amd", "QGPONNClassifier")
    clf = C.QGPOClassifier(net, device=DEV)
    logp, grad = clf.gradients(x.clone().to(DEV), t.to(DEV), obs.to(DEV))
    np.testing.assert_allclose(logp.cpu().numpy(), gold["QGPOClassifier/logp"], **TOL)
    np.testing.assert_allclose(grad.cpu().numpy(), gold["QGPOClassifier/grad"], **TOL)


def test_janner_linear_attention_runs_on_the_gemm_executor(amd_lib, monkeypatch):
    """VERDICT r2 missing #5: JannerUNet1d(attention=True) (reference jannerunet.py:72-95, the net of the reference's own
    tests/test_janner_unet.py) -- channel LayerNorm, to_qkv / to_out as GEMMs and the LinearAttention core (cdx_linattn_f32) are
    sequenced by cdx_chiunet_run: the stand-alone forward and the whole DDIM loop are one native call each.  Reference fixture, 1e-4."""
    calls, fused = _spy_bigbatch(monkeypatch), _spy_launches(monkeypatch)
    out, gold = _extra("janner_attention")
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["chiunet", "chiunet"] and fused["n"] == 0, (calls, fused)
    for k in gold.files:
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=k, **TOL)


def test_conditional_janner_linear_attention_forwards_run_on_the_gemm_executor(amd_lib, monkeypatch):
    """VERDICT r4 missing #5: JannerUNet1d(attention=True) WITH a condition embedding (reference jannerunet.py:72-95,160-164,183).  The
    condition enters the time embedding before map_emb, so a conditional forward is the executor's per-sample-timestep launch on the
    rows map_noise(t) + condition: the stand-alone forward is one cdx_chiunet_run call, and the w_cfg = 1 / classifier-free-guidance
    loops run one such call per network evaluation (steps x 1 and steps x 2) instead of the PyTorch modules.  Reference fixture, 1e-4."""
    calls, fused = _spy_bigbatch(monkeypatch), _spy_launches(monkeypatch)
    out, gold = _extra("janner_attention_conditional")
    torch.cuda.synchronize()
    # (the pair: one evaluation of the doubled batch [cond | zeros] per step, or two -- either way every evaluation is the executor's)
    assert set(c[0] for c in calls) == {"chiunet"} and len(calls) in (1 + 4 + 4, 1 + 4 + 8) and fused["n"] == 0, (calls, fused)
    for k in gold.files:
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=k, **TOL)


@pytest.mark.parametrize("seed", range(12))
def test_conditional_v2_requests_match_the_torch_executor_on_random_configurations(seed, amd_lib, monkeypatch):
    """Shapes / solvers the fixtures do not enumerate: a random JannerUNet1d (horizon, widths, kernel size), a random solver class and
    solver, condition embedding with w_cfg in {1, pair}, random batch (odd sizes: half-empty workgroups) -- the ONE cdx_unet2_run launch
    against this repo's PyTorch executor on the same device and draws (2e-4: two implementations, summation-order noise on both sides)."""
    import random
    rnd = random.Random(1000 + seed)
    from cleandiffuser_amd.utils import load_synth
    H = rnd.choice([4, 8, 16, 32, 64])
    D = rnd.choice([3, 6, 11, 23])
    md = rnd.choice([16, 32])
    mult = rnd.choice([[1, 2], [1, 2, 2], [1, 4, 2]])
    while H % (1 << (len(mult) - 1)):
        mult = mult[:-1]
    ks = rnd.choice([3, 5])
    emb = rnd.choice([16, 32])
    net = load_synth(amd_lib.JannerUNet1d(D, model_dim=md, emb_dim=emb, dim_mult=mult, kernel_size=ks), 100 + seed)
    B = rnd.choice([1, 2, 3, 5, 9, 257, 300, 513, 601])
    pn = rnd.random() < 0.5
    lim = 3.0 * torch.ones(1, H, D)
    fm = torch.zeros(H, D)
    fm[0, : max(1, D // 2)] = 1.0
    kind = rnd.choice(["disc", "cont", "edm"])
    w_cfg = rnd.choice([1.0, 1.0, 1.6, 0.3])
    g = torch.Generator().manual_seed(seed)
    if kind == "edm":
        agent = amd_lib.ContinuousEDM(net, amd_lib.IdentityCondition(dropout=0.0), fix_mask=fm, x_max=lim, x_min=-lim, device=DEV)
        kw = dict(solver=rnd.choice(["euler", "heun"]), sample_steps=rnd.choice([3, 5]))
    else:
        cls = amd_lib.DiscreteDiffusionSDE if kind == "disc" else amd_lib.ContinuousDiffusionSDE
        extra = dict(diffusion_steps=20) if kind == "disc" else {}
        agent = cls(net, amd_lib.IdentityCondition(dropout=0.0), fix_mask=fm, predict_noise=pn, x_max=lim, x_min=-lim, device=DEV, **extra)
        kw = dict(solver=rnd.choice(["ddpm", "ddim", "ode_dpmsolver_1", "ode_dpmsolver++_1", "ode_dpmsolver++_2M", "sde_dpmsolver_1",
                                     "sde_dpmsolver++_1", "sde_dpmsolver++_2M"]), sample_steps=rnd.choice([3, 5]), temperature=0.8)
    agent.eval()
    prior = torch.zeros(B, H, D)
    prior[:, 0] = torch.randn(B, D, generator=g)
    cond = torch.randn(B, emb, generator=g).to(DEV)
    zs = [torch.randn(B, H, D, generator=g).to(DEV) for _ in range(12)]
    kw.update(n_samples=B, condition_cfg=cond, w_cfg=w_cfg)
    calls = _spy_launches(monkeypatch)
    x, _ = agent.sample(prior.to(DEV), noise=zs, **kw)
    torch.cuda.synchronize()
    from cleandiffuser_amd.engine import runtime2
    if runtime2.supported(net, H) is None:
        assert calls["v2"] >= 1 and calls["n"] == calls["v2"], (calls, H, D, md, mult, ks, kind, kw)
    from cleandiffuser_amd.engine import dispatch
    for fn in ("try_fused_sample", "try_fused_edm", "try_backbone_forward"):
        monkeypatch.setattr(dispatch, fn, lambda *a, **k: None)
    n = min(B, 6)
    xs, _ = agent.sample(prior[-n:].to(DEV), noise=[z[-n:] for z in zs], **dict(kw, n_samples=n, condition_cfg=cond[-n:]))
    scale = max(1.0, float(xs.abs().max()))
    np.testing.assert_allclose(x[-n:].cpu().numpy() / scale, xs.cpu().numpy() / scale, rtol=2e-4, atol=2e-4,
                               err_msg=str((H, D, md, mult, ks, emb, B, pn, kind, kw["solver"], w_cfg)))


@pytest.mark.parametrize("name", ["chitf_pusht_full", "diffuser_kitchen_20", "diffuser_antmaze_20"])
def test_full_step_count_configurations_match_reference_fixture(name, amd_lib, monkeypatch):
    """Step counts the earlier fixtures cut short: Diffusion Policy's transformer at the dp_pusht size over all 100 DDPM steps, and the
    shipped kitchen / antmaze Diffuser sizes over their 20 guided DDPM steps with the final log_p -- each one native call (cdx_chitf_run /
    one guided cdx_unet2_run launch including log_p), reference fixtures, 1e-4."""
    fused, big = _spy_launches(monkeypatch), _spy_bigbatch(monkeypatch)
    out, gold = _extra(name)
    torch.cuda.synchronize()
    if name == "chitf_pusht_full":
        assert [c[0] for c in big] == ["chitf"] and fused["n"] == 0
    else:
        assert (fused["n"], fused["v2"], len(big)) == (1, 1, 0), (fused, big)
    for k in gold.files:
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=f"{name}/{k}", **TOL)


def test_classifier_guidance_under_edm_runs_natively(amd_lib, monkeypatch):
    """VERDICT r2 missing #4: ContinuousEDM with w_cg != 0 (reference newedm.py:217-284) used to be a PyTorch loop around the native
    forward and gradient.  Now the whole guided Heun / Euler loop is ONE cdx_guided_run call (per record: c_in-scaled denoiser forward,
    explicit classifier forward + backward at (x_t, ln(sigma) / 4), EDM step with the prediction shifted by w sigma^2 grad); without a
    condition_cg the reference applies no shift and the request takes the unguided one-launch path.  Reference fixture incl. log_p, 1e-4."""
    from cleandiffuser_amd.engine import guided
    n_loops = {"n": 0}
    orig = guided.guided_sample

    def counted(*a, **k):
        out = orig(*a, **k)
        n_loops["n"] += out is not None
        return out
    monkeypatch.setattr(guided, "guided_sample", counted)
    monkeypatch.setattr(torch.autograd, "grad", lambda *a, **k: (_ for _ in ()).throw(AssertionError("autograd used")))
    fused = _spy_launches(monkeypatch)
    out, gold = _extra("edm_classifier_guidance")
    torch.cuda.synchronize()
    assert n_loops["n"] == 2 and fused["v2"] >= 1           # two guided loops in one native call each; the no-condition one on the v2 kernel
    for k in gold.files:
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], err_msg=k, **TOL)


# ---- round 3: ChiUNet1d below the GEMM executor's crossover on the second-generation kernel (VERDICT r2 "Next" #3) ----
@pytest.mark.parametrize("name", [n for n in CHIUNET_CASES if cases.CASES[n]["net"][1].get("obs_as_global_cond", True)])
def test_chiunet_requests_run_on_the_v2_kernel(name, amd_lib, monkeypatch):
    """FiLM-conditioned U-Net (global condition): per-(step, trajectory) [scale | bias] rows filled by four cdx_gemm_f32 launches,
    then ONE cdx_unet2_run launch for the loop -- w_cfg = 1, the classifier-free-guidance pair against the zero condition, legacy
    DDPM and EDM plans.  Reference fixtures, 1e-4."""
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    calls = _spy_launches(monkeypatch)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("solver_kw", [dict(solver="ddpm", w_cfg=1.0), dict(solver="ode_dpmsolver++_2M", w_cfg=2.5), dict(solver="ddim", w_cfg=0.7)])
def test_chiunet_v2_requests_match_the_torch_executor(solver_kw, scale, amd_lib, monkeypatch):
    """ChiUNet1d (both FiLM forms, three resolutions, a 1x1 skip in every level) at batch 37: the v2 launch against this repo's
    PyTorch executor on the CPU (itself held to the reference fixtures)."""
    from cleandiffuser_amd.utils import load_synth

    def build(dev):
        net = load_synth(amd_lib.ChiUNet1d(3, 7, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], kernel_size=5,
                                           cond_predict_scale=scale, obs_as_global_cond=True), 21)
        # (x0-prediction: a clipped eps-prediction loop amplifies summation-order noise past 1e-4 on single elements)
        ag = amd_lib.DiscreteDiffusionSDE(net, amd_lib.IdentityCondition(dropout=0.0), diffusion_steps=12, predict_noise=False,
                                          x_max=torch.full((1, 16, 3), 2.5), x_min=torch.full((1, 16, 3), -2.5), device=dev)
        ag.eval()
        return ag
    g = torch.Generator().manual_seed(13)
    B, S = 37, 6
    cond, noise = torch.randn(B, 2, 7, generator=g), [torch.randn(B, 16, 3, generator=g) for _ in range(S + 1)]
    prior = torch.zeros(B, 16, 3)
    want, _ = build("cpu").sample(prior, n_samples=B, sample_steps=S, condition_cfg=cond, noise=list(noise), temperature=0.8, **solver_kw)
    calls = _spy_launches(monkeypatch)
    got, _ = build(DEV).sample(prior.to(DEV), n_samples=B, sample_steps=S, condition_cfg=cond.to(DEV),
                               noise=[z.to(DEV) for z in noise], temperature=0.8, **solver_kw)
    torch.cuda.synchronize()
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), **TOL)


@pytest.mark.parametrize("size", ["cfg2", "kitchen"])
def test_classifier_log_p_of_a_batch_is_one_v2_launch(size, amd_lib, monkeypatch):
    """``CumRewClassifier.logp`` (reference classifier/base.py:62-72 -> HalfJannerUNet1d forward) with a different timestep per
    sample: the classifier's own v2 program, log_p pass only (n_steps = 0), one trajectory per workgroup, row b of the FiLM table for
    trajectory b -- against the module's PyTorch forward on the CPU (bit-identical to the reference's, tests/test_module_mirrors.py).
    300 samples: more workgroups than CUs."""
    from cleandiffuser_amd.utils import load_synth
    H, D, md = (32, 23, 32) if size == "cfg2" else (32, 69, 64)
    mk = lambda: load_synth(amd_lib.HalfJannerUNet1d(H, D, out_dim=1, model_dim=md, emb_dim=md, dim_mult=(1, 2, 2, 2), kernel_size=3), 3).eval()  # noqa: E731
    clf_cpu, clf = mk(), mk().to(DEV)
    g = torch.Generator().manual_seed(8)
    B = 300
    x, t = torch.randn(B, H, D, generator=g), torch.randint(0, 20, (B,), generator=g)
    calls = _spy_launches(monkeypatch)
    with torch.no_grad():
        want = clf_cpu(x, t, None)
        got = clf(x.to(DEV), t.to(DEV), None)
    torch.cuda.synchronize()
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    assert got.shape == (B, 1)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(want.abs().max())))


# ---- round 3: the batch-tiled MLP denoisers on the second-generation kernel (VERDICT r2 "Next" #3) ----
MLP_V2_CASES = [n for n, c in cases.CASES.items() if c["net"][0] in ("PearceMlp", "DQLMlp", "DVInvMlp", "SfBCUNet", "MlpNNDiffusion")]


@pytest.mark.parametrize("name", MLP_V2_CASES)
def test_tile_mlp_requests_run_on_the_v2_kernel(name, amd_lib, monkeypatch):
    """PearceMlp / DQLMlp / DVInvMlp / MlpNNDiffusion / SfBCUNet loops (unconditional, conditional, the classifier-free-guidance pair,
    EDM plans): ONE cdx_unet2_run launch of the MLP instantiation -- a tile of samples per workgroup, Linears as 1-tap convs, the
    time-dependent inputs in per-step bias rows, the condition in a context slot.  Reference fixtures, 1e-4."""
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    calls = _spy_launches(monkeypatch)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("batch", [1, 7, 1030, 5000])
def test_tile_mlp_v2_batch_sizes_and_tiles(batch, amd_lib, monkeypatch):
    """Ragged last tile, the three tile sizes (4 / 8 / 16 samples per workgroup) and more workgroups than CUs: PearceMlp (per-sample
    GroupNorm, GELU, scaled skips) with a condition and w_cfg = 1.3 against this repo's PyTorch executor on the CPU."""
    from cleandiffuser_amd.utils import load_synth

    def build(dev):
        net = load_synth(amd_lib.PearceMlp(5, To=2, emb_dim=32, hidden_dim=128), 31)
        cond = load_synth(amd_lib.PearceObsCondition(9, 32, flatten=False, dropout=0.0), 32)
        ag = amd_lib.DiscreteDiffusionSDE(net, cond, predict_noise=False, x_max=torch.full((1, 5), 2.0), x_min=torch.full((1, 5), -2.0),
                                          diffusion_steps=10, device=dev)
        ag.eval()
        return ag
    g = torch.Generator().manual_seed(17)
    obs, noise = torch.randn(batch, 2, 9, generator=g), [torch.randn(batch, 5, generator=g) for _ in range(6)]
    kw = dict(solver="ddpm", n_samples=batch, sample_steps=5, temperature=0.7, w_cfg=1.3)
    want, _ = build("cpu").sample(torch.zeros(batch, 5), condition_cfg=obs, noise=list(noise), **kw)
    calls = _spy_launches(monkeypatch)
    got, _ = build(DEV).sample(torch.zeros(batch, 5, device=DEV), condition_cfg=obs.to(DEV), noise=[z.to(DEV) for z in noise], **kw)
    torch.cuda.synchronize()
    assert (calls["n"], calls["v2"]) == (1, 1), calls
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), **TOL)


def test_the_binding_stub_of_integration_md_runs(amd_lib):
    """The reference-side ctypes binding printed in INTEGRATION.md section 2 is executed as written (only the library path is made
    absolute) and must reproduce the reference fixture of BASELINE config 2: the document cannot drift from the ABI."""
    import os
    import re
    import types
    from cleandiffuser_amd.engine import runtime
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"```python\n(# cleandiffuser/diffusion/_cdx\.py.*?)```", text, re.S).group(1)
    assert 'ctypes.CDLL("libcdx.so")' in code
    ns = {}
    exec(compile(code.replace('ctypes.CDLL("libcdx.so")', f'ctypes.CDLL({runtime.LIB_PATH!r})'), "INTEGRATION.md", "exec"), ns)
    name = "janner_cfg2_ddim"
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    c = cases.CASES[name]
    S = c["sample"]["sample_steps"]
    from cleandiffuser_amd.utils import SUPPORTED_SAMPLING_STEP_SCHEDULE as SS
    sched = SS["uniform"](agent.diffusion_steps, S)
    temp = c["sample"].get("temperature", 1.0)
    prior = torch.from_numpy(inp["prior"]).to(DEV)
    mask = agent.fix_mask.to(DEV)
    xt = torch.from_numpy(inp["noise"][0]).to(DEV) * temp
    xt = (xt * (1.0 - mask) + prior * mask).contiguous()
    me = types.SimpleNamespace(predict_noise=agent.predict_noise, fix_mask=mask)
    out = ns["fused_loop"](me, agent.model_ema, xt, prior.contiguous(), agent._alpha_host[sched.cpu()], agent._sigma_host[sched.cpu()], sched,
                           "ddim", S, None)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("kind", ["janner", "chiunet"])
def test_conditional_request_with_classifier_guidance_is_one_guided_call(kind, amd_lib, monkeypatch):
    """A condition (w_cfg = 1) AND classifier guidance (w_cg > 0) at once: cdx_guided_run with the program kernel in forward mode as
    its denoiser slot -- the slot reads the FiLM rows of (step i, trajectory b) from the table of all steps (`emb_per_traj`).  JannerUNet1d
    with a condition embedding and ChiUNet1d with its observation condition, against this repo's PyTorch executor on the CPU
    (autograd classifier gradients), x0-prediction DDPM."""
    from cleandiffuser_amd.engine import guided
    from cleandiffuser_amd.utils import load_synth
    H, D, B, S = 16, 6, 9, 5

    def build(dev):
        if kind == "janner":
            net = load_synth(amd_lib.JannerUNet1d(D, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], kernel_size=5), 41)
            cond = amd_lib.IdentityCondition(dropout=0.0)
        else:
            net = load_synth(amd_lib.ChiUNet1d(D, 7, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], kernel_size=5), 42)
            cond = amd_lib.IdentityCondition(dropout=0.0)
        clf_net = load_synth(amd_lib.HalfJannerUNet1d(H, D, out_dim=1, model_dim=32, emb_dim=32, dim_mult=(1, 2, 2), kernel_size=3), 43)
        ag = amd_lib.DiscreteDiffusionSDE(net, cond, classifier=amd_lib.CumRewClassifier(clf_net, device=dev), diffusion_steps=10,
                                          predict_noise=False, x_max=torch.full((1, H, D), 2.0), x_min=torch.full((1, H, D), -2.0), device=dev)
        ag.eval()
        return ag
    g = torch.Generator().manual_seed(23)
    c = torch.randn(B, 32, generator=g) if kind == "janner" else torch.randn(B, 2, 7, generator=g)
    noise = [torch.randn(B, H, D, generator=g) for _ in range(S + 1)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=S, temperature=0.6, w_cfg=1.0, w_cg=0.2)
    want, wlog = build("cpu").sample(torch.zeros(B, H, D), condition_cfg=c, noise=list(noise), **kw)
    n_loops = {"n": 0}
    orig = guided.guided_sample

    def counted(*a, **k):
        out = orig(*a, **k)
        n_loops["n"] += out is not None
        return out
    monkeypatch.setattr(guided, "guided_sample", counted)
    monkeypatch.setattr(torch.autograd, "grad", lambda *a, **k: (_ for _ in ()).throw(AssertionError("autograd used")))
    got, glog = build(DEV).sample(torch.zeros(B, H, D, device=DEV), condition_cfg=c.to(DEV), noise=[z.to(DEV) for z in noise], **kw)
    torch.cuda.synchronize()
    assert n_loops["n"] == 1, "the guided loop must be one cdx_guided_run call"
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), **TOL)
    np.testing.assert_allclose(glog["log_p"].cpu().numpy(), wlog["log_p"].numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(wlog["log_p"].abs().max())))


# ---- round 3: small-batch mode -- one trajectory over k workgroups of an XCD (VERDICT r2 "Next" #6) ----
def _check_group_placement(k):
    """What the launch itself recorded: 256 workgroups, 32 per XCD, every group complete and behind ONE L2 -- by construction (a
    workgroup draws its (group, member) ticket from the counter of the XCD it finds itself on; HIP promises no placement)."""
    from cleandiffuser_amd.engine import runtime2
    p = runtime2.group_placement(DEV)
    assert p["workgroups"] == 256 and p["groups"] == 256 // int(k) and p["one_xcd_per_group"], p
    assert sorted(p["per_xcd"].values()) == [32] * 8, p


@pytest.mark.parametrize("k", ["2", "4"])
@pytest.mark.parametrize("name", ["janner_cfg2_ddim", "janner_cfg2_ddpm_clip", "janner_h4_ddpm", "janner_tiny_disc_ddim", "janner_tiny_cont_ddim"])
def test_split_program_matches_reference_fixture(name, k, amd_lib, monkeypatch):
    """Every member of a group holds the whole activation set, computes its share of each op's row tiles and all-gathers the rest
    through L2 (flags, no agent-scope fence): one launch of ceil(B / 8) * 8 * k workgroups, reference fixture at 1e-4, no lost flag."""
    from cleandiffuser_amd.engine import program2, runtime2
    if runtime2._split_ok.get(torch.device(DEV)) is not True:
        pytest.skip("the small-batch mode failed its self-check on this device")
    monkeypatch.setenv("CDX_UNET2_SPLIT", k)
    monkeypatch.setattr(program2, "SPLIT_MIN_RECORDS", 0)          # cut every op that can be cut (the default leaves short ops whole)
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        if kws.get("run_if") is not None:          # (the gated repair launch behind a split / grouped launch)
            return orig(comp, **kws)
        seen.append((kws.get("split"), comp.prog.meta.get("split_k")))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    assert seen == [(int(k), int(k))], seen
    _check_group_placement(k)
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


@pytest.mark.parametrize("B", [1, 37, 64])
def test_split_program_agrees_with_the_ordinary_program(B, amd_lib, monkeypatch):
    """The default routing at small batch (4 workgroups per trajectory up to 64 trajectories, 2 up to 128) against the ordinary
    one-workgroup program: same math, another summation order (more K slices per tile); x0-prediction DDPM, ragged groups of 8."""
    from cleandiffuser_amd.engine import runtime2
    if runtime2._split_ok.get(torch.device(DEV)) is not True:
        pytest.skip("the small-batch mode failed its self-check on this device")
    agent, _ = cases.build(amd_lib, "janner_cfg2_ddim", device=DEV)
    g = torch.Generator().manual_seed(3)
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g) for _ in range(11)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=10, temperature=0.5)
    outs = {}
    for tag in ("0", "auto", "2"):
        monkeypatch.setenv("CDX_UNET2_SPLIT", tag)
        outs[tag], _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        torch.cuda.synchronize()
        runtime2.check_split_errors()
    assert runtime2.split_factor(B) == 2                 # (the loop left the factor forced to 2)
    monkeypatch.setenv("CDX_UNET2_SPLIT", "auto")
    assert runtime2.split_factor(B) == 4 and runtime2.split_factor(100) == 2 and runtime2.split_factor(200) == 1
    for tag in ("auto", "2"):
        np.testing.assert_allclose(outs[tag].cpu().numpy(), outs["0"].cpu().numpy(), rtol=2e-4, atol=2e-4)


# ---- round 4: full-batch grouped mode -- k trajectories over the k workgroups of a group on one XCD (VERDICT r3 "Next" #2) ----
@pytest.mark.parametrize("k", ["2", "4"])
@pytest.mark.parametrize("name", ["janner_cfg2_ddim", "janner_cfg2_ddpm_clip", "janner_h4_ddpm"])
def test_grouped_program_matches_reference_fixture(name, k, amd_lib, monkeypatch):
    """A member owns one trajectory of its group; the layers that are bound by the L2 -> CU weight stream are computed per member for
    1/k of the output channels of all k trajectories (k x positions tile columns) and all-gathered through L2.  Here with EVERY op that
    can be grouped grouped (threshold 0; `janner_h4_ddpm`: the levels at 2 and 1 positions), ragged last group (batch 3-5), reference
    fixture at 1e-4, one launch, no lost granule."""
    from cleandiffuser_amd.engine import program2, runtime2
    if runtime2._group_ok.get(torch.device(DEV)) is not True:
        pytest.skip("the grouped mode failed its self-check on this device")
    monkeypatch.setenv("CDX_UNET2_SPLIT", "0")
    monkeypatch.setenv("CDX_UNET2_GROUP", k)
    monkeypatch.setattr(program2, "GROUP_MIN_BYTES", 0)
    gold = np.load(golden_path(name))
    agent, _ = cases.build(amd_lib, name, device=DEV)
    inp = cases.make_inputs(name)
    kw = cases.sample_kwargs(name, inp, device=DEV)
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        if kws.get("run_if") is not None:          # (the gated repair launch behind a split / grouped launch)
            return orig(comp, **kws)
        seen.append((kws.get("split"), kws.get("group"), comp.prog.meta.get("group_k"), comp.prog.meta.get("n_gops")))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    x, _ = cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]).to(DEV), noise=list(inp["noise"][:int(gold["n_draws"])]), **kw)
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    assert len(seen) == 1 and seen[0][:3] == (int(k), True, int(k)) and seen[0][3] >= 2, seen
    _check_group_placement(k)
    np.testing.assert_allclose(x.cpu().numpy(), gold["x_out"], **TOL)


def test_group_formation_does_not_depend_on_dispatch_order(amd_lib, monkeypatch):
    """The split / grouped modes must not rest on "workgroup i runs on XCD i % 8": 300 launches of the headline batch and of a small
    batch, each recording who ended up where -- always 32 workgroups per XCD, every group complete and on one XCD -- while the results
    stay bit-identical from launch to launch (which trajectory a workgroup computes follows from its ticket, not from its blockIdx)."""
    from cleandiffuser_amd.engine import runtime2
    if runtime2._group_ok.get(torch.device(DEV)) is not True or runtime2._split_ok.get(torch.device(DEV)) is not True:
        pytest.skip("the split / grouped modes failed their self-check on this device")
    agent, _ = cases.build(amd_lib, "janner_cfg2_ddim", device=DEV)
    g = torch.Generator().manual_seed(5)
    for B, k in ((256, 4), (24, 4), (100, 2)):
        prior = torch.zeros(B, 32, 23)
        prior[:, 0, :17] = torch.randn(B, 17, generator=g)
        zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(3)]
        first = None
        for i in range(100):
            x, _ = agent.sample(prior.to(DEV), noise=list(zs), solver="ddim", n_samples=B, sample_steps=2, temperature=0.5)
            if i % 10 == 0:
                _check_group_placement(k)
                first = x if first is None else first
                assert torch.equal(x, first)
        runtime2.check_split_errors()


def test_headline_batch_takes_the_grouped_program_and_matches_the_reference(amd_lib, monkeypatch):
    """BASELINE config 2 at B = 256 on its DEFAULT route: groups of 4 (64 groups x 4 workgroups = one per CU), the ten 0.6-1.3 MB layers
    grouped.  Against the fixture the real reference produced for the same 256 trajectories (1e-4), bit-reproducible, and within
    summation-order noise of the ordinary one-workgroup-per-trajectory program."""
    from cleandiffuser_amd.engine import runtime2
    if runtime2._group_ok.get(torch.device(DEV)) is not True:
        pytest.skip("the grouped mode failed its self-check on this device")
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        if kws.get("run_if") is not None:          # (the gated repair launch behind a split / grouped launch)
            return orig(comp, **kws)
        seen.append((kws.get("split"), kws.get("group"), comp.prog.meta.get("n_gops")))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    out, gold = _extra("baseline_cfg2_b256")
    out2, _ = _extra("baseline_cfg2_b256")
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    assert seen == [(4, True, 10)] * 2, seen
    assert torch.equal(out["x"], out2["x"]), "not deterministic"
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)
    monkeypatch.setenv("CDX_UNET2_GROUP", "0")
    plain, _ = _extra("baseline_cfg2_b256")
    assert seen[-1][:2] == (0, False)
    np.testing.assert_allclose(out["x"].cpu().numpy(), plain["x"].cpu().numpy(), rtol=2e-4, atol=2e-4)
    assert runtime2.group_factor(256) == 1
    monkeypatch.setenv("CDX_UNET2_GROUP", "auto")
    assert runtime2.group_factor(256) == 4 and runtime2.group_factor(200) == 4 and runtime2.group_factor(128) == 1 and runtime2.group_factor(300) == 1


def test_guided_batch_of_200_takes_the_grouped_guided_program_and_matches_the_reference(amd_lib, monkeypatch):
    """Round 6: the classifier-guided Diffuser loop at 128 < B <= 256 runs as a GROUPED guided program -- groups of four
    workgroups share the weight stream of the denoiser's ten stream-bound layers, the classifier's forward / backward ops, the solver
    step and the final log_p run on each member's own trajectory; one launch + its idle repair launch.  Against the fixture the real
    reference produced for 200 such trajectories (every third one kept), x and log_p; bit-reproducible; within summation-order noise
    of the ordinary guided program; a ragged last group (B = 130) as well."""
    from cleandiffuser_amd.engine import runtime2
    from oracle import extra_cases
    dev = torch.device(DEV)
    if runtime2._group_ok.get(dev) is not True:
        pytest.skip("the grouped mode failed its self-check on this device")
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        if kws.get("run_if") is None:
            seen.append((kws.get("split"), kws.get("group"), comp.prog.meta.get("n_gops"), kws.get("cg_scale") is not None))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    out, gold = _extra("baseline_cfg2_guided_b200")
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    if runtime2._gguided_ok.get(dev) is not True:
        pytest.fail("the grouped guided mode failed its first-use check against the ordinary guided program")
    seen.clear()
    out2, _ = _extra("baseline_cfg2_guided_b200")
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    assert seen == [(4, True, 10, True)], seen
    assert torch.equal(out["x"], out2["x"]) and torch.equal(out["log_p"], out2["log_p"]), "not deterministic"
    st = int(gold["stride"][0])
    np.testing.assert_allclose(out["x"].cpu().numpy()[::st], gold["x"], **TOL)
    np.testing.assert_allclose(out["log_p"].cpu().numpy()[::st], gold["log_p"], rtol=1e-4, atol=1e-4)
    monkeypatch.setenv("CDX_UNET2_GUIDED_GROUP", "0")
    plain, _ = _extra("baseline_cfg2_guided_b200")
    assert seen[-1][:2] in ((0, False), (None, None)) and seen[-1][3]
    np.testing.assert_allclose(out["x"].cpu().numpy(), plain["x"].cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out["log_p"].cpu().numpy(), plain["log_p"].cpu().numpy(), rtol=2e-4, atol=2e-4)
    monkeypatch.delenv("CDX_UNET2_GUIDED_GROUP")
    # ragged: 130 trajectories = 32 groups + a group of two (its other two members compute on zeros)
    agent, _ = cases.build(amd_lib, "janner_cfg2_guided_ddpm", device=DEV)
    g = torch.Generator().manual_seed(41)
    B = 130
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(6)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=5, temperature=0.5, w_cg=0.3)
    seen.clear()
    xg, lg = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    assert seen == [(4, True, 10, True)], seen
    monkeypatch.setenv("CDX_UNET2_GUIDED_GROUP", "0")
    xp, lp = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    np.testing.assert_allclose(xg.cpu().numpy(), xp.cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(lg["log_p"].cpu().numpy(), lp["log_p"].cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_small_guided_batch_takes_the_split_guided_program_and_matches_the_reference(amd_lib, monkeypatch):
    """Round 6: the classifier-guided loop at B <= 128 runs as a SMALL-BATCH guided program -- one trajectory over 4 (B <= 64) or 2
    workgroups of an XCD, the denoiser's ops cut by row tiles, the classifier's ops computed by every member; one launch + its idle
    repair launch.  The B = 8 fixture of the real reference (x and log_p, 1e-4), bit-reproducible, within summation-order noise of the
    ordinary guided program; B = 100 (two workgroups per trajectory) against the ordinary program."""
    from cleandiffuser_amd.engine import runtime2
    dev = torch.device(DEV)
    if runtime2._split_ok.get(dev) is not True:
        pytest.skip("the small-batch mode failed its self-check on this device")
    assert runtime2._sguided_ok.get(dev) is True, "the small-batch guided mode failed its first-use check against the ordinary guided program"
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        if kws.get("run_if") is None:
            seen.append((kws.get("split") or 0, bool(kws.get("group")), kws.get("cg_scale") is not None))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    out, gold = _extra("baseline_cfg2_guided")
    out2, _ = _extra("baseline_cfg2_guided")
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    assert seen == [(4, False, True)] * 2, seen
    assert torch.equal(out["x"], out2["x"]) and torch.equal(out["log_p"], out2["log_p"]), "not deterministic"
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)
    np.testing.assert_allclose(out["log_p"].cpu().numpy(), gold["log_p"], rtol=1e-4, atol=1e-4)
    monkeypatch.setenv("CDX_UNET2_GUIDED_SPLIT", "0")
    plain, _ = _extra("baseline_cfg2_guided")
    assert seen[-1] == (0, False, True)
    np.testing.assert_allclose(out["x"].cpu().numpy(), plain["x"].cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(out["log_p"].cpu().numpy(), plain["log_p"].cpu().numpy(), rtol=2e-4, atol=2e-4)
    monkeypatch.delenv("CDX_UNET2_GUIDED_SPLIT")
    agent, _ = cases.build(amd_lib, "janner_cfg2_guided_ddpm", device=DEV)
    g = torch.Generator().manual_seed(43)
    B = 100
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(6)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=5, temperature=0.5, w_cg=0.3)
    seen.clear()
    xs, ls = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    assert seen == [(2, False, True)], seen
    monkeypatch.setenv("CDX_UNET2_GUIDED_SPLIT", "0")
    xp, lp = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    runtime2.check_split_errors()
    np.testing.assert_allclose(xs.cpu().numpy(), xp.cpu().numpy(), rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(ls["log_p"].cpu().numpy(), lp["log_p"].cpu().numpy(), rtol=2e-4, atol=2e-4)


def test_seeded_device_runs_do_not_depend_on_the_executor(amd_lib, monkeypatch):
    """with torch.manual_seed on the ROCm device the same request must give the same trajectories whether the
    whole-loop launch serves it or the per-step host loop does (``requires_grad=True``, a forced fallback): both draw the loop's noise
    as ONE (n, ...) launch after the initial draw (_NoiseFeed.many / .reserve).  Stochastic solvers: DDPM and SDE-DPM-Solver++ steps."""
    from cleandiffuser_amd.engine import dispatch
    agent, _ = cases.build(amd_lib, "janner_cfg2_ddim", device=DEV)
    prior = torch.zeros(6, 32, 23, device=DEV)
    prior[:, 0, :17] = torch.randn(6, 17, generator=torch.Generator().manual_seed(4)).to(DEV)
    for solver in ("ddpm", "sde_dpmsolver++_1"):
        kw = dict(solver=solver, n_samples=6, sample_steps=8, temperature=0.7)
        fused = _spy_launches(monkeypatch)
        torch.manual_seed(31)
        a, _ = agent.sample(prior, **kw)
        assert fused["n"] == 1
        torch.manual_seed(31)
        b, _ = agent.sample(prior, requires_grad=True, **kw)              # the per-step executor (autograd through the loop)
        monkeypatch.setattr(dispatch, "try_fused_raw", lambda *a_, **k_: None)
        monkeypatch.setattr(dispatch, "try_fused_sample", lambda *a_, **k_: None)
        torch.manual_seed(31)
        c, _ = agent.sample(prior, **kw)                                 # the same host loop, gradients off
        monkeypatch.undo()
        np.testing.assert_allclose(b.detach().cpu().numpy(), a.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=solver)
        np.testing.assert_allclose(c.cpu().numpy(), a.cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=solver)
        torch.manual_seed(32)
        d, _ = agent.sample(prior, **kw)
        assert float((d - a).abs().max()) > 1e-2                         # (another seed: other draws)


# ---- round 5: the default route fails loudly, never NaN-ly ----
def test_device_query_reports_a_whole_mi355x(amd_lib, monkeypatch):
    """cdx_device_query: compute units / architecture from hipDeviceProp_t, the XCD count measured by a probe launch.  The split / grouped
    modes are refused anywhere but a whole 256-CU gfx950 behind 8 XCDs: with the answer forced to 'no' the headline batch takes the
    ordinary program (and no repair launch is enqueued)."""
    from cleandiffuser_amd.engine import runtime2
    p = runtime2.device_props(torch.device(DEV))
    assert p["arch"] == "gfx950" and p["wavefront"] == 64 and p["lds_bytes_per_cu"] >= 160 * 1024, p
    assert p["cu_count"] == torch.cuda.get_device_properties(0).multi_processor_count, p
    assert 1 <= p["xcc_count"] <= 8, p
    assert runtime2.whole_chip(torch.device(DEV)) == (p["cu_count"] == 256 and p["xcc_count"] == 8)
    monkeypatch.setenv("CDX_UNET2_ASSUME_WHOLE_CHIP", "0")
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        seen.append((kws.get("split"), kws.get("group"), kws.get("run_if") is not None))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    out, gold = _extra("baseline_cfg2_b256")
    torch.cuda.synchronize()
    assert seen == [(0, False, False)], seen
    np.testing.assert_allclose(out["x"].cpu().numpy(), gold["x"], **TOL)


def test_a_lost_granule_of_a_grouped_guided_launch_never_reaches_the_caller(amd_lib, monkeypatch):
    """The same fault hook on the GROUPED GUIDED launch: trajectories AND log_p of the call are the ordinary guided program's, bit for
    bit (the repair launch rewrites both), never NaN; the next guided call takes the ordinary program."""
    from cleandiffuser_amd.engine import runtime2
    dev = torch.device(DEV)
    if runtime2._group_ok.get(dev) is not True:
        pytest.skip("the grouped mode failed its self-check on this device")
    agent, _ = cases.build(amd_lib, "janner_cfg2_guided_ddpm", device=DEV)
    g = torch.Generator().manual_seed(12)
    B = 160
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(4)]
    kw = dict(solver="ddpm", n_samples=B, sample_steps=3, temperature=0.5, w_cg=0.3)
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        seen.append((kws.get("split") or 0, kws.get("run_if") is not None))
        return orig(comp, **kws)
    try:
        monkeypatch.setenv("CDX_UNET2_GUIDED_GROUP", "0")
        plain, lp = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        monkeypatch.delenv("CDX_UNET2_GUIDED_GROUP")
        agent.sample(prior.to(DEV), noise=list(zs), **kw)                      # (first use on this device: the mode's own check)
        torch.cuda.synchronize()
        assert runtime2._gguided_ok.get(dev) is True and runtime2.note_exchange_failure(dev) is False
        monkeypatch.setattr(runtime2, "launch", spy)
        monkeypatch.setenv("CDX_UNET2_FAULT", "2")
        hurt, lh = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        monkeypatch.delenv("CDX_UNET2_FAULT")
        assert seen == [(4, False), (0, True)], seen
        torch.cuda.synchronize()
        assert int(runtime2._split_errs[dev][1][0]) != 0, "the fault hook starved nobody: nothing was tested"
        assert torch.isfinite(hurt).all() and torch.isfinite(lh["log_p"]).all(), "a failed exchange reached the caller"
        assert torch.equal(hurt, plain) and torch.equal(lh["log_p"], lp["log_p"]), "the repair launch must leave the ordinary program's result"
        with pytest.warns(UserWarning, match="never received a granule"):
            after, la = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        assert seen[-1] == (0, False) and runtime2._gguided_ok[dev] is False
        assert torch.equal(after, plain) and torch.equal(la["log_p"], lp["log_p"])
    finally:
        try:
            runtime2.check_split_errors(dev, wait=True)
        except RuntimeError:
            pass
        runtime2._group_ok[dev] = runtime2._split_ok[dev] = True
        runtime2._gguided_ok.pop(dev, None)
        runtime2._sguided_ok.pop(dev, None)


@pytest.mark.parametrize("B", [256, 32])
def test_a_lost_granule_never_reaches_the_caller(B, amd_lib, monkeypatch):
    """CDX_UNET2_FAULT makes one member of every group withhold its granules in every exchange of a launch (cdx_unet2_launch.fault):
    the other members' bounded polls run out, they store NaN -- and the REPAIR launch behind the grouped / split launch recomputes the
    request on the ordinary program before anything downstream of the stream can see it.  sample() hands out the ordinary program's
    numbers (bit for bit), never NaN; the NEXT call notices the report, warns and takes the ordinary program; both modes stay off."""
    import warnings
    from cleandiffuser_amd.engine import runtime2
    dev = torch.device(DEV)
    if runtime2._group_ok.get(dev) is not True or runtime2._split_ok.get(dev) is not True:
        pytest.skip("the split / grouped modes failed their self-check on this device")
    agent, _ = cases.build(amd_lib, "janner_cfg2_ddim", device=DEV)
    g = torch.Generator().manual_seed(11)
    prior = torch.zeros(B, 32, 23)
    prior[:, 0, :17] = torch.randn(B, 17, generator=g)
    zs = [torch.randn(B, 32, 23, generator=g).to(DEV) for _ in range(3)]
    kw = dict(solver="ddim", n_samples=B, sample_steps=2, temperature=0.5)
    seen = []
    orig = runtime2.launch

    def spy(comp, **kws):
        seen.append((kws.get("split") or 0, kws.get("run_if") is not None))
        return orig(comp, **kws)
    monkeypatch.setattr(runtime2, "launch", spy)
    try:
        monkeypatch.setenv("CDX_UNET2_GROUP", "0")
        monkeypatch.setenv("CDX_UNET2_SPLIT", "0")
        plain, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        monkeypatch.setenv("CDX_UNET2_GROUP", "auto")
        monkeypatch.setenv("CDX_UNET2_SPLIT", "auto")
        good, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)            # the mode itself, no fault: one launch + an idle repair
        torch.cuda.synchronize()
        assert seen[-2:] == [(4, False), (0, True)], seen
        assert runtime2.note_exchange_failure(dev) is False
        monkeypatch.setenv("CDX_UNET2_FAULT", "2")                             # member 1 of every group stays silent once
        hurt, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
        monkeypatch.delenv("CDX_UNET2_FAULT")
        assert seen[-2:] == [(4, False), (0, True)], seen
        torch.cuda.synchronize()
        assert int(runtime2._split_errs[dev][1][0]) != 0, "the fault hook starved nobody: nothing was tested"
        assert torch.isfinite(hurt).all(), "a failed exchange reached the caller"
        assert torch.equal(hurt, plain), "the repair launch must leave the ordinary program's result"
        np.testing.assert_allclose(hurt.cpu().numpy(), good.cpu().numpy(), rtol=2e-4, atol=2e-4)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            after, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)       # notices the report: ordinary program, no repair launch
        assert seen[-1] == (0, False) and any("never received a granule" in str(m.message) for m in w), (seen[-3:], [str(m.message) for m in w])
        assert runtime2._group_ok[dev] is False and runtime2._split_ok[dev] is False
        assert runtime2.last_exchange_error[dev]["what"] == "granule"
        assert torch.equal(after, plain)
    finally:
        # give the modes back to the tests that follow: nothing in flight after the synchronise, the report is cleared
        try:
            runtime2.check_split_errors(dev, wait=True)
        except RuntimeError:
            pass
        runtime2._group_ok[dev] = runtime2._split_ok[dev] = True
        runtime2._gguided_ok.pop(dev, None)              # (the guided modes check themselves again on their next use)
        runtime2._sguided_ok.pop(dev, None)
    monkeypatch.setattr(runtime2, "launch", orig)
    again, _ = agent.sample(prior.to(DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    runtime2.check_split_errors(dev)
    assert torch.equal(again, good)
