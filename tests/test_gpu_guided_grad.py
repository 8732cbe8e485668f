"""The classifier gradient of the guided program kernel on silicon (run with ``pytest -m gpu`` on an MI355X): d clf(x, t).sum() / d x of
every pinned (row, form) of tests/guided_grad_cases.py -- the all-in-LDS program, its two workspace fallbacks, the two- and the
three-trajectory programs -- against ONE float64 CPU autograd run of the classifier module per row.

The bar comes from the reference side, not from the kernel: torch's own fp32 autograd is E_GRAD (max norm, relative to the largest
element) from float64 over the table; the kernel gets 16 x that (another summation order and K splits, hardware exp / reciprocal, the
few-fold spread of a ~50-op fp32 chain's max-norm error between summation orders) -- about 2e-5 of the largest element.  Rows that needed
the twin-based bar of the table (`guided_grad_cases.ROW_BARS`) say so there.  A missing program is a failure, never a skip."""
import pytest
import torch

import guided_grad_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B = 7 throughout (part-empty last workgroup at two and at three per workgroup); config 2 also at B = 70 (more workgroups than one XCD
# holds; 70 = 23 x 3 + 1) and one all-in-LDS row at B = 1
PARAMS = [(name, form, G.B) for name, form in G.PAIRS] + [("cfg2", form, 70) for form in G.ROWS["cfg2"].forms] + [("md64_h8_d37", "lds", 1)]
_built = {}


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from cleandiffuser_amd.engine import runtime
    runtime.load_library()          # hard failure if libcdx.so is missing -- never a silent eager fallback


def _nets(name, lib):
    """(denoiser, classifier, CumRewClassifier wrapper) of a row on the device -- built once, so every program is compiled once per
    (net, form) (runtime2 keeps them per owner module)."""
    if name not in _built:
        net, clf = G.build(name, lib, DEV)
        wrapper = lib.CumRewClassifier(clf, device=DEV)
        wrapper.eval()
        _built[name] = (net, clf, wrapper)
    return _built[name]


def _poison():
    """Whatever stale memory a launch might read -- its workspace, its output -- is NaN first: the program kernel's workspace is
    dropped so that the next launch allocates it anew, then a NaN-filled block (and a small one, for the allocator's small pool) is
    allocated and dropped."""
    from cleandiffuser_amd.engine import runtime2
    runtime2._ws.clear()
    torch.full((1 << 22,), float("nan"), device=DEV)
    torch.full((1 << 16,), float("nan"), device=DEV)


def _rel(got, want):
    """(max |got - want|, max |want|) over the whole batch, in float64."""
    return float((got.detach().cpu().double() - want).abs().max()), float(want.abs().max())


@pytest.mark.parametrize("name,form,b", PARAMS, ids=[f"{n}-{f}-b{b}" for n, f, b in PARAMS])
def test_guided_program_gradient_against_float64(name, form, b, amd_lib):
    from cleandiffuser_amd.engine import runtime2
    row, ref = G.ROWS[name], G.reference(name)
    net, clf, _ = _nets(name, amd_lib)
    arg = form if form in ("two", "three") else None
    comp = runtime2.compiled_guided2(net, clf, row.H, two=form == "two", three=form == "three")
    assert comp.prog is not None, (name, form, comp.why)
    assert form == (G.form_of(comp.prog) if arg is None else form) and bool(comp.prog.compact) == (form in ("ws_compact", "three"))
    x, t = ref.x[:b].to(DEV), ref.t[:b].to(DEV)
    grads = []
    for _ in range(2):
        _poison()
        grads.append(runtime2.classifier_gradient2(net, clf, x, t, form=arg))
        assert grads[-1] is not None, (name, form)
    torch.cuda.synchronize()
    assert grads[0].shape == x.shape and bool(torch.isfinite(grads[0]).all())
    assert torch.equal(grads[0], grads[1])
    err, scale = _rel(grads[0], ref.grad[:b])
    bar = G.grad_bar(name, form)
    print(f"GRAD {name} {form} b={b}: err {err / scale:.3e} of max|g64| = {scale:.3e}  (E_GRAD {G.E_GRAD:.2e}, bar {bar:.3e})")
    assert err <= bar * scale, (name, form, err / scale, bar)
    if form == "lds":
        # the log_p pass of the same kernel (the classifier's own program; one trajectory per workgroup, state in LDS)
        _poison()
        logp = runtime2.classifier_forward2(clf, x, t)
        assert logp is not None, name
        torch.cuda.synchronize()
        assert logp.shape == (b, 1) and bool(torch.isfinite(logp).all())
        err, scale = _rel(logp, ref.logp[:b])
        print(f"LOGP {name} lds b={b}: err {err / scale:.3e} of max|logp64| = {scale:.3e}  (E_LOGP {G.E_LOGP:.2e}, bar {16 * G.E_LOGP:.3e})")
        assert err <= 16 * G.E_LOGP * scale, (name, err / scale)


@pytest.mark.parametrize("name", list(G.ROWS))
def test_classifier_wrapper_gradients_against_float64(name, amd_lib, monkeypatch):
    """The second device implementation of the same gradient: ``CumRewClassifier.gradients(x, t, None)`` with per-sample timesteps
    (cdx_hjgrad_run behind engine/classifier_grad.py) -- served natively, both returned values at the same two bars."""
    from cleandiffuser_amd.engine import classifier_grad
    ref = G.reference(name, per_sample=True)
    _, _, wrapper = _nets(name, amd_lib)
    served = {"n": 0}
    real = classifier_grad.gradients

    def counted(*a, **k):
        out = real(*a, **k)
        served["n"] += out is not None
        return out
    monkeypatch.setattr(classifier_grad, "gradients", counted)
    b = G.B
    x, t = ref.x[:b].to(DEV), ref.t[:b].to(DEV)
    _poison()
    logp, grad = wrapper.gradients(x.clone(), t, None)
    torch.cuda.synchronize()
    assert served["n"] == 1, "the autograd path served the request"
    assert grad.shape == x.shape and logp.shape == (b, 1) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(logp).all())
    eg, sg = _rel(grad, ref.grad[:b])
    el, sl = _rel(logp, ref.logp[:b])
    print(f"WRAP {name}: grad err {eg / sg:.3e} (bar {16 * G.E_GRAD:.3e})  logp err {el / sl:.3e} (bar {16 * G.E_LOGP:.3e})")
    assert eg <= 16 * G.E_GRAD * sg, (name, eg / sg)
    assert el <= 16 * G.E_LOGP * sl, (name, el / sl)


@pytest.mark.parametrize("name", ["md8_h64_d31", "md8_h32_d36"])
def test_guided_sampling_with_a_narrow_classifier_is_reproducible_and_agrees_with_the_executor(name, amd_lib, monkeypatch):
    """What production sees of the same gradient: the guided sampling loop (n_steps > 0) of the one-trajectory program with a classifier
    whose layers have fewer than 32 channels -- bit-identical from call to call, and 1e-4 from the per-step executor (cdx_guided_run,
    the second implementation above).  The lane groups past C_out of the backward epilogue once stored over the next position's
    channels of such a slot: the loop then differed by several units, differently in every call."""
    row = G.ROWS[name]
    net, clf, wrapper = _nets(name, amd_lib)
    agent = amd_lib.DiscreteDiffusionSDE(net, None, classifier=wrapper, diffusion_steps=20, predict_noise=False, device=DEV)
    agent.eval()
    gen = torch.Generator().manual_seed(3)
    b = G.B
    zs = [torch.randn(b, row.H, row.D, generator=gen).to(DEV) for _ in range(6)]
    kw = dict(solver="ddpm", n_samples=b, sample_steps=3, temperature=0.5, w_cg=0.3)
    monkeypatch.setenv("CDX_UNET2_T", "1")                    # the ordinary program, not the small-batch member programs
    from cleandiffuser_amd.engine import runtime2
    guided, real = {"n": 0}, runtime2.launch

    def counted(*a, **k):
        guided["n"] += k.get("cg_scale") is not None and k.get("t_per_wg") == 1
        return real(*a, **k)
    monkeypatch.setattr(runtime2, "launch", counted)
    outs = []
    for _ in range(3):
        x, _ = agent.sample(torch.zeros(b, row.H, row.D, device=DEV), noise=list(zs), **kw)
        outs.append(x.clone())
    assert guided["n"] == 3, "the guided program did not serve the loop"
    monkeypatch.setenv("CDX_UNET2_GUIDED", "0")
    want, _ = agent.sample(torch.zeros(b, row.H, row.D, device=DEV), noise=list(zs), **kw)
    torch.cuda.synchronize()
    assert guided["n"] == 3, "the executor run went through the guided program"
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    torch.testing.assert_close(outs[0], want, rtol=1e-4, atol=1e-4)
