"""The native training graphs (cleandiffuser_amd/engine/train.py: nine families of per-layer forward / backward nodes on the HIP
kernels) against float64, whole: every case of tests/train_graph_cases.py runs ``net(x, t, cond)`` with autograd on the device and is
compared with the float64 CPU run of the module's own PyTorch forward (one run per case and process, ``train_graph_cases.reference``)
-- output, input gradient and the gradient of EVERY parameter.

Tolerance: 4 x YARDSTICK[family] in the error measure of train_graph_cases (relative to the tensor's largest element; floors: 1 for
the output, 1e-3 of the case's largest parameter gradient for a parameter gradient).  YARDSTICK is how far fp32 CPU autograd of the
same graph lies from float64 (tests/test_train_graph_cases_cpu.py); the factor 4 covers the other summation order and FMA contraction
of the device kernels.  Nothing here is derived from a device result, and no same-device ATen result is involved: the batch-257 and
batch-256 cases lie past the batch from which this ROCm build's ``group_norm`` backward is wrong.

Three gradient routes per case:

1. plain ``backward()``: autograd accumulates what the nodes return;
2. inside ``train.grads_in_place(params)``: the kernels add straight into ``.grad``, the weight-gradient products through the queued
   ``cdx_conv_wgrad_batch_f32`` launch (asserted: that launch ran and no single ``conv_wgrad`` did -- but for ChiTransformer's
   cross-attention, whose projections are slices of ``in_proj_weight`` and so stay with autograd);
3. a second forward + backward inside the scope without zeroing: ``.grad`` (and the input's) must hold 2 x the reference -- the
   kernels ADD onto what is there.

``train.forward`` is spied on: exactly one call per ``net(...)`` returns a tensor, so the native graph ran, not the torch fallback.

Measured on an MI355X, largest device error per case (the three routes agree to the second digit) against its tolerance:

    janner_ragged 1.4e-6, janner_h4 1.4e-6, janner_b257 2.3e-6 (1.2e-5)       chi_scale 1.3e-6, chi_shift 2.4e-6, chi_b256 1.8e-6 (1.2e-5)
    half_janner_b5 1.4e-6, half_janner_b1 1.3e-6 (8.0e-6)                     dit_d64 7.7e-7, dit_d72_t33 1.2e-6, dit_limits 4.6e-7, half_dit 6.6e-7 (3.6e-6)
    chitf_encoder 7.7e-7, chitf_mlp 5.3e-7 (6.0e-6)                           idql_h64 6.6e-7, idql_h320_b17 5.2e-7, newidql_cond 3.9e-7 (6.0e-6)
    dql_b5 3.6e-7, dvinv_b17 3.1e-7 (3.2e-6)                                  pearce_b7 5.8e-7 (3.2e-6)        sfbc_b6 1.5e-6 (6.0e-6)

Per family: janner 2.3e-6, chi 2.4e-6, half_janner 1.4e-6, dit 1.2e-6, chitf 7.7e-7, idql 6.6e-7, mlp 3.6e-7, pearce 5.8e-7, sfbc
1.5e-6 -- the device lies about as far from float64 as fp32 CPU autograd does (the yardsticks), a third of the tolerance at most; no
family needed a factor of its own, and no route fell back.  `pytest -s` prints every figure."""
import contextlib
import copy

import pytest
import torch

import train_graph_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _collect(net, x, y):
    return {"y": y.detach(), "dx": x.grad.detach().clone(), "grads": G.grads_of(net)}


@pytest.mark.parametrize("name", G.TABLE)
def test_native_training_graph_matches_float64(name, monkeypatch):
    from cleandiffuser_amd.engine import blocks, train
    ref = G.reference(name)
    tol = G.tolerance(name)
    monkeypatch.setenv("CDX_TRAIN_NATIVE", "1")
    for var in ("CDX_TRAIN_INPLACE_GRADS", "CDX_TRAIN_WGRAD_BATCH"):
        monkeypatch.delenv(var, raising=False)
    net = copy.deepcopy(ref.net).to(DEV).train()
    if hasattr(net, "pos_emb_cache"):
        net.pos_emb_cache = None
    params = list(net.parameters())
    x, t, cond, wgt = G.cast(ref.inp, torch.float32, DEV)

    served, launches = [], {"conv_wgrad": 0, "conv_wgrad_batch": 0}
    forward, single, batched = train.forward, blocks.conv_wgrad, blocks.conv_wgrad_batch

    def spy(*a, **k):
        out = forward(*a, **k)
        served.append(torch.is_tensor(out))
        return out

    def counted(which, fn):
        def run(*a, **k):
            launches[which] += 1
            return fn(*a, **k)
        return run
    monkeypatch.setattr(train, "forward", spy)
    monkeypatch.setattr(blocks, "conv_wgrad", counted("conv_wgrad", single))
    monkeypatch.setattr(blocks, "conv_wgrad_batch", counted("conv_wgrad_batch", batched))

    def step(in_place):
        served.clear()
        fam = train.family_of(net, x, cond)
        assert fam is not None and fam.name == ref.case.family
        y = net(x, t, cond)
        assert served == [True], f"exactly one train.forward call must serve net(...), got {served}: the torch fallback ran"
        with (train.grads_in_place(params) if in_place else contextlib.nullcontext()):
            G.objective(y, wgt).backward()
        torch.cuda.synchronize()
        assert not train._wgrad_queues
        return _collect(net, x, y)

    report = []
    # route 1: autograd's own accumulation
    e1 = G.errors(ref, step(False))
    report.append(("backward()", *G.worst(e1)))
    assert launches["conv_wgrad_batch"] == 0 and launches["conv_wgrad"] > 0
    # route 2: straight into .grad, the weight gradients in the queued batch
    net.zero_grad(set_to_none=True)
    x.grad = None
    launches.update(conv_wgrad=0, conv_wgrad_batch=0)
    got = step(True)
    e2 = G.errors(ref, got)
    report.append(("grads_in_place", *G.worst(e2)))
    # (ChiTransformer's cross-attention projects with SLICES of in_proj_weight: not parameters, so autograd keeps those products)
    assert launches["conv_wgrad_batch"] == 1 and (launches["conv_wgrad"] == 0 or ref.case.family == "chitf"), launches
    assert all(g is None or g.is_contiguous() for g in got["grads"].values())
    # route 3: once more without zeroing -- 2 x
    e3 = G.errors(ref, step(True), times=2.0)
    report.append(("grads_in_place, second pass", *G.worst(e3)))
    print()
    for route, k, w in report:
        print(f"{name} [{route}]: largest device error {w:.2e} ({k}), tolerance {tol:.1e}")
    for route, k, w in report:
        assert w <= tol, f"{name} [{route}]: {k} is {w:.3e} from float64, tolerance {tol:.1e}"
