"""TEST HELPER for QGPO's contrastive energy training step (engine/cep.py): the cases of tests/golden/qgpo_cep.npz, the classifiers they
build from either library (``oracle.cases.lib_namespace("reference" | "amd")``), the kernel's request for a case, and for each case ONE
float64 autograd run of the package's own ``QGPOClassifier.loss`` -- the reference the CPU tests compare ``reference_step`` with.
tools/gen_qgpo_cep_golden.py runs the real reference on the same table.

Every case is ``clf.update(x, t, {"soft_label", "obs"}, update_ema)`` of a QGPOClassifier(QGPONNClassifier(O, A, Ec, hidden,
"untrainable_fourier")) with ``optim_params={"lr": 1e-3}``: the call of reference pipelines/qgpo_d4rl_mujoco.py:174-196.  Weights are
``load_synth`` streams; the head is scaled by `head_scale` so that the reference's own energies stay out of the tanh's saturation (the
generator asserts it).  Soft labels are a softmax over K of a synthetic Q stream, times `label_scale`."""
import contextlib
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cases as _cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qgpo_cep.npz")
LR = 1e-3                      # what the pipeline sets
CALLS = 3                      # consecutive update() calls the fixture records
LOG_KEYS = ("loss", "f_max", "f_mean", "f_min", "grad_norm")


def _c(B, K, O, A, Ec, hidden, label_scale=1.0, clip=None, update_ema=True, head_scale=8.0, grads=True):
    return SimpleNamespace(B=B, K=K, O=O, A=A, Ec=Ec, hidden=list(hidden), label_scale=label_scale, clip=clip, update_ema=update_ema,
                           head_scale=head_scale, grads=grads)


CASES = {
    # full tiles; unequal widths; A and O no multiples of 4
    "k16_full": _c(3, 16, 7, 3, 16, [32, 48]),
    # four groups per tile; a ragged last tile of one group; labels that do not sum to 1
    "k4_ragged": _c(5, 4, 11, 3, 16, [32], label_scale=0.7),
    # K = 1: log-softmax is 0 and the loss gradient vanishes -- the step still runs
    "k1": _c(21, 1, 7, 6, 16, [32, 32, 32]),
    # two groups per tile; ragged; the gradient norm clipped
    "k8_ragged": _c(9, 8, 7, 3, 32, [48, 32], clip=0.5),
    # the shipped widths at a small batch; no EMA update (gradients too large for the fixture: not stored)
    "shipped_b8": _c(8, 16, 17, 6, 64, [256, 256, 256], update_ema=False, grads=False),
}
GOLDEN_TABLE = list(CASES)         # the cases tests/golden/qgpo_cep.npz holds a record of

# the edges of what cep_plan / em_plan admit (A <= 64, O <= 512, Ec <= 128, widths <= 512, LDS <= 160 KiB): no record of the real
# reference, held to float64 autograd of the package's own loss on the CPU and to the float64 restatement on the device
ENVELOPE = {
    # the kitchen classifier (obs 60, act 9) at the shipped widths: 85 KiB of LDS
    "kitchen_k16_b3": _c(3, 16, 60, 9, 64, [256, 256, 256]),
    # every limit at once: O = 512 (32 K blocks in obs_proj), A = 64, Ec = 128, two 512-wide layers (both sweeps): 133 KiB of LDS
    "limits_k8_b3": _c(3, 8, 512, 64, 128, [512, 512], head_scale=4.0),
    # a partial second sweep (272 = 17 column tiles), O = 85 (six K blocks through the scalar weight loads), A = 17
    "sweep272_k4_b5": _c(5, 4, 85, 17, 32, [272, 272]),
}
CASES.update(ENVELOPE)
TABLE = list(CASES)


def build(case, lib, device="cpu", dtype=torch.float32):
    """The classifier of a case from `lib` (this package or the real reference)."""
    from cleandiffuser_amd.utils import load_synth
    net = load_synth(lib.QGPONNClassifier(case.O, case.A, case.Ec, list(case.hidden), "untrainable_fourier"), 73)
    with torch.no_grad():
        head = net.mlp.mlp[-2]
        head.weight.mul_(case.head_scale)
        head.bias.mul_(case.head_scale)
    net = net.to(device=device, dtype=dtype)
    return lib.QGPOClassifier(net, grad_clip_norm=case.clip, optim_params={"lr": LR}, device=device)


def make_inputs(name: str):
    """x (B, K, A), t (B,), obs (B, O), soft_label (B, K, 1) of a case as float32 numpy arrays: seeded draws (what the fixture records)."""
    case = CASES[name]
    g = torch.Generator().manual_seed(2000 + TABLE.index(name))
    x = torch.randn(case.B, case.K, case.A, generator=g)
    t = 1e-3 + 0.999 * torch.rand(case.B, generator=g)
    obs = torch.randn(case.B, case.O, generator=g)
    soft = case.label_scale * torch.softmax(1.5 * torch.randn(case.B, case.K, 1, generator=g), 1)
    return {"x": x.numpy(), "t": t.numpy(), "obs": obs.numpy(), "soft_label": soft.numpy()}


def tensors(inp, device="cpu", dtype=torch.float32):
    """(x, t, y) of ``update`` from recorded inputs."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)          # noqa: E731
    return t(inp["x"]), t(inp["t"]), {"soft_label": t(inp["soft_label"]), "obs": t(inp["obs"])}


def golden(name: str):
    """The fixture's arrays of a case: the inputs, ``log`` (CALLS, 5) in the order of LOG_KEYS (grad_norm NaN where the reference
    returned None), ``sums`` / ``sums_ema`` (parameters, 2) = mean and mean |.| after the last call, ``grad/<parameter name>`` after the
    first backward pass (small cases)."""
    with np.load(GOLDEN) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


def checksums(module):
    """(parameters, 2): mean and mean |.| of every parameter, in ``parameters()`` order."""
    return np.array([[float(p.detach().double().mean()), float(p.detach().double().abs().mean())] for p in module.parameters()])


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def request(clf, x, t, y):
    """The kernel's request for ``clf.update(x, t, y)`` (any dtype / device; the time table by the module itself)."""
    from cleandiffuser_amd.engine import cep
    desc = cep.describe(clf.model)
    b, k, a = x.shape
    with torch.no_grad():
        temb = clf.model.map_noise(t).to(x.dtype).contiguous()
    return cep.make_request([p.detach() for p in cep.weights_of(desc)], x.reshape(b * k, a).contiguous(), y["obs"].contiguous(), temb,
                            y["soft_label"].reshape(b * k).contiguous(), k)


def trainable(module):
    """[(name, parameter)] of the parameters that take gradients, in ``engine.cep.weights_of`` order (obs_proj, act_proj, the mlp)."""
    return [(n, p) for n, p in module.named_parameters() if p.requires_grad]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Float64 autograd of this package's ``QGPOClassifier.loss`` on the CPU for case `name`: loss, the three statistics and the gradient
    of every trainable parameter.  Computed once per process and never modified."""
    case, inp = CASES[name], make_inputs(name)
    clf = build(case, _cases.lib_namespace("amd"), "cpu", torch.float64)
    x, t, y = tensors(inp, dtype=torch.float64)
    loss, stats = clf.loss(x, t, y)
    params = trainable(clf.model)
    grads = torch.autograd.grad(loss, [p for _, p in params])
    return SimpleNamespace(case=case, inp=inp, loss=float(loss.detach()), stats=stats, grads={n: g.detach() for (n, _), g in zip(params, grads)})
