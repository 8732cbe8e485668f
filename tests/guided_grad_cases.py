"""TEST HELPER for the classifier gradient of the guided program kernel (`cdx_unet2_kernel<T, 8, true, ...>`): a table of
(denoiser, classifier, horizon) rows pinned BY VALUE, the program forms each row exists in, and per row ONE float64 CPU autograd run of
the classifier module -- the reference tests/test_guided_grad_cases_cpu.py and tests/test_gpu_guided_grad.py compare with.  Computed
once per process and never modified.

Forms (what `runtime2._compile_guided2` can return):
    lds          one trajectory per workgroup, everything in LDS
    ws           one trajectory per workgroup, saved tensors in the global workspace (`save_global`)
    ws_compact   the same with state / multistep memory in global memory too (`save_global + compact`)
    two          two trajectories per workgroup (`two=True`)
    three        three trajectories per workgroup, compact (`three=True`)
The rows were chosen by running the compiler (host code) over candidate shapes; the CPU test fails when a compiler change moves a row
to another form, so the GPU coverage cannot thin out silently.
"""
import copy
import functools
from types import SimpleNamespace

import torch

from rollout_cases import float64_default

FORMS = ("lds", "ws", "ws_compact", "two", "three")
T_OF = {"lds": 1, "ws": 1, "ws_compact": 1, "two": 2, "three": 3}
T_MAX = 999           # the largest step of the default schedule (diffusion_steps = 1000)
B = 7                 # odd for two per workgroup, 2 x 3 + 1 for three: the last workgroup is part-empty in both
ALL3 = ("lds", "two", "three")


def _r(den, clf, H, D, t, forms, seeds=(1, 2), edge=""):
    """den = (model_dim, dim_mult, kernel_size) of JannerUNet1d(D, ...); clf = the same of HalfJannerUNet1d(H, D, out_dim=1, ...);
    emb_dim = model_dim in both.  t: the row's timestep.  seeds: load_synth seeds of (denoiser, classifier)."""
    return SimpleNamespace(den=den, clf=clf, H=H, D=D, t=t, forms=tuple(forms), seeds=seeds, edge=edge)


ROWS = {
    # the config-2 pair of test_guided_program_gradient_matches_autograd (oracle/cases.py: janner_cfg2_guided_ddpm, weights included)
    "cfg2": _r((32, (1, 2, 2, 2), 5), (32, (1, 2, 2, 2), 3), 32, 23, 7, ALL3, seeds=(0, 1), edge="config 2"),
    "md8_h16_d6": _r((8, (1, 2, 4), 3), (64, (1, 2), 3), 16, 6, 0, ALL3, edge="model_dim 8, t = 0"),
    "md8_h32_d36": _r((8, (1, 1), 3), (32, (1, 1), 3), 32, 36, 19, ALL3, edge="D > 32"),
    "md64_h8_d37": _r((64, (1, 2, 4), 5), (32, (1, 1), 3), 8, 37, T_MAX, ALL3, edge="odd D, model_dim 64, H = 8, t = T_MAX"),
    "md64_h4_d4": _r((64, (1,), 5), (64, (1,), 5), 4, 4, 3, ALL3, edge="H = 4, one level, classifier kernel 5"),
    "md16_h16_d14": _r((16, (1, 2, 4), 3), (16, (1, 2, 4), 3), 16, 14, 500, ALL3, edge="three-level classifier with a factor 4"),
    "md8_h8_d1": _r((8, (1,), 3), (64, (1,), 3), 8, 1, 1, ALL3, edge="D = 1"),
    "md64_h8_d28": _r((64, (1, 4), 5), (32, (1, 4), 5), 8, 28, 12, ALL3, edge="dim_mult (1, 4), classifier kernel 5"),
    "md8_h64_d31": _r((8, (1, 1), 3), (16, (1, 1), 3), 64, 31, 0, ("lds", "two"), edge="H = 64, no three"),
    "md16_h64_d25": _r((16, (1, 2, 4), 3), (32, (1, 2), 3), 64, 25, T_MAX, ("lds",), edge="one trajectory fills the CU (148 KB)"),
    "md16_h64_d33": _r((16, (1, 2, 2), 3), (32, (1, 2, 2), 5), 64, 33, 40, ("ws",), edge="smallest ws pair found, D > 32"),
    "md64_h64_d7": _r((64, (1, 1), 5), (64, (1, 2), 5), 64, 7, 250, ("ws",), edge="ws, model_dim 64"),
    # the kitchen and antmaze Diffuser sizes of test_shipped_large_diffuser_configs_stay_native (oracle/extra_cases.py, weights included)
    "kitchen": _r((64, (1, 2, 2, 2), 5), (64, (1, 2, 2, 2), 3), 32, 69, 4, ("ws",), seeds=(21, 22), edge="kitchen Diffuser"),
    "antmaze": _r((64, (1, 2, 2, 2), 5), (64, (1, 2, 2, 2), 3), 64, 37, 8, ("ws_compact",), seeds=(21, 22), edge="antmaze Diffuser"),
    "md64_h64_d2": _r((64, (1, 2, 2, 2), 5), (16, (1, 1), 5), 64, 2, 999, ("ws_compact",), edge="smallest ws_compact pair found"),
}
BATCH = {"cfg2": 70}            # (more workgroups than one XCD holds, as the old test); every other row: B
PAIRS = [(name, form) for name, row in ROWS.items() for form in row.forms]

# Distance of torch's fp32 CPU autograd (8 intra-op threads) from the float64 reference below, worst row of the table:
# E_GRAD = max|g32 - g64| / max|g64|, E_LOGP the same of the classifier's forward value.  The GPU bars are 16 x these.
# Measured 2026-10-19, torch 2.10.0 (tests/test_guided_grad_cases_cpu.py re-measures them and fails outside a factor 2).
E_GRAD = 1.33e-6        # (row md16_h16_d14; the other rows 4.9e-7 .. 1.15e-6)
E_LOGP = 1.32e-6        # (row antmaze; the other rows 2.9e-7 .. 1.23e-6)

# (row, form) -> relative bar of the rows whose kernel error is a property of the program's own fp32 summation order: 2 x the error of
# the CPU twin (oracle/lane_sim2.py) on the same inputs, never above TWIN_BAR_MAX.  Every other pair: 16 x E_GRAD.
TWIN_BAR_MAX = 2e-4
ROW_BARS = {}           # (none needed: see the table)

# Measured on an MI355X, 2026-10-19 (tests/test_gpu_guided_grad.py prints these figures): max|g_kernel - g64| / max|g64| over the batch
# per (row, form), B = 7; E_GRAD = 1.33e-6, bar applied = 16 x E_GRAD = 2.13e-5 for EVERY pair -- no row needed the twin-based bar.
#   row            lds       ws        ws_compact  two       three     | logp (lds)  | wrapper grad / logp  | CPU twin (3 samples)
#   cfg2           6.7e-7    -         -           1.0e-6    1.0e-6    | 3.2e-7      | 8.2e-7 / 2.9e-7      | 4.5e-7 .. 5.2e-7
#   cfg2 (B = 70)  7.2e-7    -         -           6.4e-7    6.4e-7    | 4.2e-7      |                      |
#   md8_h16_d6     5.5e-7    -         -           6.0e-7    6.0e-7    | 7.9e-7      | 5.4e-7 / 1.6e-6      | 3.7e-7 .. 4.3e-7
#   md8_h32_d36    4.7e-7    -         -           4.7e-7    4.7e-7    | 4.6e-7      | 4.2e-7 / 6.7e-7      | 3.6e-7
#   md64_h8_d37    6.3e-7    -         -           6.3e-7    6.3e-7    | 4.1e-7      | 7.9e-7 / 2.4e-7      | 6.3e-7
#   (B = 1)        5.6e-7                                              | 3.6e-7      |                      |
#   md64_h4_d4     4.7e-7    -         -           4.7e-7    4.7e-7    | 4.2e-7      | 3.4e-7 / 3.8e-7      | 4.3e-7
#   md16_h16_d14   1.9e-6    -         -           1.9e-6    1.9e-6    | 2.8e-7      | 6.7e-7 / 4.0e-7      | 1.4e-6
#   md8_h8_d1      7.6e-7    -         -           6.3e-7    6.3e-7    | 2.4e-7      | 5.1e-7 / 2.2e-7      | 2.5e-7 .. 3.8e-7
#   md64_h8_d28    9.5e-7    -         -           9.5e-7    9.5e-7    | 2.6e-7      | 5.6e-7 / 4.5e-7      | 5.1e-7
#   md8_h64_d31    5.0e-7    -         -           5.1e-7    -         | 4.9e-7      | 4.4e-7 / 2.0e-7      | 3.7e-7 .. 4.3e-7
#   md16_h64_d25   7.4e-7    -         -           -         -         | 4.8e-7      | 4.9e-7 / 3.8e-7      | 4.5e-7
#   md16_h64_d33   -         7.6e-7    -           -         -         |             | 4.5e-7 / 1.1e-6      | 4.1e-7
#   md64_h64_d7    -         1.3e-6    -           -         -         |             | 6.5e-7 / 4.5e-7      | 5.7e-7
#   kitchen        -         8.1e-7    -           -         -         |             | 5.5e-7 / 1.3e-6      | 6.5e-7
#   antmaze        -         -         1.1e-6      -         -         |             | 7.2e-7 / 8.0e-7      | 7.6e-7
#   md64_h64_d2    -         -         6.4e-7      -         -         |             | 5.3e-7 / 2.8e-7      | 5.0e-7
# Before the backward epilogue's second store (F2_DUAL) was kept to the lane groups that own real channels, every row whose classifier
# has a layer of fewer than 32 channels failed here with errors of 1 .. 80 x max|g64| that changed from launch to launch: md8_h64_d31 and
# md64_h64_d2 in every form, md8_h32_d36 / md64_h8_d37 / md64_h4_d4 / md16_h16_d14 / md8_h8_d1 as `two` and `three`.


def grad_bar(name, form) -> float:
    bar = ROW_BARS.get((name, form), 16 * E_GRAD)
    assert bar <= TWIN_BAR_MAX
    return bar


def build(name, lib, device="cpu"):
    """(denoiser, classifier) of row `name` with their synthetic weights, eval mode, on `device`."""
    from cleandiffuser_amd.utils import load_synth
    row = ROWS[name]
    (md, dm, ks), (cmd, cdm, cks) = row.den, row.clf
    net = load_synth(lib.JannerUNet1d(row.D, model_dim=md, emb_dim=md, dim_mult=list(dm), kernel_size=ks), row.seeds[0])
    clf = load_synth(lib.HalfJannerUNet1d(row.H, row.D, out_dim=1, model_dim=cmd, emb_dim=cmd, dim_mult=tuple(cdm), kernel_size=cks), row.seeds[1])
    return net.eval().to(device), clf.eval().to(device)


def form_of(prog) -> str:
    """The form of a one-trajectory guided program (what `runtime2._compile_guided2(net, clf, H, False, False)` returned)."""
    return "ws_compact" if prog.compact else "ws" if prog.ws_floats else "lds"


def inputs(name):
    """x (batch, H, D) fp32 from the row's seeded generator, and the per-sample timesteps of the wrapper test (a fixed pattern that holds
    0 and T_MAX in every row)."""
    row = ROWS[name]
    b = BATCH.get(name, B)
    g = torch.Generator().manual_seed(1000 + list(ROWS).index(name))
    x = torch.randn(b, row.H, row.D, generator=g)
    pattern = (0, T_MAX, 1, 19, 250, 7, 998)
    t_each = torch.tensor([pattern[(i + list(ROWS).index(name)) % len(pattern)] for i in range(b)], dtype=torch.long)
    return x, t_each


def autograd(clf, x, t):
    """(classifier value (b, 1), d value.sum() / d x) of `clf._forward_torch` under torch.autograd, in the module's dtype."""
    xr = x.clone().requires_grad_()
    y = clf._forward_torch(xr, t, None)
    y.sum().backward()
    return y.detach(), xr.grad.detach()


@functools.lru_cache(maxsize=None)
def reference(name, per_sample=False):
    """The float64 CPU autograd of row `name`: namespace with x (fp32), t (b,) -- the row's one timestep, or the per-sample pattern --
    and logp (b, 1) / grad (b, H, D) in float64.  Every sample is independent of the others, so a test may take the first rows."""
    from oracle import cases as _cases
    row = ROWS[name]
    x, t_each = inputs(name)
    t = t_each if per_sample else torch.full((x.shape[0],), row.t, dtype=torch.long)
    with float64_default():
        # (under the float64 default: integer timesteps give cos / sin of the embedding in the DEFAULT dtype, fp32 otherwise)
        _, clf = build(name, _cases.lib_namespace("amd"))
        clf = copy.deepcopy(clf).double()
        logp, grad = autograd(clf, x.double(), t)
    assert logp.dtype == grad.dtype == torch.float64
    return SimpleNamespace(row=row, x=x, t=t, logp=logp, grad=grad)
