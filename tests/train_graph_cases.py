"""TEST HELPER for the native training graphs (cleandiffuser_amd/engine/train.py): a table of small nets and inputs, one per edge of the
per-layer forward / backward graphs of the nine families of ``train.FAMILIES``, and for each of them ONE float64 CPU run of the module's
own PyTorch forward -- the reference tests/test_gpu_train_graphs.py compares the device with -- next to the same run in float32.

A case names its family, builds its net with ``load_synth`` from a seed (every dropout probability 0, ``train()`` mode) and draws
``(x, noise / t, condition)`` and the weights `wgt` of the objective from one seeded generator, in float64: every run rounds the same
numbers to its own dtype.  The scalar differentiated is ``(y * wgt).sum() / batch``, `wgt` one draw per OUTPUT element.

Error of a tensor against the float64 run:  E = max |got - g64| / max(max |g64|, floor), with the floor

* 1.0 for the output `y`;
* 1e-3 of the case's largest parameter-gradient magnitude for a parameter gradient (a gradient that is small next to the others is
  measured against them, not against itself: its absolute error is what an optimiser step sees);
* none for the input gradient `dx` (relative to its own largest element).

``YARDSTICK[family]`` is the largest E of the float32 CPU run over the family's cases and tensors, rounded up: how far plain fp32
autograd of the same graph lies from float64.  tests/test_train_graph_cases_cpu.py asserts it; the device tolerance is 4 x that (the
project's margin for another summation order and FMA contraction, as in tests/test_gpu_solver_step.py).  Nothing here is derived from
a device result.

Why these shapes (the smallest that reach the edge):

* janner_ragged: 23 channels (the scalar loads of the first layer), rows 24 / 12 / 6 per level -- every level leaves the 16-row chunk
  of ``cdx_conv_wgrad_f32`` ragged; janner_h4: H = 4 / dim_mult [1, 4, 2], one sample; janner_b257: a conditional net at batch
  257 = 4 x 64 + 1 (GroupNorm backward takes four samples per workgroup), past the batch from which the device's ATen ``group_norm``
  backward is known to be wrong, so no same-device comparison covers it.
* chi_*: FiLM as (scale, shift) and as a shift; one case at batch 256.
* dit_*: head_dim 16 / 24 / 64, an odd token count (33), both limits of ``train._dit_fits`` (64 tokens, head_dim 64), a HalfDiT1d.
* chitf_*: the TransformerEncoder memory and the MLP one (Ta 10, To 2).
* idql_*: hidden 320 at batch 17 (one row past a chunk), a NewIDQLMlp; mlp_*: DQLMlp, DVInvMlp at batch 17.

The ``chain_forward`` towers are not here: tests/test_gpu_tower.py holds them against float64."""
import contextlib
import copy
import functools
from types import SimpleNamespace

import torch

import cleandiffuser_amd.nn_diffusion as N
from cleandiffuser_amd.engine import train
from cleandiffuser_amd.utils import load_synth

PARAM_FLOOR = 1e-3          # of the case's largest parameter-gradient magnitude
FACTOR = 4.0                # device tolerance = FACTOR x YARDSTICK[family]

# The largest E of the fp32 CPU run against float64 per family, rounded up to the next of 1, 1.5, 2, 3, ... 9 x 10^k (measured: the
# docstring of tests/test_train_graph_cases_cpu.py, which asserts them from both sides).
YARDSTICK = {
    "janner": 3e-6,
    "half_janner": 2e-6,
    "chi": 3e-6,
    "dit": 9e-7,
    "chitf": 1.5e-6,
    "idql": 1.5e-6,
    "mlp": 8e-7,
    "pearce": 8e-7,
    "sfbc": 1.5e-6,
}


def _half_janner(**kw):
    from cleandiffuser_amd.nn_classifier import HalfJannerUNet1d
    return HalfJannerUNet1d(16, 6, out_dim=1, kernel_size=3, model_dim=16, emb_dim=16, dim_mult=(1, 2, 2), **kw)


def _half_dit():
    from cleandiffuser_amd.nn_classifier import HalfDiT1d
    return HalfDiT1d(7, 1, emb_dim=32, d_model=64, n_heads=4, depth=1)


def _case(family, make, seed, x, t, cond=None):
    """`x` / `cond`: shapes; `t`: "int" (timesteps 0 .. 19, as floating point of the run's dtype) or "unit" (uniform in [0, 1))."""
    return SimpleNamespace(family=family, make=make, seed=seed, x=x, t=t, cond=cond)


CASES = {
    # ---- JannerUNet1d
    "janner_ragged": _case("janner", lambda: N.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], kernel_size=5), 3, (3, 8, 23), "int"),
    "janner_h4": _case("janner", lambda: N.JannerUNet1d(23, model_dim=32, emb_dim=32, dim_mult=[1, 4, 2], kernel_size=3), 4, (1, 4, 23), "int"),
    "janner_b257": _case("janner", lambda: N.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=5), 5, (257, 4, 6), "int", (257, 16)),
    # ---- ChiUNet1d with a global condition
    "chi_scale": _case("chi", lambda: N.ChiUNet1d(2, 5, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], cond_predict_scale=True), 6, (3, 8, 2), "int", (3, 2, 5)),
    "chi_shift": _case("chi", lambda: N.ChiUNet1d(3, 5, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], cond_predict_scale=False, kernel_size=3), 7,
                       (5, 4, 3), "int", (5, 2, 5)),
    "chi_b256": _case("chi", lambda: N.ChiUNet1d(2, 5, 2, model_dim=16, emb_dim=16, dim_mult=[1, 2], cond_predict_scale=True), 8, (256, 4, 2), "int", (256, 2, 5)),
    # ---- HalfJannerUNet1d (the classifier trunk)
    "half_janner_b5": _case("half_janner", _half_janner, 9, (5, 16, 6), "int"),
    "half_janner_b1": _case("half_janner", _half_janner, 10, (1, 16, 6), "int"),
    # ---- DiT1d / HalfDiT1d
    "dit_d64": _case("dit", lambda: N.DiT1d(7, emb_dim=32, d_model=64, n_heads=4, depth=2), 11, (3, 16, 7), "int", (3, 32)),
    "dit_d72_t33": _case("dit", lambda: N.DiT1d(5, emb_dim=32, d_model=72, n_heads=3, depth=2), 12, (2, 33, 5), "int", (2, 32)),
    "dit_limits": _case("dit", lambda: N.DiT1d(7, emb_dim=32, d_model=128, n_heads=2, depth=1), 13, (1, 64, 7), "int"),
    "half_dit": _case("dit", _half_dit, 14, (3, 8, 7), "int", (3, 32)),
    # ---- ChiTransformer
    "chitf_encoder": _case("chitf", lambda: N.ChiTransformer(3, 5, 6, 3, d_model=64, nhead=4, num_layers=2, p_drop_attn=0.0, n_cond_layers=2), 15,
                           (4, 6, 3), "int", (4, 3, 5)),
    "chitf_mlp": _case("chitf", lambda: N.ChiTransformer(3, 5, 10, 2, d_model=64, nhead=4, num_layers=1, p_drop_attn=0.0, n_cond_layers=0), 16,
                       (3, 10, 3), "int", (3, 2, 5)),
    # ---- IDQLMlp / NewIDQLMlp
    "idql_h64": _case("idql", lambda: N.IDQLMlp(11, 5, emb_dim=16, hidden_dim=64, n_blocks=2, dropout=0.0), 17, (6, 5), "unit", (6, 11)),
    "idql_h320_b17": _case("idql", lambda: N.IDQLMlp(11, 5, emb_dim=16, hidden_dim=320, n_blocks=2, dropout=0.0), 18, (17, 5), "unit", (17, 11)),
    "newidql_cond": _case("idql", lambda: N.NewIDQLMlp(11, 5, emb_dim=16, hidden_dim=64, n_blocks=1, dropout=0.0), 19, (4, 5), "unit", (4, 11)),
    # ---- DQLMlp / DVInvMlp
    "dql_b5": _case("mlp", lambda: N.DQLMlp(11, 6, emb_dim=16), 20, (5, 6), "int", (5, 11)),
    "dvinv_b17": _case("mlp", lambda: N.DVInvMlp(11, 6, emb_dim=16, hidden_dim=64), 21, (17, 6), "int", (17, 22)),
    # ---- PearceMlp, SfBCUNet
    "pearce_b7": _case("pearce", lambda: N.PearceMlp(6, To=2, emb_dim=32, hidden_dim=64), 22, (7, 6), "int", (7, 2, 32)),
    "sfbc_b6": _case("sfbc", lambda: N.SfBCUNet(5, emb_dim=16, hidden_dims=[64, 32, 16]), 23, (6, 5), "unit", (6, 16)),
}
TABLE = list(CASES)
FAMILY_CASES = {f.name: [n for n, c in CASES.items() if c.family == f.name] for f in train.FAMILIES}


def tolerance(name: str) -> float:
    return FACTOR * YARDSTICK[CASES[name].family]


# ------------------------------------------------------------------------------------------------------------------ #
def build(name: str) -> torch.nn.Module:
    """The case's net: fp32, on the CPU, in train() mode, no dropout anywhere."""
    case = CASES[name]
    net = load_synth(case.make(), case.seed).train()
    assert not [m for m in net.modules() if isinstance(m, torch.nn.Dropout) and m.p > 0.0], name
    assert not [m for m in net.modules() if isinstance(m, torch.nn.MultiheadAttention) and m.dropout > 0.0], name
    return net


def inputs(name: str) -> dict:
    """x, t, cond (or None) and wgt in float64 (`wgt` is drawn once the output's shape is known: ``reference``)."""
    case = CASES[name]
    g = torch.Generator().manual_seed(1000 + case.seed)
    x = torch.randn(case.x, generator=g, dtype=torch.float64)
    b = case.x[0]
    t = torch.randint(0, 20, (b,), generator=g).double() if case.t == "int" else torch.rand(b, generator=g, dtype=torch.float64)
    cond = None if case.cond is None else torch.randn(case.cond, generator=g, dtype=torch.float64)
    return {"x": x, "t": t, "cond": cond, "gen": g}


def cast(inp: dict, dtype, device="cpu"):
    """(x, t, cond, wgt) of a run in `dtype` on `device`; x is a fresh leaf that takes a gradient."""
    to = lambda v: None if v is None else v.detach().clone().to(dtype).to(device)      # noqa: E731
    return to(inp["x"]).requires_grad_(True), to(inp["t"]), to(inp["cond"]), to(inp.get("wgt"))


def head(net, y):
    """What the module does with its trunk's output: HalfDiT1d pools the tokens and projects them (its ``_forward_torch`` and its row of
    ``train.FAMILIES`` are the DiT1d trunk's)."""
    return net.proj(y.mean(1)) if type(net).__name__ == "HalfDiT1d" else y


def torch_forward(net, x, t, cond):
    return head(net, net._forward_torch(x, t, cond)) if hasattr(net, "_forward_torch") else net(x, t, cond)


def native_forward(net, x, t, cond):
    """The family's forward of engine/train.py, called directly (the CPU tier runs it on the stand-ins of tests/torch_blocks.py)."""
    fam = next(f for f in train.FAMILIES if f.belongs(type(net)))
    return head(net, getattr(train, fam.forward)(net, x, t, cond))


def objective(y, wgt):
    return (y * wgt).sum() / y.shape[0]


def grads_of(net) -> dict:
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in net.named_parameters()}


def _torch_run(net32, inp, dtype) -> dict:
    net = copy.deepcopy(net32).to(dtype).train()
    if hasattr(net, "pos_emb_cache"):
        net.pos_emb_cache = None                          # (a plain attribute: .to() does not convert it)
    x, t, cond, wgt = cast(inp, dtype)
    y = torch_forward(net, x, t, cond)
    assert y.dtype == dtype
    if wgt is None:
        inp["wgt"] = torch.randn(y.shape, generator=inp["gen"], dtype=torch.float64)
        wgt = inp["wgt"].to(dtype)
    objective(y, wgt).backward()
    return {"y": y.detach(), "dx": x.grad.detach(), "grads": grads_of(net)}


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """One float64 and one float32 CPU run of the module's own PyTorch forward per case and process.  Callers leave it unchanged."""
    net = build(name)
    inp = inputs(name)
    r64 = _torch_run(net, inp, torch.float64)
    r32 = _torch_run(net, inp, torch.float32)
    for r in (r64, r32):
        assert all(torch.isfinite(v).all() for v in [r["y"], r["dx"]] + [g for g in r["grads"].values() if g is not None]), name
    top = max(float(g.abs().max()) for g in r64["grads"].values() if g is not None)
    return SimpleNamespace(name=name, case=CASES[name], net=net, inp=inp, r64=r64, r32=r32, top=top)


def errors(ref, got: dict, times: float = 1.0) -> dict:
    """{tensor: E} of `got` (y, dx, grads) against `times` x the float64 run of `ref`.  A parameter without a gradient in the reference
    must have none (None, or a tensor nobody wrote: all zero) on the other side: E = inf otherwise."""
    r = ref.r64
    out = {}

    def rel(g, want, floor):
        return float((g.detach().double().cpu() - want).abs().max()) / max(float(want.abs().max()), floor)
    out["y"] = rel(got["y"], r["y"], 1.0)                 # (an output does not accumulate: 1 x whatever `times`)
    out["dx"] = rel(got["dx"], r["dx"] * times, 0.0)
    assert set(got["grads"]) == set(r["grads"])
    for n, want in r["grads"].items():
        g = got["grads"][n]
        if want is None:
            out[n] = 0.0 if g is None or float(g.abs().max()) == 0.0 else float("inf")
        elif g is None or g.shape != want.shape:
            out[n] = float("inf")
        else:
            out[n] = rel(g, want * times, PARAM_FLOOR * ref.top * times)
    return out


def worst(errs: dict):
    k = max(errs, key=lambda n: errs[n])
    return k, errs[k]


def below_floor(ref) -> list:
    """The parameters whose float64 gradient lies under the floor of the error measure."""
    return [n for n, g in ref.r64["grads"].items() if g is not None and float(g.abs().max()) < PARAM_FLOOR * ref.top]


@contextlib.contextmanager
def everything_is_on_the_device():
    """``is_cuda`` answers True for every tensor: what ``train.family_of`` asks of the input and the parameters, without a device."""
    had, old = "is_cuda" in vars(torch.Tensor), vars(torch.Tensor).get("is_cuda")
    torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        if had:
            torch.Tensor.is_cuda = old
        else:
            del torch.Tensor.is_cuda
