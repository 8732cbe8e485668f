"""What the native training path (cleandiffuser_amd/engine/train.py) launches and which nets it takes, pinned on CPU tensors.

Two tables in ``train_paths_cpu.json``, recorded from the commit named in its ``parent`` field and compared for equality:

* ``traces`` -- for every case of tests/test_train_nodes_cpu.py (its tiny shapes), the ordered calls of the kernel wrappers
  (``torch_blocks._NAMES``) of one forward plus one backward of ``(y * wgt).sum()`` under ``emulated()``: under plain autograd, inside
  ``grads_in_place()``, and inside it with ``CDX_TRAIN_WGRAD_BATCH=0``; the U-Net cases also inside ``grads_in_place()`` with each of
  ``CDX_TRAIN_FUSED_ADDS`` / ``CDX_TRAIN_CONV_PAIR`` / ``CDX_TRAIN_FILM_BATCH`` set to 0.  A call is its wrapper's name and the
  arguments that differ from the defaults of the REAL wrapper in engine/blocks.py (so an argument passed as its default and one left
  out are one launch), required ones by position: tensors as dtype, shape and -- unless contiguous -- strides, scalars and strings as
  they are, None as ``N``; no addresses, no values.
  The jobs of ``conv_wgrad_batch`` are listed one by one.  For the ``grads_in_place()`` mode the file keeps every distinct call once
  (``calls``) and a trace as the list of their indices; for the other modes, to stay a small fixture, the number of calls per wrapper
  and a SHA-256 of the trace's lines.
* ``eligibility`` -- for one small net per backbone class (``is_cuda`` made to answer True for the input and the parameters, as
  tests/test_advice_r4.py does), which family takes the call, or none, over grad mode x (input needs a gradient, net frozen) x input
  dtype x input rank x condition present x ``CDX_TRAIN_NATIVE``: one letter per combination, in ``itertools.product`` order of AXES.

The recorder uses only ``train.*_forward``, ``train.grads_in_place`` and ``torch_blocks.emulated``; the family comes from
``train.family_of`` where it exists and from the ``supports_*`` functions where those do.  Regenerate with
``python tests/test_train_paths_cpu.py --record <commit>`` only when a launch or a decision is MEANT to change.
"""
import contextlib
import hashlib
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cleandiffuser_amd.nn_diffusion as N  # noqa: E402
from cleandiffuser_amd.engine import blocks, train  # noqa: E402
import test_train_nodes_cpu as nodes  # noqa: E402
import torch_blocks  # noqa: E402

EXPECTED = os.path.join(HERE, "train_paths_cpu.json")
UNETS = ("janner", "janner_cond", "half_janner")
MODES = {"autograd": (False, {}), "in_place": (True, {}), "in_place_wgrad_batch_0": (True, {"CDX_TRAIN_WGRAD_BATCH": "0"})}
UNET_MODES = {f"in_place_{v[10:].lower()}_0": (True, {v: "0"}) for v in ("CDX_TRAIN_FUSED_ADDS", "CDX_TRAIN_CONV_PAIR", "CDX_TRAIN_FILM_BATCH")}
FULL = "in_place"         # the mode whose traces the file keeps call by call (the others: _digest -- the file stays a small fixture)
TRACES = [(c, m) for c in nodes.CASES for m in list(MODES) + (list(UNET_MODES) if c in UNETS else [])]


# ------------------------------------------------------------------------------------------------------------------ #
# (a) launch traces                                                                                                            #
# ------------------------------------------------------------------------------------------------------------------ #
def _show(v):
    if torch.is_tensor(v):
        strides = "" if v.is_contiguous() else ":" + ",".join(map(str, v.stride()))
        return f"{str(v.dtype)[6:].replace('float', 'f')}[{'x'.join(map(str, v.shape))}{strides}]"
    if v is None:
        return "N"
    if isinstance(v, (list, tuple)):
        return "(" + " ".join(_show(u) for u in v) + ")"
    if isinstance(v, (bool, int, float, str)):
        return repr(v)
    return str(v)                                          # (torch.device)


def _call(name, signature, a, k):
    bound = signature.bind(*a, **k)
    shown = []
    for n, v in bound.arguments.items():
        default = signature.parameters[n].default
        if default is inspect.Parameter.empty:
            shown.append(_show(v))                         # (a required argument: by position)
        elif not (type(v) is type(default) and v == default):
            shown.append(f"{n}={_show(v)}")
    return f"{name} " + " ".join(shown)


@contextlib.contextmanager
def _environ(**values):
    old = {n: os.environ.get(n) for n in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for n, v in old.items():
            os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)


def _digest(calls):
    """What the file keeps of a trace outside the FULL mode: calls per wrapper and a SHA-256 of the lines."""
    names = [c.split(" ", 1)[0] for c in calls]
    return {"calls": {n: names.count(n) for n in sorted(set(names))}, "sha256": hashlib.sha256("\n".join(calls).encode()).hexdigest()}


def trace(case, mode):
    """The calls, in order, of one forward + backward of `case` (a fresh net: nothing registered in its weight-layout table)."""
    in_place, env = {**MODES, **UNET_MODES}[mode]
    net, fwd, args = nodes._case(case)
    net.train()
    wgt = nodes._wgt(net, args, 1)
    log = []
    real = {n: inspect.signature(getattr(blocks, n)) for n in torch_blocks._NAMES}        # (before emulated() swaps them)

    def recorder(name, fn):
        def run(*a, **k):
            if name == "conv_wgrad_batch":
                log.append(f"conv_wgrad_batch {len(a[0])}")
                log.extend("conv_wgrad_batch.job " + " ".join(_show(v) for v in job) for job in a[0])
            else:
                log.append(_call(name, real[name], a, k))
            return fn(*a, **k)
        return run

    with _environ(**env), torch_blocks.emulated():
        stand_ins = {n: getattr(blocks, n) for n in torch_blocks._NAMES}
        for n, fn in stand_ins.items():
            setattr(blocks, n, recorder(n, fn))
        try:
            x = args[0].clone().requires_grad_(True)
            y = fwd(net, x, *args[1:])
            with (train.grads_in_place() if in_place else contextlib.nullcontext()):
                (y * wgt).sum().backward()
        finally:
            for n, fn in stand_ins.items():
                setattr(blocks, n, fn)
    return log


# ------------------------------------------------------------------------------------------------------------------ #
# (b) eligibility decisions                                                                                                    #
# ------------------------------------------------------------------------------------------------------------------ #
FAMILIES = ("janner", "half_janner", "chi", "idql", "dit", "chitf", "mlp", "pearce", "sfbc")
LETTERS = dict(zip(FAMILIES, "jhcidtmps"))
AXES = (("grad mode", (True, False)), ("input needs a gradient, net frozen", ((True, False), (True, True), (False, False), (False, True))),
        ("input dtype", (torch.float32, torch.float64)), ("input rank right", (True, False)), ("condition present", (True, False)),
        ("CDX_TRAIN_NATIVE", ("1", "0")))


def _nets():
    """name -> (net, x, condition): one small net per class the modules' forward() methods ask train about, and one that never does."""
    from cleandiffuser_amd.nn_classifier import HalfDiT1d, HalfJannerUNet1d
    r = torch.randn
    return {
        "JannerUNet1d": (N.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=3), r(2, 8, 6), r(2, 16)),
        "JannerUNet1d_model_dim_48": (N.JannerUNet1d(6, model_dim=48, emb_dim=16, dim_mult=[1, 2], kernel_size=5), r(2, 8, 6), r(2, 16)),
        "JannerUNet1d_attention": (N.JannerUNet1d(6, model_dim=16, emb_dim=16, dim_mult=[1, 2], kernel_size=3, attention=True), r(2, 8, 6), r(2, 16)),
        "HalfJannerUNet1d": (HalfJannerUNet1d(16, 6, out_dim=1, kernel_size=3, model_dim=16, emb_dim=16, dim_mult=(1, 2, 2)), r(2, 16, 6), r(2, 16)),
        "HalfJannerUNet1d_odd_halving": (HalfJannerUNet1d(12, 6, out_dim=1, kernel_size=3, model_dim=16, emb_dim=16, dim_mult=(1, 2, 2)), r(2, 12, 6), r(2, 16)),
        "ChiUNet1d_global_cond": (N.ChiUNet1d(2, 5, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2], obs_as_global_cond=True), r(2, 8, 2), r(2, 2, 5)),
        "ChiUNet1d_local_cond": (N.ChiUNet1d(2, 5, 8, model_dim=32, emb_dim=32, dim_mult=[1, 2], obs_as_global_cond=False), r(2, 8, 2), r(2, 8, 5)),
        "DiT1d": (N.DiT1d(7, emb_dim=32, d_model=64, n_heads=4, depth=1), r(2, 8, 7), r(2, 32)),
        "HalfDiT1d": (HalfDiT1d(7, 1, emb_dim=32, d_model=64, n_heads=4, depth=1), r(2, 8, 7), r(2, 32)),
        "DiT1Ref": (N.DiT1Ref(7, emb_dim=32, d_model=64, n_heads=4, depth=1), r(2, 8, 14), r(2, 32)),
        "IDQLMlp": (N.IDQLMlp(11, 5, emb_dim=16, hidden_dim=64, n_blocks=1), r(3, 5), r(3, 11)),
        "NewIDQLMlp": (N.NewIDQLMlp(11, 5, emb_dim=16, hidden_dim=64, n_blocks=1), r(3, 5), r(3, 11)),
        "DQLMlp": (N.DQLMlp(11, 6, emb_dim=16), r(3, 6), r(3, 11)),
        "DVInvMlp": (N.DVInvMlp(11, 6, emb_dim=16, hidden_dim=64), r(3, 6), r(3, 22)),
        "PearceMlp": (N.PearceMlp(6, To=2, emb_dim=32, hidden_dim=64), r(3, 6), r(3, 2, 32)),
        "SfBCUNet": (N.SfBCUNet(5, emb_dim=16, hidden_dims=[64, 32, 16]), r(3, 5), r(3, 16)),
        "ChiTransformer_encoder_layers": (N.ChiTransformer(3, 5, 6, 3, d_model=64, nhead=4, num_layers=1, n_cond_layers=1), r(2, 6, 3), r(2, 3, 5)),
        "ChiTransformer_encoder_mlp": (N.ChiTransformer(3, 5, 6, 3, d_model=64, nhead=4, num_layers=1, n_cond_layers=0), r(2, 6, 3), r(2, 3, 5)),
        "unrelated_module": (torch.nn.Sequential(torch.nn.Linear(5, 5)), r(3, 5), r(3, 5)),
    }


@contextlib.contextmanager
def _everything_is_on_the_device():
    had = "is_cuda" in vars(torch.Tensor)
    old = vars(torch.Tensor).get("is_cuda")
    torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        if had:
            torch.Tensor.is_cuda = old
        else:
            del torch.Tensor.is_cuda


def family(net, x, condition):
    """The name of the family that takes ``net(x, noise, condition)``, or None -- from whichever form this tree has."""
    if hasattr(train, "family_of"):
        row = train.family_of(net, x, condition)
        return None if row is None else row.name
    fns = [train.supports] + [getattr(train, "supports_" + f) for f in FAMILIES[1:]]
    took = [f for f, fn in zip(FAMILIES, fns) if fn(net, x, condition)]
    assert len(took) <= 1, (type(net).__name__, took)
    return took[0] if took else None


def decisions(net, x, condition):
    out = []
    for grad, (x_grad, frozen), dtype, rank_ok, has_cond, native in itertools.product(*(values for _, values in AXES)):
        xx = x.to(dtype)
        xx = (xx if rank_ok else xx.unsqueeze(0)).requires_grad_(x_grad)
        net.requires_grad_(not frozen)
        with _environ(CDX_TRAIN_NATIVE=native), torch.set_grad_enabled(grad), _everything_is_on_the_device():
            took = family(net, xx, condition if has_cond else None)
        out.append("-" if took is None else LETTERS[took])
    net.requires_grad_(True)
    return "".join(out)


# ------------------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


@pytest.mark.parametrize("case,mode", TRACES)
def test_the_launches_of_a_training_pass_are_unchanged(case, mode, expected):
    want, got = expected["traces"][f"{case}/{mode}"], trace(case, mode)
    if isinstance(want, dict):
        assert _digest(got) == want
        return
    want = [expected["calls"][i] for i in want]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"{case}/{mode}: call {i} differs\n  recorded: {w}\n  now:      {g}")
            break
    else:
        if len(got) != len(want):
            i = min(len(got), len(want))
            print(f"{case}/{mode}: {len(got)} calls now, {len(want)} recorded; first one without a partner: {(got + want)[i] if len(got) < len(want) else got[i]}")
    assert got == want


@pytest.fixture(scope="module")
def nets():
    torch.manual_seed(0)
    return _nets()


@pytest.mark.parametrize("name", ["JannerUNet1d", "JannerUNet1d_model_dim_48", "JannerUNet1d_attention", "HalfJannerUNet1d", "HalfJannerUNet1d_odd_halving",
                                  "ChiUNet1d_global_cond", "ChiUNet1d_local_cond", "DiT1d", "HalfDiT1d", "DiT1Ref", "IDQLMlp", "NewIDQLMlp", "DQLMlp",
                                  "DVInvMlp", "PearceMlp", "SfBCUNet", "ChiTransformer_encoder_layers", "ChiTransformer_encoder_mlp", "unrelated_module"])
def test_the_family_that_takes_a_call_is_unchanged(name, nets, expected):
    assert set(nets) == set(expected["eligibility"])
    got, want = decisions(*nets[name]), expected["eligibility"][name]
    combos = list(itertools.product(*(values for _, values in AXES)))
    assert len(got) == len(want) == len(combos)
    for g, w, combo in zip(got, want, combos):
        if g != w:
            print(f"{name}: {dict(zip((a for a, _ in AXES), combo))}: recorded {w!r}, now {g!r} (letters: {LETTERS}, '-': none)")
            break
    assert got == want


def record(parent):
    calls, traces = {}, {}
    for case, mode in TRACES:
        got = trace(case, mode)
        traces[f"{case}/{mode}"] = [calls.setdefault(c, len(calls)) for c in got] if mode == FULL else _digest(got)
    torch.manual_seed(0)
    eligibility = {n: decisions(*v) for n, v in _nets().items()}
    rows = lambda d: "{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "\n }"      # noqa: E731
    with open(EXPECTED, "w") as f:                         # (one call, one trace, one net per line)
        f.write("{\n \"parent\": " + json.dumps(parent) + ",\n \"calls\": [\n" + ",\n".join("  " + json.dumps(c) for c in calls) + "\n ],\n"
                " \"traces\": " + rows(traces) + ",\n \"eligibility\": " + rows(eligibility) + "\n}\n")
    print(f"recorded {len(traces)} traces ({sum(map(len, traces.values()))} calls, {len(calls)} distinct) and {len(eligibility)} nets: {os.path.getsize(EXPECTED)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_train_paths_cpu.py --record <commit the fixture is recorded from>")
    record(sys.argv[2])
