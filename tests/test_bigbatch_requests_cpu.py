"""What the GEMM-executor host path (engine/bigbatch.py behind engine/dispatch.py) marshals, pinned on CPU tensors.

Every family is driven end to end through the public ``dispatch.try_*`` entries -- ``agent.sample(...)`` and the stand-alone
``backbone.forward`` -- with the device-facing pieces stubbed: ``bigbatch._run`` records the request and zero-fills ``x_out``,
``bigbatch._time_features`` returns zeros, ``dispatch._on_gpu`` says yes, and the program-kernel entries (``runtime.fused_sample`` /
``runtime.backbone_forward``) only note that the request fell through to them.  The recorded requests must equal, exactly, the ones in
``bigbatch_requests_cpu.json``; regenerate that file with ``python tests/test_bigbatch_requests_cpu.py`` only when a request is MEANT to
change.
"""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases, extra_cases  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bigbatch_requests_cpu.json")
SCALARS = ("batch", "hd", "emb_dim", "cond_dim", "n_steps", "temb_per_sample", "predict_noise", "cfg_mode", "cfg_w", "chunk")
TENSORS = ("temb", "cond", "x_in", "prior", "fix_mask", "noise", "x_min", "x_max", "x_out")


class _Refused(Exception):
    """Raised by the try_* wrappers of the refusal tests: the PyTorch executor that follows a refusal is not under test there (in the
    other scenarios it runs, on the CPU, and its per-step backbone.forward calls are requests like any other)."""


@contextlib.contextmanager
def recording(stop_when_refused=False, **module_attrs):
    """The stubs.  -> log: one entry per bigbatch._run request, per fall-through to the program kernel and per try_* sampling entry
    (what it answered and how many draws it took from the noise feed)."""
    import __graft_entry__ as g
    from cleandiffuser_amd.engine import bigbatch, dispatch, runtime
    g.build_libcdx()
    lib, log, saved = bigbatch._lib(), [], []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def run(kind, bound, **k):
        rec = {"kind": kind, "steps_len": None if k["steps"] is None else len(k["steps"])}
        rec.update({n: (float(k[n]) if n == "cfg_w" else int(k[n])) for n in SCALARS})
        rec.update({n: None if k[n] is None else list(k[n].shape) for n in TENSORS})
        rec["struct"] = {n: getattr(bound.struct, n) for n, t in bound.struct._fields_ if t is ctypes.c_int32}
        size = getattr(lib, {"dit": "cdx_dit1d", "mlp": "cdx_resmlp"}.get(kind, "cdx_" + kind) + "_workspace_floats")
        for label, chunk in (("workspace_floats", rec["chunk"]), ("workspace_floats_chunk2", 2)):
            s = bigbatch.CdxSampling(**{n: rec[n] for n in SCALARS if n != "chunk"}, chunk=chunk)
            rec[label] = size(ctypes.byref(bound.struct), ctypes.byref(s))
        log.append(rec)
        k["x_out"].zero_()

    def entry(name):
        orig = getattr(dispatch, name)

        def wrapped(*a, **k):
            feed = next(v for v in list(a) + list(k.values()) if hasattr(v, "many") and hasattr(v, "like"))
            before = feed._pos
            out = orig(*a, **k)
            log.append({"entry": name, "served": out is not None, "draws": feed._pos - before})
            if out is None and stop_when_refused and name != "try_fused_raw":     # (after try_fused_raw comes try_fused_sample)
                raise _Refused(name)
            return out
        return wrapped

    def program_kernel(name):
        def stub(*a, **k):
            log.append({"fell_through_to": name})
            return None
        return stub

    try:
        patch(bigbatch, "_run", run)
        patch(bigbatch, "_time_features", lambda net, t, dev: torch.zeros(t.shape[0], net.time_mlp[2].out_features))
        patch(dispatch, "_on_gpu", lambda t: True)
        for name in ("fused_sample", "backbone_forward"):
            patch(runtime, name, program_kernel(name))
        for name in ("try_fused_sample", "try_fused_raw", "try_fused_edm", "try_fused_legacy_ddpm"):
            patch(dispatch, name, entry(name))
        for name, value in module_attrs.items():
            patch(bigbatch, name, value)
        old_env = os.environ.get("CDX_UNET2")
        os.environ["CDX_UNET2"] = "0"       # (the program kernel would otherwise keep every JannerUNet1d loop it supports)
        yield log
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
        os.environ.pop("CDX_UNET2", None) if old_env is None else os.environ.__setitem__("CDX_UNET2", old_env)


def _lib():
    return cases.lib_namespace("amd")


def _sample_and_forward(name, tweak=None, forward=True, **sample_overrides):
    """One cases.CASES case: the sampling loop, then the stand-alone forward with a timestep per sample."""
    agent, net = cases.build(_lib(), name)
    inp = cases.make_inputs(name)
    if tweak is not None:
        tweak(agent, net, inp)
    kw = {**cases.sample_kwargs(name, inp), **sample_overrides}
    kw = {k: v for k, v in kw.items() if v is not None}
    try:
        cases.sampler_of(agent, name)(torch.from_numpy(inp["prior"]), noise=list(inp["noise"]), **kw)
    except _Refused:
        pass
    if forward:
        with torch.no_grad():
            agent.model_ema["diffusion"](*cases.forward_probe(name, agent, inp))
    return agent.model_ema["diffusion"]


def _widen(agent, net, inp):
    """One more feature than the net has: the state's last dimension is wrong."""
    import numpy as np
    pad = [(0, 0)] * (inp["prior"].ndim - 1) + [(0, 1)]
    inp["prior"], inp["noise"] = np.pad(inp["prior"], pad), np.pad(inp["noise"], [(0, 0)] + pad)
    agent.x_min = agent.x_max = None                  # (bounds of the old width would be a refusal of their own)


def _per_sample_mask(agent, net, inp):
    agent.fix_mask = torch.zeros(inp["prior"].shape)


def _legacy_ddpm_over_dit():
    lib = _lib()
    _, net = cases.build(lib, "dit_ddim_cfg")
    agent = lib.DDPM(net, lib.IdentityCondition(dropout=0.0), diffusion_steps=10, device="cpu")
    agent.eval()
    inp = cases.make_inputs("dit_ddim_cfg")
    try:
        agent.sample(torch.from_numpy(inp["prior"]), n_samples=inp["prior"].shape[0], sample_steps=10, w_cfg=1.0,
                     condition_cfg=torch.from_numpy(inp["cond"]), noise=list(inp["noise"]) * 4)
    except _Refused:
        pass


FORCED = dict(UNET_GEMM_MIN_BATCH=1, UNET_GEMM_MIN_PARAMS=1, JANNER_GEMM_MIN_BATCH=1)
SCENARIOS = {}
for _n, _c in cases.CASES.items():
    if _c["net"][0] in cases.BIGBATCH_NETS or _c["net"][0] == "PearceTransformer":
        SCENARIOS[_n] = ({}, lambda n=_n: _sample_and_forward(n))
    elif _c["net"][0] == "ChiUNet1d":
        SCENARIOS[_n] = (FORCED, lambda n=_n: _sample_and_forward(n))
for _n in ("janner_cfg2_ddim", "janner_legacy_edm_heun", "janner_cm", "janner_tiny_cond_w1"):   # the last one: the executor declines, the program kernel is asked
    SCENARIOS[_n] = (FORCED, lambda n=_n: _sample_and_forward(n))
for _n in ("dit1ref", "chiunet_local_cond", "janner_attention_conditional"):
    SCENARIOS["extra_" + _n] = ({}, lambda n=_n: extra_cases.SCENARIOS[n](_lib(), "amd", "cpu"))

# requests the executors refuse: every one answers None with no draw taken from the noise feed
REFUSALS = {
    "wrong_last_dim_dit": ({}, lambda: _sample_and_forward("dit_ddim_cfg", _widen, forward=False)),
    "wrong_last_dim_mlp": ({}, lambda: _sample_and_forward("idql_obs_ddim_cfg", _widen, forward=False)),
    "wrong_last_dim_chitf": ({}, lambda: _sample_and_forward("chitransformer_ddim", _widen, forward=False)),
    "wrong_last_dim_pearcetf": ({}, lambda: _sample_and_forward("pearcetf_ddim", _widen, forward=False)),
    "wrong_last_dim_chiunet": (FORCED, lambda: _sample_and_forward("chiunet_cfg_w18_ddim", _widen, forward=False)),
    "pearcetf_train_mode": ({}, lambda: _sample_and_forward("pearcetf_ddim", lambda a, net, i: a.model_ema["diffusion"].train(), forward=False)),
    "chiunet_without_condition": (FORCED, lambda: _sample_and_forward("chiunet_cfg_w18_ddim", forward=False, condition_cfg=None, w_cfg=0.0)),
    "janner_condition_w12": (FORCED, lambda: _sample_and_forward("janner_tiny_cond_w2", forward=False, w_cfg=1.2)),
    "per_sample_fix_mask": ({}, lambda: _sample_and_forward("dit_cfg4_cfg2_dpmpp2m", _per_sample_mask, forward=False)),
    "legacy_ddpm_over_dit": ({}, _legacy_ddpm_over_dit),
}


def _record(table, name):
    attrs, drive = table[name]
    with recording(stop_when_refused=table is REFUSALS, **attrs) as log:
        out = drive()
    return log, out


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_marshalled_requests_are_unchanged(name, expected):
    log, _ = _record(SCENARIOS, name)
    assert any("kind" in rec for rec in log) or name == "janner_tiny_cond_w1", "the scenario never reached a GEMM executor"
    assert json.loads(json.dumps(log)) == expected[name]


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_draw_no_noise(name, expected):
    log, _ = _record(REFUSALS, name)
    assert not any("kind" in rec for rec in log), "a refused request reached bigbatch._run"
    entries = [rec for rec in log if "entry" in rec]
    assert entries and all(not rec["served"] and rec["draws"] == 0 for rec in entries)
    assert json.loads(json.dumps(log)) == expected["refusal_" + name]


def test_pearcetf_in_train_mode_is_refused_before_the_binding_cache():
    from cleandiffuser_amd.engine import bigbatch
    _, net = _record(REFUSALS, "pearcetf_train_mode")
    assert net not in bigbatch._cache
    with recording() as log, torch.no_grad():
        x = torch.zeros(5, 4)
        from cleandiffuser_amd.engine import dispatch
        assert dispatch.try_backbone_forward(net, x, torch.zeros(5, dtype=torch.long), torch.zeros(5, 2, 32)) is None
    assert log == [] and net not in bigbatch._cache


def test_step_records_on_host_and_device_are_the_same_bytes():
    """bytes(host_steps(plan)) and what steps_to_device uploads: one packing.  The host array keeps at least one record (the C loop
    takes its address), the device copy exactly len(plan.steps)."""
    from types import SimpleNamespace
    from cleandiffuser_amd.engine import bigbatch, runtime
    agent, _ = cases.build(_lib(), "newidql_ddpm")
    plans = []
    with recording() as log:
        from cleandiffuser_amd.engine import dispatch
        inner = dispatch.try_fused_sample

        def grab(solver, model, plan, *a, **k):
            plans.append(plan)
            return inner(solver, model, plan, *a, **k)
        dispatch.try_fused_sample = grab
        inp = cases.make_inputs("newidql_ddpm")
        agent.sample(torch.from_numpy(inp["prior"]), noise=list(inp["noise"]), **cases.sample_kwargs("newidql_ddpm", inp))
    plan = plans[0]
    assert plan.n_noise > 0 and log
    empty = SimpleNamespace(steps=[], n_noise=0)
    for p in (plan, empty):
        n = len(p.steps) * ctypes.sizeof(runtime.CdxStep)
        host = bigbatch.host_steps(p)
        assert len(host) == max(len(p.steps), 1)
        dev = runtime.steps_to_device(p, torch.device("cpu"))
        assert dev.dtype == torch.uint8 and dev.numel() == n
        assert bytes(host)[:n] == dev.numpy().tobytes()
    noisy = [r.noise_idx for r in bigbatch.host_steps(plan)[:len(plan.steps)] if r.noise_idx >= 0]
    assert noisy == list(range(plan.n_noise))


if __name__ == "__main__":
    out = {name: _record(SCENARIOS, name)[0] for name in sorted(SCENARIOS)}
    out.update({"refusal_" + name: _record(REFUSALS, name)[0] for name in sorted(REFUSALS)})
    with open(EXPECTED, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum('kind' in r for log in out.values() for r in log)} requests of {len(out)} scenarios")
