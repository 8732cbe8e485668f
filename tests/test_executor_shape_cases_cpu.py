"""The table of tests/executor_shape_cases.py, kept honest without a GPU.

* Every family has a case in each class of shapes its host path can get wrong (``REQUIRED``).  The classes are computed from the bound
  weight struct and ``bigbatch``'s own chunk rule, not from names: a case that stops reaching its class fails.
* Every served case binds to its family; every refusal -- one past a limit each -- makes ``bigbatch._binding`` answer None.
* The yardstick: E32(case) = max |x32 - x64| / max(1, max |x64|) of the fp32 CPU run (the stock module, or the host loop of a
  sample-mode case) against the float64 one on the same inputs.  No case exceeds its family's committed YARDSTICK, which
  tests/test_gpu_executor_shapes.py multiplies by 4.
* The float64 run ALONE can show the faults the sweep is for, by a factor of 100 over that tolerance: any two samples of a chunked case
  differ (a wrong `b0`), any two positions of a multi-token case differ (a wrong row period), the two halves of every classifier-free
  denoiser call differ, and so do the results with w_cfg = 1.3 and w_cfg = 1.

Measured (8 CPU threads), E32 per family, largest first -- DiT: ditref_pair 2.87e-6, dit_depth0_pair 1.78e-6, dit_d30_pair 1.29e-6,
dit_t65 1.13e-6, the rest 2.2e-7 .. 4.2e-7; ChiTransformer: chitf_pair 3.35e-6, chitf_enc2_pair 2.20e-6, the rest 8.9e-8 .. 5.5e-7;
PearceTransformer: refuse_ptf_to63 2.22e-6, ptf_te64 1.45e-6, ptf_pair 1.28e-6, ptf_to1 1.19e-6, ptf_s64 1.08e-6, the rest 8.5e-7 ..
8.7e-7; residual MLP: mlp_h33_pair 1.37e-6, mlp_new_h130 6.0e-7, mlp_h33 2.3e-7, mlp_nb0 1.7e-7.  YARDSTICK is each family's maximum
rounded up: 3e-6, 3.5e-6, 2.5e-6, 1.5e-6.  The smallest distances of the last point, as shares of the scale: two samples 0.11 (dit_t1),
two positions 0.09 (refuse_chitf_ta65; 0.12 among the served cases, chitf_limits), the halves 0.49 (ptf_pair), w_cfg 0.14
(dit_depth0_pair) -- against 100 x 4 x 3.5e-6 = 1.4e-3.  `pytest -s` prints every case's figures."""
import pytest
import torch

import executor_shape_cases as E

FACTOR = 100.0


@pytest.fixture(scope="module")
def bindings():
    return {name: E.binding(name) for name in E.TABLE}


def test_every_family_has_a_case_in_each_class():
    have = {fam: set() for fam in E.FAMILIES}
    for name in E.SERVED:
        got = E.classes(name)
        print(f"\n{name}: {sorted(got)}")
        have[E.CASES[name].family] |= got
    for fam in E.FAMILIES:
        assert E.REQUIRED[fam] - have[fam] == set(), f"{fam}: no case reaches {sorted(E.REQUIRED[fam] - have[fam])}"


def test_a_case_that_stops_reaching_its_class_is_noticed(monkeypatch):
    """dit_depth0_pair alone is depth 0 under a pair, dit_t65 alone has 65 tokens and head_dim 64: with one block, or 64 tokens of two heads,
    the classes are gone."""
    assert {"depth0_pair", "pair_last_chunk_of_one"} <= E.classes("dit_depth0_pair")
    assert {"token_limit", "head_dim_64"} <= E.classes("dit_t65")
    monkeypatch.setitem(E.CASES["dit_depth0_pair"].ctor, "depth", 1)
    assert "depth0_pair" not in E.classes("dit_depth0_pair")
    monkeypatch.setitem(E.CASES["dit_t65"].ctor, "n_heads", 2)
    monkeypatch.setattr(E.CASES["dit_t65"], "x_shape", (64, 5))
    assert not {"token_limit", "head_dim_64"} & E.classes("dit_t65")
    monkeypatch.setattr(E.CASES["dit_d30_pair"], "chunk", None)           # the default rule holds batch 5 in one chunk
    assert not {"uneven_chunks", "pair_last_chunk_of_one"} & E.classes("dit_d30_pair")


@pytest.mark.parametrize("name", E.SERVED)
def test_served_cases_bind_to_their_family(name, bindings):
    fam, bound, _ = bindings[name]
    assert fam is not None and fam.kind == E.CASES[name].family
    assert bound is not None, "the executor does not take this shape: move the case to the refusals, with the reason"


@pytest.mark.parametrize("name", E.REFUSALS)
def test_refusals_are_refused(name, bindings):
    fam, bound, _ = bindings[name]
    assert fam is not None and fam.kind == E.CASES[name].family, "the family is the one whose limit the case is past"
    assert bound is None and E.CASES[name].mode == "forward"


def test_the_table_is_what_its_docstring_states():
    """Modes, chunks and batches as the table's docstring states them."""
    chunked = {n for n in E.TABLE if E.CASES[n].chunk is not None}
    pairs = {n for n in E.TABLE if E.CASES[n].mode == "sample"}
    assert pairs == {"dit_depth0_pair", "dit_d30_pair", "ditref_pair", "chitf_enc2_pair", "chitf_pair", "ptf_pair", "mlp_h33_pair"}
    assert chunked == pairs | {"dit_d30", "dit_t65", "ditref_fwd", "chitf_d30", "chitf_enc2_fwd", "ptf_te15", "mlp_h33"}
    assert all(E.CASES[n].chunk == 2 and E.CASES[n].batch == 5 for n in chunked)
    assert all(E.CASES[n].cond_shape is not None for n in pairs)
    assert len(E.SERVED) == 24 and len(E.REFUSALS) == 5
    for a, b in (("dit_d30_pair", "dit_d30"), ("ditref_pair", "ditref_fwd"), ("chitf_enc2_pair", "chitf_enc2_fwd"), ("chitf_pair", "chitf_d30"),
                 ("ptf_pair", "ptf_to1"), ("mlp_h33_pair", "mlp_h33")):
        assert (E.CASES[a].cls, E.CASES[a].ctor) == (E.CASES[b].cls, E.CASES[b].ctor)


@pytest.mark.parametrize("name", E.TABLE)
def test_fp32_cpu_run_is_within_the_yardstick(name):
    r = E.reference(name)
    x32 = E.cpu_run(name, torch.float32).x
    assert x32.dtype == torch.float32 and r.x.dtype == torch.float64 and torch.isfinite(r.x).all()
    assert r.x.shape == (E.CASES[name].batch, *E.CASES[name].x_shape)
    e32 = float((x32.double() - r.x).abs().max()) / max(1.0, float(r.x.abs().max()))
    print(f"\n{name}: E32 {e32:.3e}  max|x64| {float(r.x.abs().max()):.3f}  (yardstick {E.YARDSTICK[E.CASES[name].family]:.1e})")
    assert e32 <= E.YARDSTICK[E.CASES[name].family]


def _closest(x, dim):
    """The smallest max-distance between two slices of x along `dim`."""
    rows = x.movedim(dim, 0).flatten(1)
    dist = (rows[:, None] - rows[None]).abs().amax(-1)
    return float(dist[~torch.eye(len(rows), dtype=torch.bool)].min())


@pytest.mark.parametrize("name", E.TABLE)
def test_float64_run_can_show_the_faults(name):
    c, r = E.CASES[name], E.reference(name)
    scale = max(1.0, float(r.x.abs().max()))
    bar = FACTOR * E.tolerance(name) * scale
    samples = _closest(r.x, 0)
    print(f"\n{name}: closest samples {samples / scale:.3e} of the scale {scale:.3f} (bar {bar / scale:.1e})")
    assert samples > bar, "two samples give the same output: a wrong b0 would not show"
    if len(c.x_shape) == 2 and c.x_shape[0] > 1:
        positions = _closest(r.x, 1)
        print(f"{name}: closest positions {positions / scale:.3e}")
        assert positions > bar, "two positions give the same output: a wrong row period would not show"
    if c.mode == "sample":
        assert len(r.plan.steps) == 2 and r.plan.n_noise == 0 and r.env == (0, 0, 1), "a two-step deterministic plan under cfg_mode 2"
        assert len(r.halves) == 2
        halves = min(float((cond - unc).abs().max()) for cond, unc in r.halves)
        w1 = float((E.cpu_run(name, torch.float64, w_cfg=1.0).x - r.x).abs().max())
        print(f"{name}: halves {halves / scale:.3e}, w_cfg 1.3 against 1 {w1 / scale:.3e}")
        assert halves > bar, "the conditional and the unconditional half agree: a swapped or missing half would not show"
        assert w1 > bar, "w_cfg has no visible effect"
    else:
        assert not r.halves
