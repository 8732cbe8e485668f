"""The table of tests/unet2_shape_cases.py, kept honest without a GPU.

* Forms pinned: every row exists in exactly the forms it lists, by ``runtime2``'s own rules on the compiler's answers, each within
  160 KiB of LDS for its trajectories per workgroup; every refusal makes the compiler raise ValueError with the listed message and
  ``runtime2.supported`` answer a reason.  A compiler change that moves a row fails here.
* Axes covered, computed from the table (``axes``): every value of ``REQUIRED``, every form in at least two rows, a narrow-slot row in
  the ordinary, the compact and the split programs.
* The twin: every (row, form) pair's program runs one denoiser forward through ``oracle.lane_sim2`` on NaN-poisoned LDS (split and
  grouped members in lockstep) and agrees with the fp32 module within the TOL of tests/test_program2_random_shapes.py.  This is the gate
  in front of the device: an address outside the LDS plan reads NaN here.  A row the twin cannot run is not in the table.
* The yardstick per family: E32(row) = max |x32 - x64| / max(1, max |x64|) of the fp32 CPU run (the stock module, or the host loop of a
  sample-mode row) against the float64 one.  No row exceeds its family's committed YARDSTICK and the family's largest is at least half
  of it, so the constant can neither be missed nor grow slack.
* The float64 run ALONE can show the faults the sweep is for, by a factor of 100 over the row's tolerance: any two samples differ (a wrong
  trajectory offset, a ragged last workgroup or group), any two positions (a wrong row period or conv offset), any two channels (a wrong
  GroupNorm partition or cut offset), the two halves of every classifier-free denoiser call, and w_cfg = 1.3 against 1.

Measured (8 CPU threads), E32 per family, largest first -- Janner forward: refuse_gn48 6.6e-7, refuse_lds 6.1e-7, refuse_k7 6.1e-7, w64_m4
5.6e-7, n8_m3 5.0e-7, the rest 2.7e-7 .. 4.9e-7; Janner sample: n8_l4_s 4.01e-6, w64_s 3.42e-6, w64_m4_s 3.20e-6, w32_l4_s 2.03e-6;
conditional pair: cond_pair 2.58e-6; ChiUNet forward: chi_to1 7.1e-7, chi_bias 6.1e-7; ChiUNet sample: chi_pair 3.07e-6.  YARDSTICK:
1e-6, 5.5e-6, 3.5e-6, 1e-6, 4e-6.  The smallest distances of the last point, as shares of the scale: two samples 0.35 (n8_m3), two
positions 0.083 (w16_d1), two channels 0.19 (n8_l1), the halves 0.53 and w_cfg 0.18 (cond_pair) -- against bars of 4e-4 .. 2.2e-3.  The twin against the fp32 module: 2.6e-7 .. 1.6e-6 over the 38 programs (the bar is 5e-5); the
whole file takes about two minutes, nearly all of it the twin.  `pytest -s` prints every row's figures and the smallest distances."""
import pytest
import torch

import unet2_shape_cases as U
from test_program2_random_shapes import TOL

FACTOR = 100.0


@pytest.fixture(scope="module")
def nets():
    return {name: U.build_net(name) for name in U.TABLE}


@pytest.mark.parametrize("name", U.TABLE)
def test_rows_exist_in_exactly_the_forms_they_list(name, nets):
    c, have = U.CASES[name], U.available(name, nets[name])
    print(f"\n{name}: " + ", ".join(f"{f} {p.lds_bytes(int(f[-1]) if '_t' in f else 1) / 1024:.1f} KiB" for f, p in have.items()))
    assert tuple(f for f in U.FORMS if f in have) == c.forms, "the compiler moved this row: update the table, keeping every form in two rows"
    for form, prog in have.items():
        t = int(form[-1]) if "_t" in form else 1
        assert prog.lds_bytes(t) <= U.LDS_LIMIT
        assert (prog.nw, bool(prog.compact)) == {"nw4": (4, False), "compact": (8, True)}.get(U.program_key(form), (8, False))
        assert prog.meta.get("split_k", 0) == (int(form[5:]) if form.startswith("split") else 0)
        assert prog.meta.get("group_k", 0) == (int(form[5:]) if form.startswith("group") else 0)
    assert c.forms == () or c.mode == "sample" or set(c.forms) <= set(U.ORDINARY), "a forward serves the ordinary forms only"


@pytest.mark.parametrize("name", U.REFUSALS)
def test_refusals_are_refused_with_a_value_error(name, nets):
    from cleandiffuser_amd.engine import program2 as P2, runtime2
    c = U.CASES[name]
    for nw in (4, 8):
        with pytest.raises(ValueError, match=c.refused):
            P2.compile_janner2(nets[name], c.H, nw=nw)
    with pytest.raises(ValueError, match=c.refused):
        P2.compile_janner2(nets[name], c.H, nw=8, compact=True)          # (the one-trajectory compact stand-in of a plan too large)
    why = runtime2.supported(nets[name], c.H)
    assert why is not None and c.refused in why
    assert c.mode == "forward" and c.forms == ()


def test_every_axis_and_form_is_covered():
    have, rows_of = set(), {f: [] for f in U.FORMS}
    for name in U.SERVED:
        got = U.axes(name)
        print(f"\n{name}: {sorted(got)}")
        have |= got
        for f in U.CASES[name].forms:
            rows_of[f].append(name)
    assert U.REQUIRED - have == set(), f"no row reaches {sorted(U.REQUIRED - have)}"
    for f, rows in rows_of.items():
        assert len(rows) >= 2, f"{f}: rows {rows}"
    narrow = [n for n in U.SERVED if any(a.startswith("narrow_slot") for a in U.axes(n))]
    for kind in (U.ORDINARY, U.COMPACT, U.SPLIT):
        assert any(set(kind) & set(U.CASES[n].forms) for n in narrow), f"no narrow-slot row in {kind}"
    assert 60 <= len(U.PAIRS) <= 90 and all(U.CASES[n].batch == U.B for n in U.SERVED)
    for model_dim in (32, 64):          # split and grouped forms at both widths, for each k
        wide = [n for n in U.SERVED if U.CASES[n].ctor["model_dim"] == model_dim]
        assert set(U.SPLIT + U.GROUP) <= {f for n in wide for f in U.CASES[n].forms}


def test_a_row_that_stops_reaching_its_axis_is_noticed(monkeypatch):
    assert {"narrow_slot_24", "mult_3"} <= U.axes("n8_m3") and "D_1" in U.axes("w16_d1")
    monkeypatch.setitem(U.CASES["n8_m3"].ctor, "dim_mult", [1, 2])
    assert not {"narrow_slot_24", "mult_3"} & U.axes("n8_m3")
    monkeypatch.setattr(U.CASES["w16_d1"], "D", 2)
    assert "D_1" not in U.axes("w16_d1")


@pytest.mark.parametrize("name,form", U.PAIRS)
def test_every_program_runs_on_the_poisoned_twin(name, form):
    err = U.twin_error(name, U.program_key(form))          # (one run per program: the t1 / t2 / t3 forms share it)
    print(f"\n{name} {form}: twin against the fp32 module {err:.3e}")
    assert err < TOL                                        # (NaN, an unwritten read, fails this too)


@pytest.fixture(scope="module")
def e32():
    out = {}
    for name in U.TABLE:
        r, x32 = U.reference(name), U.cpu_run(name, torch.float32).x
        assert x32.dtype == torch.float32 and r.x.dtype == torch.float64 and torch.isfinite(r.x).all()
        assert r.x.shape == (U.CASES[name].batch, U.CASES[name].H, U.CASES[name].D)
        out[name] = float((x32.double() - r.x).abs().max()) / max(1.0, float(r.x.abs().max()))
    return out


@pytest.mark.parametrize("name", U.TABLE)
def test_fp32_cpu_run_is_within_the_yardstick(name, e32):
    fam = U.CASES[name].family
    print(f"\n{name}: E32 {e32[name]:.3e}  max|x64| {float(U.reference(name).x.abs().max()):.3f}  (yardstick {U.YARDSTICK[fam]:.1e})")
    assert e32[name] <= U.YARDSTICK[fam]


@pytest.mark.parametrize("family", U.FAMILIES)
def test_the_yardstick_is_the_measured_one_within_a_factor_of_two(family, e32):
    worst = max(e32[n] for n in U.TABLE if U.CASES[n].family == family)
    print(f"\n{family}: largest E32 {worst:.3e}, YARDSTICK {U.YARDSTICK[family]:.1e}")
    assert U.YARDSTICK[family] / 2.0 <= worst <= U.YARDSTICK[family]


def _closest(x, dim):
    """The smallest max-distance between two slices of x along `dim`."""
    rows = x.movedim(dim, 0).flatten(1)
    dist = (rows[:, None] - rows[None]).abs().amax(-1)
    return float(dist[~torch.eye(len(rows), dtype=torch.bool)].min())


@pytest.mark.parametrize("name", U.TABLE)
def test_float64_run_can_show_the_faults(name):
    c, r = U.CASES[name], U.reference(name)
    scale = max(1.0, float(r.x.abs().max()))
    bar = FACTOR * U.tolerance(name) * scale
    gaps = {"samples": _closest(r.x, 0), "positions": _closest(r.x, 1)}
    if c.D > 1:
        gaps["channels"] = _closest(r.x, 2)
    if c.mode == "sample":
        assert len(r.plan.steps) == 2 and r.plan.n_noise == 0, "a two-step deterministic plan"
        assert r.env == (0, 0, int(c.cond_shape is not None))
    if c.mode == "sample" and c.cond_shape is not None:
        assert len(r.halves) == 2
        gaps["halves"] = min(float((cond - unc).abs().max()) for cond, unc in r.halves)
        gaps["w_cfg"] = float((U.cpu_run(name, torch.float64, w_cfg=1.0).x - r.x).abs().max())
    else:
        assert not r.halves
    print(f"\n{name}: " + ", ".join(f"{k} {v / scale:.3e}" for k, v in gaps.items()) + f" of the scale {scale:.3f} (bar {bar / scale:.1e})")
    for what, gap in gaps.items():
        assert gap > bar, f"two {what} of the float64 run agree to {gap / scale:.1e}: a fault there would not show"
