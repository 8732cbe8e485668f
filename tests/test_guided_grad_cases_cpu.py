"""The pinned table of tests/guided_grad_cases.py on the CPU: every row compiles to exactly the program forms it names (so a compiler
change that moves a row fails HERE instead of thinning the GPU coverage), the table covers the shapes it promises, and the constants
the GPU bars are built from -- the distance of torch's fp32 autograd from the float64 reference -- are what the table says."""
import pytest
import torch

import guided_grad_cases as G
from cleandiffuser_amd.engine import runtime2

LDS_MAX = 160 * 1024


def test_table_covers_the_promised_shapes():
    rows = G.ROWS.values()
    assert 10 <= len(G.ROWS) <= 16
    for form in G.FORMS:
        assert sum(form in r.forms for r in rows) >= 2, form
    ds, hs = {r.D for r in rows}, {r.H for r in rows}
    assert 1 in ds and any(d % 4 for d in ds) and any(d > 32 for d in ds)
    assert {4, 8, 64} <= hs
    assert {8, 64} <= {r.den[0] for r in rows}
    assert {3, 5} <= {r.clf[2] for r in rows} and any(4 in r.clf[1] for r in rows)
    assert {0, G.T_MAX} <= {r.t for r in rows}
    cfg2 = G.ROWS["cfg2"]
    assert (cfg2.den, cfg2.clf, cfg2.H, cfg2.D, cfg2.seeds) == ((32, (1, 2, 2, 2), 5), (32, (1, 2, 2, 2), 3), 32, 23, (0, 1))
    assert set(G.ROWS["cfg2"].forms) == {"lds", "two", "three"}


@pytest.mark.parametrize("name", list(G.ROWS))
def test_rows_compile_to_the_forms_they_name(name, amd_lib):
    row = G.ROWS[name]
    net, clf = G.build(name, amd_lib)
    got = {}
    for key, two, three in (("t1", False, False), ("two", True, False), ("three", False, True)):
        try:
            prog = runtime2._compile_guided2(net, clf, row.H, two, three)
        except ValueError:
            continue
        got[G.form_of(prog) if key == "t1" else key] = prog
    assert set(got) == set(row.forms), (name, sorted(got))
    for form, prog in got.items():
        assert prog.lds_bytes(G.T_OF[form]) <= LDS_MAX, (name, form)
        assert (prog.ws_floats > 0) == (form != "lds"), (name, form)
        assert bool(prog.compact) == (form in ("ws_compact", "three")), (name, form)
        assert prog.grad_off >= 0 and (prog.horizon, prog.dim) == (row.H, row.D)
    # the forms the row does not name: refused with the compiler's ValueError (the loop above let nothing else through), and a
    # one-trajectory program always exists
    assert len(set(row.forms) & {"lds", "ws", "ws_compact"}) == 1


def test_gradient_entry_returns_none_for_a_program_that_does_not_exist(amd_lib):
    """`runtime2.classifier_gradient2(..., form=)`: None -- before anything is launched -- when the requested program does not exist."""
    name = "md8_h64_d31"                                   # lds and two, no three
    net, clf = G.build(name, amd_lib)
    x, t = G.reference(name).x[:2], G.reference(name).t[:2]
    assert runtime2.compiled_guided2(net, clf, 64, two=True).prog is not None
    assert runtime2.classifier_gradient2(net, clf, x, t, form="three") is None
    with pytest.raises(ValueError, match="unknown program form"):
        runtime2.classifier_gradient2(net, clf, x, t, form="ws")


@pytest.fixture(scope="module")
def measured(amd_lib):
    """Per row (fp32 CPU autograd - float64 reference) in the max norm, relative to the reference's largest element."""
    out = {}
    for name in G.ROWS:
        ref = G.reference(name)
        _, clf = G.build(name, amd_lib)
        logp, grad = G.autograd(clf, ref.x, ref.t)
        assert logp.dtype == grad.dtype == torch.float32
        out[name] = (float((grad.double() - ref.grad).abs().max() / ref.grad.abs().max()),
                     float((logp.double() - ref.logp).abs().max() / ref.logp.abs().max()))
    return out


def test_fp32_autograd_distance_from_float64_is_the_stored_constant(measured):
    for name, (eg, el) in measured.items():
        print(f"{name:14s} E_grad {eg:.3e}  E_logp {el:.3e}")
    e_grad, e_logp = max(v[0] for v in measured.values()), max(v[1] for v in measured.values())
    print(f"E_GRAD {e_grad:.3e} (stored {G.E_GRAD:.3e})  E_LOGP {e_logp:.3e} (stored {G.E_LOGP:.3e})")
    assert e_grad < 1e-5 and e_logp < 1e-5
    assert G.E_GRAD / 2 <= e_grad <= 2 * G.E_GRAD
    assert G.E_LOGP / 2 <= e_logp <= 2 * G.E_LOGP


def test_reference_is_float64_and_per_sample(amd_lib):
    """The reference really ran in float64 (timestep embedding included), and a sample's gradient does not depend on its batch."""
    ref = G.reference("md8_h8_d1")
    with G.float64_default():
        _, clf = G.build("md8_h8_d1", amd_lib)
        clf = clf.double()
        assert clf.map_noise(ref.t).dtype == torch.float64
        logp, grad = G.autograd(clf, ref.x[2:3].double(), ref.t[2:3])
    assert grad.dtype == torch.float64
    torch.testing.assert_close(grad, ref.grad[2:3], rtol=0, atol=1e-13 * float(ref.grad.abs().max()))
    torch.testing.assert_close(logp, ref.logp[2:3], rtol=0, atol=1e-13 * float(ref.logp.abs().max()))
    each = G.reference("md8_h8_d1", per_sample=True)
    assert {0, G.T_MAX} <= set(each.t.tolist()) and torch.equal(each.x, ref.x)
