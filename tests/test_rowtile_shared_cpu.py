"""What the row-tile bindings share (engine/rowtile.py, ``energy.describe_classifier``, ``runtime.pack_steps``) without a GPU: one
description of QGPONNClassifier refuses the same malformed nets on the guided-sampling and on the training route, and the step records
the three requests hand to C carry what the kernels read."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cep_cases as cc  # noqa: E402
import energy_cases as ec  # noqa: E402
import rollout_cases as rc  # noqa: E402
import torch_blocks  # noqa: E402
from test_cep_cpu import routed as cep_routed  # noqa: E402,F401
from test_energy_cpu import routed as energy_routed  # noqa: E402,F401
from test_train_paths_cpu import _everything_is_on_the_device  # noqa: E402


class _MyLinear(nn.Linear):
    pass


def _relu_hidden(net):
    net.mlp.mlp[0][1] = nn.ReLU()


def _no_bias(net):
    old = net.mlp.mlp[1][0]
    net.mlp.mlp[1][0] = nn.Linear(old.in_features, old.out_features, bias=False)


def _no_bias_act_proj(net):
    net.act_proj = nn.Linear(net.act_proj.in_features, net.act_proj.out_features, bias=False)


def _head_of_two(net):
    net.mlp.mlp[-2] = nn.Linear(net.mlp.mlp[-2].in_features, 2)


def _wide_obs_proj(net):
    net.obs_proj = nn.Linear(net.obs_proj.in_features, net.obs_proj.out_features + 16)


def _subclassed_projection(net):
    net.act_proj.__class__ = _MyLinear


def _subclassed_hidden(net):
    net.mlp.mlp[0][0].__class__ = _MyLinear


def _tanh_output(net):
    net.mlp.mlp[-1] = nn.Tanh()


def _broken_chain(net):
    old = net.mlp.mlp[1][0]
    net.mlp.mlp[1][0] = nn.Linear(old.in_features + 16, old.out_features)


MALFORMED = [_relu_hidden, _no_bias, _no_bias_act_proj, _head_of_two, _wide_obs_proj, _subclassed_projection, _subclassed_hidden, _tanh_output,
             _broken_chain]
CEP_CASE = "k8_ragged"              # two hidden layers, as the classifier of the energy cases has


@pytest.mark.parametrize("spoil", [None] + MALFORMED, ids=lambda f: "intact" if f is None else f.__name__.strip("_"))
def test_both_routes_refuse_the_same_malformed_classifiers(spoil, energy_routed, cep_routed, amd_lib):  # noqa: F811
    """A QGPONNClassifier that is not SiLU hidden layers of plain biased nn.Linear on a chain of matching widths, an identity output and
    a head to one scalar: ``describe_classifier`` answers None, ``try_energy_guided`` answers None before it draws, ``try_cep_update``
    answers None before it writes.  The intact net is taken by both."""
    from cleandiffuser_amd.engine import cep, energy
    assert cep.describe is energy.describe_classifier
    # the guided sampling route
    case = ec._c()
    agent = ec.build(case, amd_lib)
    if spoil is not None:
        spoil(agent.classifier.model_ema)
    assert (energy.describe_classifier(agent.classifier.model_ema) is None) == (spoil is not None)
    took, draws, _, _ = energy_routed(agent, case)
    assert took == (spoil is None) and (took or draws == 0)
    # the training route
    clf = cc.build(cc.CASES[CEP_CASE], amd_lib)
    x, t, y = cc.tensors(cc.make_inputs(CEP_CASE))
    if spoil is None:
        assert cep_routed(clf, x, t, y)[0]
        return
    spoil(clf.model)
    assert cep.describe(clf.model) is None
    before = [p.detach().clone() for p in clf.model.parameters()]
    with torch_blocks.emulated(), _everything_is_on_the_device():
        assert cep.try_cep_update(clf, x, t, y, True) is None
    assert all(torch.equal(p.detach(), p0) and p.grad is None for p, p0 in zip(clf.model.parameters(), before))


def test_the_stricter_checks_refuse_nothing_that_ran(amd_lib):
    """The description checks two things the guided route did not check before: plain nn.Linear inside the mlp, and the in / out chain
    of its layers.  Neither refuses a net that route could serve: ``mlp_grad._mlp_layers`` never understood a subclassed Linear, and a
    chain of mismatched widths cannot run ``forward``."""
    from cleandiffuser_amd.engine import mlp_grad
    net = ec.build(ec._c(), amd_lib).classifier.model_ema
    _subclassed_hidden(net)
    assert mlp_grad._mlp_layers(net.mlp) is None
    net = ec.build(ec._c(), amd_lib).classifier.model_ema
    x, t, obs = torch.zeros(2, 3), torch.zeros(2), torch.zeros(2, 7)
    assert net(x, t, obs).shape == (2, 1)
    _broken_chain(net)
    with pytest.raises(RuntimeError):
        net(x, t, obs)


def test_the_description_serves_both_requests(amd_lib):
    """One description: the sizes and Linears of the training request, the detached parameters of the guided request, and the transposed
    operands only the guided kernel reads -- copies made when first asked for."""
    from cleandiffuser_amd.engine import cep, energy
    net = ec.build(ec._c(), amd_lib).classifier.model_ema
    d = energy.describe_classifier(net)
    assert (d.Ec, d.O, d.A, d.hidden) == (32, 7, 3, [48, 48]) and d.lins[:2] == [net.obs_proj, net.act_proj] and len(d.lins) == 5
    assert [p.data_ptr() for p in cep.weights_of(d)] == [t.data_ptr() for t in (d.obs_w, d.obs_b, d.act_w, d.act_b, d.w[0], d.b[0], d.w[1],
                                                                                  d.b[1], d.wo, d.bo)]
    assert "wt" not in vars(d) and "act_wt" not in vars(d)
    assert torch.equal(d.wt[0], d.w[0][:, 32:64].t()) and torch.equal(d.wt[1], d.w[1].t()) and torch.equal(d.act_wt, d.act_w.t())
    assert all(t.is_contiguous() for t in d.wt + [d.act_wt]) and d.wt is d.wt


# ------------------------------------------------------------------------------------------------------------------- #
def _expected(steps):
    """What the kernels read of every record (RowStep::of in csrc/cdx_rowtile.h), written out: kind, vsel, the draw's number among the
    stochastic steps or -1, alpha, sigma and k[0..3] as fp32."""
    rows, draws = [], 0
    for st in steps:
        rows.append((st.kind, st.vsel, draws if st.noise else -1, np.float32(st.alpha), np.float32(st.sigma),
                     tuple(np.float32(v) for v in st.k[:4])))
        draws += 1 if st.noise else 0
    return rows


def _read(arr, n):
    return [(arr[i].kind, arr[i].vsel, arr[i].noise_idx, np.float32(arr[i].alpha), np.float32(arr[i].sigma),
             tuple(np.float32(arr[i].k[j]) for j in range(4))) for i in range(n)]


def _plans():
    return [(f"rollout/{n}", rc.reference(n).plan) for n in rc.CASES] + [(f"energy/{n}", ec.reference(n).plan) for n in ec.TABLE]


def test_pack_steps_carries_what_the_row_tile_kernels_read():
    """``runtime.pack_steps`` -- which packs the records of all three requests, from a plan or from its list of steps -- against the
    expectation written out above, for every plan of tests/rollout_cases.py and tests/energy_cases.py (all admissible) and for a plan that
    mixes stochastic and deterministic steps; flags are 0 on every admissible record."""
    from cleandiffuser_amd.engine import rowtile, runtime
    plans = _plans()
    by_name = dict(plans)
    ddpm, ddim = by_name["rollout/dql_ddpm_eps"].steps, by_name["rollout/dql_ddim_eps"].steps
    assert all(st.noise for st in ddpm[:2]) and not any(st.noise for st in ddim)
    mixed = [ddpm[0], ddim[1], ddim[2], ddpm[1], ddim[3], ddpm[2]]
    assert [r[2] for r in _expected(mixed)] == [0, -1, -1, 1, -1, 2]
    kinds = set()
    for name, steps in [(n, p.steps) for n, p in plans] + [("mixed", mixed)]:
        assert rowtile.step_admissible(steps, 64), name
        want = _expected(steps)
        assert [r[2] for r in want] == rowtile.noise_index(steps), name
        arr = runtime.pack_steps(steps)
        assert len(arr) == len(steps) and _read(arr, len(steps)) == want, name
        assert all(arr[i].flags == 0 for i in range(len(steps))), name
        kinds |= {(st.kind, st.vsel, bool(st.noise)) for st in steps}
    for name, plan in plans:
        assert bytes(runtime.pack_steps(plan)) == bytes(runtime.pack_steps(plan.steps)), name
    assert {k for k, _, _ in kinds} == {0, 1, 2} and {v for _, v, _ in kinds} == {0, 1} and {z for _, _, z in kinds} == {True, False}


def test_step_admission_is_what_the_c_side_admits():
    """``step_admissible``: 1 .. max_steps records of kind 0-2 with vsel <= 1 and no flags (``ro_check_steps`` of csrc/cdx_rowtile.h)."""
    from types import SimpleNamespace
    from cleandiffuser_amd.engine import rowtile
    ok = SimpleNamespace(kind=2, vsel=1, flags=0)
    assert rowtile.step_admissible([ok], 64) and rowtile.step_admissible([ok] * 64, 64)
    assert not rowtile.step_admissible([], 64) and not rowtile.step_admissible([ok] * 65, 64)
    for bad in (dict(kind=3), dict(vsel=2), dict(flags=1)):
        assert not rowtile.step_admissible([ok, SimpleNamespace(**{**vars(ok), **bad})], 64), bad
