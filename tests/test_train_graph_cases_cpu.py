"""The table of tests/train_graph_cases.py, kept honest without a GPU.

* Every case is admitted by ``train.family_of`` under its family's name (with ``is_cuda`` made to answer True).
* The yardstick: E32 of every tensor of the fp32 CPU run of the module's PyTorch forward against the float64 one stays within
  ``YARDSTICK[family]``, and the family's largest E32 is more than half of it (the constant is the measured maximum rounded up, not a
  loose guess).  No case has more than 10 % of its parameter gradients under the 1e-3 floor of the error measure.
* The bar admits a correct implementation that is written differently: the native forward of engine/train.py in fp32, its kernel
  wrappers replaced by the torch expressions of tests/torch_blocks.py, stays within 4 x YARDSTICK of float64 on both gradient routes
  (autograd's accumulation, and straight into ``.grad`` through the queued weight-gradient batch).
* Resolving power: with ONE stand-in made subtly wrong, every affected case has a tensor beyond the device tolerance --
  GroupNorm backward without its ``xhat * mean(g * xhat)`` term, the weight-gradient product without the last of its batch x length
  rows, LayerNorm backward without ``mean(g)``.  The first and the third are explicit restatements of the backward formulas; with the
  term kept they pass (the control run of the same test), so the term alone is what is caught.

Measured (8 CPU threads; fp32 ATen sums in threads, the last digit moves from run to run).  Largest E32 per case, `y` / `dx` / worst
parameter gradient:

    janner_ragged   7.9e-7 / 9.9e-7 / 1.6e-6      janner_h4       7.5e-7 / 1.7e-6 / 2.7e-6      janner_b257    6.4e-7 / 1.0e-6 / 2.0e-6
    chi_scale       7.7e-7 / 5.1e-7 / 1.6e-6      chi_shift       4.5e-7 / 7.3e-7 / 2.5e-6      chi_b256       7.2e-7 / 8.7e-7 / 1.3e-6
    half_janner_b5  6.5e-7 / 9.3e-7 / 1.3e-6      half_janner_b1  9.4e-7 / 9.8e-7 / 1.6e-6
    dit_d64         3.8e-7 / 4.6e-7 / 6.4e-7      dit_d72_t33     3.5e-7 / 3.6e-7 / 8.7e-7      dit_limits     3.7e-7 / 2.8e-7 / 5.6e-7
    half_dit        2.4e-7 / 5.4e-7 / 6.3e-7      chitf_encoder   3.8e-7 / 4.8e-7 / 1.1e-6      chitf_mlp      3.9e-7 / 6.1e-7 / 6.7e-7
    idql_h64        2.2e-7 / 2.5e-7 / 8.0e-7      idql_h320_b17   6.9e-7 / 5.7e-7 / 1.1e-6      newidql_cond   1.4e-7 / 2.1e-7 / 6.8e-7
    dql_b5          8.8e-8 / 5.7e-7 / 7.1e-7      dvinv_b17       2.2e-7 / 3.8e-7 / 6.0e-7      pearce_b7      2.5e-7 / 3.2e-7 / 7.2e-7
    sfbc_b6         3.6e-7 / 4.4e-7 / 1.4e-6

Per family (maximum -> YARDSTICK): janner 2.7e-6 -> 3e-6, half_janner 1.6e-6 -> 2e-6, chi 2.5e-6 -> 3e-6, dit 8.7e-7 -> 9e-7, chitf
1.12e-6 -> 1.5e-6, idql 1.11e-6 -> 1.5e-6, mlp 7.1e-7 -> 8e-7, pearce 7.2e-7 -> 8e-7, sfbc 1.38e-6 -> 1.5e-6.  No parameter gradient
of any case lies under the floor.  The emulated native forward lies as far from float64 as fp32 autograd does, the same on both routes:
3.4e-7 (dql_b5) .. 3.0e-6 (chi_shift), a quarter of its tolerance at most.  The seeded faults, smallest error among the affected
cases: GroupNorm backward 1.05 (janner_h4: 88 000 x its tolerance), the weight gradient 2.6e-2 (half_dit: 7 200 x; chi_b256, one row of 1024: 1.3e-1),
LayerNorm backward 5.4e-2 (idql_h320_b17: 8 900 x); the restated GroupNorm / LayerNorm backward with the term kept: 3.0e-6 at most.
`pytest -s` prints every figure."""
import contextlib

import pytest
import torch

import torch_blocks as TB
import train_graph_cases as G
from cleandiffuser_amd.engine import blocks, train


@pytest.mark.parametrize("name", G.TABLE)
def test_case_is_admitted_under_its_familys_name(name):
    ref = G.reference(name)
    x, t, cond, _ = G.cast(ref.inp, torch.float32)
    with G.everything_is_on_the_device():
        fam = train.family_of(ref.net, x, cond)
    assert fam is not None and fam.name == ref.case.family
    assert set(G.FAMILY_CASES) == {f.name for f in train.FAMILIES} and all(G.FAMILY_CASES.values()), "a family without a case"


@pytest.mark.parametrize("name", G.TABLE)
def test_fp32_autograd_is_within_the_yardstick(name):
    ref = G.reference(name)
    e32 = G.errors(ref, ref.r32)
    k, w = G.worst({n: e for n, e in e32.items() if n not in ("y", "dx")})
    low = G.below_floor(ref)
    print(f"\n{name}: E32 y {e32['y']:.2e}  dx {e32['dx']:.2e}  worst parameter gradient {w:.2e} ({k}); "
          f"{len(low)} of {len(e32) - 2} parameter gradients under the floor; yardstick {G.YARDSTICK[ref.case.family]:.1e}")
    assert ref.r64["y"].dtype == torch.float64 and ref.r32["y"].dtype == torch.float32
    assert all(e <= G.YARDSTICK[ref.case.family] for e in e32.values()), G.worst(e32)
    assert len(low) <= 0.1 * (len(e32) - 2), low


@pytest.mark.parametrize("family", list(G.FAMILY_CASES))
def test_yardstick_is_the_measured_maximum_rounded_up(family):
    top = max(max(G.errors(G.reference(n), G.reference(n).r32).values()) for n in G.FAMILY_CASES[family])
    print(f"\n{family}: largest E32 {top:.3e}, YARDSTICK {G.YARDSTICK[family]:.1e}")
    assert 0.5 * G.YARDSTICK[family] < top <= G.YARDSTICK[family]


# ------------------------------------------------------------------------------------------------------------------ #
def _native_run(ref, in_place: bool) -> dict:
    """One forward + backward of the family's native forward on CPU tensors (call inside ``torch_blocks.emulated()``)."""
    net = ref.net
    net.zero_grad(set_to_none=True)
    if hasattr(net, "pos_emb_cache"):
        net.pos_emb_cache = None
    x, t, cond, wgt = G.cast(ref.inp, torch.float32)
    y = G.native_forward(net, x, t, cond)
    with (train.grads_in_place(list(net.parameters())) if in_place else contextlib.nullcontext()):
        G.objective(y, wgt).backward()
    assert not train._wgrad_queues
    got = {"y": y.detach(), "dx": x.grad.detach(), "grads": G.grads_of(net)}
    net.zero_grad(set_to_none=True)
    return got


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("name", G.TABLE)
def test_emulated_native_forward_is_within_the_device_tolerance(name, in_place):
    ref = G.reference(name)
    with TB.emulated():
        errs = G.errors(ref, _native_run(ref, in_place))
    k, w = G.worst(errs)
    print(f"\n{name} (in place {in_place}): largest error {w:.2e} ({k}), tolerance {G.tolerance(name):.1e}")
    assert w <= G.tolerance(name), (k, w)


# ------------------------------------------------------------------------------------------------------------------ #
# the seeded faults                                                                                                            #
# ------------------------------------------------------------------------------------------------------------------ #
def _groupnorm_backward(keep_term: bool):
    """``torch_blocks.groupnorm_backward`` restated term by term: dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), the means over
    a sample's group; `keep_term` False drops the last one."""
    def run(dy, x, gamma, beta, batch, length, groups, act="mish", eps=1e-5, out=None, param_grads=False, grads_out=None, possum_out=None):
        c = x.shape[1]
        x4 = x.reshape(batch, length, groups, c // groups)
        mean, var = x4.mean((1, 3), keepdim=True), x4.var((1, 3), unbiased=False, keepdim=True)
        rstd = (var + eps).rsqrt()
        xhat = (x4 - mean) * rstd
        z = xhat.reshape(batch * length, c) * gamma + beta
        dz = TB._vjp(TB.ACTS[act], (z,), dy)[0]
        dxh = (dz * gamma).reshape(x4.shape)
        dx = dxh - dxh.mean((1, 3), keepdim=True)
        if keep_term:
            dx = dx - xhat * (dxh * xhat).mean((1, 3), keepdim=True)
        dx = (rstd * dx).reshape(batch * length, c)
        if possum_out is not None:
            possum_out.copy_(dy.view(batch, length, -1).sum(1))
        if not param_grads:
            return dx
        dg, db = (dz * xhat.reshape(batch * length, c)).sum(0), dz.sum(0)
        if grads_out is not None:
            grads_out[0].add_(dg)
            grads_out[1].add_(db)
            return dx, None, None
        return dx, dg, db
    return {"groupnorm_backward": run}


def _layernorm_backward(keep_term: bool):
    """``torch_blocks.layernorm_backward`` restated: dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) over a row, dxhat = dy x gain
    (or x (1 + scale) of the row's sample); `keep_term` False drops mean(dxhat)."""
    def run(dy, x, gamma=None, scale=None, rows_per_mod=1, eps=1e-5, want_dyxhat=False):
        mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        rstd = (var + eps).rsqrt()
        xhat = (x - mean) * rstd
        dxh = dy
        if gamma is not None:
            dxh = dy * gamma
        elif scale is not None:
            dxh = (dy.view(-1, rows_per_mod, x.shape[1]) * (1 + scale[:, None])).reshape(x.shape)
        dx = dxh - xhat * (dxh * xhat).mean(1, keepdim=True)
        if keep_term:
            dx = dx - dxh.mean(1, keepdim=True)
        dx = rstd * dx
        return (dx, dy * xhat) if want_dyxhat else dx
    return {"layernorm_backward": run}


def _wgrad_without_the_last_row(keep_term: bool):
    """The weight-gradient product over all but the last of the batch x length rows of its first operand (the bias sums stay whole)."""
    def one(p, q, batch, l_p, l_q, taps, stride=1, pad=0, k_split=0, bias_grad=False, dw_out=None, db_out=None):
        short = p if keep_term else torch.cat([p[:-1], torch.zeros_like(p[-1:])], 0)
        dw, db = TB.conv_wgrad(short, q, batch, l_p, l_q, taps, stride, pad), p.sum(0)
        if dw_out is not None:
            dw_out.add_(dw.view(dw_out.shape))
            if bias_grad:
                db_out.add_(db)
            return (dw_out, db_out) if bias_grad else dw_out
        return (dw, db) if bias_grad else dw

    def batch_of(jobs):
        for p, q, batch, l_p, l_q, taps, stride, pad, dw, db in jobs:
            one(p, q, batch, l_p, l_q, taps, stride, pad, bias_grad=db is not None, dw_out=dw, db_out=db)
        return -(-len(jobs) // 32)
    return {"conv_wgrad": one, "conv_wgrad_batch": batch_of}


FAULTS = {
    "groupnorm_backward_without_the_xhat_term": (_groupnorm_backward, ("janner", "half_janner", "chi", "pearce")),
    "wgrad_without_the_last_row": (_wgrad_without_the_last_row, tuple(G.FAMILY_CASES)),
    "layernorm_backward_without_the_mean": (_layernorm_backward, ("dit", "chitf", "idql")),
}


@pytest.mark.parametrize("fault,name", [(f, n) for f, (_, fams) in FAULTS.items() for n in G.TABLE if G.CASES[n].family in fams])
def test_a_subtly_wrong_node_exceeds_the_device_tolerance(fault, name):
    ref = G.reference(name)
    worst = {}
    for keep_term in (True, False):
        with TB.emulated():
            called = []
            stand_ins = FAULTS[fault][0](keep_term)
            saved = {n: getattr(blocks, n) for n in stand_ins}
            for n, fn in stand_ins.items():
                setattr(blocks, n, lambda *a, _fn=fn, **k: (called.append(1), _fn(*a, **k))[1])
            try:
                worst[keep_term] = G.worst(G.errors(ref, _native_run(ref, in_place=True)))
            finally:
                for n, fn in saved.items():
                    setattr(blocks, n, fn)
        assert called, "the case never runs the node the fault sits in"
    tol = G.tolerance(name)
    print(f"\n{fault} / {name}: with the term {worst[True][1]:.2e}, without {worst[False][1]:.2e} ({worst[False][0]}) = "
          f"{worst[False][1] / tol:.0f} x the tolerance {tol:.1e}")
    assert worst[True][1] <= tol, "the restated node is not the stand-in"
    assert worst[False][1] > tol, "the fault passes: the bar or the case cannot tell"
