"""Candidate scoring and selection (engine/select.py, utils/selection.py) without a GPU: the torch restatements of the two kernels in
float64 against the pipelines' literal expressions on the stock modules, the public calls on the CPU, the routing decisions with the
C calls replaced by their restatements, the C layout of the ctypes mirrors, the LDS plan and the messages of the C side's validation."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_cases as sc  # noqa: E402

MODES = (("argmax", 1), ("sample", 1), ("topk_mean", 4), ("none", 1))


def _close(got, want, what, tol=1e-10):
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert err <= tol * max(float(want.abs().max()) if want.numel() else 1.0, 1.0), (what, err)


def _compare(q, want, what, tol=1e-10):
    _close(q.scores.view(q.S, q.K), want["scores"], what + " scores", tol)
    _close(q.value, want["value"], what + " value", tol)
    if q.weights is not None:
        _close(q.weights, want["weights"], what + " weights", tol)
    if want["index"] is not None:
        assert torch.equal(q.index.long().view(want["index"].shape), want["index"]), what + " index"
        _close(q.picked, want["picked"], what + " picked", tol)
    else:
        assert q.index is None and q.picked is None


@pytest.mark.parametrize("name", sc.TABLE)
def test_restatement_equals_the_pipelines_expressions_in_float64(name):
    """``reference_scores`` + ``reference_select`` in float64 against the pipelines' own lines on the stock modules, every mode at every
    temperature of the range: scores, weights, value to 1e-10, index equal, picked to 1e-10."""
    from cleandiffuser_amd.engine import select as E
    case = sc.CASES[name]
    critic = sc.build_critic(case, dtype=torch.float64)
    obs, cand, u = (None if t is None else t.double() for t in sc.make_inputs(case))
    for T in sc.TEMPERATURES:
        for mode, top_k in MODES:
            top_k = min(top_k, case.K)
            q = sc.request(E, case, critic, obs, cand, mode, T, top_k, u)
            E.reference_run(q)
            _compare(q, sc.pipeline_expression(critic, obs, cand, case.K, mode, T, top_k, u), f"{name} {mode} T={T}")


def test_idql_advantage_cancels():
    """IDQL re-weights with softmax((Q - V(obs)) T): V is one constant per state, so weights and draws are those of Q alone."""
    from cleandiffuser_amd.engine import select as E
    from cleandiffuser_amd.utils import V, load_synth
    case = sc.CASES["twinq_s2_k17"]
    critic = sc.build_critic(case, dtype=torch.float64)
    v_net = load_synth(V(case.O, hidden_dim=32), 3).double().requires_grad_(False)
    obs, cand, u = (t.double() for t in sc.make_inputs(case))
    want = sc.pipeline_expression(critic, obs, cand, case.K, "sample", 3.0, 1, u, v_net=v_net)
    q = sc.request(E, case, critic, obs, cand, "sample", 3.0, 1, u)
    E.reference_run(q)
    _close(q.weights, want["weights"], "weights")
    assert torch.equal(q.index[:, 0].long(), want["index"])
    _close(q.picked, want["picked"], "picked")


def test_ties_go_to_the_lowest_index_and_the_payload_may_be_strided():
    """Given scores with exact ties: argmax is the first maximum, the top 4 are taken "largest not yet taken, lowest index on ties",
    the payload is read through its row stride; the running sum's catch-all is the last index."""
    from cleandiffuser_amd.utils.selection import select_by_score
    t = sc.tie_case()
    payload = t.wide[:, t.cols]
    assert payload.stride(0) == 9 and not payload.is_contiguous()
    s2 = t.scores.view(t.S, t.K)
    sel = select_by_score(t.scores, payload, t.K, mode="topk_mean", top_k=t.top_k, want_weights=True)
    for s in range(t.S):
        order = sorted(range(t.K), key=lambda k: (-float(s2[s, k]), k))[:t.top_k]
        assert sel.index[s].tolist() == order
        _close(sel.picked[s], payload.view(t.S, t.K, -1)[s, order].mean(0), "picked", 1e-6)
    sel = select_by_score(t.scores, payload, t.K, mode="argmax")
    assert sel.index.tolist() == [int((s2[s] == s2[s].max()).nonzero()[0]) for s in range(t.S)] and sel.index.dtype == torch.int32
    assert (s2 == s2.max(1, keepdim=True).values).sum(1).max() > 1, "the case has tied maxima"
    sel = select_by_score(t.scores, payload, t.K, mode="sample", u=torch.tensor([0.0, 0.5, 0.99999994]))
    assert sel.index[0] == 0 and sel.index[2] == t.K - 1
    sel = select_by_score(t.scores, None, t.K, mode="none", temperature=2.0, want_weights=True)
    assert sel.picked is None and sel.index is None
    _close(sel.weights, torch.softmax(2.0 * s2, 1), "weights", 1e-6)
    _close(sel.value, (torch.softmax(2.0 * s2, 1) * s2).sum(1), "value", 1e-6)


@pytest.mark.parametrize("name", ["dql_s3_k16", "mlp_s2_k256", "mlp_noobs_s2_k40", "twinq_s2_k17"])
def test_select_candidates_on_the_cpu(name):
    """The public call on the CPU (float32, the restatement) against the pipelines' expression; a callable critic and a GELU tower take
    the module route and land on the same numbers; ``u=None`` draws from the generator."""
    from cleandiffuser_amd.utils.selection import Selection, select_candidates
    case = sc.CASES[name]
    critic = sc.build_critic(case)
    obs, cand, u = sc.make_inputs(case)
    for mode, top_k in MODES:
        top_k = min(top_k, case.K)
        want = sc.pipeline_expression(critic, obs, cand, case.K, mode, 2.0, top_k, u)
        sel = select_candidates(critic, obs, cand.view(case.S, case.K, case.A), case.K, mode=mode, temperature=2.0, top_k=top_k, u=u,
                                want_weights=True)
        assert isinstance(sel, Selection) and sel.scores.shape == (case.S, case.K)
        _close(sel.scores, want["scores"], "scores", 1e-5)
        _close(sel.weights, want["weights"], "weights", 1e-5)
        _close(sel.value, want["value"], "value", 1e-5)
        if mode != "none" and sc.decision_margin(want["scores"], mode, 2.0, top_k, u) > 1e-4:
            assert torch.equal(sel.index.long(), want["index"])
            _close(sel.picked, want["picked"], "picked", 1e-6)
    if case.O:
        def fn(o, a):
            return critic(o, a) if case.kind != "mlp" else critic(torch.cat([o, a], -1))
        if case.kind == "dql":
            fn = critic.q_min
        a = select_candidates(fn, obs, cand, case.K, mode="argmax")
        b = select_candidates(critic, obs, cand, case.K, mode="argmax")
        _close(a.scores, b.scores, "callable", 1e-6)
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    a = select_candidates(critic, obs, cand, case.K, mode="sample", generator=g1)
    b = select_candidates(critic, obs, cand, case.K, mode="sample", u=torch.rand(case.S, generator=g2))
    assert torch.equal(a.index, b.index) and torch.equal(a.picked, b.picked)


def test_limits_are_refused_in_python():
    from cleandiffuser_amd.utils.selection import select_by_score
    s = torch.zeros(2 * 1025)
    for kw in (dict(num_candidates=1025), dict(num_candidates=5, mode="topk_mean", top_k=6), dict(num_candidates=50, mode="topk_mean", top_k=17),
               dict(num_candidates=5, temperature=float("inf")), dict(num_candidates=5, mode="best")):
        with pytest.raises(ValueError):
            select_by_score(s, None, **kw)
    with pytest.raises(ValueError):
        select_by_score(s, torch.zeros(2 * 1025, 65), 5)


def _patch_to_cpu(monkeypatch, E, calls):
    def score_select(q):
        calls.append("score_select")
        E.reference_scores(q)
        if q.K <= 16:
            E.reference_select(q)

    def select(q):
        calls.append("select")
        E.reference_select(q)
    monkeypatch.setattr(E, "on_device", lambda *ts: True)
    monkeypatch.setattr(E, "native_score_select", score_select)
    monkeypatch.setattr(E, "native_select", select)
    monkeypatch.delenv("CDX_SELECT", raising=False)


def test_routing(monkeypatch):
    """With the C calls replaced by their restatements: one call for K <= 16, two for K > 16, one over given scores; a GELU tower and a
    callable run as modules and only the reduction is native; ``CDX_SELECT=0`` takes no native call and agrees."""
    from cleandiffuser_amd.engine import select as E
    from cleandiffuser_amd.utils.selection import select_by_score, select_candidates
    calls = []
    _patch_to_cpu(monkeypatch, E, calls)
    for name, want in (("dql_s3_k16", ["score_select"]), ("dql_s5_k5", ["score_select"]), ("twinq_s2_k17", ["score_select", "select"]),
                       ("mlp_s2_k256", ["score_select", "select"])):
        case = sc.CASES[name]
        critic = sc.build_critic(case)
        obs, cand, u = sc.make_inputs(case)
        del calls[:]
        a = select_candidates(critic, obs, cand, case.K, mode="sample", temperature=3.0, u=u, want_weights=True)
        assert calls == want, (name, calls)
        monkeypatch.setenv("CDX_SELECT", "0")
        b = select_candidates(critic, obs, cand, case.K, mode="sample", temperature=3.0, u=u, want_weights=True)
        monkeypatch.delenv("CDX_SELECT")
        assert calls == want
        _close(a.scores, b.scores, "scores", 1e-5)
        _close(a.weights, b.weights, "weights", 1e-5)
    case = sc.CASES["dql_s3_k16"]
    obs, cand, u = sc.make_inputs(case)
    gelu = nn.Sequential(nn.Linear(10, 32), nn.GELU(), nn.Linear(32, 1))
    wide = nn.Sequential(nn.Linear(10, 24), nn.Tanh(), nn.Linear(24, 1))
    for critic in (gelu, wide, lambda o, a: gelu(torch.cat([o, a], -1))):
        del calls[:]
        sel = select_candidates(critic, obs, cand, case.K, mode="argmax")
        assert calls == ["select"]
        rows = torch.cat([obs.repeat_interleave(case.K, 0), cand], -1)
        _close(sel.scores.reshape(-1, 1), (critic(rows) if isinstance(critic, nn.Module) else gelu(rows)).detach(), "module scores", 1e-6)
    del calls[:]
    select_by_score(torch.randn(3 * 64), torch.randn(3 * 64, 4), 64)
    assert calls == ["select"]


def _c_side():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import select as E
    return E, E._lib()


_c_request = sc.c_request


def test_select_validation_fails_loudly():
    """Every limit of csrc/cdx_select.hip is refused with CDX_EINVAL and a message before anything is launched (no GPU needed)."""
    E, lib = _c_side()
    err = lib.cdx_last_error
    assert lib.cdx_select_f32(None, None) == -1 and b"null request" in err()
    assert lib.cdx_score_select_f32(None, None) == -1 and b"null request" in err()
    assert lib.cdx_score_select_lds_bytes(None) == -1 and b"null request" in err()
    inf = float("inf")
    for change, word in ((dict(K=0), b"K must be"), (dict(K=1025), b"K must be"), (dict(S=-1), b"bad size: S"), (dict(S=1 << 30, K=4), b"S * K"),
                         (dict(mode=4), b"mode"), (dict(temperature=inf), b"temperature"), (dict(temperature=float("nan")), b"temperature"),
                         (dict(mode=3, top_k=0), b"top_k"), (dict(mode=3, top_k=17, K=50), b"top_k"), (dict(mode=3, top_k=6), b"top_k"),
                         (dict(mode=0, index=8), b"need a mode"), (dict(mode=1, picked=8, P=65, payload=8, payload_ld=65), b"P must be"),
                         (dict(mode=1, picked=8, P=0, payload=8), b"P must be"), (dict(mode=1, picked=8, P=4, payload_ld=3, payload=8), b"payload_ld"),
                         (dict(mode=1, picked=8, P=4, payload_ld=4), b"null pointer: payload"), (dict(mode=2), b"null pointer: u"),
                         (dict(mode=1), b"null pointer: scores")):
        kw = dict(S=4, K=5, temperature=1.0)
        kw.update(change)
        q = E.CdxSelect(**kw)
        assert lib.cdx_select_f32(ctypes.byref(q), None) == -1 and word in err(), (change, err())
        if word != b"null pointer: scores":                  # the same refusals in front of the critic
            g = _c_request(E)
            g.sel = q
            assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and word in err(), (change, err())
    assert lib.cdx_select_f32(ctypes.byref(E.CdxSelect(S=0, K=5, temperature=1.0)), None) == 0          # no states: not an error
    for change, word in ((dict(A=0), b"A must be"), (dict(A=65), b"A must be"), (dict(O=509, A=4), b"O + A"), (dict(O=-1), b"bad size: O"),
                         (dict(widths=(24, 1)), b"multiple of 16"), (dict(widths=(528, 1)), b"multiple of 16"), (dict(widths=(16, 2)), b"last width must be 1"),
                         (dict(widths=(16,) * 6 + (1,)), b"n_layers")):
        g = _c_request(E, **change)
        assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and word in err(), (change, err())
        assert lib.cdx_score_select_lds_bytes(ctypes.byref(g)) == -1
    for field, value, word in (("n_towers", 3, b"n_towers"), ("n_layers", 0, b"n_layers")):
        g = _c_request(E)
        setattr(g, field, value)
        assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and word in err()
    g = _c_request(E)
    g.act[0] = 2                                                                                         # GELU
    assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and b"activation" in err()
    g = _c_request(E)
    g.norm[0], g.eps[0] = 1, 0.0
    assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and b"eps" in err()
    g = _c_request(E)
    assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and b"obs must be given" in err()
    g.obs = 8
    assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and b"null pointer: cand" in err()
    g.cand = g.scores = 8
    assert lib.cdx_score_select_f32(ctypes.byref(g), None) == -1 and b"null pointer: weights" in err()
    assert lib.cdx_score_select_f32(ctypes.byref(_c_request(E, S=0)), None) == 0


def test_lds_plan_matches_the_c_side():
    """``select.lds_bytes`` (what the router checks) == ``cdx_score_select_lds_bytes`` (what the launch uses); the widest admissible critic
    stays under the bound the entry point checks."""
    from types import SimpleNamespace
    E, lib = _c_side()
    worst = 0
    for O, A, w, depth in ((0, 1, 16, 2), (7, 3, 32, 4), (17, 6, 256, 4), (448, 64, 512, 6), (500, 12, 48, 3)):
        widths = (w,) * (depth - 1) + (1,)
        got = lib.cdx_score_select_lds_bytes(ctypes.byref(_c_request(E, O=O, A=A, widths=widths)))
        assert got == E.lds_bytes(SimpleNamespace(K0=O + A, width=list(widths))), (O, A, widths, got)
        worst = max(worst, got)
    assert worst == 4 * (32 + 16 * 516 + 32 * 516) <= E.MAX_LDS


def test_select_mirrors_have_the_c_layout(tmp_path):
    """``CdxSelect`` / ``CdxScoreSelect`` == the structs of include/cdx.h (gcc sizeof / offsetof); the entries were purely additive: the
    header's ABI number is still 19."""
    from cleandiffuser_amd.engine import select as E
    mirrors = {"cdx_select": E.CdxSelect, "cdx_score_select": E.CdxScoreSelect}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "cdx.h"', 'int main(void){',
           'printf("%d\\n%d\\n%d\\n", CDX_ABI_VERSION, CDX_SELECT_MAX_K, CDX_SELECT_MAX_TOPK);',
           'printf("%d\\n%d\\n%d\\n%d\\n", CDX_SELECT_NONE, CDX_SELECT_ARGMAX, CDX_SELECT_SAMPLE, CDX_SELECT_TOPK_MEAN);']
    for cname, mirror in mirrors.items():
        src.append(f'printf("%zu\\n", sizeof({cname}));')
        src += [f'printf("%zu\\n", offsetof({cname}, {f[0]}));' for f in mirror._fields_]
    src += ['return 0;}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = iter(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert [int(next(out)) for _ in range(3)] == [19, E.MAX_K, E.MAX_TOPK]
    assert [int(next(out)) for _ in range(4)] == [E.MODES[m] for m in ("none", "argmax", "sample", "topk_mean")]
    for cname, mirror in mirrors.items():
        assert int(next(out)) == ctypes.sizeof(mirror), cname
        for f in mirror._fields_:
            assert getattr(mirror, f[0]).offset == int(next(out)), (cname, f[0])
