"""Candidate scoring and selection on the MI355X (csrc/cdx_select.hip behind engine/select.py and utils/selection.py): the critic's
scores and the reduction against the float64 restatements, the public call against the pipelines' expression on the stock route, the
launch structure, reproducibility, the ``CDX_SELECT=0`` route."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = (("argmax", 1), ("sample", 1), ("topk_mean", 4))


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    for var in ("CDX_SELECT", "CDX_TOWER", "CDX_TRAIN_NATIVE"):
        monkeypatch.delenv(var, raising=False)


def _spy(monkeypatch):
    """The names of the native calls that ran."""
    from cleandiffuser_amd.engine import select as E
    seen = []
    for name in ("native_score_select", "native_select"):
        def spy(q, real=getattr(E, name), name=name):
            real(q)
            seen.append(name)
        monkeypatch.setattr(E, name, spy)
    return seen


def _on_device(case):
    critic = sc.build_critic(case, device=DEV)
    obs, cand, u = (None if t is None else t.to(DEV) for t in sc.make_inputs(case))
    return critic, obs, cand, u


def _float64_scores(E, case):
    """The float64 restatement of the critic on the CPU -> (S, K)."""
    critic = sc.build_critic(case, dtype=torch.float64)
    obs, cand, _ = (None if t is None else t.double() for t in sc.make_inputs(case))
    q = sc.request(E, case, critic, obs, cand, "none", 1.0)
    E.reference_scores(q)
    return q.scores.view(case.S, case.K)


def _assert_close(got, want, tol, what):
    a, b = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
    print(f"  {what}: max|d| {float(np.abs(a - b).max()) if a.size else 0.0:.3e}  max|ref| {float(np.abs(b).max()) if b.size else 0.0:.3e}")
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol, err_msg=what)


@pytest.mark.parametrize("name", sc.TABLE)
def test_scores_match_the_float64_restatement(name):
    """``cdx_score_select_f32``'s scores against the float64 restatement at rtol = atol = 1e-4 (the bar of tests/test_gpu_tower.py)."""
    from cleandiffuser_amd.engine import select as E
    case = sc.CASES[name]
    critic, obs, cand, u = _on_device(case)
    q = sc.request(E, case, critic, obs, cand, "none", 1.0)
    E.native_score_select(q)
    torch.cuda.synchronize()
    _assert_close(q.scores.view(case.S, case.K), _float64_scores(E, case), 1e-4, f"{name} scores")


def _check_reduction(E, got, what, payload64):
    """A served request against the float64 restatement over the kernel's OWN fp32 scores (so the scores' error times the temperature
    does not enter): weights and value at 1e-4, picked at 1e-5, index exactly -- in "sample" mode after asserting that no float64
    running sum of any state comes within 1e-4 of its uniform."""
    scores = got.scores.detach().cpu().double()
    u = None if got.u is None else got.u.cpu().double()
    want = E.make_request(got.S, got.K, got.mode, got.temperature, got.top_k, u, scores=scores, payload=payload64,
                          want_weights=got.weights is not None)
    E.reference_select(want)
    if got.mode == "sample":
        margin = sc.sample_margin(scores.view(got.S, got.K), got.temperature, u)
        print(f"  {what}: the running sums stay {margin:.3e} away from u")
        assert margin >= 1e-4, (what, margin)
    if got.weights is not None:
        _assert_close(got.weights, want.weights, 1e-4, what + " weights")
    _assert_close(got.value, want.value, 1e-4, what + " value")
    if got.mode != "none":
        assert torch.equal(got.index.cpu(), want.index), (what, got.index.cpu(), want.index)
        _assert_close(got.picked, want.picked, 1e-5, what + " picked")


@pytest.mark.parametrize("temperature", sc.TEMPERATURES)
@pytest.mark.parametrize("name", sc.TABLE)
def test_reduction_matches_float64_on_the_kernels_own_scores(name, temperature):
    """Every mode of every case at temperatures 1, 20 and 300 through the launches ``run`` issues (the one-launch path for K <= 16,
    ``cdx_select_f32`` behind the critic for K > 16)."""
    from cleandiffuser_amd.engine import select as E
    case = sc.CASES[name]
    critic, obs, cand, u = _on_device(case)
    for mode, top_k in MODES + (("none", 1),):
        q = sc.request(E, case, critic, obs, cand, mode, temperature, min(top_k, case.K), u if mode == "sample" else None)
        assert E.run(q) == (1 if case.K <= 16 else 2)
        torch.cuda.synchronize()
        _check_reduction(E, q, f"{name} {mode} T={temperature}", cand.cpu().double())


@pytest.mark.parametrize("path", ["given_scores", "fused"])
def test_the_reduction_at_its_limits_k1024_top16(path):
    """K = 1024 uses all 16 `taken` bits of every lane and ``top_k = 16`` all 16 ranks: argmax, sample and topk_mean at temperatures 1, 20
    and 300 through ``cdx_select_f32`` over given scores (one launch) and behind the critic (64 tiles per state, two launches)."""
    from cleandiffuser_amd.engine import select as E
    case = sc.CASES["mlp_s2_k1024"]
    assert case.K == E.MAX_K
    critic, obs, cand, u = _on_device(case)
    scores = None
    if path == "given_scores":
        q = sc.request(E, case, critic, obs, cand, "none", 1.0)
        E.native_score_select(q)
        scores = q.scores.clone()
    for mode, top_k in (("argmax", 1), ("sample", 1), ("topk_mean", E.MAX_TOPK)):
        for temperature in sc.TEMPERATURES:
            q = sc.request(E, case, critic, obs, cand, mode, temperature, top_k, u if mode == "sample" else None, scores=scores)
            assert E.run(q) == (1 if path == "given_scores" else 2)
            torch.cuda.synchronize()
            if mode == "topk_mean":
                assert q.index.shape == (case.S, E.MAX_TOPK) and all(len(set(row)) == E.MAX_TOPK for row in q.index.tolist())
            _check_reduction(E, q, f"k1024 {path} {mode} T={temperature}", cand.cpu().double())


def test_given_scores_with_ties_and_a_strided_payload():
    """``cdx_select_f32`` alone over scores with exact ties: the first maximum, the top 4 with the lowest index on ties, the payload read
    through a row stride wider than P."""
    from cleandiffuser_amd.engine import select as E
    t = sc.tie_case()
    scores, wide = t.scores.to(DEV), t.wide.to(DEV)
    payload = wide[:, t.cols]
    assert not payload.is_contiguous()
    u = torch.tensor([0.07, 0.41, 0.93], device=DEV)        # (chosen on the CPU: 7.6e-3 away from every running sum at the three temperatures)
    for mode, top_k in MODES + (("none", 1),):
        for temperature in sc.TEMPERATURES:
            q = E.make_request(t.S, t.K, mode, temperature, t.top_k if mode == "topk_mean" else 1, u if mode == "sample" else None,
                               scores=scores, payload=payload, want_weights=True)
            assert E.run(q) == 1
            torch.cuda.synchronize()
            _check_reduction(E, q, f"ties {mode} T={temperature}", t.wide[:, t.cols].double())
    s2 = t.scores.view(t.S, t.K)
    q = E.make_request(t.S, t.K, "topk_mean", 1.0, t.top_k, scores=scores, payload=payload)
    E.run(q)
    for s in range(t.S):
        assert q.index[s].tolist() == sorted(range(t.K), key=lambda k: (-float(s2[s, k]), k))[:t.top_k]


@pytest.mark.parametrize("name", sc.TABLE)
def test_select_candidates_equals_the_pipelines_expression(name, monkeypatch):
    """End to end on the device: ``select_candidates`` against the pipelines' own lines on the stock route (the observation repeated,
    the critic as a module, torch's softmax / argmax / argsort / gather): scores at 1e-4, indices equal, picked at 1e-5 -- after
    asserting that every decision of every state has a margin of at least 1e-3 in the float64 restatement; one launch for K <= 16, two
    for K > 16; a second run gives the same bits; ``CDX_SELECT=0`` takes no native launch and agrees."""
    from cleandiffuser_amd.engine import select as E
    from cleandiffuser_amd.utils.selection import select_candidates
    case = sc.CASES[name]
    critic, obs, cand, u = _on_device(case)
    scores64 = _float64_scores(E, case)
    seen = _spy(monkeypatch)
    T = sc.E2E_TEMPERATURE
    for mode, top_k in MODES:
        top_k = min(top_k, case.K)
        margin = sc.decision_margin(scores64, mode, T, top_k, u.cpu())
        print(f"  {name} {mode}: decision margin {margin:.3e}")
        assert margin >= 1e-3, (name, mode, margin)
        with torch.no_grad():
            want = sc.pipeline_expression(critic, obs, cand, case.K, mode, T, top_k, u)
        del seen[:]
        kw = dict(mode=mode, temperature=T, top_k=top_k, u=u, want_weights=True)
        got = select_candidates(critic, obs, cand, case.K, **kw)
        assert seen == (["native_score_select"] if case.K <= 16 else ["native_score_select", "native_select"]), seen
        again = select_candidates(critic, obs, cand, case.K, **kw)
        torch.cuda.synchronize()
        _assert_close(got.scores, want["scores"], 1e-4, f"{name} {mode} scores")
        assert torch.equal(got.index.long(), want["index"]), (name, mode)
        _assert_close(got.picked, want["picked"], 1e-5, f"{name} {mode} picked")
        for a, b in zip(got, again):
            assert torch.equal(a, b), (name, mode, "two runs differ")
        del seen[:]
        monkeypatch.setenv("CDX_SELECT", "0")
        off = select_candidates(critic, obs, cand, case.K, **kw)
        monkeypatch.delenv("CDX_SELECT")
        assert not seen
        _assert_close(off.scores, got.scores, 1e-4, f"{name} {mode} CDX_SELECT=0 scores")
        assert torch.equal(off.index, got.index)
        _assert_close(off.picked, got.picked, 1e-5, f"{name} {mode} CDX_SELECT=0 picked")


def test_select_by_score_is_one_launch(monkeypatch):
    """Given scores (Diffuser's log_p, Decision Veteran's values) with a payload slice ``traj[:, 0, obs_dim:]`` read in place: one native
    call, the pipelines' argmax and index; a critic the kernel does not take (GELU) runs as a module and the reduction is one call."""
    import torch.nn as nn
    from cleandiffuser_amd.utils.selection import select_by_score, select_candidates
    seen = _spy(monkeypatch)
    g = torch.Generator().manual_seed(9)
    S, K, H, D, O = 4, 64, 5, 9, 4
    traj, log_p = torch.randn(S * K, H, D, generator=g).to(DEV), torch.randn(S * K, generator=g).to(DEV)
    sel = select_by_score(log_p, traj[:, 0, O:], K, mode="argmax")
    assert seen == ["native_select"]
    idx = torch.argmax(log_p.view(S, K), -1)
    assert torch.equal(sel.index.long(), idx)
    assert torch.equal(sel.picked, traj.view(S, K, H, D)[torch.arange(S), idx][:, 0, O:])
    del seen[:]
    gelu = nn.Sequential(nn.Linear(D, 32), nn.GELU(), nn.Linear(32, 1)).to(DEV)
    obs, cand = traj[:S, 0, :O].contiguous(), traj[:, 0, O:].contiguous()
    sel = select_candidates(gelu, obs, cand, K, mode="argmax")
    assert seen == ["native_select"]
    with torch.no_grad():
        want = gelu(torch.cat([obs.unsqueeze(1).repeat(1, K, 1).view(-1, O), cand], -1)).view(S, K)
    _assert_close(sel.scores, want, 1e-5, "module scores")
    assert torch.equal(sel.index.long(), torch.argmax(want, -1))
