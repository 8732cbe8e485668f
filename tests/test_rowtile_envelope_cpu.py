"""CPU tier: the seven row-tile case tables (tests/*_cases.py) against the sizes the kernels' host checks admit.  The GPU tests can only
run what the tables list; this check makes the tables reach the edges of the admitted envelope -- more than one trip of the (16 x A) element
loops, each admitted maximum, a partial second sweep of the product, many K blocks with a ragged end -- and holds the routers and the C
entry points to the same boundary: the last admitted size passes both, the first size past it is refused by both, by the C side with
CDX_EINVAL before anything is launched."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cep_cases  # noqa: E402
import critic_step_cases  # noqa: E402
import denoise_cases  # noqa: E402
import energy_cases  # noqa: E402
import rollout_cases  # noqa: E402
import select_cases  # noqa: E402
import tower_cases  # noqa: E402
from test_train_paths_cpu import _everything_is_on_the_device  # noqa: E402

EINVAL = -1
critic_request, select_request, tower_request = critic_step_cases.sizes_request, select_cases.c_request, tower_cases.c_request


def _row_mlp(case):
    """DQLMlp / DVInvMlp (class, obs, act, emb, hidden): three hidden layers of one width on [x | temb | cond]."""
    cls, obs, act, emb, hidden = case.net
    return dict(A=[act], E=[emb], width=[256 if hidden is None else hidden], first_k=[act + emb + (obs if cls == "DQLMlp" else 2 * obs)])


def _select(case):
    hidden = case.hidden if isinstance(case.hidden, list) else [case.hidden]
    return dict(A=[case.A], width=hidden, first_k=[case.O + case.A], K=[case.K])


# family -> (its table module, case -> the values each dimension takes in that case)
FAMILIES = {
    "rollout": (rollout_cases, lambda c: {k: v for k, v in _row_mlp(c).items() if k != "E"}),      # (ro_check bounds E through A + E + O alone)
    "denoise": (denoise_cases, _row_mlp),
    "tower": (tower_cases, lambda c: dict(width=c.widths[:-1], first_k=[c.k0], last=[c.widths[-1]])),
    "critic_step": (critic_step_cases, lambda c: dict(width=c.live[:-1] + c.target[:-1], first_k=[c.a0 + c.a1, c.b0 + c.b1], K=[c.group])),
    "select": (select_cases, _select),
    "cep": (cep_cases, lambda c: dict(A=[c.A], E=[c.Ec], width=c.hidden, first_k=[c.O])),
    "energy": (energy_cases, lambda c: dict(A=[c.A], E=[c.emb, c.clf_emb], width=c.hidden + c.clf_hidden, first_k=[c.O])),
}
# the admitted maximum of every dimension a family's host check names (csrc/cdx_rowtile.h: RO_MAX_*; cdx_tower_layers.h; 2 E <= 512 in
# cdx_denoise.hip; CDX_CRITIC_MAX_K; CDX_SELECT_MAX_K).  first_k: A + E + O of the row MLPs, K0 of a tower or critic, O of obs_proj.
MAXIMA = {
    "rollout": dict(A=64, width=512, first_k=512),
    "denoise": dict(A=64, E=256, width=512, first_k=512),
    "tower": dict(width=512, first_k=512, last=64),
    "critic_step": dict(width=512, first_k=512, K=16),
    "select": dict(A=64, width=512, first_k=512, K=1024),
    "cep": dict(A=64, E=128, width=512, first_k=512),
    "energy": dict(A=64, E=128, width=512, first_k=512),
}


def _values(family):
    module, sizes = FAMILIES[family]
    out = {}
    for name in module.TABLE:
        for dim, values in sizes(module.CASES[name]).items():
            out.setdefault(dim, set()).update(values)
    return out


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_table_reaches_the_edges_of_the_admitted_envelope(family):
    """Every family's TABLE (what both the CPU restatement tests and the GPU tests iterate) has, where the dimension exists for it: a
    case with A > 16, one at each admitted maximum, a last width above 16, a hidden width in (256, 512) that is no multiple of 64 and a
    first-layer K above 64 that is no multiple of 4."""
    module, _ = FAMILIES[family]
    assert set(module.ENVELOPE) <= set(module.TABLE) and set(module.TABLE) <= set(module.CASES)
    seen = _values(family)
    assert set(seen) == set(MAXIMA[family]), (family, sorted(seen))
    for dim, top in MAXIMA[family].items():
        assert max(seen[dim]) == top, f"{family}: no case at {dim} = {top} (largest: {max(seen[dim])})"
    if "A" in seen:
        assert any(a > 16 for a in seen["A"]), f"{family}: no case with A > 16"
    if "last" in seen:
        assert any(16 < w < 64 for w in seen["last"]), f"{family}: no last width between 16 and 64"
    assert any(256 < w < 512 and w % 64 for w in seen["width"]), f"{family}: no partial second sweep of the product"
    assert any(k > 64 and k % 4 for k in seen["first_k"]), f"{family}: no ragged first-layer K above 64"


# ------------------------------------------------------------------------------------------------------------------- #
# The boundary itself: router and C entry point, at the limit and one step past it                                            #
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build_libcdx()
    from cleandiffuser_amd.engine import runtime
    return runtime.load_library()


def _passes_the_size_checks(lib, rc):
    """A request of sizes alone (every pointer null) that the size checks admit ends at the pointer checks, which come after them."""
    return rc == EINVAL and b"null pointer" in lib.cdx_last_error()


def _refused_for(lib, rc, word):
    return rc == EINVAL and word in lib.cdx_last_error()


def _rollout_steps():
    from cleandiffuser_amd.engine import runtime
    steps = (runtime.CdxStep * 1)()
    steps[0].noise_idx = -1
    return steps


# (A, E, O, W) at the limits, then one step past each: (sizes, the word of the C side's message)
# (O even: DVInvMlp reads (obs, next_obs), and only it has a width to choose)
ROW_MLP_OK = [(64, 128, 320, 512), (64, 16, 2, 16), (2, 16, 494, 512), (17, 16, 120, 272)]
ROW_MLP_PAST = [((65, 16, 2, 32), b"A must be"), ((64, 128, 322, 512), b"A + E + O"), ((6, 16, 10, 528), b"multiple of 16"),
                ((6, 16, 10, 24), b"multiple of 16")]


def test_rollout_boundary(lib, amd_lib):
    """``rollout._trunk`` and ``cdx_rollout_fwd_f32`` / ``cdx_rollout_bwd_f32``: A = 64, A + E + O = 512 and W = 512 pass, 65 / 513 / 528
    are refused."""
    from cleandiffuser_amd.engine import rollout
    steps = _rollout_steps()

    def c_request(a, e, o, w):
        return rollout.CdxRollout(B=4, A=a, E=e, O=o, W=w, S=1, steps=ctypes.cast(steps, ctypes.c_void_p))
    for a, e, o, w in ROW_MLP_OK:
        assert rollout._trunk(amd_lib.DVInvMlp(o // 2, a, emb_dim=e, hidden_dim=w)) is not None, (a, e, o, w)
        for fn in (lib.cdx_rollout_fwd_f32, lib.cdx_rollout_bwd_f32):
            assert _passes_the_size_checks(lib, fn(ctypes.byref(c_request(a, e, o, w)), None)), (a, e, o, w, lib.cdx_last_error())
    for (a, e, o, w), word in ROW_MLP_PAST:
        assert rollout._trunk(amd_lib.DVInvMlp(o // 2, a, emb_dim=e, hidden_dim=w)) is None, (a, e, o, w)
        for fn in (lib.cdx_rollout_fwd_f32, lib.cdx_rollout_bwd_f32):
            assert _refused_for(lib, fn(ctypes.byref(c_request(a, e, o, w)), None), word), (a, e, o, w, lib.cdx_last_error())


def test_denoise_boundary(lib, amd_lib):
    """``denoise._net_spec`` / ``denoise.lds_bytes`` and ``cdx_denoise_fwd_f32`` / ``cdx_denoise_bwd_f32``: the limits of the rollout, and
    2 E = 512 passes where 2 E = 528 is refused."""
    from cleandiffuser_amd.engine import denoise

    def spec(a, e, o, w):
        net = amd_lib.DVInvMlp(o // 2, a, emb_dim=e, hidden_dim=w)
        with _everything_is_on_the_device():
            return denoise._net_spec(net, a)
    for a, e, o, w in ROW_MLP_OK + [(3, 256, 8, 32)]:
        assert denoise.lds_bytes(a, e, o, w) <= denoise.MAX_LDS
        assert spec(a, e, o, w) is not None, (a, e, o, w)
        for fn in (lib.cdx_denoise_fwd_f32, lib.cdx_denoise_bwd_f32):
            assert _passes_the_size_checks(lib, fn(ctypes.byref(denoise.CdxDenoise(R=4, A=a, E=e, O=o, W=w)), None)), (a, e, o, w)
    for (a, e, o, w), word in ROW_MLP_PAST + [((3, 264, 8, 32), b"2 E")]:
        assert spec(a, e, o, w) is None, (a, e, o, w)
        for fn in (lib.cdx_denoise_fwd_f32, lib.cdx_denoise_bwd_f32):
            assert _refused_for(lib, fn(ctypes.byref(denoise.CdxDenoise(R=4, A=a, E=e, O=o, W=w)), None), word), (a, e, o, w)


TOWER_OK = [(512, [512, 512, 64]), (1, [16, 1]), (69, [256, 256, 256, 1]), (33, [48, 33]), (512, [512] * 5 + [64])]
TOWER_PAST = [((513, [16, 1]), b"K0"), ((7, [528, 1]), b"multiple of 16"), ((7, [16, 65]), b"last width"), ((7, [24, 1]), b"multiple of 16")]


def _tower_desc(k0, widths):
    return SimpleNamespace(K0=k0, width=list(widths), norm=[False] * len(widths), eps=[0.0] * len(widths))


def test_tower_boundary(lib):
    """``tower.within_limits`` and ``cdx_tower_fwd_f32`` / ``cdx_tower_bwd_f32``: K0 = 512, width 512 and a last width of 64 pass, 513 /
    528 / 65 are refused."""
    from cleandiffuser_amd.engine import tower
    for k0, widths in TOWER_OK:
        assert tower.within_limits(_tower_desc(k0, widths)) and tower.lds_bytes(_tower_desc(k0, widths)) <= tower.MAX_LDS
        for fn in (lib.cdx_tower_fwd_f32, lib.cdx_tower_bwd_f32):
            assert _passes_the_size_checks(lib, fn(ctypes.byref(tower_request(tower, k0, widths)), None)), (k0, widths)
    for (k0, widths), word in TOWER_PAST:
        assert not tower.within_limits(_tower_desc(k0, widths))
        for fn in (lib.cdx_tower_fwd_f32, lib.cdx_tower_bwd_f32):
            assert _refused_for(lib, fn(ctypes.byref(tower_request(tower, k0, widths)), None), word), (k0, widths, lib.cdx_last_error())


def test_critic_step_boundary(lib):
    """``critic_step.shapes_ok``'s LDS plan and ``cdx_critic_step_f32``: K0 = 512 into a 512-wide layer and K = 16 pass; K0 = 513, a
    528-wide layer, K = 17 and a plan over 160 KiB are refused."""
    from cleandiffuser_amd.engine import critic_step, tower
    net = lambda k0, widths: SimpleNamespace(K0=k0, width=list(widths))                                  # noqa: E731
    for live, target, k in (((512, [512, 1]), (512, [512, 1]), 1), ((69, [256, 256, 256, 1]), (69, [256, 256, 256, 1]), 16),
                            ((85, [272, 272, 1]), (76, [272, 1]), 1)):
        assert critic_step.lds_bytes(net(*live), net(*target)) <= critic_step.MAX_LDS and k <= critic_step.MAX_K
        assert tower.within_limits(_tower_desc(*live)) and tower.within_limits(_tower_desc(*target))
        assert _passes_the_size_checks(lib, lib.cdx_critic_step_f32(ctypes.byref(critic_request(critic_step, live, target, K=k)), None)), (live, k)
    for live, target, k, word in (((513, [16, 1]), (14, [16, 1]), 1, b"K0"), ((14, [16, 1]), (513, [16, 1]), 1, b"K0"),
                                  ((14, [528, 1]), (14, [16, 1]), 1, b"multiple of 16"), ((14, [16, 1]), (14, [16, 1]), 17, b"K must be"),
                                  ((512, [512] * 5 + [1]), (14, [16, 1]), 1, b"160 KiB")):
        assert k > critic_step.MAX_K or not (tower.within_limits(_tower_desc(*live)) and tower.within_limits(_tower_desc(*target))
                                             and critic_step.lds_bytes(net(*live), net(*target)) <= critic_step.MAX_LDS)
        assert _refused_for(lib, lib.cdx_critic_step_f32(ctypes.byref(critic_request(critic_step, live, target, K=k)), None), word), \
            (live, target, k, lib.cdx_last_error())


def test_select_boundary(lib):
    """``select.describe_critic`` / ``select.within_limits`` and ``cdx_score_select_f32`` / ``cdx_select_f32``: O + A = 512 with A = 64, a
    512-wide layer, K = 1024 and top_k = 16 pass; 513, A = 65, 528, K = 1025 and top_k = 17 are refused."""
    from cleandiffuser_amd.engine import select as E

    def critic(k0, widths):
        mods, k = [], k0
        for w in widths[:-1]:
            mods += [nn.Linear(k, w), nn.SiLU()]
            k = w
        return [nn.Sequential(*mods, nn.Linear(k, widths[-1]))]
    for o, a, widths in ((448, 64, (512, 1)), (0, 1, (16, 1)), (76, 9, (272, 272, 1))):
        assert E.describe_critic(critic(o + a, widths), o, a) is not None, (o, a, widths)
        g = select_request(E, O=o, A=a, widths=widths, K=1024, mode=3, top_k=16)
        assert 0 < lib.cdx_score_select_lds_bytes(ctypes.byref(g)) <= E.MAX_LDS
        rc = lib.cdx_score_select_f32(ctypes.byref(g), None)
        assert rc == EINVAL and (b"null pointer" in lib.cdx_last_error() or b"obs must be given" in lib.cdx_last_error()), lib.cdx_last_error()
    for o, a, widths, word in ((449, 64, (16, 1), b"O + A"), (7, 65, (16, 1), b"A must be"), (7, 3, (528, 1), b"multiple of 16")):
        assert E.describe_critic(critic(o + a, widths), o, a) is None, (o, a, widths)
        assert _refused_for(lib, lib.cdx_score_select_f32(ctypes.byref(select_request(E, O=o, A=a, widths=widths)), None), word), (o, a, widths)
    assert E.within_limits(2, 1024, "topk_mean", 16, 1.0, 64)
    for kw, word in ((dict(K=1025), b"K must be"), (dict(K=50, mode=3, top_k=17), b"top_k"),
                     (dict(K=5, mode=1, picked=8, P=65, payload=8, payload_ld=65), b"P must be")):
        assert not E.within_limits(2, kw["K"], "topk_mean" if kw.get("mode") == 3 else "argmax", kw.get("top_k", 1), 1.0, kw.get("P", 4))
        assert _refused_for(lib, lib.cdx_select_f32(ctypes.byref(E.CdxSelect(S=2, temperature=1.0, **kw)), None), word), kw
        assert _refused_for(lib, lib.cdx_score_select_f32(ctypes.byref(select_request(E, S=2, **kw)), None), word), kw
    assert _passes_the_size_checks(lib, lib.cdx_select_f32(ctypes.byref(E.CdxSelect(S=2, K=1024, temperature=1.0, mode=3, top_k=16)), None))


def _cep_request(cep, a, o, ec, hidden, k=16):
    g = cep.CdxCepStep(B=2, K=k, A=a, O=o, Ec=ec, n_hidden=len(hidden))
    for l, w in enumerate(hidden[:len(g.hidden)]):           # (a layer count past CDX_ENERGY_MAX_HIDDEN travels with the widths that fit)
        g.hidden[l] = w
    return g


CLF_OK = [(64, 512, 128, [512, 512]), (9, 60, 64, [256, 256, 256]), (17, 85, 32, [272, 272]), (1, 1, 1, [16])]
CLF_PAST = [((65, 7, 16, [32]), b"A must be"), ((3, 513, 16, [32]), b"O must be"), ((3, 7, 129, [32]), b"must be at most 128"),
            ((3, 7, 16, [528]), b"multiple of 16"), ((3, 7, 16, [32] * 5), b"n_hidden"), ((64, 512, 128, [512] * 4), b"160 KiB")]


def test_cep_boundary(lib):
    """``cep.within_limits`` and ``cdx_cep_step_f32``: A = 64, O = 512, Ec = 128 and two 512-wide layers pass together (133 KiB); 65 / 513 /
    129 / 528, a fifth hidden layer and a plan over 160 KiB are refused."""
    from cleandiffuser_amd.engine import cep
    for a, o, ec, hidden in CLF_OK:
        desc = SimpleNamespace(A=a, O=o, Ec=ec, hidden=hidden)
        assert cep.within_limits(desc, 16) and cep.lds_bytes(desc) <= cep.MAX_LDS
        assert _passes_the_size_checks(lib, lib.cdx_cep_step_f32(ctypes.byref(_cep_request(cep, a, o, ec, hidden)), None)), (a, o, ec, hidden)
    for (a, o, ec, hidden), word in CLF_PAST:
        assert not cep.within_limits(SimpleNamespace(A=a, O=o, Ec=ec, hidden=hidden), 16)
        assert _refused_for(lib, lib.cdx_cep_step_f32(ctypes.byref(_cep_request(cep, a, o, ec, hidden)), None), word), \
            (a, o, ec, hidden, lib.cdx_last_error())
    assert not cep.within_limits(SimpleNamespace(A=3, O=7, Ec=16, hidden=[32]), 32)
    assert _refused_for(lib, lib.cdx_cep_step_f32(ctypes.byref(_cep_request(cep, 3, 7, 16, [32], k=32)), None), b"K must divide 16")


def _unet_rows(a, hidden):
    """The block table of SfBCUNet(a, hidden_dims=hidden) as ``describe_denoiser`` reads it: (in, in2, out) per block."""
    widths = [a] + list(hidden)
    rows = [(i, 0, o) for i, o in zip(widths[:-1], widths[1:])] + [(widths[-1], 0, widths[-1])]
    cur = widths[-1]
    for skip_w, out_w in zip(reversed(widths[2:]), reversed(widths[1:-1])):
        rows.append((cur, skip_w, out_w))
        cur = out_w
    return rows, len(hidden)


def _energy_request(energy, steps, cg, a, e, o, ec, hidden, clf_hidden):
    rows, n_down = _unet_rows(a, hidden)
    arr = (energy.CdxEnergyBlock * len(rows))(*[energy.CdxEnergyBlock(in_=i, in2=i2, out=w, ws=None if i + i2 == w else 8, bs=None if i + i2 == w else 8)
                                                 for i, i2, w in rows])
    g = energy.CdxEnergyGuided(B=2, A=a, E=e, O=o, S=1, Ec=ec, n_blocks=len(rows), n_down=n_down, n_hidden=len(clf_hidden), blocks=arr,
                               steps=steps, cg_scale=cg)
    for l, w in enumerate(clf_hidden):
        g.hidden[l] = w
    g._keep = arr
    den = SimpleNamespace(A=a, E=e, n_down=n_down, rows=[SimpleNamespace(in_=i, in2=i2, out=w) for i, i2, w in rows])
    return g, den, SimpleNamespace(A=a, O=o, Ec=ec, hidden=list(clf_hidden))


def test_energy_boundary(lib):
    """``energy.within_limits`` and ``cdx_energy_guided_run``: A = 64, O = 512, E = Ec = 128 and a 512-wide block in either net pass
    together, as does a concat input of 544 columns; 65 / 513 / 129 / 528, a concat input over 1024 and a plan over 160 KiB are refused."""
    from cleandiffuser_amd.engine import energy, runtime
    steps = (runtime.CdxStep * 1)()
    steps[0].noise_idx = -1
    cg = (ctypes.c_float * 1)()
    base = dict(a=3, e=32, o=7, ec=32, hidden=[64, 48, 32], clf_hidden=[48, 48])
    for change in (dict(a=64, e=128, o=512, ec=128, hidden=[512, 128], clf_hidden=[512]), dict(hidden=[32, 272, 272], o=85),
                   dict(a=9, o=60, e=64, ec=64, hidden=[512, 256, 128], clf_hidden=[256] * 3), dict(a=33)):
        g, den, clf = _energy_request(energy, steps, cg, **{**base, **change})
        assert energy.within_limits(den, clf, 1) and energy.lds_bytes(den, clf) <= energy.MAX_LDS, change
        assert lib.cdx_energy_guided_lds_bytes(ctypes.byref(g)) == energy.lds_bytes(den, clf), change
        assert _passes_the_size_checks(lib, lib.cdx_energy_guided_run(ctypes.byref(g), None)), (change, lib.cdx_last_error())
    for change, word in ((dict(a=65), b"A must be"), (dict(o=513), b"O must be"), (dict(e=129), b"E and Ec"), (dict(ec=129), b"E and Ec"),
                         (dict(hidden=[528, 32]), b"multiple of 16"), (dict(clf_hidden=[528]), b"multiple of 16"),
                         (dict(hidden=[16, 512, 512], clf_hidden=[512] * 4), b"160 KiB")):
        g, den, clf = _energy_request(energy, steps, cg, **{**base, **change})
        assert not energy.within_limits(den, clf, 1), change
        assert _refused_for(lib, lib.cdx_energy_guided_run(ctypes.byref(g), None), word), (change, lib.cdx_last_error())
    # a concat input over 1024 columns cannot come from widths of at most 512 (512 + 512 = 1024 passes that check): the table by hand
    g, den, clf = _energy_request(energy, steps, cg, **{**base, "hidden": [16, 512, 512]})
    assert max(r.in_ + r.in2 for r in den.rows) == energy.MAX_CONCAT
    g.blocks[4].in2 = den.rows[4].in2 = 528
    assert not energy.within_limits(den, clf, 1)
    assert _refused_for(lib, lib.cdx_energy_guided_run(ctypes.byref(g), None), b"concat input")
