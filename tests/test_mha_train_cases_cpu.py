"""The reference, the table and the yardsticks of tests/mha_train_cases.py, without a GPU.

* The float64 reference (plain torch ops: scores, softmax, keep, the product with v; autograd for dq, dk, dv) equals
  ``F.multi_head_attention_forward`` in float64 with identity projections, ``need_weights=False`` and ``dropout_p=0`` to 1e-12 of the
  largest element, output and input gradients, on one packed and one cross case.
* The table is what it says, on the reference alone: every float64 tensor of every case is finite; every query row has a key that is
  not -inf, and `floor_mask_row` has no -inf at all while its row 2 is masked entirely and comes out uniform; the dropped row of out
  and the dropped row of dv are exactly 0; `one_key` has dq = dk = 0 exactly; `shifted`'s scores lie in 95 .. 105 and their fp32 exp
  without a shift is not finite; `odd_blocks`' layout starts off a 16-byte boundary; the limits case needs the 99.8 KB it claims.
* YARDSTICK: the same ops in fp32 on the CPU against float64, E = max |a - b| / max(1, max |b|) per tensor.  No case exceeds its
  family's constant, and the largest of each family lies above half of it.

Measured (8 CPU threads; the same with 1), largest fp32 E per case over out / dq / dk / dv:
  limits_self 3.33e-7, wide_heads 6.81e-7, one_token 0, one_key 1.42e-7, one_query 1.45e-7, ragged_cross 1.66e-7, odd_blocks 3.71e-7,
  dropped_row_and_column 1.82e-7, floor_mask_row 1.59e-7                          -> YARDSTICK["mha"] = 8e-7
  shifted 1.10e-5 (out; dq 7.4e-6, dk 5.4e-6, dv 6.8e-6)                          -> YARDSTICK["mha_shifted"] = 1.2e-5
  peaked 9.94e-7 (dk; out 7.6e-7, dq 9.5e-7, dv 3.6e-7)                           -> YARDSTICK["mha_peaked"] = 1.2e-6
  attention_backward: 4.50e-7, 4.67e-7, 3.47e-7, 0, 1.76e-7 in table order        -> YARDSTICK["attn_bwd"] = 6e-7
  column sums, fp32 accumulated row by row (torch's pairwise ``sum`` in brackets): 0 (0), 1.27e-7 (1.11e-7), 1.69e-7 (1.27e-7),
  1.94e-7 (8.6e-8), 1.51e-7 (8.0e-8), 8.21e-7 (8.7e-8) in table order               -> YARDSTICK["colsum"] = 1e-6
`pytest -s` prints every case's figure next to its yardstick."""
import pytest
import torch
import torch.nn.functional as F

import mha_train_cases as M

NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def ref64():
    return {name: M.reference(case) for name, case in M.CASES.items()}


@pytest.mark.parametrize("name", ["limits_self", "ragged_cross"])
def test_float64_reference_is_torchs_multi_head_attention(name):
    case = M.CASES[name]
    assert case.layout == ("packed" if name == "limits_self" else "cross")
    x = M.inputs(case)
    e = case.dm
    q, k, v = (z.double().reshape(case.B, -1, e).transpose(0, 1).detach().requires_grad_(True) for z in (x.q, x.k, x.v))     # (T, B, E)
    eye = torch.eye(e, dtype=torch.float64)
    out, _ = F.multi_head_attention_forward(q, k, v, e, case.H, torch.cat([eye, eye, eye]), None, None, None, False, 0.0, eye, None,
                                            training=True, need_weights=False, attn_mask=x.mask.double())
    out.backward(x.dout.double().reshape(case.B, -1, e).transpose(0, 1))
    got = {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    ref = M.reference(case, dropout=False)
    for t in M.TENSORS:
        want = getattr(ref, t)
        d = float((got[t].transpose(0, 1).reshape(want.shape) - want).abs().max()) / float(want.abs().max())
        print(f"\n{name} {t}: reference against F.multi_head_attention_forward in float64 {d:.2e}")
        assert d <= 1e-12


def test_every_float64_tensor_is_finite(ref64):
    for name, r in ref64.items():
        for t in M.TENSORS:
            assert bool(torch.isfinite(getattr(r, t)).all()), (name, t)
    for shape in M.ATTN_BWD_CASES:
        assert bool(torch.isfinite(M.attn_bwd_reference(shape)).all()), shape


def test_the_masks_are_what_the_table_says():
    kinds = set()
    for name, case in M.CASES.items():
        mask = M.mask_of(case)
        kinds.add(case.mask)
        if mask is None:
            continue
        assert mask.shape == (case.Tq, case.Tk) and mask.dtype == torch.float32
        assert bool((mask > NEG_INF).any(dim=1).all()), f"{name}: a query row without a key"
    assert kinds == {None, "causal", "staggered", "floor"}
    case = M.CASES["floor_mask_row"]
    mask, floor = M.mask_of(case), torch.finfo(torch.float32).min
    assert not bool(torch.isinf(mask).any()) and bool((mask[M.FLOOR_ROW] == floor).all())
    assert all(bool((mask[i] == 0).any()) for i in range(case.Tq) if i != M.FLOOR_ROW)
    x = M.inputs(case)
    for dtype in (torch.float32, torch.float64):           # torch: the score is absorbed by the floor, the row is uniform
        p = torch.softmax(M.scores(x.q.to(dtype), x.k.to(dtype), case.B, case.H, mask), dim=-1)
        assert torch.equal(p[:, :, M.FLOOR_ROW], torch.full((case.B, case.H, case.Tk), 1.0 / case.Tk, dtype=dtype))


def test_the_dropped_row_and_column_are_exactly_zero(ref64):
    case, r = M.CASES["dropped_row_and_column"], ref64["dropped_row_and_column"]
    keep = M.inputs(case).keep
    (b, h, i), (b2, h2, j) = M.DROPPED_ROW, M.DROPPED_COLUMN
    assert float(keep[b, h, i].abs().max()) == 0.0 and float(keep[b2, h2, :, j].abs().max()) == 0.0
    out = r.out.view(case.B, case.Tq, case.H, case.dh)
    dv = r.dv.view(case.B, case.Tk, case.H, case.dh)
    assert float(out[b, i, h].abs().max()) == 0.0 and float(dv[b2, j, h2].abs().max()) == 0.0
    assert float(out[b, i].abs().max()) > 0.0 and float(dv[b2, j].abs().max()) > 0.0          # (the other heads of those rows are not)
    assert 0.0 < float((keep == 0).float().mean()) < 0.5 and set(keep.unique().tolist()) == {0.0, float(torch.tensor(1.0) / (1.0 - case.drop))}


def test_one_key_has_no_query_or_key_gradient(ref64):
    r = ref64["one_key"]
    assert float(r.dq.abs().max()) == 0.0 and float(r.dk.abs().max()) == 0.0 and float(r.dv.abs().max()) > 1.0


def test_shifted_scores_overflow_without_the_max_subtraction():
    case = M.CASES["shifted"]
    x = M.inputs(case)
    sc = M.scores(x.q, x.k, case.B, case.H)
    print(f"\nshifted: scores {float(sc.min()):.1f} .. {float(sc.max()):.1f}")
    assert sc.dtype == torch.float32 and 95.0 < float(sc.min()) and float(sc.max()) < 105.0
    assert not bool(torch.isfinite(torch.exp(sc)).any())


def test_the_shapes_reach_what_the_table_says():
    lds = lambda c, bwd: 4 * ((2 if bwd else 1) * c.Tq * (c.dh + 1) + 2 * c.Tk * (c.dh + 1) + (2 if bwd else 1) * c.Tq * (c.Tk + 1))
    lim, wide = M.CASES["limits_self"], M.CASES["wide_heads"]
    assert (lds(lim, True), lds(lim, False)) == (99840, 66560) and lds(wide, True) == 67072       # csrc/cdx_train.hip: mha_lds_bytes
    assert all(c.B in (2, 3) and max(c.Tq, c.Tk, c.dh) <= 64 for c in M.CASES.values())
    assert {c.layout for c in M.CASES.values()} == {"packed", "cross", "odd"}
    assert all(c.Tq == c.Tk for c in M.CASES.values() if c.layout == "packed")
    assert (M.ODD_OFF + M.ODD_COL) % 4 != 0 and M.ODD_LD % 2 == 1 and M.ODD_COL + M.CASES["odd_blocks"].dm <= M.ODD_LD
    p, r = M.inputs(M.CASES["peaked"]), M.inputs(M.CASES["ragged_cross"])
    assert float(M.scores(p.q, p.k, 2, 3).std()) > 12.0 > 2.0 > float(M.scores(r.q, r.k, 2, 3).std())
    assert [s[1:] for s in M.COLSUM_CASES if s[1] != s[2]] == [(33, 40)]
    assert {-(-r // 64) for r, _, _ in M.COLSUM_CASES} >= {1, 2, 65} and {-(-c // 64) for _, c, _ in M.COLSUM_CASES} >= {1, 2, 3}


def test_fp32_attention_is_within_the_yardstick(ref64):
    top = {}
    for name, case in M.CASES.items():
        errs = M.errors(M.reference(case, torch.float32), ref64[name])
        k, w = M.worst(errs)
        print(f"\n{name}: fp32 CPU against float64 " + ", ".join(f"{t} {e:.2e}" for t, e in errs.items()) +
              f" (YARDSTICK[{case.family}] {M.YARDSTICK[case.family]:.1e})")
        assert w <= M.YARDSTICK[case.family], (name, k, w)
        top[case.family] = max(top.get(case.family, 0.0), w)
    assert set(top) == {"mha", "mha_shifted", "mha_peaked"}
    for family, w in top.items():
        assert w > 0.5 * M.YARDSTICK[family], f"YARDSTICK[{family}] is the measured maximum rounded up, not a loose guess"
    assert top["mha"] < top["mha_peaked"] < top["mha_shifted"]


def test_fp32_attention_backward_is_within_the_yardstick():
    top = 0.0
    for shape in M.ATTN_BWD_CASES:
        e = M.error(M.attn_bwd_reference(shape, torch.float32), M.attn_bwd_reference(shape))
        print(f"\nattention_backward {shape}: fp32 CPU against float64 {e:.2e} (YARDSTICK[attn_bwd] {M.YARDSTICK['attn_bwd']:.1e})")
        assert e <= M.YARDSTICK["attn_bwd"], shape
        top = max(top, e)
    assert top > 0.5 * M.YARDSTICK["attn_bwd"]


def test_fp32_row_by_row_column_sums_are_within_the_yardstick():
    top = 0.0
    for shape in M.COLSUM_CASES:
        x = M.colsum_input(shape)
        want = x.double().sum(0)
        e, pairwise = M.error(M.colsum_sequential_fp32(x), want), M.error(x.sum(0), want)
        print(f"\ncolsum {shape}: fp32 row by row against float64 {e:.2e} (torch.sum {pairwise:.2e}; YARDSTICK[colsum] {M.YARDSTICK['colsum']:.1e})")
        assert e <= M.YARDSTICK["colsum"], shape
        top = max(top, e)
    assert top > 0.5 * M.YARDSTICK["colsum"]
