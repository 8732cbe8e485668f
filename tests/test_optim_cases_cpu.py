"""The reference and the yardstick of tests/optim_cases.py, without a GPU.

* The float64 reference (written term by term from csrc/cdx_optim.hip) equals ``clip_grad_norm_`` + ``torch.optim.AdamW`` / ``Adam``
  (``foreach=False``) + the reference's EMA loop in float64 on the CPU to 1e-12 of each tensor's largest element, in every scenario --
  and with a NaN or an infinite gradient element, where it must reproduce torch's non-finite values exactly.
* YARDSTICK: the same torch sequence in fp32 against float64, over p, exp_avg, exp_avg_sq, the EMA copy and the reported norms, each
  relative to its tensor's largest element.  No scenario exceeds the committed constant, and the largest lies above half of it.
* The table is what it says: the clip engages at steps 1 and 3 and not at step 2; the carved views start off a 16-byte boundary;
  both groups hold aligned and carved tensors.

Measured (8 CPU threads), largest fp32 error per kind over the 16 scenarios: p 1.51e-7, exp_avg 1.18e-7, exp_avg_sq
1.95e-7, the EMA copy 1.71e-7, the norm 5.95e-8 -- YARDSTICK is the maximum rounded up to 2e-7.  `pytest -s` prints every scenario."""
import pytest
import torch

import optim_cases as O


@pytest.mark.parametrize("name", O.TABLE)
def test_float64_reference_is_torchs_sequence(name):
    scn = O.SCENARIOS[name]
    ref, seq = O.reference(scn), O.torch_sequence(scn, torch.float64)
    k, w = O.worst(O.errors(seq, ref))
    print(f"\n{name}: reference against torch in float64 {w:.2e} {k}")
    assert w <= 1e-12
    assert seq.steps == [float(O.STEPS)] * len(seq.p)
    if scn.clip:
        assert ref.norms[0] > O.MAX_NORM and ref.norms[1] < O.MAX_NORM and ref.norms[2] > O.MAX_NORM, ref.norms


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_float64_reference_follows_torch_through_a_non_finite_gradient(value):
    """One NaN element: torch's coefficient is NaN (``clamp`` keeps it) and every parameter ends NaN.  One infinite element: the
    coefficient is 0, every gradient becomes 0 except the infinite element (inf x 0 = NaN), so one parameter element ends NaN."""
    scn = O.SCENARIOS["adamw_clip_ema_zero"]
    grads = O.gradients(poison=(value, 0, 3, 17))
    ref, seq = O.reference(scn, grads, steps=1), O.torch_sequence(scn, torch.float64, grads, steps=1)
    assert O.worst(O.errors(seq, ref))[1] <= 1e-12
    n_nan = sum(int(torch.isnan(p).sum()) for p in ref.p)
    if value != value:
        assert ref.norms[0] != ref.norms[0] and n_nan == 2 * sum(O.NUMEL)
        assert all(torch.isnan(e).all() for e in ref.ema)
    else:
        assert ref.norms[0] == float("inf") and n_nan == 1 and torch.isnan(ref.p[3].view(-1)[17])


def test_fp32_sequence_is_within_the_yardstick():
    top = {}
    for name, scn in O.SCENARIOS.items():
        errs = O.errors(O.torch_sequence(scn, torch.float32), O.reference(scn))
        for (kind, _), e in errs.items():
            top[kind] = max(top.get(kind, 0.0), e)
        k, w = O.worst(errs)
        print(f"\n{name}: fp32 torch sequence against float64 {w:.3e} {k}")
        assert w <= O.YARDSTICK, (name, k, w)
    print("\nlargest per kind: " + ", ".join(f"{k} {e:.3e}" for k, e in top.items()))
    assert set(top) == {"p", "m", "v", "ema", "norm"}
    assert max(top.values()) > 0.5 * O.YARDSTICK, "YARDSTICK is the measured maximum rounded up, not a loose guess"


def test_the_parameter_set_is_what_the_table_says():
    flat = torch.zeros(O.flat_size())
    assert flat.data_ptr() % 16 == 0
    views = O.carve(flat)
    assert [tuple(v.shape) for v in views] == O.SHAPES and all(v.is_contiguous() and v.data_ptr() % 16 != 0 for v in views)
    assert views[0].data_ptr() - flat.data_ptr() == 4 * O.GUARD
    for k in range(len(O.GROUPS)):
        mine = [i for i, g in enumerate(O.GROUP_OF) if g == k]
        assert any(i < O.N_ALIGNED for i in mine) and any(i >= O.N_ALIGNED for i in mine)
    chunk = 4096
    assert {n % 4 for n in O.NUMEL} == {0, 1, 3} and {-(-n // chunk) for n in O.NUMEL} == {1, 2, 3}
    assert {chunk - 1, chunk, chunk + 1} <= set(O.NUMEL)
    assert O.GROUPS[0]["weight_decay"] > 0 and O.GROUPS[1]["weight_decay"] == 0
    assert len(O.TABLE) == 16
