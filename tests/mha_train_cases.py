"""TEST HELPER for the training step's attention core and row-sum kernels (csrc/cdx_train.hip: ``cdx_mha_train_kernel<false|true>``
behind ``cdx_mha_train_fwd_f32`` / ``cdx_mha_train_bwd_f32`` / ``cdx_attention_bwd_f32``, and ``cdx_colsum_f32``): the case tables, a
float64 reference in plain torch ops on the CPU, and the error measure.  tests/test_mha_train_cases_cpu.py holds the reference
against ``F.multi_head_attention_forward`` in float64 and measures the YARDSTICK (the same ops in fp32 on the CPU);
tests/test_gpu_mha_train.py runs every case on the device at FACTOR x that.  Nothing here is derived from a device result.

The operation:  P = softmax(q k^T / sqrt(dh) + mask),  Pd = P o keep,  out = Pd v  per (sample, head); autograd of exactly these ops
gives dq, dk, dv for a seeded ``dout``.  `keep` is DRAWN ONCE per case as 0 | 1 / (1 - p) (the kernel applies a mask its caller drew),
and the reference and the device use the same one.

Error measure (that of train_graph_cases.py): E = max |a - b| / max(1, max |b|) per tensor (out, dq, dk, dv).

``CASES`` -- each the smallest shape at which one thing can go wrong (B, Tq, Tk, H, dh; layout; mask; dropout):

* limits_self   2, 64, 64, 2, 64   packed [q | k | v], causal, 0.3: the kernel's limits -- 99.8 KB of LDS backward, 66.6 KB forward;
* wide_heads    2, 64, 64, 10, 32  packed, no mask, 0.1: the shipped DiT shape (67 KB backward, 10 heads per sample);
* one_token     3, 1, 1, 1, 1      packed: every loop runs one trip;
* one_key       2, 63, 1, 3, 6     cross, 0.1: softmax over one key -- dq and dk are exactly 0, dv is a column sum;
* one_query     2, 1, 64, 3, 24    cross, staggered (i >= j - 1): one row, 4 lanes walking 64 keys;
* ragged_cross  2, 33, 17, 3, 24   cross (q next to a packed [k | v] of another length), staggered, 0.5;
* odd_blocks    2, 7, 5, 3, 6      staggered, 0.3: q, k, v and the three gradients are column blocks starting at column ODD_COL of
                                   matrices with a row stride of ODD_LD floats whose first element sits ODD_OFF floats into its
                                   allocation -- no base on a 16-byte boundary, no stride a multiple of anything;
* peaked        as ragged_cross    q and k times 4: the logits' s.d. is ~16, the rows are near one-hot (a family of its own);
* shifted       2, 9, 12, 2, 16    cross, no mask: the first channel of every head of q and k is sqrt(100 sqrt(dh)) = 20, so every
                                   score is ~ +100 (97 .. 104) and exp without the max subtraction overflows fp32;
* dropped_row_and_column  2, 10, 10, 4, 16  packed, causal, 0.3: one (sample, head, query) row and one (sample, head, key) column of
                                   `keep` forced to 0 -- that row of out and that row of dv are exactly 0;
* floor_mask_row 2, 6, 4, 2, 8     cross: the staggered mask with query row 2 masked ENTIRELY, then ``clamp_min(finfo.min)`` the way
                                   engine/bigbatch.py prepares masks ("-inf entries map onto that floor").  No -inf is left; torch gives
                                   that row the uniform 1 / Tk in fp32 and in float64 (the score is absorbed by the floor).

``ATTN_BWD_CASES`` (B, T, H, dh) for ``blocks.attention_backward``: packed rows, no mask, no keep.
``COLSUM_CASES`` (R, C, ld) for ``blocks.colsum``: one row; one short of / exactly / one past the 64 x 64 tile; a column block of a wider
matrix (ld != C); 65 row slices meeting in the atomics.  ``out`` starts at COLSUM_START, not 0: the sums are ADDED."""
import math
from types import SimpleNamespace

import torch

FACTOR = 4.0                # device tolerance = FACTOR x YARDSTICK[family], the project's factor

# The largest E of the fp32 CPU run against float64 per family, rounded up (tests/test_mha_train_cases_cpu.py asserts that no case
# exceeds its constant and that the largest lies above half of it; the measured values are in that module's docstring).
# `shifted` is held to a yardstick of its own: its scores sit near +100, where one fp32 ulp of a LOGIT is 7.6e-6, and the fp32 run's
# error (1.1e-5) is 16 x that of any other case.  Folded into "mha" it would have set every plain case's tolerance by a conditioning
# only it has; kept apart, no case is checked more loosely than a yardstick over all of them would check it.
YARDSTICK = {
    "mha": 8e-7,            # measured 6.81e-7 (wide_heads dq)
    "mha_shifted": 1.2e-5,  # measured 1.10e-5 (out)
    "mha_peaked": 1.2e-6,   # measured 9.94e-7 (dk)
    "attn_bwd": 6e-7,       # measured 4.67e-7 ((2, 64, 1, 64))
    "colsum": 1e-6,         # measured 8.21e-7 ((4097, 33, 33)), fp32 accumulated row by row
}

ODD_COL, ODD_LD, ODD_OFF = 3, 41, 2
COLSUM_START = 0.5
TENSORS = ("out", "dq", "dk", "dv")


def _case(name, B, Tq, Tk, H, dh, layout, mask, drop, family="mha"):
    return SimpleNamespace(name=name, B=B, Tq=Tq, Tk=Tk, H=H, dh=dh, dm=H * dh, layout=layout, mask=mask, drop=drop, family=family)


CASES = {c.name: c for c in (
    _case("limits_self", 2, 64, 64, 2, 64, "packed", "causal", 0.3),
    _case("wide_heads", 2, 64, 64, 10, 32, "packed", None, 0.1),
    _case("one_token", 3, 1, 1, 1, 1, "packed", None, 0.0),
    _case("one_key", 2, 63, 1, 3, 6, "cross", None, 0.1),
    _case("one_query", 2, 1, 64, 3, 24, "cross", "staggered", 0.0),
    _case("ragged_cross", 2, 33, 17, 3, 24, "cross", "staggered", 0.5),
    _case("odd_blocks", 2, 7, 5, 3, 6, "odd", "staggered", 0.3),
    _case("peaked", 2, 33, 17, 3, 24, "cross", "staggered", 0.5, family="mha_peaked"),
    _case("shifted", 2, 9, 12, 2, 16, "cross", None, 0.0, family="mha_shifted"),
    _case("dropped_row_and_column", 2, 10, 10, 4, 16, "packed", "causal", 0.3),
    _case("floor_mask_row", 2, 6, 4, 2, 8, "cross", "floor", 0.0),
)}
TABLE = list(CASES)

DROPPED_ROW = (1, 2, 7)      # (sample, head, query) of dropped_row_and_column whose keep row is 0
DROPPED_COLUMN = (0, 3, 0)   # (sample, head, key) whose keep column is 0 (key 0: the one every causal row attends to)
FLOOR_ROW = 2

ATTN_BWD_CASES = [(3, 64, 10, 32), (2, 64, 1, 64), (2, 33, 3, 24), (1, 1, 1, 1), (2, 7, 3, 6)]
COLSUM_CASES = [(1, 1, 1), (63, 65, 65), (64, 64, 64), (65, 130, 130), (70, 33, 40), (4097, 33, 33)]


def tolerance(family: str) -> float:
    return FACTOR * YARDSTICK[family]


def _draw(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).float()


def mask_of(case):
    """The additive (Tq, Tk) fp32 mask of a case, or None."""
    if case.mask is None:
        return None
    i, j = torch.meshgrid(torch.arange(case.Tq), torch.arange(case.Tk), indexing="ij")
    allowed = (i >= j) if case.mask == "causal" else (i >= j - 1)
    if case.mask == "floor":
        allowed[FLOOR_ROW] = False
    m = torch.zeros(case.Tq, case.Tk).masked_fill(~allowed, float("-inf"))
    if case.mask == "floor":
        m = m.clamp_min(torch.finfo(torch.float32).min)
    return m


def inputs(case):
    """-> q (B Tq, dm), k, v (B Tk, dm), dout (B Tq, dm), mask (Tq, Tk) | None, keep (B, H, Tq, Tk) | None: fp32 CPU tensors, seeded by
    the case's position in the table."""
    gen = torch.Generator().manual_seed(1000 + TABLE.index(case.name))
    q, k, v = _draw(gen, case.B * case.Tq, case.dm), _draw(gen, case.B * case.Tk, case.dm), _draw(gen, case.B * case.Tk, case.dm)
    dout = _draw(gen, case.B * case.Tq, case.dm)
    keep = None
    if case.drop:
        keep = (torch.rand(case.B, case.H, case.Tq, case.Tk, generator=gen) >= case.drop).float().div(1.0 - case.drop)
    if case.name == "peaked":
        q, k = q * 4.0, k * 4.0
    if case.name == "shifted":
        q[:, ::case.dh] = math.sqrt(100.0 * math.sqrt(case.dh))
        k[:, ::case.dh] = math.sqrt(100.0 * math.sqrt(case.dh))
    if case.name == "dropped_row_and_column":
        (b, h, i), (b2, h2, j) = DROPPED_ROW, DROPPED_COLUMN
        keep[b, h, i, :] = 0.0
        keep[b2, h2, :, j] = 0.0
    return SimpleNamespace(q=q, k=k, v=v, dout=dout, mask=mask_of(case), keep=keep)


def scores(q, k, B, H, mask=None):
    """q k^T / sqrt(dh) + mask -> (B, H, Tq, Tk) in the operands' dtype."""
    dh = q.shape[1] // H
    qh, kh = (z.reshape(B, -1, H, dh).transpose(1, 2) for z in (q, k))
    sc = qh @ kh.transpose(-1, -2) / dh ** 0.5
    return sc if mask is None else sc + mask.to(sc.dtype)


def attention_core(q, k, v, dout, B, H, mask, keep, dtype):
    """softmax(q k^T / sqrt(dh) + mask) o keep @ v and autograd's dq, dk, dv for `dout`, in `dtype` on the CPU."""
    q, k, v = (z.detach().cpu().to(dtype).requires_grad_(True) for z in (q, k, v))
    p = torch.softmax(scores(q, k, B, H, mask), dim=-1)
    if keep is not None:
        p = p * keep.to(dtype)
    out = (p @ v.reshape(B, -1, H, v.shape[1] // H).transpose(1, 2)).transpose(1, 2).reshape(-1, q.shape[1])
    out.backward(dout.to(dtype))
    return SimpleNamespace(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def reference(case, dtype=torch.float64, dropout=True):
    """The case in `dtype` on the CPU: float64 is the reference, float32 the yardstick run.  `dropout` False: without `keep`."""
    x = inputs(case)
    return attention_core(x.q, x.k, x.v, x.dout, case.B, case.H, x.mask, x.keep if dropout else None, dtype)


def attn_bwd_inputs(shape):
    """-> qkv (B T, 3 dm), dout (B T, dm) of an ATTN_BWD_CASES entry."""
    B, T, H, dh = shape
    gen = torch.Generator().manual_seed(2000 + ATTN_BWD_CASES.index(shape))
    return _draw(gen, B * T, 3 * H * dh), _draw(gen, B * T, H * dh)


def attn_bwd_reference(shape, dtype=torch.float64):
    """-> d qkv (B T, 3 dm) in `dtype`."""
    B, T, H, dh = shape
    qkv, dout = attn_bwd_inputs(shape)
    r = attention_core(*qkv.chunk(3, dim=1), dout, B, H, None, None, dtype)
    return torch.cat([r.dq, r.dk, r.dv], dim=1)


def colsum_input(shape):
    """-> the (R, C) fp32 matrix of a COLSUM_CASES entry."""
    R, C, ld = shape
    return _draw(torch.Generator().manual_seed(3000 + COLSUM_CASES.index(shape)), R, C)


def colsum_sequential_fp32(x):
    """The plainest order of the same sum: one fp32 accumulator per column, rows in order."""
    acc = torch.zeros(x.shape[1], dtype=torch.float32)
    for r in range(x.shape[0]):
        acc += x[r]
    return acc


def error(got, want) -> float:
    """max |got - want| / max(1, max |want|); inf when `got` is not finite where `want` is."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - want).abs().max()) / max(1.0, float(want.abs().max()))


def errors(got, ref) -> dict:
    return {t: error(getattr(got, t), getattr(ref, t)) for t in TENSORS}


def worst(errs: dict):
    k = max(errs, key=lambda n: errs[n])
    return k, errs[k]
