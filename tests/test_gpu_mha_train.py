"""The training step's attention core (``cdx_mha_train_kernel<false|true>`` in csrc/cdx_train.hip behind ``blocks.mha_train``,
``blocks.attention_backward`` and ``train._MHA``) and the row-sum kernels ``cdx_colsum_f32`` / ``cdx_gather_windows_f32`` against
float64: every case of tests/mha_train_cases.py on the device, compared with the float64 CPU reference of the same ops
(``mha_train_cases.reference``, which tests/test_mha_train_cases_cpu.py holds against ``F.multi_head_attention_forward``).

Tolerance: FACTOR = 4 x YARDSTICK[family] in E = max |a - b| / max(1, max |b|) per tensor.  YARDSTICK is the error of the same ops in
fp32 on the CPU against float64; nothing here is derived from a device result.

Every output and gradient buffer is pre-filled with a sentinel, stale device memory is poisoned with NaN first, and in `odd_blocks`
(operands and gradients as column blocks at column 3 of 41-float rows, first element 20 bytes into its allocation) the operands'
matrices hold NaN outside the blocks and the gradients' matrices must still hold the sentinel there afterwards.

`floor_mask_row`: a query row whose mask entries all sit at ``finfo(float32).min``.  torch gives the uniform row.  The kernel stored its
scores unclamped and started the row maximum at -3.0e38, so every exp(-3.4e38 + 3.0e38) of that row was 0, the sum 0 and the row
0 x inf: on the device this case FAILED before the fix (see "Measured" below), with NaN in out, dq, dk and dv of the masked rows.
The scores are now clamped at -3.0e38 where they are stored, as in the sampling attention kernels.

Measured on an MI355X, largest device E per family (tolerance): mha 6.81e-7, wide_heads dq (3.2e-6); mha_shifted 1.09e-5, out
(4.8e-5); mha_peaked 1.24e-6, dk (4.8e-6) -- ``__expf`` in the row softmax stays, the peaked rows are no further from float64 than
the fp32 CPU run; attention_backward 5.42e-7 (2.4e-6); column sums 1.43e-7 at 4097 rows (4.0e-6): 16-row thread sums, then 4-way LDS,
then atomics across slices is a shorter chain than the row-by-row yardstick's; gather_windows exact.  The figures follow the fp32 CPU
run's almost digit for digit.  `floor_mask_row` before the clamp: out 32, dq 32, dk 128, dv 128 NaN elements (the masked row of both
samples in out and dq, everything in dk and dv, which sum over the query rows); after it 7.7e-8 / 7.3e-8 / 1.5e-7 / 9.5e-8.
`pytest -s` prints every figure."""
import ctypes

import pytest
import torch

import mha_train_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
NAN = float("nan")
EINVAL = -1                            # CDX_EINVAL (include/cdx.h)


def _poison():
    torch.full((1 << 22,), NAN, device=DEV)                # whatever stale memory the kernel might touch is poisoned first


def _odd(rows, dm, fill, block=None):
    """A (rows, dm) column block at column ODD_COL of a (rows, ODD_LD) matrix that starts ODD_OFF floats into `flat`; the rest of
    `flat` holds `fill`.  -> flat, block view, the boolean map of `flat`'s elements outside the block."""
    flat = torch.full((M.ODD_OFF + rows * M.ODD_LD + M.ODD_OFF,), fill, device=DEV)
    wide = flat[M.ODD_OFF:M.ODD_OFF + rows * M.ODD_LD].view(rows, M.ODD_LD)
    view = wide[:, M.ODD_COL:M.ODD_COL + dm]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == M.ODD_LD
    if block is not None:
        view.copy_(block)
    outside = torch.ones_like(flat, dtype=torch.bool)
    outside[M.ODD_OFF:M.ODD_OFF + rows * M.ODD_LD].view(rows, M.ODD_LD)[:, M.ODD_COL:M.ODD_COL + dm] = False
    return flat, view, outside


def _operands(case, x):
    """The case's operands and sentinel-filled gradient views on the device, laid out the way the table says.
    -> (q, k, v), (dq, dk, dv), check(): asserts that nothing outside the gradient blocks was written."""
    dm, rq, rk = case.dm, case.B * case.Tq, case.B * case.Tk
    if case.layout == "packed":
        qkv = torch.cat([x.q, x.k, x.v], dim=1).to(DEV)
        g = torch.full((rq, 3 * dm), SENTINEL, device=DEV)
        return tuple(qkv[:, i * dm:(i + 1) * dm] for i in range(3)), tuple(g[:, i * dm:(i + 1) * dm] for i in range(3)), lambda: None
    if case.layout == "cross":
        kv = torch.cat([x.k, x.v], dim=1).to(DEV)
        dq, dkv = torch.full((rq, dm), SENTINEL, device=DEV), torch.full((rk, 2 * dm), SENTINEL, device=DEV)
        return (x.q.to(DEV), kv[:, :dm], kv[:, dm:]), (dq, dkv[:, :dm], dkv[:, dm:]), lambda: None
    assert case.layout == "odd"
    ops = [_odd(rows, dm, NAN, t.to(DEV)) for rows, t in ((rq, x.q), (rk, x.k), (rk, x.v))]
    grads = [_odd(rows, dm, SENTINEL) for rows in (rq, rk, rk)]

    def check():
        for name, (flat, _, outside) in zip(("dq", "dk", "dv"), grads):
            assert bool((flat[outside] == SENTINEL).all()), f"{name}: a write outside its column block"
        for name, (flat, view, outside) in zip("qkv", ops):
            assert bool(torch.isnan(flat[outside]).all()) and not bool(torch.isnan(view).any()), f"{name}: an operand was written"
    return tuple(o[1] for o in ops), tuple(g[1] for g in grads), check


def _device_run(case, forward=True, backward=True):
    from types import SimpleNamespace
    from cleandiffuser_amd.engine import blocks
    x = M.inputs(case)
    _poison()
    (q, k, v), grads, check = _operands(case, x)
    mask = None if x.mask is None else x.mask.to(DEV)
    keep = None if x.keep is None else x.keep.to(DEV)
    got = SimpleNamespace(out=None, dq=None, dk=None, dv=None)
    if forward:
        out = torch.full((case.B * case.Tq, case.dm), SENTINEL, device=DEV)
        assert blocks.mha_train(q, k, v, case.B, case.H, mask=mask, keep=keep, out=out) is out
        got.out = out
    if backward:
        res = blocks.mha_train(q, k, v, case.B, case.H, mask=mask, keep=keep, dout=x.dout.to(DEV), grads=grads)
        assert all(r is g for r, g in zip(res, grads))
        got.dq, got.dk, got.dv = grads
    torch.cuda.synchronize()
    check()
    return got


@pytest.fixture(scope="module")
def ref64():
    return {name: M.reference(case) for name, case in M.CASES.items()}


def _compare(name, got, ref, tensors=M.TENSORS):
    case = M.CASES[name]
    tol = M.tolerance(case.family)
    errs = {t: M.error(getattr(got, t), getattr(ref, t)) for t in tensors}
    n_nan = {t: int(torch.isnan(getattr(got, t)).sum()) for t in tensors}
    print(f"\n{name}: device error " + ", ".join(f"{t} {e:.2e}" for t, e in errs.items()) + f" (tolerance {tol:.1e})" +
          (f"; NaN elements {n_nan}" if any(n_nan.values()) else ""))
    k, w = M.worst(errs)
    assert w <= tol, (name, k, w)


@pytest.mark.parametrize("name", M.TABLE)
def test_forward_and_backward_match_float64(name, ref64):
    case, ref = M.CASES[name], ref64[name]
    got = _device_run(case)
    _compare(name, got, ref)
    if name == "one_key":
        assert float(got.dq.abs().max()) == 0.0 and float(got.dk.abs().max()) == 0.0
    if name == "dropped_row_and_column":
        (b, h, i), (b2, h2, j) = M.DROPPED_ROW, M.DROPPED_COLUMN
        assert float(got.out.view(case.B, case.Tq, case.H, case.dh)[b, i, h].abs().max()) == 0.0
        assert float(got.dv.reshape(case.B, case.Tk, case.H, case.dh)[b2, j, h2].abs().max()) == 0.0
    if name == "floor_mask_row":
        x = M.inputs(case)
        uniform = x.v.double().view(case.B, case.Tk, case.dm).mean(1)
        assert M.error(got.out.view(case.B, case.Tq, case.dm)[:, M.FLOOR_ROW], uniform) <= M.tolerance(case.family)


@pytest.mark.parametrize("name", ["limits_self", "ragged_cross"])
def test_autograd_wrappers_return_gradients_packed_like_the_operands(name, ref64):
    from types import SimpleNamespace
    from cleandiffuser_amd.engine import train
    case, ref, x = M.CASES[name], ref64[name], M.inputs(M.CASES[name])
    dm = case.dm
    _poison()
    mask, keep = x.mask.to(DEV), x.keep.to(DEV)
    if case.layout == "packed":
        qkv = torch.cat([x.q, x.k, x.v], dim=1).to(DEV).requires_grad_(True)
        out = train._MHA.apply(qkv, None, case.B, case.H, mask, keep)
        out.backward(x.dout.to(DEV))
        assert qkv.grad.shape == qkv.shape
        got = SimpleNamespace(out=out.detach(), dq=qkv.grad[:, :dm], dk=qkv.grad[:, dm:2 * dm], dv=qkv.grad[:, 2 * dm:])
    else:
        q = x.q.to(DEV).requires_grad_(True)
        kv = torch.cat([x.k, x.v], dim=1).to(DEV).requires_grad_(True)
        out = train._MHA.apply(q, kv, case.B, case.H, mask, keep)
        out.backward(x.dout.to(DEV))
        assert q.grad.shape == q.shape and kv.grad.shape == kv.shape
        got = SimpleNamespace(out=out.detach(), dq=q.grad, dk=kv.grad[:, :dm], dv=kv.grad[:, dm:])
    torch.cuda.synchronize()
    _compare(name, got, ref)


def test_backward_lds_attribute_is_raised_in_any_order(ref64):
    """67 KB, then 99.8 KB, then 67 KB again: the launcher raises the kernel's dynamic-LDS limit only when a launch needs more than any
    before it (the static ``raised[]``), and a smaller launch after a larger one must still be launched and correct."""
    for name in ("wide_heads", "limits_self", "wide_heads"):
        _compare(name, _device_run(M.CASES[name], forward=False), ref64[name], tensors=("dq", "dk", "dv"))


@pytest.mark.parametrize("shape", M.ATTN_BWD_CASES)
def test_attention_backward_matches_float64(shape):
    from cleandiffuser_amd.engine import blocks
    B, T, H, dh = shape
    qkv, dout = M.attn_bwd_inputs(shape)
    _poison()
    got = blocks.attention_backward(qkv.to(DEV), dout.to(DEV), B, T, H)
    torch.cuda.synchronize()
    e, tol = M.error(got, M.attn_bwd_reference(shape)), M.tolerance("attn_bwd")
    print(f"\nattention_backward {shape}: device error {e:.2e} (tolerance {tol:.1e})")
    assert got.shape == qkv.shape and e <= tol


def _raw_args(B=2, Tq=8, Tk=8, H=2, dh=8):
    """A valid argument block on sentinel-filled buffers large enough for every shape the refusals try (<= 65 of each)."""
    from cleandiffuser_amd.engine import blocks
    n = 4 * 65 * 2 * 65
    bufs = {k: torch.full((n,), SENTINEL, device=DEV) for k in ("q", "k", "v", "out", "dout", "dq", "dk", "dv")}
    dm = H * dh
    a = blocks.CdxMhaTrainArgs(**{k: t.data_ptr() for k, t in bufs.items()}, B=B, Tq=Tq, Tk=Tk, n_heads=H, head_dim=dh, ldq=dm, ldk=dm,
                               ldv=dm, ldo=dm, lddq=dm, lddk=dm, lddv=dm, scale=float(dh) ** -0.5)
    return a, bufs


@pytest.mark.parametrize("change,text", [(dict(Tq=65), b"<= 64"), (dict(Tk=65), b"<= 64"), (dict(head_dim=65), b"<= 64"),
                                         (dict(ldq=15), b"row stride"), (dict(dout=None), b"null pointer"), (dict(B=0), b"")])
def test_refusals_write_nothing(change, text):
    from cleandiffuser_amd.engine import blocks
    lib = blocks._lib()
    want = 0 if change == dict(B=0) else EINVAL
    for fn in (lib.cdx_mha_train_fwd_f32, lib.cdx_mha_train_bwd_f32):
        if "dout" in change and fn is lib.cdx_mha_train_fwd_f32:
            continue                                       # (the forward does not read dout)
        a, bufs = _raw_args()
        for k, val in change.items():
            setattr(a, k, val)
        assert fn(ctypes.byref(a), None) == want and text in lib.cdx_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in bufs.values()), change


@pytest.mark.parametrize("shape", M.COLSUM_CASES)
def test_colsum_adds_onto_out_and_matches_float64(shape):
    from cleandiffuser_amd.engine import blocks
    R, C, ld = shape
    x = M.colsum_input(shape)
    _poison()
    wide = torch.full((R, ld), NAN, device=DEV)
    xd = wide[:, ld - C:]                                  # (the LAST C columns: every other column of the source is NaN)
    xd.copy_(x)
    assert (xd.stride(0) == ld or R == 1) and (ld == C or bool(torch.isnan(wide[:, :ld - C]).all()))
    out = torch.full((C + 2,), M.COLSUM_START, device=DEV)
    assert blocks.colsum(xd, out=out[1:1 + C]).data_ptr() == out[1:].data_ptr()
    torch.cuda.synchronize()
    assert float(out[0]) == M.COLSUM_START and float(out[-1]) == M.COLSUM_START
    e, tol = M.error(out[1:1 + C].double().cpu() - M.COLSUM_START, x.double().sum(0)), M.tolerance("colsum")
    print(f"\ncolsum {shape}: device error {e:.2e} (tolerance {tol:.1e})")
    assert e <= tol


# (width, steps) per field of one launch: segments of 256 / 255 / 529, of 257 / 23, and -- equal steps, so that one row0 is the last
# valid window of every field -- of 527 / 713 / 31 floats.  A workgroup copies a 256-float slice of a segment for 8 batch items.
GATHER_FIELDS = {"256_255_529": [(1, 256), (17, 15), (23, 23)], "257_23": [(1, 257), (23, 1)], "527_713_31": [(17, 31), (23, 31), (1, 31)]}
GATHER_ROWS = 300


@pytest.mark.parametrize("batch", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("fields", list(GATHER_FIELDS))
def test_gather_windows_equals_host_indexing(fields, batch):
    from cleandiffuser_amd.engine import blocks
    from cleandiffuser_amd.engine.runtime import _stream_ptr
    spec = GATHER_FIELDS[fields]
    gen = torch.Generator().manual_seed(batch)
    steps_max = max(s for _, s in spec)
    last = GATHER_ROWS - steps_max
    row0 = torch.randint(0, last + 1, (batch,), generator=gen, dtype=torch.int32)
    row0[-1] = last                                        # the last valid window (of every field where the steps are equal)
    if batch > 1:
        row0[0] = last if batch > 8 else 0
        row0[batch // 2] = row0[0]                         # a repeated entry
    srcs = [torch.randn(GATHER_ROWS, w, generator=gen) for w, _ in spec]
    want = [torch.stack([s[r:r + steps] for r in row0.tolist()]) for s, (_, steps) in zip(srcs, spec)]
    _poison()
    dsrc, drow0 = [s.to(DEV) for s in srcs], row0.to(DEV)
    outs = blocks.gather_windows(drow0, [(s, steps) for s, (_, steps) in zip(dsrc, spec)], GATHER_ROWS)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert o.shape == w.shape and torch.equal(o.cpu(), w)
    # the same launch into buffers of the test's own, 512 sentinel floats on either side of every output
    guard = 512
    a = blocks.CdxGatherArgs(row0=drow0.data_ptr(), batch=batch, n_fields=len(spec), rows=GATHER_ROWS)
    flats = []
    for i, (s, (w, steps)) in enumerate(zip(dsrc, spec)):
        flat = torch.full((guard + batch * steps * w + guard,), SENTINEL, device=DEV)
        a.field[i] = blocks.CdxGatherField(src=s.data_ptr(), out=flat[guard:].data_ptr(), width=w, steps=steps)
        flats.append(flat)
    assert blocks._lib().cdx_gather_windows_f32(ctypes.byref(a), _stream_ptr(torch.device(DEV))) == 0
    torch.cuda.synchronize()
    for flat, w in zip(flats, want):
        assert torch.equal(flat[guard:-guard].cpu(), w.reshape(-1))
        assert bool((flat[:guard] == SENTINEL).all()) and bool((flat[-guard:] == SENTINEL).all()), "a write outside an output"
