"""The host paths of the four GEMM executors (csrc/cdx_bigbatch.hip: ``cdx_dit1d_run``, ``cdx_chitf_run``, ``cdx_pearcetf_run``,
``cdx_resmlp_run``) against float64, over the shapes of tests/executor_shape_cases.py: widths that are no multiple of 4 (every adaLN
offset unaligned, the launchers off their float4 variants), one token, the token limits, head_dim 64 and odd ones, depth 0, chunks of
2, 2 and 1 samples, the classifier-free pair with one trajectory in its last chunk.  A wrong stride, period or `b0` in those host
paths gives plausible numbers, not a fault; the float64 run alone tells them apart (tests/test_executor_shape_cases_cpu.py).

Every case goes through the public route -- ``net(x, t, cond)`` or ``agent.sample`` -> ``dispatch`` -> ``bigbatch`` -- and is checked for

* route: exactly one ``bigbatch._run`` request of the family, n_steps 0 (forward) or 2 (sample), with the chunk the case overrides or,
  without an override, one that holds the whole batch; a refusal makes no request and the stock module serves it;
* value: against the float64 CPU run (one per case and process) within 4 x YARDSTICK[family], relative to max(1, max |x64|), as rtol
  and as atol.  YARDSTICK is the largest error of the fp32 CPU run against the float64 one over the family's cases; the factor 4 is the
  margin of tests/test_gpu_solver_step.py for the other summation order and FMA contraction of the device GEMMs.  Nothing here is
  derived from a device result;
* workspace: ``bigbatch._workspace`` hands out a view of a larger buffer, pre-filled with 1e30 -- finite, so a masked-out lane times an
  exact zero stays zero, but a stale value that feeds a result is a huge error and not last run's plausible leftovers -- and followed by
  256 sentinel floats past the ``workspace_floats`` the library asked for, which must be untouched afterwards;
* determinism: a second identical call gives the same bits.

Measured on an MI355X, largest device error per family against its tolerance: DiT 3.16e-6 of 1.2e-5 (dit_t1), ChiTransformer 6.16e-6
of 1.4e-5 (chitf_enc2_fwd), PearceTransformer 2.23e-6 of 1.0e-5 (ptf_pair), residual MLP 2.41e-6 of 6.0e-6 (mlp_h33_pair), the refusals
on the stock modules at most 1.94e-6; the 29 cases take 5 s.  DESIGN.md, "Executor shapes against float64", has the host-path changes
the sweep was seen to notice."""
import pytest
import torch

import executor_shape_cases as E
from test_gpu_solver_step import _spy_loops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON, SENTINEL, N_SENTINELS = 1e30, -12345.0, 256


def _guard_workspace(monkeypatch):
    """Every workspace request as (buffer, floats asked for): the executor gets buffer[:floats], poisoned; the sentinels follow it."""
    from cleandiffuser_amd.engine import bigbatch
    handed = []

    def workspace(device, floats):
        buf = torch.full((int(floats) + N_SENTINELS,), POISON, dtype=torch.float32, device=device)
        buf[int(floats):] = SENTINEL
        handed.append((buf, int(floats)))
        return buf[:int(floats)]
    monkeypatch.setattr(bigbatch, "_workspace", workspace)
    return handed


def _run(name, monkeypatch):
    from cleandiffuser_amd.engine import bigbatch
    c = E.CASES[name]
    with monkeypatch.context() as m:
        m.setitem(bigbatch.CHUNK_OVERRIDE, "dit" if c.family == "pearcetf" else c.family, c.chunk)     # (bigbatch.FAMILIES: `override`)
        calls, handed = _spy_loops(m), _guard_workspace(m)
        x = E.device_run(name, DEV)
        torch.cuda.synchronize()
    for buf, floats in handed:
        assert bool((buf[floats:] == SENTINEL).all()), "the executor wrote past the workspace_floats it asked for"
    return x, calls, handed


@pytest.mark.parametrize("name", E.TABLE)
def test_executor_matches_float64(name, monkeypatch):
    c, ref = E.CASES[name], E.reference(name)
    x, calls, handed = _run(name, monkeypatch)
    if c.refused:
        assert calls == [] and handed == [], "the executor served a request past its limit"
    else:
        assert len(calls) == 1 and len(handed) == 1, f"exactly one native call must serve the request, got {calls}"
        kind, n_steps, chunk = calls[0]
        assert (kind, n_steps) == (c.family, 2 if c.mode == "sample" else 0)
        if c.chunk is not None:
            assert chunk == c.chunk
        else:
            assert chunk >= c.batch, "the default chunk rule holds this batch in one chunk"
    tol, scale = E.tolerance(name), max(1.0, float(ref.x.abs().max()))
    assert x.dtype == torch.float32 and x.shape == ref.x.shape
    err = float((x.double().cpu() - ref.x).abs().max()) / scale
    print(f"\n{name}: device error {err:.3e} of the scale {scale:.3f} (tolerance {tol:.1e})")
    assert torch.isfinite(x).all()
    torch.testing.assert_close(x.double().cpu(), ref.x, rtol=tol, atol=tol * scale)
    again, calls2, _ = _run(name, monkeypatch)
    assert calls2 == calls
    assert torch.equal(again, x), "a second identical call gives other bits"
