"""What the program compiler (engine/program2.py) emits, pinned bit for bit on the CPU.

The whole output of that module is integers and copied floats (nothing beyond exact copies and ``0 + bias``), so a program has a
portable fingerprint: sha256 of ``ops_buffer`` and of ``blob``, ``ops.shape``, every scalar field of ``Program2``, ``embtab`` /
``embtabs`` in full and ``meta`` (scalars in full, tensors and arrays as sha256).  A case that refuses records its ``ValueError``
text.  The fingerprints must equal, exactly, the ones in ``program2_fingerprints_cpu.json``; regenerate that file with
``CDX_RECORD_FINGERPRINTS=1 python tests/test_program2_fingerprints_cpu.py`` only when a program is MEANT to change.

Which case reaches which branch of ``_Builder2.conv`` (traced when the file was recorded):

* the fuse refusal (an extra conv next to a main conv whose K slices are longer than ``fuse_max``; the block falls back to two
  ops): the ``janner_n32_nw*``, ``janner_n3_nw*`` and ``janner_n64_nw*`` cases, ``chiunet_*_nw4_compact``, ``classifier_c32``,
  ``guided_n32_c32``, ``guided_n32_c32_two_traj``, ``guided_n64_c64_save_global``;
* the grouped-op fallback (a grouped candidate whose row tiles do not come out as whole lane groups becomes an ordinary op):
  ``group_small_k2_min1024``;
* ``single_round`` (skip streams as first-round items next to ring-aligned main slices) and the SIMD dealing that follows it:
  ``group_n32_k2_*``, ``group_n32_k4_*``, ``group_w64_k4_min1024``, ``guided_group_k2`` / ``guided_group_k4`` (and
  ``group_n64_k2_*`` before it refuses);
* ``uneven`` (the two-slice cut, one ring revolution shorter for the wave that also draws a skip item): ``group_n32_k4_*``,
  ``group_w64_k4_min1024``, ``guided_group_k4`` (and the ``group_n64_*`` cases before they refuse);
* the multi-phase path (``ConvTranspose1d`` as two phases; the stride-2 scatter of the classifier's backward): every Janner /
  ChiUNet case with more than one resolution, and the guided cases;
* ``col_norm`` / ``cg_real``: ``mlp_pearce64`` / ``mlp_pearce256`` (per-sample GroupNorm), ``mlp_pearce192`` (padded groups:
  ``W2_CGREAL4`` set);
* ``film``: ``chiunet_film_nw8`` / ``chiunet_film_nw4_compact`` (``cond_predict_scale``).
"""
import dataclasses
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cleandiffuser_amd.engine import program2 as P2  # noqa: E402
from cleandiffuser_amd.utils import load_synth  # noqa: E402
from oracle import cases as _oracle_cases  # noqa: E402

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "program2_fingerprints_cpu.json")


@functools.lru_cache(maxsize=None)
def _lib():
    return _oracle_cases.lib_namespace("amd")


@functools.lru_cache(maxsize=None)
def _janner(d, md, dm, k=5, seed=0):
    return load_synth(_lib().JannerUNet1d(d, model_dim=md, emb_dim=32, dim_mult=list(dm), kernel_size=k), seed).eval()


@functools.lru_cache(maxsize=None)
def _clf(h, d, md, dm):
    return load_synth(_lib().HalfJannerUNet1d(h, d, out_dim=1, model_dim=md, emb_dim=32, dim_mult=tuple(dm), kernel_size=3), 1).eval()


@functools.lru_cache(maxsize=None)
def _chi(scale):
    return load_synth(_lib().ChiUNet1d(6, 10, 2, model_dim=32, emb_dim=32, dim_mult=[1, 2, 2], kernel_size=5,
                                       cond_predict_scale=scale, obs_as_global_cond=True), 3).eval()


@functools.lru_cache(maxsize=None)
def _mlp(kind):
    import torch.nn as nn
    lib = _lib()
    return {
        "pearce64": lambda: load_synth(lib.PearceMlp(6, To=2, emb_dim=32, hidden_dim=64), 1),
        "pearce192": lambda: load_synth(lib.PearceMlp(6, To=1, emb_dim=64, hidden_dim=192), 7),
        "pearce256": lambda: load_synth(lib.PearceMlp(6, To=1, emb_dim=64, hidden_dim=256), 2),
        "sfbc": lambda: load_synth(lib.SfBCUNet(4, emb_dim=32, hidden_dims=[128, 64, 64]), 6),
        "dql": lambda: load_synth(lib.DQLMlp(11, 3, emb_dim=16), 3),
        "dvinv": lambda: load_synth(lib.DVInvMlp(5, 3, emb_dim=16, hidden_dim=128), 4),
        "mlpnn": lambda: load_synth(lib.MlpNNDiffusion(5, emb_dim=16, hidden_dims=[64, 128], activation=nn.SiLU()), 5),
    }[kind]().eval()


NETS = {"n32": ((6, 32, (1, 2, 2, 2), 5, 0), 32), "n64": ((69, 64, (1, 2, 2, 2), 5, 9), 32),
        "n3": ((6, 32, (1, 2, 4), 5, 9), 16), "n16": ((6, 16, (1, 2), 3, 0), 16)}
CLFS = {"c32": (32, 6, 32, (1, 2, 2, 2)), "c16": (16, 6, 32, (1, 2)), "c64": (32, 69, 64, (1, 2, 2, 2))}
MLP_COMPILERS = {"pearce64": "compile_pearce_mlp2", "pearce192": "compile_pearce_mlp2", "pearce256": "compile_pearce_mlp2",
                 "sfbc": "compile_sfbc_unet2", "dql": "compile_dql_mlp2", "dvinv": "compile_dql_mlp2", "mlpnn": "compile_mlp_nn2"}

CASES = {}          # name -> (GROUP_MIN_BYTES, thunk -> Program2)


def _case(name, thunk, gmin=None):
    assert name not in CASES
    CASES[name] = (gmin, thunk)


for _n, (_spec, _h) in NETS.items():
    for _nw in (4, 8):
        for _compact in (False, True):
            _case(f"janner_{_n}_nw{_nw}" + ("_compact" if _compact else ""),
                  lambda s=_spec, h=_h, nw=_nw, c=_compact: P2.compile_janner2(_janner(*s), h, nw=nw, compact=c))
_case("janner_n32_no4x4", lambda: P2.compile_janner2(_janner(*NETS["n32"][0]), 32, allow_4x4=False))
_case("janner_n32_nw8_stage2304", lambda: P2.compile_janner2(_janner(*NETS["n32"][0]), 32, nw=8, max_stage=2304))
for _n in ("n32", "n64"):
    for _k in (2, 4):
        for _gmin in (None, 65536):
            _tag = f"{_n}_k{_k}_min{_gmin}"
            _case("split_" + _tag, lambda s=NETS[_n][0], k=_k: P2.compile_janner2_split(_janner(*s), 32, k), _gmin)
            _case("group_" + _tag, lambda s=NETS[_n][0], k=_k: P2.compile_janner2_group(_janner(*s), 32, k), _gmin)
_case("group_w64_k4_min1024", lambda: P2.compile_janner2_group(_janner(6, 64, (1, 2, 2)), 16, 4), 1024)
_case("group_small_k2_min1024", lambda: P2.compile_janner2_group(_janner(6, 32, (1, 2)), 8, 2), 1024)

_G32 = lambda: (_janner(*NETS["n32"][0]), _clf(*CLFS["c32"]))      # noqa: E731
_case("guided_n32_c32", lambda: P2.compile_guided2(*_G32(), 32))
_case("guided_n32_c32_two_traj", lambda: P2.compile_guided2(*_G32(), 32, save_global=True, max_stage=2304, max_lds_bytes=80 * 1024))
_case("guided_small_c16_compact", lambda: P2.compile_guided2(_janner(6, 32, (1, 2)), _clf(*CLFS["c16"]), 16, compact=True))
_case("guided_n64_c64_save_global", lambda: P2.compile_guided2(_janner(*NETS["n64"][0]), _clf(*CLFS["c64"]), 32, save_global=True))
for _k in (2, 4):
    _case(f"guided_split_k{_k}", lambda k=_k: P2.compile_guided2_split(*_G32(), 32, k))
    _case(f"guided_group_k{_k}", lambda k=_k: P2.compile_guided2_group(*_G32(), 32, k))
_case("classifier_c32", lambda: P2.compile_classifier2(_clf(*CLFS["c32"]), 32))
for _scale in (False, True):
    _tag = "chiunet_film" if _scale else "chiunet_add"
    _case(_tag + "_nw8", lambda s=_scale: P2.compile_chiunet2(_chi(s), 16, nw=8))
    _case(_tag + "_nw4_compact", lambda s=_scale: P2.compile_chiunet2(_chi(s), 16, nw=4, compact=True))
for _kind, _fn in MLP_COMPILERS.items():
    _case("mlp_" + _kind, lambda kind=_kind, fn=_fn: getattr(P2, fn)(_mlp(kind), 16))


def _sha(a, dtype) -> str:
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a), dtype=dtype).tobytes()).hexdigest()


def _plain(v):
    """meta / embtab values: scalars in full, tensors and arrays as sha256, containers element by element."""
    if isinstance(v, torch.Tensor):
        return {"sha256": _sha(v.detach().cpu().numpy(), np.float32 if v.is_floating_point() else np.int64), "shape": list(v.shape)}
    if isinstance(v, np.ndarray):
        return {"sha256": _sha(v, np.int32 if v.dtype.kind in "iu" else np.float32), "shape": list(v.shape)}
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    raise TypeError(f"no fingerprint for a {type(v).__name__}")


def fingerprint(prog) -> dict:
    fp = {"ops_buffer": _sha(prog.ops_buffer, np.int32), "blob": _sha(prog.blob.detach().cpu().numpy(), np.float32),
          "ops_shape": list(prog.ops.shape)}
    for f in dataclasses.fields(prog):
        v = getattr(prog, f.name)
        if isinstance(v, (bool, int, float)):
            fp[f.name] = v
    fp["embtab"], fp["embtabs"], fp["meta"] = _plain(prog.embtab), _plain(prog.embtabs), _plain(prog.meta)
    return fp


def _record(name):
    gmin, thunk = CASES[name]
    saved = P2.GROUP_MIN_BYTES
    P2.GROUP_MIN_BYTES = gmin
    try:
        return fingerprint(thunk())
    except ValueError as e:
        return {"refused": str(e)}
    finally:
        P2.GROUP_MIN_BYTES = saved


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as f:
        return json.load(f)


def test_every_case_is_recorded(expected):
    assert sorted(expected) == sorted(CASES)
    refused = sorted(n for n, fp in expected.items() if "refused" in fp)
    assert refused == sorted(n for n in CASES if n.startswith(("split_n64_k4", "group_n64")))


@pytest.mark.parametrize("name", sorted(CASES))
def test_program_fingerprint_is_unchanged(name, expected):
    assert json.loads(json.dumps(_record(name))) == expected[name]


def test_refused_fuse_leaves_no_trace():
    """A conv with an `extra` that the builder declines to fuse answers False and has emitted nothing: no blob chunk, no MAC count, no
    op, no staging area -- the caller lowers the block as two ops instead."""
    b = P2._Builder2(torch.device("cpu"), 8)
    b.fuse_max = 0
    g = torch.Generator().manual_seed(0)
    src, t1, out = b.act(8, 32), b.act(8, 64), b.act(8, 64)
    before = (b.blob_len, len(b.chunks), b.macs, len(b.ops), len(b.op_acts), len(b.op_items), len(b.op_item_src), b.stage)
    ok = b.conv([t1], out, torch.randn(64, 5, 64, generator=g), torch.randn(64, generator=g), pad=2, gn=torch.nn.GroupNorm(8, 64),
                extra=[dict(srcs=[src], w_eff=torch.randn(64, 1, 32, generator=g), pad=0, bias=torch.randn(64, generator=g), post=True)])
    assert ok is False
    assert (b.blob_len, len(b.chunks), b.macs, len(b.ops), len(b.op_acts), len(b.op_items), len(b.op_item_src), b.stage) == before
    b.fuse_max = 1 << 30
    assert b.conv([t1], out, torch.randn(64, 5, 64, generator=g), None, pad=2, gn=torch.nn.GroupNorm(8, 64),
                  extra=[dict(srcs=[src], w_eff=torch.randn(64, 1, 32, generator=g), pad=0, bias=None, post=True)]) is True
    assert len(b.ops) == 1 and b.blob_len > before[0] and b.stage > 0


if __name__ == "__main__":
    if os.environ.get("CDX_RECORD_FINGERPRINTS") != "1":
        sys.exit("set CDX_RECORD_FINGERPRINTS=1 to overwrite " + os.path.basename(EXPECTED))
    out = {name: _record(name) for name in sorted(CASES)}
    with open(EXPECTED, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(out)} programs, {sum('refused' in fp for fp in out.values())} of them refusals")
