"""Recorded results of the real reference for the tests that compare this package against it on random settings.

The reference tree is only importable in the build container; the tests read what it computed from small fixtures under
``tests/golden/ref_records/`` instead, so that they run wherever the repository is checked out.  ``result(key, tag, fn)``:

* ``CDX_RECORD_REFERENCE=1`` (reference importable): runs ``fn()`` -- the reference side of the comparison -- and (re)writes the record;
* otherwise: returns the record.  ``tag`` describes the drawn setting and must equal the recorded one, so a change of the draw code
  cannot silently compare against a stale record.

``fn()`` returns a dict of arrays / numbers / nested dicts and lists of them, or raises; a raise is recorded as the exception's type
name and replayed as an instance of that type (builtins, or the type ``fn`` raised when it is importable by name).

Re-recording (where the reference tree is importable):
    CDX_RECORD_REFERENCE=1 python -m pytest -m "not gpu" tests/test_solver_settings_vs_reference.py \\
        tests/test_training_settings_vs_reference.py tests/test_dataset_settings_vs_reference.py tests/test_plugin_custom_backbone.py"""
import builtins
import importlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "ref_records")


def recording() -> bool:
    return os.environ.get("CDX_RECORD_REFERENCE") == "1"


def _flatten(obj, prefix, out):
    if isinstance(obj, dict):
        out[prefix + "#d"] = np.array(list(obj.keys()), dtype=np.str_)
        for i, (k, v) in enumerate(obj.items()):
            _flatten(v, f"{prefix}/{i}", out)
    elif isinstance(obj, (list, tuple)):
        out[prefix + "#l"] = np.array(len(obj))
        for i, v in enumerate(obj):
            _flatten(v, f"{prefix}/{i}", out)
    elif isinstance(obj, (bool, np.bool_)):
        out[prefix + "#b"] = np.array(bool(obj))
    elif isinstance(obj, (int, np.integer)):
        out[prefix + "#i"] = np.array(int(obj), dtype=np.int64)
    elif isinstance(obj, (float, np.floating)):
        out[prefix + "#f"] = np.array(float(obj), dtype=np.float64)
    elif isinstance(obj, str):
        out[prefix + "#s"] = np.array(obj, dtype=np.str_)
    else:
        out[prefix + "#a"] = np.asarray(obj)


def _unflatten(z, prefix):
    for kind in ("d", "l", "b", "i", "f", "s", "a"):
        if prefix + "#" + kind in z.files:
            v = z[prefix + "#" + kind]
            if kind == "d":
                return {str(k): _unflatten(z, f"{prefix}/{i}") for i, k in enumerate(v.tolist())}
            if kind == "l":
                return [_unflatten(z, f"{prefix}/{i}") for i in range(int(v))]
            if kind == "b":
                return bool(v)
            if kind == "i":
                return int(v)
            if kind == "f":
                return float(v)
            if kind == "s":
                return str(v)
            return v
    raise KeyError(prefix)


def _exception_type(qualname):
    mod, _, name = qualname.rpartition(".")
    if mod in ("", "builtins"):
        return getattr(builtins, name)
    return getattr(importlib.import_module(mod), name)


def result(key: str, tag: str, fn):
    path = os.path.join(DIR, key + ".npz")
    if recording():
        rec = {"tag": np.array(tag, dtype=np.str_)}
        try:
            value = fn()
        except Exception as e:  # noqa: BLE001 -- recorded, then re-raised for the caller
            t = type(e)
            rec["raises"] = np.array(("" if t.__module__ == "builtins" else t.__module__ + ".") + t.__qualname__, dtype=np.str_)
            os.makedirs(DIR, exist_ok=True)
            np.savez_compressed(path, **rec)
            raise
        _flatten(value, "v", rec)
        os.makedirs(DIR, exist_ok=True)
        np.savez_compressed(path, **rec)
        return value
    with np.load(path) as z:
        assert str(z["tag"]) == tag, f"stale reference record {key}: recorded for {str(z['tag'])!r}, drawn {tag!r}"
        if "raises" in z.files:
            raise _exception_type(str(z["raises"]))(f"the reference rejected this setting (recorded in {key})")
        return _unflatten(z, "v")
