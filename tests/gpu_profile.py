"""torch.profiler over a region of a GPU test, and the device kernels it launched."""
import re

import pytest
import torch


def profiled(body, activities=None, rerun=True, skip=True):
    """torch.profiler over ``body()`` -> (profiler, body's result).  roctracer occasionally hands the profiler NO device activity for a
    region (one full-suite run in ~25 this round: every kernel name missing, only the host-side ops listed).  A test that asserts on
    kernel names then has nothing to look at: the region is profiled once more where running it again is harmless (`rerun`), else the
    test is skipped rather than failed for a tracing dropout -- or, `skip` False, gets (None, body's result): what it asserts about
    the RESULT must not depend on the tracer."""
    from torch.profiler import profile, ProfilerActivity
    acts = activities or [ProfilerActivity.CPU, ProfilerActivity.CUDA]
    for attempt in range(2 if rerun else 1):
        with profile(activities=acts) as prof:
            out = body()
            torch.cuda.synchronize()
        if any(e.device_time_total > 0 for e in prof.key_averages()):
            return prof, out
    if not skip:
        return None, out
    pytest.skip("torch.profiler recorded no device activity for this region (roctracer dropout)")


def kernel_names(prof):
    """The names of the device kernels a profiled region launched, as roctracer demangles them (``void cdx_gemm_kernel<true, 2, false,
    8>(cdx_gemm_args, int, int, int)``) without the return type and whitespace: ``cdx_gemm_kernel<true,2,false,8>(cdx_gemm_args,...)``."""
    return {"".join(re.sub(r"^void\s+", "", e.key).split()) for e in prof.key_averages() if e.device_time_total > 0}


def missing(names, wanted):
    """Those of `wanted` (``kernel`` or ``kernel<template arguments>``, no whitespace) that none of `names` is an instantiation of."""
    def hit(w):
        pat = re.compile(r"(?<![\w])" + re.escape(w) + ("" if w.endswith(">") else r"(?![\w<])"))
        return any(pat.search(n) for n in names)
    return [w for w in wanted if not hit(w)]
