"""CPU tier: the tables of tests/block_variants.py against the launch sites in the sources.  The GPU coverage guard can only require
what is listed; this check makes the list follow the launchers."""
import block_variants as V


def test_every_launched_instantiation_is_guarded_or_has_a_documented_reason():
    counts = V.launch_sites()
    sites = set(counts)
    guarded = {k for names in V.GUARDED.values() for k in names}
    known = guarded | set(V.EXCLUDED) | set(V.UNCONDITIONAL)
    assert len(sites) > 40, sites                        # (the reader found the launch sites at all)
    assert not sites - known, f"launched in csrc but in no table of tests/block_variants.py: {sorted(sites - known)}"
    assert not known - sites, f"listed in tests/block_variants.py but launched nowhere: {sorted(known - sites)}"
    assert not guarded & set(V.EXCLUDED) and not guarded & set(V.UNCONDITIONAL)
    assert all(reason.strip() for reason in V.EXCLUDED.values())
    assert {k: counts[k] for k in V.UNCONDITIONAL} == {k: 1 for k in V.UNCONDITIONAL}      # nothing chooses them: one site each


def test_the_reader_sees_macros_picked_variables_and_skips_definitions_and_comments():
    text = """
    template <bool F> __global__ void cdx_a_kernel(int x) {}
    __global__ void cdx_b_kernel(int x) {}       // cdx_c_kernel<3> in a comment
    #define GM_LAUNCH(F, W, C) hipLaunchKernelGGL((cdx_gemm_kernel<F, W, C>), grid)
    if (v) { if (c) GM_LAUNCH(true, 2, true); else GM_LAUNCH(false, 1, false); }
    GM_LAUNCH8(false);
    auto kern = c <= 1024 ? cdx_a_kernel<true> : cdx_a_kernel< false >;
    hipLaunchKernelGGL(cdx_b_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(s), 1);
    """
    assert V.launched(text) == {"cdx_gemm_kernel<true,2,true,4>": 1, "cdx_gemm_kernel<false,1,false,4>": 1, "cdx_gemm_kernel<true,2,false,8>": 1,
                                "cdx_a_kernel<true>": 1, "cdx_a_kernel<false>": 1, "cdx_b_kernel": 1}
    import pytest
    for bad in ("hipLaunchKernelGGL(cdx_a_kernel<FAST>, grid, block, 0, s, 1);", "if (v) GM_LAUNCH(vec, 2, true);", "MY_LAUNCH(cdx_a_kernel<W>);"):
        with pytest.raises(ValueError, match="no literals"):
            V.launched(bad)
