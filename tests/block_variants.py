"""Which kernel instantiations the launchers of the building blocks can pick (csrc/cdx_gemm.hip, csrc/cdx_train.hip), as three tables:

GUARDED        per family, the instantiations a default process reaches.  The GPU tier runs every family's unit-test cases under the
               profiler and requires each name among the launched kernels (tests/test_gpu_blocks.py, the coverage guard).
EXCLUDED       instantiations only a non-default hook or a library-internal entry reaches, with that hook.  The hooks are read once per
               process, so a test cannot switch them.
UNCONDITIONAL  kernels whose entry point has nothing to choose: ONE launch site in the sources, whatever the shape (the CPU check counts
               the sites; a second one means a launcher has begun to choose and the kernel belongs under GUARDED).

tests/test_block_variants_cpu.py reads the launch sites out of the sources and fails when they and these tables disagree -- a new
instantiation needs a unit-test case that reaches it (or a documented reason why none can)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cleandiffuser_amd", "csrc")
SOURCES = ("cdx_gemm.hip", "cdx_train.hip")

GUARDED = {
    # <unguarded float4 loads, 1 = 64 x 64 tile | 2 = 128 x 128, implicit conv, waves>
    "gemm": ["cdx_gemm_kernel<true,1,false,4>", "cdx_gemm_kernel<true,1,true,4>", "cdx_gemm_kernel<false,1,false,4>",
             "cdx_gemm_kernel<false,1,true,4>", "cdx_gemm_kernel<true,2,false,8>", "cdx_gemm_kernel<true,2,true,8>",
             "cdx_gemm_kernel<false,2,false,4>", "cdx_gemm_kernel<false,2,true,4>"],
    "splitk_reduce": ["gm_splitk_reduce_kernel<true>", "gm_splitk_reduce_kernel<false>"],
    "layernorm": ["cdx_layernorm_vec_kernel<4>", "cdx_layernorm_vec_kernel<8>", "cdx_layernorm_vec_kernel<16>",
                  "cdx_layernorm_kernel<16>", "cdx_layernorm_kernel<32>", "cdx_layernorm_kernel<64>"],
    "layernorm_bwd": ["cdx_layernorm_bwd_kernel<16>", "cdx_layernorm_bwd_kernel<32>", "cdx_layernorm_bwd_kernel<64>"],
    "groupnorm": ["cdx_groupnorm_vec_kernel<false>", "cdx_groupnorm_kernel"],
    "groupnorm_bwd": ["cdx_groupnorm_bwd_vec_kernel<true>", "cdx_groupnorm_bwd_vec_kernel<false>", "cdx_groupnorm_bwd_kernel<true>",
                      "cdx_groupnorm_bwd_kernel<false>"],
    "attention": ["cdx_attention_long_kernel", "cdx_attention_mfma_kernel<1,1>", "cdx_attention_mfma_kernel<1,2>",
                  "cdx_attention_mfma_kernel<2,1>", "cdx_attention_mfma_kernel<2,2>", "cdx_attention_kernel"],
    "cross_attention": [f"cdx_cross_attention_vec_kernel<{gl}>" for gl in (1, 2, 4, 8, 16, 32, 64)] + ["cdx_cross_attention_kernel"],
}

EXCLUDED = {
    "cdx_gemm_kernel<true,2,false,4>": "CDX_GEMM_W8=0 (A/B hook: the 4-wave shape of the unguarded 128 x 128 tile)",
    "cdx_gemm_kernel<true,2,true,4>": "CDX_GEMM_W8=0 (A/B hook: the 4-wave shape of the unguarded 128 x 128 tile)",
    "cdx_groupnorm_vec_kernel<true>": "cdx_groupnorm_slices_f32, library-internal: the split-K conv + GroupNorm pair of the sampling "
                                      "executors (csrc/cdx_bigbatch.hip), covered by the whole-network fixtures",
}

UNCONDITIONAL = ["cdx_act_kernel", "cdx_act_bwd_kernel", "cdx_mha_train_kernel<true>", "cdx_mha_train_kernel<false>", "cdx_relayout_kernel",
                 "cdx_conv_wgrad_kernel", "cdx_conv_wgrad_batch_kernel", "cdx_colsum_kernel", "cdx_gather_kernel"]

_KERNEL = re.compile(r"\b((?:cdx|gm)_\w+_kernel)\b\s*(<[^<>()]*>)?")
_LITERAL = re.compile(r"true|false|\d+")


def launched(text: str):
    """The kernel instantiations named outside kernel definitions in a .hip source: hipLaunchKernelGGL sites, kernels picked into a
    variable first, and the uses of the GM_LAUNCH / GM_LAUNCH8 macros of gm_launch (default wave count: 4) -> {instantiation: number
    of places that name it}.  A kernel named with template or macro arguments that are no literals -- a launcher written in a way this
    reader cannot follow -- is an error, not something to pass over."""
    found = {}
    for line in text.splitlines():
        line = line.split("//")[0]
        if "__global__" in line or line.lstrip().startswith("#define"):
            continue
        line = re.sub(r"reinterpret_cast<const void\*>\([^()]*\)", "", line)      # (a kernel's address for hipFuncSetAttribute: no launch)
        for name, targs in _KERNEL.findall(line):
            args = [a.strip() for a in targs[1:-1].split(",")] if targs else []
            if not all(_LITERAL.fullmatch(a) for a in args):
                raise ValueError(f"cannot tell which instantiation is launched here (template arguments that are no literals): {line.strip()}")
            if name == "cdx_gemm_kernel" and len(args) == 3:
                args.append("4")
            key = name + ("<" + ",".join(args) + ">" if args else "")
            found[key] = found.get(key, 0) + 1
        for macro, args in re.findall(r"\b(GM_LAUNCH8?)\(([^()]*)\)", line):
            args = [a.strip() for a in args.split(",")]
            if len(args) != (3 if macro == "GM_LAUNCH" else 1) or not all(_LITERAL.fullmatch(a) for a in args):
                raise ValueError(f"cannot tell which instantiation is launched here (macro arguments that are no literals): {line.strip()}")
            key = f"cdx_gemm_kernel<{args[0]},{args[1]},{args[2]},4>" if macro == "GM_LAUNCH" else f"cdx_gemm_kernel<true,2,{args[0]},8>"
            found[key] = found.get(key, 0) + 1
    return found


def launch_sites():
    out = {}
    for f in SOURCES:
        with open(os.path.join(CSRC, f)) as fh:
            for k, n in launched(fh.read()).items():
                out[k] = out.get(k, 0) + n
    return out
