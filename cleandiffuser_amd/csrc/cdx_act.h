// cdx_act.h -- the per-element activation formulas of the library, one device function per CDX_ACT_* id (include/cdx.h) plus the Mish,
// SiLU, ReLU and tanh derivatives.  gm_act (cdx_gemm.hip), act2_f (cdx_unet2.hip), the rollout kernels (cdx_rollout.hip), the energy model
// of the row-tile kernels (cdx_energy_mlp.h, cdx_energy.hip) and the critic towers (cdx_tower.hip) dispatch to these.  Two use sites write their formula out instead (Mish in gm_act, GELU_ERF in act2_f): the same arithmetic, but through the call hipcc emits other
// code for the kernels around them.  A change to a formula here goes to those two as well.
#pragma once
#include <hip/hip_runtime.h>

// x * tanh(softplus(x)), tanh(log(1 + e^x)) = n / (n + 2), n = e^x (e^x + 2); softplus threshold 20 as ATen
__device__ __forceinline__ float cdx_act_mish(float x) {
    const float e = __expf(fminf(x, 20.0f));
    const float n = e * (e + 2.0f);
    return x > 20.0f ? x : x * n * __builtin_amdgcn_rcpf(n + 2.0f);
}
// d/dx [x tanh(softplus x)] = t + x (1 - t^2) sigmoid(x), t = tanh(softplus x)
__device__ __forceinline__ float cdx_act_mish_grad(float x) {
    const float e = __expf(fminf(x, 20.0f));
    const float n = e * (e + 2.0f);
    const float t = x > 20.0f ? 1.0f : n / (n + 2.0f);
    const float sg = e / (1.0f + e);
    return t + x * (1.0f - t * t) * sg;
}
// erf by Abramowitz-Stegun 7.1.26 (|err| < 1.5e-7, branch-free: libm erff costs ~4x as much in a GEMM epilogue):
// erf|x| = 1 - poly(t) e^{-x^2}, t = 1 / (1 + 0.3275911 |x|)
__device__ __forceinline__ float cdx_erf_poly(float t) {
    return t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
}
__device__ __forceinline__ float cdx_act_gelu_erf(float x) {     // exact GELU
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    const float erf_abs = 1.0f - cdx_erf_poly(t) * __expf(-z * z);
    return 0.5f * x * (1.0f + copysignf(erf_abs, x));
}
__device__ __forceinline__ float cdx_act_leaky(float x) { return x > 0.f ? x : 0.01f * x; }
__device__ __forceinline__ float cdx_act_silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// d/dx [x sigmoid(x)] = s (1 + x (1 - s)), s = sigmoid(x): the formula of cdx_act_bwd_f32
__device__ __forceinline__ float cdx_act_silu_grad(float x) {
    const float sg = 1.0f / (1.0f + __expf(-x));
    return sg * (1.0f + x * (1.0f - sg));
}
__device__ __forceinline__ float cdx_act_relu(float x) { return fmaxf(x, 0.f); }
__device__ __forceinline__ float cdx_act_relu_grad(float x) { return x > 0.f ? 1.0f : 0.f; }      // (0 at 0, as ATen's threshold_backward)
// 0.5 x (1 + tanh u) == x * sigmoid(2u): one v_exp, one v_rcp, no branches
__device__ __forceinline__ float cdx_act_gelu_tanh(float x) {
    const float u2 = 1.5957691216057308f * (x + 0.044715f * x * x * x);
    return x * __builtin_amdgcn_rcpf(1.0f + __expf(-u2));
}
// sign(x) (1 - e^{-2|x|}) / (1 + e^{-2|x|}): no overflow, no branches
__device__ __forceinline__ float cdx_act_tanh(float x) {
    const float t = __expf(-2.0f * fabsf(x));
    return copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
}
// d/dx tanh(x) = 1 - tanh^2(x) = 4 t / (1 + t)^2, t = e^{-2|x|}: no cancellation where tanh saturates
__device__ __forceinline__ float cdx_act_tanh_grad(float x) {
    const float t = __expf(-2.0f * fabsf(x));
    const float d = 1.0f + t;
    return 4.0f * t / (d * d);
}
