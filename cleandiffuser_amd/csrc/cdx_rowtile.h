// cdx_rowtile.h -- what the row-tile kernels share (cdx_rollout.hip, cdx_energy.hip, cdx_cep.hip, cdx_tower.hip, cdx_select.hip, cdx_critic_step.hip, cdx_regress_step.hip; cdx_energy_mlp.h and cdx_tower_layers.h build on it): one
// workgroup of 4 wave64 owns 16 rows, activations live in LDS, weights are read from global memory (L2-resident, the same for every
// workgroup), products run on v_mfma_f32_16x16x4_f32 (exact fp32, rows on the M axis; lane maps: cdx_probe_mfma_layout).  Device side: the
// product routine, the tile strides and loader, and what the sampling kernels need to run the solver step of cdx_step.h on their (16 x A) state
// tile.  Host side (the end of the file): the size limits, the failure helper, the admission of step records and the one launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "cdx_step.h"

extern void cdx_set_err(const char* msg);

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RO_ROWS = 16;      // rows of a tile = the M side of one 16x16x4 MFMA
constexpr int RO_XLD = 64;       // row stride of a (16 x A) state / prediction / gradient tile (A <= 64)
constexpr int RO_ALD = 68;       // row stride of such a tile when it is an MFMA A operand: padded against bank conflicts, zero past A

__host__ __device__ inline int ro_r16(int v) { return (v + 15) & ~15; }

// four consecutive k of one weight column n (zero outside the matrix).  TRANS = false: the weight is (N, K) row-major (nn.Linear.weight
// in a forward product), TRANS = true: (K, N) row-major (the same tensor in the transposed product of the backward pass: 16 lanes x 4 B
// are one 64-B segment of a weight row).
template <bool TRANS>
__device__ __forceinline__ float4 ro_wload(const float* __restrict__ w, int ldw, int n, int kb, int N, int K, bool vec) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n >= N || kb >= K) return b;
    if (!TRANS) {
        const float* p = w + (size_t)n * ldw + kb;
        if (vec) return *reinterpret_cast<const float4*>(p);           // (K % 4 == 0: kb + 3 < K)
        b.x = p[0];
        if (kb + 1 < K) b.y = p[1];
        if (kb + 2 < K) b.z = p[2];
        if (kb + 3 < K) b.w = p[3];
    } else {
        const float* p = w + (size_t)kb * ldw + n;
        b.x = p[0];
        if (kb + 1 < K) b.y = p[ldw];
        if (kb + 2 < K) b.z = p[2 * (size_t)ldw];
        if (kb + 3 < K) b.w = p[3 * (size_t)ldw];
    }
    return b;
}

// out[i][n] = sum_k in[i][k] * Wt(k, n) for the 16 rows of the tile: `in` is an LDS image [16][ld], zero up to the next multiple of 16
// past K.  The ceil(N / 16) column tiles go round the 4 waves, four of them at a time per wave (independent accumulators behind one A
// operand).  A K block of 16 is four MFMAs: lane (j = lane & 15, g = lane >> 4) feeds k = kc + 4 g + t to instruction t on BOTH sides
// (A: in[j][k], B: Wt(k, n0 + j)) -- the order of the sum inside a block is free as long as the two operands agree.  The result comes
// back as D[4 g + r][n0 + j] in register r: ep(row, column, value) is called for every column < N.
template <bool TRANS, class Ep>
__device__ __forceinline__ void ro_product(const float* in, int ld, const float* __restrict__ w, int ldw, int N, int K, int lane, int wave,
                                           Ep ep) {
    const int j = lane & 15, g = lane >> 4;
    const int n_tiles = (N + 15) >> 4;
    const int K16 = (K + 15) & ~15;
    const bool vec = !TRANS && (K & 3) == 0 && (ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    for (int t0 = wave; t0 < n_tiles; t0 += 16) {
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < K16; kc += 16) {
            const int kb = kc + 4 * g;
            const float4 a = *reinterpret_cast<const float4*>(in + j * ld + kb);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (t0 + 4 * q < n_tiles) {                               // (wave-uniform)
                    const float4 b = ro_wload<TRANS>(w, ldw, (t0 + 4 * q) * 16 + j, kb, N, K, vec);
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc[q], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = (t0 + 4 * q) * 16 + j;
            if (t0 + 4 * q < n_tiles && n < N) {
#pragma unroll
                for (int r = 0; r < 4; ++r) ep(4 * g + r, n, acc[q][r]);
            }
        }
    }
}

// rows [row0, row0 + 16) of the row-major (.., C) matrix `src` as an MFMA A operand t [16][ld]: columns [0, fill) are written, zero past
// C and past row `rows`; src_row(row) is the row of `src` behind row `row` of the batch.  No barrier.
template <class Row, class SrcRow>
__device__ __forceinline__ void ro_load_rows(float* t, int ld, int fill, const float* __restrict__ src, int C, Row row0, Row rows, int tid,
                                             SrcRow src_row) {
    for (int i = tid; i < RO_ROWS * fill; i += 256) {
        const int rr = i / fill, c = i - rr * fill;
        const Row row = row0 + rr;
        t[rr * ld + c] = (c < C && row < rows) ? src[(size_t)src_row(row) * C + c] : 0.f;
    }
}

// what a row-tile kernel carries of a cdx_step in its argument block (the entry points admit kinds 0-2 with vsel <= 1 and no flags:
// no multistep memory, no push, k[4] unused)
struct RowStep {
    int32_t kind, vsel, noise_idx;
    float alpha, sigma, k0, k1, k2, k3;
    static RowStep of(const cdx_step& st) {
        return RowStep{st.kind, st.vsel, st.noise_idx, st.alpha, st.sigma, st.k[0], st.k[1], st.k[2], st.k[3]};
    }
    __device__ cdx_step record() const { return cdx_step{kind, vsel, noise_idx, 0, alpha, sigma, {k0, k1, k2, k3, 0.f}, 0}; }
};

// cdx_step_element()'s view of element e of batch row `row`: bounds and mask (A), prior (B, A) and noise (n_noise, B, A) in global
// memory; rows of the tile past the batch read noise and prior as 0
struct RowStepIO {
    const float *lo, *hi, *fix_mask, *prior_rows, *noise_rows;
    int B, A, row, e;
    __device__ bool has_min() const { return lo != nullptr; }
    __device__ bool has_max() const { return hi != nullptr; }
    __device__ bool has_mask() const { return fix_mask != nullptr; }
    __device__ float x_min() const { return lo[e]; }
    __device__ float x_max() const { return hi[e]; }
    __device__ float mask() const { return fix_mask[e]; }
    __device__ float prior() const { return row < B ? prior_rows[(size_t)row * A + e] : 0.f; }
    __device__ float noise(int idx) const { return row < B ? noise_rows[((size_t)idx * B + row) * A + e] : 0.f; }
    __device__ float prev() const { return 0.f; }
    __device__ float xold() const { return 0.f; }
    __device__ void push(float) const {}
    __device__ void push_edm(float, float) const {}
};

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
constexpr int RO_MAX_X = 64, RO_MAX_EMB = 128, RO_MAX_WIDTH = 512, RO_MAX_CONCAT = 1024;   // A; E, Ec; a layer's width, O, A + E + O; in + in2

// "<entry point>: <what>" -> cdx_last_error(), CDX_EINVAL
inline int ro_fail(const char* who, const char* what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    cdx_set_err(msg);
    return CDX_EINVAL;
}

// the step records a row-tile kernel takes (RowStep): kinds 0-2 without multistep memory, no flags, noise there when a step draws it
template <class Fail>
int ro_check_steps(const cdx_step* steps, int S, bool has_noise, Fail fail) {
    for (int i = 0; i < S; ++i) {
        const cdx_step& st = steps[i];
        if (st.kind < 0 || st.kind > 2) return fail("step kind must be 0, 1 or 2");
        if (st.vsel < 0 || st.vsel > 1) return fail("step vsel must be 0 or 1 (no multistep memory)");
        if (st.flags != 0) return fail("step flags are not supported");
        if (st.noise_idx >= 0 && !has_noise) return fail("step draws noise but noise == NULL");
    }
    return CDX_OK;
}

// one workgroup of 256 threads per 16 rows (times `grid_y`: the twin towers of cdx_tower.hip); `raised` is the kernel's own high-water
// mark of the attribute that admits > 48 KiB of LDS
template <class Args>
int ro_launch_tiles(void (*kernel)(Args), const Args& args, long long rows, size_t lds, void* hip_stream, size_t& raised,
                    unsigned grid_y = 1) {
    if (lds > 48 * 1024 && lds > raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
        raised = lds;
    }
    const dim3 grid((unsigned)((rows + RO_ROWS - 1) / RO_ROWS), grid_y);
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), args);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
    return CDX_OK;
}

}  // namespace
