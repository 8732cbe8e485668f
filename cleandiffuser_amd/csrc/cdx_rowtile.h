// cdx_rowtile.h -- the product routine of the row-tile kernels (cdx_rollout.hip, cdx_energy.hip): one workgroup of 4 wave64 owns 16 rows,
// activations live in LDS, weights are read from global memory (L2-resident, the same for every workgroup), products run on
// v_mfma_f32_16x16x4_f32 (exact fp32, rows on the M axis; lane maps: cdx_probe_mfma_layout); and what both need to run the solver step
// of cdx_step.h on their (16 x A) state tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cdx_step.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RO_ROWS = 16;      // rows of a tile = the M side of one 16x16x4 MFMA

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

}  // namespace
