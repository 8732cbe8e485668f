// cdx_energy_mlp.h -- QGPONNClassifier, the energy model of QGPO (reference nn_classifier/mlp.py:25-55), on one 16-row tile: the one copy
// the guided sampling kernel (cdx_energy.hip) and the contrastive training kernel (cdx_cep.hip) both run, on ro_product of cdx_rowtile.h.
//   features  feat = [obs_proj(obs) | act_proj(x) | temb] (16 x 3 Ec), an activation image [16][ld], zero up to the next multiple of 16;
//   forward   h_l = SiLU(W_l h_{l-1} + b_l) over two alternating images, the pre-activations saved in LDS; the head o = w_o . h + b_o,
//             f = 10 tanh(o / 10) and 1 - tanh^2(o / 10);
//   backward  G_{L-1} = go w_o SiLU'(pre_{L-1}) for a per-row go = d / do, then G_{l-1} = (G_l W_l) SiLU'(pre_{l-1}) from the top down.
// Every function is called by all 256 threads of the workgroup and ends behind a barrier unless it says otherwise.  What a kernel keeps
// of a (16 x N) result it says through sink(row, column, value), called by the lane that made the element; a function that walks the
// layers takes sink_of(layer), asked once per layer for that layer's sink (so a base pointer is made outside the product).
#pragma once
#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"

namespace {

// the hidden layers and the head as both request structs carry them, and where the tile keeps them in LDS
struct EmNet {
    int L, Ec;                                  // hidden layers; the width of each of the three feature blocks
    const int32_t* hidden;                      // [L] widths
    const float* const* w;                      // [L] (hidden[l], l ? hidden[l-1] : 3 Ec)
    const float* const* b;                      // [L]
    const float *wo, *bo;                       // (1, hidden[L-1]), (1)
    float* lds; int ld;                         // image i = lds + i * 16 * ld
    const int32_t* off_pre;                     // [L] the saved pre-activations [16][hidden[l]], in floats from lds
    __device__ float* image(int i) const { return lds + (size_t)i * RO_ROWS * ld; }
};

// obs_proj of the observation tile ot [16][ld] (ro_load_rows up to the next multiple of 16 past O) -> sink.  No barrier.
template <class Sink>
__device__ __forceinline__ void em_obs_proj(const float* ot, int ld, const float* __restrict__ w, const float* __restrict__ b, int O, int Ec,
                                            int lane, int wave, Sink sink) {
    ro_product<false>(ot, ld, w, O, Ec, O, lane, wave, [&](int rr, int n, float v) { sink(rr, n, v + b[n]); });
}

// act_proj of the state tile xs [16][RO_ALD] into columns [Ec, 2 Ec) of the feature image, and to sink.  No barrier.
template <class Sink>
__device__ __forceinline__ void em_act_proj(const float* xs, float* feat, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                            int A, int Ec, int lane, int wave, Sink sink) {
    ro_product<false>(xs, RO_ALD, w, A, Ec, A, lane, wave, [&](int rr, int n, float v) {
        const float y = v + b[n];
        feat[rr * ld + Ec + n] = y;
        sink(rr, n, y);
    });
}

// the hidden layers from the feature image `src`, every activation h to sink_of(layer).  Returns the image that holds the last one.
template <class Sink>
__device__ __forceinline__ int em_forward(const EmNet& m, int src, int lane, int wave, Sink sink_of) {
    for (int l = 0; l < m.L; ++l) {
        const int W = m.hidden[l], K = l ? m.hidden[l - 1] : 3 * m.Ec;
        const float* bias = m.b[l];
        float* pre = m.lds + m.off_pre[l];
        float* dst = m.image(src ^ 1);
        auto keep = sink_of(l);
        ro_product<false>(m.image(src), m.ld, m.w[l], K, W, K, lane, wave, [&](int rr, int n, float v) {
            const float z = v + bias[n];
            const float h = cdx_act_silu(z);
            pre[rr * W + n] = z;
            dst[rr * m.ld + n] = h;
            keep(rr, n, h);
        });
        __syncthreads();
        src ^= 1;
    }
    return src;
}

// the head on the last activation in image `src`: f[16] = 10 tanh(o / 10), dt[16] = 1 - tanh^2(o / 10)
__device__ __forceinline__ void em_head(const EmNet& m, int src, float* f, float* dt, int lane, int wave) {
    const int WL = m.hidden[m.L - 1];
    ro_product<false>(m.image(src), m.ld, m.wo, WL, 1, WL, lane, wave, [&](int rr, int n, float v) {
        const float t = cdx_act_tanh((v + m.bo[0]) / 10.0f);
        f[rr] = 10.0f * t;
        dt[rr] = 1.0f - t * t;
    });
    __syncthreads();
}

// G_l = d / d pre_l from go[16] = d / do, the last hidden layer first into image `dst`, then downwards: sink_of(layer)(row, column, G).
// `wback[l]`, l >= 1, is what carries G_l to layer l - 1: TRANS = true the live weight w[l] (hidden[l], hidden[l-1]), TRANS = false its
// transposed copy (hidden[l-1], hidden[l]); both read the same elements in the same MFMA order.  Returns the image that holds G_0.
template <bool TRANS, class Sink>
__device__ __forceinline__ int em_backward(const EmNet& m, const float* const* wback, const float* go, int dst, int tid, int lane, int wave,
                                           Sink sink_of) {
    const int WL = m.hidden[m.L - 1];
    {
        const float* pre = m.lds + m.off_pre[m.L - 1];
        float* d = m.image(dst);
        auto keep = sink_of(m.L - 1);
        for (int i = tid; i < RO_ROWS * WL; i += 256) {
            const int rr = i / WL, n = i - rr * WL;
            const float v = go[rr] * m.wo[n] * cdx_act_silu_grad(pre[i]);
            d[rr * m.ld + n] = v;
            keep(rr, n, v);
        }
    }
    __syncthreads();
    int src = dst;
    for (int l = m.L - 1; l >= 1; --l) {
        const int N = m.hidden[l - 1], K = m.hidden[l];
        const float* pre = m.lds + m.off_pre[l - 1];
        float* d = m.image(src ^ 1);
        auto keep = sink_of(l - 1);
        ro_product<TRANS>(m.image(src), m.ld, wback[l], TRANS ? N : K, N, K, lane, wave, [&](int rr, int n, float v) {
            const float y = v * cdx_act_silu_grad(pre[rr * N + n]);
            d[rr * m.ld + n] = y;
            keep(rr, n, y);
        });
        __syncthreads();
        src ^= 1;
    }
    return src;
}

// ------------------------------------------------------------------------------------------------
// host side: the sizes of the net and its share of an LDS plan
// ------------------------------------------------------------------------------------------------
struct EmPlan {
    int maxw;                                    // the widest MFMA operand among the obs tile, the feature image and the hidden layers
    int32_t off_col[CDX_ENERGY_MAX_HIDDEN];      // the widths before layer l (0 past n_hidden): its saved pre-activations start 16 x that
    long long pre_floats;                        // many floats in, its matrix in a layer-major (rows, .) buffer rows x that many; the total
};

// fail(message) -> CDX_EINVAL for sizes the kernels do not take; `emb_msg` / `width_msg` are the entry point's wording of those two
template <class Fail>
int em_plan(int A, int O, int Ec, int n_hidden, const int32_t* hidden, EmPlan* p, Fail fail, const char* emb_msg, const char* width_msg) {
    if (A > RO_MAX_X) return fail("A must be at most 64");
    if (Ec > RO_MAX_EMB) return fail(emb_msg);
    if (O > RO_MAX_WIDTH) return fail("O must be at most 512");
    if (n_hidden < 1 || n_hidden > CDX_ENERGY_MAX_HIDDEN) return fail("n_hidden must be 1 .. CDX_ENERGY_MAX_HIDDEN");
    *p = EmPlan{ro_r16(O) > ro_r16(3 * Ec) ? ro_r16(O) : ro_r16(3 * Ec), {0}, 0};
    int cols = 0;
    for (int l = 0; l < n_hidden; ++l) {
        const int w = hidden[l];
        if (w <= 0 || w % 16 != 0 || w > RO_MAX_WIDTH) return fail(width_msg);
        p->maxw = w > p->maxw ? w : p->maxw;
        p->off_col[l] = cols;
        cols += w;
    }
    p->pre_floats = (long long)RO_ROWS * cols;
    return CDX_OK;
}

}  // namespace
