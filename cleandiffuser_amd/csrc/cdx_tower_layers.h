// cdx_tower_layers.h -- the forward and the backward-data body of a Linear -> [LayerNorm] -> activation tower on one 16-row tile, once
// for the kernels that run them: cdx_tower_fwd_kernel / cdx_tower_bwd_kernel (cdx_tower.hip: a training forward, which saves what the
// backward reads, and that backward), cdx_score_select_kernel (cdx_select.hip: the critic in front of the candidate selection, which keeps
// the last layer's image only) and cdx_critic_step_kernel (cdx_critic_step.hip: target, forward, loss and backward-data of a critic step in
// one launch, P_l and rstd_l staying in LDS) and cdx_regress_step_kernel (cdx_regress_step.hip: the same for an MSE step against a given
// target, a last width up to 64).  Forward, per layer: z = h W^T + b (ro_product<false>); with a norm, 16 lanes per row take the
// mean and then the biased variance of the centred values over the row in LDS (two passes, a fixed butterfly), xhat = (z - mean) rstd,
// y = xhat gamma + beta; h = act(y).  Backward, per layer from the top: y from the saved P_l (xhat or z), dy = dH act'(y), with a norm
// g = dy gamma, dz = rstd (g - mean(g) - xhat mean(g xhat)) and the tile's column sums of dy and dy xhat (rows in order), then
// dH_{l-1} = dz W_l on the live weight (ro_product<true>).  Host side (the end of the file): the admission of the layers' sizes, shared by
// the entry points of these files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"

namespace {

__device__ __forceinline__ float tw_act(int act, float y) {
    switch (act) {
        case CDX_ACT_MISH: return cdx_act_mish(y);
        case CDX_ACT_SILU: return cdx_act_silu(y);
        case CDX_ACT_RELU: return cdx_act_relu(y);
        case CDX_ACT_TANH: return cdx_act_tanh(y);
        default: return y;
    }
}
__device__ __forceinline__ float tw_act_grad(int act, float y) {
    switch (act) {
        case CDX_ACT_MISH: return cdx_act_mish_grad(y);
        case CDX_ACT_SILU: return cdx_act_silu_grad(y);
        case CDX_ACT_RELU: return cdx_act_relu_grad(y);
        case CDX_ACT_TANH: return cdx_act_tanh_grad(y);
        default: return 1.0f;
    }
}
// the sum over the 16 lanes of a row (tid >> 4): a butterfly, the same bits in every lane
__device__ __forceinline__ float tw_sum16(float v) {
    v += __shfl_xor(v, 8, 16);
    v += __shfl_xor(v, 4, 16);
    v += __shfl_xor(v, 2, 16);
    v += __shfl_xor(v, 1, 16);
    return v;
}

// what a kernel that saves nothing hands to tw_forward_layers
struct TwKeepNothing {
    __device__ void element(int, int, int, float, float) const {}
    __device__ void row_rstd(int, int, float) const {}
};

// The n_layers layers of tower `t` of request `g` (any struct with the per-layer fields of cdx_tower: width, norm, act, eps, w, b,
// gamma, beta) on the tile `in` [16][ld_in] of K0 columns, zero up to the next multiple of 16.  Layer l writes its h into
// img[l & 1] [16][ld] (zero padding is not needed behind it: every width but the last is a multiple of 16 and the last feeds no
// product); the caller finds the tower's output in img[(n_layers - 1) & 1].  save.element(l, r, c, h, p) is called once for every
// element of every layer (tile row r, column c; p = xhat of a normed layer, else z), save.row_rstd(l, r, rstd) once per row of a normed
// layer: what reaches global memory, and for which rows, is the caller's.  Called by all 256 threads behind a barrier that covers `in`;
// ends with a barrier.
template <class G, class Save>
__device__ __forceinline__ void tw_forward_layers(const G& g, int t, int K0, const float* in, int ld_in, float* img0, float* img1, int ld,
                                                  int tid, int lane, int wave, Save save) {
    const int rr = tid >> 4, sub = tid & 15;          // the norm's view: 16 lanes per row
    const float* src = in;
    int ld_src = ld_in;
    for (int l = 0; l < g.n_layers; ++l) {
        const int W = g.width[l], K = l ? g.width[l - 1] : K0, act = g.act[l];
        const float* bias = g.b[t][l];
        float* dst = (l & 1) ? img1 : img0;
        if (!g.norm[l]) {
            ro_product<false>(src, ld_src, g.w[t][l], K, W, K, lane, wave, [&](int r, int n, float v) {
                const float z = v + bias[n];
                const float h = tw_act(act, z);
                dst[r * ld + n] = h;
                save.element(l, r, n, h, z);
            });
            __syncthreads();
        } else {
            ro_product<false>(src, ld_src, g.w[t][l], K, W, K, lane, wave, [&](int r, int n, float v) { dst[r * ld + n] = v + bias[n]; });
            __syncthreads();
            const float* gamma = g.gamma[t][l];
            const float* beta = g.beta[t][l];
            float* zr = dst + rr * ld;
            float s = 0.f;
            for (int c = sub; c < W; c += 16) s += zr[c];
            const float mean = tw_sum16(s) / (float)W;
            float q = 0.f;
            for (int c = sub; c < W; c += 16) {
                const float d = zr[c] - mean;
                q += d * d;
            }
            const float rstd = 1.0f / sqrtf(tw_sum16(q) / (float)W + g.eps[l]);
            for (int c = sub; c < W; c += 16) {
                const float xhat = (zr[c] - mean) * rstd;
                const float h = tw_act(act, xhat * gamma[c] + beta[c]);
                zr[c] = h;
                save.element(l, rr, c, h, xhat);
            }
            if (sub == 0) save.row_rstd(l, rr, rstd);
            __syncthreads();
        }
        src = dst;
        ld_src = ld;
    }
}

// The backward-data pass of tower `t` of request `g` (the per-layer fields of cdx_tower) on one tile: img[0] [16][ld] holds dH of the
// last layer (zero in the rows past the batch and up to the next multiple of 16 past its width), img[1] is scratch.  What the forward
// kept and where the results go is the caller's:
//   saved.p(l, r, c)            P_l of tile row r (xhat of a normed layer, else z), 0 for a row past the batch;
//   saved.rstd(l, r)            rstd_l of that row, 0 past the batch;
//   sink.element(l, r, c, dz)   G_l, once per element (the sink drops rows past the batch);
//   sink.sums(l, c, sb, sg)     the tile's sums of dy and dy xhat over its 16 rows in order, once per column of a normed layer;
//   sink.gx(r, n, v)            g_x = dz_0 W_0, once per element.
// `params`: call element / sums at all; `want_gx`: run the last product.  Called by all 256 threads behind a barrier that covers
// img[0]; ends without one.
template <class G, class Saved, class Sink>
__device__ __forceinline__ void tw_backward_layers(const G& g, int t, int K0, float* img0, float* img1, int ld, int tid, int lane, int wave,
                                                   bool params, bool want_gx, Saved saved, Sink sink) {
    const int rr = tid >> 4, sub = tid & 15;
    int cur = 0;
    for (int l = g.n_layers - 1; l >= 0; --l) {
        const int W = g.width[l], K = l ? g.width[l - 1] : K0, act = g.act[l];
        float* d = cur ? img1 : img0;                 // dH_l, then dy, then dz: the A operand of the transposed product
        float* o = cur ? img0 : img1;                 // xhat of a normed layer, then dH_{l-1}
        float* dr = d + rr * ld;
        if (!g.norm[l]) {
            for (int c = sub; c < W; c += 16) {
                const float z = saved.p(l, rr, c);
                const float dz = dr[c] * tw_act_grad(act, z);
                dr[c] = dz;
                if (params) sink.element(l, rr, c, dz);
            }
            __syncthreads();
        } else {
            const float* gamma = g.gamma[t][l];
            const float* beta = g.beta[t][l];
            float* xr = o + rr * ld;
            const float rs = saved.rstd(l, rr);
            float s1 = 0.f, s2 = 0.f;
            for (int c = sub; c < W; c += 16) {
                const float xh = saved.p(l, rr, c);
                const float dy = dr[c] * tw_act_grad(act, xh * gamma[c] + beta[c]);
                const float gg = dy * gamma[c];
                s1 += gg;
                s2 += gg * xh;
                dr[c] = dy;
                xr[c] = xh;
            }
            s1 = tw_sum16(s1) / (float)W;
            s2 = tw_sum16(s2) / (float)W;
            __syncthreads();
            if (params) {                             // the tile's share of the shift / gain gradients: its 16 rows in order
                for (int c = tid; c < W; c += 256) {
                    float sb = 0.f, sg = 0.f;
                    for (int r = 0; r < RO_ROWS; ++r) {
                        const float dy = d[r * ld + c];
                        sb += dy;
                        sg += dy * o[r * ld + c];
                    }
                    sink.sums(l, c, sb, sg);
                }
            }
            __syncthreads();
            for (int c = sub; c < W; c += 16) {
                const float dz = rs * (dr[c] * gamma[c] - s1 - xr[c] * s2);
                dr[c] = dz;
                if (params) sink.element(l, rr, c, dz);
            }
            __syncthreads();
        }
        if (l == 0) {
            if (want_gx) ro_product<true>(d, ld, g.w[t][0], K, K, W, lane, wave, [&](int r, int n, float v) { sink.gx(r, n, v); });
        } else {
            ro_product<true>(d, ld, g.w[t][l], K, K, W, lane, wave, [&](int r, int n, float v) { o[r * ld + n] = v; });
            __syncthreads();
            cur ^= 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the layers a tower kernel takes; *maxw: the widest of them, up to the next multiple of 16
template <class Fail>
int tw_check_layers(int n_layers, const int32_t* width, const int32_t* norm, const int32_t* act, const float* eps, int* maxw, Fail fail) {
    if (n_layers < 1 || n_layers > CDX_TOWER_MAX_LAYERS) return fail("n_layers must be 1 .. CDX_TOWER_MAX_LAYERS");
    *maxw = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int w = width[l];
        if (l == n_layers - 1) {
            if (w <= 0 || w > RO_MAX_X) return fail("the last width must be 1 .. 64");
        } else if (w <= 0 || w % 16 != 0 || w > RO_MAX_WIDTH) {
            return fail("every width but the last must be a multiple of 16, at most 512");
        }
        const int a = act[l];
        if (a != CDX_ACT_NONE && a != CDX_ACT_MISH && a != CDX_ACT_SILU && a != CDX_ACT_RELU && a != CDX_ACT_TANH)
            return fail("activation must be none, mish, silu, relu or tanh");
        if (norm[l] && !(eps[l] > 0.f)) return fail("eps must be positive");
        *maxw = ro_r16(w) > *maxw ? ro_r16(w) : *maxw;
    }
    return CDX_OK;
}

}  // namespace
