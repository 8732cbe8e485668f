// cdx_denoise.hip -- the denoising loss of the row-MLP denoisers (DQLMlp / DVInvMlp) in one forward and one backward launch.
//
// Diffusion-QL and EDP call ``actor.loss(act, obs)`` on every gradient step next to their Q term (reference pipelines/dql_d4rl_*.py,
// edp_d4rl_mujoco.py:97), and EDP evaluates the same net once more on a noised action (edp_d4rl_mujoco.py:100-108).  One evaluation is
//     xt = (1 - m) (a x0 + s eps) + m x0;  temb = Linear(Mish(Linear(emb0)));  feat = [xt | temb | cond]
//     -> 3 x (Linear -> Mish) -> Linear = pred;  loss = mean((pred - target)^2 lw (1 - m) wr)
// which as library nodes is ~15 launches forward and ~35 backward on 256 rows.  Rows are independent and a row's loss gradient depends on
// that row only, so
//   * cdx_denoise_fwd_f32: ONE launch, one workgroup of 4 wave64 per 16-row tile (cdx_rowtile.h), activations in LDS, weights read from
//     global memory, products on v_mfma_f32_16x16x4_f32; saves Zt, Ht, feat, Z[l], H[l], pred and the tile's share of the loss;
//   * cdx_denoise_bwd_f32: ONE launch, d loss / d pred from the loss (or the caller's rows), then the head, the trunk and the time MLP
//     transposed; G_l = d loss / d Z_l is written over Z_l (each element's Mish' is read before its G is written, by the same lane),
//     Gt over Zt.
// No atomics, one fixed lane and order per element: both kernels are bit-reproducible.  The weight / bias sums over the rows are NOT done
// here: one cdx_conv_wgrad_f32 product per layer (engine/denoise.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"

namespace {

constexpr size_t DN_MAX_LDS = 160 * 1024;

// row stride of the two activation images: the widest MFMA A operand (features, a hidden layer, the hidden layer of the time MLP)
__host__ __device__ inline int dn_ld(int A, int E, int O, int W) {
    int m = ro_r16(A + E + O);
    if (W > m) m = W;
    if (ro_r16(2 * E) > m) m = ro_r16(2 * E);
    return m + 4;
}

// two images [16][ld] and one (16 x A) tile [16][68]: the per-element loss (forward), d loss / d pred as an MFMA A operand (backward)
inline long long dn_lds(const cdx_denoise* g) {
    return (long long)sizeof(float) * ((long long)2 * RO_ROWS * dn_ld(g->A, g->E, g->O, g->W) + (long long)RO_ROWS * RO_ALD);
}

__device__ __forceinline__ float dn_target(const cdx_denoise& r, size_t i) { return r.predict_noise ? r.eps[i] : r.x0[i]; }

// (lw (1 - m) wr) of element e of row `row`
__device__ __forceinline__ float dn_weight(const cdx_denoise& r, int row, int e) {
    float w = r.lw ? r.lw[e] : 1.0f;
    if (r.fix_mask) w *= 1.0f - r.fix_mask[e];
    if (r.wr) w *= r.wr[row];
    return w;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cdx_denoise_fwd_kernel(const cdx_denoise r) {
    extern __shared__ __attribute__((aligned(16))) float dn_lds_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = r.R, A = r.A, E = r.E, O = r.O, W = r.W, F = A + E + O, F16 = ro_r16(F), E2 = 2 * E;
    const int ld = dn_ld(A, E, O, W);
    const int row0 = blockIdx.x * RO_ROWS;
    float* bufA = dn_lds_mem;                   // [16][ld]
    float* bufB = bufA + RO_ROWS * ld;          // [16][ld]
    float* lt = bufB + RO_ROWS * ld;            // [16][68] the per-element loss
    const size_t RW = (size_t)R * W;

    // time MLP: emb0 -> bufB, Ht = Mish(emb0 W_t1^T + b_t1) -> bufA (zero from 2E to the next multiple of 16)
    ro_load_rows(bufB, ld, ro_r16(E), r.emb0, E, row0, R, tid, [](int row) { return row; });
    for (int i = tid; i < RO_ROWS * (ro_r16(E2) - E2); i += 256) {
        const int rr = i / (ro_r16(E2) - E2), c = E2 + i - rr * (ro_r16(E2) - E2);
        bufA[rr * ld + c] = 0.f;
    }
    __syncthreads();
    ro_product<false>(bufB, ld, r.tw1, E, E2, E, lane, wave, [&](int rr, int n, float v) {
        const float z = v + r.tb1[n];
        const float h = cdx_act_mish(z);
        bufA[rr * ld + n] = h;
        const int row = row0 + rr;
        if (row < R) {
            r.Zt[(size_t)row * E2 + n] = z;
            r.Ht[(size_t)row * E2 + n] = h;
        }
    });
    __syncthreads();
    // features [xt | temb | cond] -> bufB, zero up to F16: the x and condition columns here, the temb columns out of the product
    for (int i = tid; i < RO_ROWS * F16; i += 256) {
        const int rr = i / F16, c = i - rr * F16, row = row0 + rr;
        if (c >= A && c < A + E) continue;
        float v = 0.f;
        if (row < R) {
            if (c < A) {
                const size_t at = (size_t)row * A + c;
                if (r.xt != nullptr) {
                    v = r.xt[at];
                } else {
                    const float x0 = r.x0[at];
                    v = r.a[row] * x0 + r.s[row] * r.eps[at];
                    if (r.fix_mask) v = (1.0f - r.fix_mask[c]) * v + r.fix_mask[c] * x0;
                }
            } else if (c < F && r.cond != nullptr) {
                v = r.cond[(size_t)row * O + (c - A - E)];
            }
            if (c < F) r.feat[(size_t)row * F + c] = v;
        }
        bufB[rr * ld + c] = v;
    }
    ro_product<false>(bufA, ld, r.tw2, E2, E, E2, lane, wave, [&](int rr, int n, float v) {
        const int row = row0 + rr;
        const float t = row < R ? v + r.tb2[n] : 0.f;
        bufB[rr * ld + A + n] = t;
        if (row < R) r.feat[(size_t)row * F + A + n] = t;
    });
    __syncthreads();
    // trunk
    float* src = bufB;
    float* dst = bufA;
    for (int l = 0; l < 3; ++l) {
        const float* w = l == 0 ? r.w1 : l == 1 ? r.w2 : r.w3;
        const float* bias = l == 0 ? r.b1 : l == 1 ? r.b2 : r.b3;
        const int K = l == 0 ? F : W;
        float* Z = r.Z + (size_t)l * RW;
        float* H = r.H + (size_t)l * RW;
        ro_product<false>(src, ld, w, K, W, K, lane, wave, [&](int rr, int n, float v) {
            const float z = v + bias[n];
            const float h = cdx_act_mish(z);
            dst[rr * ld + n] = h;
            const int row = row0 + rr;
            if (row < R) {
                Z[(size_t)row * W + n] = z;
                H[(size_t)row * W + n] = h;
            }
        });
        __syncthreads();
        float* t = src;
        src = dst;
        dst = t;
    }
    // head, and the per-element loss (rows past R carry zero)
    ro_product<false>(src, ld, r.wh, W, A, W, lane, wave, [&](int rr, int n, float v) {
        const float p = v + r.bh[n];
        const int row = row0 + rr;
        float l = 0.f;
        if (row < R) {
            const size_t at = (size_t)row * A + n;
            r.pred[at] = p;
            if (r.loss_mode) {
                const float d = p - dn_target(r, at);
                l = d * d * dn_weight(r, row, n);
            }
        }
        lt[rr * RO_ALD + n] = l;
    });
    if (!r.loss_mode) return;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.f;
        for (int rr = 0; rr < RO_ROWS; ++rr)
            for (int e = 0; e < A; ++e) sum += lt[rr * RO_ALD + e];
        r.loss_part[blockIdx.x] = sum / (float)((double)R * (double)A);
    }
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cdx_denoise_bwd_kernel(const cdx_denoise r) {
    extern __shared__ __attribute__((aligned(16))) float dn_lds_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = r.R, A = r.A, E = r.E, O = r.O, W = r.W, F = A + E + O, E2 = 2 * E;
    const int ld = dn_ld(A, E, O, W);
    const int row0 = blockIdx.x * RO_ROWS;
    float* bufA = dn_lds_mem;                   // [16][ld]
    float* bufB = bufA + RO_ROWS * ld;          // [16][ld]
    float* ghd = bufB + RO_ROWS * ld;           // [16][68] d loss / d pred, zero up to column 64 (an MFMA A operand)
    const size_t RW = (size_t)R * W;

    {
        const float scale = r.loss_mode ? 2.0f * r.g_loss[0] / (float)((double)R * (double)A) : 0.f;
        for (int i = tid; i < RO_ROWS * RO_XLD; i += 256) {
            const int rr = i / RO_XLD, e = i - rr * RO_XLD, row = row0 + rr;
            float gp = 0.f;
            if (e < A && row < R) {
                const size_t at = (size_t)row * A + e;
                gp = r.loss_mode ? scale * (r.pred[at] - dn_target(r, at)) * dn_weight(r, row, e) : r.g_pred[at];
                r.G_head[at] = gp;
            }
            ghd[rr * RO_ALD + e] = gp;
        }
    }
    __syncthreads();
    // head^T, then the hidden layers^T: G_l = (G_{l+1} W_{l+1}) * Mish'(Z_l), written over Z_l
    const float* src = ghd;
    int src_ld = RO_ALD, K = A;
    float* dst = bufA;
    for (int l = 2; l >= 0; --l) {
        const float* w = l == 2 ? r.wh : l == 1 ? r.w3 : r.w2;             // (K, W) row-major: the layer ABOVE Z_l
        float* Z = r.Z + (size_t)l * RW;
        ro_product<true>(src, src_ld, w, W, W, K, lane, wave, [&](int rr, int n, float v) {
            const int row = row0 + rr;
            float gz = 0.f;
            if (row < R) {
                gz = v * cdx_act_mish_grad(Z[(size_t)row * W + n]);
                Z[(size_t)row * W + n] = gz;
            }
            dst[rr * ld + n] = gz;
        });
        __syncthreads();
        src = dst;
        src_ld = ld;
        K = W;
        dst = dst == bufA ? bufB : bufA;
    }
    // layer 1^T: d loss / d feat = G_1 W_1 -> [x part | temb part | cond part]; the temb part -> bufB as the next A operand
    // (src == bufA, dst == bufB here)
    for (int i = tid; i < RO_ROWS * (ro_r16(E) - E); i += 256) {
        const int rr = i / (ro_r16(E) - E), c = E + i - rr * (ro_r16(E) - E);
        dst[rr * ld + c] = 0.f;
    }
    ro_product<true>(src, ld, r.w1, F, F, W, lane, wave, [&](int rr, int n, float v) {
        const int row = row0 + rr;
        if (n < A) {
            if (r.g_xt != nullptr && row < R) r.g_xt[(size_t)row * A + n] = v;
        } else if (n < A + E) {
            dst[rr * ld + (n - A)] = v;                                    // (rows past R: G_1 is zero there, so is v)
            if (row < R) r.G_t2[(size_t)row * E + (n - A)] = v;
        } else if (r.g_cond != nullptr && row < R) {
            r.g_cond[(size_t)row * O + (n - A - E)] = v;
        }
    });
    __syncthreads();
    // time MLP^T: Gt = (G_t2 W_t2) * Mish'(Zt), written over Zt
    float* gt = bufA;                                                      // (the product above has read it)
    for (int i = tid; i < RO_ROWS * (ro_r16(E2) - E2); i += 256) {
        const int rr = i / (ro_r16(E2) - E2), c = E2 + i - rr * (ro_r16(E2) - E2);
        gt[rr * ld + c] = 0.f;
    }
    ro_product<true>(dst, ld, r.tw2, E2, E2, E, lane, wave, [&](int rr, int n, float v) {
        const int row = row0 + rr;
        float gz = 0.f;
        if (row < R) {
            gz = v * cdx_act_mish_grad(r.Zt[(size_t)row * E2 + n]);
            r.Zt[(size_t)row * E2 + n] = gz;
        }
        gt[rr * ld + n] = gz;
    });
    if (r.g_emb0 == nullptr) return;
    __syncthreads();
    ro_product<true>(gt, ld, r.tw1, E, E, E2, lane, wave, [&](int rr, int n, float v) {
        const int row = row0 + rr;
        if (row < R) r.g_emb0[(size_t)row * E + n] = v;
    });
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int dn_check(const cdx_denoise* r, bool bwd, const char* who) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (!r) return fail("null request");
    if (r->R < 0 || r->A <= 0 || r->E <= 0 || r->O < 0 || r->W <= 0) return fail("bad size");
    if (r->W % 16 != 0 || r->W > RO_MAX_WIDTH) return fail("W must be a multiple of 16, at most 512");
    if (r->A + r->E + r->O > RO_MAX_WIDTH) return fail("A + E + O must be at most 512");
    if (r->A > RO_MAX_X) return fail("A must be at most 64");
    if (2 * r->E > RO_MAX_WIDTH) return fail("2 E must be at most 512");
    if ((size_t)dn_lds(r) > DN_MAX_LDS) return fail("the LDS plan is over 160 KiB");
    if (r->R == 0) return CDX_OK;
    if (!r->tw1 || !r->tb1 || !r->tw2 || !r->tb2 || !r->w1 || !r->b1 || !r->w2 || !r->b2 || !r->w3 || !r->b3 || !r->wh || !r->bh)
        return fail("null pointer: weights");
    if (!r->emb0) return fail("null pointer: emb0");
    if (!r->xt && (!r->x0 || !r->eps || !r->a || !r->s)) return fail("null pointer: xt, or x0 / eps / a / s");
    if (r->loss_mode && !(r->predict_noise ? r->eps : r->x0)) return fail("null pointer: the loss target");
    if (r->cond && r->O == 0) return fail("cond given with O == 0");
    if (!r->Zt || !r->Ht || !r->feat || !r->Z || !r->H || !r->pred) return fail("null pointer: saved-tensor buffers");
    if (r->loss_mode && !r->loss_part) return fail("null pointer: loss_part");
    if (bwd) {
        if (!r->G_head || !r->G_t2) return fail("null pointer: backward buffers");
        if (!(r->loss_mode ? r->g_loss : r->g_pred)) return fail("null pointer: g_loss / g_pred");
        if (r->g_cond && !r->cond) return fail("g_cond asked without cond");
    }
    return CDX_OK;
}

int dn_launch(const cdx_denoise* r, void* hip_stream, bool bwd) {
    const char* who = bwd ? "cdx_denoise_bwd_f32" : "cdx_denoise_fwd_f32";
    cdx_set_err("");
    const int rc = dn_check(r, bwd, who);
    if (rc != CDX_OK || r->R == 0) return rc;
    static size_t raised[2] = {0, 0};
    return ro_launch_tiles(bwd ? cdx_denoise_bwd_kernel : cdx_denoise_fwd_kernel, *r, r->R, (size_t)dn_lds(r), hip_stream, raised[bwd]);
}

}  // namespace

extern "C" {

long long cdx_denoise_lds_bytes(const cdx_denoise* g) {
    if (!g || g->A <= 0 || g->E <= 0 || g->O < 0 || g->W <= 0) return CDX_EINVAL;
    return dn_lds(g);
}
int cdx_denoise_fwd_f32(const cdx_denoise* r, void* hip_stream) { return dn_launch(r, hip_stream, false); }
int cdx_denoise_bwd_f32(const cdx_denoise* r, void* hip_stream) { return dn_launch(r, hip_stream, true); }

}  // extern "C"
