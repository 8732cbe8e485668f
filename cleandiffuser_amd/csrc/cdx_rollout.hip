// cdx_rollout.hip -- the differentiable denoising loop of the row-MLP denoisers (DQLMlp / DVInvMlp) in two launches.
//
// Diffusion-QL's policy update back-propagates through ``sample(..., requires_grad=True)`` (reference pipelines/dql_d4rl_mujoco.py:98-101,
// diffusion/diffusionsde.py:526-594 over nn_diffusion/dqlmlp.py:30-52): S denoising steps of
//     feat = [x_t | temb_s | cond] -> 3 x (Linear -> Mish) -> Linear -> clip -> eps<->x0 -> affine solver update [+ k z] -> fix-mask blend.
// Stepped on the host that is ~25 launches forward and 50-75 backward PER STEP, each a few microseconds of work on a 256-row tensor.
// Rows are independent and nothing in a step needs more than 16 rows x 512 features of state, so
//   * cdx_rollout_fwd_f32: ONE launch runs the whole loop, one workgroup of 4 wave64 per 16-row tile, activations in LDS, weights read
//     from global memory (0.8 MB, L2-resident, the same for every workgroup), products on v_mfma_f32_16x16x4_f32 (exact fp32, rows on
//     the M axis; lane maps: cdx_probe_mfma_layout), and saves X[s], P_raw[s], feat[s], Z[l][s], H[l][s] for the backward pass;
//   * cdx_rollout_bwd_f32: ONE launch walks the steps in reverse with d loss / d x_s (16 x A) carried in LDS, recomputes the clip state
//     from X[s] / P_raw[s], and writes G[l][s] = d loss / d Z over Z (each element's Mish' is read before its G is written, by the same
//     lane), G_head[s], g_cond (summed over the steps in LDS: row-local) and g_temb as (B, S*E) rows -- one cdx_colsum_f32 over the B rows
//     gives (S*E).  No atomics anywhere: both kernels are bit-reproducible.
// The weight / bias sums over the batch are NOT done here: dW_l = sum_s G[l][s]^T H[l-1][s] is one cdx_conv_wgrad_f32 product per layer
// over the S*B rows (engine/rollout.py).  The solver step is cdx_step_element() (cdx_step.h), the one every sampling kernel runs, on
// kinds 0 / 1 / 2 with vsel 0 / 1, so the values agree with the no-grad one-launch path.
//
// Saved activations are laid out (3, S, B, W) -- layer-major -- so that the S*B rows of one layer are ONE row-major matrix.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"

namespace {

// the step record, plus the two derivatives of the update the backward pass uses:
//   x' = cx * x + cp * P (+ noise)   with P the CLIPPED prediction (d x'/d x at fixed P, d x'/d P)
struct RoStep {
    RowStep s;
    float cx, cp;
};

struct RoArgs {
    cdx_rollout r;
    RoStep st[CDX_ROLLOUT_MAX_STEPS];
};

__host__ __device__ inline int ro_ld(int A, int E, int O, int W) {        // row stride of the two activation images
    const int f16 = ro_r16(A + E + O);
    return (f16 > W ? f16 : W) + 4;
}

// ------------------------------------------------------------------------------------------------
// forward: the whole loop for one 16-row tile
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cdx_rollout_fwd_kernel(const RoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ro_lds[];
    const cdx_rollout& r = a.r;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = r.B, A = r.A, E = r.E, O = r.O, W = r.W, S = r.S, F = A + E + O, F16 = ro_r16(F);
    const int ld = ro_ld(A, E, O, W);
    const int row0 = blockIdx.x * RO_ROWS;
    float* bufA = ro_lds;                       // [16][ld]
    float* bufB = bufA + RO_ROWS * ld;          // [16][ld]
    float* xs = bufB + RO_ROWS * ld;            // [16][64] the state x_s
    float* pr = xs + RO_ROWS * RO_XLD;          // [16][64] the raw prediction
    const size_t SBW = (size_t)S * B * W;       // one layer's block of Z / H

    for (int i = tid; i < RO_ROWS * A; i += 256) {
        const int rr = i / A, e = i - rr * A, row = row0 + rr;
        const float v = row < B ? r.x_in[(size_t)row * A + e] : 0.f;
        xs[rr * RO_XLD + e] = v;
        if (row < B) r.X[(size_t)row * A + e] = v;
    }
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const RoStep& st = a.st[s];
        // features [x_s | temb_s | cond], zero up to F16
        for (int i = tid; i < RO_ROWS * F16; i += 256) {
            const int rr = i / F16, c = i - rr * F16, row = row0 + rr;
            float v = 0.f;
            if (c < A) v = xs[rr * RO_XLD + c];
            else if (c < A + E) v = r.temb[(size_t)s * E + (c - A)];
            else if (c < F && r.cond != nullptr && row < B) v = r.cond[(size_t)row * O + (c - A - E)];
            bufA[rr * ld + c] = v;
            if (c < F && row < B) r.feat[((size_t)s * B + row) * F + c] = v;
        }
        __syncthreads();
        float* src = bufA;
        float* dst = bufB;
        for (int l = 0; l < 3; ++l) {
            const float* w = l == 0 ? r.w1 : l == 1 ? r.w2 : r.w3;
            const float* bias = l == 0 ? r.b1 : l == 1 ? r.b2 : r.b3;
            const int K = l == 0 ? F : W;
            float* Z = r.Z + (size_t)l * SBW + (size_t)s * B * W;
            float* H = r.H + (size_t)l * SBW + (size_t)s * B * W;
            ro_product<false>(src, ld, w, K, W, K, lane, wave, [&](int rr, int n, float v) {
                const float z = v + bias[n];
                const float h = cdx_act_mish(z);
                dst[rr * ld + n] = h;
                const int row = row0 + rr;
                if (row < B) {
                    Z[(size_t)row * W + n] = z;
                    H[(size_t)row * W + n] = h;
                }
            });
            __syncthreads();
            float* t = src;
            src = dst;
            dst = t;
        }
        // head: P_raw (16 x A)
        ro_product<false>(src, ld, r.wh, W, A, W, lane, wave, [&](int rr, int n, float v) {
            const float p = v + r.bh[n];
            pr[rr * RO_XLD + n] = p;
            const int row = row0 + rr;
            if (row < B) r.P_raw[((size_t)s * B + row) * A + n] = p;
        });
        __syncthreads();
        // solver step (cdx_step.h; kinds 0-2 without memory, by ro_check)
        const cdx_step rec = st.s.record();
        for (int i = tid; i < RO_ROWS * A; i += 256) {
            const int rr = i / A, e = i - rr * A, row = row0 + rr;
            const RowStepIO io{r.clip ? r.x_min : nullptr, r.clip ? r.x_max : nullptr, r.fix_mask, r.prior, r.noise, B, A, row, e};
            const float xn = cdx_step_element<false>(rec, r.predict_noise, xs[rr * RO_XLD + e], pr[rr * RO_XLD + e], io);
            xs[rr * RO_XLD + e] = xn;
            if (row < B) r.X[((size_t)(s + 1) * B + row) * A + e] = xn;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// backward: the steps in reverse for one 16-row tile
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cdx_rollout_bwd_kernel(const RoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ro_lds[];
    const cdx_rollout& r = a.r;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = r.B, A = r.A, E = r.E, O = r.O, W = r.W, S = r.S, F = A + E + O;
    const int ld = ro_ld(A, E, O, W);
    const int row0 = blockIdx.x * RO_ROWS;
    float* bufA = ro_lds;                       // [16][ld]
    float* bufB = bufA + RO_ROWS * ld;          // [16][ld]
    float* gxs = bufB + RO_ROWS * ld;           // [16][64] d loss / d x_{s+1}, then d loss / d x_s
    float* gdir = gxs + RO_ROWS * RO_XLD;       // [16][64] the part of d loss / d x_s that does not pass through the network
    float* ghd = gdir + RO_ROWS * RO_XLD;       // [16][68] d loss / d P_raw, zero up to column 64 (an MFMA A operand)
    float* gcs = ghd + RO_ROWS * RO_ALD;        // [16][O]  d loss / d cond, summed over the steps
    const bool want_cond = r.cond != nullptr && r.g_cond != nullptr;
    const size_t SBW = (size_t)S * B * W;

    for (int i = tid; i < RO_ROWS * RO_XLD; i += 256) {
        const int rr = i / RO_XLD, e = i - rr * RO_XLD, row = row0 + rr;
        gxs[i] = (e < A && row < B) ? r.g_out[(size_t)row * A + e] : 0.f;
    }
    if (want_cond)
        for (int i = tid; i < RO_ROWS * O; i += 256) gcs[i] = 0.f;
    __syncthreads();

    for (int s = S - 1; s >= 0; --s) {
        const RoStep& st = a.st[s];
        const float al = st.s.alpha, sg = st.s.sigma;
        // blend, update, conversion and clamp: d loss / d P_raw and the direct part of d loss / d x_s
        for (int i = tid; i < RO_ROWS * RO_XLD; i += 256) {
            const int rr = i / RO_XLD, e = i - rr * RO_XLD, row = row0 + rr;
            float gp = 0.f;
            if (e < A && row < B) {
                float g = gxs[i];
                if (r.fix_mask) g *= 1.0f - r.fix_mask[e];
                const float x = r.X[((size_t)s * B + row) * A + e];
                const float p = r.P_raw[((size_t)s * B + row) * A + e];
                bool below = false, above = false;                       // P_raw outside the bounds the forward pass clamped to
                if (r.clip) {
                    if (r.predict_noise) {
                        if (r.x_max) below = p < (x - al * r.x_max[e]) / sg;
                        if (r.x_min) above = p > (x - al * r.x_min[e]) / sg;
                    } else {
                        if (r.x_min) below = p < r.x_min[e];
                        if (r.x_max) above = p > r.x_max[e];
                    }
                }
                gp = g * st.cp;
                float gd = g * st.cx;
                if (below || above) {
                    if (r.predict_noise) gd += gp / sg;                  // the bound is (x - alpha * x_m) / sigma: its gradient goes to x
                    gp = 0.f;
                }
                gdir[i] = gd;
                r.G_head[((size_t)s * B + row) * A + e] = gp;
            } else if (e < A) {
                gdir[i] = 0.f;
            }
            ghd[rr * RO_ALD + e] = gp;
        }
        __syncthreads();
        // head^T, then the three hidden layers^T: G_l = (G_{l+1} W_{l+1}) * Mish'(Z_l), written over Z_l
        const float* src = ghd;
        int src_ld = RO_ALD, K = A;
        float* dst = bufA;
        for (int l = 2; l >= 0; --l) {
            const float* w = l == 2 ? r.wh : l == 1 ? r.w3 : r.w2;         // (K, W) row-major: the layer ABOVE Z_l
            float* Z = r.Z + (size_t)l * SBW + (size_t)s * B * W;
            ro_product<true>(src, src_ld, w, W, W, K, lane, wave, [&](int rr, int n, float v) {
                const int row = row0 + rr;
                float gz = 0.f;
                if (row < B) {
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
        // layer 1^T: d loss / d feat = G_1 W_1 -> [x part | temb part | cond part]
        ro_product<true>(src, ld, r.w1, F, F, W, lane, wave, [&](int rr, int n, float v) {
            const int row = row0 + rr;
            if (n < A) {
                gxs[rr * RO_XLD + n] = gdir[rr * RO_XLD + n] + v;
            } else if (n < A + E) {
                if (row < B) r.g_temb[(size_t)row * ((size_t)S * E) + (size_t)s * E + (n - A)] = v;
            } else if (want_cond) {
                gcs[rr * O + (n - A - E)] += v;
            }
        });
        __syncthreads();
    }
    if (r.g_x != nullptr)
        for (int i = tid; i < RO_ROWS * A; i += 256) {
            const int rr = i / A, e = i - rr * A, row = row0 + rr;
            if (row < B) r.g_x[(size_t)row * A + e] = gxs[rr * RO_XLD + e];
        }
    if (want_cond)
        for (int i = tid; i < RO_ROWS * O; i += 256) {
            const int rr = i / O, o = i - rr * O, row = row0 + rr;
            if (row < B) r.g_cond[(size_t)row * O + o] = gcs[i];
        }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int ro_check(const cdx_rollout* r, bool bwd, const char* who) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (!r) return fail("null request");
    if (r->B < 0 || r->A <= 0 || r->E <= 0 || r->O < 0 || r->W <= 0) return fail("bad size");
    if (r->S < 1 || r->S > CDX_ROLLOUT_MAX_STEPS) return fail("S must be 1 .. CDX_ROLLOUT_MAX_STEPS");
    if (r->W % 16 != 0 || r->W > RO_MAX_WIDTH) return fail("W must be a multiple of 16, at most 512");
    if (r->A + r->E + r->O > RO_MAX_WIDTH) return fail("A + E + O must be at most 512");
    if (r->A > RO_MAX_X) return fail("A must be at most 64");
    if (!r->steps) return fail("null pointer: steps");
    if (const int rs = ro_check_steps(r->steps, r->S, r->noise != nullptr, fail); rs != CDX_OK) return rs;
    if (r->B == 0) return CDX_OK;
    if (!r->w1 || !r->b1 || !r->w2 || !r->b2 || !r->w3 || !r->b3 || !r->wh || !r->bh) return fail("null pointer: weights");
    if (!r->temb || !r->x_in) return fail("null pointer: temb / x_in");
    if (r->cond && r->O == 0) return fail("cond given with O == 0");
    if (r->fix_mask && !r->prior) return fail("fix_mask given without prior");
    if (!r->X || !r->P_raw || !r->feat || !r->Z || !r->H) return fail("null pointer: saved-tensor buffers");
    if (bwd && (!r->g_out || !r->G_head || !r->g_temb)) return fail("null pointer: backward buffers");
    return CDX_OK;
}

void ro_pack(const cdx_rollout* r, RoArgs* a) {
    a->r = *r;
    a->r.steps = nullptr;                                     // (host memory: the records travel in the kernel argument)
    for (int i = 0; i < r->S; ++i) {
        const cdx_step& st = r->steps[i];
        RoStep& o = a->st[i];
        o.s = RowStep::of(st);
        // x' = ax * x + ae * eps + at * xth, with eps = ex * x + ep * P and xth = tx * x + tp * P
        const double al = st.alpha, sg = st.sigma, k0 = st.k[0], k1 = st.k[1], k2 = st.k[2], k3 = st.k[3];
        const double ex = r->predict_noise ? 0.0 : 1.0 / sg, ep = r->predict_noise ? 1.0 : -al / sg;
        const double tx = r->predict_noise ? 1.0 / al : 0.0, tp = r->predict_noise ? -sg / al : 1.0;
        double ax, ae = 0.0, at = 0.0;
        if (st.kind == 0) { ax = k0; ae = k2 - k0 * k1; }
        else if (st.kind == 1) { ax = k0 / k2; ae = k3 - k0 * k1 / k2; }
        else { ax = k0; if (st.vsel & 1) at = -k1; else ae = -k1; }
        o.cx = (float)(ax + ae * ex + at * tx);
        o.cp = (float)(ae * ep + at * tp);
    }
}

int ro_launch(const cdx_rollout* r, void* hip_stream, bool bwd) {
    const char* who = bwd ? "cdx_rollout_bwd_f32" : "cdx_rollout_fwd_f32";
    cdx_set_err("");
    const int rc = ro_check(r, bwd, who);
    if (rc != CDX_OK || r->B == 0) return rc;
    RoArgs a;
    ro_pack(r, &a);
    const int ld = ro_ld(r->A, r->E, r->O, r->W);
    size_t floats = (size_t)2 * RO_ROWS * ld + (size_t)2 * RO_ROWS * RO_XLD;
    if (bwd) floats += (size_t)RO_ROWS * RO_ALD + (size_t)RO_ROWS * r->O;
    const size_t lds = floats * sizeof(float);                          // <= 66 KB + 44 KB
    static size_t raised[2] = {0, 0};
    return ro_launch_tiles(bwd ? cdx_rollout_bwd_kernel : cdx_rollout_fwd_kernel, a, r->B, lds, hip_stream, raised[bwd]);
}

}  // namespace

extern "C" {

int cdx_rollout_fwd_f32(const cdx_rollout* r, void* hip_stream) { return ro_launch(r, hip_stream, false); }
int cdx_rollout_bwd_f32(const cdx_rollout* r, void* hip_stream) { return ro_launch(r, hip_stream, true); }

}  // extern "C"
