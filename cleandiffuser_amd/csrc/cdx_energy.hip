// cdx_energy.hip -- QGPO's energy-guided sampling loop (SfBCUNet denoiser + QGPONNClassifier energy model) in one launch.
//
// QGPO's evaluation calls ``actor.sample(..., w_cfg=1, condition_cg=obs, w_cg=w)`` once per environment step (reference
// pipelines/qgpo_d4rl_mujoco.py:244-249) on 50-800 rows of low-dimensional actions.  Stepped on the host every denoising step is the
// denoiser forward, ~20 launches of the explicit classifier gradient (engine/mlp_grad.py) and the ATen shift / clip / update / mask
// kernels, each a few microseconds of work.  Rows are independent and nothing in a step needs more than 16 rows x 512 features at once, so
// cdx_energy_kernel runs the WHOLE loop for one 16-row tile per workgroup of 4 wave64 -- the row-tile design of cdx_rollout.hip, with
// the same product routine (cdx_rowtile.h): activations in LDS, weights from global memory (a few MB, L2-resident, the same for every
// workgroup), products on v_mfma_f32_16x16x4_f32.  Per step record s:
//   1. denoiser (reference nn_diffusion/sfbc_unet.py:53-82): c = den_c[s] + cond[row]; every ResidualBlock is two phases
//        t1 = SiLU(W1 [h | skip] + b1) + Wc c + bc          (h, the popped skip and c are three K ranges accumulated by the same lane)
//        o  = SiLU(W2 t1 + b2) + skip(h)                    (the skip Linear first, into o; identity: read [h | skip])
//      over three rotating activation images (h, t1 and o are live together); down outputs a later block pops are also written to a skip
//      stack; the out layer gives the raw prediction (16 x A);
//   2. energy model (reference nn_classifier/mlp.py:25-55): f = mlp([obs_proj(obs) | act_proj(x_s) | clf_temb[s]]), logp = 10 tanh(f / 10)
//      with the hidden pre-activations kept in LDS, then g = d logp.sum() / d x_s as engine/mlp_grad.py does it: x SiLU'(pre), the
//      transposed weights, then through act_proj.  obs_proj(obs) does not depend on the step: once per tile before the loop.  The
//      classifier's images alias the denoiser's (the prediction is in its own tile by then);
//   3. pred += cg_scale[s] g, then cdx_step_element() (cdx_step.h): clip, eps <-> x0, the affine update, + k z, fix-mask blend.
// After the last step one more energy forward on the unclipped x_S with clf_temb[S] (t = 0) gives logp_out.  No atomics, every element
// is produced by one fixed lane in one fixed order: bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"

extern void cdx_set_err(const char* msg);

namespace {

constexpr int EN_XLD = 64;       // row stride of the prediction / gradient tiles (A <= 64)
constexpr int EN_ALD = 68;       // row stride of the state tile (an MFMA A operand: padded against bank conflicts), zero past A
constexpr long long EN_LDS_MAX = 160 * 1024;

struct EnStep {
    RowStep s;
    float cg;              // cg_scale of the step
};

// the LDS plan, in floats.  [0, region) is shared by the two nets: the denoiser has three activation images [16][ld] and the skip stack
// behind them, the classifier the first two images and its saved pre-activations [16][hidden[l]] behind those.
struct EnPlan {
    int32_t ld;                                   // row stride of the activation images: the widest operand + 4
    int32_t ldc;                                  // row stride of the c rows: E rounded up to 16, + 4
    int32_t off_stack, off_pre[CDX_ENERGY_MAX_HIDDEN];
    int32_t off_crow, off_xs, off_pr, off_gr, off_po, off_gf, total;
    int32_t push_off[CDX_ENERGY_MAX_BLOCKS];      // where a block's output goes on the skip stack (relative to off_stack), -1: not kept
    int32_t pop_off[CDX_ENERGY_MAX_BLOCKS];       // where a block with in2 > 0 finds its concat partner, -1
};

struct EnArgs {
    cdx_energy_guided g;
    cdx_energy_block blk[CDX_ENERGY_MAX_BLOCKS];
    EnStep st[CDX_ENERGY_MAX_STEPS];
    EnPlan p;
};
static_assert(sizeof(EnArgs) <= 4096, "the kernel argument segment holds 4 KiB");

__host__ __device__ inline int en_r16(int v) { return (v + 15) & ~15; }

// s (1 + x (1 - s)), s = sigmoid(x): the formula of cdx_act_bwd_f32
__device__ __forceinline__ float en_silu_grad(float x) {
    const float sg = 1.0f / (1.0f + __expf(-x));
    return sg * (1.0f + x * (1.0f - sg));
}

__global__ __launch_bounds__(256) void cdx_energy_kernel(const EnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float en_lds[];
    const cdx_energy_guided& g = a.g;
    const EnPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = g.B, A = g.A, E = g.E, O = g.O, S = g.S, Ec = g.Ec, L = g.n_hidden;
    const int ld = p.ld, ldc = p.ldc;
    const int row0 = blockIdx.x * RO_ROWS;
    float* stack = en_lds + p.off_stack;
    float* crow = en_lds + p.off_crow;          // [16][ldc]    c = den_c[s] + cond, zero past E
    float* xs = en_lds + p.off_xs;              // [16][EN_ALD] the state x_s, zero past A
    float* pr = en_lds + p.off_pr;              // [16][EN_XLD] the raw prediction
    float* gr = en_lds + p.off_gr;              // [16][EN_XLD] d logp / d x_s
    float* po = en_lds + p.off_po;              // [16][Ec]     obs_proj(obs)
    float* gf = en_lds + p.off_gf;              // [16] d logp / d f, then [16] logp
    float* lp = gf + RO_ROWS;
    auto image = [&](int i) { return en_lds + (size_t)i * RO_ROWS * ld; };

    // columns [K, next multiple of 16) of an MFMA A operand
    auto zero_pad = [&](float* t, int ldt, int K) {
        const int n = en_r16(K) - K;
        for (int i = tid; i < RO_ROWS * n; i += 256) t[(i / n) * ldt + K + i % n] = 0.f;
    };

    // f and logp of the 16 rows at the state in xs with the time embedding `temb` (Ec): pre-activations saved, d logp / d f in gf, logp in
    // lp.  Returns the image the backward pass may write first (the one that does not hold the last hidden activation).
    auto clf_forward = [&](const float* __restrict__ temb) -> int {
        float* feat = image(0);
        const int K0 = 3 * Ec, K0p = en_r16(K0);
        for (int i = tid; i < RO_ROWS * K0p; i += 256) {
            const int rr = i / K0p, c = i - rr * K0p;
            if (c < Ec) feat[rr * ld + c] = po[rr * Ec + c];
            else if (c >= 2 * Ec) feat[rr * ld + c] = c < K0 ? temb[c - 2 * Ec] : 0.f;
        }
        ro_product<false>(xs, EN_ALD, g.act_w, A, Ec, A, lane, wave,
                          [&](int rr, int n, float v) { feat[rr * ld + Ec + n] = v + g.act_b[n]; });
        __syncthreads();
        int src = 0;
        for (int l = 0; l < L; ++l) {
            const int W = g.hidden[l], K = l ? g.hidden[l - 1] : K0;
            const float* bias = g.clf_b[l];
            float* pre = en_lds + p.off_pre[l];
            float* dst = image(src ^ 1);
            ro_product<false>(image(src), ld, g.clf_w[l], K, W, K, lane, wave, [&](int rr, int n, float v) {
                const float z = v + bias[n];
                pre[rr * W + n] = z;
                dst[rr * ld + n] = cdx_act_silu(z);
            });
            __syncthreads();
            src ^= 1;
        }
        const int WL = g.hidden[L - 1];
        ro_product<false>(image(src), ld, g.clf_wo, WL, 1, WL, lane, wave, [&](int rr, int n, float v) {
            const float t = cdx_act_tanh((v + g.clf_bo[0]) / 10.0f);
            gf[rr] = 1.0f - t * t;
            lp[rr] = 10.0f * t;
        });
        __syncthreads();
        return src ^ 1;
    };

    // d logp.sum() / d x_s -> gr, from what clf_forward left
    auto clf_backward = [&](int dst_i) {
        const int WL = g.hidden[L - 1];
        {
            const float* pre = en_lds + p.off_pre[L - 1];
            float* dst = image(dst_i);
            for (int i = tid; i < RO_ROWS * WL; i += 256) {
                const int rr = i / WL, n = i - rr * WL;
                dst[rr * ld + n] = gf[rr] * g.clf_wo[n] * en_silu_grad(pre[i]);
            }
        }
        __syncthreads();
        int src = dst_i;
        for (int l = L - 1; l >= 1; --l) {
            const int N = g.hidden[l - 1], K = g.hidden[l];
            const float* pre = en_lds + p.off_pre[l - 1];
            float* dst = image(src ^ 1);
            ro_product<false>(image(src), ld, g.clf_wt[l], K, N, K, lane, wave,
                              [&](int rr, int n, float v) { dst[rr * ld + n] = v * en_silu_grad(pre[rr * N + n]); });
            __syncthreads();
            src ^= 1;
        }
        float* ga = image(src ^ 1);             // d logp / d act_proj(x_s): (16 x Ec)
        ro_product<false>(image(src), ld, g.clf_wt[0], g.hidden[0], Ec, g.hidden[0], lane, wave,
                          [&](int rr, int n, float v) { ga[rr * ld + n] = v; });
        zero_pad(ga, ld, Ec);
        __syncthreads();
        ro_product<false>(ga, ld, g.act_wt, Ec, A, Ec, lane, wave, [&](int rr, int n, float v) { gr[rr * EN_XLD + n] = v; });
        __syncthreads();
    };

    // ---- before the loop: the state tile and obs_proj(obs) ----
    for (int i = tid; i < RO_ROWS * EN_ALD; i += 256) {
        const int rr = i / EN_ALD, e = i - rr * EN_ALD, row = row0 + rr;
        xs[i] = (e < A && row < B) ? g.x_in[(size_t)row * A + e] : 0.f;
    }
    {
        float* ot = image(0);
        const int Op = en_r16(O);
        for (int i = tid; i < RO_ROWS * Op; i += 256) {
            const int rr = i / Op, c = i - rr * Op, row = row0 + rr;
            ot[rr * ld + c] = (c < O && row < B) ? g.obs[(size_t)row * O + c] : 0.f;
        }
        __syncthreads();
        ro_product<false>(ot, ld, g.obs_w, O, Ec, O, lane, wave, [&](int rr, int n, float v) { po[rr * Ec + n] = v + g.obs_b[n]; });
        __syncthreads();
    }

    for (int s = 0; s < S; ++s) {
        const EnStep& st = a.st[s];
        // ---- 1. denoiser ----
        {
            const int Ep = en_r16(E);
            for (int i = tid; i < RO_ROWS * Ep; i += 256) {
                const int rr = i / Ep, c = i - rr * Ep, row = row0 + rr;
                float v = 0.f;
                if (c < E) {
                    v = g.den_c[(size_t)s * E + c];
                    if (g.cond != nullptr && row < B) v += g.cond[(size_t)row * E + c];
                }
                crow[rr * ldc + c] = v;
            }
        }
        __syncthreads();
        const float* src = xs;
        int src_ld = EN_ALD, cur = 0;
        for (int bi = 0; bi < g.n_blocks; ++bi) {
            const cdx_energy_block& b = a.blk[bi];
            const int in = b.in, in2 = b.in2, W = b.out, ldw = in + in2;
            float* t1 = image((cur + 1) % 3);
            float* o = image((cur + 2) % 3);
            const float* partner = stack + (in2 > 0 ? p.pop_off[bi] : 0);
            const int pld = in2 + 4;
            ro_product<false>(src, src_ld, b.w1, ldw, W, in, lane, wave, [&](int rr, int n, float v) { t1[rr * ld + n] = v; });
            if (in2 > 0)
                ro_product<false>(partner, pld, b.w1 + in, ldw, W, in2, lane, wave, [&](int rr, int n, float v) { t1[rr * ld + n] += v; });
            ro_product<false>(crow, ldc, b.wc, E, W, E, lane, wave, [&](int rr, int n, float v) {
                t1[rr * ld + n] = cdx_act_silu(t1[rr * ld + n] + b.b1[n]) + (v + b.bc[n]);
            });
            __syncthreads();
            const bool lin_skip = b.ws != nullptr;
            if (lin_skip) {
                ro_product<false>(src, src_ld, b.ws, ldw, W, in, lane, wave, [&](int rr, int n, float v) { o[rr * ld + n] = v + b.bs[n]; });
                if (in2 > 0)
                    ro_product<false>(partner, pld, b.ws + in, ldw, W, in2, lane, wave, [&](int rr, int n, float v) { o[rr * ld + n] += v; });
            }
            float* keep = p.push_off[bi] >= 0 ? stack + p.push_off[bi] : nullptr;
            ro_product<false>(t1, ld, b.w2, W, W, W, lane, wave, [&](int rr, int n, float v) {
                const float y = cdx_act_silu(v + b.b2[n]) +
                                (lin_skip ? o[rr * ld + n] : n < in ? src[rr * src_ld + n] : partner[rr * pld + (n - in)]);
                o[rr * ld + n] = y;
                if (keep != nullptr) keep[rr * (W + 4) + n] = y;
            });
            __syncthreads();
            src = o;
            src_ld = ld;
            cur = (cur + 2) % 3;
        }
        ro_product<false>(src, src_ld, g.out_w, a.blk[g.n_blocks - 1].out, A, a.blk[g.n_blocks - 1].out, lane, wave,
                          [&](int rr, int n, float v) {
            const float y = v + g.out_b[n];
            pr[rr * EN_XLD + n] = y;
            const int row = row0 + rr;
            if (g.trace_pred != nullptr && row < B) g.trace_pred[((size_t)s * B + row) * A + n] = y;
        });
        __syncthreads();
        // ---- 2. energy model: logp and its gradient at x_s ----
        clf_backward(clf_forward(g.clf_temb + (size_t)s * Ec));
        if (g.trace_logp != nullptr && tid < RO_ROWS && row0 + tid < B) g.trace_logp[(size_t)s * B + row0 + tid] = lp[tid];
        // ---- 3. shift and solver step (cdx_step.h; kinds 0-2 without memory, by en_check) ----
        const cdx_step rec = st.s.record();
        for (int i = tid; i < RO_ROWS * A; i += 256) {
            const int rr = i / A, e = i - rr * A, row = row0 + rr;
            const float gv = gr[rr * EN_XLD + e];
            if (g.trace_grad != nullptr && row < B) g.trace_grad[((size_t)s * B + row) * A + e] = gv;
            const RowStepIO io{g.clip ? g.x_min : nullptr, g.clip ? g.x_max : nullptr, g.fix_mask, g.prior, g.noise, B, A, row, e};
            xs[rr * EN_ALD + e] = cdx_step_element<false>(rec, g.predict_noise, xs[rr * EN_ALD + e], pr[rr * EN_XLD + e] + st.cg * gv, io);
        }
        __syncthreads();
    }

    for (int i = tid; i < RO_ROWS * A; i += 256) {
        const int rr = i / A, e = i - rr * A, row = row0 + rr;
        if (row < B) g.x_out[(size_t)row * A + e] = xs[rr * EN_ALD + e];
    }
    if (g.logp_out != nullptr) {
        clf_forward(g.clf_temb + (size_t)S * Ec);
        if (tid < RO_ROWS && row0 + tid < B) g.logp_out[row0 + tid] = lp[tid];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int en_fail(const char* what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "cdx_energy_guided_run: %s", what);
    cdx_set_err(msg);
    return CDX_EINVAL;
}

// sizes, the block table and the LDS plan: everything that can be checked without touching device memory
int en_plan(const cdx_energy_guided* g, EnPlan* p) {
    if (!g) return en_fail("null request");
    if (g->B < 0 || g->A <= 0 || g->E <= 0 || g->O <= 0 || g->Ec <= 0) return en_fail("bad size");
    if (g->A > 64) return en_fail("A must be at most 64");
    if (g->E > 128 || g->Ec > 128) return en_fail("E and Ec must be at most 128");
    if (g->O > 512) return en_fail("O must be at most 512");
    if (g->S < 1 || g->S > CDX_ENERGY_MAX_STEPS) return en_fail("S must be 1 .. CDX_ENERGY_MAX_STEPS");
    if (g->n_blocks < 1 || g->n_blocks > CDX_ENERGY_MAX_BLOCKS || g->n_down < 0 || g->n_down > g->n_blocks)
        return en_fail("n_blocks must be 1 .. CDX_ENERGY_MAX_BLOCKS with 0 <= n_down <= n_blocks");
    if (g->n_hidden < 1 || g->n_hidden > CDX_ENERGY_MAX_HIDDEN) return en_fail("n_hidden must be 1 .. CDX_ENERGY_MAX_HIDDEN");
    if (!g->blocks) return en_fail("null pointer: blocks");
    int maxw = en_r16(g->O) > en_r16(3 * g->Ec) ? en_r16(g->O) : en_r16(3 * g->Ec);
    long long pre_floats = 0;
    for (int l = 0; l < g->n_hidden; ++l) {
        const int w = g->hidden[l];
        if (w <= 0 || w % 16 != 0 || w > 512) return en_fail("hidden width must be a multiple of 16, at most 512 (classifier)");
        maxw = w > maxw ? w : maxw;
        p->off_pre[l] = (int32_t)pre_floats;                               // (relative to the end of the second image: below)
        pre_floats += (long long)RO_ROWS * w;
    }
    for (int l = g->n_hidden; l < CDX_ENERGY_MAX_HIDDEN; ++l) p->off_pre[l] = 0;
    int pops = 0;
    for (int i = 0; i < g->n_blocks; ++i) pops += g->blocks[i].in2 > 0;
    if (pops > g->n_down) return en_fail("more concat inputs than down blocks");
    int depth = 0, top[CDX_ENERGY_MAX_BLOCKS], width[CDX_ENERGY_MAX_BLOCKS];
    long long stack_floats = 0;
    for (int i = 0; i < g->n_blocks; ++i) {
        const cdx_energy_block& b = g->blocks[i];
        if (b.in <= 0 || b.in2 < 0 || b.out <= 0) return en_fail("bad size in the block table");
        if (b.out % 16 != 0 || b.out > 512) return en_fail("hidden width must be a multiple of 16, at most 512 (denoiser)");
        if (b.in + b.in2 > 1024) return en_fail("a concat input must be at most 1024 wide");
        if (b.in != (i ? g->blocks[i - 1].out : g->A)) return en_fail("block input width does not continue the chain");
        if (!b.ws && b.in + b.in2 != b.out) return en_fail("identity skip needs in + in2 == out");
        maxw = b.out > maxw ? b.out : maxw;
        p->pop_off[i] = p->push_off[i] = -1;
        if (b.in2 > 0) {
            if (depth == 0 || width[depth - 1] != b.in2) return en_fail("concat partner width does not match the skip stack");
            p->pop_off[i] = top[--depth];
        }
        if (i < g->n_down && i >= g->n_down - pops) {                        // (earlier down outputs are never popped: not kept)
            top[depth] = p->push_off[i] = (int32_t)stack_floats;
            width[depth++] = b.out;
            stack_floats += (long long)RO_ROWS * (b.out + 4);
        }
    }
    for (int i = g->n_blocks; i < CDX_ENERGY_MAX_BLOCKS; ++i) p->pop_off[i] = p->push_off[i] = -1;
    p->ld = maxw + 4;
    p->ldc = en_r16(g->E) + 4;
    const long long img = (long long)RO_ROWS * p->ld;
    p->off_stack = (int32_t)(3 * img);
    for (int l = 0; l < g->n_hidden; ++l) p->off_pre[l] += (int32_t)(2 * img);
    const long long den = 3 * img + stack_floats, clf = 2 * img + pre_floats;
    long long at = den > clf ? den : clf;
    p->off_crow = (int32_t)at; at += (long long)RO_ROWS * p->ldc;
    p->off_xs = (int32_t)at;   at += (long long)RO_ROWS * EN_ALD;
    p->off_pr = (int32_t)at;   at += (long long)RO_ROWS * EN_XLD;
    p->off_gr = (int32_t)at;   at += (long long)RO_ROWS * EN_XLD;
    p->off_po = (int32_t)at;   at += (long long)RO_ROWS * en_r16(g->Ec);
    p->off_gf = (int32_t)at;   at += 2 * RO_ROWS;
    p->total = (int32_t)at;
    return CDX_OK;
}

int en_check(const cdx_energy_guided* g, EnPlan* p) {
    const int rc = en_plan(g, p);
    if (rc != CDX_OK) return rc;
    if (!g->steps || !g->cg_scale) return en_fail("null pointer: steps / cg_scale");
    for (int i = 0; i < g->S; ++i) {
        const cdx_step& st = g->steps[i];
        if (st.kind < 0 || st.kind > 2) return en_fail("step kind must be 0, 1 or 2");
        if (st.vsel < 0 || st.vsel > 1) return en_fail("step vsel must be 0 or 1 (no multistep memory)");
        if (st.flags != 0) return en_fail("step flags are not supported");
        if (st.noise_idx >= 0 && !g->noise) return en_fail("step draws noise but noise == NULL");
    }
    if ((long long)p->total * (long long)sizeof(float) > EN_LDS_MAX) return en_fail("the LDS plan exceeds 160 KiB");
    if (g->B == 0) return CDX_OK;
    for (int i = 0; i < g->n_blocks; ++i) {
        const cdx_energy_block& b = g->blocks[i];
        if (!b.w1 || !b.b1 || !b.w2 || !b.b2 || !b.wc || !b.bc || (!b.ws) != (!b.bs)) return en_fail("null pointer: denoiser weights");
    }
    if (!g->out_w || !g->out_b || !g->den_c) return en_fail("null pointer: denoiser weights");
    if (!g->obs_w || !g->obs_b || !g->act_w || !g->act_b || !g->act_wt || !g->clf_wo || !g->clf_bo || !g->clf_temb)
        return en_fail("null pointer: classifier weights");
    for (int l = 0; l < g->n_hidden; ++l)
        if (!g->clf_w[l] || !g->clf_b[l] || !g->clf_wt[l]) return en_fail("null pointer: classifier weights");
    if (!g->obs || !g->x_in) return en_fail("null pointer: obs / x_in");
    if (!g->x_out) return en_fail("null pointer: x_out");
    if (g->fix_mask && !g->prior) return en_fail("fix_mask given without prior");
    return CDX_OK;
}

}  // namespace

extern "C" {

long long cdx_energy_guided_lds_bytes(const cdx_energy_guided* g) {
    cdx_set_err("");
    EnPlan p;
    const int rc = en_plan(g, &p);
    return rc != CDX_OK ? rc : (long long)p.total * (long long)sizeof(float);
}

int cdx_energy_guided_run(const cdx_energy_guided* g, void* hip_stream) {
    cdx_set_err("");
    EnArgs a;
    const int rc = en_check(g, &a.p);
    if (rc != CDX_OK || g->B == 0) return rc;
    a.g = *g;
    a.g.blocks = nullptr;                                      // (host memory: tables and records travel in the kernel argument)
    a.g.steps = nullptr;
    a.g.cg_scale = nullptr;
    for (int i = 0; i < CDX_ENERGY_MAX_BLOCKS; ++i) a.blk[i] = g->blocks[i < g->n_blocks ? i : 0];
    for (int i = 0; i < g->S; ++i) a.st[i] = EnStep{RowStep::of(g->steps[i]), g->cg_scale[i]};
    for (int i = g->S; i < CDX_ENERGY_MAX_STEPS; ++i) a.st[i] = EnStep{RowStep{0, 0, -1, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f}, 0.f};
    const size_t lds = (size_t)a.p.total * sizeof(float);
    static size_t raised = 0;
    if (lds > 48 * 1024 && lds > raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cdx_energy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
        raised = lds;
    }
    const dim3 grid((unsigned)((g->B + RO_ROWS - 1) / RO_ROWS));
    hipLaunchKernelGGL(cdx_energy_kernel, grid, dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
    return CDX_OK;
}

}  // extern "C"
