// cdx_energy.hip -- QGPO's energy-guided sampling loop (SfBCUNet denoiser + QGPONNClassifier energy model) in one launch.
//
// QGPO's evaluation calls ``actor.sample(..., w_cfg=1, condition_cg=obs, w_cg=w)`` once per environment step (reference
// pipelines/qgpo_d4rl_mujoco.py:244-249) on 50-800 rows of low-dimensional actions.  Stepped on the host every denoising step is the
// denoiser forward, ~20 launches of the explicit classifier gradient (engine/mlp_grad.py) and the ATen shift / clip / update / mask
// kernels, each a few microseconds of work.  Rows are independent and nothing in a step needs more than 16 rows x 512 features at once, so
// cdx_energy_kernel runs the WHOLE loop for one 16-row tile per workgroup of 4 wave64 -- the row-tile design of cdx_rollout.hip, with
// the same product routine (cdx_rowtile.h; the energy model itself is cdx_energy_mlp.h, shared with cdx_cep.hip): activations in LDS, weights from global memory (a few MB, L2-resident, the same for every
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
#include "cdx_energy_mlp.h"
#include "cdx_rowtile.h"

namespace {

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
    float* xs = en_lds + p.off_xs;              // [16][RO_ALD] the state x_s, zero past A
    float* pr = en_lds + p.off_pr;              // [16][RO_XLD] the raw prediction
    float* gr = en_lds + p.off_gr;              // [16][RO_XLD] d logp / d x_s
    float* po = en_lds + p.off_po;              // [16][Ec]     obs_proj(obs)
    float* gf = en_lds + p.off_gf;              // [16] d logp / d f, then [16] logp
    float* lp = gf + RO_ROWS;
    const EmNet clf{L, Ec, g.hidden, g.clf_w, g.clf_b, g.clf_wo, g.clf_bo, en_lds, ld, p.off_pre};
    auto image = [&](int i) { return clf.image(i); };
    auto no_rows = [](int, int, float) {};
    auto no_layers = [=](int) { return no_rows; };

    // columns [K, next multiple of 16) of an MFMA A operand
    auto zero_pad = [&](float* t, int ldt, int K) {
        const int n = ro_r16(K) - K;
        for (int i = tid; i < RO_ROWS * n; i += 256) t[(i / n) * ldt + K + i % n] = 0.f;
    };

    // f and logp of the 16 rows at the state in xs with the time embedding `temb` (Ec): pre-activations saved, d logp / d f in gf, logp in
    // lp.  Returns the image the backward pass may write first (the one that does not hold the last hidden activation).
    auto clf_forward = [&](const float* __restrict__ temb) -> int {
        float* feat = image(0);
        const int K0 = 3 * Ec, K0p = ro_r16(K0);
        for (int i = tid; i < RO_ROWS * K0p; i += 256) {
            const int rr = i / K0p, c = i - rr * K0p;
            if (c < Ec) feat[rr * ld + c] = po[rr * Ec + c];
            else if (c >= 2 * Ec) feat[rr * ld + c] = c < K0 ? temb[c - 2 * Ec] : 0.f;
        }
        em_act_proj(xs, feat, ld, g.act_w, g.act_b, A, Ec, lane, wave, no_rows);
        __syncthreads();
        const int src = em_forward(clf, 0, lane, wave, no_layers);
        em_head(clf, src, lp, gf, lane, wave);
        return src ^ 1;
    };

    // d logp.sum() / d x_s -> gr, from what clf_forward left
    auto clf_backward = [&](int dst_i) {
        const int src = em_backward<false>(clf, g.clf_wt, gf, dst_i, tid, lane, wave, no_layers);
        float* ga = image(src ^ 1);             // d logp / d act_proj(x_s): (16 x Ec)
        ro_product<false>(image(src), ld, g.clf_wt[0], g.hidden[0], Ec, g.hidden[0], lane, wave,
                          [&](int rr, int n, float v) { ga[rr * ld + n] = v; });
        zero_pad(ga, ld, Ec);
        __syncthreads();
        ro_product<false>(ga, ld, g.act_wt, Ec, A, Ec, lane, wave, [&](int rr, int n, float v) { gr[rr * RO_XLD + n] = v; });
        __syncthreads();
    };

    // ---- before the loop: the state tile and obs_proj(obs) ----
    auto same_row = [](int row) { return row; };
    ro_load_rows(xs, RO_ALD, RO_ALD, g.x_in, A, row0, B, tid, same_row);
    ro_load_rows(image(0), ld, ro_r16(O), g.obs, O, row0, B, tid, same_row);
    __syncthreads();
    em_obs_proj(image(0), ld, g.obs_w, g.obs_b, O, Ec, lane, wave, [&](int rr, int n, float y) { po[rr * Ec + n] = y; });
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const EnStep& st = a.st[s];
        // ---- 1. denoiser ----
        {
            const int Ep = ro_r16(E);
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
        int src_ld = RO_ALD, cur = 0;
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
            pr[rr * RO_XLD + n] = y;
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
            const float gv = gr[rr * RO_XLD + e];
            if (g.trace_grad != nullptr && row < B) g.trace_grad[((size_t)s * B + row) * A + e] = gv;
            const RowStepIO io{g.clip ? g.x_min : nullptr, g.clip ? g.x_max : nullptr, g.fix_mask, g.prior, g.noise, B, A, row, e};
            xs[rr * RO_ALD + e] = cdx_step_element<false>(rec, g.predict_noise, xs[rr * RO_ALD + e], pr[rr * RO_XLD + e] + st.cg * gv, io);
        }
        __syncthreads();
    }

    for (int i = tid; i < RO_ROWS * A; i += 256) {
        const int rr = i / A, e = i - rr * A, row = row0 + rr;
        if (row < B) g.x_out[(size_t)row * A + e] = xs[rr * RO_ALD + e];
    }
    if (g.logp_out != nullptr) {
        clf_forward(g.clf_temb + (size_t)S * Ec);
        if (tid < RO_ROWS && row0 + tid < B) g.logp_out[row0 + tid] = lp[tid];
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int en_fail(const char* what) { return ro_fail("cdx_energy_guided_run", what); }

// sizes, the block table and the LDS plan: everything that can be checked without touching device memory
int en_plan(const cdx_energy_guided* g, EnPlan* p) {
    if (!g) return en_fail("null request");
    if (g->B < 0 || g->A <= 0 || g->E <= 0 || g->O <= 0 || g->Ec <= 0) return en_fail("bad size");
    EmPlan clf;
    const int rc = em_plan(g->A, g->O, g->Ec, g->n_hidden, g->hidden, &clf, en_fail, "E and Ec must be at most 128",
                           "hidden width must be a multiple of 16, at most 512 (classifier)");
    if (rc != CDX_OK) return rc;
    if (g->E > RO_MAX_EMB) return en_fail("E and Ec must be at most 128");
    if (g->S < 1 || g->S > CDX_ENERGY_MAX_STEPS) return en_fail("S must be 1 .. CDX_ENERGY_MAX_STEPS");
    if (g->n_blocks < 1 || g->n_blocks > CDX_ENERGY_MAX_BLOCKS || g->n_down < 0 || g->n_down > g->n_blocks)
        return en_fail("n_blocks must be 1 .. CDX_ENERGY_MAX_BLOCKS with 0 <= n_down <= n_blocks");
    if (!g->blocks) return en_fail("null pointer: blocks");
    int maxw = clf.maxw;
    int pops = 0;
    for (int i = 0; i < g->n_blocks; ++i) pops += g->blocks[i].in2 > 0;
    if (pops > g->n_down) return en_fail("more concat inputs than down blocks");
    int depth = 0, top[CDX_ENERGY_MAX_BLOCKS], width[CDX_ENERGY_MAX_BLOCKS];
    long long stack_floats = 0;
    for (int i = 0; i < g->n_blocks; ++i) {
        const cdx_energy_block& b = g->blocks[i];
        if (b.in <= 0 || b.in2 < 0 || b.out <= 0) return en_fail("bad size in the block table");
        if (b.out % 16 != 0 || b.out > RO_MAX_WIDTH) return en_fail("hidden width must be a multiple of 16, at most 512 (denoiser)");
        if (b.in + b.in2 > RO_MAX_CONCAT) return en_fail("a concat input must be at most 1024 wide");
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
    p->ldc = ro_r16(g->E) + 4;
    const long long img = (long long)RO_ROWS * p->ld;
    p->off_stack = (int32_t)(3 * img);
    for (int l = 0; l < CDX_ENERGY_MAX_HIDDEN; ++l)
        p->off_pre[l] = l < g->n_hidden ? (int32_t)(2 * img + RO_ROWS * clf.off_col[l]) : 0;
    const long long den = 3 * img + stack_floats, cls = 2 * img + clf.pre_floats;
    long long at = den > cls ? den : cls;
    p->off_crow = (int32_t)at; at += (long long)RO_ROWS * p->ldc;
    p->off_xs = (int32_t)at;   at += (long long)RO_ROWS * RO_ALD;
    p->off_pr = (int32_t)at;   at += (long long)RO_ROWS * RO_XLD;
    p->off_gr = (int32_t)at;   at += (long long)RO_ROWS * RO_XLD;
    p->off_po = (int32_t)at;   at += (long long)RO_ROWS * ro_r16(g->Ec);
    p->off_gf = (int32_t)at;   at += 2 * RO_ROWS;
    p->total = (int32_t)at;
    return CDX_OK;
}

int en_check(const cdx_energy_guided* g, EnPlan* p) {
    const int rc = en_plan(g, p);
    if (rc != CDX_OK) return rc;
    if (!g->steps || !g->cg_scale) return en_fail("null pointer: steps / cg_scale");
    if (const int rs = ro_check_steps(g->steps, g->S, g->noise != nullptr, en_fail); rs != CDX_OK) return rs;
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
    return ro_launch_tiles(cdx_energy_kernel, a, g->B, lds, hip_stream, raised);
}

}  // extern "C"
