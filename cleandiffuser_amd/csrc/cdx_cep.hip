// cdx_cep.hip -- QGPO's contrastive energy training step (forward, loss, backward-data) for one 16-row tile per workgroup.
//
// The energy model of QGPO is trained by ``clf.update(noisy_act, t, {"soft_label", "obs"})`` once per gradient step (reference
// pipelines/qgpo_d4rl_mujoco.py:172-212 over classifier/qgpo_classifier.py:16-61): B states x K support actions, R = B K rows of a
// 3 x 256 SiLU MLP, the loss a cross entropy between the soft labels and the softmax of the energies over the K rows of a state.  As
// autograd that is about a hundred launches of a few microseconds each.  Rows of different states are independent and K divides 16, so
// one workgroup of 4 wave64 owns 16 consecutive rows -- 16 / K whole softmax groups -- and runs, with the product routine of the row-tile
// kernels (cdx_rowtile.h: activations in LDS, weights from global memory, v_mfma_f32_16x16x4_f32):
//   forward   feat = [obs_proj(obs[b]) | act_proj(x[r]) | temb[b]] (b = r / K), h_l = SiLU(W_l h_{l-1} + b_l) with the pre-activations
//             kept in LDS, o = w_o . h + b_o, f = 10 tanh(o / 10);
//   loss      per state: lse = logsumexp_k f, loss = -sum_k y_k (f_k - lse), max_k f, min_k f, sum_k f -> stats (B, 4);
//   backward  dL/df = (softmax_k(f) sum_j y_j - y_k) / B, x (1 - tanh^2), through w_o, then per hidden layer x SiLU'(pre) and the transposed
//             product on the LIVE weight (ro_product<true>), down to d / d feat: its act_proj columns are G_act, its obs_proj columns
//             summed over the K rows of the state are G_obs, the time columns have no parameters behind them.
// feat, H_l, G_l = dL/d pre_l, G_out = dL/do, G_act and G_obs go to global memory: the weight and bias sums over the rows are the caller's
// (one cdx_conv_wgrad_batch_f32).  Rows of the last tile past R carry a zero loss gradient and nothing is written for them.  No atomics,
// every element is produced by one fixed lane in one fixed order: bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"

extern void cdx_set_err(const char* msg);

namespace {

constexpr int CEP_ALD = 68;      // row stride of the action tile (an MFMA A operand: padded against bank conflicts), zero past A
constexpr int CEP_SC = 64;       // the per-row scalars: f, 1 - tanh^2, dL/do (16 each)
constexpr long long CEP_LDS_MAX = 160 * 1024;

// the LDS plan, in floats: two activation images [16][ld], the saved pre-activations [16][hidden[l]], the action tile, the scalars
struct CepPlan {
    int32_t ld;                                   // row stride of the activation images: the widest operand + 4
    int32_t off_pre[CDX_ENERGY_MAX_HIDDEN];
    int32_t off_xs, off_sc, total;
};

struct CepArgs {
    cdx_cep_step g;
    CepPlan p;
};
static_assert(sizeof(CepArgs) <= 4096, "the kernel argument segment holds 4 KiB");

__host__ __device__ inline int cep_r16(int v) { return (v + 15) & ~15; }

// s (1 + x (1 - s)), s = sigmoid(x): the formula of cdx_act_bwd_f32
__device__ __forceinline__ float cep_silu_grad(float x) {
    const float sg = 1.0f / (1.0f + __expf(-x));
    return sg * (1.0f + x * (1.0f - sg));
}

__global__ __launch_bounds__(256) void cdx_cep_kernel(const CepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cep_lds[];
    const cdx_cep_step& g = a.g;
    const CepPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = g.K, A = g.A, O = g.O, Ec = g.Ec, L = g.n_hidden, ld = p.ld;
    const long long R = (long long)g.B * K;
    const long long row0 = (long long)blockIdx.x * RO_ROWS;
    const int K0 = 3 * Ec;
    float* xs = cep_lds + p.off_xs;             // [16][CEP_ALD] the noisy actions, zero past A
    float* sc_f = cep_lds + p.off_sc;           // [16] f
    float* sc_dt = sc_f + RO_ROWS;              // [16] 1 - tanh^2(o / 10)
    float* sc_go = sc_dt + RO_ROWS;             // [16] dL/do
    auto image = [&](int i) { return cep_lds + (size_t)i * RO_ROWS * ld; };

    // ---- the tile's inputs: actions, the observation of each row's state, the time columns of feat ----
    for (int i = tid; i < RO_ROWS * CEP_ALD; i += 256) {
        const int rr = i / CEP_ALD, e = i - rr * CEP_ALD;
        const long long row = row0 + rr;
        xs[i] = (e < A && row < R) ? g.x[(size_t)row * A + e] : 0.f;
    }
    float* feat = image(1);
    {
        float* ot = image(0);
        const int Op = cep_r16(O);
        for (int i = tid; i < RO_ROWS * Op; i += 256) {
            const int rr = i / Op, c = i - rr * Op;
            const long long row = row0 + rr;
            ot[rr * ld + c] = (c < O && row < R) ? g.obs[(size_t)(row / K) * O + c] : 0.f;
        }
        const int nt = cep_r16(K0) - 2 * Ec;    // the time columns and the zero columns up to the next multiple of 16
        for (int i = tid; i < RO_ROWS * nt; i += 256) {
            const int rr = i / nt, c = 2 * Ec + (i - rr * nt);
            const long long row = row0 + rr;
            const bool live = c < K0 && row < R;
            const float v = live ? g.temb[(size_t)(row / K) * Ec + (c - 2 * Ec)] : 0.f;
            feat[rr * ld + c] = v;
            if (live) g.feat[(size_t)row * K0 + c] = v;
        }
        __syncthreads();
        ro_product<false>(ot, ld, g.obs_w, O, Ec, O, lane, wave, [&](int rr, int n, float v) {
            const float y = v + g.obs_b[n];
            feat[rr * ld + n] = y;
            if (row0 + rr < R) g.feat[(size_t)(row0 + rr) * K0 + n] = y;
        });
        ro_product<false>(xs, CEP_ALD, g.act_w, A, Ec, A, lane, wave, [&](int rr, int n, float v) {
            const float y = v + g.act_b[n];
            feat[rr * ld + Ec + n] = y;
            if (row0 + rr < R) g.feat[(size_t)(row0 + rr) * K0 + Ec + n] = y;
        });
        __syncthreads();
    }

    // ---- forward: the hidden layers (pre-activations stay in LDS, activations go to H), the head ----
    int src = 1;
    size_t col0 = 0;                            // columns of the layers before l: layer l's (R, hidden[l]) matrix starts at R * col0
    for (int l = 0; l < L; ++l) {
        const int W = g.hidden[l], Kd = l ? g.hidden[l - 1] : K0;
        const float* bias = g.b[l];
        float* pre = cep_lds + p.off_pre[l];
        float* dst = image(src ^ 1);
        float* Hl = g.H + (size_t)R * col0;
        ro_product<false>(image(src), ld, g.w[l], Kd, W, Kd, lane, wave, [&](int rr, int n, float v) {
            const float z = v + bias[n];
            const float h = cdx_act_silu(z);
            pre[rr * W + n] = z;
            dst[rr * ld + n] = h;
            if (row0 + rr < R) Hl[(size_t)(row0 + rr) * W + n] = h;
        });
        __syncthreads();
        src ^= 1;
        col0 += W;
    }
    const int WL = g.hidden[L - 1];
    ro_product<false>(image(src), ld, g.wo, WL, 1, WL, lane, wave, [&](int rr, int n, float v) {
        const float t = cdx_act_tanh((v + g.bo[0]) / 10.0f);
        sc_f[rr] = 10.0f * t;
        sc_dt[rr] = 1.0f - t * t;
    });
    __syncthreads();

    // ---- loss: one thread per softmax group, its K rows in order ----
    const int groups = RO_ROWS / K;
    if (tid < groups) {
        const int r_lo = tid * K;
        const long long row = row0 + r_lo;
        if (row < R) {
            float mx = sc_f[r_lo], mn = sc_f[r_lo], sf = 0.f, sy = 0.f;
            for (int k = 0; k < K; ++k) {
                const float f = sc_f[r_lo + k];
                mx = fmaxf(mx, f);
                mn = fminf(mn, f);
                sf += f;
                sy += g.soft[row + k];
            }
            float se = 0.f;
            for (int k = 0; k < K; ++k) se += expf(sc_f[r_lo + k] - mx);
            const float lse = mx + logf(se), inv = 1.0f / se, inv_b = 1.0f / (float)g.B;
            float loss = 0.f;
            for (int k = 0; k < K; ++k) {
                const float f = sc_f[r_lo + k], y = g.soft[row + k];
                loss -= y * (f - lse);
                const float go = (expf(f - mx) * inv * sy - y) * inv_b * sc_dt[r_lo + k];
                sc_go[r_lo + k] = go;
                g.G_out[row + k] = go;
            }
            float* st = g.stats + (size_t)(row / K) * 4;
            st[0] = loss;
            st[1] = mx;
            st[2] = mn;
            st[3] = sf;
        } else {
            for (int k = 0; k < K; ++k) sc_go[r_lo + k] = 0.f;
        }
    }
    __syncthreads();

    // ---- backward-data: G_l = dL/d pre_l from the last hidden layer down, then d / d feat ----
    col0 -= WL;
    {
        const float* pre = cep_lds + p.off_pre[L - 1];
        float* dst = image(src ^ 1);
        float* Gl = g.G + (size_t)R * col0;
        for (int i = tid; i < RO_ROWS * WL; i += 256) {
            const int rr = i / WL, n = i - rr * WL;
            const float v = sc_go[rr] * g.wo[n] * cep_silu_grad(pre[i]);
            dst[rr * ld + n] = v;
            if (row0 + rr < R) Gl[(size_t)(row0 + rr) * WL + n] = v;
        }
    }
    __syncthreads();
    src ^= 1;
    for (int l = L - 1; l >= 1; --l) {
        const int N = g.hidden[l - 1], Kd = g.hidden[l];
        const float* pre = cep_lds + p.off_pre[l - 1];
        float* dst = image(src ^ 1);
        col0 -= N;
        float* Gl = g.G + (size_t)R * col0;
        ro_product<true>(image(src), ld, g.w[l], N, N, Kd, lane, wave, [&](int rr, int n, float v) {
            const float y = v * cep_silu_grad(pre[rr * N + n]);
            dst[rr * ld + n] = y;
            if (row0 + rr < R) Gl[(size_t)(row0 + rr) * N + n] = y;
        });
        __syncthreads();
        src ^= 1;
    }
    float* gf = image(src ^ 1);                 // the obs_proj columns of d / d feat: [16][Ec]
    ro_product<true>(image(src), ld, g.w[0], K0, 2 * Ec, g.hidden[0], lane, wave, [&](int rr, int n, float v) {
        if (n < Ec) gf[rr * ld + n] = v;
        else if (row0 + rr < R) g.G_act[(size_t)(row0 + rr) * Ec + (n - Ec)] = v;
    });
    __syncthreads();
    for (int i = tid; i < groups * Ec; i += 256) {
        const int gi = i / Ec, n = i - gi * Ec;
        const long long row = row0 + gi * K;
        if (row < R) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += gf[(gi * K + k) * ld + n];
            g.G_obs[(size_t)(row / K) * Ec + n] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int cep_fail(const char* what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "cdx_cep_step_f32: %s", what);
    cdx_set_err(msg);
    return CDX_EINVAL;
}

// sizes and the LDS plan: everything that can be checked without touching device memory
int cep_plan(const cdx_cep_step* g, CepPlan* p) {
    if (!g) return cep_fail("null request");
    if (g->B < 0 || g->A <= 0 || g->O <= 0 || g->Ec <= 0) return cep_fail("bad size");
    if (g->K != 1 && g->K != 2 && g->K != 4 && g->K != 8 && g->K != 16) return cep_fail("K must divide 16 (1, 2, 4, 8, 16)");
    if ((long long)g->B * g->K > 0x7fffffffLL - RO_ROWS) return cep_fail("bad size: B K does not fit 32 bits");
    if (g->A > 64) return cep_fail("A must be at most 64");
    if (g->Ec > 128) return cep_fail("Ec must be at most 128");
    if (g->O > 512) return cep_fail("O must be at most 512");
    if (g->n_hidden < 1 || g->n_hidden > CDX_ENERGY_MAX_HIDDEN) return cep_fail("n_hidden must be 1 .. CDX_ENERGY_MAX_HIDDEN");
    int maxw = cep_r16(g->O) > cep_r16(3 * g->Ec) ? cep_r16(g->O) : cep_r16(3 * g->Ec);
    long long pre_floats = 0;
    for (int l = 0; l < g->n_hidden; ++l) {
        const int w = g->hidden[l];
        if (w <= 0 || w % 16 != 0 || w > 512) return cep_fail("hidden width must be a multiple of 16, at most 512");
        maxw = w > maxw ? w : maxw;
        pre_floats += (long long)RO_ROWS * w;
    }
    p->ld = maxw + 4;
    long long at = 2LL * RO_ROWS * p->ld;
    for (int l = 0; l < CDX_ENERGY_MAX_HIDDEN; ++l) {
        p->off_pre[l] = l < g->n_hidden ? (int32_t)at : 0;
        if (l < g->n_hidden) at += (long long)RO_ROWS * g->hidden[l];
    }
    p->off_xs = (int32_t)at; at += (long long)RO_ROWS * CEP_ALD;
    p->off_sc = (int32_t)at; at += CEP_SC;
    p->total = (int32_t)at;
    return CDX_OK;
}

int cep_check(const cdx_cep_step* g, CepPlan* p) {
    const int rc = cep_plan(g, p);
    if (rc != CDX_OK) return rc;
    if ((long long)p->total * (long long)sizeof(float) > CEP_LDS_MAX) return cep_fail("the LDS plan exceeds 160 KiB");
    if (g->B == 0) return CDX_OK;
    if (!g->x || !g->obs || !g->temb || !g->soft) return cep_fail("null pointer: x / obs / temb / soft");
    if (!g->obs_w || !g->obs_b || !g->act_w || !g->act_b || !g->wo || !g->bo) return cep_fail("null pointer: weights");
    for (int l = 0; l < g->n_hidden; ++l)
        if (!g->w[l] || !g->b[l]) return cep_fail("null pointer: weights");
    if (!g->feat || !g->H || !g->G || !g->G_out || !g->G_act || !g->G_obs || !g->stats) return cep_fail("null pointer: outputs");
    return CDX_OK;
}

}  // namespace

extern "C" {

long long cdx_cep_lds_bytes(const cdx_cep_step* g) {
    cdx_set_err("");
    CepPlan p;
    const int rc = cep_plan(g, &p);
    return rc != CDX_OK ? rc : (long long)p.total * (long long)sizeof(float);
}

int cdx_cep_step_f32(const cdx_cep_step* g, void* hip_stream) {
    cdx_set_err("");
    CepArgs a;
    const int rc = cep_check(g, &a.p);
    if (rc != CDX_OK || g->B == 0) return rc;
    a.g = *g;
    const size_t lds = (size_t)a.p.total * sizeof(float);
    static size_t raised = 0;
    if (lds > 48 * 1024 && lds > raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cdx_cep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
        raised = lds;
    }
    const long long R = (long long)g->B * g->K;
    const dim3 grid((unsigned)((R + RO_ROWS - 1) / RO_ROWS));
    hipLaunchKernelGGL(cdx_cep_kernel, grid, dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
    return CDX_OK;
}

}  // extern "C"
