// cdx_cep.hip -- QGPO's contrastive energy training step (forward, loss, backward-data) for one 16-row tile per workgroup.
//
// The energy model of QGPO is trained by ``clf.update(noisy_act, t, {"soft_label", "obs"})`` once per gradient step (reference
// pipelines/qgpo_d4rl_mujoco.py:172-212 over classifier/qgpo_classifier.py:16-61): B states x K support actions, R = B K rows of a
// 3 x 256 SiLU MLP, the loss a cross entropy between the soft labels and the softmax of the energies over the K rows of a state.  As
// autograd that is about a hundred launches of a few microseconds each.  Rows of different states are independent and K divides 16, so
// one workgroup of 4 wave64 owns 16 consecutive rows -- 16 / K whole softmax groups -- and runs, with the product routine of the row-tile
// kernels (cdx_rowtile.h: activations in LDS, weights from global memory, v_mfma_f32_16x16x4_f32) and its one energy model (cdx_energy_mlp.h):
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
#include "cdx_energy_mlp.h"
#include "cdx_rowtile.h"

namespace {

constexpr int CEP_SC = 64;       // the per-row scalars: f, 1 - tanh^2, dL/do (16 each)
constexpr long long CEP_LDS_MAX = 160 * 1024;

// the LDS plan, in floats: two activation images [16][ld], the saved pre-activations [16][hidden[l]], the action tile, the scalars
struct CepPlan {
    int32_t ld;                                   // row stride of the activation images: the widest operand + 4
    int32_t off_pre[CDX_ENERGY_MAX_HIDDEN];
    int32_t off_col[CDX_ENERGY_MAX_HIDDEN];       // the widths before layer l: its (R, hidden[l]) matrix starts at float R * off_col[l] of H / G
    int32_t off_xs, off_sc, total;
};

struct CepArgs {
    cdx_cep_step g;
    CepPlan p;
};
static_assert(sizeof(CepArgs) <= 4096, "the kernel argument segment holds 4 KiB");

__global__ __launch_bounds__(256) void cdx_cep_kernel(const CepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cep_lds[];
    const cdx_cep_step& g = a.g;
    const CepPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = g.K, A = g.A, O = g.O, Ec = g.Ec, L = g.n_hidden, ld = p.ld;
    const long long R = (long long)g.B * K;
    const long long row0 = (long long)blockIdx.x * RO_ROWS;
    const int K0 = 3 * Ec;
    float* xs = cep_lds + p.off_xs;             // [16][RO_ALD] the noisy actions, zero past A
    float* sc_f = cep_lds + p.off_sc;           // [16] f
    float* sc_dt = sc_f + RO_ROWS;              // [16] 1 - tanh^2(o / 10)
    float* sc_go = sc_dt + RO_ROWS;             // [16] dL/do
    const EmNet net{L, Ec, g.hidden, g.w, g.b, g.wo, g.bo, cep_lds, ld, p.off_pre};
    // H / G of layer l: element (tile row rr, column n)
    auto keep = [&](float* buf, int l) {
        float* m = buf + (size_t)R * p.off_col[l];
        const int W = g.hidden[l];
        return [=](int rr, int n, float v) { if (row0 + rr < R) m[(size_t)(row0 + rr) * W + n] = v; };
    };

    // ---- the tile's inputs: actions, the observation of each row's state, the time columns of feat ----
    ro_load_rows(xs, RO_ALD, RO_ALD, g.x, A, row0, R, tid, [](long long row) { return row; });
    float* feat = net.image(1);
    {
        float* ot = net.image(0);
        ro_load_rows(ot, ld, ro_r16(O), g.obs, O, row0, R, tid, [&](long long row) { return row / K; });
        const int nt = ro_r16(K0) - 2 * Ec;    // the time columns and the zero columns up to the next multiple of 16
        for (int i = tid; i < RO_ROWS * nt; i += 256) {
            const int rr = i / nt, c = 2 * Ec + (i - rr * nt);
            const long long row = row0 + rr;
            const bool live = c < K0 && row < R;
            const float v = live ? g.temb[(size_t)(row / K) * Ec + (c - 2 * Ec)] : 0.f;
            feat[rr * ld + c] = v;
            if (live) g.feat[(size_t)row * K0 + c] = v;
        }
        __syncthreads();
        em_obs_proj(ot, ld, g.obs_w, g.obs_b, O, Ec, lane, wave, [&](int rr, int n, float y) {
            feat[rr * ld + n] = y;
            if (row0 + rr < R) g.feat[(size_t)(row0 + rr) * K0 + n] = y;
        });
        em_act_proj(xs, feat, ld, g.act_w, g.act_b, A, Ec, lane, wave, [&](int rr, int n, float y) {
            if (row0 + rr < R) g.feat[(size_t)(row0 + rr) * K0 + Ec + n] = y;
        });
        __syncthreads();
    }

    // ---- forward: the hidden layers (pre-activations stay in LDS, activations go to H), the head ----
    int src = em_forward(net, 1, lane, wave, [&](int l) { return keep(g.H, l); });
    em_head(net, src, sc_f, sc_dt, lane, wave);

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
    src = em_backward<true>(net, g.w, sc_go, src ^ 1, tid, lane, wave, [&](int l) { return keep(g.G, l); });
    float* gf = net.image(src ^ 1);                 // the obs_proj columns of d / d feat: [16][Ec]
    ro_product<true>(net.image(src), ld, g.w[0], K0, 2 * Ec, g.hidden[0], lane, wave, [&](int rr, int n, float v) {
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
int cep_fail(const char* what) { return ro_fail("cdx_cep_step_f32", what); }

// sizes and the LDS plan: everything that can be checked without touching device memory
int cep_plan(const cdx_cep_step* g, CepPlan* p) {
    if (!g) return cep_fail("null request");
    if (g->B < 0 || g->A <= 0 || g->O <= 0 || g->Ec <= 0) return cep_fail("bad size");
    if (g->K != 1 && g->K != 2 && g->K != 4 && g->K != 8 && g->K != 16) return cep_fail("K must divide 16 (1, 2, 4, 8, 16)");
    if ((long long)g->B * g->K > 0x7fffffffLL - RO_ROWS) return cep_fail("bad size: B K does not fit 32 bits");
    EmPlan net;
    const int rc = em_plan(g->A, g->O, g->Ec, g->n_hidden, g->hidden, &net, cep_fail, "Ec must be at most 128",
                           "hidden width must be a multiple of 16, at most 512");
    if (rc != CDX_OK) return rc;
    p->ld = net.maxw + 4;
    long long at = 2LL * RO_ROWS * p->ld;
    for (int l = 0; l < CDX_ENERGY_MAX_HIDDEN; ++l) {
        p->off_col[l] = net.off_col[l];
        p->off_pre[l] = l < g->n_hidden ? (int32_t)(at + RO_ROWS * net.off_col[l]) : 0;
    }
    at += net.pre_floats;
    p->off_xs = (int32_t)at; at += (long long)RO_ROWS * RO_ALD;
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
    return ro_launch_tiles(cdx_cep_kernel, a, (long long)g->B * g->K, lds, hip_stream, raised);   // (cep_plan: B K fits 32 bits)
}

}  // extern "C"
