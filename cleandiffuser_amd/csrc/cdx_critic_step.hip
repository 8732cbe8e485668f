// cdx_critic_step.hip -- a critic's TD or expectile training step, for one 16-row tile of one live tower per workgroup: the no-grad target
// evaluation, y = rew + discount (1 - done) T, the live forward, the loss with its gradient and the backward-data pass in ONE launch.
//
// The dql / edp / idql / qgpo pipelines step a value critic on every gradient update.  With the towers on one forward and one backward
// launch (cdx_tower.hip) the step is still a chain of small kernels around them: the target towers, the reduction over the target rows,
// the TD expression, the loss, its backward and autograd's accumulations.  Rows are independent and the loss gradient of a row depends
// on that row only, so one workgroup of 4 wave64 owns 16 live rows of one live tower (grid (ceil(R / 16), live.n_towers)) and runs
//   A  target    K passes; pass j loads [z0[row] | z1[row K + j]] and runs every target tower's forward (tw_forward_layers, nothing kept);
//                lane r < 16 then reduces the K x towers values of its row to T in one fixed order and forms y;
//   B  forward   the live tower on [x0 | x1]: H_l to global memory (the weight-gradient launch reads it), P_l and rstd_l to LDS;
//   C  loss      lane r < 16: l and dq of its row; lane 0 sums the tile's l and y in row order;
//   D  backward  tw_backward_layers from dq on the P_l / rstd_l in LDS: G_l, Sb, Sg to global memory.
// With two live towers both workgroups of a tile run phase A on the same inputs in the same order (the CUs a batch of a few hundred
// rows leaves idle absorb it) and tower 0 writes y.  No atomics, every element is produced by one fixed lane in one fixed order:
// bit-reproducible.  The weight, bias, gain and shift sums over the rows and tiles are the caller's (include/cdx.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"
#include "cdx_tower_layers.h"

namespace {

constexpr long long CS_LDS_MAX = 160 * 1024;

// the LDS plan, in floats
struct CriticPlan {
    int32_t ld;                                   // row stride of the two images: the widest operand of both nets (next multiple of 16) + 4
    int32_t off_col[CDX_TOWER_MAX_LAYERS];        // the live widths before layer l: H_l / G_l start at float R * off_col[l], P_l in LDS at 16 * off_col[l]
    int32_t cols;                                 // the sum of the live widths
    int32_t at_p, at_rstd, at_tq, at_row;         // P_l [16][width[l]] per layer; rstd [n_layers][16]; target values [2][K][16]; y, q, dq, l [4][16]
    int32_t total;
};

struct CriticArgs {
    cdx_critic_step g;
    CriticPlan p;
};
static_assert(sizeof(CriticArgs) <= 4096, "the kernel argument segment holds 4 KiB");

// torch.min / torch.max on two values: a NaN stays
__device__ __forceinline__ float cs_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float cs_max(float a, float b) { return (a > b || a != a) ? a : b; }

// the live forward's results: H_l of the live rows to global memory, P_l, rstd_l and the tower's output to LDS
struct CriticSave {
    const cdx_critic_step& g;
    const CriticPlan& p;
    float* lds;
    int t;
    long long R, row0;
    __device__ void element(int l, int r, int c, float h, float pre) const {
        const int W = g.live.width[l];
        lds[p.at_p + RO_ROWS * p.off_col[l] + r * W + c] = pre;
        if (l == g.live.n_layers - 1) {
            lds[p.at_row + RO_ROWS + r] = h;
            if (row0 + r < R) g.q_out[t][row0 + r] = h;
        } else if (row0 + r < R) {
            (g.H[t] + (size_t)R * p.off_col[l])[(size_t)(row0 + r) * W + c] = h;
        }
    }
    __device__ void row_rstd(int l, int r, float rstd) const { lds[p.at_rstd + l * RO_ROWS + r] = rstd; }
};
struct CriticSaved {
    const cdx_critic_step& g;
    const CriticPlan& plan;
    const float* lds;
    long long R, row0;
    __device__ float p(int l, int r, int c) const {
        return row0 + r < R ? lds[plan.at_p + RO_ROWS * plan.off_col[l] + r * g.live.width[l] + c] : 0.f;
    }
    __device__ float rstd(int l, int r) const { return row0 + r < R ? lds[plan.at_rstd + l * RO_ROWS + r] : 0.f; }
};
struct CriticGrads {
    const cdx_critic_step& g;
    const CriticPlan& p;
    int t;
    long long R, row0, tiles, tile;
    __device__ void element(int l, int r, int c, float dz) const {
        if (row0 + r < R) (g.G[t] + (size_t)R * p.off_col[l])[(size_t)(row0 + r) * g.live.width[l] + c] = dz;
    }
    __device__ void sums(int l, int c, float sb, float sg) const {
        const size_t at = (size_t)tiles * p.off_col[l] + (size_t)tile * g.live.width[l] + c;
        g.Sb[t][at] = sb;
        g.Sg[t][at] = sg;
    }
    __device__ void gx(int, int, float) const {}
};

__global__ __launch_bounds__(256) void cdx_critic_step_kernel(const CriticArgs a) {
    extern __shared__ __attribute__((aligned(16))) float cs_lds[];
    const cdx_critic_step& g = a.g;
    const CriticPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.y, ld = p.ld, K = g.K;
    const long long R = g.R, row0 = (long long)blockIdx.x * RO_ROWS, tile = blockIdx.x;
    auto image = [&](int i) { return cs_lds + (size_t)i * RO_ROWS * ld; };
    float* tq = cs_lds + p.at_tq;                     // [tower][pass][row]
    float* y_s = cs_lds + p.at_row;                   // then q, dq, l: [16] each
    float* q_s = y_s + RO_ROWS;
    float* dq_s = q_s + RO_ROWS;
    float* l_s = dq_s + RO_ROWS;

    // A. the target
    const int Kt = g.target.K0, Lt = g.target.n_layers;
    const float* t_out = image(Lt & 1);               // (layer l writes image((l & 1) ^ 1): the last one image(Lt & 1))
    for (int j = 0; j < K; ++j) {
        for (int tt = 0; tt < g.target.n_towers; ++tt) {
            if (g.B0) ro_load_rows(image(0), ld, g.B1 ? g.B0 : ro_r16(Kt), g.z0, g.B0, row0, R, tid, [](long long row) { return row; });
            if (g.B1)
                ro_load_rows(image(0) + g.B0, ld, ro_r16(Kt) - g.B0, g.z1, g.B1, row0, R, tid, [=](long long row) { return row * K + j; });
            __syncthreads();
            tw_forward_layers(g.target, tt, Kt, image(0), ld, image(1), image(0), ld, tid, lane, wave, TwKeepNothing{});
            if (tid < RO_ROWS) tq[(tt * CDX_CRITIC_MAX_K + j) * RO_ROWS + tid] = t_out[tid * ld];
            __syncthreads();
        }
    }
    if (tid < RO_ROWS) {
        const long long row = row0 + tid;
        auto q_of = [&](int tt, int j) { return tq[(tt * CDX_CRITIC_MAX_K + j) * RO_ROWS + tid]; };
        auto q_min = [&](int j) { return g.target.n_towers == 2 ? cs_min(q_of(0, j), q_of(1, j)) : q_of(0, j); };
        float T;
        if (g.reduce == CDX_CRITIC_SOFTMAX) {
            float m = g.beta * q_min(0);
            for (int j = 1; j < K; ++j) m = cs_max(m, g.beta * q_min(j));
            float num = 0.f, den = 0.f;
            for (int j = 0; j < K; ++j) {
                const float q = q_min(j), w = expf(g.beta * q - m);
                den += w;
                num += w * q;
            }
            T = num / den;
        } else {                                      // (CDX_CRITIC_MIN is K == 1)
            T = 0.f;
            for (int tt = 0; tt < g.target.n_towers; ++tt) {
                float m = q_of(tt, 0);
                for (int j = 1; j < K; ++j) m = cs_max(m, q_of(tt, j));
                T = tt ? cs_min(T, m) : m;
            }
        }
        float y = 0.f;
        if (row < R) {
            y = g.rew ? g.rew[row] + g.discount * (1.0f - g.done[row]) * T : T;
            if (t == 0) g.y_out[row] = y;
        }
        y_s[tid] = y;
    }

    // B. the live forward
    const int K0 = g.live.K0;
    for (int i = tid; i < RO_ROWS * ro_r16(K0); i += 256) {
        const int rr = i / ro_r16(K0), c = i - rr * ro_r16(K0);
        const long long row = row0 + rr;
        float v = 0.f;
        if (row < R && c < K0) {
            v = c < g.A0 ? g.x0[(size_t)row * g.A0 + c] : g.x1[(size_t)row * g.A1 + (c - g.A0)];
            if (t == 0) g.x_cat[(size_t)row * K0 + c] = v;
        }
        image(0)[rr * ld + c] = v;
    }
    __syncthreads();
    tw_forward_layers(g.live, t, K0, image(0), ld, image(1), image(0), ld, tid, lane, wave, CriticSave{g, p, cs_lds, t, R, row0});

    // C. the loss and its gradient
    if (tid < RO_ROWS) {
        float l = 0.f, dq = 0.f;
        if (row0 + tid < R) {
            const float q = q_s[tid], y = y_s[tid], inv = 1.0f / (float)R;
            if (g.loss == CDX_CRITIC_EXPECTILE) {
                const float adv = y - q, w = fabsf(g.tau - (adv < 0.f ? 1.0f : 0.f));
                l = w * adv * adv;
                dq = -2.0f * w * adv * inv;
            } else {
                const float e = q - y;
                l = e * e;
                dq = 2.0f * e * inv;
            }
        }
        l_s[tid] = l;
        dq_s[tid] = dq;
    }
    __syncthreads();
    if (tid == 0) {
        float sl = 0.f, sy = 0.f;
        for (int r = 0; r < RO_ROWS; ++r) {
            sl += l_s[r];
            sy += y_s[r];
        }
        g.loss_part[t][tile] = sl / (float)R;
        if (t == 0) g.y_part[tile] = sy / (float)R;
    }
    for (int i = tid; i < RO_ROWS * RO_ROWS; i += 256) image(0)[(i >> 4) * ld + (i & 15)] = (i & 15) ? 0.f : dq_s[i >> 4];
    __syncthreads();

    // D. backward-data
    tw_backward_layers(g.live, t, K0, image(0), image(1), ld, tid, lane, wave, true, false, CriticSaved{g, p, cs_lds, R, row0},
                       CriticGrads{g, p, t, R, row0, (long long)gridDim.x, tile});
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
template <class Fail>
int critic_net_check(const cdx_critic_net& n, int* maxw, Fail fail) {
    if (n.n_towers != 1 && n.n_towers != 2) return fail("n_towers must be 1 or 2");
    if (n.K0 <= 0 || n.K0 > RO_MAX_WIDTH) return fail("K0 must be 1 .. 512");
    const int rc = tw_check_layers(n.n_layers, n.width, n.norm, n.act, n.eps, maxw, fail);
    if (rc != CDX_OK) return rc;
    if (n.width[n.n_layers - 1] != 1) return fail("the last width must be 1");
    *maxw = ro_r16(n.K0) > *maxw ? ro_r16(n.K0) : *maxw;
    return CDX_OK;
}

// sizes and the LDS plan: everything that can be checked without touching device memory
int critic_plan(const char* who, const cdx_critic_step* g, CriticPlan* p) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (!g) return fail("null request");
    if (g->K < 1 || g->K > CDX_CRITIC_MAX_K) return fail("K must be 1 .. CDX_CRITIC_MAX_K");
    if (g->R < 0 || (long long)g->R * g->K > 0x7fffffffLL - RO_ROWS) return fail("bad size: R");
    if (g->reduce != CDX_CRITIC_MIN && g->reduce != CDX_CRITIC_MAX && g->reduce != CDX_CRITIC_SOFTMAX) return fail("unknown reduction");
    if (g->reduce == CDX_CRITIC_MIN && g->K != 1) return fail("CDX_CRITIC_MIN takes K == 1");
    if (g->loss != CDX_CRITIC_MSE && g->loss != CDX_CRITIC_EXPECTILE) return fail("unknown loss");
    int wl = 0, wt = 0;
    int rc = critic_net_check(g->live, &wl, fail);
    if (rc != CDX_OK) return rc;
    rc = critic_net_check(g->target, &wt, fail);
    if (rc != CDX_OK) return rc;
    if (g->A0 < 1 || g->A1 < 0 || g->A0 + g->A1 != g->live.K0) return fail("A0 + A1 must be the live K0");
    if (g->B0 < 0 || g->B1 < 0 || g->B0 + g->B1 != g->target.K0) return fail("B0 + B1 must be the target K0");
    if (g->K > 1 && g->B1 == 0) return fail("K > 1 needs z1");
    int cols = 0;
    for (int l = 0; l < CDX_TOWER_MAX_LAYERS; ++l) {
        p->off_col[l] = l < g->live.n_layers ? cols : 0;
        cols += l < g->live.n_layers ? g->live.width[l] : 0;
    }
    p->cols = cols;
    p->ld = (wl > wt ? wl : wt) + 4;
    p->at_p = 2 * RO_ROWS * p->ld;
    p->at_rstd = p->at_p + RO_ROWS * cols;
    p->at_tq = p->at_rstd + RO_ROWS * g->live.n_layers;
    p->at_row = p->at_tq + 2 * CDX_CRITIC_MAX_K * RO_ROWS;
    p->total = p->at_row + 4 * RO_ROWS;
    return CDX_OK;
}

int critic_check(const char* who, const cdx_critic_step* g, CriticPlan* p) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    const int rc = critic_plan(who, g, p);
    if (rc != CDX_OK) return rc;
    if ((long long)p->total * (long long)sizeof(float) > CS_LDS_MAX) return fail("the LDS plan exceeds 160 KiB");
    if (g->R == 0) return CDX_OK;
    if (!g->x0 || (g->A1 != 0) != (g->x1 != nullptr)) return fail("null pointer: x0 / x1");
    if ((g->B0 != 0) != (g->z0 != nullptr) || (g->B1 != 0) != (g->z1 != nullptr)) return fail("null pointer: z0 / z1");
    if ((g->rew != nullptr) != (g->done != nullptr)) return fail("rew and done come together");
    if (!g->y_out || !g->y_part || !g->x_cat) return fail("null pointer: y_out / y_part / x_cat");
    for (int k = 0; k < 2; ++k) {
        const cdx_critic_net& n = k ? g->target : g->live;
        for (int t = 0; t < n.n_towers; ++t)
            for (int l = 0; l < n.n_layers; ++l) {
                if (!n.w[t][l] || !n.b[t][l]) return fail("null pointer: weights");
                if (n.norm[l] && (!n.gamma[t][l] || !n.beta[t][l])) return fail("null pointer: norm parameters");
            }
    }
    for (int t = 0; t < g->live.n_towers; ++t) {
        if (!g->q_out[t] || !g->loss_part[t]) return fail("null pointer: q_out / loss_part");
        if (g->live.n_layers > 1 && !g->H[t]) return fail("null pointer: H");
        if (!g->G[t] || !g->Sb[t] || !g->Sg[t]) return fail("null pointer: G / Sb / Sg");
    }
    return CDX_OK;
}

}  // namespace

extern "C" {

long long cdx_critic_step_lds_bytes(const cdx_critic_step* g) {
    cdx_set_err("");
    CriticPlan p;
    const int rc = critic_plan("cdx_critic_step_lds_bytes", g, &p);
    return rc != CDX_OK ? rc : (long long)p.total * (long long)sizeof(float);
}

int cdx_critic_step_f32(const cdx_critic_step* g, void* hip_stream) {
    static size_t raised = 0;
    cdx_set_err("");
    CriticArgs a;
    const int rc = critic_check("cdx_critic_step_f32", g, &a.p);
    if (rc != CDX_OK || g->R == 0) return rc;
    a.g = *g;
    return ro_launch_tiles(cdx_critic_step_kernel, a, g->R, (size_t)a.p.total * sizeof(float), hip_stream, raised, (unsigned)g->live.n_towers);
}

}  // extern "C"
