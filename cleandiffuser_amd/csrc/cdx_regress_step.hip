// cdx_regress_step.hip -- a supervised MSE training step of one Linear -> [LayerNorm] -> activation tower against a GIVEN target, for one
// 16-row tile per workgroup: the load of [x0 | x1], the forward, the loss with its gradient and the backward-data pass in ONE launch.
//
// Decision Diffuser and Decision Veteran step an inverse-dynamics head a(o, o') on every gradient update, SfBC re-trains a critic by the
// same step: rows [x0 | x1] through the tower, mean((out - y)^2), backward.  As library nodes that is a concatenation, one launch per
// Linear and activation forward, the loss arithmetic and twice that backward.  Rows are independent and the loss gradient of an element
// depends on that element only, so one workgroup of 4 wave64 owns 16 rows (grid ceil(R / 16)) and runs
//   A  load      [x0 | x1] of its rows into image 0, zero up to the next multiple of 16 columns, and x_cat (R, K0) to global memory (the
//                weight-gradient launch reads it).  x0, x1 and y are read in place through a row map: batch row r is row
//                (r / inner) period + r % inner of a matrix of row stride ld -- a matrix of any row stride (inner 1, period 1; obs[:, 0]
//                of a (B, H, D) batch: ld H D) or obs[:, :-1] / obs[:, 1:] of that batch (inner H - 1, period H, ld D) without a copy;
//   B  forward   tw_forward_layers: H_l of the hidden layers to global memory, P_l and rstd_l to LDS, out (R, W) to global memory and LDS;
//   C  loss      16 lanes per row: e = out - y, d_out = 2 e / (R W) into image 0 (zero in the rows past R and up to the next multiple of
//                16 columns), e^2 into the tile; lane 0 sums the tile's e^2 row-major: loss_part[tile] = sum / (R W);
//   D  backward  tw_backward_layers from d_out on the P_l / rstd_l in LDS: G_l, Sb, Sg to global memory in cdx_critic_step's layout.
// No atomics, every element is produced by one fixed lane in one fixed order: bit-reproducible.  The weight, bias, gain and shift sums
// over the rows and tiles are the caller's (include/cdx.h).
//
// The LDS plan, in floats (regress_plan; engine/regress_step.py: lds_bytes restates it): two images [16][ld], ld = the widest of K0 and
// the widths (next multiple of 16) + 4; P_l [16][width[l]] of every layer; rstd [n_layers][16]; the out / e^2 tile [16][64].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"
#include "cdx_tower_layers.h"

namespace {

constexpr long long RS_LDS_MAX = 160 * 1024;

struct RegressPlan {
    int32_t ld;                                   // row stride of the two images
    int32_t off_col[CDX_TOWER_MAX_LAYERS];        // the widths before layer l: H_l / G_l start at float R * off_col[l], P_l in LDS at 16 * off_col[l]
    int32_t cols;                                 // the sum of the widths
    int32_t at_p, at_rstd, at_tile;
    int32_t total;
};

struct RegressArgs {
    cdx_regress_step g;
    RegressPlan p;
};
static_assert(sizeof(RegressArgs) <= 4096, "the kernel argument segment holds 4 KiB");

// where batch row `row` of an operand starts, in floats from its pointer
__device__ __forceinline__ size_t rs_row_at(const cdx_regress_rows& o, long long row) {
    const unsigned r = (unsigned)row, inner = (unsigned)o.inner;       // (row < R <= 2^31 - 17)
    const unsigned blk = r / inner;
    return ((size_t)blk * (size_t)o.period + (size_t)(r - blk * inner)) * (size_t)o.ld;
}

// the forward's results: H_l to global memory, P_l and rstd_l to LDS, the tower's output to both
struct RegressSave {
    const cdx_regress_step& g;
    const RegressPlan& p;
    float* lds;
    long long R, row0;
    __device__ void element(int l, int r, int c, float h, float pre) const {
        const int W = g.net.width[l];
        lds[p.at_p + RO_ROWS * p.off_col[l] + r * W + c] = pre;
        if (l == g.net.n_layers - 1) {
            lds[p.at_tile + r * RO_XLD + c] = h;
            if (row0 + r < R) g.out[(size_t)(row0 + r) * W + c] = h;
        } else if (row0 + r < R) {
            (g.H + (size_t)R * p.off_col[l])[(size_t)(row0 + r) * W + c] = h;
        }
    }
    __device__ void row_rstd(int l, int r, float rstd) const { lds[p.at_rstd + l * RO_ROWS + r] = rstd; }
};
struct RegressSaved {
    const cdx_regress_step& g;
    const RegressPlan& plan;
    const float* lds;
    long long R, row0;
    __device__ float p(int l, int r, int c) const {
        return row0 + r < R ? lds[plan.at_p + RO_ROWS * plan.off_col[l] + r * g.net.width[l] + c] : 0.f;
    }
    __device__ float rstd(int l, int r) const { return row0 + r < R ? lds[plan.at_rstd + l * RO_ROWS + r] : 0.f; }
};
struct RegressGrads {
    const cdx_regress_step& g;
    const RegressPlan& p;
    long long R, row0, tiles, tile;
    __device__ void element(int l, int r, int c, float dz) const {
        if (row0 + r < R) (g.G + (size_t)R * p.off_col[l])[(size_t)(row0 + r) * g.net.width[l] + c] = dz;
    }
    __device__ void sums(int l, int c, float sb, float sg) const {
        const size_t at = (size_t)tiles * p.off_col[l] + (size_t)tile * g.net.width[l] + c;
        g.Sb[at] = sb;
        g.Sg[at] = sg;
    }
    __device__ void gx(int, int, float) const {}
};

__global__ __launch_bounds__(256) void cdx_regress_step_kernel(const RegressArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const cdx_regress_step& g = a.g;
    const RegressPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = tid >> 4, sub = tid & 15;          // the loader's and the loss's view: 16 lanes per row
    const int ld = p.ld, K0 = g.net.K0, A0 = g.x0.width, W = g.net.width[g.net.n_layers - 1];
    const long long R = g.R, row0 = (long long)blockIdx.x * RO_ROWS, tile = blockIdx.x, row = row0 + rr;
    float* img0 = rs_lds;
    float* img1 = rs_lds + (size_t)RO_ROWS * ld;
    float* tl = rs_lds + p.at_tile;                   // [16][RO_XLD]: out, then e^2

    // A. the rows [x0 | x1]
    {
        const bool live = row < R;
        const float* s0 = live ? g.x0.ptr + rs_row_at(g.x0, row) : nullptr;
        const float* s1 = live && g.x1.width ? g.x1.ptr + rs_row_at(g.x1, row) : nullptr;
        for (int c = sub; c < ro_r16(K0); c += 16) {
            float v = 0.f;
            if (live && c < K0) {
                v = c < A0 ? s0[c] : s1[c - A0];
                g.x_cat[(size_t)row * K0 + c] = v;
            }
            img0[rr * ld + c] = v;
        }
    }
    __syncthreads();

    // B. the forward
    tw_forward_layers(g.net, 0, K0, img0, ld, img1, img0, ld, tid, lane, wave, RegressSave{g, p, rs_lds, R, row0});

    // C. the loss and its gradient
    {
        const bool live = row < R;
        const float* ys = live ? g.y.ptr + rs_row_at(g.y, row) : nullptr;
        const float inv = 1.0f / ((float)R * (float)W);
        for (int c = sub; c < ro_r16(W); c += 16) {
            float e = 0.f;
            if (live && c < W) e = tl[rr * RO_XLD + c] - ys[c];
            img0[rr * ld + c] = 2.0f * e * inv;
            if (c < W) tl[rr * RO_XLD + c] = e * e;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int r = 0; r < RO_ROWS; ++r)
            for (int c = 0; c < W; ++c) s += tl[r * RO_XLD + c];
        g.loss_part[tile] = s / ((float)R * (float)W);
    }

    // D. backward-data
    tw_backward_layers(g.net, 0, K0, img0, img1, ld, tid, lane, wave, true, false, RegressSaved{g, p, rs_lds, R, row0},
                       RegressGrads{g, p, R, row0, (long long)gridDim.x, tile});
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// sizes and the LDS plan: everything that can be checked without touching device memory
int regress_plan(const char* who, const cdx_regress_step* g, RegressPlan* p) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (!g) return fail("null request");
    if (g->R < 0 || (long long)g->R > 0x7fffffffLL - RO_ROWS) return fail("bad size: R");
    const cdx_critic_net& n = g->net;
    if (n.n_towers != 1) return fail("n_towers must be 1");
    if (n.K0 <= 0 || n.K0 > RO_MAX_WIDTH) return fail("K0 must be 1 .. 512");
    int maxw = 0;
    const int rc = tw_check_layers(n.n_layers, n.width, n.norm, n.act, n.eps, &maxw, fail);
    if (rc != CDX_OK) return rc;
    maxw = ro_r16(n.K0) > maxw ? ro_r16(n.K0) : maxw;
    if (g->x0.width < 1 || g->x1.width < 0 || (long long)g->x0.width + g->x1.width != n.K0) return fail("A0 >= 1 and A0 + A1 must be K0");
    if (g->y.width != n.width[n.n_layers - 1]) return fail("the width of y must be the last width");
    const cdx_regress_rows* ops[3] = {&g->x0, &g->x1, &g->y};
    for (const cdx_regress_rows* o : ops) {
        if (o->width == 0) continue;
        if (o->inner < 1 || o->period < o->inner) return fail("the row map needs inner >= 1 and period >= inner");
        if (o->ld < 1) return fail("the row stride must be positive");
    }
    int cols = 0;
    for (int l = 0; l < CDX_TOWER_MAX_LAYERS; ++l) {
        p->off_col[l] = l < n.n_layers ? cols : 0;
        cols += l < n.n_layers ? n.width[l] : 0;
    }
    p->cols = cols;
    p->ld = maxw + 4;
    p->at_p = 2 * RO_ROWS * p->ld;
    p->at_rstd = p->at_p + RO_ROWS * cols;
    p->at_tile = p->at_rstd + RO_ROWS * n.n_layers;
    p->total = p->at_tile + RO_ROWS * RO_XLD;
    return CDX_OK;
}

int regress_check(const char* who, const cdx_regress_step* g, RegressPlan* p) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    const int rc = regress_plan(who, g, p);
    if (rc != CDX_OK) return rc;
    if ((long long)p->total * (long long)sizeof(float) > RS_LDS_MAX) return fail("the LDS plan exceeds 160 KiB");
    if (g->R == 0) return CDX_OK;
    if (!g->x0.ptr || (g->x1.width != 0) != (g->x1.ptr != nullptr)) return fail("null pointer: x0 / x1");
    if (!g->y.ptr) return fail("null pointer: y");
    const cdx_critic_net& n = g->net;
    for (int l = 0; l < n.n_layers; ++l) {
        if (!n.w[0][l] || !n.b[0][l]) return fail("null pointer: weights");
        if (n.norm[l] && (!n.gamma[0][l] || !n.beta[0][l])) return fail("null pointer: norm parameters");
    }
    if (!g->out || !g->loss_part || !g->x_cat) return fail("null pointer: out / loss_part / x_cat");
    if (n.n_layers > 1 && !g->H) return fail("null pointer: H");
    if (!g->G || !g->Sb || !g->Sg) return fail("null pointer: G / Sb / Sg");
    return CDX_OK;
}

}  // namespace

extern "C" {

long long cdx_regress_step_lds_bytes(const cdx_regress_step* g) {
    cdx_set_err("");
    RegressPlan p;
    const int rc = regress_plan("cdx_regress_step_lds_bytes", g, &p);
    return rc != CDX_OK ? rc : (long long)p.total * (long long)sizeof(float);
}

int cdx_regress_step_f32(const cdx_regress_step* g, void* hip_stream) {
    static size_t raised = 0;
    cdx_set_err("");
    RegressArgs a;
    const int rc = regress_check("cdx_regress_step_f32", g, &a.p);
    if (rc != CDX_OK || g->R == 0) return rc;
    a.g = *g;
    return ro_launch_tiles(cdx_regress_step_kernel, a, g->R, (size_t)a.p.total * sizeof(float), hip_stream, raised);
}

}  // extern "C"
