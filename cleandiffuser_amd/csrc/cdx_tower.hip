// cdx_tower.hip -- the critics' Linear -> [LayerNorm] -> activation towers, forward and backward-data, for one 16-row tile per workgroup.
//
// DQLCritic, TwinQ and V (utils/critics.py; reference utils/building_blocks.py:111-147, utils/iql.py:7-37) are stepped on every gradient
// update of the dql / edp / idql / qgpo pipelines.  As library nodes a tower costs one launch per Linear, LayerNorm and activation forward
// and about twice that backward: a TwinQ.both with its backward is about 40 launches of a few microseconds of work each.  Rows are
// independent, so one workgroup of 4 wave64 owns 16 rows of one tower (grid (ceil(R / 16), n_towers): twin towers read the same rows) and
// runs, with the product routine of the row-tile kernels (cdx_rowtile.h: activations in LDS, weights from global memory,
// v_mfma_f32_16x16x4_f32),
//   forward   per layer z = h W^T + b (ro_product<false>); with a norm, 16 lanes per row take the mean and then the biased variance of the
//             centred values over the row in LDS (two passes, a fixed butterfly), xhat = (z - mean) rstd, y = xhat gamma + beta; h = act(y);
//   backward  per layer from the top: y from the saved P_l (xhat or z), dy = dH act'(y), with a norm g = dy gamma,
//             dz = rstd (g - mean(g) - xhat mean(g xhat)) and the tile's column sums of dy and dy xhat (rows in order), then
//             dH_{l-1} = dz W_l on the live weight (ro_product<true>); at layer 0 that is g_x.  (tw_backward_layers of cdx_tower_layers.h,
//             which cdx_critic_step.hip runs too.)
// H_l, P_l, rstd_l (forward) and G_l = dz, Sb, Sg (backward) go to global memory: the weight and bias sums over the rows are the caller's
// (one cdx_conv_wgrad_batch_f32), the gain and shift sums over the tiles one cdx_colsum_batch_f32 (below).  Rows of the last tile past R
// carry a zero gradient and nothing is written for them.  No atomics in the two tower kernels, every element is produced by one fixed
// lane in one fixed order: bit-reproducible.  The forward's per-layer body lives in cdx_tower_layers.h, which cdx_select.hip runs too.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_act.h"
#include "cdx_rowtile.h"
#include "cdx_tower_layers.h"

namespace {

constexpr long long TW_LDS_MAX = 160 * 1024;

// the LDS plan, in floats: two activation images [16][ld]
struct TowerPlan {
    int32_t ld;                                   // row stride of the images: the widest operand (up to the next multiple of 16) + 4
    int32_t off_col[CDX_TOWER_MAX_LAYERS];        // the widths before layer l: its (R, width[l]) matrix starts at float R * off_col[l]
    int32_t total;
};

struct TowerArgs {
    cdx_tower g;
    TowerPlan p;
};
static_assert(sizeof(TowerArgs) <= 4096, "the kernel argument segment holds 4 KiB");

// what the forward writes to global memory for the live rows of its tile: the last layer's h to out, and with `save` H_l, P_l, rstd_l
struct TowerSave {
    const cdx_tower& g;
    const TowerPlan& p;
    int t;
    long long R, row0;
    __device__ void element(int l, int r, int c, float h, float pre) const {
        if (row0 + r >= R) return;
        const int W = g.width[l];
        const size_t at = (size_t)(row0 + r) * W + c;
        if (l == g.n_layers - 1) g.out[t][at] = h;
        else if (g.save) (g.H[t] + (size_t)R * p.off_col[l])[at] = h;
        if (g.save) (g.P[t] + (size_t)R * p.off_col[l])[at] = pre;
    }
    __device__ void row_rstd(int l, int r, float rstd) const {
        if (row0 + r < R && g.save) g.rstd[t][(size_t)l * R + (row0 + r)] = rstd;
    }
};

// what the backward reads of the forward's buffers, and where its results go
struct TowerSaved {
    const cdx_tower& g;
    const TowerPlan& plan;
    int t;
    long long R, row0;
    __device__ float p(int l, int r, int c) const {
        return row0 + r < R ? (g.P[t] + (size_t)R * plan.off_col[l])[(size_t)(row0 + r) * g.width[l] + c] : 0.f;
    }
    __device__ float rstd(int l, int r) const { return row0 + r < R ? g.rstd[t][(size_t)l * R + (row0 + r)] : 0.f; }
};
struct TowerGrads {
    const cdx_tower& g;
    const TowerPlan& p;
    int t;
    long long R, row0, tiles, tile;
    __device__ void element(int l, int r, int c, float dz) const {
        if (row0 + r < R) (g.G[t] + (size_t)R * p.off_col[l])[(size_t)(row0 + r) * g.width[l] + c] = dz;
    }
    __device__ void sums(int l, int c, float sb, float sg) const {
        const size_t at = (size_t)tiles * p.off_col[l] + (size_t)tile * g.width[l] + c;
        g.Sb[t][at] = sb;
        g.Sg[t][at] = sg;
    }
    __device__ void gx(int r, int n, float v) const {
        if (row0 + r < R) g.g_x[t][(size_t)(row0 + r) * g.K0 + n] = v;
    }
};

__global__ __launch_bounds__(256) void cdx_tower_fwd_kernel(const TowerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    const cdx_tower& g = a.g;
    const TowerPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.y, ld = p.ld;
    const long long R = g.R, row0 = (long long)blockIdx.x * RO_ROWS;
    auto image = [&](int i) { return tw_lds + (size_t)i * RO_ROWS * ld; };

    ro_load_rows(image(0), ld, ro_r16(g.K0), g.x, g.K0, row0, R, tid, [](long long row) { return row; });
    __syncthreads();
    tw_forward_layers(g, t, g.K0, image(0), ld, image(1), image(0), ld, tid, lane, wave, TowerSave{g, p, t, R, row0});
}

__global__ __launch_bounds__(256) void cdx_tower_bwd_kernel(const TowerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tw_lds[];
    const cdx_tower& g = a.g;
    const TowerPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.y, L = g.n_layers, ld = p.ld;
    const long long R = g.R, row0 = (long long)blockIdx.x * RO_ROWS;
    auto image = [&](int i) { return tw_lds + (size_t)i * RO_ROWS * ld; };

    const int WL = g.width[L - 1];
    ro_load_rows(image(0), ld, ro_r16(WL), g.g_out[t], WL, row0, R, tid, [](long long r) { return r; });
    __syncthreads();
    tw_backward_layers(g, t, g.K0, image(0), image(1), ld, tid, lane, wave, g.want_params != 0, g.want_gx != 0,
                       TowerSaved{g, p, t, R, row0}, TowerGrads{g, p, t, R, row0, (long long)gridDim.x, (long long)blockIdx.x});
}

// out[c] += sum_r src[r][c] for every job: 64 columns x 64 rows per workgroup, the body of cdx_colsum_f32 (cdx_train.hip)
constexpr int CSB_ROWS = 64;
__global__ __launch_bounds__(256) void cdx_colsum_batch_kernel(const cdx_colsum_batch B) {
    __shared__ float part[4][64];
    int j = 0;
    while (j + 1 < B.n_jobs && (int)blockIdx.x >= B.wg_start[j + 1]) ++j;
    const cdx_colsum_job q = B.job[j];
    const int local = (int)blockIdx.x - B.wg_start[j];
    const int col_tiles = (q.cols + 63) / 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = (local % col_tiles) * 64 + tx;
    const long long r0 = (long long)(local / col_tiles) * CSB_ROWS;
    const long long r1 = r0 + CSB_ROWS < q.rows ? r0 + CSB_ROWS : q.rows;
    float s = 0.f;
    if (c < q.cols)
        for (long long r = r0 + ty; r < r1; r += 4) s += q.src[r * q.ld + c];
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < q.cols) atomicAdd(q.out + c, (part[0][tx] + part[1][tx]) + (part[2][tx] + part[3][tx]));
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// sizes and the LDS plan: everything that can be checked without touching device memory
int tower_plan(const char* who, const cdx_tower* g, TowerPlan* p) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (!g) return fail("null request");
    if (g->R < 0 || g->R > 0x7fffffff - RO_ROWS) return fail("bad size: R");
    if (g->n_towers != 1 && g->n_towers != 2) return fail("n_towers must be 1 or 2");
    if (g->K0 <= 0 || g->K0 > RO_MAX_WIDTH) return fail("K0 must be 1 .. 512");
    int maxw = 0, cols = 0;
    const int rc = tw_check_layers(g->n_layers, g->width, g->norm, g->act, g->eps, &maxw, fail);
    if (rc != CDX_OK) return rc;
    maxw = ro_r16(g->K0) > maxw ? ro_r16(g->K0) : maxw;
    for (int l = 0; l < CDX_TOWER_MAX_LAYERS; ++l) {
        p->off_col[l] = l < g->n_layers ? cols : 0;
        cols += l < g->n_layers ? g->width[l] : 0;
    }
    p->ld = maxw + 4;
    p->total = 2 * RO_ROWS * p->ld;
    return CDX_OK;
}

int tower_check(const char* who, const cdx_tower* g, TowerPlan* p, bool backward) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    const int rc = tower_plan(who, g, p);
    if (rc != CDX_OK) return rc;
    if ((long long)p->total * (long long)sizeof(float) > TW_LDS_MAX) return fail("the LDS plan exceeds 160 KiB");
    if (g->R == 0) return CDX_OK;
    if (!g->x && !backward) return fail("null pointer: x");
    const bool saved = backward || g->save;
    for (int t = 0; t < g->n_towers; ++t) {
        for (int l = 0; l < g->n_layers; ++l) {
            if (!g->w[t][l] || (!backward && !g->b[t][l])) return fail("null pointer: weights");
            if (g->norm[l] && (!g->gamma[t][l] || !g->beta[t][l])) return fail("null pointer: norm parameters");
        }
        if (!backward && !g->out[t]) return fail("null pointer: out");
        if (saved && (!g->P[t] || !g->rstd[t])) return fail("null pointer: P / rstd");
        if (!backward && g->save && g->n_layers > 1 && !g->H[t]) return fail("null pointer: H");
        if (backward) {
            if (!g->g_out[t]) return fail("null pointer: g_out");
            if (g->want_params && (!g->G[t] || !g->Sb[t] || !g->Sg[t])) return fail("null pointer: G / Sb / Sg");
            if (g->want_gx && !g->g_x[t]) return fail("null pointer: g_x");
        }
    }
    return CDX_OK;
}

int tower_launch(const char* who, void (*kernel)(TowerArgs), const cdx_tower* g, void* hip_stream, bool backward, size_t& raised) {
    cdx_set_err("");
    TowerArgs a;
    const int rc = tower_check(who, g, &a.p, backward);
    if (rc != CDX_OK || g->R == 0) return rc;
    a.g = *g;
    return ro_launch_tiles(kernel, a, g->R, (size_t)a.p.total * sizeof(float), hip_stream, raised, (unsigned)g->n_towers);
}

}  // namespace

extern "C" {

long long cdx_tower_lds_bytes(const cdx_tower* g) {
    cdx_set_err("");
    TowerPlan p;
    const int rc = tower_plan("cdx_tower_lds_bytes", g, &p);
    return rc != CDX_OK ? rc : (long long)p.total * (long long)sizeof(float);
}

int cdx_tower_fwd_f32(const cdx_tower* g, void* hip_stream) {
    static size_t raised = 0;
    return tower_launch("cdx_tower_fwd_f32", cdx_tower_fwd_kernel, g, hip_stream, false, raised);
}

int cdx_tower_bwd_f32(const cdx_tower* g, void* hip_stream) {
    static size_t raised = 0;
    return tower_launch("cdx_tower_bwd_f32", cdx_tower_bwd_kernel, g, hip_stream, true, raised);
}

int cdx_colsum_batch_f32(const cdx_colsum_batch* B, void* hip_stream) {
    cdx_set_err("");
    auto fail = [](const char* what) { return ro_fail("cdx_colsum_batch_f32", what); };
    if (!B) return fail("null request");
    if (B->n_jobs < 0 || B->n_jobs > CDX_COLSUM_BATCH) return fail("n_jobs must be 0 .. CDX_COLSUM_BATCH");
    if (B->n_jobs == 0) return CDX_OK;
    if (B->wg_start[0] != 0) return fail("wg_start[0] must be 0");
    for (int j = 0; j < B->n_jobs; ++j) {
        const cdx_colsum_job& q = B->job[j];
        if (q.rows < 0 || q.cols <= 0 || q.ld < q.cols) return fail("bad shape");
        if (q.rows > 0 && (!q.src || !q.out)) return fail("null pointer");
        const long long wgs = (long long)((q.cols + 63) / 64) * ((q.rows + CSB_ROWS - 1) / CSB_ROWS);
        if ((long long)B->wg_start[j + 1] - B->wg_start[j] != wgs) return fail("wg_start does not match the jobs");
    }
    const int grid = B->wg_start[B->n_jobs];
    if (grid == 0) return CDX_OK;
    hipLaunchKernelGGL(cdx_colsum_batch_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), *B);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
    return CDX_OK;
}

}  // extern "C"
