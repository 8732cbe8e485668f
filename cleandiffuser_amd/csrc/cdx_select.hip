// cdx_select.hip -- score K candidates per state and pick among them.
//
// Every value-guided pipeline ends its sample() call with the same tail on the rows it just sampled (reference
// pipelines/idql_d4rl_mujoco.py:181-194, dql_d4rl_mujoco.py:192-200, sfbc_d4rl_mujoco.py:116-120 / 192-196, qgpo_d4rl_mujoco.py:141-144 /
// 190-194, veteran_d4rl_mujoco.py:440-446 / 474-478): the observation repeated K times and concatenated with the candidates, a critic
// (twin towers and their minimum), then softmax / multinomial / argmax / argsort and a gather -- 15 to 25 launches of a few microseconds.
//   cdx_score_select_kernel  one workgroup of 4 wave64 per 16-row tile of ONE state (grid S * ceil(K / 16)): the image [obs_s | cand_row]
//                            is built in LDS from the un-repeated observation, the towers run on it one after the other with the layer
//                            body of cdx_tower_layers.h, the minimum of their outputs goes to scores; with K <= 16 the tile is the whole
//                            state and the workgroup goes on to the reduction.
//   cdx_select_kernel        one wave64 per state over given scores: the reduction alone.
// The reduction (sel_reduce) is one device function for both.  It is run by the first wave of the workgroup: lane j owns k = j, j + 64,
// ..; sums are the lane's own in increasing k, then a fixed butterfly over the 64 lanes; the running sum of the sampling mode is taken
// serially in index order.  No atomics, no workgroup waits for another, every element is produced in one fixed order: bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cdx.h"
#include "cdx_rowtile.h"
#include "cdx_tower_layers.h"

namespace {

constexpr long long SEL_LDS_MAX = 160 * 1024;
constexpr int SEL_HEAD = 2 * RO_ROWS;             // floats in front of the images of cdx_score_select_kernel: scores and weights of the tile

// the LDS plan of cdx_score_select_kernel, in floats: [16] scores, [16] weights, the input image [16][ldx], two activation images [16][ld]
struct ScorePlan {
    int32_t ldx, ld, total;
};
struct ScoreArgs {
    cdx_score_select g;
    ScorePlan p;
};
static_assert(sizeof(ScoreArgs) <= 4096, "the kernel argument segment holds 4 KiB");

// butterflies over the 64 lanes of a wave: the same bits in every lane
__device__ __forceinline__ float sel_sum64(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float sel_max64(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// The reduction over the K scores of state s.  `sc` [K] (the scores) and `wk` [K] (scratch: the weights) are LDS; called by every
// thread of the workgroup behind a barrier that covers `sc`; threads 0 .. 63 (one whole wave) work.
__device__ __forceinline__ void sel_reduce(const cdx_select& q, long long s, const float* sc, float* wk, int tid) {
    const int K = q.K;
    const size_t base = (size_t)s * K;
    if (tid < 64) {
        const float T = q.temperature;
        float m = -INFINITY;
        for (int k = tid; k < K; k += 64) {
            const float x = T * sc[k];
            wk[k] = x;
            m = fmaxf(m, x);
        }
        m = sel_max64(m);
        float part = 0.f;
        for (int k = tid; k < K; k += 64) {
            const float e = expf(wk[k] - m);
            wk[k] = e;
            part += e;
        }
        const float total = sel_sum64(part);
        float pv = 0.f;
        for (int k = tid; k < K; k += 64) {
            const float w = wk[k] / total;
            wk[k] = w;
            pv += w * sc[k];
            if (q.weights) q.weights[base + k] = w;
        }
        pv = sel_sum64(pv);
        if (tid == 0 && q.value) q.value[s] = pv;
    }
    __syncthreads();                                  // (the running sum below reads other lanes' weights)
    if (tid >= 64 || q.mode == CDX_SELECT_NONE) return;

    const int P = q.picked ? q.P : 0;
    float acc = 0.f;                                  // lane c < P: column c of the picked row
    auto take = [&](int rank, int n, int k) {
        if (tid == 0 && q.index) q.index[(size_t)s * n + rank] = k;
        if (tid < P) acc += q.payload[(base + k) * (size_t)q.payload_ld + tid];
    };
    int n = 1;
    if (q.mode == CDX_SELECT_SAMPLE) {
        const float u = q.u[s];
        int pick = K - 1;
        float run = 0.f;
        for (int k = 0; k < K - 1; ++k) {             // (every lane the same walk: LDS broadcasts)
            run += wk[k];
            if (run > u) {
                pick = k;
                break;
            }
        }
        take(0, 1, pick);
    } else {
        n = q.mode == CDX_SELECT_TOPK_MEAN ? q.top_k : 1;
        uint32_t taken = 0;                           // bit i: this lane's k = tid + 64 i is taken (K <= 1024 = 64 x 16)
        for (int rank = 0; rank < n; ++rank) {
            float best = 0.f;
            int at = -1;
            for (int k = tid, i = 0; k < K; k += 64, ++i) {
                const float v = sc[k];
                if (!((taken >> i) & 1u) && (at < 0 || v > best)) {      // (increasing k: the first of equals stays)
                    best = v;
                    at = k;
                }
            }
#pragma unroll
            for (int msk = 32; msk >= 1; msk >>= 1) {
                const float ob = __shfl_xor(best, msk, 64);
                const int oa = __shfl_xor(at, msk, 64);
                if (oa >= 0 && (at < 0 || ob > best || (ob == best && oa < at))) {
                    best = ob;
                    at = oa;
                }
            }
            at = __shfl(at, 0, 64);                   // (one answer for the wave whatever a NaN did to the comparisons)
            if ((at & 63) == tid) taken |= 1u << (at >> 6);
            take(rank, n, at);
        }
    }
    if (tid < P) q.picked[(size_t)s * q.P + tid] = n > 1 ? acc / (float)n : acc;
}

__global__ __launch_bounds__(64) void cdx_select_kernel(const cdx_select q) {
    extern __shared__ __attribute__((aligned(16))) float sel_lds[];
    const int tid = threadIdx.x, K = q.K;
    const long long s = blockIdx.x;
    float* sc = sel_lds;
    float* wk = sel_lds + ((K + 3) & ~3);
    for (int k = tid; k < K; k += 64) sc[k] = q.scores[(size_t)s * K + k];
    __syncthreads();
    sel_reduce(q, s, sc, wk, tid);
}

__global__ __launch_bounds__(256) void cdx_score_select_kernel(const ScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sel_lds[];
    const cdx_score_select& g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = g.sel.K, O = g.O, A = g.A, K0 = O + A, ldx = a.p.ldx, ld = a.p.ld;
    const int tiles_per = (K + RO_ROWS - 1) / RO_ROWS;
    const long long s = blockIdx.x / tiles_per;
    const int k0 = (int)(blockIdx.x % tiles_per) * RO_ROWS;           // the tile is candidates [k0, k0 + 16) of state s
    const int n_live = K - k0 < RO_ROWS ? K - k0 : RO_ROWS;
    float* sc = sel_lds;
    float* wk = sel_lds + RO_ROWS;
    float* X = sel_lds + SEL_HEAD;
    float* img0 = X + (size_t)RO_ROWS * ldx;
    float* img1 = img0 + (size_t)RO_ROWS * ld;

    // the image [obs_s | cand_row | 0]: the observation once from global memory into row 0, then from there into the other live rows
    const int fill = ro_r16(K0);
    for (int c = tid; c < O; c += 256) X[c] = g.obs[(size_t)s * O + c];
    for (int i = tid; i < RO_ROWS * (fill - O); i += 256) {
        const int rr = i / (fill - O), c = i - rr * (fill - O);
        X[rr * ldx + O + c] = (c < A && rr < n_live) ? g.cand[((size_t)s * K + k0 + rr) * A + c] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < (RO_ROWS - 1) * O; i += 256) {
        const int rr = 1 + i / O, c = i - (rr - 1) * O;
        X[rr * ldx + c] = rr < n_live ? X[c] : 0.f;
    }
    __syncthreads();

    float* last = ((g.n_layers - 1) & 1) ? img1 : img0;               // column 0 of it: the tower's output
    for (int t = 0; t < g.n_towers; ++t) {
        tw_forward_layers(g, t, K0, X, ldx, img0, img1, ld, tid, lane, wave, TwKeepNothing{});
        if (tid < RO_ROWS) {
            const float v = last[tid * ld];
            const float m = sc[tid];
            sc[tid] = (t == 0 || v < m || v != v) ? v : m;             // torch.min: a NaN stays
        }
        __syncthreads();
    }
    if (tid < n_live) g.scores[(size_t)s * K + k0 + tid] = sc[tid];
    if (tiles_per == 1) sel_reduce(g.sel, s, sc, wk, tid);             // (uniform over the grid: K <= 16)
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the reduction's request; `fused`: as part of a cdx_score_select (scores come from the kernel itself)
int select_check(const char* who, const cdx_select* q, bool fused) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (q->S < 0) return fail("bad size: S");
    if (q->K < 1 || q->K > CDX_SELECT_MAX_K) return fail("K must be 1 .. 1024");
    if ((long long)q->S * q->K > 0x7fffffffLL - RO_ROWS) return fail("bad size: S * K must fit 31 bits");
    if (q->mode != CDX_SELECT_NONE && q->mode != CDX_SELECT_ARGMAX && q->mode != CDX_SELECT_SAMPLE && q->mode != CDX_SELECT_TOPK_MEAN)
        return fail("mode must be none, argmax, sample or topk_mean");
    if (!isfinite(q->temperature)) return fail("temperature must be finite");
    if (q->mode == CDX_SELECT_TOPK_MEAN && (q->top_k < 1 || q->top_k > CDX_SELECT_MAX_TOPK || q->top_k > q->K))
        return fail("top_k must be 1 .. min(K, 16)");
    if (q->mode == CDX_SELECT_NONE && (q->index || q->picked)) return fail("index and picked need a mode other than none");
    if (q->picked) {
        if (q->P < 1 || q->P > RO_MAX_X) return fail("P must be 1 .. 64");
        if (q->payload_ld < q->P) return fail("payload_ld must be at least P");
    }
    if (q->S == 0) return CDX_OK;
    if (q->picked && !q->payload) return fail("null pointer: payload");
    if (q->mode == CDX_SELECT_SAMPLE && !q->u) return fail("null pointer: u (sample mode draws from the caller's uniforms)");
    if (!fused && !q->scores) return fail("null pointer: scores");
    return CDX_OK;
}

// sizes and the LDS plan: everything that can be checked without touching device memory
int score_plan(const char* who, const cdx_score_select* g, ScorePlan* p) {
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    if (!g) return fail("null request");
    if (g->n_towers != 1 && g->n_towers != 2) return fail("n_towers must be 1 or 2");
    if (g->O < 0) return fail("bad size: O");
    if (g->A < 1 || g->A > RO_MAX_X) return fail("A must be 1 .. 64");
    if (g->O + g->A > RO_MAX_WIDTH) return fail("O + A must be at most 512");
    int maxw = 0;
    const int rc = tw_check_layers(g->n_layers, g->width, g->norm, g->act, g->eps, &maxw, fail);
    if (rc != CDX_OK) return rc;
    if (g->width[g->n_layers - 1] != 1) return fail("the last width must be 1: a critic gives one score per row");
    p->ldx = ro_r16(g->O + g->A) + 4;
    p->ld = maxw + 4;
    p->total = SEL_HEAD + RO_ROWS * p->ldx + 2 * RO_ROWS * p->ld;
    return CDX_OK;
}

}  // namespace

extern "C" {

int cdx_select_f32(const cdx_select* q, void* hip_stream) {
    cdx_set_err("");
    if (!q) return ro_fail("cdx_select_f32", "null request");
    const int rc = select_check("cdx_select_f32", q, false);
    if (rc != CDX_OK || q->S == 0) return rc;
    const size_t lds = 2 * (size_t)((q->K + 3) & ~3) * sizeof(float);
    hipLaunchKernelGGL(cdx_select_kernel, dim3((unsigned)q->S), dim3(64), lds, reinterpret_cast<hipStream_t>(hip_stream), *q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
    return CDX_OK;
}

long long cdx_score_select_lds_bytes(const cdx_score_select* g) {
    cdx_set_err("");
    ScorePlan p;
    const int rc = score_plan("cdx_score_select_lds_bytes", g, &p);
    return rc != CDX_OK ? rc : (long long)p.total * (long long)sizeof(float);
}

int cdx_score_select_f32(const cdx_score_select* g, void* hip_stream) {
    static size_t raised = 0;
    const char* who = "cdx_score_select_f32";
    auto fail = [&](const char* what) { return ro_fail(who, what); };
    cdx_set_err("");
    ScoreArgs a;
    int rc = score_plan(who, g, &a.p);
    if (rc != CDX_OK) return rc;
    if ((long long)a.p.total * (long long)sizeof(float) > SEL_LDS_MAX) return fail("the LDS plan exceeds 160 KiB");
    rc = select_check(who, &g->sel, true);
    if (rc != CDX_OK || g->sel.S == 0) return rc;
    a.g = *g;                                          // (K > 16: the kernel writes scores only, `sel`'s outputs wait for cdx_select_f32)
    if ((g->O > 0) != (g->obs != nullptr)) return fail("obs must be given exactly when O > 0");
    if (!g->cand || !g->scores) return fail("null pointer: cand / scores");
    for (int t = 0; t < g->n_towers; ++t)
        for (int l = 0; l < g->n_layers; ++l) {
            if (!g->w[t][l] || !g->b[t][l]) return fail("null pointer: weights");
            if (g->norm[l] && (!g->gamma[t][l] || !g->beta[t][l])) return fail("null pointer: norm parameters");
        }
    const long long tiles = (long long)g->sel.S * ((g->sel.K + RO_ROWS - 1) / RO_ROWS);
    if (tiles > 0x7fffffffLL) return fail("bad size: too many tiles");
    return ro_launch_tiles(cdx_score_select_kernel, a, tiles * RO_ROWS, (size_t)a.p.total * sizeof(float), hip_stream, raised);
}

}  // extern "C"
