// cdx_hcritic.hip -- Decision Veteran's horizon critic (reference utils/building_blocks.py:149-229) as one executor call on gfx950.
//
// The critic is a small transformer over the tokens of a plan whose output is final_layer(h)[:, 0]: only token 0 of the last block is
// read.  The pipelines score num_envs x candidates plans per environment step (2500 x 40 tokens, 7500 x 32), so M = batch x tokens is
// large and every Linear is a plain GEMM: the host sequences cdx_gemm_f32 / cdx_layernorm_f32 / cdx_attention_f32 launches
// (csrc/cdx_gemm.hip) on the caller's stream, as cdx_dit1d_run does, and prunes the last block to what token 0 needs -- keys and
// values of all tokens, then one row per trajectory.  The one kernel of its own is the single-query attention in between.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cdx.h"

extern void cdx_set_err(const char* msg);

namespace {

// ------------------------------------------------------------------------------------------------
// Single-query attention: core0[b][h*dh + j] = sum_t softmax_t(scale * q0[b][h] . k[b][t][h]) v[b][t][h][j]
// ------------------------------------------------------------------------------------------------
// One wave64 per (trajectory, head), `blockDim.x / 64` pairs per workgroup.  kv: (chunk * T, 2d) = [k | v] rows as in_proj[d:3d] writes
// them.  The pair's T x dh key and value tiles are a streaming read (2 d T floats per trajectory over the heads): they come in with
// 16-byte loads, consecutive lanes on consecutive 16 bytes of a row, into the wave's own LDS slice -- keys with an odd row stride (lane
// t then walks row t conflict-free), values densely (lane j walks column j).  Lane t < T forms its score; lanes >= T hold p = 0 and
// never enter a sum; lane j < dh accumulates p_t v[t][j] in ascending t.  No atomics, one fixed lane and order per element.
struct SqAttnArgs {
    const float* q0;     // (chunk, d)
    const float* kv;     // (chunk * T, 2d)
    float* core0;        // (chunk, d)
    int chunk, T, n_heads, dh, vec, wave_floats;
    float scale;
};

__host__ __device__ inline int sq_r4(int n) { return (n + 3) & ~3; }
// LDS floats of one wave: values (T, dh) | query (dh) | keys (T, dh + 1), every part starting on 16 bytes
__host__ __device__ inline int sq_wave_floats(int T, int dh) { return sq_r4(T * dh) + sq_r4(dh) + sq_r4(T * (dh + 1)); }

__global__ __launch_bounds__(256) void cdx_sqattn_kernel(const SqAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sq_smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const long long pair = (long long)blockIdx.x * waves + wave;
    const bool live = pair < (long long)a.chunk * a.n_heads;
    const int T = a.T, dh = a.dh, d = a.n_heads * dh, ldk = dh + 1;
    float* vs = sq_smem + (size_t)wave * a.wave_floats;
    float* qs = vs + sq_r4(T * dh);
    float* ks = qs + sq_r4(dh);
    const int b = live ? (int)(pair / a.n_heads) : 0, h = live ? (int)(pair % a.n_heads) : 0;
    const float* kbase = a.kv + (size_t)b * T * 2 * d + (size_t)h * dh;        // key row t at + t * 2d, its value row d further
    if (live) {
        if (a.vec) {
            const int dh4 = dh >> 2, per_row = 2 * dh4;
            for (int e = lane; e < T * per_row; e += 64) {
                const int t = e / per_row, r = e - t * per_row;
                const int half = r >= dh4 ? 1 : 0, c = (r - half * dh4) * 4;
                const float4 x = *reinterpret_cast<const float4*>(kbase + (size_t)t * 2 * d + (size_t)half * d + c);
                if (half) {
                    *reinterpret_cast<float4*>(vs + t * dh + c) = x;
                } else {
                    float* p = ks + t * ldk + c;
                    p[0] = x.x; p[1] = x.y; p[2] = x.z; p[3] = x.w;
                }
            }
        } else {
            const int per_row = 2 * dh;
            for (int e = lane; e < T * per_row; e += 64) {
                const int t = e / per_row, r = e - t * per_row;
                const int half = r >= dh ? 1 : 0, c = r - half * dh;
                const float x = kbase[(size_t)t * 2 * d + (size_t)half * d + c];
                if (half) vs[t * dh + c] = x; else ks[t * ldk + c] = x;
            }
        }
        if (lane < dh) qs[lane] = a.q0[(size_t)b * d + (size_t)h * dh + lane];
    }
    __syncthreads();                       // (the only barrier: every wave reaches it, live or not)
    if (!live) return;
    float s = -3.0e38f;
    if (lane < T) {
        const float* kr = ks + lane * ldk;
        float acc = 0.f;
        for (int c = 0; c < dh; ++c) acc += qs[c] * kr[c];
        s = a.scale * acc;
    }
    float m = s;
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const float p = lane < T ? expf(s - m) : 0.f;
    float sum = p;
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {
        const float pt = __shfl(p, t, 64);
        if (lane < dh) acc += pt * vs[t * dh + lane];
    }
    if (lane < dh) a.core0[(size_t)b * d + (size_t)h * dh + lane] = acc / sum;
}

int sq_attention(hipStream_t st, const float* q0, const float* kv, float* core0, int chunk, int T, int n_heads, int dh) {
    SqAttnArgs a;
    a.q0 = q0; a.kv = kv; a.core0 = core0; a.chunk = chunk; a.T = T; a.n_heads = n_heads; a.dh = dh;
    a.vec = (dh % 4 == 0 && ((uintptr_t)kv % 16) == 0) ? 1 : 0;
    a.wave_floats = sq_wave_floats(T, dh);
    a.scale = 1.0f / sqrtf((float)dh);
    // pairs per workgroup: four, or as many as keep the workgroup's LDS within 48 KiB (T = dh = 64: 33 KiB per wave)
    int waves = 4;
    while (waves > 1 && (size_t)waves * a.wave_floats * sizeof(float) > 48u * 1024u) waves >>= 1;
    const long long pairs = (long long)chunk * n_heads;
    const long long grid = (pairs + waves - 1) / waves;
    if (grid <= 0) return CDX_OK;
    if (grid > 0x7fffffffLL) { cdx_set_err("cdx_hcritic_run: chunk too large for one launch"); return CDX_EINVAL; }
    hipLaunchKernelGGL(cdx_sqattn_kernel, dim3((unsigned)grid), dim3(64 * waves), (size_t)waves * a.wave_floats * sizeof(float), st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cdx_set_err(hipGetErrorString(e)); return CDX_EHIP; }
    return CDX_OK;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#define CDX_TRY(expr)            \
    do {                         \
        const int rc_ = (expr);  \
        if (rc_ != CDX_OK) return rc_; \
    } while (0)

int gemm(void* stream, const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N, int K,
         int act = CDX_ACT_NONE, const float* residual = nullptr, int ldr = 0, const float* table = nullptr, int table_rows = 0) {
    cdx_gemm_args g;
    g.A = A; g.W = W; g.bias = bias; g.gate = nullptr; g.residual = residual; g.table = table; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.ldg = 0; g.ldr = ldr;
    g.rows_per_gate = 1; g.table_rows = table_rows; g.act = act;
    g.conv_taps = g.conv_cin = g.conv_lin = g.conv_lout = g.conv_stride = g.conv_pad = 0;
    g.partial = nullptr; g.partial_slices = 0;
    return cdx_gemm_f32(&g, stream);
}

int layernorm(void* stream, const float* x, int ldx, float* y, int M, int C, float eps) {      // no gain / shift
    cdx_ln_args a;
    a.x = x; a.y = y; a.gamma = a.beta = a.scale = a.shift = nullptr;
    a.M = M; a.C = C; a.ldx = ldx; a.ldy = C; a.ldmod = 0; a.rows_per_mod = 1; a.eps = eps; a.x_rows = 0;
    return cdx_layernorm_f32(&a, stream);
}

// One pass of nb trajectories, R = nb * T rows.  Blocks in 256-byte steps: every buffer stays float4-loadable.
struct HcBuffers {
    float *h, *u, *qkv, *att, *a, *v, *f, *o;        // (R, .): the full blocks; the last block's [k | v] rows live in qkv
    float *q0, *core0, *a0, *v0, *f0, *o0, *hf;      // (nb, .): the last block behind its attention
};

long long hc_layout(const cdx_hcritic_weights* w, long long nb, float* base, HcBuffers* B) {
    const long long d = w->d_model, R = nb * w->tokens;
    long long used = 0;
    auto take = [&](long long n) {
        float* p = base ? base + used : nullptr;
        used += (n + 63) & ~63LL;
        return p;
    };
    HcBuffers b;
    b.h = take(R * d);
    b.u = take(R * d);
    b.qkv = take(R * 3 * d);
    b.att = b.a = b.v = b.f = b.o = nullptr;
    if (w->depth > 1) {
        b.att = take(R * d);
        b.a = take(R * d);
        b.v = take(R * d);
        b.f = take(R * 4 * d);
        b.o = take(R * d);
    }
    b.q0 = take(nb * d);
    b.core0 = take(nb * d);
    b.a0 = take(nb * d);
    b.v0 = take(nb * d);
    b.f0 = take(nb * 4 * d);
    b.o0 = take(nb * d);
    b.hf = take(nb * d);
    if (B) *B = b;
    return used;
}

// Trajectories per pass when the caller leaves it to the library: the GEMMs are compute bound, so tall passes win until the widest
// activation (rows x 4 d floats) outgrows the Infinity Cache by much -- the rule the DiT1d executor measured (engine/bigbatch.py);
// profiles/hcritic_ab.txt has the sweep at the shipped shapes.
long long hc_default_chunk(const cdx_hcritic_weights* w) {
    long long rows = (320LL << 20) / (16LL * w->d_model);
    if (rows < 2048) rows = 2048;
    const long long c = rows / w->tokens;
    return c < 1 ? 1 : c;
}

int hc_check(const cdx_hcritic_weights* w, int batch, int chunk, long long* nb_out) {
    if (!w) { cdx_set_err("cdx_hcritic: null weights"); return CDX_EINVAL; }
    if (w->tokens < 1 || w->tokens > 64) { cdx_set_err("cdx_hcritic: 1 <= tokens <= 64 required"); return CDX_EINVAL; }
    if (w->d_model < 1 || w->d_model > 1024 || w->n_heads < 1 || w->d_model % w->n_heads != 0 || w->d_model / w->n_heads > 64) {
        cdx_set_err("cdx_hcritic: d_model <= 1024, d_model % n_heads == 0 and head dimension <= 64 required"); return CDX_EINVAL;
    }
    if (w->depth < 1) { cdx_set_err("cdx_hcritic: depth >= 1 required"); return CDX_EINVAL; }
    if (w->in_dim < 1) { cdx_set_err("cdx_hcritic: in_dim >= 1 required"); return CDX_EINVAL; }
    if (!(w->eps > 0.f)) { cdx_set_err("cdx_hcritic: eps > 0 required"); return CDX_EINVAL; }
    if (batch < 0 || chunk < 0) { cdx_set_err("cdx_hcritic: batch and chunk must not be negative"); return CDX_EINVAL; }
    long long nb = chunk > 0 ? chunk : hc_default_chunk(w);
    if (nb > batch) nb = batch;
    if (nb * w->tokens * 4 * w->d_model > 0x7fffffffLL) {
        cdx_set_err("cdx_hcritic: chunk too large (chunk * tokens * 4 * d_model must stay below 2^31)"); return CDX_EINVAL;
    }
    *nb_out = nb;
    return CDX_OK;
}

int hc_pass(const cdx_hcritic_weights* w, hipStream_t st, const HcBuffers& B, const float* x, float* out, int nb) {
    const int T = w->tokens, d = w->d_model, R = nb * T, pre = w->pre_norm != 0;
    const float eps = w->eps;
    CDX_TRY(gemm(st, x, w->in_dim, w->x_proj_w, w->in_dim, w->x_proj_b, B.h, d, R, d, w->in_dim, CDX_ACT_NONE, nullptr, 0, w->pos, T));
    const float* h = B.h;
    // The two norm orders are one sequence: `pre` decides whether a LayerNorm stands in front of the attention or behind the MLP, and
    // whether the MLP's residual is the attention's sum `a` or its normalised copy `v`.
    for (int i = 0; i + 1 < w->depth; ++i) {
        const cdx_hcritic_block& k = w->blocks[i];
        const float* u = h;
        if (pre) { CDX_TRY(layernorm(st, h, d, B.u, R, d, eps)); u = B.u; }
        CDX_TRY(gemm(st, u, d, k.qkv_w, d, k.qkv_b, B.qkv, 3 * d, R, 3 * d, d));
        cdx_attn_args at;
        at.qkv = B.qkv; at.out = B.att; at.B = nb; at.T = T; at.n_heads = w->n_heads; at.head_dim = d / w->n_heads;
        at.scale = 1.0f / sqrtf((float)at.head_dim); at.mask = nullptr;
        CDX_TRY(cdx_attention_f32(&at, st));
        CDX_TRY(gemm(st, B.att, d, k.proj_w, d, k.proj_b, B.a, d, R, d, d, CDX_ACT_NONE, u, d));
        CDX_TRY(layernorm(st, B.a, d, B.v, R, d, eps));
        CDX_TRY(gemm(st, B.v, d, k.fc1_w, d, k.fc1_b, B.f, 4 * d, R, 4 * d, d, CDX_ACT_GELU_TANH));
        CDX_TRY(gemm(st, B.f, 4 * d, k.fc2_w, 4 * d, k.fc2_b, B.o, d, R, d, 4 * d, CDX_ACT_NONE, pre ? B.a : B.v, d));
        if (pre) {
            h = B.o;
        } else {
            CDX_TRY(layernorm(st, B.o, d, B.h, R, d, eps));
            h = B.h;
        }
    }
    // the last block: keys and values of every token, everything else for token 0 (row b * T of the stream: leading dimension T * d)
    const cdx_hcritic_block& k = w->blocks[w->depth - 1];
    const float* u = h;
    if (pre) { CDX_TRY(layernorm(st, h, d, B.u, R, d, eps)); u = B.u; }
    CDX_TRY(gemm(st, u, d, k.qkv_w + (size_t)d * d, d, k.qkv_b + d, B.qkv, 2 * d, R, 2 * d, d));
    CDX_TRY(gemm(st, u, T * d, k.qkv_w, d, k.qkv_b, B.q0, d, nb, d, d));
    CDX_TRY(sq_attention(st, B.q0, B.qkv, B.core0, nb, T, w->n_heads, d / w->n_heads));
    CDX_TRY(gemm(st, B.core0, d, k.proj_w, d, k.proj_b, B.a0, d, nb, d, d, CDX_ACT_NONE, u, T * d));
    CDX_TRY(layernorm(st, B.a0, d, B.v0, nb, d, eps));
    CDX_TRY(gemm(st, B.v0, d, k.fc1_w, d, k.fc1_b, B.f0, 4 * d, nb, 4 * d, d, CDX_ACT_GELU_TANH));
    CDX_TRY(gemm(st, B.f0, 4 * d, k.fc2_w, 4 * d, k.fc2_b, B.o0, d, nb, d, 4 * d, CDX_ACT_NONE, pre ? B.a0 : B.v0, d));
    const float* hf = B.o0;
    if (!pre) { CDX_TRY(layernorm(st, B.o0, d, B.hf, nb, d, eps)); hf = B.hf; }
    return gemm(st, hf, d, w->fin_w, d, w->fin_b, out, 1, nb, 1, d);
}

}  // namespace

extern "C" {

long long cdx_hcritic_workspace_floats(const cdx_hcritic_weights* w, int32_t batch, int32_t chunk) {
    long long nb = 0;
    const int rc = hc_check(w, batch, chunk, &nb);
    if (rc != CDX_OK) return rc;
    return hc_layout(w, nb, nullptr, nullptr);
}

int cdx_hcritic_run(const cdx_hcritic_weights* w, const float* x, float* out, int32_t batch, int32_t chunk, float* workspace,
                    long long workspace_floats, void* hip_stream) {
    long long nb = 0;
    CDX_TRY(hc_check(w, batch, chunk, &nb));
    if (batch == 0) return CDX_OK;
    if (!x || !out || !workspace || !w->blocks || !w->x_proj_w || !w->x_proj_b || !w->pos || !w->fin_w || !w->fin_b) {
        cdx_set_err("cdx_hcritic_run: null pointer"); return CDX_EINVAL;
    }
    for (int i = 0; i < w->depth; ++i) {
        const cdx_hcritic_block& k = w->blocks[i];
        if (!k.qkv_w || !k.qkv_b || !k.proj_w || !k.proj_b || !k.fc1_w || !k.fc1_b || !k.fc2_w || !k.fc2_b) {
            cdx_set_err("cdx_hcritic_run: null pointer in a block"); return CDX_EINVAL;
        }
    }
    HcBuffers B;
    if (hc_layout(w, nb, workspace, &B) > workspace_floats) { cdx_set_err("cdx_hcritic_run: workspace too small"); return CDX_EINVAL; }
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const size_t per = (size_t)w->tokens * w->in_dim;
    for (long long b0 = 0; b0 < batch; b0 += nb) {
        const int n = (int)(batch - b0 < nb ? batch - b0 : nb);
        CDX_TRY(hc_pass(w, st, B, x + (size_t)b0 * per, out + b0, n));
    }
    return CDX_OK;
}

}  // extern "C"
