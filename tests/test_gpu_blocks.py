"""GPU unit tests of the big-batch building blocks (cdx_gemm_f32 / cdx_layernorm_f32 / cdx_attention_f32) against the
plain PyTorch fp32 ops they replace -- evaluated on the CPU in fp64 as the reference, so the bar is fp32 round-off."""
import pytest
import torch
import torch.nn.functional as F

from block_variants import GUARDED
from gpu_profile import kernel_names, missing, profiled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = "failed with code -1"        # (CDX_EINVAL through runtime._check)


def _ref(t):
    return t.detach().cpu().double()


_guard_open = []                      # the coverage guard at the end of the file is profiling a whole family (profilers do not nest)


def _launched(body):
    """body() under the profiler -> (names of the device kernels it launched, its result).  Names None inside the coverage guard and
    when the tracer delivered nothing: the numerical check of the result never depends on the profiler, only the guard may skip."""
    from torch.profiler import ProfilerActivity
    if _guard_open:
        return None, body()
    prof, out = profiled(body, activities=[ProfilerActivity.CUDA], skip=False)
    return (None if prof is None else kernel_names(prof)), out


def _expect_kernels(names, want):
    assert names is None or not missing(names, want), f"expected {want} among the launches: {sorted(n for n in names if 'cdx_' in n or 'gm_' in n)}"


# The instantiations gm_launch picks (block_variants.GUARDED["gemm"]): unguarded 64 x 64, 8-wave 128 x 128 and guarded 128 x 128 tiles
S64, W8, G128 = "cdx_gemm_kernel<true,1,false,4>", "cdx_gemm_kernel<true,2,false,8>", "cdx_gemm_kernel<false,2,false,4>"
W8_CONV, G128_CONV = "cdx_gemm_kernel<true,2,true,8>", "cdx_gemm_kernel<false,2,true,4>"


@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (7, 29, 320), (300, 320, 29), (1024, 960, 320), (130, 129, 17),
                                   (4096, 1280, 320), (513, 320, 1280)])
def test_gemm_matches_linear(m, n, k):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(m * 7 + n)
    a, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g)
    out = blocks.linear(a.to(DEV), w.to(DEV), b.to(DEV))
    ref = F.linear(_ref(a), _ref(w), _ref(b))
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)


def test_gemm_asymmetric_identity_catches_transposes():
    from cleandiffuser_amd.engine import blocks
    a = torch.eye(160)
    w = torch.arange(96 * 160, dtype=torch.float32).reshape(96, 160) * 1e-3
    out = blocks.linear(a.to(DEV), w.to(DEV))
    torch.testing.assert_close(out.cpu(), w.t().contiguous(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("act", ["none", "mish", "gelu", "gelu_tanh", "silu", "leaky", "relu", "tanh"])
def test_gemm_fused_epilogue(act):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(3)
    B, T, K, N = 5, 16, 64, 96
    a, w, b = torch.randn(B * T, K, generator=g), torch.randn(N, K, generator=g) / 8, torch.randn(N, generator=g)
    gate, res, tab = torch.randn(B, N, generator=g), torch.randn(B * T, N, generator=g), torch.randn(T, N, generator=g)
    out = blocks.linear(a.to(DEV), w.to(DEV), b.to(DEV), act=act, gate=gate.to(DEV), rows_per_gate=T,
                        residual=res.to(DEV), table=tab.to(DEV))
    y = F.linear(_ref(a), _ref(w), _ref(b))
    fn = {"none": lambda v: v, "mish": F.mish, "gelu": F.gelu, "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"),
          "silu": F.silu, "leaky": lambda v: F.leaky_relu(v, 0.01), "relu": F.relu, "tanh": torch.tanh}[act]
    ref = fn(y) * _ref(gate).repeat_interleave(T, 0) + _ref(res) + _ref(tab).repeat(B, 1)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)


def test_gemm_strided_views_and_empty():
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(4)
    big = torch.randn(40, 96, generator=g).to(DEV)
    a = big[:, 32:64]                                   # row stride 96, 32 columns
    w = torch.randn(24, 32, generator=g).to(DEV)
    out = blocks.linear(a, w)
    torch.testing.assert_close(out.cpu().double(), F.linear(_ref(a), _ref(w)), rtol=2e-5, atol=2e-5)
    assert blocks.linear(torch.zeros(0, 32, device=DEV), w).shape == (0, 24)


@pytest.mark.parametrize("c", [64, 320, 1024, 100,                       # the float4 kernels <4>, <8>, <16>, <4>
                               30, 1023, 1500, 4096, 2050])              # the scalar kernels <16>, <16>, <32>, <64>, <64>
def test_layernorm_modulate(c):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(c)
    B, T = 3, 8
    x = torch.randn(B * T, c, generator=g) * 3 + 1
    sc, sh = torch.randn(B, c, generator=g), torch.randn(B, c, generator=g)
    y = blocks.layernorm(x.to(DEV), scale=sc.to(DEV), shift=sh.to(DEV), rows_per_mod=T, eps=1e-6)
    ref = F.layer_norm(_ref(x), (c,), eps=1e-6) * (1 + _ref(sc).repeat_interleave(T, 0)) + _ref(sh).repeat_interleave(T, 0)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=2e-5, atol=2e-5)
    ga, be = torch.randn(c, generator=g), torch.randn(c, generator=g)
    y2 = blocks.layernorm(x.to(DEV), gamma=ga.to(DEV), beta=be.to(DEV), eps=1e-5)
    torch.testing.assert_close(y2.cpu().double(), F.layer_norm(_ref(x), (c,), _ref(ga), _ref(be), 1e-5), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("tokens,heads,dh", [(64, 10, 32), (16, 4, 16), (5, 2, 64), (1, 1, 8), (64, 3, 64), (33, 5, 20), (7, 3, 6),
                                             (65, 2, 32), (96, 4, 32), (200, 3, 64), (128, 2, 6)])     # > 64: streamed-key kernel
def test_attention_matches_mha_core(tokens, heads, dh):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(tokens)
    B, dm = 3, heads * dh
    torch.full((1 << 22,), float("nan"), device=DEV)     # whatever stale memory the kernel might touch is poisoned first
    qkv = torch.randn(B * tokens, 3 * dm, generator=g) * 2
    out = blocks.attention(qkv.to(DEV), B, tokens, heads)
    q, k, v = (_ref(qkv).reshape(B, tokens, 3, heads, dh)[:, :, i].transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * tokens, dm)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("tokens,heads,dh", [(16, 4, 64), (64, 2, 32), (12, 4, 16), (9, 3, 6), (100, 2, 32)])
def test_attention_with_additive_mask(tokens, heads, dh):
    """Causal mask built the way nn.Transformer builds it (0 / -inf, clamped to the fp32 floor by the binding)."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(tokens + dh)
    B, dm = 3, heads * dh
    qkv = torch.randn(B * tokens, 3 * dm, generator=g) * 2
    allowed = torch.tril(torch.ones(tokens, tokens)) == 1
    mask = torch.zeros(tokens, tokens).masked_fill(~allowed, float("-inf"))
    out = blocks.attention(qkv.to(DEV), B, tokens, heads, mask=mask.clamp_min(torch.finfo(torch.float32).min).to(DEV))
    q, k, v = (_ref(qkv).reshape(B, tokens, 3, heads, dh)[:, :, i].transpose(1, 2) for i in range(3))
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask.double()).transpose(1, 2).reshape(B * tokens, dm)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)


def _linear_attention_ref(qkv, B, L, heads, dh, scale):
    """The core of LinearAttention.forward (nn_diffusion/jannerunet.py) in float64: q * scale, softmax of k over the positions,
    ctx = k v^T, out = ctx^T q.  Rows are positions, columns [q | k | v] x (head, channel)."""
    q, k, v = (_ref(qkv).reshape(B, L, 3, heads, dh)[:, :, i].permute(0, 2, 3, 1) for i in range(3))        # (B, heads, dh, L)
    ctx = torch.einsum("b h d n, b h e n -> b h d e", k.softmax(dim=-1), v)
    out = torch.einsum("b h d e, b h d n -> b h e n", ctx, q * scale)
    return out.permute(0, 3, 1, 2).reshape(B * L, heads * dh)


# one position / one channel; odd sizes; the shipped shape; 64 KiB of LDS (past the 48 KiB a kernel gets without the attribute); 124 KiB;
# L > 256: each softmax thread walks a long column and the staging loops take several trips
@pytest.mark.parametrize("B,L,heads,dh", [(3, 1, 1, 1), (2, 7, 3, 6), (2, 32, 4, 32), (1, 64, 2, 64), (1, 144, 1, 64), (5, 300, 2, 8)])
def test_linear_attention_matches_float64(B, L, heads, dh):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(L * 7 + dh)
    torch.full((1 << 22,), float("nan"), device=DEV)     # whatever stale memory the kernel might touch is poisoned first
    qkv = torch.randn(B * L, 3 * heads * dh, generator=g) * 2
    out = blocks.linear_attention(qkv.to(DEV), B, L, heads, dh)
    assert out.shape == (B * L, heads * dh)
    torch.testing.assert_close(out.cpu().double(), _linear_attention_ref(qkv, B, L, heads, dh, dh ** -0.5), rtol=2e-5, atol=2e-5)
    scaled = blocks.linear_attention(qkv.to(DEV), B, L, heads, dh, scale=0.37, out=torch.full_like(out, float("nan")))
    torch.testing.assert_close(scaled.cpu().double(), _linear_attention_ref(qkv, B, L, heads, dh, 0.37), rtol=2e-5, atol=2e-5)


def test_linear_attention_softmax_is_shifted():
    """k entries of +-80: exp(80) overflows fp32, so a softmax that does not subtract the column maximum gives inf / inf."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(80)
    B, L, heads, dh = 2, 33, 2, 16
    inner = heads * dh
    torch.full((1 << 22,), float("nan"), device=DEV)
    qkv = torch.randn(B * L, 3 * inner, generator=g)
    qkv[:, inner:2 * inner] = 80.0 * torch.sign(torch.randn(B * L, inner, generator=g))
    out = blocks.linear_attention(qkv.to(DEV), B, L, heads, dh)
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.cpu().double(), _linear_attention_ref(qkv, B, L, heads, dh, dh ** -0.5), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("B,L,heads,dh,code", [(1, 1025, 1, 8, EINVAL), (1, 8, 1, 65, EINVAL), (1, 1024, 1, 64, "failed with code -2")])
def test_linear_attention_refuses(B, L, heads, dh, code):
    """L > 1024 and dim_head > 64 are CDX_EINVAL; q, k, v of one head past 160 KiB of LDS is CDX_ELDS.  Nothing is launched."""
    from cleandiffuser_amd.engine import blocks
    qkv = torch.zeros(B * L, 3 * heads * dh, device=DEV)
    out = torch.full((B * L, heads * dh), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=code):
        blocks.linear_attention(qkv, B, L, heads, dh, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_linear_attention_empty_batch():
    from cleandiffuser_amd.engine import blocks
    out = blocks.linear_attention(torch.empty(0, 3 * 2 * 8, device=DEV), 0, 5, 2, 8)
    torch.cuda.synchronize()
    assert out.shape == (0, 16)


@pytest.mark.parametrize("tokens,n_obs,heads,dh,per_sample", [(16, 2, 4, 64, False), (12, 3, 4, 16, True), (5, 0, 2, 8, False),
                                                              (16, 15, 2, 4, False), (7, 2, 3, 6, True), (3, 1, 1, 256, False),
                                                              (33, 4, 5, 128, True), (1, 0, 7, 32, False)])
def test_cross_attention_against_short_memory(tokens, n_obs, heads, dh, per_sample):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(tokens * 3 + n_obs)
    B, dm, S = 4, heads * dh, 1 + n_obs
    q = torch.randn(B * tokens, dm, generator=g)
    kv_shared = torch.randn(B if per_sample else 3, 2 * dm, generator=g)
    kv_rows = torch.randn(max(B * n_obs, 1), 2 * dm, generator=g)
    t_idx, s_idx = torch.meshgrid(torch.arange(tokens), torch.arange(S), indexing="ij")
    mask = torch.zeros(tokens, S).masked_fill(~(t_idx >= (s_idx - 1)), float("-inf"))
    out = blocks.cross_attention(q.to(DEV), kv_shared.to(DEV), kv_rows.to(DEV) if n_obs else None, B, tokens, n_obs, heads,
                                 shared_row=2, shared_per_sample=per_sample,
                                 mask=mask.clamp_min(torch.finfo(torch.float32).min).to(DEV))
    shared = _ref(kv_shared)[torch.arange(B)] if per_sample else _ref(kv_shared)[2].expand(B, -1)
    mem = torch.cat([shared[:, None], _ref(kv_rows)[:B * n_obs].reshape(B, n_obs, 2 * dm)], 1)       # (B, S, 2dm)
    k = mem[..., :dm].reshape(B, S, heads, dh).transpose(1, 2)
    v = mem[..., dm:].reshape(B, S, heads, dh).transpose(1, 2)
    qq = _ref(q).reshape(B, tokens, heads, dh).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qq, k, v, attn_mask=mask.double()).transpose(1, 2).reshape(B * tokens, dm)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("cin,cout,k,stride,pad,L", [(32, 64, 5, 1, 2, 16), (256, 256, 3, 2, 1, 8), (2, 48, 5, 1, 2, 16),
                                                     (23, 32, 5, 1, 2, 32), (64, 23, 1, 1, 0, 4), (48, 40, 3, 1, 1, 1),
                                                     # K = 48: the 128 x 128 tile, 8-wave (c_in % 4 == 0) and guarded (c_in = 6)
                                                     (16, 40, 3, 1, 1, 16), (6, 40, 8, 1, 3, 16)])
def test_implicit_gemm_conv1d(cin, cout, k, stride, pad, L):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(cin + cout)
    B = 5
    x = torch.randn(B, cin, L, generator=g)
    conv = torch.nn.Conv1d(cin, cout, k, stride, pad)
    rows = x.permute(0, 2, 1).reshape(B * L, cin).contiguous().to(DEV)
    out = blocks.conv1d(rows, blocks.pack_conv(conv.weight).to(DEV), conv.bias.detach().to(DEV), B, L, stride, pad)
    ref = conv.double()(x.double()).permute(0, 2, 1).reshape(-1, cout)
    torch.testing.assert_close(out.cpu().double(), ref.detach(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("c,L", [(64, 4), (32, 16), (20, 3)])
def test_implicit_gemm_conv_transpose(c, L):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(c)
    B = 3
    x = torch.randn(B, c, L, generator=g)
    up = torch.nn.ConvTranspose1d(c, c, 4, 2, 1)
    rows = x.permute(0, 2, 1).reshape(B * L, c).contiguous().to(DEV)
    packed = tuple(t.to(DEV) for t in blocks.pack_conv_transpose_k4s2p1(up.weight))
    out = blocks.conv_transpose1d_k4s2p1(rows, packed, up.bias.detach().to(DEV), B, L)
    ref = up.double()(x.double()).permute(0, 2, 1).reshape(-1, c)
    torch.testing.assert_close(out.cpu().double(), ref.detach(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("c,groups,L,film", [(256, 8, 16, 1), (1024, 8, 4, 1), (32, 8, 32, 2), (48, 4, 5, 0), (4096, 2, 16, 1),
                                             # groups of 5 and 6 channels: the scalar kernel, every FiLM mode
                                             (20, 4, 7, 0), (20, 4, 7, 2), (48, 8, 6, 1), (48, 8, 6, 2)])
def test_groupnorm_mish_film_residual(c, groups, L, film):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(c + L)
    B = 3
    x = torch.randn(B, c, L, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    width = {0: c, 1: 2 * c, 2: c}[film]
    fa, fb = torch.randn(4, width, generator=g), torch.randn(B, width, generator=g)
    res = torch.randn(B * L, c, generator=g)
    rows = x.permute(0, 2, 1).reshape(B * L, c).contiguous()
    out = blocks.groupnorm(rows.to(DEV), gamma.to(DEV), beta.to(DEV), B, L, groups, act="mish", fa=fa.to(DEV) if film else None,
                           fb=fb.to(DEV) if film else None, fa_row=2, film_mode=film, residual=res.to(DEV))
    y = F.mish(F.group_norm(_ref(x), groups, _ref(gamma), _ref(beta), 1e-5))                       # (B, C, L)
    f = _ref(fa)[2][None] + _ref(fb)
    if film == 1:
        y = f[:, :c, None] * y + f[:, c:, None]
    elif film == 2:
        y = y + f[:, :, None]
    ref = y.permute(0, 2, 1).reshape(B * L, c) + _ref(res)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=3e-5, atol=3e-5)


@pytest.mark.parametrize("m,n,k,slices", [(256, 256, 4096, 6), (300, 130, 2048, 4), (128, 64, 512, 8)])
def test_gemm_split_k_is_exact_and_deterministic(m, n, k, slices):
    """Few tiles + long K: the library splits K over `slices` partial buffers and reduces them in slice order."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(k)
    a, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    part = torch.full((slices * m * n,), float("nan"), device=DEV)
    kw = dict(act="mish", residual=res.to(DEV), partial=part)
    o1 = blocks.linear(a.to(DEV), w.to(DEV), b.to(DEV), **kw)
    o2 = blocks.linear(a.to(DEV), w.to(DEV), b.to(DEV), **kw)
    assert torch.equal(o1, o2)
    ref = F.mish(F.linear(_ref(a), _ref(w), _ref(b))) + _ref(res)
    torch.testing.assert_close(o1.cpu().double(), ref, rtol=2e-5, atol=2e-5)


# ----------------------------------------------------------------------------------------------------------------------------- #
# One case per kernel variant the launchers pick.  The shapes above were chosen for their edges; the ones below for the branch of
# gm_launch / cdx_gemm_f32 they land on, which each case NAMES and checks among the kernels its call launched -- a re-tuned threshold
# that moves a case to another variant fails here instead of silently thinning the coverage.
# ----------------------------------------------------------------------------------------------------------------------------- #
def _gemm_inputs(m, n, k, lda=None, period=16, table_rows=16, seed=0):
    g = torch.Generator().manual_seed(seed + m * 7 + n)
    a = torch.randn(m, lda or k, generator=g)[:, :k]
    w, b = torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g)
    gate, res, tab = torch.randn(-(-m // period), n, generator=g), torch.randn(m, n, generator=g), torch.randn(table_rows, n, generator=g)
    return a, w, b, gate, res, tab


def _epilogue_ref(y, gate, period, res, tab):
    """mish(y) * gate[row // period] + res + tab[row % len(tab)] in float64, in place (the big cases hold 5e7 elements)."""
    rows = torch.arange(y.shape[0])
    y = F.mish(y)
    if gate is not None:
        y *= _ref(gate)[rows // period]
    y += _ref(res)
    if tab is not None:
        y += _ref(tab)[rows % tab.shape[0]]
    return y


GEMM_MATRIX = [
    # (m, n, k, options, kernels of the bias-only call, kernels of the full-epilogue call)
    pytest.param(7, 29, 48, dict(period=3, table_rows=4), [W8], [W8], id="k48-one-big-tile-slow-epilogue"),
    pytest.param(7, 32, 48, dict(lda=49, period=3, table_rows=4), [G128], [G128], id="lda49-guarded-big-tile"),
    pytest.param(4096, 1024, 29, dict(), [G128], [G128], id="k29-guarded-big-tile-256-tiles"),
    # without a table N = 1028 meets the split-N rule: 1024 columns on the 8-wave kernel, a 4-column remainder on the 64 x 64 one
    pytest.param(4100, 1028, 320, dict(period=41, table_rows=100), [W8, S64], [W8], id="ragged-297-tiles-fast-epilogue"),
    pytest.param(4100, 1027, 320, dict(period=41, table_rows=100), [W8], [W8], id="ragged-297-tiles-slow-epilogue"),
    pytest.param(2048, 1664, 512, dict(slices=6), [W8, "gm_splitk_reduce_kernel<true>"], [W8, "gm_splitk_reduce_kernel<true>"],
                 id="split-k-3-on-the-big-tile"),
    pytest.param(2048, 1662, 512, dict(slices=6), [W8, "gm_splitk_reduce_kernel<false>"], [W8, "gm_splitk_reduce_kernel<false>"],
                 id="split-k-3-on-the-big-tile-scalar-reduce"),
    pytest.param(16384, 320, 1280, dict(table=False), [W8, S64], [W8, S64], id="split-n-256-plus-64-columns"),
    pytest.param(163840, 320, 64, dict(period=10, table_rows=10), [W8, S64], [W8], id="divmod-163840-rows-period-10"),
    pytest.param(163840, 322, 64, dict(period=10, table_rows=10), [W8], [W8], id="divmod-163840-rows-period-10-slow-epilogue"),
    pytest.param(80, 98, 64, dict(), [S64], [S64], id="small-tile-slow-epilogue-all-terms"),
]


@pytest.mark.parametrize("epilogue", ["bias", "full"])
@pytest.mark.parametrize("m,n,k,opt,kernels_bias,kernels_full", GEMM_MATRIX)
def test_gemm_variant_matrix(m, n, k, opt, kernels_bias, kernels_full, epilogue):
    """Every row (a) with a bias only and (b) with act = mish, gate, residual and table (split-N excludes the table) against float64."""
    from cleandiffuser_amd.engine import blocks
    period = opt.get("period", 16)
    a, w, b, gate, res, tab = _gemm_inputs(m, n, k, opt.get("lda"), period, opt.get("table_rows", 16))
    if not opt.get("table", True):
        tab = None
    kw = {}
    if "slices" in opt:
        kw["partial"] = torch.full((opt["slices"] * m * n,), float("nan"), device=DEV)
    if epilogue == "full":
        kw.update(act="mish", gate=gate.to(DEV), rows_per_gate=period, residual=res.to(DEV), table=None if tab is None else tab.to(DEV))
    ad = torch.randn(m, opt["lda"], device=DEV)[:, :k].copy_(a) if "lda" in opt else a.to(DEV)
    assert ad.stride(0) == (opt.get("lda") or k)
    wd, bd = w.to(DEV), b.to(DEV)
    names, out = _launched(lambda: blocks.linear(ad, wd, bd, **kw))
    ref = F.linear(_ref(a), _ref(w), _ref(b))
    if epilogue == "full":
        ref = _epilogue_ref(ref, gate, period, res, tab)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)
    _expect_kernels(names, kernels_full if epilogue == "full" else kernels_bias)


@pytest.mark.parametrize("epilogue", ["bias", "mish+residual"])
@pytest.mark.parametrize("B,cin,cout,k,stride,pad,L,kernel", [
    (5, 16, 40, 3, 1, 1, 16, W8_CONV),                  # K = 48: one 8-wave tile, conv edges inside it
    (5, 6, 40, 8, 1, 3, 16, G128_CONV),                 # c_in % 4 != 0 on the big tile
    (512, 64, 256, 3, 1, 1, 32, W8_CONV),               # config-3-like: M = 16384, 256 tiles
    (1024, 64, 256, 3, 2, 1, 32, W8_CONV),              # ... and its stride-2 downsample
    (1024, 23, 96, 5, 1, 2, 32, G128_CONV),             # config 2's first layer (c_in = 23) at the guarded big tile, 256 tiles
])
def test_implicit_gemm_conv1d_variant_matrix(B, cin, cout, k, stride, pad, L, kernel, epilogue):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(cin + cout + B)
    x = torch.randn(B, cin, L, generator=g)
    conv = torch.nn.Conv1d(cin, cout, k, stride, pad)
    l_out = (L + 2 * pad - k) // stride + 1
    res = torch.randn(B * l_out, cout, generator=g)
    rows = x.permute(0, 2, 1).reshape(B * L, cin).contiguous().to(DEV)
    wp, bias = blocks.pack_conv(conv.weight).to(DEV), conv.bias.detach().to(DEV)
    kw = dict(residual=res.to(DEV), act="mish") if epilogue != "bias" else {}
    names, out = _launched(lambda: blocks.conv1d(rows, wp, bias, B, L, stride, pad, **kw))
    ref = conv.double()(x.double()).permute(0, 2, 1).reshape(-1, cout).detach()
    if epilogue != "bias":
        ref = F.mish(ref) + _ref(res)
    torch.testing.assert_close(out.cpu().double(), ref, rtol=2e-5, atol=2e-5)
    _expect_kernels(names, [kernel])


@pytest.mark.parametrize("m,c,width,off,kernel", [(37, 320, 400, 32, "cdx_layernorm_vec_kernel<8>"),      # 16-byte aligned block: float4
                                                  (37, 320, 400, 33, "cdx_layernorm_kernel<16>"),         # odd first column: scalar
                                                  (21, 1500, 1600, 3, "cdx_layernorm_kernel<32>")])
def test_layernorm_on_a_column_block(m, c, width, off, kernel):
    """x (and y) as a column block of a wider matrix: ldx != C; the launcher picks the float4 kernel from the POINTERS too."""
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(c + off)
    T = 1 if m % 2 else 2
    wide = (torch.randn(m, width, generator=g) * 3 + 1).to(DEV)
    x = wide[:, off:off + c]
    sc, sh = torch.randn(m // T, c, generator=g), torch.randn(m // T, c, generator=g)
    out_wide = torch.full((m, width), 7.0, device=DEV)
    scd, shd = sc.to(DEV), sh.to(DEV)
    names, y = _launched(lambda: blocks.layernorm(x, out=out_wide[:, off:off + c], scale=scd, shift=shd, rows_per_mod=T, eps=1e-6))
    ref = F.layer_norm(_ref(x), (c,), eps=1e-6) * (1 + _ref(sc).repeat_interleave(T, 0)) + _ref(sh).repeat_interleave(T, 0)
    torch.testing.assert_close(y.cpu().double(), ref, rtol=2e-5, atol=2e-5)
    assert float(out_wide[:, :off].min()) == 7.0 and float(out_wide[:, off + c:].max()) == 7.0        # nothing outside the block
    _expect_kernels(names, [kernel])


@pytest.mark.parametrize("c,groups,L,film,off,kernel", [(20, 4, 7, 0, None, "cdx_groupnorm_kernel"),             # groups of 5 channels
                                                        (48, 8, 6, 2, 3, "cdx_groupnorm_kernel"),                # 6 channels, odd first column
                                                        (64, 8, 8, 0, 1, "cdx_groupnorm_kernel"),                # float4 shape, unaligned base
                                                        (64, 8, 8, 1, 32, "cdx_groupnorm_vec_kernel<false>")])   # aligned block: float4, ldx != C
def test_groupnorm_without_activation_on_strided_input(c, groups, L, film, off, kernel):
    from cleandiffuser_amd.engine import blocks
    g = torch.Generator().manual_seed(c + L + film)
    B = 3
    x = torch.randn(B, c, L, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    width = {0: c, 1: 2 * c, 2: c}[film]
    fa, fb = torch.randn(4, width, generator=g), torch.randn(B, width, generator=g)
    rows = x.permute(0, 2, 1).reshape(B * L, c)
    xd = rows.contiguous().to(DEV)
    if off is not None:
        wide = torch.randn(B * L, c + 72, generator=g).to(DEV)
        wide[:, off:off + c] = xd
        xd = wide[:, off:off + c]
    args = (gamma.to(DEV), beta.to(DEV), B, L, groups)
    kw = dict(act="none", fa=fa.to(DEV) if film else None, fb=fb.to(DEV) if film else None, fa_row=1, film_mode=film,
              out=torch.empty(B * L, c, device=DEV))
    names, out = _launched(lambda: blocks.groupnorm(xd, *args, **kw))
    y = F.group_norm(_ref(x), groups, _ref(gamma), _ref(beta), 1e-5)
    f = _ref(fa)[1][None] + _ref(fb)
    if film == 1:
        y = f[:, :c, None] * y + f[:, c:, None]
    elif film == 2:
        y = y + f[:, :, None]
    torch.testing.assert_close(out.cpu().double(), y.permute(0, 2, 1).reshape(B * L, c), rtol=3e-5, atol=3e-5)
    _expect_kernels(names, [kernel])


# ----------------------------------------------------------------------------------------------------------------------------- #
# Activations: cdx_act_f32 / cdx_act_bwd_f32 and the same formulas inside the GEMM epilogue, over the whole range a pre-activation
# can take -- the softplus threshold at 20, the range where exp() overflows fp32 (|x| > 88.7) or underflows (x < -103.9), +-0
# ----------------------------------------------------------------------------------------------------------------------------- #
def _act_sweep():
    t20 = torch.tensor(20.0)
    inf = torch.tensor(float("inf"))
    special = [0.0, -0.0, 20.0, float(torch.nextafter(t20, inf)), float(torch.nextafter(t20, -inf)), 88.0, -88.0, 89.0, -89.0, -103.9,
               1e-30, -1e-30, 1e4, -1e4]
    return torch.cat([torch.linspace(-110, 110, 4097), torch.tensor(special)]).float()


ACT_REF = {"none": lambda v: v, "mish": F.mish, "gelu": F.gelu, "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"), "silu": F.silu,
           "leaky": lambda v: F.leaky_relu(v, 0.01), "relu": F.relu, "tanh": torch.tanh}


def _act_ref(act, x64, param=1.0):
    """(act(x), d act / dx) in float64; "mish_grad" IS the derivative of Mish; tanh with a scale: param * tanh(x / param)."""
    x = x64.clone().requires_grad_(True)
    fn = F.mish if act == "mish_grad" else ((lambda v: param * torch.tanh(v / param)) if act == "tanh" else ACT_REF[act])
    y = fn(x)
    (dy,) = torch.autograd.grad(y.sum(), x)
    return (dy, None) if act == "mish_grad" else (y.detach(), dy)


def test_activation_names_are_all_covered():
    from cleandiffuser_amd.engine import blocks
    assert set(blocks.ACT) == set(ACT_REF) | {"mish_grad"}


@pytest.mark.parametrize("act", ["none", "mish", "gelu", "gelu_tanh", "silu", "leaky", "relu", "tanh", "mish_grad"])
def test_activation_and_its_derivative_over_the_whole_range(act):
    from cleandiffuser_amd.engine import blocks
    x = _act_sweep()
    y = blocks.activation(x.to(DEV), act).cpu().double()
    ref, dref = _act_ref(act, x.double())
    assert ref.isfinite().all() and y.isfinite().all()
    torch.testing.assert_close(y, ref, rtol=2e-5, atol=2e-5)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    if act == "mish_grad":                                   # no second derivative in the library: the documented refusal
        with pytest.raises(RuntimeError, match=EINVAL):
            blocks.activation_backward(x.to(DEV), g.to(DEV), act)
        return
    for param in ((1.0, 10.0) if act == "tanh" else (1.0,)):
        d = blocks.activation_backward(x.to(DEV), g.to(DEV), act, param).cpu().double()
        dref = _act_ref(act, x.double(), param)[1] * g.double()
        assert dref.isfinite().all() and d.isfinite().all()
        torch.testing.assert_close(d, dref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("k,kernel", [(32, S64), (48, W8)])
@pytest.mark.parametrize("act", ["none", "mish", "gelu", "gelu_tanh", "silu", "leaky", "relu", "tanh"])
def test_gemm_epilogue_activation_over_the_whole_range(act, k, kernel):
    """The sweep as EXACT pre-activations of the GEMM epilogue: A is zero except one column holding it, W zero except a 1 there."""
    from cleandiffuser_amd.engine import blocks
    x = _act_sweep()
    a, w = torch.zeros(x.numel(), k), torch.zeros(48, k)
    a[:, 5] = x
    w[:, 5] = 1.0
    ad, wd = a.to(DEV), w.to(DEV)
    names, out = _launched(lambda: blocks.linear(ad, wd, act=act))
    ref = _act_ref(act, x.double())[0]
    assert out.isfinite().all()
    torch.testing.assert_close(out.cpu().double(), ref[:, None].expand(-1, 48), rtol=2e-5, atol=2e-5)
    _expect_kernels(names, [kernel])


# ----------------------------------------------------------------------------------------------------------------------------- #
# The coverage guard: every instantiation a launcher can pick by default (block_variants.GUARDED; the CPU tier keeps that table equal
# to the launch sites in the sources) is reached by the unit tests of its family.
# ----------------------------------------------------------------------------------------------------------------------------- #
def _cases(fn):
    """Every parameter set of a (parametrised) test function, as keyword dictionaries."""
    sets = [{}]
    for mark in getattr(fn, "pytestmark", []):
        if mark.name == "parametrize":
            names = [n.strip() for n in mark.args[0].split(",")]
            values = [v.values if hasattr(v, "values") else (v if len(names) > 1 else (v,)) for v in mark.args[1]]
            sets = [dict(s, **dict(zip(names, v))) for s in sets for v in values]
    return sets


def _family_tests(family):
    import test_gpu_parity as parity
    here = globals()
    return {
        "gemm": [here[n] for n in ("test_gemm_matches_linear", "test_gemm_fused_epilogue", "test_gemm_strided_views_and_empty",
                                   "test_implicit_gemm_conv1d", "test_implicit_gemm_conv_transpose", "test_gemm_variant_matrix",
                                   "test_implicit_gemm_conv1d_variant_matrix")],
        "splitk_reduce": [test_gemm_split_k_is_exact_and_deterministic],
        "layernorm": [test_layernorm_modulate, test_layernorm_on_a_column_block],
        "layernorm_bwd": [parity.test_layernorm_and_attention_backward_kernels_match_autograd,
                          parity.test_layernorm_backward_against_float64_on_column_blocks],
        "groupnorm": [test_groupnorm_mish_film_residual, test_groupnorm_without_activation_on_strided_input],
        "groupnorm_bwd": [parity.test_groupnorm_backward_adds_its_gain_and_shift_sums_onto_the_callers_buffers,
                          parity.test_groupnorm_backward_in_registers_and_its_position_sums,
                          parity.test_groupnorm_backward_of_a_group_width_that_is_no_power_of_two],
        "attention": [test_attention_matches_mha_core, test_attention_with_additive_mask],
        "cross_attention": [test_cross_attention_against_short_memory],
    }[family]


@pytest.mark.parametrize("family", list(GUARDED))
def test_unit_cases_reach_every_kernel_variant(family):
    from torch.profiler import ProfilerActivity

    def body():
        for fn in _family_tests(family):
            for kw in _cases(fn):
                fn(**kw)
    _guard_open.append(family)
    try:
        prof, _ = profiled(body, activities=[ProfilerActivity.CUDA])
    finally:
        _guard_open.pop()
    names = kernel_names(prof)
    lost = missing(names, GUARDED[family])
    assert not lost, f"{family}: no unit-test case reaches {lost}; launched: {sorted(n for n in names if 'cdx_' in n or 'gm_' in n)}"
