"""TEST HELPER for the host paths of the four GEMM executors in csrc/cdx_bigbatch.hip -- ``cdx_dit1d_run`` (DiT1d, DiT1Ref),
``cdx_chitf_run`` (ChiTransformer), ``cdx_pearcetf_run`` (PearceTransformer), ``cdx_resmlp_run`` (IDQLMlp, NewIDQLMlp): a table of the
smallest shapes at which each piece of their arena layout, leading dimensions, row periods and chunk offsets can go wrong, and for
each case ONE float64 CPU run -- the reference tests/test_gpu_executor_shapes.py compares the device with.

A case is a net (class, constructor arguments), a state and a condition shape, a batch, a chunk override (None: the default rule) and
a mode:

* ``forward``: ``net(x, t, cond)`` with a timestep per sample -- ``bigbatch.forward``, one ``_run`` request with n_steps == 0.  The
  reference is the stock module on the CPU in float64.  The time embedding stays the fp32 one the host evaluates for the device: a
  positional embedding is evaluated on the fp32 timesteps and handed on as float64 (the hooks of ``solver_step_cases.build``); a
  Fourier embedding has weights, so the float64 net evaluates it on the same timesteps as float64 -- continuous ones in (0, 1), where
  the fp32 angles cost under 1e-6 (at integer timesteps up to 1000 they cost the fp32 module alone 1e-4 and more).
* ``sample``: ``agent.sample`` of a DiscreteDiffusionSDE with a two-step ddim plan on a recorded x_T, w_cfg = 1.3: the classifier-free
  pair, cfg_mode 2.  The reference is the package's own host loop in float64, built and run by ``solver_step_cases``.  The nets predict
  x0, so the finished sample is the combined prediction of the last step at full scale.

Weights are ``load_synth`` streams, inputs seeded draws.  "chunked" is batch 5 in chunks of 2: chunks of 2, 2 and 1 samples, so `b0` is
non-zero and the last chunk of a pair holds one trajectory.

The table (`+` marks a case added to the list the sweep was asked for, with the reason):

DiT1d (in_dim, d_model / n_heads, tokens, depth)
  dit_d30          (3, 30/2, 5, 2) chunked, conditional   head_dim 15; every adaLN offset but the first is unaligned
  dit_t1           (1, 36/3, 1, 2) conditional            one token, in_dim 1
  dit_t65          (5, 64/1, 65, 1) Fourier, chunked      head_dim 64; the first token count past the one-tile attention
  dit_d130_uncond  (7, 130/5, 17, 2) no condition         cfg_mode 0
  dit_depth0_pair  (3, 32/2, 4, 0) sample, chunked        the final LayerNorm's h_rows != rows broadcast
  dit_d30_pair     the dit_d30 net, sample, chunked       the first block's broadcast with unaligned offsets
DiT1Ref (state rows [reference | noisy])
  ditref_fwd       (3, 32/2, 6, 2) chunked                the cross variant
  ditref_pair      the same net, sample, chunked          the `rep` loop with cb / nb = 2 from the second block on; copy_ref_cols_kernel
ChiTransformer (act_dim, obs_dim, Ta, To, d_model / nhead, num_layers)
  chitf_d30        (3, 7, 3, 1, 30/2, 2) chunked          unaligned width, head_dim 15
  chitf_limits     (2, 5, 64, 15, 32/4, 1) batch 3        both token limits
  chitf_ta1        (3, 7, 1, 2, 32/2, 1)                  one action token
  chitf_dh64       (2, 5, 17, 2, 128/2, 1)                head_dim 64
  chitf_enc2_fwd   (3, 5, 7, 3, 36/3, 2, n_cond_layers=2) chunked    per-sample shared K / V in forward
  chitf_enc2_pair  the same net, sample, chunked          the memory built per step
  chitf_pair       the chitf_d30 net, sample, chunked     obs_rows_kernel's unconditional half; shared_row = rec
PearceTransformer (act_dim, To, emb_dim, trans_emb_dim, nhead)
  ptf_to1          (5, 1, 16, 12, 3)                      three tokens, the fewest the net has
  ptf_te64         (3, 7, 20, 64, 2)                      trans_emb_dim (= head_dim) at its limit
  ptf_s64          (2, 62, 16, 8, 1) batch 3              64 tokens, the limit
+ ptf_te15         (3, 2, 16, 15, 2) chunked              no listed case has an odd head_dim or te * nhead % 4 != 0, and none is a
                                                          chunked forward (the `b0` offset into the per-sample time rows)
  ptf_pair         the ptf_to1 net (output layer x 0.25), sample, chunked    the zero-condition half of ptf_tokens_kernel
residual MLP
  mlp_h33          IDQLMlp obs 7, act 5, emb 16, hidden 33, 3 blocks, chunked
  mlp_new_h130     NewIDQLMlp obs 3, act 1, emb 16, hidden 130, 2 blocks
  mlp_nb0          IDQLMlp obs 0, act 4, emb 16, hidden 20, no blocks, no condition (the class constructs it)
  mlp_h33_pair     the mlp_h33 net, sample, chunked

Refusals, one past a limit each: ``bigbatch._binding`` answers None and the stock module serves the request.
  refuse_dit_dh65     DiT1d 130/2: head_dim 65.  (Not d_model 65 with one head: DiT1d's own SinusoidalEmbedding gives 2 * (d_model // 2)
                      columns, so the class cannot run an odd d_model at all.)
  refuse_chitf_ta65   ChiTransformer Ta = 65
  refuse_chitf_to16   ChiTransformer To = 16
  refuse_ptf_te65     PearceTransformer trans_emb_dim = 65
  refuse_ptf_to63     PearceTransformer To = 63
"""
import functools
from types import SimpleNamespace

import torch

import solver_step_cases as S

B, CHUNK = 5, 2             # "chunked": chunks of 2, 2 and 1
W_CFG = 1.3                 # the classifier-free weight of the sample-mode cases
EMB = 16                    # emb_dim of every net that has one

# ------------------------------------------------------------------------------------------------ #
# the table                                                                                            #
# ------------------------------------------------------------------------------------------------ #
_KIND = {"DiT1d": "dit", "DiT1Ref": "dit", "ChiTransformer": "chitf", "PearceTransformer": "pearcetf", "IDQLMlp": "mlp",
         "NewIDQLMlp": "mlp"}


def _k(cls, ctor, x_shape, cond_shape, mode="forward", batch=B, chunk=None, refused=False):
    return SimpleNamespace(family=_KIND[cls], cls=cls, ctor=dict(ctor), x_shape=tuple(x_shape),
                           cond_shape=None if cond_shape is None else tuple(cond_shape), mode=mode, batch=batch, chunk=chunk,
                           refused=refused, den_scale=1.0)


def _dit(in_dim, d_model, n_heads, tokens, depth, cond=True, cls="DiT1d", emb="positional", **kw):
    ctor = dict(in_dim=in_dim, emb_dim=EMB, d_model=d_model, n_heads=n_heads, depth=depth, timestep_emb_type=emb)
    return _k(cls, ctor, (tokens, in_dim * (2 if cls == "DiT1Ref" else 1)), (EMB,) if cond else None, **kw)


def _chitf(act_dim, obs_dim, Ta, To, d_model, nhead, num_layers, n_cond_layers=0, **kw):
    ctor = dict(act_dim=act_dim, obs_dim=obs_dim, Ta=Ta, To=To, d_model=d_model, nhead=nhead, num_layers=num_layers,
                n_cond_layers=n_cond_layers)
    return _k("ChiTransformer", ctor, (Ta, act_dim), (To, obs_dim), **kw)


def _ptf(act_dim, To, emb_dim, te, nhead, **kw):
    return _k("PearceTransformer", dict(act_dim=act_dim, To=To, emb_dim=emb_dim, trans_emb_dim=te, nhead=nhead), (act_dim,),
              (To, emb_dim), **kw)


def _mlp(cls, obs_dim, act_dim, hidden_dim, n_blocks, **kw):
    return _k(cls, dict(obs_dim=obs_dim, act_dim=act_dim, emb_dim=EMB, hidden_dim=hidden_dim, n_blocks=n_blocks), (act_dim,),
              (obs_dim,) if obs_dim else None, **kw)


def _pair(case, den_scale=1.0):
    """The same net under the classifier-free pair, in chunks of 2; `den_scale` scales its output layer (``solver_step_cases.build``)."""
    return SimpleNamespace(**{**vars(case), "mode": "sample", "batch": B, "chunk": CHUNK, "den_scale": den_scale})


def _table():
    t = {}
    t["dit_d30"] = _dit(3, 30, 2, 5, 2, chunk=CHUNK)
    t["dit_t1"] = _dit(1, 36, 3, 1, 2)
    t["dit_t65"] = _dit(5, 64, 1, 65, 1, emb="fourier", chunk=CHUNK)
    t["dit_d130_uncond"] = _dit(7, 130, 5, 17, 2, cond=False)
    t["dit_depth0_pair"] = _pair(_dit(3, 32, 2, 4, 0))
    t["dit_d30_pair"] = _pair(t["dit_d30"])
    t["ditref_fwd"] = _dit(3, 32, 2, 6, 2, cls="DiT1Ref", chunk=CHUNK)
    t["ditref_pair"] = _pair(t["ditref_fwd"])
    t["chitf_d30"] = _chitf(3, 7, 3, 1, 30, 2, 2, chunk=CHUNK)
    t["chitf_limits"] = _chitf(2, 5, 64, 15, 32, 4, 1, batch=3)
    t["chitf_ta1"] = _chitf(3, 7, 1, 2, 32, 2, 1)
    t["chitf_dh64"] = _chitf(2, 5, 17, 2, 128, 2, 1)
    t["chitf_enc2_fwd"] = _chitf(3, 5, 7, 3, 36, 3, 2, n_cond_layers=2, chunk=CHUNK)
    t["chitf_enc2_pair"] = _pair(t["chitf_enc2_fwd"])
    t["chitf_pair"] = _pair(t["chitf_d30"])
    t["ptf_to1"] = _ptf(5, 1, 16, 12, 3)
    t["ptf_te64"] = _ptf(3, 7, 20, 64, 2)
    t["ptf_s64"] = _ptf(2, 62, 16, 8, 1, batch=3)
    t["ptf_te15"] = _ptf(3, 2, 16, 15, 2, chunk=CHUNK)
    # (at full scale this net's x0 is ~8 for a state of ~1 and the second step amplifies the first one's rounding: the fp32 host loop
    #  alone is 3.5e-5 from float64, ten times every other case)
    t["ptf_pair"] = _pair(t["ptf_to1"], den_scale=0.25)
    t["mlp_h33"] = _mlp("IDQLMlp", 7, 5, 33, 3, chunk=CHUNK)
    t["mlp_new_h130"] = _mlp("NewIDQLMlp", 3, 1, 130, 2)
    t["mlp_nb0"] = _mlp("IDQLMlp", 0, 4, 20, 0)
    t["mlp_h33_pair"] = _pair(t["mlp_h33"])
    t["refuse_dit_dh65"] = _dit(3, 130, 2, 5, 1, batch=3, refused=True)
    t["refuse_chitf_ta65"] = _chitf(2, 5, 65, 2, 32, 2, 1, batch=3, refused=True)
    t["refuse_chitf_to16"] = _chitf(2, 5, 4, 16, 32, 2, 1, batch=3, refused=True)
    t["refuse_ptf_te65"] = _ptf(3, 2, 16, 65, 1, batch=3, refused=True)
    t["refuse_ptf_to63"] = _ptf(2, 63, 16, 8, 1, batch=3, refused=True)
    return t


CASES = _table()
TABLE = sorted(CASES)
SERVED = [n for n in TABLE if not CASES[n].refused]
REFUSALS = [n for n in TABLE if CASES[n].refused]
FAMILIES = ("dit", "chitf", "pearcetf", "mlp")

# YARDSTICK[family]: the largest E32 over the family's cases (the refusals included), E32 = max |x32 - x64| / max(1, max |x64|) of the fp32
# CPU run -- the stock module (forward) or the host loop (sample) -- against the float64 one on the same inputs, as
# tests/test_executor_shape_cases_cpu.py measures it (its docstring has the figures), rounded up.  The GPU tolerance is 4 x this.  One
# constant per family: the residual MLP's is less than half the transformers', and the largest must not cover all.
YARDSTICK = {"dit": 3e-6, "chitf": 3.5e-6, "pearcetf": 2.5e-6, "mlp": 1.5e-6}


def tolerance(name):
    return 4.0 * YARDSTICK[CASES[name].family]


# ------------------------------------------------------------------------------------------------ #
# what a case reaches: read off the bound weight struct and bigbatch's own chunk rule                  #
# ------------------------------------------------------------------------------------------------ #
# every family: a width the float4 variants cannot take; the fewest tokens the net can have (1; PearceTransformer's 2 + To >= 3); the token
# limit (the first count past the one-tile attention for DiT); head_dim 64 and an odd one; a chunk that does not divide the batch; a pair
# whose last chunk holds one trajectory.  The residual MLP has no tokens and no heads.
_COMMON = {"unaligned_width", "fewest_tokens", "token_limit", "head_dim_64", "odd_head_dim", "uneven_chunks", "pair_last_chunk_of_one"}
REQUIRED = {"dit": _COMMON | {"depth0_pair", "no_condition", "cross"},
            "chitf": _COMMON | {"encoder_forward", "encoder_pair"},
            "pearcetf": _COMMON,
            "mlp": {"unaligned_width", "uneven_chunks", "pair_last_chunk_of_one", "no_blocks", "head_mish"}}


def spec_of(name):
    """The net of a case as ``solver_step_cases.build`` takes it."""
    c = CASES[name]
    return SimpleNamespace(net=(c.cls, c.ctor), x_shape=c.x_shape, cond_shape=c.cond_shape, kind=c.family, needs_cond=False)


_PLAN = S._c("DiscreteDiffusionSDE", dict(diffusion_steps=20, predict_noise=False),
             dict(solver="ddim", sample_steps=2, sample_step_schedule="uniform"))


def solver_case(name, w_cfg=W_CFG):
    """The two-step deterministic plan over the net of `name`, as a case of ``solver_step_cases``."""
    return SimpleNamespace(**{**vars(_PLAN), "x_shape": CASES[name].x_shape, "w_cfg": w_cfg, "den_scale": CASES[name].den_scale})


def build_net(name, device="cpu", dtype=torch.float32):
    """The net of a case in eval mode: ``solver_step_cases.build`` (its weights, its dtype hooks) under the plan's solver class."""
    return S.build(None, None, device, dtype, case=solver_case(name), spec=spec_of(name)).model_ema["diffusion"]


def binding(name):
    """-> (family of the net, bound weights or None, the net): what ``bigbatch`` answers for the state of this case, on CPU tensors."""
    from cleandiffuser_amd.engine import bigbatch
    c, net = CASES[name], build_net(name)
    fam = bigbatch.family_of(net)
    return fam, (None if fam is None else bigbatch._binding(fam, net, torch.zeros(c.batch, *c.x_shape))), net


def classes(name):
    """The coverage classes a served case is in."""
    c = CASES[name]
    fam, bound, net = binding(name)
    w, pair = bound.struct, c.mode == "sample"
    if c.family == "dit":
        width, heads, tokens, limit = w.d_model, w.n_heads, w.tokens, 65
    elif c.family == "chitf":
        width, heads, tokens, limit = w.d_model, w.n_heads, w.Ta, 64
    elif c.family == "pearcetf":
        width, heads, tokens, limit = w.te * w.n_heads, w.n_heads, 2 + w.To, 64
    else:
        width, heads, tokens, limit = w.hidden, None, None, None
    chunk = c.chunk or fam.chunk(net, w, c.batch, 2 if pair else 1)
    out = set()
    if width % 4:
        out.add("unaligned_width")
    if tokens is not None:
        if tokens == (3 if c.family == "pearcetf" else 1):
            out.add("fewest_tokens")
        if tokens == limit and (c.family != "chitf" or 1 + w.To == 16):
            out.add("token_limit")
        if width // heads == 64:
            out.add("head_dim_64")
        if (width // heads) % 2:
            out.add("odd_head_dim")
    if chunk < c.batch and c.batch % chunk:
        out.add("uneven_chunks")
        if pair and c.batch % chunk == 1:
            out.add("pair_last_chunk_of_one")
    if c.family == "dit":
        out |= ({"depth0_pair"} if pair and w.depth == 0 else set()) | ({"no_condition"} if c.cond_shape is None else set()) | \
               ({"cross"} if w.cross else set())
    if c.family == "chitf" and w.n_enc_layers > 0:
        out.add("encoder_pair" if pair else "encoder_forward")
    if c.family == "mlp":
        out |= ({"no_blocks"} if w.n_blocks == 0 else set()) | ({"head_mish"} if w.head_mish else set())
    return out


# ------------------------------------------------------------------------------------------------ #
# inputs and runs                                                                                      #
# ------------------------------------------------------------------------------------------------ #
def is_fourier(name):
    return CASES[name].ctor.get("timestep_emb_type") == "fourier"


def make_inputs(name):
    """Seeded float32 numpy inputs of a case.  forward: x, t, cond.  sample: prior, noise (the recorded draws, x_T first), cond."""
    c = CASES[name]
    g = torch.Generator().manual_seed(3000 + TABLE.index(name))
    x = torch.randn(c.batch, *c.x_shape, generator=g)
    cond = torch.randn(c.batch, *(c.cond_shape or (1,)), generator=g)
    if c.mode == "sample":
        noise = torch.randn(S.N_DRAWS, c.batch, *c.x_shape, generator=g)
        return {"prior": x.numpy(), "noise": noise.numpy(), "cond": cond.numpy()}
    # Fourier: continuous times in (0, 1).  Positional: integer timesteps, as the solvers of the discrete classes hand them on
    t = 0.01 + 0.98 * torch.rand(c.batch, generator=g) if is_fourier(name) else torch.randint(0, 1000, (c.batch,), generator=g).float()
    return {"x": x.numpy(), "t": t.numpy(), "cond": cond.numpy()}


def forward(name, net, inp, device="cpu", dtype=torch.float32):
    """``net(x, t, cond)`` of a forward-mode case.  The timesteps stay fp32 (the embedding the host evaluates for the device) unless the
    embedding has weights of `dtype` (Fourier)."""
    c = CASES[name]
    to = lambda a, dt: torch.from_numpy(a).to(device=device, dtype=dt)          # noqa: E731
    with torch.no_grad():
        return net(to(inp["x"], dtype), to(inp["t"], dtype if is_fourier(name) else torch.float32),
                   None if c.cond_shape is None else to(inp["cond"], dtype)).detach()


def cpu_run(name, dtype, w_cfg=W_CFG):
    """One CPU run of a case in `dtype` -> x and, for a sample-mode case, the classifier-free halves of every denoiser call."""
    c, inp = CASES[name], make_inputs(name)
    if c.mode == "sample":
        r = S.host_run(None, dtype, None, inp=inp, case=solver_case(name, w_cfg), spec=spec_of(name))
        return SimpleNamespace(x=r.x, halves=r.halves, plan=r.plan, env=r.env, inp=inp)
    return SimpleNamespace(x=forward(name, build_net(name, "cpu", dtype), inp, dtype=dtype), halves=[], plan=None, env=None, inp=inp)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 CPU run of a case: computed once per process and never modified."""
    return cpu_run(name, torch.float64)


def device_run(name, device):
    """The case through the package's public route on `device`, fp32 -> x."""
    c, inp = CASES[name], make_inputs(name)
    if c.mode == "sample":
        case = solver_case(name)
        return S.sample(S.build(None, None, device, case=case, spec=spec_of(name)), case, inp, device=device)
    return forward(name, build_net(name, device), inp, device=device)
