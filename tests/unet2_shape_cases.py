"""TEST HELPER for the denoiser forward of the program kernel (csrc/cdx_unet2.hip: the op interpreter -- conv taps, stride-2 down and
transposed up, the GroupNorm epilogue partition, FiLM, residual and skip concat -- behind ``runtime2.backbone_forward2`` and
``runtime2.fused_sample2``): a fixed table of the smallest nets that reach each axis of its shapes, in every program form ``runtime2``
can launch for them, and for each row ONE float64 CPU run -- the reference tests/test_gpu_unet2_shapes.py compares the device with.
Nothing is drawn at test time: the table is pinned by value, the weights are ``load_synth`` streams, the inputs seeded draws.

A row is a net (class, constructor arguments), H and D, a condition shape or None, a batch, a mode and the set of forms it exists in:

* ``forward``: ``net(x, t, cond)`` with a timestep per sample (0 and 999 among them) -- ``runtime2.backbone_forward2``, one launch
  with n_steps 0 and a FiLM row per trajectory.  The reference is the stock module on the CPU in float64; the positional embedding is
  evaluated on the fp32 timesteps and handed on as float64 (the hook of ``solver_step_cases.build``).  The four ordinary forms only.
* ``sample``: ``agent.sample`` of a DiscreteDiffusionSDE with a two-step ddim plan and x0-prediction on a recorded x_T --
  ``runtime2.fused_sample2``, the only route to the compact, split and grouped programs; a conditional row runs the classifier-free
  pair (w_cfg 1.3: two passes per step, the unconditional FiLM row).  The reference is the package's own host loop in float64
  (``solver_step_cases.host_run``).

Forms, and the hooks of ``runtime2`` that select them (``ENV``): ``nw4_t1 nw4_t2 nw8_t1 nw8_t2`` the ordinary program with 4 or 8 waves
and one or two trajectories per workgroup (CDX_UNET2_NW, CDX_UNET2_T); ``compact_t1..3`` the compact program (CDX_UNET2_COMPACT, and
CDX_UNET2_T=3); ``split2 split4`` one trajectory over 2 or 4 workgroups (CDX_UNET2_SPLIT); ``group2 group4`` the grouped program
(CDX_UNET2_GROUP).  A row lists exactly the forms it exists in (``available``; tests/test_unet2_shape_cases_cpu.py pins them): a
compiler change that moves a row fails there, so the device coverage cannot thin out silently.

Batch 7 = 2 x 3 + 1 everywhere: the last workgroup is part-empty at two and at three trajectories per workgroup, the last group ragged
at k = 2 (one member) and k = 4 (three).

The table (JannerUNet1d: D, model_dim, dim_mult, kernel, emb_dim, H):
  n8_l1        (37, 8, [1], 3, 32, 8)           8-channel slots (half a 16-row tile), one level, D odd above 32
  n8_m4        (18, 8, [1,4], 5, 32, 4)         8 next to 32 channels, H 4
  n8_m3        (17, 8, [1,3], 3, 32, 8)         24-channel slots
  w16_d1       (1, 16, [1,2], 3, 16, 32)        D 1, H 32
  w16_h64      (40, 16, [1,2], 3, 16, 64)       H 64, D 40
  w64_m4       (9, 64, [1,2,4], 5, 64, 16)      81 / 89 KiB: two trajectories do not fit, so the t2 forms do not exist
  cond_fwd     (3, 32, [1,4], 3, 16, 8)         a per-sample condition (the kernel's COND instantiation), emb_dim != model_dim
  n8_l4_s      (3, 8, [1,2,2,2], 5, 32, 16)     sample: narrow slots in the ordinary, compact and split programs; four levels
  w32_l4_s     (5, 32, [1,2,2,2], 5, 32, 16)    sample: every form, group4 included (123.7 KiB)
  w64_s        (6, 64, [1,2,2], 5, 64, 16)      sample: every form at model_dim 64 (group4 155.1 KiB)
  w64_m4_s     the w64_m4 net, sample           split2, split4 and group2 at 105.8 / 129.4 KiB; no compact, no group4, no t2
  cond_pair    the cond_fwd net, sample         the classifier-free pair on per-trajectory FiLM rows
ChiUNet1d with a global condition (act_dim, obs_dim, To, model_dim, dim_mult, kernel, emb_dim, H):
  chi_bias     (3, 7, 2, 16, [1,2], 5, 16, 8)   cond_predict_scale False: bias-only FiLM
  chi_to1      (2, 5, 1, 32, [1,2,2], 5, 16, 16)   To = 1, scale FiLM, emb_dim != model_dim
  chi_pair     (3, 7, 2, 16, [1,2], 3, 16, 4)   sample: scale FiLM under the classifier-free pair, H 4
Refusals (forward, batch 3): the compiler answers ValueError, ``runtime2.supported`` the reason, and the GEMM executor serves the request
(`gemm`) at the same bar -- or, for refuse_k7, nobody native does and the stock module runs: JannerUNet1d's final conv has 5 taps whatever
kernel_size says, and ``bigbatch._janner_adds`` binds nets of one kernel size only
  refuse_gn48  (33, 16, [1,3], 5, 16, 8)        "v2 epilogue needs GroupNorm groups of pad32(C)/8 channels (C=48, G=8)"
  refuse_k7    (5, 16, [1,2], 7, 16, 8)         "kernel size 7 needs more than 2 halo rows"; not `gemm`
  refuse_lds   (6, 64, [1,2,4,2], 5, 64, 32)    "LDS plan needs 187968 B > 163840 B per trajectory"; its one-trajectory compact stand-in
                                                needs 167936 B.  (Not a wide D or a long H on a smaller net: (20 .. 40, 64, [1,2,2,2], 5,
                                                H 64) and (40, 128, [1,2,2], 5, H 32) still fit as that stand-in, 157.6 KiB and less)

Candidates that were asked for and do not exist, with the compiler's message:
  kernel_size 7: (5, 16, [1,2], H 8), (5, 32, [1], H 4), (5, 8, [1], emb 32, H 8), (5, 64, [1,2], H 16) -- every one
      "kernel size 7 needs more than 2 halo rows": no 7 row, refuse_k7 instead.
  a 3 in dim_mult at model_dim 16: 48 channels, "v2 epilogue needs GroupNorm groups of pad32(C)/8 channels (C=48, G=8)" (refuse_gn48);
      the 3 is covered at model_dim 8.
  split / grouped forms of the narrow one- and two-level nets, of (1, 16, [1,2]), (4 / 40, 16, [1,2], H 64) and (38, 32, [1,2], H 8):
      "split program: no op of this net streams enough weights to be cut over the members" (the grouped compiler fails on the same
      merge first).  n8_l4_s is the only narrow net with a split form (one cut op); none has a grouped one.
  group4 of (6, 32, [1,2,4], 5, H 32): the same message (8 grouped ops at k = 2, none worth it at k = 4); of w64_m4: "LDS plan needs
      224064 B > 163840 B per trajectory".  compact of w64_m4: "LDS plan needs 64576 B > 54608 B per trajectory".
  (6, 64, [1,2,4], 5, H 64): "epilogue: 256 float4 items per group > 128 (horizon too long for v2)".
  (6, 64, [1,2,2,2], 5, H 32): 107.6 KiB, split2 123.6, split4 155.6 KiB; group2 "LDS plan needs 179840 B > 163840 B", group4 "LDS plan
      beyond the 16-bit slot offsets of the item format (slot at float 66240)" -- not a row: w64_s has every form at a quarter of the twin's time.
"""
import functools
from types import SimpleNamespace

import torch

import solver_step_cases as S

B = 7                       # 2 x 3 + 1
W_CFG = 1.3
LDS_LIMIT = 160 * 1024
T_LAST = 999                # the last step of the solver classes' default schedule

ORDINARY = ("nw4_t1", "nw4_t2", "nw8_t1", "nw8_t2")
COMPACT = ("compact_t1", "compact_t2", "compact_t3")
SPLIT = ("split2", "split4")
GROUP = ("group2", "group4")
FORMS = ORDINARY + COMPACT + SPLIT + GROUP
HOOKS = ("CDX_UNET2_T", "CDX_UNET2_NW", "CDX_UNET2_COMPACT", "CDX_UNET2_SPLIT", "CDX_UNET2_GROUP")
ENV = {**{f"nw{nw}_t{t}": {"CDX_UNET2_NW": str(nw), "CDX_UNET2_T": str(t)} for nw in (4, 8) for t in (1, 2)},
       **{f"compact_t{t}": {"CDX_UNET2_COMPACT": "1", "CDX_UNET2_T": str(t)} for t in (1, 2, 3)},
       **{f"split{k}": {"CDX_UNET2_SPLIT": str(k), "CDX_UNET2_GROUP": "0"} for k in (2, 4)},
       **{f"group{k}": {"CDX_UNET2_SPLIT": "0", "CDX_UNET2_GROUP": str(k)} for k in (2, 4)}}


def program_key(form):
    """The program a form runs: the t1 / t2 / t3 forms of one program share it."""
    return form.split("_t")[0]


# ------------------------------------------------------------------------------------------------ #
# the table                                                                                            #
# ------------------------------------------------------------------------------------------------ #
def _j(D, md, dm, ks, emb, H, mode="forward", cond=False, forms=ORDINARY, batch=B, refused=None, gemm=True, den_scale=1.0):
    ctor = dict(in_dim=D, model_dim=md, emb_dim=emb, dim_mult=list(dm), kernel_size=ks)
    family = ("cond_pair" if cond else "janner_sample") if mode == "sample" else "janner_fwd"
    return SimpleNamespace(cls="JannerUNet1d", ctor=ctor, H=H, D=D, cond_shape=(emb,) if cond else None, batch=batch, mode=mode,
                           forms=tuple(forms), family=family, refused=refused, gemm=gemm, den_scale=den_scale)


def _chi(act, obs, To, md, dm, ks, emb, H, scale=True, mode="forward", forms=ORDINARY, den_scale=1.0):
    ctor = dict(act_dim=act, obs_dim=obs, To=To, model_dim=md, emb_dim=emb, dim_mult=list(dm), kernel_size=ks, cond_predict_scale=scale,
                obs_as_global_cond=True)
    return SimpleNamespace(cls="ChiUNet1d", ctor=ctor, H=H, D=act, cond_shape=(To, obs), batch=B, mode=mode, forms=tuple(forms),
                           family="chi_sample" if mode == "sample" else "chi_fwd", refused=None, gemm=True, den_scale=den_scale)


def _sampled(row, forms, den_scale=1.0):
    return SimpleNamespace(**{**vars(row), "mode": "sample", "forms": tuple(forms), "den_scale": den_scale,
                              "family": "cond_pair" if row.cond_shape is not None else "janner_sample"})


def _table():
    t = {}
    t["n8_l1"] = _j(37, 8, [1], 3, 32, 8)
    t["n8_m4"] = _j(18, 8, [1, 4], 5, 32, 4)
    t["n8_m3"] = _j(17, 8, [1, 3], 3, 32, 8)
    t["w16_d1"] = _j(1, 16, [1, 2], 3, 16, 32)
    t["w16_h64"] = _j(40, 16, [1, 2], 3, 16, 64)
    t["w64_m4"] = _j(9, 64, [1, 2, 4], 5, 64, 16, forms=("nw4_t1", "nw8_t1"))
    t["cond_fwd"] = _j(3, 32, [1, 4], 3, 16, 8, cond=True)
    t["n8_l4_s"] = _j(3, 8, [1, 2, 2, 2], 5, 32, 16, mode="sample", forms=ORDINARY + COMPACT + SPLIT)
    t["w32_l4_s"] = _j(5, 32, [1, 2, 2, 2], 5, 32, 16, mode="sample", forms=FORMS)
    t["w64_s"] = _j(6, 64, [1, 2, 2], 5, 64, 16, mode="sample", forms=FORMS)
    t["w64_m4_s"] = _sampled(t["w64_m4"], ("nw4_t1", "nw8_t1") + SPLIT + ("group2",))
    t["cond_pair"] = _sampled(t["cond_fwd"], ORDINARY + COMPACT)
    t["chi_bias"] = _chi(3, 7, 2, 16, [1, 2], 5, 16, 8, scale=False)
    t["chi_to1"] = _chi(2, 5, 1, 32, [1, 2, 2], 5, 16, 16)
    t["chi_pair"] = _chi(3, 7, 2, 16, [1, 2], 3, 16, 4, mode="sample", forms=ORDINARY + COMPACT)
    t["refuse_gn48"] = _j(33, 16, [1, 3], 5, 16, 8, forms=(), batch=3, refused="GroupNorm groups of pad32")
    t["refuse_k7"] = _j(5, 16, [1, 2], 7, 16, 8, forms=(), batch=3, refused="kernel size 7 needs more", gemm=False)
    t["refuse_lds"] = _j(6, 64, [1, 2, 4, 2], 5, 64, 32, forms=(), batch=3, refused="LDS plan needs")
    return t


CASES = _table()
TABLE = sorted(CASES)
SERVED = [n for n in TABLE if CASES[n].refused is None]
REFUSALS = [n for n in TABLE if CASES[n].refused is not None]
PAIRS = [(n, f) for n in SERVED for f in FORMS if f in CASES[n].forms]
FAMILIES = ("janner_fwd", "janner_sample", "cond_pair", "chi_fwd", "chi_sample")

# YARDSTICK[family]: the largest E32 over the family's rows (the refusals included), E32 = max |x32 - x64| / max(1, max |x64|) of the
# fp32 CPU run -- the stock module (forward) or the package's host loop (sample) -- against the float64 one on the same inputs, as
# tests/test_unet2_shape_cases_cpu.py measures it (its docstring has the figures), rounded up.  That test fails when the measured
# maximum leaves [YARDSTICK / 2, YARDSTICK].  The GPU tolerance is 4 x this.
YARDSTICK = {"janner_fwd": 1e-6, "janner_sample": 5.5e-6, "cond_pair": 3.5e-6, "chi_fwd": 1e-6, "chi_sample": 4e-6}

# guided_grad_cases' rule for a pair whose miss of 4 x YARDSTICK is the program's own fp32 summation order: 2 x the CPU twin's error on the
# same inputs, never above TWIN_BAR_MAX.  (row, form) -> (device error, twin error), as measured.  Empty: no pair needed it.
TWIN_BAR_MAX = 2e-4
TWIN_BAR = {}


def tolerance(name):
    return 4.0 * YARDSTICK[CASES[name].family]


# ------------------------------------------------------------------------------------------------ #
# what a row reaches: read off the constructor arguments                                               #
# ------------------------------------------------------------------------------------------------ #
REQUIRED = {"narrow_slot_8", "narrow_slot_24", "model_dim_16", "model_dim_32", "model_dim_64", "mult_3", "mult_4", "one_level", "four_levels",
            "emb_dim_differs", "kernel_3", "kernel_5", "H_4", "H_8", "H_16", "H_32", "H_64", "D_1", "D_multiple_of_4", "D_odd_above_32",
            "D_37_to_40", "batch_7", "cond_forward", "cond_pair", "chi_scale", "chi_bias", "chi_to_1"}


def widths(name):
    c, out, w = CASES[name], [], 1
    for m in c.ctor["dim_mult"]:
        w *= m
        out.append(int(c.ctor["model_dim"] * w))
    return out


def axes(name):
    """The axis values a served row reaches."""
    c, k = CASES[name], CASES[name].ctor
    out = {f"model_dim_{k['model_dim']}", f"kernel_{k['kernel_size']}", f"H_{c.H}", f"batch_{c.batch}"}
    out |= {f"narrow_slot_{w}" for w in widths(name) if w % 16}
    out |= {f"mult_{m}" for m in k["dim_mult"] if m > 2}
    out |= {{1: "one_level", 4: "four_levels"}.get(len(k["dim_mult"]), "levels")}
    out |= {"emb_dim_differs"} if k["emb_dim"] != k["model_dim"] else set()
    out |= ({"D_1"} if c.D == 1 else set()) | ({"D_multiple_of_4"} if c.D % 4 == 0 else set()) | \
           ({"D_odd_above_32"} if c.D > 32 and c.D % 2 else set()) | ({"D_37_to_40"} if 37 <= c.D <= 40 else set())
    if c.cls == "ChiUNet1d":
        out |= {"chi_scale" if k["cond_predict_scale"] else "chi_bias"} | ({"chi_to_1"} if k["To"] == 1 else set())
    elif c.cond_shape is not None:
        out.add("cond_pair" if c.mode == "sample" else "cond_forward")
    return out


# ------------------------------------------------------------------------------------------------ #
# nets, programs and forms                                                                             #
# ------------------------------------------------------------------------------------------------ #
def spec_of(name):
    """The net of a row as ``solver_step_cases.build`` takes it."""
    c = CASES[name]
    return SimpleNamespace(net=(c.cls, c.ctor), x_shape=(c.H, c.D), cond_shape=c.cond_shape, kind="chiunet", needs_cond=c.cls == "ChiUNet1d")


_PLAN = S._c("DiscreteDiffusionSDE", dict(diffusion_steps=20, predict_noise=False),
             dict(solver="ddim", sample_steps=2, sample_step_schedule="uniform"))


def solver_case(name, w_cfg=W_CFG):
    """The two-step deterministic plan over the net of `name`, as a case of ``solver_step_cases``; w_cfg only for a conditional row."""
    c = CASES[name]
    return SimpleNamespace(**{**vars(_PLAN), "x_shape": (c.H, c.D), "w_cfg": w_cfg if c.cond_shape is not None else None,
                              "den_scale": c.den_scale})


def build_net(name, device="cpu", dtype=torch.float32):
    """The net of a row in eval mode: ``solver_step_cases.build`` (its weights, its dtype hooks) under the plan's solver class."""
    return S.build(None, None, device, dtype, case=solver_case(name), spec=spec_of(name)).model_ema["diffusion"]


def available(name, net=None):
    """form -> Program2 for every form `runtime2` can launch for this row in its mode, by ``runtime2``'s own rules (shape_for, plan_for,
    member_route) on the programs of its own cache: an ordinary form needs the program of that wave count (not its compact stand-in)
    and room for its trajectories; the compact, split and grouped ones are offered to sampling loops whose 8-wave program exists, the
    last two to unconditional JannerUNet1d loops only."""
    from cleandiffuser_amd.engine import runtime2
    c, out = CASES[name], {}
    net = build_net(name) if net is None else net
    if runtime2.supported(net, c.H) is not None:
        return out
    for nw in (4, 8):
        prog = runtime2.compiled2(net, c.H, nw).prog
        if prog is not None and not prog.compact:
            out.update({f"nw{nw}_t{t}": prog for t in (1, 2) if prog.lds_bytes(t) <= LDS_LIMIT})
    if c.mode == "sample" and "nw8_t1" in out:
        prog = runtime2.compiled2(net, c.H, 8, compact=True).prog
        if prog is not None:
            out.update({f"compact_t{t}": prog for t in (1, 2, 3) if prog.lds_bytes(t) <= LDS_LIMIT})
        if c.cls == "JannerUNet1d" and c.cond_shape is None:
            for k in (2, 4):
                for tag, compiled in (("split", runtime2.compiled_split2), ("group", runtime2.compiled_group2)):
                    prog = compiled(net, c.H, k).prog
                    if prog is not None and prog.lds_bytes(1) <= LDS_LIMIT:
                        out[f"{tag}{k}"] = prog
    return out


# ------------------------------------------------------------------------------------------------ #
# inputs and runs                                                                                      #
# ------------------------------------------------------------------------------------------------ #
def make_inputs(name):
    """Seeded float32 numpy inputs of a row.  forward: x, t, cond.  sample: prior, noise (the recorded draws, x_T first), cond."""
    c = CASES[name]
    g = torch.Generator().manual_seed(4000 + TABLE.index(name))
    x = torch.randn(c.batch, c.H, c.D, generator=g)
    cond = torch.randn(c.batch, *(c.cond_shape or (1,)), generator=g)
    if c.mode == "sample":
        noise = torch.randn(S.N_DRAWS, c.batch, c.H, c.D, generator=g)
        return {"prior": x.numpy(), "noise": noise.numpy(), "cond": cond.numpy()}
    t = torch.randint(1, T_LAST, (c.batch,), generator=g).float()
    t[0], t[1] = 0.0, float(T_LAST)
    return {"x": x.numpy(), "t": t.numpy(), "cond": cond.numpy()}


def forward(name, net, inp, device="cpu", dtype=torch.float32):
    """``net(x, t, cond)`` of a forward-mode row.  The timesteps stay fp32: the embedding the host evaluates for the device."""
    c = CASES[name]
    to = lambda a, dt: torch.from_numpy(a).to(device=device, dtype=dt)          # noqa: E731
    with torch.no_grad():
        return net(to(inp["x"], dtype), to(inp["t"], torch.float32), None if c.cond_shape is None else to(inp["cond"], dtype)).detach()


def cpu_run(name, dtype, w_cfg=W_CFG):
    """One CPU run of a row in `dtype` -> x and, for a pair, the classifier-free halves of every denoiser call."""
    c, inp = CASES[name], make_inputs(name)
    if c.mode == "sample":
        r = S.host_run(None, dtype, None, inp=inp, case=solver_case(name, w_cfg), spec=spec_of(name))
        return SimpleNamespace(x=r.x, halves=r.halves, plan=r.plan, env=r.env, inp=inp)
    return SimpleNamespace(x=forward(name, build_net(name, "cpu", dtype), inp, dtype=dtype), halves=[], plan=None, env=None, inp=inp)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 CPU run of a row: computed once per process and never modified."""
    return cpu_run(name, torch.float64)


def device_build(name, device):
    """What ``device_run`` calls, built once: the agent of a sample-mode row, the net of a forward-mode one."""
    if CASES[name].mode == "sample":
        return S.build(None, None, device, case=solver_case(name), spec=spec_of(name))
    return build_net(name, device)


def device_run(name, device, built=None):
    """The row through the package's public route on `device`, fp32 -> x."""
    c, inp = CASES[name], make_inputs(name)
    built = device_build(name, device) if built is None else built
    if c.mode == "sample":
        return S.sample(built, solver_case(name), inp, device=device)
    return forward(name, built, inp, device=device)


# ------------------------------------------------------------------------------------------------ #
# the CPU twin: one denoiser forward of a program on NaN-poisoned LDS                                  #
# ------------------------------------------------------------------------------------------------ #
TWIN_T = 11                 # the timestep of the twin's forward


@functools.lru_cache(maxsize=None)
def twin_error(name, key):
    """One denoiser forward of the program `key` ("nw4", "nw8", "compact", "split2", ...) of a row through ``oracle.lane_sim2`` with
    ``poison_arena()`` -- members in lockstep for the split and grouped programs, the k members of a grouped one on k different
    trajectories -- against the fp32 module on the same inputs -> max |twin - module| / max(1, max |module|).  An address outside the
    plan reads NaN there, which is what keeps it off the device."""
    import numpy as np
    from oracle.lane_sim2 import LaneSim2, chi_film_rows, emb_table, run_forward_group, run_forward_split
    c, net = CASES[name], build_net(name)
    prog = {program_key(f): p for f, p in available(name, net).items()}[key]
    inp = make_inputs(name)
    k = int(key[5:]) if key.startswith("group") else 1
    x = torch.from_numpy(inp["x" if c.mode == "forward" else "prior"][:k])
    t = torch.full((k,), TWIN_T)
    cond = None if c.cond_shape is None else torch.from_numpy(inp["cond"][:k])
    with torch.no_grad():
        want = net(x, t, cond).numpy()
        if c.cls == "ChiUNet1d":
            rows = chi_film_rows(prog, net, t, cond)
        else:
            temb = net.map_noise(t)
            rows = emb_table(prog, (temb if cond is None else temb + cond).numpy())
    if key.startswith("group") or key.startswith("split"):
        sims = [LaneSim2(prog, member=m) for m in range(int(key[5:]))]
        for m, s in enumerate(sims):
            s.poison_arena()
            s.load_x(x[m if k > 1 else 0].numpy())
        got = np.stack(run_forward_group(sims, rows[0])) if k > 1 else run_forward_split(sims, rows[0])[None]
    else:
        sim = LaneSim2(prog)
        sim.poison_arena()
        sim.load_x(x[0].numpy())
        got = sim.run_forward(rows[0])[None]
    return float(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())))
