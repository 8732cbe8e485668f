"""TEST HELPER for the multi-tensor optimiser step (csrc/cdx_optim.hip: ``cdx_optim_f32`` behind engine/optim.py): ONE parameter set, a
table of step scenarios, and a float64 reference written term by term from the kernel's comments -- clip, then AdamW (decoupled decay)
or Adam (L2 decay), then the EMA fold, over three steps.  tests/test_optim_cases_cpu.py holds that reference against torch's own
sequence in float64 and measures the YARDSTICK (the same sequence in fp32); tests/test_gpu_optim.py runs every scenario on the device
at 4 x that.  Nothing here is derived from a device result.

The parameter set (``SHAPES``, twice):

* 1-D tensors of 1, 3, 5, 4095, 4096, 4097 and 8195 elements and one 40 x 12: a chunk of the kernel is 4096 floats, a float4 four --
  so the set has tensors shorter than a float4, float4 tails of 1 and 3 elements (also in the sum-of-squares pass), a tensor one
  short of a chunk, exactly one chunk, one element into a second chunk, and three elements into a third;
* the same shapes again as contiguous views carved back to back from ONE flat buffer at an offset of 1 float (``carve``): none of them
  starts on a 16-byte boundary.  Parameters, gradients and EMA copies are carved that way, the moments are the optimiser's own
  (aligned) tensors -- the kernel's scalar path.  One guard float on either side of the flat buffers must come out untouched.

Two parameter groups with different lr, betas, eps and weight decay (one group decays nothing), each holding aligned and carved
tensors of every other shape.  Gradients are drawn per step with a scale that makes the first and third step clip at ``MAX_NORM`` and
the second not; they are large next to weight_decay x p, so that the L2 form's ``g + wd p`` is nowhere a cancellation down to eps.  All initial values and gradients are fp32-representable: every side starts from the same numbers."""
import itertools
from types import SimpleNamespace

import torch

SHAPES = [(1,), (3,), (5,), (4095,), (4096,), (4097,), (8195,), (40, 12)]
N_ALIGNED = len(SHAPES)                     # tensors 0 .. 7: their own allocations; 8 .. 15: carved from one flat buffer
NUMEL = [int(torch.Size(s).numel()) for s in SHAPES]
GUARD = 1                                   # floats in front of and behind the carved views
STEPS = 3
GRAD_SCALE = (0.5, 0.02, 0.5)               # total norms ~ 102, 4.1, 102
MAX_NORM = 20.0
EMA_RATE = 0.9
GROUPS = ({"lr": 3e-3, "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": 1e-2},
          {"lr": 1e-3, "betas": (0.8, 0.95), "eps": 1e-6, "weight_decay": 0.0})
GROUP_OF = [i % 2 for i in range(2 * N_ALIGNED)]      # tensor -> its group: both groups hold aligned and carved tensors

# The largest error of torch's own sequence in fp32 on the CPU against float64, over every scenario and p / exp_avg / exp_avg_sq / the
# EMA copy / the reported norm, each relative to its tensor's largest element, rounded up (tests/test_optim_cases_cpu.py asserts it).
YARDSTICK = 2e-7
FACTOR = 4.0

SCENARIOS = {f"{'adamw' if decoupled else 'adam'}_{'clip' if clip else 'noclip'}_{'ema' if ema else 'noema'}_{'zero' if zero else 'keep'}":
             SimpleNamespace(decoupled=decoupled, clip=clip, ema=ema, zero_grad=zero)
             for decoupled, clip, ema, zero in itertools.product((True, False), repeat=4)}
TABLE = list(SCENARIOS)


def carve(flat: torch.Tensor) -> list:
    """Views of SHAPES carved back to back from `flat` (GUARD + sum(NUMEL) + GUARD floats), the first at an offset of GUARD."""
    out, off = [], GUARD
    for shape, n in zip(SHAPES, NUMEL):
        out.append(flat[off:off + n].view(shape))
        off += n
    assert off + GUARD == flat.numel()
    return out


def flat_size() -> int:
    return 2 * GUARD + sum(NUMEL)


def _draw(gen, shape, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale).float().double()


def initial() -> list:
    """The 16 initial parameter values (float64 tensors holding fp32-representable numbers)."""
    g = torch.Generator().manual_seed(41)
    return [_draw(g, s) for s in SHAPES + SHAPES]


def gradients(poison=None) -> list:
    """[step][tensor] -> gradient (float64, fp32-representable).  `poison`: (value, step, tensor, flat index) written over one element."""
    g = torch.Generator().manual_seed(42)
    # (the steps share a component, as the gradients of a real loss do: the first moment of a one-element tensor is then a sum of like
    #  signs, not a cancellation whose relative error says nothing about the arithmetic)
    base = [torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES + SHAPES]
    base = [b + torch.sign(b) for b in base]
    out = [[((b + 0.5 * torch.randn(b.shape, generator=g, dtype=torch.float64)) * 0.5 * GRAD_SCALE[step]).float().double() for b in base]
           for step in range(STEPS)]
    if poison is not None:
        value, step, tensor, index = poison
        out[step][tensor].view(-1)[index] = value
    return out


def reference(scn, grads=None, steps=STEPS):
    """The float64 reference: csrc/cdx_optim.hip's arithmetic, term by term.  -> p, m, v, ema (or None): lists of 16; norms: per step."""
    grads = gradients() if grads is None else grads
    p = [t.clone() for t in initial()]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    ema = [t.clone() for t in p] if scn.ema else None
    norms = []
    for step in range(1, steps + 1):
        gs = [g.clone() for g in grads[step - 1]]
        if scn.clip:
            # mode SUMSQ: the total norm; torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1) -- NaN stays NaN
            total = torch.sqrt(sum((g * g).sum() for g in gs))
            coef = torch.clamp(MAX_NORM / (total + 1e-6), max=1.0)
            norms.append(float(total))
            gs = [g * coef for g in gs]                               # gg *= clip
        for i, g in enumerate(gs):
            o = GROUPS[GROUP_OF[i]]
            (b1, b2), lr, wd, eps = o["betas"], o["lr"], o["weight_decay"], o["eps"]
            if scn.decoupled:
                p[i] = p[i] * (1.0 - lr * wd)                         # pp *= decay
            else:
                g = g + wd * p[i]                                     # gg = gg + l2 * pp
            m[i] = m[i] + (1.0 - b1) * (g - m[i])                     # lerp_(grad, 1 - beta1)
            v[i] = v[i] * b2 + (1.0 - b2) * g * g                     # mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
            denom = torch.sqrt(v[i]) / (1.0 - b2 ** step) ** 0.5 + eps
            p[i] = p[i] - (lr / (1.0 - b1 ** step)) * (m[i] / denom)  # addcdiv_(exp_avg, denom, value = -step_size)
            if ema is not None:
                ema[i] = ema[i] * EMA_RATE + (1.0 - EMA_RATE) * p[i]  # the EMA of the NEW parameter
    return SimpleNamespace(p=p, m=m, v=v, ema=ema, norms=norms)


def torch_sequence(scn, dtype, grads=None, steps=STEPS):
    """The reference's own sequence on the CPU in `dtype`: clip_grad_norm_ -> torch.optim.AdamW / Adam (single-tensor path) -> the EMA
    loop (reference diffusion/basic.py:66,83-86)."""
    grads = gradients() if grads is None else grads
    ps = [torch.nn.Parameter(t.to(dtype)) for t in initial()]
    ema = [p.detach().clone() for p in ps] if scn.ema else None
    cls = torch.optim.AdamW if scn.decoupled else torch.optim.Adam
    opt = cls([{"params": [p for p, gi in zip(ps, GROUP_OF) if gi == k], **GROUPS[k]} for k in range(len(GROUPS))], foreach=False)
    norms = []
    for step in range(steps):
        for p, g in zip(ps, grads[step]):
            p.grad = g.to(dtype)
        if scn.clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False)))
        opt.step()
        if ema is not None:
            with torch.no_grad():
                for p, e in zip(ps, ema):
                    e.mul_(EMA_RATE).add_(p.detach(), alpha=1.0 - EMA_RATE)
    return SimpleNamespace(p=[p.detach() for p in ps], m=[opt.state[p]["exp_avg"] for p in ps], v=[opt.state[p]["exp_avg_sq"] for p in ps],
                           ema=ema, norms=norms, steps=[float(opt.state[p]["step"]) for p in ps])


def errors(got, ref) -> dict:
    """{(kind, tensor): max |got - ref| / max |ref|} over p, m, v, ema and the norms (a norm: relative to itself).  Where the reference
    is not finite the other side must hold the same non-finite value (inf otherwise); the rest is measured among the finite elements."""
    out = {}
    for kind in ("p", "m", "v", "ema"):
        want = getattr(ref, kind)
        if want is None:
            assert getattr(got, kind) is None
            continue
        for i, (g, w) in enumerate(zip(getattr(got, kind), want)):
            g = g.detach().double().cpu()
            assert g.shape == w.shape
            ok = torch.isfinite(w)
            same = torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(g[~ok & ~torch.isnan(w)], w[~ok & ~torch.isnan(w)])
            if not same:
                out[kind, i] = float("inf")
            elif ok.any():
                d, top = float((g[ok] - w[ok]).abs().max()), float(w[ok].abs().max())
                out[kind, i] = d / top if top > 0.0 else (0.0 if d == 0.0 else float("inf"))
            else:
                out[kind, i] = 0.0
    assert len(got.norms) == len(ref.norms)
    for s, (g, w) in enumerate(zip(got.norms, ref.norms)):
        if w != w or w in (float("inf"), -float("inf")):
            out["norm", s] = 0.0 if (g != g if w != w else g == w) else float("inf")
        else:
            out["norm", s] = abs(g - w) / w
    return out


def worst(errs: dict):
    k = max(errs, key=lambda n: errs[n])
    return k, errs[k]
