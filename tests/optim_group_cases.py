"""The rule of a grouped, clipped AdamW step in numpy / float64, for cir_grads_sumsq, cir_adamw_begin_clip, cir_adamw_step_groups
(csrc/train_optim.hip) and for train_optim.AdamW with several parameter groups and max_grad_norm.  A plain module in the style of
tests/optim_cases.py, whose one-step float64 reference and elementwise bound (`step_terms`) it applies per element with that element's
group scalars.  Imported by tests/test_optim_group_cases_cpu.py (a correct fp32 stand-in passes every scenario, each wrong form fails on a
named one) and by tests/test_optim_groups_gpu.py (the kernels through their wrappers).

The norm.  total = sqrt(sum over EVERY element the step applies of g^2), the sum in float64 from the fp32 gradients, the root rounded to
fp32 (`norm32`).  A square of an fp32 number has 48 significant bits: exact in float64.  A float64 sum of N non-negative terms, in any
order and with any tree, is within (N - 1) 2^-53 relative of the exact sum (every partial sum is rounded once, relative to a value no
larger than the total); the square root halves a relative error and adds its own 2^-53.  At N = 4e7 the sum is within 4.4e-9 and the
root within 2.3e-9, against half an fp32 ulp of at least 2^-25 = 3.0e-8 relative: the float64 norm of ANY summation order lies within 0.08
fp32 ulp of the exact norm, so two
such norms rounded to fp32 are the same number or neighbours.  One more ulp is granted to a root taken in fp32 from the rounded sum:
the fp32 norm must be within NORM_ULPS = 2 ulp of `norm32`.  Nothing here is measured.

The coefficient.  coef = min(1, max_norm / (norm + 1e-6)) in fp32 from the fp32 norm (torch.nn.utils.clip_grad_norm_'s rule): the fp32
sum norm + float32(1e-6), the correctly rounded fp32 quotient of float32(max_norm) by it, the clamp.  `coef32` is bit for bit what
cir_adamw_begin_clip must leave FROM ITS OWN fp32 norm.

The step.  g_c = float32(g * coef), one fp32 rounding; then optim_cases.step_terms(p, g_c, m, v, (lr_k, b1, b2, eps_k, wd_k), t) on the
elements of group k, with lr_k = float32(lr * lr_scale).  `elem_groups` maps a segment table (ascending END offsets, one group id per
segment) to the group of every element; the padding behind a parameter belongs to the segment before it.

Scenarios (`SCENARIOS`).  One whole step each: work items (each a buffer with its segment lengths and group ids), group scalars, max_norm
and a gradient scale.  Segment lengths 8, 16, 2040, 2048 and 2056 (in the order 2040, 8, 16, 2048, 2056) put boundaries before, on and
behind the edge of the kernel's 2048-element block; the second work item starts with a segment of 1032, which puts its boundaries behind
the kernel's two-float4 stride (float4 256 of a block: a thread's SECOND float4).  Gradients are seeded and span +-[2^-12, 2^4); p is
normal, m and v a plausible history.  The range rule of optim_cases (`in_range`) must hold for the CLIPPED gradient - asserted for every
scenario by the CPU file.
    clip_active     norm > max_norm, three groups with different lr_scale / weight_decay / eps, two work items
    clip_inactive   norm < max_norm: coef must be exactly 1
    clip_at         max_norm = the norm itself: coef = norm / (norm + 1e-6), 1 or just under it
    no_clip         groups only
    one_item        one work item, two groups
    tiny_norm       norm of the order of 1e-6: the +1e-6 halves the coefficient
    huge            gradients of 1e20: the squares overflow fp32, the float64 sum does not; the clip brings g_c back into range
    eight_groups    8 groups in one buffer
    one_group       ONE group, clip active - AdamW(params, max_grad_norm=x): a buffer of 2051 elements (no table can describe it: a tail)
                    and one of 2056 (one segment)
    one_group_no_clip   the same without a clip
"""
import numpy as np
import torch

from tests import optim_cases as O

NORM_ULPS = 2
SEG_LENGTHS = (2040, 8, 16, 2048, 2056)            # ends 2040, 2048, 2064, 4112, 6168: before, on and behind a block's edge
SEG_LENGTHS_B = (1032, 2056, 8, 2040)              # ends 1032, 3088, 3096, 5136: boundaries in the SECOND float4 of a thread
B1, B2 = O.f32(0.9), O.f32(0.999)


def f32(x):
    return float(np.float32(x))


# ================================================================================================ norm and coefficient
def sumsq64(grads):
    """The float64 sum of squares of fp32 arrays / tensors."""
    return float(sum(np.square(np.asarray(g, dtype=np.float32).astype(np.float64)).sum() for g in grads))


def norm32(grads):
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(np.float64(sumsq64(grads))))


def ulps32(a, b):
    """Distance of two finite fp32 numbers in units in the last place (ordered-integer distance)."""
    def key(x):
        i = int(np.array(x, dtype=np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def coef32(norm, max_norm):
    """clip_grad_norm_'s coefficient from an fp32 norm, in fp32, as np.float32."""
    with np.errstate(all="ignore"):
        return np.float32(min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))))


def clipped(g, coef):
    """float32(g * coef) of an fp32 tensor."""
    return (g.float() * torch.tensor(float(coef), dtype=torch.float32)).float()


# ================================================================================================ segments and the step
def seg_ends(lengths):
    return np.cumsum(np.asarray(lengths, dtype=np.int64)).tolist()


def elem_groups(ends, ids, n):
    """The group id of every element of a buffer of n elements under a segment table."""
    assert ends[-1] == n and len(ends) == len(ids)
    return torch.from_numpy(np.repeat(np.asarray(ids, dtype=np.int64), np.diff([0] + list(ends))))


def applied(groups):
    """[(lr, wd, eps)] as the kernel receives them: float32(lr * lr_scale), float32(wd), float32(eps), held in Python floats."""
    return [(f32(g["lr"] * g.get("lr_scale", 1.0)), f32(g["weight_decay"]), f32(g["eps"])) for g in groups]


def group_step_terms(p, g, m, v, egroups, scalars, t, coef=None, betas=(B1, B2)):
    """(ref, bound) {p, m, v: float64 tensor} of one step of a buffer whose element i belongs to group egroups[i] with
    scalars[k] = (lr, wd, eps) (fp32 values); coef: the fp32 clip coefficient (None: no clip)."""
    gc = g if coef is None else clipped(g, coef)
    ref = {k: torch.zeros(p.numel(), dtype=torch.float64) for k in "pmv"}
    bnd = {k: torch.zeros(p.numel(), dtype=torch.float64) for k in "pmv"}
    for k, (lr, wd, eps) in enumerate(scalars):
        sel = egroups == k
        if not bool(sel.any()):
            continue
        hp = (lr, betas[0], betas[1], eps, wd)
        assert bool(O.in_range(gc[sel], v[sel], hp, t).all()), "the clipped gradient leaves the range rule"
        r, b = O.step_terms(p[sel], gc[sel], m[sel], v[sel], hp, t)
        for name in "pmv":
            ref[name][sel], bnd[name][sel] = r[name], b[name]
    return ref, bnd


def check_step(what, outputs, ref, bnd):
    return O._check(what, outputs, {n: ref[n] for n in outputs}, {n: bnd[n] for n in outputs})


# ================================================================================================ scenarios
class Scenario:
    def __init__(self, name, items, groups, max_norm, gscale=1.0, t=3, seed=0):
        """items: [(segment lengths, group ids)]; groups: [{lr, lr_scale?, weight_decay, eps}]; max_norm: float, None, or ("x", f) = f times
        the scenario's own norm32."""
        self.name, self.items, self.groups, self.gscale, self.t, self.seed = name, items, groups, gscale, t, seed
        self._max_norm = max_norm

    def __repr__(self):
        return f"scenario[{self.name}]"

    def inputs(self):
        """Per work item: dict(p, g, m, v fp32 tensors, ends, ids, egroups)."""
        out = []
        for j, (lengths, ids) in enumerate(self.items):
            n = int(sum(lengths))
            gen = torch.Generator(device="cpu").manual_seed(7000 + 131 * self.seed + j)
            g = (torch.randn((n,), generator=gen) * torch.exp2(torch.randint(-12, 4, (n,), generator=gen).float())).float() * np.float32(self.gscale)
            p = torch.randn((n,), generator=gen)
            m = torch.randn((n,), generator=gen) * 1e-2
            v = torch.rand((n,), generator=gen) * 1e-3
            ends = seg_ends(lengths)
            out.append(dict(p=p, g=g.float(), m=m, v=v, ends=ends, ids=list(ids), egroups=elem_groups(ends, ids, n)))
        return out

    @property
    def max_norm(self):
        if isinstance(self._max_norm, tuple):
            return float(norm32([i["g"].numpy() for i in self.inputs()])) * self._max_norm[1]
        return self._max_norm


_G3 = [dict(lr=1e-2, weight_decay=0.05, eps=1e-6), dict(lr=1e-2, weight_decay=0.0, eps=1e-8),
       dict(lr=1e-2, lr_scale=0.1, weight_decay=0.5, eps=1e-7)]
_G8 = [dict(lr=1e-2 * (k + 1), lr_scale=1.0 / (k + 1) if k % 2 else 0.5, weight_decay=0.05 * k, eps=10.0 ** -(5 + k % 4)) for k in range(8)]
_TWO = [(SEG_LENGTHS, (0, 1, 2, 0, 1)), (SEG_LENGTHS_B, (2, 1, 0, 2))]

SCENARIOS = {s.name: s for s in (
    Scenario("clip_active", _TWO, _G3, ("x", 0.5), seed=1),
    Scenario("clip_inactive", _TWO, _G3, ("x", 4.0), seed=2),
    Scenario("clip_at", _TWO, _G3, ("x", 1.0), seed=3),
    Scenario("no_clip", _TWO, _G3, None, seed=4),
    Scenario("one_item", [((2048, 16), (0, 1))], _G3[:2], ("x", 0.25), seed=5),
    Scenario("tiny_norm", [((8, 8), (0, 1))], _G3[:2], 1e-6, gscale=2.0 ** -22, seed=6),
    Scenario("huge", _TWO, _G3, 1.0, gscale=1e20, seed=7),
    Scenario("one_group", [((2051,), (0,)), ((2056,), (0,))], _G3[:1], ("x", 0.5), seed=9),
    Scenario("one_group_no_clip", [((2051,), (0,)), ((2056,), (0,))], _G3[:1], None, seed=10),
    Scenario("eight_groups", [((8, 16, 2040, 2048, 2056, 8, 8, 8), tuple(range(8)))], _G8, ("x", 0.5), seed=8),
)}


def reference(scn):
    """(norm32, coef32 or None, [(ref, bnd)] per work item) of a scenario."""
    items = scn.inputs()
    norm = norm32([i["g"].numpy() for i in items])
    coef = None if scn.max_norm is None else coef32(norm, scn.max_norm)
    return norm, coef, [group_step_terms(i["p"], i["g"], i["m"], i["v"], i["egroups"], applied(scn.groups), scn.t, coef) for i in items]


# ================================================================================================ an fp32 stand-in and its wrong forms
WRONG = ("coef_no_eps", "coef_no_clamp", "norm_per_item", "clip_update", "boundary_early", "boundary_late", "lr_scale_ignored",
         "wd_of_previous", "norm_fp32")


def standin(scn, wrong=None):
    """The step in fp32 numpy as the kernels order it: (norms per item (one global norm repeated when right), coefs per item, [{p, m, v}]).
    `wrong`: one of WRONG."""
    items = scn.inputs()
    f = np.float32

    def norm_of(gs):
        if wrong == "norm_fp32":
            with np.errstate(all="ignore"):
                return f(np.sqrt(sum(np.square(g.numpy(), dtype=np.float32).sum(dtype=np.float32) for g in gs), dtype=np.float32))
        return norm32([g.numpy() for g in gs])

    def coef_of(norm):
        if scn.max_norm is None:
            return None
        with np.errstate(all="ignore"):
            c = f(scn.max_norm) / (f(norm) + (f(0.0) if wrong == "coef_no_eps" else f(1e-6)))
        return f(c) if wrong == "coef_no_clamp" else f(min(f(1.0), c))

    norms = [norm_of([i["g"]]) for i in items] if wrong == "norm_per_item" else [norm_of([i["g"] for i in items])] * len(items)
    coefs = [coef_of(x) for x in norms]
    groups = [dict(g, lr_scale=1.0) for g in scn.groups] if wrong == "lr_scale_ignored" else scn.groups
    sc = applied(groups)
    b1, b2, t = f(B1), f(B2), scn.t
    bc1, bc2 = f(1.0 - float(b1) ** t), f(1.0 - float(b2) ** t)
    outs = []
    for i, coef in zip(items, coefs):
        n = i["p"].numel()
        ends = list(i["ends"])
        if wrong in ("boundary_early", "boundary_late") and len(ends) > 1:
            ends = [e + (-4 if wrong == "boundary_early" else 4) for e in ends[:-1]] + ends[-1:]
        eg = elem_groups(ends, i["ids"], n).numpy()
        wd_g = eg.copy()
        if wrong == "wd_of_previous":
            for e, prev in zip(i["ends"][:-1], i["ids"][:-1]):
                wd_g[e:e + 4] = prev
        lr, eps = (np.array([s[k] for s in sc], dtype=np.float32)[eg] for k in (0, 2))
        wd = np.array([s[1] for s in sc], dtype=np.float32)[wd_g]
        p, g, m, v = (i[k].numpy().astype(np.float32) for k in "pgmv")
        with np.errstate(all="ignore"):
            gc = g if coef is None or wrong == "clip_update" else (g * coef).astype(np.float32)
            m1 = (b1 * m + (f(1.0) - b1) * gc).astype(np.float32)
            v1 = (b2 * v + (f(1.0) - b2) * gc * gc).astype(np.float32)
            upd = (lr * (m1 / bc1) / (np.sqrt(v1 / bc2, dtype=np.float32) + eps)).astype(np.float32)
            if wrong == "clip_update" and coef is not None:
                upd = (upd * coef).astype(np.float32)
            p1 = (p * (f(1.0) - lr * wd) - upd).astype(np.float32)
        outs.append({k: torch.from_numpy(x) for k, x in (("p", p1), ("m", m1), ("v", v1))})
    return norms, coefs, outs


def check(scn, norms, coefs, outs):
    """Every failure of a stand-in's (or the kernels') results against the reference of a scenario."""
    norm, coef, terms = reference(scn)
    fails = []
    for j, (nj, cj, out, (ref, bnd)) in enumerate(zip(norms, coefs, outs, terms)):
        if not (np.isfinite(nj) and ulps32(nj, norm) <= NORM_ULPS):
            fails.append(f"{scn} item {j}: norm {nj!r}, expected {norm!r} within {NORM_ULPS} ulp")
        if coef is not None and np.float32(cj).tobytes() != coef32(nj, scn.max_norm).tobytes():
            fails.append(f"{scn} item {j}: coef {cj!r} is not {coef32(nj, scn.max_norm)!r}, the rule applied to the norm {nj!r}")
        fails += check_step(f"{scn} item {j}", out, ref, bnd)
    return fails
