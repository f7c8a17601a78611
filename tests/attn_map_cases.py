"""Case table, float64 reference, a-priori ELEMENTWISE error bounds and a CPU stand-in for the attention-map kernels of
csrc/attn_maps.hip: cir_attention_maps (probs, dprobs) and cir_attention_gradcam (cam) - the conventions of tests/attn_bwd_cases.py, whose
inputs (`inputs`), layout and weight-error terms are reused, on top of attn_cases.core_terms.

A plain module, imported by tests/test_attn_map_cases_cpu.py (the stand-in `emulate`: "kernel" passes every comparison, every wrong form
fails on a named case) and by tests/test_attn_maps_gpu.py (the kernels themselves).

            CASES                the list of `Case`s: one forward launch and one launch of each entry point per case,
            dmul(case)           the multiplier handed to the kernels (1, or the inverse of the power of two of a `do = loss` case),
            ref64(case)          {probs, dprobs, cam: float64 tensor} from the rounded operands,
            bound(case)          the same names: the elementwise error bound; row_bound(case): the bound of |sum_j P_ij - 1|,
            check(case, outputs) -> list of failure messages (empty = pass),
            emulate(case, variant) -> outputs of a torch fp32 model of the kernels.

Cases
--------------------------------------------------------------------------------------------------------------------------------
The p = 0 cases of attn_bwd_cases.CASES (the maps are the PRE-dropout quantities: the kernels take no dropout argument) - six shapes
(1, 1) .. (70, 197), bf16 / fp16, the masks of that table incl. tail40, all10k and min_all, `do = loss` - and the two `items = sub7`
launches of that table at p = 0 (one head, 7 groups: the last workgroup has idle waves; H = 1: the head mean is the identity).  The three
forms of the backward call differ in nothing these kernels see; they stay in the table as they are.

Reference (float64, from the rounded operands)
--------------------------------------------------------------------------------------------------------------------------------
P^ = the softmax of attn_cases.core_terms;  G = dO V^T;  dprobs = dmul G;  cam = mean_h P^ max(dmul G, 0).

Bounds (u = 2^-24; first order, elementwise; nothing is fitted to what a kernel returns)
--------------------------------------------------------------------------------------------------------------------------------
eps_ij: the relative error of p = exp2(fma(s, scale log2e, mask log2e - lse)) against P^, exactly attn_bwd_cases' backward weight error
(score error incl. the forward's own lse error, 5 u; 1 where the weight may be flushed; a saturated row: the error of exp2(-log2 Lk)).
    |P - P^|       <= eps P^ + 2 u P^ + 2^-149                            (one fp32 ulp is at most 2 u P^)
    |dP - dmul G|  <= dmul dG + 2 u |dmul G| + 2^-149,  dG = 66 u sum_d |dO_id v_jd|      (dmul is a power of two: exact)
    |cam - ref|    <= SECOND mean_h [ eps P^ max(dmul G, 0) + P^ dmul dG ] + (H + 3) u ref + 2^-149
    |sum_j P_ij - 1| <= sum_j eps_ij P^_ij + (Lk + 4) u                  (the sum formed in float64 from the fp32 outputs: (Lk + 4) u granted)
|max(a, 0) - max(b, 0)| <= |a - b|, so the rectifier costs nothing; (H + 3) u: the H fused multiply-adds, the products with dmul and
1 / H and the reciprocal itself.  SECOND = 1 + 2^-4 covers eps dG cross terms (attn_bwd_cases.second_order_ok: E <= 0.05).
"""
import math

import torch

from tests import attn_bwd_cases as B
from tests import attn_cases as A
from tests.attn_cases import BF16, DT_NAME, F16, LN2, LOG2E, SCALE, SECOND, U, Case, case_id  # noqa: F401

OUTPUTS = ("probs", "dprobs", "cam")
SUB32 = 2.0 ** -149


def _cases():
    out = [c for c in B.CASES if c.p == 0.0]
    for dt in (BF16, F16):                                          # attn_bwd_cases' two sub7 launches, without the dropout
        out.append(Case("train_bwd", shape=(33, 100), dt=dt, mask="tail", p=0.0, form="t16", items="sub7"))
        out.append(Case("train_bwd", shape=(9, 9), dt=dt, mask="none", p=0.0, form="t16", items="sub7"))
    return out


CASES = _cases()


def case(cid):
    return next(c for c in CASES if c.id == cid)


def named(shape, dt, mask, items=None, do=None):
    """The first case with these attributes."""
    return next(c for c in CASES if (c.shape, c.dt, c.mask, getattr(c, "items", None), getattr(c, "do", None)) == (shape, dt, mask, items, do))


def dmul(c):
    """1, or for a `do = loss` case the inverse of the power of two its dO was multiplied by (exact: read off the largest element)."""
    if getattr(c, "do", None) != "loss":
        return 1.0
    plain = Case("train_bwd", shape=c.shape, dt=c.dt, mask=c.mask, p=c.p, form=c.form)
    small = float(B.inputs(plain)["do"].double().abs().max())
    big = float(B.inputs(c)["do"].double().abs().max())
    k = round(math.log2(big / small))
    assert big == small * 2.0 ** k
    return 2.0 ** -k


_last = {}


def _cached(c, key, fn):
    if _last.get("case") is not c:
        _last.clear()
        _last["case"] = c
    if key not in _last:
        _last[key] = fn(c)
    return _last[key]


# ================================================================================================ reference and bound
def _terms(c):
    dm = dmul(c)                                                    # (first: it reads another case's inputs through the same one-slot cache)
    i = B.inputs(c)
    lq, lk = c.shape
    g_n, h_n, _ = B.layout(c)
    q, k, v, do = (i[n].double() for n in ("q", "k", "v", "do"))
    mask = i["mask"]
    t = A.core_terms(i["q"], i["k"], i["v"], mask, c.dt)
    ph, x, sat, lse, b_lse = t["p"], t["x"], t["sat"], t["lse"], t["b_lse"]
    if mask is not None:                                            # a row whose EVERY key is saturated: the kernels' lse is their clamp
        all_sat = sat.all(-1)
        lse = torch.where(all_sat, mask.double().clamp_min(B.KERNEL_CLAMP).max(-1).values[:, None] * LOG2E + math.log2(lk), lse)
        b_lse = torch.where(all_sat, 2 * U * lse.abs(), b_lse)
    # ---- the weight error of the recomputed p (attn_bwd_cases._terms, "backward: the weights")
    sl = SCALE * LOG2E
    s = q @ k.transpose(1, 2) * sl
    e_s = 66 * U * sl * (q.abs() @ k.abs().transpose(1, 2)) + 3 * U * s.abs()
    if mask is not None:
        m2 = mask.double().clamp_min(-1e30)[:, None, :] * LOG2E
        e_s = e_s + U * m2.abs() + U * (m2 - lse[:, :, None]).abs()
    e_s = e_s + U * (x - lse[:, :, None]).abs() + b_lse[:, :, None]
    e_s = torch.where(sat, torch.full_like(e_s, 2 * U * (math.log2(lk) + 6)), e_s)
    eps = LN2 * e_s + 5 * U
    eps = torch.where(lse[:, :, None] - x > 125, torch.ones_like(eps), eps)
    # ---- the maps
    g = do @ v.transpose(1, 2) * dm
    d_g = 66 * U * (do.abs() @ v.abs().transpose(1, 2)) * dm
    heads = lambda z: z.view(g_n, h_n, lq, lk)                      # noqa: E731
    cam = heads(ph * g.clamp_min(0)).mean(1)
    b_cam = SECOND * heads(eps * ph * g.clamp_min(0) + ph * d_g).mean(1) + (h_n + 3) * U * cam + SUB32
    ref = dict(probs=ph, dprobs=g, cam=cam)
    bnd = dict(probs=eps * ph + 2 * U * ph + SUB32, dprobs=d_g + 2 * U * g.abs() + SUB32, cam=b_cam)
    return dict(ref=ref, bound=bnd, row=(eps * ph).sum(-1) + (lk + 4) * U)


def terms(c):
    return _cached(c, "terms", _terms)


def ref64(c):
    return terms(c)["ref"]


def bound(c):
    return terms(c)["bound"]


def row_bound(c):
    return terms(c)["row"]


def worst_ratio(c, outputs):
    """{output name: max |out - ref| / bound} and "rowsum" (NaN counts as inf)."""
    ref, bnd = ref64(c), bound(c)
    w = {n: float(((o.double() - ref[n]).abs() / bnd[n]).nan_to_num(nan=math.inf).max()) for n, o in outputs.items()}
    if "probs" in outputs:
        w["rowsum"] = float(((outputs["probs"].double().sum(-1) - 1).abs() / row_bound(c)).nan_to_num(nan=math.inf).max())
    return w


def check(c, outputs):
    """Compare `outputs` {probs, dprobs: (N, Lq, Lk) in attn_bwd_cases' items layout; cam: (G, Lq, Lk)} (CPU tensors) with ref64 within
    bound, every element; and every row of probs sums to 1 within row_bound.  -> list of failures (empty = pass)."""
    ref, bnd = ref64(c), bound(c)
    assert set(outputs) == set(OUTPUTS), set(outputs)
    fails = []
    for name, out in outputs.items():
        rf, b = ref[name], bnd[name]
        if tuple(out.shape) != tuple(rf.shape):
            fails.append(f"{c} {name}: shape {tuple(out.shape)} != {tuple(rf.shape)}")
            continue
        err = (out.double() - rf).abs()
        bad = ~(err <= b)                                           # NaN lands here
        if bool(bad.any()):
            ratio = (err / b).nan_to_num(nan=math.inf).flatten()
            j = int(torch.where(bad.flatten(), ratio, torch.zeros(())).argmax())
            fails.append(f"{c} {name}: {int(bad.sum())} of {out.numel()} elements outside the bound; worst error / bound {float(ratio[j]):.3g} "
                         f"at flat index {j}: got {out.flatten()[j].item()!r} ref {rf.flatten()[j].item()!r} bound {b.flatten()[j].item():.3e}")
    if tuple(outputs["probs"].shape) == tuple(ref["probs"].shape):
        rs = (outputs["probs"].double().sum(-1) - 1).abs()
        bad = ~(rs <= row_bound(c))
        if bool(bad.any()):
            fails.append(f"{c} rowsum: {int(bad.sum())} rows of probs do not sum to 1; worst |sum - 1| / bound {float((rs / row_bound(c)).max()):.3g}")
    return fails


# ================================================================================================ the CPU stand-in
CORRECT = ("kernel",)
WRONG = ("no_unscale", "natural_lse", "mask_dropped", "g_from_k", "relu_after_mean", "no_head_mean", "sat_row_unhandled")


def emulate(c, variant="kernel"):
    """The kernels in torch fp32, in the layout `check` takes: the forward's lse is attn_cases.emulate_core(.., "plain")'s.
      kernel              the kernels as they are
    Wrong forms (each wrong in value only):
      no_unscale          dprobs and cam without dmul (the loss scale stays in the gradient)
      natural_lse         the lse taken for a natural-log one (multiplied by ln 2 before it is subtracted)
      mask_dropped        the recomputation leaves the key mask out
      g_from_k            G = dO K^T
      relu_after_mean     cam = max(mean_h P dP, 0)
      no_head_mean        cam = sum_h, not the mean
      sat_row_unhandled   a group under a saturated mask gets exp2(s + mask - lse) like any other"""
    assert variant in CORRECT + WRONG, variant
    dm = dmul(c)
    i = B.inputs(c)
    lq, lk = c.shape
    g_n, h_n, _ = B.layout(c)
    mask = i["mask"]
    f32 = lambda z: torch.tensor(z, dtype=torch.float32)            # noqa: E731
    lse = A.emulate_core(i["q"], i["k"], i["v"], mask, c.dt, "plain")["lse"]
    qf, kf, vf, dof = (i[n].float() for n in ("q", "k", "v", "do"))
    sl = f32(SCALE) * f32(LOG2E)
    sub = lse * f32(LN2) if variant == "natural_lse" else lse
    cc = -sub[:, :, None]
    if mask is not None and variant != "mask_dropped":
        cc = (mask.float().clamp_min(B.KERNEL_CLAMP) * f32(LOG2E))[:, None, :] - sub[:, :, None]
    x = qf @ kf.transpose(1, 2) * sl + cc
    if mask is not None and variant != "sat_row_unhandled":
        row_sat = (lse == f32(B.KERNEL_CLAMP) * f32(LOG2E))[:, :, None]
        x = torch.where(row_sat, -torch.log2(f32(float(lk))).expand_as(x), x)
    p = torch.exp2(x)
    g = dof @ (kf if variant == "g_from_k" else vf).transpose(1, 2)
    dp = g if variant == "no_unscale" else g * f32(dm)
    heads = lambda z: z.view(g_n, h_n, lq, lk)                      # noqa: E731
    if variant == "relu_after_mean":
        cam = heads(p * dp).sum(1).clamp_min(0) * (f32(1.0) / h_n)
    else:
        cam = heads(p * dp.clamp_min(0)).sum(1)
        if variant != "no_head_mean":
            cam = cam * (f32(1.0) / h_n)
    return dict(probs=p, dprobs=dp, cam=cam)
