"""Case table, float64 reference, a-priori ELEMENTWISE error bounds and a CPU stand-in for the fused training attention, forward and
recomputing backward: cir_attention_train_fwd / cir_attention_train_bwd (train_attn.hip: tattn_fwd_kernel, tattn_bwd_dq_kernel,
tattn_bwd_dkv_kernel) - the conventions of tests/attn_cases.py, whose dialled inputs, `core_terms` and `emulate_core` are reused.

A plain module, imported by tests/test_attn_bwd_cases_cpu.py (the stand-in `emulate`: every correct form passes every comparison, every
wrong form fails on named cases) and by tests/test_attn_bwd_gpu.py (the kernels themselves).

            CASES                the list of `Case`s: ONE forward and ONE backward launch each,
            inputs(case)         the CPU tensors of the case (operands and dO already rounded to the operand type; the dropout mask),
            ref64(case)          {out, out32, lse, dq, dk, dv: float64 tensor} from the rounded operands,
            bound(case)          the same names: the elementwise error bound,
            check(case, outputs) -> list of failure messages (empty = pass); worst_ratio(case, outputs) -> {name: max error / bound},
            emulate(case, variant) -> outputs of a torch fp32 model of the three kernels.

Cases
--------------------------------------------------------------------------------------------------------------------------------
Inputs: attn_cases._inputs (the key column 0 carries the item's profile AND a common offset of up to 33: the situation the centre
correction of tattn_bwd_dq_kernel exists for); dO = 0.5 randn rounded to the operand type, seeded from the case.  Shapes (Lq, Lk):
(1, 1) a single element | (9, 9) one ragged tile each way | (32, 32) exact tiles: the dQ kernel's `edge == false` branch when unmasked |
(33, 100) a ragged second tile each way | (64, 65) one key in the last key tile, full query tiles | (70, 197) several tiles, the ViT's
key count.  Axes: bf16 / fp16; the masks of attn_cases wherever they mask something and leave something (tail, min_tail: Lk > 7;
front: Lk > 32), tail40, all10k (-10000 on EVERY key of the odd profiles' items, what an all-zero encoder mask produces) and min_all
(p = 0) at (33, 100); p_drop 0 and 0.1 everywhere, 0.25 at (33, 100); the FORM of the backward call: t16 = fp32 twin of O, gradients in the
operand type (the ViT trainer's call: the full table) | t32 = twin, fp32 gradients | n32 = no twin, fp32 gradients (both on every
shape at one mask per dtype).  `items = sub7`: profiles 1..7 with ONE head - G H nqt = 14 at (33, 100) and 7 units for all three
kernels at (9, 9), so the last workgroup has idle waves.  `do = loss`: dO times the power of two that brings max |dO| into
[256, 512), where the trainers' loss scale aims (fp16).  The dropout mask is helpers.pair_keep(seed, N Lq, Lk, p) with row =
(g H + h) Lq + query; two seeds, one with a non-zero high word.

Reference (float64, from the rounded operands)
--------------------------------------------------------------------------------------------------------------------------------
w_ij = keep_ij / (1 - p) (p as the fp32 number the kernels get; 1 at p = 0); P^ = the softmax of attn_cases.core_terms (mask clamped at
-1e30); Pd = P^ w; O = Pd V; D_i = sum_d dO_id O_id; G_ij = sum_d dO_id v_jd; dS_ij = P^_ij (w_ij G_ij - D_i);
dQ = scale dS K, dK = scale dS^T Q, dV = Pd^T dO; lse as in attn_cases (it does not depend on the dropout).  sum_j dS_ij = 0.

What the kernels compute (read from train_attn.hip)
--------------------------------------------------------------------------------------------------------------------------------
forward: attn_cases' online softmax rescaled on every tile, with rnd16(p_j keep_j / (1 - p)) at the RUNNING reference in the numerator.
backward, both kernels: p = exp2(fma(s, scale log2e, c)), c = mask log2e - lse_fwd; pd16 = rnd16(p w); ds = pd16 G' - pf D' with
pf = pd16 (1 - p) for a kept element, else p (p = 0: ds = pd16 (G' - D')); ds16 = rnd16(ds); D' = sum_d dO O from the fp32 twin of O, or
from the 16-bit O when no twin is passed;
    dQ = scale (sum_j ds16_j k_j - (sum_j ds16_j / sum_j pd16_j) sum_j pd16_j k_j),  dK = scale sum_i ds16_i q_i,  dV = sum_i pd16_i dO_i.

How the bound is made (u = 2^-24; first order, elementwise; no constant below is fitted to what a kernel returns)
--------------------------------------------------------------------------------------------------------------------------------
* Forward under dropout: core_terms' bound with Pd in the numerator terms and 3 u more on a numerator weight when p > 0 (1 - p, its
  reciprocal, the product with it):  b32 = SECOND [ (Pd (eps_f + r_f + 3u)) |V| + |O| sum_j P^ eps_f + (Pd |V|) (2 Lk + 4 nkt + 7) u ].
  At p = 0 this IS core_terms' b32.
* Backward weight error eps_ij (relative error of p against P^).  Score error e_s in log2 units: the dot product 66 u scale log2e
  sum_d |q k|; scale log2e formed in fp32 and multiplied on 3 u |s|; c: log2e rounded u |mask log2e|, the FMA's result u |mask log2e -
  lse|; the exponent's FMA u |x - lse|; the forward's own lse error b_lse of the row (attn_cases).  eps = ln2 e_s + 5 u: 2 u GRANTED to
  v_exp_f32 as in attn_cases, 2 u for 1 / (1 - p), u for the product with it.  eps = 1 where lse - x > 125 (p may be flushed; P^ < 2^-125).
  A SATURATED key (mask <= -1e30) is treated as in attn_cases: beside any other key its weight is exactly 0 in both evaluations; in a
  row of saturated keys only, its e_s is that of the kernels' exp2(-log2 Lk) (the last paragraph).
* 16-bit rounding, r = 2^-8 bf16, 2^-11 fp16.  Whether fp16 subnormals survive is unmeasured, so the bound holds either way:
  r_P = 1 where a kept element has Pd < 2^-14 (1 + 2^-7) (a dropped one is exactly 0);  e1 = eps + r_P is the relative error of pd16.
* dG_ij = 66 u sum_d |dO_id v_jd|;  dD_i = sum_d |dO_id| b_O,id + 66 u sum_d |dO_id O_id| with b_O the forward bound of out32 when the
  twin is passed and of the 16-bit out (its rounding included) otherwise.
* Element error before the rounding of dS.  The kernels' ds FACTORISES: a kept element is pd16 (G' - (1 - p) D'), a dropped one
  -p D', at p = 0 pd16 (G' - D') - the one rounded weight multiplies both terms, so its error e1 (eps for a dropped element) acts on
  dS = Pd (G - D / w) itself, not on |G| and |D| apart (which would let a row with G ~ D, every peaked row, hide 2^-8 |G|):
      e_pre = ((e1 if kept else eps) + 4 u) |dS| + 3 u P^ |D| + Pd dG + P^ dD
  (4 u: the subtraction and the FMA's result; 3 u: 1 - p in fp32 and the products pd16 (1 - p), pf D').  An unrounded p inside dS
  (`p32_in_ds`) factorises the same way.  This is tighter than bounding the two products apart and holds for every correct stand-in.
  Rounding: r_S = 1 where |dS| - e_pre < 2^-14 in fp16 (the COMPUTED value may lie below the normal range), else r; the rounding acts on
  the computed value:  e_ij = e_pre + r_S (|dS| + e_pre) + 2^-25 (half a subnormal spacing of fp16).
* dQ.  sum_j dS_j = 0, so the exact dQ equals sum_j dS_j (k_j - kappa') for the kernel's own centre kappa', and the error of the
  corrected sum is sum_j (ds16_j - dS_j)(k_j - kappa').  kappa_i = sum_j Pd_ij k_j / sum_j Pd_ij in float64, 0 for a row whose every
  element was dropped (the kernel applies no correction there; dS = 0 on such a row).  The kernel's centre is made of pd16:
      |kappa' - kappa|_id <= dk_id = sum_j Pd e1 |k_jd - kappa_id| / (sum_j Pd (1 - E_i)),  E_i = sum_j Pd e1 / sum_j Pd,
  usually a 2^-8 of the keys' spread - but a row whose peak was DROPPED keeps only weights below fp16's normal range (r_P = 1, E_i ~ 1):
  its sum of pd16 may be anything down to 0 (then no correction), and kappa' is only known to be 0 or inside the hull of the keys:
  dk_id = |kappa_id| + max_j |k_jd| where E_i >= 1/2 (and never more than that).  Accumulation: the products sum_j ds16 k_j and the
  row sum of ds16 (which multiplies kappa') in fp32, (Lk + 4) u each on the sums of magnitudes:
      b(dQ_id) = scale SECOND [ sum_j e_ij (|k_jd - kappa_id| + dk_id) + (Lk + 4) u sum_j (|dS_ij| + e_ij) (|k_jd| + |kappa_id| + dk_id) ]
                 + 4 u |dQ_id|.
* dK:  scale SECOND [ sum_i e_ij |q_id| + (Lq + 2) u sum_i (|dS_ij| + e_ij) |q_id| ] + 4 u |dK_jd|.
* dV:  SECOND [ sum_i Pd_ij e1_ij |dO_id| + (Lq + 2) u sum_i Pd_ij |dO_id| ] + 2 u |dV_jd|.
* Output rounding: glue_cases.out_bound in the gradient's type (fp32 gradients: one subnormal).
* SECOND = 1 + 2^-4 as in attn_cases; `second_order_ok` returns E = sum_j P^ (eps + r_P) per row and the CPU file asserts E <= 0.05.

Every key under finfo.min (`min_all`, at (33, 100)): in fp32 every score IS the clamped mask, the rows are uniform, and the forward's
lse = m + log2 l is the kernels' clamp -2e38 log2e itself (the scores and log2 l are absorbed).  The reference clamps at -1e30 and yields
the same uniform P^; only the lse of such a row shows the clamp, so its reference is the kernels' clamp times log2e (+ log2 Lk) with
2 u |lse| around it.  The backward cannot rebuild P from that lse by exp2(s + mask - lse) - this table found dQ NaN there - and now
recognises the group by it (train_attn.hip, kSatLse): p = exp2(-log2 Lk), whose error 2 u (log2 Lk + 6) is the e_s of a saturated key.
"""
import math

import torch

from tests import attn_cases as A
from tests import helpers
from tests.attn_cases import BF16, DT_NAME, F16, F32, GAINS, LN2, LOG2E, PREC, PROFILES, SCALE, SECOND, U, Case, case_id, out_bound  # noqa: F401

SHAPES = ((1, 1), (9, 9), (32, 32), (33, 100), (64, 65), (70, 197))
SEEDS = (0x5EED1234, 0x1234567800C0FFEE)            # the second has a non-zero high 32-bit word (drop_row_key folds it in)
FORMS = {"t16": (True, True), "t32": (True, False), "n32": (False, False)}      # form: (fp32 twin of O passed, 16-bit gradients)
OUTPUTS = ("out", "out32", "lse", "dq", "dk", "dv")
H = A.H
KERNEL_CLAMP = -2.0e38                               # the kernels clamp the mask here (the reference at -1e30): only the lse of a saturated row shows it
SUB7 = tuple(range(1, 8))                           # the profiles of an `items = sub7` case (one head each)


def masks_at(lk):
    return ["none"] + (["tail"] if lk > 7 else []) + (["front"] if lk > 32 else []) + (["min_tail"] if lk > 7 else [])


def _cases():
    out = []
    for s in SHAPES:
        for dt in (BF16, F16):
            for m in masks_at(s[1]) + (["tail40", "all10k"] if s == (33, 100) else []):
                for p in (0.0, 0.1) + ((0.25,) if s == (33, 100) and m in ("none", "tail") else ()):
                    out.append(Case("train_bwd", shape=s, dt=dt, mask=m, p=p, form="t16"))
    for form in ("t32", "n32"):
        for s in SHAPES:
            for dt in (BF16, F16):
                m = "tail" if dt == BF16 and s[1] > 7 else "none"
                out += [Case("train_bwd", shape=s, dt=dt, mask=m, p=p, form=form) for p in (0.0, 0.1)]
    for dt in (BF16, F16):
        out.append(Case("train_bwd", shape=(33, 100), dt=dt, mask="tail", p=0.1, form="t16", items="sub7"))
        out.append(Case("train_bwd", shape=(9, 9), dt=dt, mask="none", p=0.1, form="t16", items="sub7"))
    out += [Case("train_bwd", shape=(33, 100), dt=F16, mask="none", p=p, form="t16", do="loss") for p in (0.0, 0.1)]
    out += [Case("train_bwd", shape=(33, 100), dt=dt, mask="min_all", p=0.0, form="t16") for dt in (BF16, F16)]
    return out


CASES = _cases()


def case(cid):
    return next(c for c in CASES if c.id == cid)


def layout(c):
    """(G, H) of the launch and the items (index into attn_cases' NP * H items) it carries."""
    if getattr(c, "items", "all") == "sub7":
        return len(SUB7), 1, [p * H for p in SUB7]
    return A.NP, H, list(range(A.NP * H))


def seed_of(c):
    return SEEDS[(SHAPES.index(c.shape) + (c.dt == F16)) % 2]


def p32(c):
    """p_drop as the fp32 number the kernels receive."""
    return float(torch.tensor(c.p, dtype=torch.float32))


# ================================================================================================ inputs
def _inputs(c):
    """q (N, Lq, 64), k, v (N, Lk, 64), do (N, Lq, 64) in the operand type; mask (N, Lk) per item and mask_g (G, Lk) per group, fp32 or None;
    keep (N, Lq, Lk) bool; item n = group * H + head."""
    lq, lk = c.shape
    g, h, idx = layout(c)
    base = Case("train_bwd", shape=c.shape, dt=c.dt, mask=c.mask)          # q, k, v, dO do not depend on p, the form or the item subset
    i = A._inputs(base)
    mask = i["mask"]
    if c.mask == "all10k":
        mask = torch.zeros((A.NP, lk), dtype=torch.float32)
        mask[1::2] = -10000.0
    q, k, v = (i[n][idx] for n in ("q", "k", "v"))
    gen = torch.Generator(device="cpu").manual_seed(base.seed ^ 0xD0)
    do = (torch.randn((A.NP * H, lq, 64), generator=gen, dtype=torch.float64) * 0.5)[idx]
    if getattr(c, "do", None) == "loss":
        do = do * 2.0 ** math.ceil(math.log2(256.0 / float(do.to(c.dt).abs().max())))
    n = g * h
    keep = helpers.pair_keep(seed_of(c), n * lq, lk, c.p).view(n, lq, lk) if c.p > 0 else torch.ones((n, lq, lk), dtype=torch.bool)
    groups = sorted({j // H for j in idx})
    return dict(q=q, k=k, v=v, do=do.to(c.dt), keep=keep, mask=None if mask is None else mask[[j // H for j in idx]],
                mask_g=None if mask is None else mask[groups].contiguous())


_last = {}


def _cached(c, key, fn):
    if _last.get("case") is not c:
        _last.clear()
        _last["case"] = c
    if key not in _last:
        _last[key] = fn(c)
    return _last[key]


def inputs(case):
    return _cached(case, "inputs", _inputs)


# ================================================================================================ reference and bound
def _terms(c):
    """Everything of the module docstring: dict(ref {name: float64}, bound {name: float64}, e (N, Lq), ds_max, g_max, p, pd)."""
    i = inputs(c)
    lq, lk = c.shape
    nkt = (lk + 31) // 32
    twin, g16 = FORMS[c.form]
    gdt = c.dt if g16 else F32
    q, k, v, do = (i[n].double() for n in ("q", "k", "v", "do"))
    mask, keep = i["mask"], i["keep"]
    t = A.core_terms(i["q"], i["k"], i["v"], mask, c.dt)
    ph, eps_f, r_f, x, sat, lse, b_lse = t["p"], t["eps"], t["r"], t["x"], t["sat"], t["lse"], t["b_lse"]
    if mask is not None:                                                                # a row whose EVERY key is saturated: the kernels' lse is their clamp
        all_sat = sat.all(-1)
        lse = torch.where(all_sat, mask.double().clamp_min(KERNEL_CLAMP).max(-1).values[:, None] * LOG2E + math.log2(lk), lse)
        b_lse = torch.where(all_sat, 2 * U * lse.abs(), b_lse)
    w = keep.double() / (1.0 - p32(c))
    pd = ph * w
    # ---- forward
    o = pd @ v
    pe = (ph * eps_f).sum(-1, keepdim=True)
    b_o = SECOND * ((pd * (eps_f + r_f + (3 * U if c.p > 0 else 0.0))) @ v.abs() + o.abs() * pe + (pd @ v.abs()) * ((2 * lk + 4 * nkt + 7) * U))
    # ---- backward: the weights
    sl = SCALE * LOG2E
    s = q @ k.transpose(1, 2) * sl
    e_s = 66 * U * sl * (q.abs() @ k.abs().transpose(1, 2)) + 3 * U * s.abs()
    if mask is not None:
        m2 = mask.double().clamp_min(-1e30)[:, None, :] * LOG2E
        e_s = e_s + U * m2.abs() + U * (m2 - lse[:, :, None]).abs()
    e_s = e_s + U * (x - lse[:, :, None]).abs() + b_lse[:, :, None]
    e_s = torch.where(sat, torch.full_like(e_s, 2 * U * (math.log2(lk) + 6)), e_s)       # (a saturated ROW: p = exp2(-log2 Lk), the logarithm's error)
    eps = LN2 * e_s + 5 * U
    eps = torch.where(lse[:, :, None] - x > 125, torch.ones_like(eps), eps)
    r = 2.0 ** -PREC[c.dt]
    r_p = torch.full_like(eps, r)
    if c.dt == F16:
        r_p = torch.where(keep & (pd < 2.0 ** -14 * (1 + 2.0 ** -7)), torch.ones_like(r_p), r_p)      # (a dropped element is exactly 0)
    e1 = eps + r_p
    # ---- backward: the element
    g = do @ v.transpose(1, 2)
    d_g = 66 * U * (do.abs() @ v.abs().transpose(1, 2))
    d = (do * o).sum(-1)
    b_out = out_bound(o, b_o, F32 if twin else c.dt)
    d_d = (do.abs() * b_out).sum(-1) + 66 * U * (do * o).abs().sum(-1)
    ds = ph * (w * g - d[:, :, None])
    e_pre = (torch.where(keep, e1, eps) + 4 * U) * ds.abs() + 3 * U * ph * d.abs()[:, :, None] + pd * d_g + ph * d_d[:, :, None]
    r_s = torch.full_like(eps, r)
    if c.dt == F16:
        r_s = torch.where(ds.abs() - e_pre < 2.0 ** -14, torch.ones_like(r_s), r_s)
    e = e_pre + r_s * (ds.abs() + e_pre) + 2.0 ** -25
    a = ds.abs() + e
    # ---- gradients
    dq = SCALE * (ds @ k)
    dk = SCALE * (ds.transpose(1, 2) @ q)
    dv = pd.transpose(1, 2) @ do
    psum = pd.sum(-1, keepdim=True)
    kappa = torch.where(psum > 0, (pd @ k) / psum.clamp_min(1e-300), torch.zeros_like(dq))
    e_pd = (pd * e1).sum(-1, keepdim=True) / psum.clamp_min(1e-300)                       # relative error of sum_j pd16_j
    centred, d_kappa = [], []
    for n in range(q.shape[0]):                                                          # (Lq, Lk, 64) per item, never for all items at once
        dev = (k[n][None, :, :] - kappa[n][:, None, :]).abs()
        centred.append(torch.einsum("ij,ijd->id", e[n], dev))
        d_kappa.append(torch.einsum("ij,ijd->id", pd[n] * e1[n], dev))
    anywhere = kappa.abs() + k.abs().max(1, keepdim=True).values                         # kappa' is 0 or inside the hull of the keys
    d_kappa = torch.where(e_pd < 0.5, torch.stack(d_kappa) / (psum * (1 - e_pd.clamp_max(0.5))).clamp_min(1e-300), anywhere)
    d_kappa = torch.where(psum > 0, torch.minimum(d_kappa, anywhere), torch.zeros_like(anywhere))
    b_dq = SCALE * SECOND * (torch.stack(centred) + d_kappa * e.sum(-1, keepdim=True)
                             + (lk + 4) * U * (a @ k.abs() + (kappa.abs() + d_kappa) * a.sum(-1, keepdim=True))) + 4 * U * dq.abs()
    b_dk = SCALE * SECOND * (e.transpose(1, 2) @ q.abs() + (lq + 2) * U * (a.transpose(1, 2) @ q.abs())) + 4 * U * dk.abs()
    b_dv = SECOND * ((pd * e1).transpose(1, 2) @ do.abs() + (lq + 2) * U * (pd.transpose(1, 2) @ do.abs())) + 2 * U * dv.abs()
    ref = dict(out=o, out32=o, lse=lse, dq=dq, dk=dk, dv=dv)
    bnd = dict(out=out_bound(o, b_o, c.dt), out32=out_bound(o, b_o, F32), lse=b_lse + 2.0 ** -149,
               dq=out_bound(dq, b_dq, gdt), dk=out_bound(dk, b_dk, gdt), dv=out_bound(dv, b_dv, gdt))
    return dict(ref=ref, bound=bnd, e=torch.maximum(t["e"], (ph * (eps + r_p)).sum(-1)), ds_max=float(ds.abs().max()),
                g_max=float(g.abs().max()), p=ph, pd=pd)


def terms(case):
    return _cached(case, "terms", _terms)


def ref64(case):
    return terms(case)["ref"]


def bound(case):
    return terms(case)["bound"]


def second_order_ok(case):
    """E per row, forward (attn_cases) and backward (with r_P): SECOND covers E <= 0.05."""
    return terms(case)["e"]


def worst_ratio(case, outputs):
    """{output name: max |out - ref| / bound} (NaN counts as inf)."""
    ref, bnd = ref64(case), bound(case)
    return {n: float(((o.double() - ref[n]).abs() / bnd[n]).nan_to_num(nan=math.inf).max()) for n, o in outputs.items()}


def check(case, outputs):
    """Compare `outputs` {name: CPU tensor in the items layout (N, L, 64) / (N, Lq)} with ref64(case) within bound(case): every element
    of every output, no share of mismatches allowed.  -> list of failures (empty = pass)."""
    ref, bnd = ref64(case), bound(case)
    assert set(outputs) == set(OUTPUTS), set(outputs)
    idx = layout(case)[2]
    fails = []
    for name, out in outputs.items():
        rf, b = ref[name], bnd[name]
        if tuple(out.shape) != tuple(rf.shape):
            fails.append(f"{case} {name}: shape {tuple(out.shape)} != {tuple(rf.shape)}")
            continue
        err = (out.double() - rf).abs()
        bad = ~(err <= b)                                           # NaN lands here
        if bool(bad.any()):
            ratio = (err / b).nan_to_num(nan=math.inf).flatten()
            j = int(torch.where(bad.flatten(), ratio, torch.zeros(())).argmax())
            n = j // (out.numel() // out.shape[0])
            fails.append(f"{case} {name}: {int(bad.sum())} of {out.numel()} elements outside the bound; worst error / bound {float(ratio[j]):.3g} "
                         f"at flat index {j} (item {n}, profile {PROFILES[idx[n] // H]}): got {out.flatten()[j].item()!r} "
                         f"ref {rf.flatten()[j].item()!r} bound {b.flatten()[j].item():.3e}")
    return fails


# ================================================================================================ the CPU stand-in
CORRECT = ("kernel", "ftz", "p32_in_ds")
WRONG = ("no_centre", "mask_shift", "drop_last", "pad_query", "pad_key", "dkv_row_slip", "dq_col_parity", "dropped_no_D", "dk_scale_twice",
         "grad16_cols")
OTHER_FORM = ("no_twin_as_twin",)                   # not wrong: the no-twin form's D under a twin case (test_attn_bwd_cases_cpu.py)


def emulate(case, variant="kernel"):
    """The three kernels in torch fp32, in the layout `check` takes.  The forward is attn_cases.emulate_core(.., "plain") with the
    dropout weights (P keep / (1 - p) rounded at the RUNNING reference); the backward recomputes p from that forward's lse, once for the
    dQ side and once for the dK / dV side, each with its own copy of the dropout mask so that the two can be made to disagree.
    Correct variants (the bound holds for each):
      kernel            the kernels as they are
      ftz               fp16 values of pd16 and ds16 below 2^-14 flushed to zero
      p32_in_ds         the unrounded p inside dS (pd16 still feeds dV and the centre)
    Wrong variants (each wrong in value only):
      no_centre         corr = 0: dQ = scale sum_j ds16_j k_j (the defect test_training_attention_backward_profiles found)
      mask_shift        the backward reads the mask one key late
      drop_last         the last key never enters the backward
      pad_query         the clamped copy of row Lq - 1 is counted once more in dK and dV (ragged Lq)
      pad_key           the clamped copy of key Lk - 1 is counted once more in dQ (ragged Lk)
      dkv_row_slip      the dK / dV side's dropout mask is one row late inside the last query tile
      dq_col_parity     the dQ side takes the other half of a column pair in the last key tile
      dropped_no_D      a dropped element contributes dS = 0 instead of -p D
      dk_scale_twice    the softmax scale is applied twice to dK
      grad16_cols       the 16-bit gradient store swaps the two 32-column halves
    `no_twin_as_twin` forms D from the 16-bit O whatever the form of the case: the no-twin computation under a twin case's bound."""
    assert variant in CORRECT + WRONG + OTHER_FORM, variant
    i = inputs(case)
    lq, lk = case.shape
    dt = case.dt
    twin, g16 = FORMS[case.form]
    mask, keep = i["mask"], i["keep"]
    f32 = lambda z: torch.tensor(z, dtype=torch.float32)                                          # noqa: E731
    drop = case.p > 0
    keepw, ikeep = 1.0 / (1.0 - f32(case.p)), 1.0 - f32(case.p)
    fwd = A.emulate_core(i["q"], i["k"], i["v"], mask, dt, "plain", w=keep.float() * keepw if drop else None)
    out32, lse = fwd["out32"], fwd["lse"]
    out16 = out32.to(dt)
    qf, kf, vf, dof = (i[n].float() for n in ("q", "k", "v", "do"))
    sl = f32(SCALE) * f32(LOG2E)
    c = -lse[:, :, None]
    if mask is not None:
        mk = mask.float()
        if variant == "mask_shift":
            mk = torch.cat([mk[:, :1] * 0, mk[:, :-1]], 1)
        c = (mk.clamp_min(-2.0e38) * f32(LOG2E))[:, None, :] - lse[:, :, None]
    x = qf @ kf.transpose(1, 2) * sl + c
    if mask is not None:                                            # the group's every key at the clamp: lse is the clamp itself, p = 1 / Lk
        row_sat = (lse == f32(KERNEL_CLAMP) * f32(LOG2E))[:, :, None]
        x = torch.where(row_sat, -torch.log2(f32(float(lk))).expand_as(x), x)
    p = torch.exp2(x)
    g = dof @ vf.transpose(1, 2)
    d = (dof * (out32 if twin and variant != "no_twin_as_twin" else out16.float())).sum(-1)[:, :, None]

    def side(kp):
        if drop:
            pw = p * torch.where(kp, keepw, f32(0.0))
            pd16 = pw.to(dt).float()
            pf = torch.where(kp, pd16 * ikeep, torch.zeros_like(p) if variant == "dropped_no_D" else p)
            ds = pw * g - p * d if variant == "p32_in_ds" else pd16 * g - pf * d
        else:
            pd16 = p.to(dt).float()
            ds = (p if variant == "p32_in_ds" else pd16) * (g - d)
        ds16 = ds.to(dt).float()
        if variant == "ftz" and dt == F16:
            pd16 = torch.where(pd16.abs() < 2.0 ** -14, torch.zeros_like(pd16), pd16)
            ds16 = torch.where(ds16.abs() < 2.0 ** -14, torch.zeros_like(ds16), ds16)
        if variant == "drop_last":
            pd16[:, :, -1] = 0.0
            ds16[:, :, -1] = 0.0
        return pd16, ds16

    # ---- dQ side
    kq = keep
    if variant == "dq_col_parity":
        j = torch.arange(lk)
        swapped = torch.where((j >= (lk - 1) // 32 * 32) & ((j ^ 1) < lk), j ^ 1, j)
        kq = keep[:, :, swapped]
    pd16, ds16 = side(kq)
    kx = kf
    if variant == "pad_key" and lk % 32:
        pd16, ds16, kx = torch.cat([pd16, pd16[:, :, -1:]], 2), torch.cat([ds16, ds16[:, :, -1:]], 2), torch.cat([kf, kf[:, -1:]], 1)
    esum, psum = ds16.sum(-1, keepdim=True), pd16.sum(-1, keepdim=True)
    corr = torch.where(psum > 0, esum / psum.clamp_min(1e-38), torch.zeros_like(esum))
    if variant == "no_centre":
        corr = torch.zeros_like(corr)
    dq = (ds16 @ kx - corr * (pd16 @ kx)) * f32(SCALE)
    # ---- dK / dV side
    kk = keep
    if variant == "dkv_row_slip":
        q0 = (lq - 1) // 32 * 32
        rows = torch.arange(lq)
        kk = keep[:, torch.where((rows >= q0) & (rows > 0), rows - 1, rows)]
    pd16, ds16 = side(kk)
    qx, dox = qf, dof
    if variant == "pad_query" and lq % 32:
        pd16, ds16, qx, dox = (torch.cat([z, z[:, -1:]], 1) for z in (pd16, ds16, qf, dof))
    dk = ds16.transpose(1, 2) @ qx * f32(SCALE)
    if variant == "dk_scale_twice":
        dk = dk * f32(SCALE)
    dv = pd16.transpose(1, 2) @ dox
    grads = [z.to(dt) if g16 else z for z in (dq, dk, dv)]
    if variant == "grad16_cols" and g16:
        grads = [torch.cat([z[..., 32:], z[..., :32]], -1) for z in grads]
    return dict(out=out16, out32=out32, lse=lse, dq=grads[0], dk=grads[1], dv=grads[2])
