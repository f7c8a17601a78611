"""Case tables, float64 references and a-priori error bounds for the LayerNorm family and the row passes of the training step:
cir_layernorm (ops.layernorm), cir_residual_layernorm_train, cir_layernorm_bwd, cir_layernorm_bwd_fused (plain and ordered forms),
cir_rows16_colsum (both modes, strided views, ordered form) and cir_rows_scale_add.

A plain module in the style of tests/glue_cases.py, whose `Case`, `half_ulp`, `out_bound`, `round_once`, `check` and `worst_ratio` it uses.
Imported by tests/test_rowpass_cases_cpu.py (fp32 stand-ins written with torch's CPU operators: the correct ones pass every comparison,
seventeen wrong ones fail on a named case) and by tests/test_rowpass_gpu.py (the kernels through their wrappers).

For every kernel:  CASES[kernel], inputs(case), ref64(case) {output: float64 tensor}, bound(case) {output: float64 tensor or None = bit for
bit}, check(case, outputs) -> list of failures, worst(case, outputs) -> {output: max |error| / bound}.

Inputs.  Every row operand of a case (x, residual, t0, t1, a, b) is drawn from the case's seed as one of eight ROW KINDS (s = randn):
randn 2 s + 0.3; vit 1.5 s + 0.3 with channel 5 raised by 320 and channel cols - 3 lowered by 200 (the outlier channels of a ViT residual
stream; at widths below 8 the nearest channels); offset100 0.5 s + 50; offset1000 0.5 s + 500; const 3.7; zero; onehot 7.0 in column 1;
tiny 1e-5 s.  dy and t_add are randn, gamma = 1 + 0.5 s, beta = 0.5 s.  Every input is rounded to its storage type first (eps to fp32
too) and the reference - the operation as include/cirrank.h states it - is evaluated in float64 on the stored values.  The dropout keep
mask is tests.helpers.pair_keep.  dgamma, dbeta, the bias gradients and the column sums start from 0.25.

How the bounds are made (u = 2^-24; first order in u, then DOUBLED - the convention of glue_cases.py for its LayerNorm bound; no constant
is tuned to a kernel's output)
--------------------------------------------------------------------------------------------------------------------------------
* The row entering the statistics.  cir_layernorm: pre = x (+ residual), e_pre = u |pre| with a residual (one fp32 addition), 0 without.
  cir_residual_layernorm_train: s = t0 (+ t1: u |s|), tv = s alpha k on kept positions with k = 1 / (1 - p) formed in fp32 (p, 1 - p, the
  division, the product: 4 u |tv|, as glue_cases.py has it; the product with alpha: u |tv|), pre = tv + residual (u |pre|):
      e_pre = alpha k u |s| [t1] + 5 u |tv| + u |pre|      at kept positions;  0 at dropped ones (pre IS the residual there).
* LayerNorm forward over n columns, y = d r g + b with m = mean(pre), d = pre - m, q = mean(d^2), r = (q + eps)^-1/2, a = mean |pre|:
      e_m = (n + 3) u a + mean(e_pre)                     (n - 1 additions and the division, any order)
      e_d = e_pre + e_m + u |d|
      e_q = mean(2 |d| e_d + e_d^2) + (n + 3) u q         (the e_d^2 term is kept: on constant rows d = 0 and it is all there is)
      e_r = e_q / (2 (q + eps)) + 3 u                     (relative; rsqrt 2 u, the addition of eps)
      |dy| <= |g| r e_d + |d r g| (e_r + 3 u) + u |y|
  and a 16-bit or fp16-stream output adds half an ulp of its format at the result (`out_bound`), rounded from the fp32 value.
* The adjoint, from the saved fp32 row x (no input error), gq = dy g, xh = d r, A = mean(gq), B = mean(gq xh),
  dx = r (gq - A - xh B):
      e_d  = (n + 3) u mean|x| + u |d|
      e_q  = mean(2 |d| e_d + e_d^2) + (n + 3) u q
      e_r  = e_q / (2 (q + eps)) + 3 u
      e_xh = r e_d + |xh| (e_r + u)
      e_A  = (n + 3) u mean|gq|
      e_B  = mean(|gq| e_xh) + (n + 4) u mean|gq xh|
      e_t  = u |gq| + e_A + |B| e_xh + |xh| e_B + 3 u (|gq| + |A| + |xh B|)
      |ddx| <= r e_t + |dx| (e_r + 2 u)
      dgamma (R rows, into the starting value g0)   sum_rows |dy| e_xh + D u (sum |dy xh| + |g0|)
      dbeta                                         D u (sum |dy| + |b0|)
  D, the depth of a column sum.  A sum of R + 1 terms in ANY order is off by at most (R + 2) u sum|terms|; at 2100 rows that alone is
  2 to 3 % of the largest dgamma of the vit and onehot rows, where one channel carries the sum.  The header fixes more than "any order":
  a workgroup sums the rows of ITS block (32 rows: cir_layernorm_bwd[_fused], 64 rows: cir_rows16_colsum) and the blocks are then added
  to the destination.  With any order inside a block and any order across the blocks no term passes through more than
      D = min(R, block) + ceil(R / block) + 3
  additions (the term's own product and the starting value included): 101 instead of 2103 at 2100 rows.  The stand-ins of the CPU file
  sum the same way (blocks first), in two different orders.
* dt = alpha k (dx + t_add) on kept positions, 0 on dropped ones (bit for bit: bound 0):
      e_s = e_dx + u |dx + t_add| [t_add]
      e_dt = alpha k e_s + 5 u |dt|                        (4 u the dropout scaling, u the product with alpha)
  dt16 adds half an ulp of the 16-bit format at the result; the bias gradients are the column sums of the fp32 dt into b0:
      sum_rows e_dt + D u (sum |dt| + |b0|).
* cir_rows16_colsum.  mode 0: sums = s0 + sum_rows a, the 16-bit a converted exactly: D u (sum |a| + |s0|).  mode 1:
  out = a gelu'(z) with the gelu' terms of glue_cases.py (`gelu_bwd_terms`, not doubled there and not here) and one 16-bit rounding;
  sums = s0 + sum_rows of the fp32 products: sum_rows (their bound) + D u (sum |out| + |s0|).
* cir_rows_scale_add.  out = a + sc b: u |sc b| + u |out| (two roundings, or one when contracted into an FMA).  With `a` absent the
  one fp32 product is correctly rounded, which the float64 product rounded once reproduces bit for bit - for every scale, 0 and 1 included.

Exact expectations (bound None): zero rows give y = beta (rounded once to the output type), pre = 0, 0 * gelu'(z) = 0, sums = the
starting value, a + sc b = 0; with p = 0, alpha = 1 and no t1 pre = round_once(t0 + residual); cir_rows_scale_add without `a`.  Exact
positions inside a bounded output (bound 0): dropped positions of pre (the residual) and of dt16 (0).

Two choices in the tables that follow from the formats and the bounds, not from any kernel.  (1) On zero and const rows
|dx| reaches eps^-1/2 |dy| = 10^3 .. 10^6, beyond the largest fp16 number (65504) once the dropout scale joins: their dt16 is bf16 -
except in four added cases at eps 1e-6 without dropout, where |dt| <= 10^3 |dy gamma| + |t_add| fits fp16 and fp16 is compared.
(2) The adjoint tables leave out ONE (kind, shape) pair, offset1000 at 2100 x 768: the any-order bound of a row mean near 500,
(n + 3) u 500 = 0.023 against a spread of 0.5, enters dgamma once per row, so that term grows like R while dgamma grows like sqrt(R) and
beyond about 1000 rows the bound exceeds the reference.  offset1000 runs at the five smaller shapes, 2100 x 768 with the other seven kinds.

Exclusions.  An output of a case leaves the bounded comparison only when the largest bound exceeds the largest magnitude of its own
reference - a bound that large says nothing.  That happens on `const` rows alone, where q = 0 and r = eps^-1/2 multiplies the rounding
error of the mean: `EXCLUDED` lists the pairs, test_rowpass_cases_cpu.py asserts that the rule gives exactly that list, that every pair
is of kind const and that pre, dbeta and the column sums of cir_rows16_colsum are never in it.  An excluded output must still be finite.
"""
import itertools

import numpy as np
import torch

from tests import helpers as H
from tests.glue_cases import BF16, DT_NAME, F16, F32, SUB32, U, Case, case_id, gelu_bwd_terms, half_ulp, out_bound, round_once  # noqa: F401
from tests.glue_cases import check as _check
from tests.glue_cases import worst_ratio as _worst_ratio

KINDS = ("randn", "vit", "offset100", "offset1000", "const", "zero", "onehot", "tiny")
SHAPES = ((1, 4), (33, 132), (5, 260), (203, 768), (70, 1024), (2100, 768))      # 5 x 260: one active lane in chunk 2; 2100 rows: 66 blocks of 32
SHAPES8 = ((1, 8), (33, 136), (5, 264), (203, 768), (70, 1024), (2100, 768))     # the next legal widths where cols % 8 == 0 is required
EPS = (1e-12, 1e-6)                                                              # BERT, ViT
P_DROP = (0.0, 0.1, 0.9)
START = 0.25                                                                     # what every accumulated output holds before the launch
GUARDED_SHAPES = ((5, 260), (5, 264), (2100, 768), (70, 776))                    # the GPU file puts canaries around these


def f32(v):
    return float(np.float32(v))


def drop_seed(c):
    return (0x5EED << 32) ^ c.seed                                               # both halves of the 64-bit seed in use


def rows_of(kind, rows, cols, g):
    s = torch.randn((rows, cols), generator=g)
    if kind == "randn":
        return 2.0 * s + 0.3
    if kind == "vit":
        x = 1.5 * s + 0.3
        x[:, min(5, cols - 1)] += 320.0
        x[:, cols - 3] -= 200.0
        return x
    if kind == "offset100":
        return 0.5 * s + 50.0
    if kind == "offset1000":
        return 0.5 * s + 500.0
    if kind == "const":
        return torch.full((rows, cols), 3.7)
    if kind == "zero":
        return torch.zeros((rows, cols))
    if kind == "onehot":
        x = torch.zeros((rows, cols))
        x[:, 1] = 7.0
        return x
    assert kind == "tiny", kind
    return 1e-5 * s


def _affine(g, cols, lead=()):
    return 1.0 + 0.5 * torch.randn(lead + (cols,), generator=g), 0.5 * torch.randn(lead + (cols,), generator=g)


def _keep(c, rows, cols):
    """(keep mask, k = 1 / (1 - p) on the fp32 p) of the fused kernels' dropout."""
    p = f32(c.p)
    if p == 0.0:
        return torch.ones((rows, cols), dtype=torch.bool), 1.0
    return H.pair_keep(drop_seed(c), rows, cols, p), 1.0 / (1.0 - p)


# ================================================================================================ shared terms
def ln_fwd_terms(pre, e_pre, gamma, beta, eps):
    """(y, first-order-doubled fp32 bound) of LayerNorm(pre) on float64 operands; e_pre bounds the fp32 row's own error."""
    n = pre.shape[-1]
    m = pre.mean(-1, keepdim=True)
    d = pre - m
    q = (d * d).mean(-1, keepdim=True)
    r = (q + eps) ** -0.5
    y = d * r * gamma + beta
    e_m = (n + 3) * U * pre.abs().mean(-1, keepdim=True) + e_pre.mean(-1, keepdim=True)
    e_d = e_pre + e_m + U * d.abs()
    e_q = (2 * d.abs() * e_d + e_d * e_d).mean(-1, keepdim=True) + (n + 3) * U * q
    e_r = e_q / (2 * (q + eps)) + 3 * U
    return y, 2.0 * (gamma.abs() * r * e_d + (d * r * gamma).abs() * (e_r + 3 * U) + U * y.abs())


def depth(rows, block):
    """The additions a term of a column sum passes through at most: its workgroup's rows (any order), the workgroups (any order), the
    starting value; and the rounding of the term itself.
    `block` - 32 rows for cir_layernorm_bwd[_fused], 64 for cir_rows16_colsum, as the callers pass it - is the rows-per-workgroup that
    include/cirrank.h states for these operators (with the ordered forms, "as cir_layernorm_bwd does" for the plain ones) and must follow
    that header: a kernel that sums other blocks needs the header changed first, and then these two constants."""
    return min(rows, block) + -(-rows // block) + 3


def ln_bwd_terms(x, gamma, dy, eps):
    """dx, dgamma / dbeta (without the starting value) and their first-order bounds (NOT yet doubled), float64."""
    rows, n = x.shape
    m = x.mean(-1, keepdim=True)
    d = x - m
    q = (d * d).mean(-1, keepdim=True)
    r = (q + eps) ** -0.5
    xh = d * r
    gq = dy * gamma
    a = gq.mean(-1, keepdim=True)
    b = (gq * xh).mean(-1, keepdim=True)
    dx = r * (gq - a - xh * b)
    e_d = (n + 3) * U * x.abs().mean(-1, keepdim=True) + U * d.abs()
    e_q = (2 * d.abs() * e_d + e_d * e_d).mean(-1, keepdim=True) + (n + 3) * U * q
    e_r = e_q / (2 * (q + eps)) + 3 * U
    e_xh = r * e_d + xh.abs() * (e_r + U)
    e_a = (n + 3) * U * gq.abs().mean(-1, keepdim=True)
    e_b = (gq.abs() * e_xh).mean(-1, keepdim=True) + (n + 4) * U * (gq * xh).abs().mean(-1, keepdim=True)
    e_t = U * gq.abs() + e_a + b.abs() * e_xh + xh.abs() * e_b + 3 * U * (gq.abs() + a.abs() + (xh * b).abs())
    e_dx = r * e_t + dx.abs() * (e_r + 2 * U)
    return dict(dx=dx, e_dx=e_dx, dgamma=(dy * xh).sum(0), e_dgamma=(dy.abs() * e_xh).sum(0) + depth(rows, 32) * U * ((dy * xh).abs().sum(0) + START),
                dbeta=dy.sum(0), e_dbeta=depth(rows, 32) * U * (dy.abs().sum(0) + START))


def _sum_into_start(ref, e1):
    """An accumulated fp32 output: the reference with the starting value, the doubled bound."""
    return START + ref, 2.0 * e1 + SUB32


# ================================================================================================ cir_layernorm
def _flags(i, n):
    """n binary flags from the case counter, each with its own period (1, 2, 3, 5, 7 ...): every value of each meets every kind and shape."""
    return [(i // per) % 2 for per in (1, 2, 3, 5, 7, 11)[:n]]


def _layernorm_cases():
    out = []
    for i, (kind, si) in enumerate(itertools.product(KINDS, range(6))):
        res, twin, half16, e = _flags(i, 4)
        for xdt, shape, sdts, dt16s, r, t, ee in ((F32, SHAPES[si], (F32, F16, None), (BF16, F16, None), res, twin, e),
                                                  (F16, SHAPES8[si], (F16, F32, None), (F16, None, BF16), 1 - res, half16, 1 - e)):
            sdt, dt16 = sdts[i % 3], dt16s[(i // 3 + i) % 3]
            out.append(Case("layernorm", kind=kind, shape=shape, xdt=xdt, sdt=xdt if sdt is None and dt16 is None else sdt, dt16=dt16,
                            res=r, twin=t, eps=EPS[ee]))             # (one of the two outputs must exist)
    out += [Case("layernorm", kind=k, shape=s, xdt=F16, sdt=F16, dt16=BF16, res=1, twin=0, eps=1e-6)        # fp16 rows whose width is no multiple
            for k, s in (("randn", (33, 132)), ("vit", (5, 260)))]                                            # of 8: the four-per-lane kernel
    return out


def _layernorm_inputs(c):
    g, (rows, cols) = c.gen(), c.shape
    lead = (2,) if c.twin else ()
    i = dict(x=rows_of(c.kind, rows, cols, g).to(c.xdt), residual=None)
    if c.res:
        # the twin form: one residual PER BRANCH, (2, rows, cols) - the launch then carries a non-zero residual batch stride
        i["residual"] = torch.stack([rows_of(c.kind, rows, cols, g) for _ in range(2)]).to(c.xdt) if c.twin else rows_of(c.kind, rows, cols, g).to(c.xdt)
    i["gamma"], i["beta"] = _affine(g, cols, lead)
    return i


def _layernorm_terms(c):
    i = inputs(c)
    pre = i["x"].double()
    e_pre = torch.zeros_like(pre)
    if c.res:
        pre = pre + i["residual"].double()
        e_pre = U * pre.abs()
    gamma, beta = i["gamma"].double(), i["beta"].double()
    if c.twin:
        gamma, beta = gamma[:, None, :], beta[:, None, :]
        pre, e_pre = pre.expand((2,) + tuple(c.shape)), e_pre.expand((2,) + tuple(c.shape))
    y, b32 = ln_fwd_terms(pre, e_pre, gamma, beta, f32(c.eps))
    ref, bnd = {}, {}
    for name, dt in (("stream", c.sdt), ("y16", c.dt16)):
        if dt is not None:
            ref[name] = y
            bnd[name] = None if c.kind == "zero" else out_bound(y, b32, dt)
    return ref, bnd


# ================================================================================================ cir_residual_layernorm_train
def _res_ln_cases():
    out = []
    for i, (kind, si) in enumerate(itertools.product(KINDS, range(6))):
        t1, alpha, e, want32 = _flags(i, 4)
        out.append(Case("res_ln_train", kind=kind, shape=SHAPES[si], eps=EPS[e], p=P_DROP[(i + i // 6) % 3], alpha=(1.0, 0.5)[alpha], t1=t1,
                        dt16=(BF16, F16)[(i // 2 + i // 6) % 2], want32=max(want32, int(kind == "zero"))))
    return out


def _res_ln_inputs(c):
    g, (rows, cols) = c.gen(), c.shape
    i = dict(t0=rows_of(c.kind, rows, cols, g), t1=rows_of(c.kind, rows, cols, g) if c.t1 else None, residual=rows_of(c.kind, rows, cols, g))
    i["gamma"], i["beta"] = _affine(g, cols)
    return i


def res_ln_pre(c, i):
    """(pre, e_pre first order, keep mask) in float64."""
    keep, k = _keep(c, *c.shape)
    s = i["t0"].double() + (i["t1"].double() if c.t1 else 0.0)
    alpha = f32(c.alpha)
    tv = torch.where(keep, s * alpha * k, torch.zeros_like(s))
    pre = tv + i["residual"].double()
    e_pre = torch.where(keep, (alpha * k * U * s.abs() if c.t1 else 0.0) + 5 * U * tv.abs() + U * pre.abs(), torch.zeros_like(s))
    return pre, e_pre, keep


def _res_ln_terms(c):
    i = inputs(c)
    pre, e_pre, keep = res_ln_pre(c, i)
    y, b32 = ln_fwd_terms(pre, e_pre, i["gamma"].double(), i["beta"].double(), f32(c.eps))
    zero = c.kind == "zero"
    exact_pre = zero or (c.p == 0.0 and c.alpha == 1.0 and not c.t1)
    ref = dict(pre=pre, y16=y)
    bnd = dict(pre=None if exact_pre else torch.where(keep, 2.0 * e_pre + SUB32, torch.zeros_like(pre)), y16=None if zero else out_bound(y, b32, c.dt16))
    if c.want32:
        ref["y32"], bnd["y32"] = y, None if zero else out_bound(y, b32, F32)
    return ref, bnd


# ================================================================================================ cir_layernorm_bwd (+ ordered)
NO_ADJOINT = ("offset1000", (2100, 768))          # see the module docstring: the one (kind, shape) pair the adjoint tables leave out


def _ln_bwd_cases():
    out = []
    for i, (kind, si) in enumerate(itertools.product(KINDS, range(6))):
        if (kind, SHAPES[si]) == NO_ADJOINT:
            continue
        out.append(Case("ln_bwd", kind=kind, shape=SHAPES[si], eps=EPS[(i + i // 6) % 2], ordered=0))
        if (i + i // 6) % 2 == 0 or SHAPES[si][0] == 2100:
            out.append(Case("ln_bwd", kind=kind, shape=SHAPES[si], eps=EPS[(i // 2) % 2], ordered=1))
    return out


def _ln_bwd_inputs(c):
    g, (rows, cols) = c.gen(), c.shape
    i = dict(x=rows_of(c.kind, rows, cols, g), dy=torch.randn((rows, cols), generator=g))
    i["gamma"], _ = _affine(g, cols)
    return i


def _ln_bwd_terms(c):
    i = inputs(c)
    t = ln_bwd_terms(i["x"].double(), i["gamma"].double(), i["dy"].double(), f32(c.eps))
    ref, bnd = dict(dx=t["dx"]), dict(dx=2.0 * t["e_dx"] + SUB32)
    for name in ("dgamma", "dbeta"):
        ref[name], bnd[name] = _sum_into_start(t[name], t["e_" + name])
    return ref, bnd


# ================================================================================================ cir_layernorm_bwd_fused (+ ordered)
FUSED_OUT = ("both", "both", "both", "dt_only", "dx_only")        # dx and dt16 / dt16 alone (dx NULL) / dx alone (no dense branch, no bias gradient)


def _ln_bwd_fused_cases():
    out = []
    for i, (kind, si) in enumerate(itertools.product(KINDS, range(6))):
        if (kind, SHAPES[si]) == NO_ADJOINT:
            continue
        for ordered in ((0, 1) if ((i + i // 6) % 2 == 1 or SHAPES[si][0] == 2100) else (0,)):
            j = i + 3 * ordered
            t_add, alpha, e = _flags(j, 3)
            outs = FUSED_OUT[(j + j // 6) % 5]
            out.append(Case("ln_bwd_fused", kind=kind, shape=SHAPES[si], eps=EPS[e], p=P_DROP[(j + j // 6) % 3], alpha=(1.0, 0.5)[alpha], t_add=t_add,
                            nbias=0 if outs == "dx_only" else (j // 2 + j // 6) % 3, dt16=BF16 if kind in ("zero", "const") else (BF16, F16)[(j // 3) % 2], outs=outs, ordered=ordered))
    # fp16 dt16 on the degenerate rows where it still fits: eps 1e-6 and no dropout scale, |dt| <= 10^3 |dy gamma| + |t_add| < 65504
    out += [Case("ln_bwd_fused", kind=kind, shape=shape, eps=1e-6, p=0.0, alpha=1.0, t_add=1, nbias=1, dt16=F16, outs="both", ordered=ordered)
            for kind, shape, ordered in (("zero", (33, 132), 0), ("const", (33, 132), 0), ("zero", (203, 768), 1), ("const", (5, 260), 1))]
    return out


def _ln_bwd_fused_inputs(c):
    g, (rows, cols) = c.gen(), c.shape
    i = dict(x=rows_of(c.kind, rows, cols, g), dy=torch.randn((rows, cols), generator=g))
    i["gamma"], _ = _affine(g, cols)
    i["t_add"] = 0.5 * torch.randn((rows, cols), generator=g) if c.t_add else None
    return i


def _ln_bwd_fused_terms(c):
    i = inputs(c)
    rows = c.shape[0]
    t = ln_bwd_terms(i["x"].double(), i["gamma"].double(), i["dy"].double(), f32(c.eps))
    ref, bnd = {}, {}
    if c.outs != "dt_only":
        ref["dx"], bnd["dx"] = t["dx"], 2.0 * t["e_dx"] + SUB32
    for name in ("dgamma", "dbeta"):
        ref[name], bnd[name] = _sum_into_start(t[name], t["e_" + name])
    if c.outs != "dx_only":
        keep, k = _keep(c, *c.shape)
        alpha = f32(c.alpha)
        s, e_s = t["dx"], t["e_dx"]
        if c.t_add:
            s = s + i["t_add"].double()
            e_s = e_s + U * s.abs()
        dt = torch.where(keep, s * alpha * k, torch.zeros_like(s))
        e_dt = torch.where(keep, alpha * k * e_s + 5 * U * dt.abs(), torch.zeros_like(s))
        ref["dt16"], bnd["dt16"] = dt, torch.where(keep, out_bound(dt, 2.0 * e_dt, c.dt16), torch.zeros_like(s))
        for name in ("dbias", "dbias2")[:c.nbias]:
            ref[name], bnd[name] = _sum_into_start(dt.sum(0), e_dt.sum(0) + depth(rows, 32) * U * (dt.abs().sum(0) + START))
    return ref, bnd


# ================================================================================================ cir_rows16_colsum (+ ordered)
ROWS16_SHAPES = SHAPES8 + ((333, 3072), (70, 776), (70, 776))       # the last two: the halves of ONE 70 x 1552 buffer (row stride 1552)


def _rows16_cases():
    out = []
    for n, (si, mode, dti) in enumerate(itertools.product(range(len(ROWS16_SHAPES)), (0, 1), (0, 1))):
        half = si - 7 if si >= 7 else None
        ordered = (si + mode + dti) % 2
        out.append(Case("rows16_colsum", kind=KINDS[(3 * si + 2 * mode + dti) % 8], shape=ROWS16_SHAPES[si], mode=mode, dt=(BF16, F16)[dti],
                        pad=1552 - 776 if half is not None else 8 * ((si // 2 + dti) % 2) * (1 + si), half=half, ordered=ordered,
                        sums=1 if (mode == 0 or ordered) else int((si + dti) % 3 != 0)))
    return out


def _rows16_inputs(c):
    g, (rows, cols) = c.gen(), c.shape
    lo = cols * (c.half or 0)
    buf = (rows_of(c.kind, rows, cols + c.pad, g)).to(c.dt)
    zbuf = (torch.randn((rows, cols + c.pad), generator=g) * 2.5).to(c.dt)
    return dict(abuf=buf, zbuf=zbuf, a=buf[:, lo:lo + cols], z=zbuf[:, lo:lo + cols])


def _rows16_terms(c):
    i = inputs(c)
    rows = c.shape[0]
    a = i["a"].double()
    zero = c.kind == "zero"                                         # 0 * gelu'(z) and a sum of zeros are exact
    if c.mode == 0:
        return dict(sums=START + a.sum(0)), dict(sums=None if zero else 2.0 * depth(rows, 64) * U * (a.abs().sum(0) + START) + SUB32)
    y, b32 = gelu_bwd_terms(i["z"].double(), a)
    ref, bnd = dict(out=y), dict(out=None if zero else out_bound(y, b32, c.dt))
    if c.sums:
        ref["sums"], bnd["sums"] = _sum_into_start(y.sum(0), b32.sum(0) + depth(rows, 64) * U * (y.abs().sum(0) + START))
        if zero:
            bnd["sums"] = None
    return ref, bnd


# ================================================================================================ cir_rows_scale_add
RPG = {1: 1, 33: 11, 5: 1, 203: 29, 70: 35, 2100: 700}               # rows per group: 1, 3, 5, 7, 2 and 3 groups
SCALES = ("zero_one", "droppath", "randn")


def _rows_scale_add_cases():
    return [Case("rows_scale_add", kind=KINDS[(3 * si + 2 * oi + a) % 8], shape=SHAPES[si], out=o, a=a, scale=SCALES[(si + oi + a) % 3])
            for si, (oi, o), a in itertools.product(range(6), enumerate((F32, BF16, F16)), (0, 1))]


def _rows_scale_add_inputs(c):
    g, (rows, cols) = c.gen(), c.shape
    groups = rows // RPG[rows]
    pick = torch.rand((groups,), generator=g) < 0.5
    if groups > 1:
        pick[0], pick[1] = True, False
    if c.scale == "zero_one":
        sc = pick.float()
    elif c.scale == "droppath":
        sc = pick.float() / (1.0 - 0.1)
    else:
        sc = torch.randn((groups,), generator=g)
    return dict(a=rows_of(c.kind, rows, cols, g) if c.a else None, b=rows_of(c.kind, rows, cols, g), scale=sc, rows_per_group=RPG[rows])


def _rows_scale_add_terms(c):
    i = inputs(c)
    sb = i["scale"].double().repeat_interleave(i["rows_per_group"])[:, None] * i["b"].double()
    if not c.a or c.kind == "zero":
        return dict(out=sb), dict(out=None)
    y = i["a"].double() + sb
    return dict(out=y), dict(out=out_bound(y, 2.0 * U * (sb.abs() + y.abs()), c.out))


# ================================================================================================ registry
_KERNELS = {
    "layernorm": (_layernorm_cases, _layernorm_inputs, _layernorm_terms),
    "res_ln_train": (_res_ln_cases, _res_ln_inputs, _res_ln_terms),
    "ln_bwd": (_ln_bwd_cases, _ln_bwd_inputs, _ln_bwd_terms),
    "ln_bwd_fused": (_ln_bwd_fused_cases, _ln_bwd_fused_inputs, _ln_bwd_fused_terms),
    "rows16_colsum": (_rows16_cases, _rows16_inputs, _rows16_terms),
    "rows_scale_add": (_rows_scale_add_cases, _rows_scale_add_inputs, _rows_scale_add_terms),
}
CASES = {k: v[0]() for k, v in _KERNELS.items()}
for _k, _cs in CASES.items():
    assert len({c.id for c in _cs}) == len(_cs), _k
_last = {}


def _cached(case):
    if _last.get("case") is not case:
        _last.clear()
        _last.update(case=case, inputs=_KERNELS[case.kernel][1](case))
    return _last


def inputs(case):
    """The CPU tensors of a case, in their storage types (the last case asked for is kept: ref64 and bound read the same tensors)."""
    return _cached(case)["inputs"]


def _terms(case):
    c = _cached(case)
    if "terms" not in c:
        c["terms"] = _KERNELS[case.kernel][2](case)
    return c["terms"]


def ref64(case):
    return _terms(case)[0]


def bound(case):
    return _terms(case)[1]


def says_nothing(case):
    """The outputs of a case whose largest bound exceeds the largest magnitude of their own reference (the rule behind EXCLUDED)."""
    ref, bnd = _terms(case)
    return [name for name, b in bnd.items() if b is not None and float(b.max()) > float(ref[name].abs().max())]


# (kernel, case id, output), as `says_nothing` gives them; test_rowpass_cases_cpu.py::test_excluded_set holds the two together
EXCLUDED = frozenset([
    ('layernorm', 'const-1x4-xdt_f32-sdt_f32-dt16None-res0-twin0-eps1e-12', 'stream'),
    ('layernorm', 'const-33x136-xdt_f16-sdt_f32-dt16_f16-res0-twin0-eps1e-12', 'stream'),
    ('layernorm', 'const-33x136-xdt_f16-sdt_f32-dt16_f16-res0-twin0-eps1e-12', 'y16'),
    ('layernorm', 'const-5x264-xdt_f16-sdt_f16-dt16None-res1-twin0-eps1e-12', 'stream'),
    ('layernorm', 'const-203x768-xdt_f32-sdt_f32-dt16_bf16-res1-twin1-eps1e-06', 'stream'),
    ('layernorm', 'const-203x768-xdt_f32-sdt_f32-dt16_bf16-res1-twin1-eps1e-06', 'y16'),
    ('layernorm', 'const-203x768-xdt_f16-sdt_f16-dt16_f16-res0-twin1-eps1e-12', 'stream'),
    ('layernorm', 'const-203x768-xdt_f16-sdt_f16-dt16_f16-res0-twin1-eps1e-12', 'y16'),
    ('layernorm', 'const-70x1024-xdt_f16-sdt_f32-dt16None-res1-twin1-eps1e-12', 'stream'),
    ('layernorm', 'const-2100x768-xdt_f16-sdtNone-dt16_bf16-res0-twin1-eps1e-12', 'y16'),
    ('res_ln_train', 'const-1x4-eps1e-12-p0.1-alpha1.0-t10-dt16_bf16-want320', 'y16'),
    ('res_ln_train', 'const-5x260-eps1e-12-p0.0-alpha0.5-t10-dt16_f16-want321', 'y16'),
    ('res_ln_train', 'const-5x260-eps1e-12-p0.0-alpha0.5-t10-dt16_f16-want321', 'y32'),
    ('res_ln_train', 'const-2100x768-eps1e-06-p0.0-alpha1.0-t11-dt16_bf16-want321', 'y16'),
    ('res_ln_train', 'const-2100x768-eps1e-06-p0.0-alpha1.0-t11-dt16_bf16-want321', 'y32'),
    ('ln_bwd', 'const-1x4-eps1e-12-ordered0', 'dx'),
    ('ln_bwd', 'const-1x4-eps1e-12-ordered0', 'dgamma'),
    ('ln_bwd', 'const-1x4-eps1e-12-ordered1', 'dx'),
    ('ln_bwd', 'const-1x4-eps1e-12-ordered1', 'dgamma'),
    ('ln_bwd', 'const-33x132-eps1e-06-ordered0', 'dgamma'),
    ('ln_bwd', 'const-5x260-eps1e-12-ordered0', 'dx'),
    ('ln_bwd', 'const-5x260-eps1e-12-ordered0', 'dgamma'),
    ('ln_bwd', 'const-5x260-eps1e-06-ordered1', 'dgamma'),
    ('ln_bwd', 'const-203x768-eps1e-06-ordered0', 'dgamma'),
    ('ln_bwd', 'const-70x1024-eps1e-12-ordered0', 'dx'),
    ('ln_bwd', 'const-70x1024-eps1e-12-ordered0', 'dgamma'),
    ('ln_bwd', 'const-70x1024-eps1e-12-ordered1', 'dx'),
    ('ln_bwd', 'const-70x1024-eps1e-12-ordered1', 'dgamma'),
    ('ln_bwd', 'const-2100x768-eps1e-06-ordered0', 'dgamma'),
    ('ln_bwd', 'const-2100x768-eps1e-12-ordered1', 'dx'),
    ('ln_bwd', 'const-2100x768-eps1e-12-ordered1', 'dgamma'),
    ('ln_bwd_fused', 'const-1x4-eps1e-12-p0.1-alpha1.0-t_add0-nbias1-dt16_bf16-dt_only-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-1x4-eps1e-12-p0.1-alpha1.0-t_add0-nbias1-dt16_bf16-dt_only-ordered0', 'dt16'),
    ('ln_bwd_fused', 'const-1x4-eps1e-12-p0.1-alpha1.0-t_add0-nbias1-dt16_bf16-dt_only-ordered0', 'dbias'),
    ('ln_bwd_fused', 'const-33x132-eps1e-12-p0.9-alpha1.0-t_add1-nbias0-dt16_bf16-dx_only-ordered0', 'dx'),
    ('ln_bwd_fused', 'const-33x132-eps1e-12-p0.9-alpha1.0-t_add1-nbias0-dt16_bf16-dx_only-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-33x132-eps1e-06-p0.9-alpha1.0-t_add0-nbias0-dt16_bf16-both-ordered1', 'dgamma'),
    ('ln_bwd_fused', 'const-5x260-eps1e-12-p0.0-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered0', 'dx'),
    ('ln_bwd_fused', 'const-5x260-eps1e-12-p0.0-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-5x260-eps1e-12-p0.0-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered0', 'dt16'),
    ('ln_bwd_fused', 'const-5x260-eps1e-12-p0.0-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered0', 'dbias'),
    ('ln_bwd_fused', 'const-5x260-eps1e-12-p0.0-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered0', 'dbias2'),
    ('ln_bwd_fused', 'const-203x768-eps1e-06-p0.1-alpha0.5-t_add1-nbias2-dt16_bf16-both-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-203x768-eps1e-12-p0.9-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered1', 'dx'),
    ('ln_bwd_fused', 'const-203x768-eps1e-12-p0.9-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered1', 'dgamma'),
    ('ln_bwd_fused', 'const-203x768-eps1e-12-p0.9-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered1', 'dt16'),
    ('ln_bwd_fused', 'const-203x768-eps1e-12-p0.9-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered1', 'dbias'),
    ('ln_bwd_fused', 'const-203x768-eps1e-12-p0.9-alpha0.5-t_add0-nbias2-dt16_bf16-both-ordered1', 'dbias2'),
    ('ln_bwd_fused', 'const-70x1024-eps1e-06-p0.9-alpha1.0-t_add0-nbias0-dt16_bf16-both-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-2100x768-eps1e-06-p0.0-alpha1.0-t_add1-nbias0-dt16_bf16-dt_only-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-2100x768-eps1e-12-p0.1-alpha1.0-t_add0-nbias0-dt16_bf16-both-ordered1', 'dx'),
    ('ln_bwd_fused', 'const-2100x768-eps1e-12-p0.1-alpha1.0-t_add0-nbias0-dt16_bf16-both-ordered1', 'dgamma'),
    ('ln_bwd_fused', 'const-2100x768-eps1e-12-p0.1-alpha1.0-t_add0-nbias0-dt16_bf16-both-ordered1', 'dt16'),
    ('ln_bwd_fused', 'const-33x132-eps1e-06-p0.0-alpha1.0-t_add1-nbias1-dt16_f16-both-ordered0', 'dgamma'),
    ('ln_bwd_fused', 'const-5x260-eps1e-06-p0.0-alpha1.0-t_add1-nbias1-dt16_f16-both-ordered1', 'dgamma'),
])


def excluded(case):
    return [name for (k, cid, name) in EXCLUDED if k == case.kernel and cid == case.id]


def check(case, outputs):
    """glue_cases.check on the outputs that are not excluded; the excluded ones must be there, in shape and finite."""
    ref, bnd = _terms(case)
    skip = excluded(case)
    assert set(outputs) == set(ref), (case, set(outputs), set(ref))
    fails = [f"{case} {name}: excluded from the bounded comparison, but not finite" for name in skip
             if tuple(outputs[name].shape) != tuple(ref[name].shape) or not bool(torch.isfinite(outputs[name].float()).all())]
    keep = [name for name in outputs if name not in skip]
    return fails + _check(case, {n: outputs[n] for n in keep}, {n: ref[n] for n in keep}, {n: bnd[n] for n in keep})


def worst(case, outputs):
    """{output: max |error| / bound} over the bounded, non-excluded outputs (for printing next to an assertion)."""
    ref, bnd = _terms(case)
    skip = excluded(case)
    return {n: _worst_ratio(case, {n: outputs[n]}, ref, bnd) for n in outputs if n not in skip and bnd[n] is not None}
