"""Case tables, float64 references and a-priori error bounds for the optimizer step of csrc/train_optim.hip: cir_adamw_step_dev and
cir_adamw_step (one AdamW update), cir_adamw_begin (the step count and the bias corrections) and cir_grads_check (the unscale and the
finite test), and for the Python around them (train_optim.AdamW, train_core.loss_scale).

A plain module in the style of tests/glue_cases.py and tests/rowpass_cases.py, whose `Case`, `U`, `SUB32`, `half_ulp`, `check` and
`worst_ratio` it uses.  Imported by tests/test_optim_cases_cpu.py (two correct fp32 stand-ins pass every case, twelve wrong update rules
and seven wrong finite checks fail on a named case) and by tests/test_optim_gpu.py (the kernels through their wrappers).

    CASES["adamw_dev"], CASES["adamw"]   the update kernels' cases;  inputs(case), ref64(case), bound(case), check(case, outputs),
    worst(case, outputs);  step_terms(p, g, m, v, hp, t, form) the reference and the bound on ANY fp32 state (the chained run and the
    `AdamW` class test call it);  GC_* and gc_* the table of cir_grads_check.

The reference.  ONE AdamW step (torch.optim.AdamW's rule: decoupled decay, no amsgrad) in float64 from the fp32 p, g, m, v:
    m' = b1 m + (1 - b1) g        v' = b2 v + (1 - b2) g^2        bc1 = 1 - b1^t        bc2 = 1 - b2^t
    p' = p (1 - lr wd) - lr (m' / bc1) / (sqrt(v' / bc2) + eps)
with the five scalars lr, b1, b2, eps, wd FIRST ROUNDED TO fp32, because the C entry points take floats: the kernels never see the
doubles.  torch.optim.AdamW computes its corrections from the double betas, so it is not this reference: float32(0.999) =
0.99900001287..., and 1 - float32(0.999) differs from 1e-3 by 1.3e-5 RELATIVE - that is the deviation of bc2 at t = 1, and it falls with t
(6.4e-6 at t = 2, 1.3e-6 at t = 10, below 1e-9 from t = 1000 on; for b1 = 0.9: 2.4e-7 at t = 1).  Through the square root it moves the
update by up to 6.4e-6 relative, a hundred times the bound below; torch with the fp32-rounded scalars as Python floats IS this reference
(tests/test_optim_cases_cpu.py runs both and shows the first leaving the bound at t = 1).  Outputs: p', m', v' and bc1, bc2.

The bound (u = 2^-24; elementwise, first order in u, then times 1 + 2^-10 for the second order; nothing is fitted to a kernel's output)
--------------------------------------------------------------------------------------------------------------------------------
Every operation also has a floor of ONE fp32 subnormal spacing (SUB32 = 2^-149: a result that underflows gradually is off by at most half
of it), written "+ s" below.
* m'.  In the kernels' form the worst term, (1 - b1) g, passes three roundings (the constant, the product, the sum); in torch's form,
  m + (1 - b1)(g - m), the difference, the constant, the product and the sum are four roundings of values no larger than
  A = |b1 m| + |(1 - b1) g| (b1 >= 1/2):
      e_m = 4 u A + 3 s.
* v'.  Both terms are non-negative, so the error is relative: (1 - b2) g g passes the constant, two products and the sum, and one more
  is granted to an implementation that rounds g^2 and 1 - b2 separately before a scaled accumulation:
      e_v = 5 u v' + 4 s.
* bc1, bc2.  The device form (cir_adamw_begin) evaluates 1 - pow(b, t) in double and rounds once: r = u, relative.  The host form
  (cir_adamw_step) calls powf, which gets the 16 ulp the OpenCL C table grants pow (as glue_cases.py grants erff 16 u), and then goes
  through the cancellation 1 - x with one more rounding:   r = (16 u b^t + s) / bc + u.   (float)t is exact below 2^24.
* mhat = m' / bc1, vhat = v' / bc2: the division gets 2 u (granted, not measured; the device division need not be correctly rounded):
      e_mhat = e_m / bc1 + |mhat| (r1 + 2 u) + s          e_vhat = e_v / bc2 + vhat (r2 + 2 u) + s.
* S = sqrt(vhat): the root gets 2 u (granted likewise).  |sqrt(x) - sqrt(a)| = |x - a| / (sqrt(x) + sqrt(a)), which for x >= a - e is at
  most e / (sqrt(a) + sqrt(max(a - e, 0))) - e / (2 sqrt(a)) to first order - and never more than sqrt(e): below a zero or tiny vhat the
  error of the root is the ROOT of the absolute error, not a relative one:
      e_S = min(e_vhat / (S + sqrt(max(vhat - e_vhat, 0))), sqrt(e_vhat)) + 2 u S + s.
* D = S + eps (eps is an input, exact): e_D = e_S + u D + s.   Q = mhat / D: e_Q = e_mhat / D + |Q| (e_D / D + 2 u) + s.
  The update U = lr Q: e_U = lr e_Q + u |U| + s + s / D.  The kernels form (lr mhat) / D: the same roundings in another order, but the
  floor of the product lr mhat then stands BEFORE the division and is magnified by 1 / D (up to 1 / eps): with a subnormal m' and
  lr = 2e-5 the product is a subnormal with two significant bits.  s / D is at most 2^-149 / eps = 1.4e-37.
* The decayed parameter W = p (1 - lr wd): the product lr wd, the difference and the product with p are three roundings of at most
  u |p| each (lr wd <= 1), and the form p - (lr wd) p has as many; e_W = 4 u |p| covers both with one to spare.
* p' = W - U:   e_p = e_W + e_U + u |p'| + s.
A contraction into FMA removes roundings and never adds one.  What a correct fp32 implementation leaves of this (measured on the CPU with
600 regimes x 3 hyperparameter sets x 5 step counts, overflowing rows left out): a numpy fp32 transcription of the kernel with the
corrections from the same float64 formula stays at or below 0.35 of the bound on p', torch's single-tensor CPU AdamW given the
fp32-rounded betas does the same, and on m' and v' the largest ratio is 0.44.  Those figures belong to the sketch of the bound, taken
before this table existed; what the same two stand-ins leave on THIS table is printed by tests/test_optim_cases_cpu.py (which asserts
that it is at most 1) and recorded in LABNOTES section 28, next to the kernels' ratios.

Inputs.  Every element of a launch is independent, so ONE vector carries every regime; a regime is the product of
    |g| in 0, 1e-30, 1e-20, 1e-12, 1e-10, 1e-8, 3e-8, 1e-6, 1e-3, 1, 1e3, 1e15, both signs (-0 too),
    the moment history: zero; steady m = g, v = g^2; collapsed m = 1e3 g, v = 1e6 g^2; spike m = 1e-3 g, v = 1e-6 g^2; flipped m = -g,
    v = g^2; fp32-subnormal m and v,
    |p| in 0, 1e-6, 1e-3, 1, 100 (the sign of p alternates over the table),
720 in all, each rounded to fp32 first.  The p = 0 and p = 1e-6 elements are where the update is resolved to full precision: there
u |p'| and 4 u |p| vanish next to the update and the bound is about ten roundings of the update itself, whereas at |p| = 1 an update of
2e-5 is seen to 2 digits only.  Hyperparameters (lr, b1, b2, eps, wd): (2e-5, 0.9, 0.999, 1e-8, 0.05), the reference's
(stage2_train.py:138); (1e-2, 0.9, 0.98, 1e-6, 0.05), the existing tests'; (0.1, 0.9, 0.999, 1e-8, 0.5), where lr wd = 0.05 makes the
order of decay and update visible.  Each also with wd = 0.  Step counts t: 1, 2, 10, 1000, 100000.

Conditions, not measurements.  No (case, element) is exempt from the bound.  The inputs of a case are the regimes whose float64
v' / bc2 and g^2 stay below 2^127 under that case's hyperparameters and t (`in_range`): fp32 must not overflow where float64 does not.
The rule drops the 1e15 x collapsed regimes at t <= 2 under b2 = 0.999 (v' / bc2 = 1e39 and 5e38) and nothing else;
test_optim_cases_cpu.py asserts the rule on every case and that those are the ones it drops.

Lengths and the index map.  adamw_dev_kernel: a block takes 512 float4, thread j the float4 j and j + 256; block 0's first threads take
the n % 4 tail.  Lengths 1, 3 (tail only), 4, 7 (one float4, a tail), 1027 (first float4 of every thread, a tail), 2048 (both), 2051 and
3 * 2048 + 1029 + 2 = 7175 (four blocks, the last with 257 float4: one thread with a second float4; a tail).  adamw_kernel: one element
per thread, lengths 1, 255, 256, 257, 1027.  The kept regimes of a case are laid through its vector with a rotation chosen so that over
the table every regime lands in a first float4, in a second float4 and in a tail (`zones`; asserted by the CPU file): a cursor walks the
regimes and every case's tail starts where the last one's ended.

cir_grads_check.  The launch rule of train_optim.hip: n4 = n / 4 float4, blocks = min(max(ceil(n4 / 1024), 1), 8192) of 256 threads,
stride = 256 blocks float4; a trip of the loop covers 4 stride float4 in four quarters u = 0..3 (float4 i + u stride), so ONE trip of
the full grid is 8192 * 256 * 4 float4 = 33 554 432 floats, and block 0 takes the n % 4 tail.  A second trip exists only beyond that, so
no short length reaches it and the table has ONE long case, GC_LONG_N: trip one complete (8 388 608 float4), of trip two the whole u = 0
quarter (2 097 152 float4) and 257 float4 of the u = 1 quarter (one whole block and one thread of the next; the u = 2 and u = 3
predicates are false for every thread), and a 3-element tail: n = 4 (8 388 608 + 2 097 152 + 257) + 3 = 41 944 071.  That is the shortest
length of this shape; a buffer that merely enters trip two would leave the u offsets inside it untested.
Values are BIT PATTERNS (GC_VALUES): +-0, the smallest and the largest subnormal, the smallest normal, +-largest finite (never flagged by
itself), +-inf, and the NaNs 0x7fc00000, 0x7f800001 (signalling), 0xffffffff.  Scales (GC_SCALES): 1 (g's bits untouched, NaN payloads
included), 2^-10 (exact), 0.3 (no power of two: the output is bit for bit the fp32 product g * float32(0.3)), 2 (the largest finite
overflows: the overflow the scaling itself makes must be flagged), 0 (inf * 0 = NaN is flagged; a finite buffer becomes zeros, unflagged).
`gc_expected` is that rule: the fp32 product, then "exponent field all ones" on the PRODUCT.  One value is planted per buffer
(`gc_positions`): first and last element, the last element of the float4 body, each tail element, one element in each non-empty u quarter.
"""
import itertools

import numpy as np
import torch

from tests.glue_cases import BF16, DT_NAME, F16, F32, SUB32, U, Case, case_id, half_ulp  # noqa: F401
from tests.glue_cases import check as _check
from tests.glue_cases import worst_ratio as _worst_ratio

HYPER = ((2e-5, 0.9, 0.999, 1e-8, 0.05), (1e-2, 0.9, 0.98, 1e-6, 0.05), (0.1, 0.9, 0.999, 1e-8, 0.5))     # lr, b1, b2, eps, wd
STEPS = (1, 2, 10, 1000, 100000)
G_ABS = (0.0, 1e-30, 1e-20, 1e-12, 1e-10, 1e-8, 3e-8, 1e-6, 1e-3, 1.0, 1e3, 1e15)
HISTORY = ("zero", "steady", "collapsed", "spike", "flipped", "subnormal")
P_ABS = (0.0, 1e-6, 1e-3, 1.0, 100.0)
DEV_LENGTHS = (1, 3, 4, 7, 1027, 2048, 2051, 3 * 2048 + 1029 + 2)
HOST_LENGTHS = (1, 255, 256, 257, 1027)
SECOND = 1.0 + 2.0 ** -10                                  # the second-order factor
LIMIT = 2.0 ** 127                                         # the range rule


def f32(v):
    return float(np.float32(v))


def hyper(case):
    """(lr, b1, b2, eps, wd) of a case as the kernels receive them: fp32 values, held in Python floats."""
    lr, b1, b2, eps, wd = HYPER[case.hp]
    return tuple(f32(x) for x in (lr, b1, b2, eps, wd if case.wd else 0.0))


# ================================================================================================ the regime table
def _regimes():
    p, g, m, v = [], [], [], []
    for (gi, ga), sign, (hi, hist), pa in itertools.product(enumerate(G_ABS), (1.0, -1.0), enumerate(HISTORY), P_ABS):
        gv = np.float64(np.float32(sign * ga))
        mv, vv = {"zero": (0.0, 0.0), "steady": (gv, gv * gv), "collapsed": (1e3 * gv, 1e6 * gv * gv), "spike": (1e-3 * gv, 1e-6 * gv * gv),
                  "flipped": (-gv, gv * gv), "subnormal": (sign * 2.0 ** -130, 3 * 2.0 ** -149)}[hist]
        p.append(pa if (gi + hi) % 2 == 0 else -pa)
        g.append(gv); m.append(mv); v.append(vv)
    return tuple(torch.tensor(np.array(x, dtype=np.float64).astype(np.float32)) for x in (p, g, m, v))


REGIMES = _regimes()                                       # fp32 (p, g, m, v), 720 long
N_REGIMES = REGIMES[0].numel()


def in_range(g, v, hp, t):
    """The range rule on fp32 g, v: float64 v' / bc2 and g^2 stay below 2^127."""
    _, _, b2, _, _ = hp
    g, v = g.double(), v.double()
    return ((b2 * v + (1.0 - b2) * g * g) / (1.0 - b2 ** t) < LIMIT) & (g * g < LIMIT)


_kept = {}


def kept(case):
    """The indices into REGIMES that a case's (hyperparameters, t) keep."""
    key = (case.hp, case.t)
    if key not in _kept:
        _kept[key] = torch.nonzero(in_range(REGIMES[1], REGIMES[3], hyper(case), case.t)).flatten()
    return _kept[key]


def regime_of(case):
    """The REGIMES index of every element of a case's vector."""
    k = kept(case)
    return k[(torch.arange(case.n) + case.rot) % k.numel()]


def zones(case):
    """{zone: the REGIMES indices that land in it}: first / second float4 of a thread of adamw_dev_kernel, the tail."""
    r, i = regime_of(case), torch.arange(case.n)
    body = i < case.n // 4 * 4
    first = body & ((i // 4) % 512 < 256)
    return dict(first=set(r[first].tolist()), second=set(r[body & ~first].tolist()), tail=set(r[~body].tolist()))


def _update_cases():
    dev, host, cursor = [], [], 0
    for p16 in (F16, BF16, None):
        for hp, wd, t, n in itertools.product(range(len(HYPER)), (1, 0), STEPS, DEV_LENGTHS):
            if p16 is None and hp != 0:                    # the form without a 16-bit copy: on the reference's hyperparameters
                continue
            c = Case("adamw_dev", hp=hp, wd=wd, t=t, n=n, p16=p16)
            c.form = "dev"
            body = n // 4 * 4
            c.rot = (cursor - body) % kept(c).numel()      # the tail starts at the cursor
            cursor += n - body
            dev.append(c)
    for i, (hp, wd, t, n) in enumerate(itertools.product(range(len(HYPER)), (1, 0), STEPS, HOST_LENGTHS)):
        c = Case("adamw", hp=hp, wd=wd, t=t, n=n)
        c.form, c.rot, c.p16 = "host", 97 * i, None
        host.append(c)
    return dict(adamw_dev=dev, adamw=host)


CASES = _update_cases()
for _k, _cs in CASES.items():
    assert len({c.id for c in _cs}) == len(_cs), _k


def inputs(case):
    """fp32 CPU tensors p, g, m, v of length n."""
    r = regime_of(case)
    return dict(zip("pgmv", (x[r].clone() for x in REGIMES)))


# ================================================================================================ the reference and the bound
def corrections(hp, t, form="dev"):
    """(bc1, bc2, r1, r2): the float64 bias corrections and the relative error granted to their fp32 values."""
    out = []
    for b in (hp[1], hp[2]):
        x = b ** t
        bc = 1.0 - x
        out.append((bc, U if form == "dev" else (16 * U * x + SUB32) / bc + U))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def step_terms(p, g, m, v, hp, t, form="dev"):
    """(ref, bound) {p, m, v, bc1, bc2: float64 tensor} of one step from the fp32 tensors p, g, m, v; `hp` the fp32-rounded scalars
    (lr, b1, b2, eps, wd) as Python floats; `form`: "dev" (cir_adamw_begin's corrections) or "host" (cir_adamw_step's powf)."""
    lr, b1, b2, eps, wd = hp
    assert all(f32(x) == x for x in hp), hp
    p, g, m, v = (x.double() for x in (p, g, m, v))
    bc1, bc2, r1, r2 = corrections(hp, t, form)
    c1, c2 = 1.0 - b1, 1.0 - b2
    m1 = b1 * m + c1 * g
    e_m = 4 * U * ((b1 * m).abs() + (c1 * g).abs()) + 3 * SUB32
    v1 = b2 * v + c2 * g * g
    e_v = 5 * U * v1 + 4 * SUB32
    mh, vh = m1 / bc1, v1 / bc2
    e_mh = e_m / bc1 + mh.abs() * (r1 + 2 * U) + SUB32
    e_vh = e_v / bc2 + vh * (r2 + 2 * U) + SUB32
    s = vh.sqrt()
    e_s = torch.minimum(e_vh / (s + (vh - e_vh).clamp_min(0.0).sqrt()), e_vh.sqrt()) + 2 * U * s + SUB32
    d = s + eps
    e_d = e_s + U * d + SUB32
    q = mh / d
    e_q = e_mh / d + q.abs() * (e_d / d + 2 * U) + SUB32
    upd = lr * q
    e_u = lr * e_q + U * upd.abs() + SUB32 + SUB32 / d
    w = p * (1.0 - lr * wd)
    p1 = w - upd
    e_p = 4 * U * p.abs() + e_u + U * p1.abs() + SUB32
    one = torch.ones((1,), dtype=torch.float64)
    ref = dict(p=p1, m=m1, v=v1, bc1=bc1 * one, bc2=bc2 * one)
    bnd = dict(p=SECOND * e_p, m=SECOND * e_m, v=SECOND * e_v, bc1=SECOND * r1 * bc1 * one, bc2=SECOND * r2 * bc2 * one)
    return ref, bnd


_last = {}


def _terms(case):
    if _last.get("case") is not case:
        i = inputs(case)
        _last.clear()
        _last.update(case=case, terms=step_terms(i["p"], i["g"], i["m"], i["v"], hyper(case), case.t, case.form))
    return _last["terms"]


def ref64(case):
    return _terms(case)[0]


def bound(case):
    return _terms(case)[1]


def _named(case, outputs):
    ref, bnd = _terms(case)
    assert {"p", "m", "v"} <= set(outputs) <= set(ref), (case, set(outputs))          # (the host form shows no corrections)
    return {n: ref[n] for n in outputs}, {n: bnd[n] for n in outputs}


def check(case, outputs):
    """glue_cases.check of {p, m, v[, bc1, bc2]} (fp32 CPU tensors) against the reference within the bound: the list of failures."""
    return _check(case, outputs, *_named(case, outputs))


def worst(case, outputs):
    """{output: max |error| / bound}."""
    ref, bnd = _named(case, outputs)
    return {n: _worst_ratio(case, {n: outputs[n]}, ref, bnd) for n in outputs}


worst_ratio = _worst_ratio


def check_state(what, outputs, p, g, m, v, hp, t, form="dev"):
    """`check` on a state that is no table case (the chained run, the `AdamW` class): outputs {p, m, v} against step_terms(...)."""
    ref, bnd = step_terms(p.flatten(), g.flatten(), m.flatten(), v.flatten(), hp, t, form)
    outs = {n: o.flatten() for n, o in outputs.items()}
    return _check(what, outs, {n: ref[n] for n in outs}, {n: bnd[n] for n in outs}), {n: _worst_ratio(what, {n: outs[n]}, ref, bnd) for n in outs}


# ================================================================================================ cir_grads_check
GC_VALUES = (                                              # (name, bit pattern, non-finite by itself)
    ("+0", 0x00000000, False), ("-0", 0x80000000, False), ("sub_min", 0x00000001, False), ("sub_max", 0x007FFFFF, False),
    ("norm_min", 0x00800000, False), ("+max", 0x7F7FFFFF, False), ("-max", 0xFF7FFFFF, False), ("+inf", 0x7F800000, True),
    ("-inf", 0xFF800000, True), ("qnan", 0x7FC00000, True), ("snan", 0x7F800001, True), ("nan_ones", 0xFFFFFFFF, True))
GC_SCALES = (("one", 1.0), ("2^-10", 2.0 ** -10), ("0.3", 0.3), ("two", 2.0), ("zero", 0.0))
GC_LENGTHS = DEV_LENGTHS
GC_CAP = 8192                                              # the largest grid of the launch rule
GC_TRIP = GC_CAP * 256 * 4 * 4                             # floats in one trip of the full grid: 33 554 432
GC_LONG_N4 = GC_TRIP // 4 + GC_CAP * 256 + 257
GC_LONG_N = 4 * GC_LONG_N4 + 3                             # 41 944 071
assert GC_TRIP == 33554432 and GC_LONG_N == 41944071


def gc_grid(n, cap=GC_CAP):
    """(n4, blocks, stride in float4) of cir_grads_check's launch."""
    n4 = n // 4
    blocks = min(max(-(-n4 // 1024), 1), cap)
    return n4, blocks, blocks * 256


def gc_quarter_of(n, cap=GC_CAP):
    """(trip, u) of every body element, -1 for the tail: which trip of the loop and which of its four loads reads it."""
    n4, _, stride = gc_grid(n, cap)
    f = np.arange(n, dtype=np.int64) // 4
    trip, u = f // (4 * stride), f % (4 * stride) // stride
    tail = np.arange(n) >= 4 * n4
    return np.where(tail, -1, trip), np.where(tail, -1, u)


def gc_positions(n, cap=GC_CAP):
    """{name: element} where the one special value of a buffer is planted."""
    n4 = gc_grid(n, cap)[0]
    pos = {"first": 0, "last": n - 1}
    if n4:
        pos["body_last"] = 4 * n4 - 1
    for k in range(n - 4 * n4):
        pos[f"tail{k}"] = 4 * n4 + k
    trip, u = gc_quarter_of(n, cap) if n < 1 << 22 else (None, None)
    if trip is not None:
        for tr, q in sorted({(int(a), int(b)) for a, b in zip(trip, u) if a >= 0}):
            idx = np.nonzero((trip == tr) & (u == q))[0]
            pos[f"trip{tr}_u{q}"] = int(idx[len(idx) // 2 + (q + 1) % 4 if len(idx) > 4 else 0])      # (mid-quarter, another float4 lane per quarter)
    return pos


def gc_base(n, seed=0):
    """A finite fp32 buffer whose products with every scale of the table stay finite and mostly inexact: +-[2^-20, 2^20)."""
    g = torch.Generator(device="cpu").manual_seed(1000 + n + seed)
    return (torch.randn((n,), generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())).float()


def gc_buffer(n, pos, bits):
    """The base buffer with the bit pattern `bits` planted at element `pos`, as int32 bits (a NaN payload survives no float copy)."""
    b = gc_base(n).view(torch.int32).clone()
    b[pos] = int(np.array(bits, dtype=np.uint32).view(np.int32))
    return b


def gc_expected(bits, scale):
    """(the int32 bits cir_grads_check leaves, the flag it ORs in) for a buffer given as int32 bits: scale == 1 writes nothing; otherwise
    the fp32 product with float32(scale); the flag is "exponent field all ones" anywhere in the RESULT."""
    a = bits.numpy().view(np.float32)
    with np.errstate(all="ignore"):
        out = a if f32(scale) == 1.0 else (a * np.float32(scale)).astype(np.float32)
    ob = out.view(np.uint32)
    return torch.from_numpy(out.view(np.int32).copy()), int(bool(((ob & 0x7F800000) == 0x7F800000).any()))


def gc_same(got_bits, want_bits, scale):
    """Bit equality of two int32 buffers; under a scale other than 1 a NaN need only be a NaN where one is expected (the payload of a
    product is the hardware's), under scale 1 the payload is part of the comparison."""
    if f32(scale) == 1.0:
        return bool(torch.equal(got_bits, want_bits))
    g, w = got_bits.view(torch.float32), want_bits.view(torch.float32)
    nan = w != w
    return bool(torch.equal(g != g, nan)) and bool(torch.equal(got_bits[~nan], want_bits[~nan]))


def gc_check(what, bits, scale, got_bits, got_flag, preset=0):
    """The ONE comparison of cir_grads_check both suites apply: the buffer `bits` (int32) under `scale` must become gc_expected's bits
    and the flag must be `preset` OR gc_expected's.  Returns the list of failures."""
    want_bits, flag = gc_expected(bits, scale)
    fails = []
    if not gc_same(got_bits, want_bits, scale):
        bad = got_bits != want_bits
        fails.append(f"{what}: {int(bad.sum())} of {bits.numel()} elements are not the fp32 product (first at {int(bad.nonzero()[0])})")
    if int(got_flag) != (preset | flag):
        fails.append(f"{what}: flag {int(got_flag)}, expected {preset | flag}")
    return fails
