"""Case tables, float64 references, a-priori error bounds and a CPU stand-in for the online-softmax attention kernels:
cir_attention (attn_shared_kernel / attn_stream_kernel: `softmax_tile`, the LAZY rescale; attn_f32_kernel: `softmax_plain`),
cir_cls_cross_attention (cls_xattn_kernel) and cir_attention_train_fwd (tattn_fwd_kernel) - the conventions of tests/glue_cases.py.

A plain module, imported by tests/test_attn_cases_cpu.py (the stand-in `emulate`: both correct forms pass every comparison, the obvious
wrong ones fail) and by tests/test_attn_profiles_gpu.py (the kernels themselves).

            CASES[kernel]        the list of `Case`s: ONE launch each, its items carrying the eight score profiles,
            inputs(case)         the CPU tensors of the case (operands already rounded to the operand type),
            ref64(case)          {output name: float64 tensor}: softmax(q k^T scale + mask) v in float64 from the rounded operands,
            probabilities(case)  (items, Lq, Lk) float64 p^ of that reference,
            bound(case)          {output name: float64 tensor}: the elementwise error bound,
            check(case, outputs) -> list of failure messages (empty = pass): the ONE comparison both suites apply,
            worst_ratio(case, outputs) -> {output name: max error / bound},
            emulate(case, variant) -> outputs of a torch fp32 tile-by-tile model of the kernels' online softmax.

Inputs with dialled scores (head dimension 64, scale 1/8)
--------------------------------------------------------------------------------------------------------------------------------
Per (item, head):  k[j, 0] = c_j (the item's PROFILE over the keys, in nats), k[j, 1] = 1, k[j, 2:] = 0.05 randn;
q[r, 0] = g_r / scale with the row gains g_r cycling through GAINS = (0, 1, -1, 0.5, 2, -2, 1, 0.25) (head h starts the cycle at 4 h),
q[r, 1] = randn (a per-row constant on every score: it must drop out), q[r, 2:] = 0.5 randn;  v = randn.  The score of (r, j) is
g_r c_j + const_r + noise of ~0.03 nat.  Gain 0 = a uniform row, a negative gain = the profile reversed: the rows of one 32-row tile
disagree about when their maximum grows, which is what the vote of the lazy rescale is about.
Profiles (t = j // 32, noise in [0, 1); log2 units of the final score at gain 1 except for the spikes): PROFILES below.
Mask modes (additive fp32, valid = Lk - 7 keys so that the edge lies inside a tile wherever Lk > 7; `spike_last` puts its spike on the
last VALID key): none | tail: -10000 from `valid` on | tail40: tail, and key `valid` (masked) carries +40 nats - it must keep weight 0 |
front: -10000 on keys 0..31, the first reference point comes from masked keys only | min_tail: finfo(float32).min from `valid` on |
min_all: finfo(float32).min on every key - uniform rows, like the reference.

The reference clamps the mask at -1e30 (as the fold tests do).  A key under such a SATURATED mask has, in float64 as in the kernels'
fp32, a score that IS the mask (the q.k term is absorbed: |s| < 2^-53 |mask|); among themselves saturated keys are exactly equal in
both evaluations, against any other key their weight is exactly 0 in both.  Their score error is therefore taken as 0.

How the bound is made (u = 2^-24; first order, elementwise; no constant below is fitted to what a kernel returns)
--------------------------------------------------------------------------------------------------------------------------------
Notation, per query row: x_j = (q.k_j scale + mask_j) log2 e, the score in the log2 domain the kernels work in; M = max_j x_j;
D_j = M - x_j >= 0; p^_j = 2^-D_j / sum_i 2^-D_i; out_d = sum_j p^_j v_jd; A_d = sum_j p^_j |v_jd|; nkt = ceil(Lk / 32).
The kernels form, tile by tile, p_j = exp2(x_j - m) at a running reference m, l = sum p_j, O_d = sum rnd(p_j) v_jd, and multiply l and
O by alpha = exp2(m_old - m_new) when the reference moves; out = O / l.  The reference m is ARBITRARY as long as l and O share it (the
lazy rescale relies on exactly this), so the rounding of m itself costs nothing; what costs is what follows.
* Score error e_s,j (log2 units).
    - the dot product, depth 64 (D for the CLS form), fp32 accumulation of (for 16-bit operands exact) products, any order:
      (64 + 2) u sum_d |q_d k_jd| * scale log2 e                                                                 [glue_cases: gamma_K]
    - scale log2 e is formed in fp32 (the constant, the product) and multiplied on: 3 u |s_j|, s_j the unmasked score in log2 units
    - the mask FMA: log2 e rounded (u |mask_j log2 e|) and the result rounded (u |x_j|); for a key under -10000 this is 2 u * 14427
    - the subtraction of the reference and the arguments of later alphas: u |x_j - m_0| + sum_k u |m_{k-1} - m_k|.  The references
      only grow and end at or below M, and the one a key is exponentiated at lies at most 6 (the lazy threshold) below x_j.  If
      m_0 >= x_j everything telescopes to m_last - x_j <= D_j; otherwise x_j - m_0 <= 6 and m_last - m_0 <= D_j + 6: u (D_j + 12).
* Relative error of a weight: eps_j = ln 2 * e_s,j + 2 u for the hardware exponential (v_exp_f32).  2 u is GRANTED in the spirit of the
  device square root in glue_cases.py: nobody has measured v_exp_f32's error here.  A key with D_j > 125 may vanish in fp32 (flushed
  exponential): eps_j = 1 there (its p^_j is below 2^-125).
* Rounding of P for the second product (numerator only; l sums the unrounded values): r_j = 2^-11 for fp16, 2^-8 for bf16 (half an
  ulp relative to the value, at the bottom of a binade), 0 for the fp32 kernel.
* fp16 subnormals of P: whether the conversion and the MFMA keep them has not been measured, so the bound holds either way: a key with
  D_j > 14 - 2^-7 (p^_j below 2^-14 of the row's largest, less the score error) may be lost entirely, r_j = 1.  Every other key cannot
  have been flushed whatever reference the lazy rescale used: the reference never exceeds M, so p_j >= 2^-D_j >= 2^-14.
* Accumulation: each of the two sums (Lk + 2) u; a rescale costs 2 u in the weight (alpha's exponential) and u in each sum (the
  products), at most nkt of them: 4 nkt u; the reciprocal and the final product 3 u.
* Assembled, fp32:   |d out_d| <= sum_j p^_j (eps_j + r_j) |v_jd|  +  |out_d| sum_j p^_j eps_j  +  A_d (2 Lk + 4 nkt + 7) u.
* Second order.  Exactly, out' = (out + N) / (1 + d) with N the numerator's and d the denominator's relative perturbation, so the
  first-order bound is off by 1 / (1 - |d|) times (1 + the largest elementwise eps_j + r_j of a key that is not lost), |d| <=
  E = sum_j p^_j (eps_j + r_j).  The bound is the first-order one times SECOND = 1 + 2^-4, which covers E <= 0.05 with the elementwise
  2^-8 + eps of bf16 (1.0045 / 0.95 < 1.0625); `second_order_ok` returns E per row and the CPU file asserts E <= 0.05 on every case.
* Output rounding: glue_cases.out_bound (half an ulp of the output type at |ref| + bound; fp32 outputs: one subnormal).
* lse = m + log2 l (training form, log2 domain): the weights' errors enter as their p^-weighted mean (<= max_j), the sum and the
  logarithm's argument ((Lk + 2) u + 4 u) / ln 2, the logarithm's own result 2 u (log2 Lk + 6) (l <= 64 Lk under any reference the
  kernels use) and the final sum and store 2 u |lse|:
      |d lse| <= sum_j p^_j eps_j / ln 2 + ((Lk + 2) u + 4 u) / ln 2 + 2 u (log2 Lk + 6) + 2 u |lse|.
"""
import math

import torch

from tests.glue_cases import BF16, DT_NAME, F16, F32, PREC, U, Case, case_id, half_ulp, out_bound  # noqa: F401  (re-exported for the test files)

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
SCALE = 0.125
LAZY = 6.0                                          # softmax_tile's kLazyLog2
SECOND = 1.0 + 2.0 ** -4
GAINS = (0.0, 1.0, -1.0, 0.5, 2.0, -2.0, 1.0, 0.25)
PROFILES = ("uniform", "ramp5", "ramp8", "step6", "descend", "saw", "spike_last", "spike_first")
LATE_PROFILES = ("ramp5", "ramp8", "step6", "saw", "spike_last")      # must take the late-rescale branch (test_attn_cases_cpu.py)
MASKS = ("none", "tail", "tail40", "front", "min_tail", "min_all")
FMIN = float(torch.finfo(torch.float32).min)
NP = len(PROFILES)

# cir_attention's dispatch (the end of attention.hip): nqt = ceil(Lq / 32), lk_pad = Lk rounded up to 32;
#   shared kernel iff nqt >= 2 and lk_pad <= 608 (TUNE_ATTN_SHARED_MAX = -1: never); waves = nqt (<= 16);
#   wide_store iff one round, waves * 4096 <= lk_pad * 256 and the output base / strides are multiples of 16 bytes.
ATTN_PATHS = {                                      # name: (Lq, Lk, extra output columns, forced stream kernel)
    "stream_1tile": (32, 197, 0, False),            # nqt = 1: stream kernel, one full query tile
    "stream_ragged": (5, 33, 0, False),             # nqt = 1: stream kernel, 5 rows, one key in the second tile
    "shared_wide": (70, 197, 0, False),             # 3 waves, 12 KiB <= 56 KiB: wide_store
    "shared_plain_lds": (197, 40, 0, False),        # 7 waves * 4096 > 64 * 256: plain stores
    "shared_plain_stride": (70, 100, 4, False),     # output row stride 132: a multiple of 4, not of 8: plain stores
    "shared_2rounds": (520, 100, 0, False),         # nqt = 17 > 16: two rounds, plain stores
    "stream_long": (40, 641, 0, False),             # lk_pad = 672 > 608: stream kernel, two query tiles
    "stream_forced": (70, 197, 0, True),            # TUNE_ATTN_SHARED_MAX = -1
}
F32_SHAPES = ((33, 100), (70, 197))
CLS_SHAPES = tuple((d, n) for d in (128, 768) for n in (33, 100, 197))
TRAIN_SHAPES = ((9, 9), (33, 100), (70, 197))
TRAIN_MASKS = ("none", "tail", "tail40", "front", "min_tail")
H = 2


def _cases():
    out = {"attention": [Case("attention", path=p, dt=dt, mask=m) for p in ATTN_PATHS for dt in (BF16, F16) for m in MASKS],
           "attention_f32": [Case("attention_f32", shape=s, dt=F32, mask=m) for s in F32_SHAPES for m in MASKS],
           "cls": [Case("cls", d=d, n=n, dt=dt, mask="none") for d, n in CLS_SHAPES for dt in (BF16, F16)],
           "train": [Case("train", shape=s, dt=dt, mask=m) for s in TRAIN_SHAPES for dt in (BF16, F16) for m in TRAIN_MASKS]}
    return out


CASES = _cases()


def shape(c):
    """(Lq, Lk) of a case."""
    if c.kernel == "attention":
        return ATTN_PATHS[c.path][:2]
    return (32, c.n) if c.kernel == "cls" else c.shape


def valid_keys(c):
    lk = shape(c)[1]
    return lk - 7 if c.mask in ("tail", "tail40", "min_tail") and lk > 7 else lk


def late_rescale_expected(c):
    """A 16-bit cir_attention case whose LATE_PROFILES must take softmax_tile's rescale branch behind the first key tile: at least two
    key tiles hold a valid key (5 x 33 under a tail mask keeps 26 keys: one tile) and the rows are not all uniform."""
    return c.kernel == "attention" and c.mask != "min_all" and valid_keys(c) > 32


# ================================================================================================ inputs
def profile(name, lk, valid, g):
    """c_j in nats for `lk` keys of which `valid` are unmasked."""
    t = (torch.arange(lk) // 32).double()
    noise = torch.rand((lk,), generator=g, dtype=torch.float64)
    if name == "uniform":
        return torch.zeros(lk, dtype=torch.float64)
    if name == "ramp5":
        return (5 * t + noise) / LOG2E
    if name == "ramp8":
        return (8 * t + noise) / LOG2E
    if name == "step6":
        return 6 * t / LOG2E
    if name == "descend":
        return (-9 * t + noise) / LOG2E
    if name == "saw":
        return (7 * (t % 2) + noise) / LOG2E
    c = noise.clone()
    c[valid - 1 if name == "spike_last" else 0] += 40.0
    return c


def _mask(mode, lk, valid):
    m = torch.zeros((lk,), dtype=torch.float32)
    if mode in ("tail", "tail40"):
        m[valid:] = -10000.0
    elif mode == "front":
        m[:32] = -10000.0
    elif mode == "min_tail":
        m[valid:] = FMIN
    elif mode == "min_all":
        m[:] = FMIN
    return m


def _inputs(c):
    """q (N, Lq, D), k (N, Lk, D), v (N, Lk, Dv), mask (NP, Lk) fp32 or None; item n = profile * H + head (CLS: N = NP)."""
    g, (lq, lk), valid = c.gen(), shape(c), valid_keys(c)
    cls = c.kernel == "cls"
    d, heads = (c.d, 1) if cls else (64, H)
    q = torch.randn((NP * heads, lq, d), generator=g, dtype=torch.float64) * (0.05 if cls else 0.5)
    k = torch.randn((NP * heads, lk, d), generator=g, dtype=torch.float64) * (1.0 if cls else 0.05)
    v = torch.randn((NP * heads, lk, 64), generator=g, dtype=torch.float64)
    for n in range(NP * heads):
        k[n, :, 0] = profile(PROFILES[n // heads], lk, valid, g)
        if c.mask == "tail40":
            k[n, valid, 0] += 40.0
        k[n, :, 1] = 1.0
        q[n, :, 0] = torch.tensor(GAINS, dtype=torch.float64)[(torch.arange(lq) + 4 * (n % heads)) % 8] / SCALE
        q[n, :, 1] = torch.randn((lq,), generator=g, dtype=torch.float64)
    q, k = q.to(c.dt), k.to(c.dt)
    v = k if cls else v.to(c.dt)                                    # the CLS form: the values ARE the keys (the raw tokens)
    mask = None if c.mask == "none" else _mask(c.mask, lk, valid).expand(NP, lk).contiguous()
    return dict(q=q, k=k, v=v, mask=mask)


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


def _item_mask(i, heads):
    return None if i["mask"] is None else i["mask"].repeat_interleave(heads, dim=0)       # (N, Lk)


# ================================================================================================ reference and bound
def core_terms(q, k, v, mask, dt, depth=64):
    """Everything of the module docstring for operands q (N, Lq, D), k (N, Lk, D), v (N, Lk, Dv) and mask (N, Lk) fp32 or None:
    dict(out, p, lse, b32, b_lse, e) - reference, probabilities, log2-domain log-sum-exp, the fp32 bounds, E per row."""
    q, k, v = q.double(), k.double(), v.double()
    lk = k.shape[1]
    nkt = (lk + 31) // 32
    sl = SCALE * LOG2E
    s = q @ k.transpose(1, 2) * sl                                  # unmasked scores, log2 units
    x, sat = s, torch.zeros_like(s, dtype=torch.bool)
    e_s = (depth + 2) * U * sl * (q.abs() @ k.abs().transpose(1, 2)) + 3 * U * s.abs()
    if mask is not None:
        m2 = mask.double().clamp_min(-1e30)[:, None, :] * LOG2E
        x = s + m2
        sat = (mask <= -1e30)[:, None, :].expand_as(s)
        e_s = e_s + U * m2.abs() + U * x.abs()
    big = x.max(-1, keepdim=True).values
    dj = big - x
    e_s = torch.where(sat, torch.zeros_like(e_s), e_s + U * (dj + 2 * LAZY))
    eps = LN2 * e_s + 2 * U
    eps = torch.where(dj > 125, torch.ones_like(eps), eps)
    p = torch.softmax(x * LN2, -1)
    r = torch.zeros_like(eps)
    if dt != F32:
        r = torch.full_like(eps, 2.0 ** -PREC[dt])
        if dt == F16:
            r = torch.where(dj > 14 - 2.0 ** -7, torch.ones_like(r), r)
    out = p @ v
    a = p @ v.abs()
    pe = (p * eps).sum(-1, keepdim=True)
    b32 = SECOND * ((p * (eps + r)) @ v.abs() + out.abs() * pe + a * ((2 * lk + 4 * nkt + 7) * U))
    lse = torch.logsumexp(x * LN2, -1) * LOG2E
    b_lse = pe[..., 0] / LN2 + ((lk + 2) * U + 4 * U) / LN2 + 2 * U * (math.log2(lk) + 6) + 2 * U * lse.abs()
    return dict(out=out, p=p, lse=lse, b32=b32, b_lse=b_lse, e=(p * (eps + r)).sum(-1), p_term=(p * r) @ v.abs(),
                eps=eps, r=r, x=x, sat=sat)                         # the elementwise pieces, for tests/attn_bwd_cases.py


def _terms(c):
    i = inputs(c)
    heads = 1 if c.kernel == "cls" else H
    return core_terms(i["q"], i["k"], i["v"], _item_mask(i, heads), c.dt, depth=i["q"].shape[2])


def terms(case):
    return _cached(case, "terms", _terms)


def probabilities(case):
    return terms(case)["p"]


def second_order_ok(case):
    """E = sum_j p^_j (eps_j + r_j) per row: SECOND covers E <= 0.05 (module docstring)."""
    return terms(case)["e"]


def ref64(case):
    t = terms(case)
    if case.kernel == "train":
        return dict(out=t["out"], out32=t["out"], lse=t["lse"])
    return dict(out=t["out"])


def bound(case):
    t = terms(case)
    b = dict(out=out_bound(t["out"], t["b32"], case.dt))
    if case.kernel == "train":
        b.update(out32=out_bound(t["out"], t["b32"], F32), lse=t["b_lse"] + 2.0 ** -149)
    return b


def worst_ratio(case, outputs):
    """{output name: max |out - ref| / bound} (NaN counts as inf)."""
    ref, bnd = ref64(case), bound(case)
    return {n: float(((o.double() - ref[n]).abs() / bnd[n]).nan_to_num(nan=math.inf).max()) for n, o in outputs.items()}


def check(case, outputs):
    """Compare `outputs` {name: CPU tensor in the items layout (N, Lq, Dv) / (N, Lq)} with ref64(case) within bound(case): every
    element of every output, no share of mismatches allowed.  Returns the list of failures (empty = pass)."""
    ref, bnd = ref64(case), bound(case)
    assert set(outputs) == set(ref), (set(outputs), set(ref))
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
            i = int(torch.where(bad.flatten(), ratio, torch.zeros(())).argmax())
            n = i // (out.numel() // out.shape[0])
            fails.append(f"{case} {name}: {int(bad.sum())} of {out.numel()} elements outside the bound; worst error / bound {float(ratio[i]):.3g} "
                         f"at flat index {i} (profile {PROFILES[n // (1 if case.kernel == 'cls' else H)]}): got {out.flatten()[i].item()!r} "
                         f"ref {rf.flatten()[i].item()!r} bound {b.flatten()[i].item():.3e}")
    return fails


# ================================================================================================ the CPU stand-in
CORRECT = ("lazy", "plain", "lazy_ftz")
WRONG = ("drop_last", "pad_key", "no_l_rescale", "vote_rows_only", "mask_shift", "alpha_after_move", "mask_unclamped", "p_unscaled_tail", "ge_no_move")


def emulate_core(q, k, v, mask, dt, variant="lazy", stats=None, w=None):
    """The kernels' online softmax in torch fp32: 32-key tiles, 32-row query tiles (rows past Lq repeat row Lq - 1 and VOTE, as in the
    kernels), the lazy vote with threshold 6 (`plain`: rescale on every tile), P rounded to `dt`, fp32 O and l.
    -> dict(out32 (N, Lq, Dv) fp32 before the output rounding, lse (N, Lq)); stats["late"] (N, nqt): rescales taken behind key tile 0.
    `lazy_ftz` is `lazy` with the fp16 subnormals of P flushed to zero: correct as well - the bound holds either way.
    `w` (N, Lq, Lk): the dropout weights keep / (1 - p) of tattn_fwd_kernel - they multiply P at the running reference before its
    rounding, in the numerator only (l sums the unweighted values); tests/attn_bwd_cases.py.
    Wrong variants (each wrong in value only):
      drop_last         the last valid key (Lk - 1) never enters
      pad_key           a ragged last tile lets ONE zero-filled key past Lk in (score 0, value 0)
      no_l_rescale      alpha multiplies O but not l
      vote_rows_only    only the rows that voted are rescaled, the reference of every row moves
      mask_shift        the mask is read one key late (mask[j - 1] for key j)
      alpha_after_move  alpha is formed after the reference has moved (= 1)
      mask_unclamped    no clamp at -2e38: finfo.min * log2 e overflows to -inf
      ge_no_move        the vote uses >= 6, every row of the tile is multiplied by alpha, but a row whose maximum grew by EXACTLY 6 keeps
                        its old reference (shows only on `exact_step_inputs`: no case of the table holds an exact equality)
      p_unscaled_tail   the ragged last tile skips the vote: it is accumulated at the stale reference whatever its maximum (P overflows
                        or is rescaled late; wrong only through the 16-bit range of P)"""
    n, lq, _ = q.shape
    lk = k.shape[1]
    nqt = (lq + 31) // 32
    pad = nqt * 32 - lq
    qf = torch.cat([q.float(), q.float()[:, -1:].expand(n, pad, -1)], 1) if pad else q.float()
    sl = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s_all = qf @ k.float().transpose(1, 2)                           # fp32 accumulation
    mk = None
    if mask is not None:
        mk = mask.float()
        if variant == "mask_shift":
            mk = torch.cat([mk[:, :1] * 0, mk[:, :-1]], 1)
        if variant != "mask_unclamped":
            mk = mk.clamp_min(-2.0e38)
        mk = mk * torch.tensor(LOG2E, dtype=torch.float32)
    rows = nqt * 32
    m = torch.full((n, rows), -math.inf)
    l = torch.zeros((n, rows))
    o = torch.zeros((n, rows, v.shape[2]))
    late = torch.zeros((n, nqt), dtype=torch.int64)
    vf = v.float()
    if w is not None:
        wf = torch.cat([w.float(), w.float()[:, -1:].expand(n, pad, -1)], 1) if pad else w.float()
    for t0 in range(0, lk, 32):
        t1 = min(t0 + 32, lk)
        sv = s_all[:, :, t0:t1] * sl
        if mk is not None:
            sv = sv + mk[:, None, t0:t1]
        vt = vf[:, t0:t1]
        if variant == "drop_last" and t1 == lk:
            sv = sv.clone()
            sv[:, :, -1] = -math.inf
        if variant == "pad_key" and t1 == lk and lk % 32:
            sv = torch.cat([sv, torch.zeros((n, rows, 1))], 2)
            vt = torch.cat([vt, torch.zeros((n, 1, v.shape[2]))], 1)
        mx = sv.max(-1).values
        m_new = torch.maximum(m, mx)
        grew = mx > m + LAZY
        vote = grew.view(n, nqt, 32).any(-1)                         # one wave = one 32-row query tile
        if variant == "plain":
            vote = torch.ones_like(vote)
        if variant == "p_unscaled_tail" and t1 == lk and lk % 32 and t0 > 0:
            vote = torch.zeros_like(vote)
        if t0 > 0:
            late += (vote & grew.view(n, nqt, 32).any(-1)).long()
        if variant == "ge_no_move":
            vote = (mx >= m + LAZY).view(n, nqt, 32).any(-1)
        vr = vote[:, :, None].expand(n, nqt, 32).reshape(n, rows)
        m_moved = torch.where(vr, m_new, m)
        if variant == "ge_no_move":
            m_moved = torch.where(mx == m + LAZY, m, m_moved)
        alpha = torch.exp2(torch.where(vr, m - m_new, torch.zeros_like(m)))
        alpha = torch.where(vr & (m == -math.inf), torch.zeros_like(alpha), alpha)        # first tile: exp2(-inf)
        if variant == "alpha_after_move":
            alpha = torch.where(m == -math.inf, alpha, torch.ones_like(alpha))
        a_o = torch.where(grew | (m == -math.inf), alpha, torch.ones_like(alpha)) if variant == "vote_rows_only" else alpha
        a_l = torch.ones_like(alpha) if variant == "no_l_rescale" else a_o
        m = m_moved
        p = torch.exp2(sv - m[:, :, None])
        l = l * a_l + p.sum(-1)
        if w is not None:
            p = p * wf[:, :, t0:t1]
        p16 = p.to(dt).float() if dt != F32 else p
        if variant == "lazy_ftz" and dt == F16:
            p16 = torch.where(p16 < 2.0 ** -14, torch.zeros_like(p16), p16)
        o = o * a_o[:, :, None] + p16 @ vt
    if stats is not None:
        stats["late"] = late
    return dict(out32=(o / l[:, :, None])[:, :lq], lse=(m + torch.log2(l))[:, :lq])


def exact_step_inputs(dt):
    """(q, k, v) (1, 32 / 64 / 64, 64) in `dt` whose second key tile exceeds the first by EXACTLY 6 in fp32 log2 units: keys 0..31 and
    33..63 have q.k = 0, key 32 has q.k = 33.27106475830078 = 0x1.0a2b24p+5 (three exact 16-bit terms), and fl32(that * fl32(scale log2 e)) = 6.
    v = 1 on the first tile, 0 on the second: softmax_tile's `>` accumulates the second tile at the stale reference (P = 64)."""
    q = torch.zeros((1, 32, 64), dtype=torch.float64)
    k = torch.zeros((1, 64, 64), dtype=torch.float64)
    v = torch.zeros((1, 64, 64), dtype=torch.float64)
    q[0, :, :3] = 1.0                                                # q.k is the plain sum of the three key terms
    rest = float.fromhex("0x1.0a2b24p+5")
    for d in range(3):
        k[0, 32, d] = float(torch.tensor(rest, dtype=torch.float64).to(dt))
        rest -= float(k[0, 32, d])
    assert rest == 0.0
    v[0, :32] = 1.0
    return q.to(dt), k.to(dt), v.to(dt)


def emulate(case, variant="lazy", stats=None):
    """`emulate_core` on a case, in the layout `check` takes.  The kernels that rescale on every tile (attn_f32_kernel, cls_xattn_kernel,
    tattn_fwd_kernel) are `plain`; both correct variants must pass every case."""
    i = inputs(case)
    heads = 1 if case.kernel == "cls" else H
    e = emulate_core(i["q"], i["k"], i["v"], _item_mask(i, heads), case.dt, variant, stats)
    out = e["out32"].to(case.dt)
    return dict(out=out, out32=e["out32"], lse=e["lse"]) if case.kernel == "train" else dict(out=out)


# ================================================================================================ layouts of the entry points
def to_launch(t):
    """Items layout (N = NP * H, L, 64) -> the (B1 = NP, B0 = 1, L, H * 64) layout of ops.attention."""
    return t.view(NP, H, t.shape[1], 64).permute(0, 2, 1, 3).reshape(NP, 1, t.shape[1], H * 64)


def from_launch(t):
    """(NP, 1, L, H * 64) -> (N, L, 64)."""
    return t.reshape(NP, t.shape[2], H, 64).permute(0, 2, 1, 3).reshape(NP * H, t.shape[2], 64)
