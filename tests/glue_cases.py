"""Case tables, float64 references and a-priori error bounds for the small kernels around the GEMMs: the stage-I ranking path
(cir_linear_f32, cir_l2_normalize, cir_topk_desc, validate.rank_index), the inference glue (cir_gather_rows, cir_patchify,
cir_vit_assemble, cir_small_linear, cir_embed_layernorm) and the training glue (cir_eltwise, cir_colsum, cir_embed_bwd).

A plain module, imported by tests/test_glue_cases_cpu.py (torch's own CPU operators as stand-ins for the kernels: a correct
single-precision implementation passes every comparison, the obvious wrong ones fail) and by the GPU files (the kernels themselves).

For every kernel:  CASES[kernel]  the list of `Case`s (shape, dtypes, strides, special values; the seed is derived from the id),
                   inputs(case)   the CPU tensors of the case, generated from the seed,
                   ref64(case)    {output name: float64 tensor}: the operation as include/cirrank.h states it, in float64 on the CPU,
                   bound(case)    {output name: float64 tensor, or None}: the elementwise error bound; None = bit-exact,
                   check(case, outputs) -> list of failure messages (empty = pass): the ONE comparison both suites apply.

How the bounds are made (u = 2^-24, the unit roundoff of fp32; no constant below is tuned to a kernel's output)
--------------------------------------------------------------------------------------------------------------------------------
* A dot product of depth K accumulated in fp32 in ANY order (with or without FMA contraction) misses the exact value by at most
  gamma_K * (|x| . |w|) with gamma_K = K u / (1 - K u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1);
  (K + 2) u covers gamma_K for every K < 2^21.  Each further fp32 operation on a value v whose error so far is e (the bias add,
  `1 - v`) adds u * (|result| + e).
* A column sum over R rows (any order, partial sums combined by atomics): (R + 2) u * sum |x|.  An accumulation INTO an existing
  value counts that value as one more term.
* A 16-bit output rounds the fp32 result once more: half an ulp of the output format AT the result.  Half an ulp of a format with p
  significant bits at y is 2^(floor(log2 |y|) - p): p = 11 for fp16 (so <= 2^-11 |y|) and p = 8 for bf16 (between 2^-9 |y| and
  2^-8 |y|: the flat figure 2^-9 |y| holds only at the top of a binade, and a correctly rounded bf16 value just above a power of two
  misses it - test_glue_cases_cpu.py::test_half_ulp_is_attained shows both).  `half_ulp` evaluates the exact expression at
  |y| + (the fp32 bound), so a result that the fp32 error pushes into the next binade is covered, with the subnormal spacing as floor.
* cir_l2_normalize, y = x / max(sqrt(sum x^2), 1e-12) over n columns.  The sum of squares has only non-negative terms, so its
  RELATIVE error is <= (n + 1) u (n products, n - 1 additions); the square root halves a relative error and adds its own rounding
  (2 u allowed: the device square root need not be correctly rounded); the reciprocal or division 2 u; the final product u:
      |dy| <= (n / 2 + 6) u |y|          (+ one fp32 subnormal).
  A row under the clamp has a smaller error (the constant 1e-12 rounded to fp32, one division, one product).  No case puts a norm
  within 1e-3 (relative) of the clamp itself, where the two branches meet.
* cir_embed_layernorm, y = (x - m) * r * g + b with x = word + pos (one rounding: u |x|), m = mean(x), r = (mean((x - m)^2) + eps)^-1/2
  over n columns.  With a = mean |x| and d = x - m:
      error of m     <= (n + 3) u a                              (the sum, the division by n, the roundings of x)
      error of d     <= e_d = u |x| + (n + 3) u a + u |d|
      error of q = mean(d^2)  <= mean(2 |d| e_d) + (n + 3) u q
      relative error of r     <= e_r = (error of q) / (2 (q + eps)) + 3 u            (rsqrt 2 u, the division by n)
      |dy| <= |g| r e_d + |d r g| (e_r + 3 u) + u |y|
  which is first order in u; the bound used is TWICE that, which covers the dropped second-order terms (they are below
  (n u) times the first-order ones, n u < 2^-13) with room to spare.
* cir_eltwise.  relu, relu', add and scale round once (exact against the float64 result rounded to fp32 and then to the output
  type).  The GELU modes go through erff and __expf: erff is allowed the 16 ulp that the OpenCL C specification grants erf (the table the ROCm
  device library's math functions are built to), its argument x / sqrt(2) carries two roundings (the constant, the product) which move the result by at
  most erf'(t) |t| 2 u; __expf(a) is 2^(a log2 e) on the hardware exponential (1 ulp) whose argument carries (a, log2 e, product)
  three roundings: a relative error of at most (3 |a| + 2) u, (4 |a| + 4) u used, floored by one flushed fp32 denormal (2^-126).
      gelu(x)  = x/2 (1 + erf t):         |dy| <= |x|/2 (E + u |1 + erf t|) + 2 u |y|,   E = 16 u |erf t| + erf'(t) |t| 2 u
      gelu'(x) = (1 + erf t)/2 + x phi(x): |dg| <= (E + u |1 + erf t|)/2 + |x| phi(x) ((4 |a| + 4) u + 3 u) + 2^-126 |x| + u |g'|,
      and dz = dy * gelu'(z) adds |dy| |dg| + u |dz|.
  Dropout keeps element i iff the generator says so (tests/helpers.splitmix_keep) and scales by 1 / (1 - p) formed in fp32
  (p, 1 - p, the division, the product: 4 u |y|).
"""
import functools
import itertools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import helpers as H

U = 2.0 ** -24                       # unit roundoff of fp32
SUB32 = 2.0 ** -149                  # spacing of the fp32 subnormals
PREC = {torch.float16: 11, torch.bfloat16: 8}            # significant bits
EMIN = {torch.float16: -14, torch.bfloat16: -126}        # exponent of the smallest normal number
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF16: "bf16", F16: "f16", F32: "f32"}
VOCAB = H.FULL_BERT["vocab_size"]    # 30524


def _fmt(key, value):
    if isinstance(value, torch.dtype):
        return f"{key}_{DT_NAME[value]}"
    if isinstance(value, tuple):
        return "x".join(map(str, value))
    return value if isinstance(value, str) else f"{key}{value}"


class Case:
    def __init__(self, kernel, **kw):
        self.kernel = kernel
        self.p = dict(kw)
        self.__dict__.update(kw)
        self.id = "-".join(_fmt(k, v) for k, v in kw.items())
        self.seed = zlib.crc32(f"{kernel}/{self.id}".encode())

    def __repr__(self):
        return f"{self.kernel}[{self.id}]"

    def gen(self):
        return torch.Generator(device="cpu").manual_seed(self.seed)


def ids(cases):
    return [c.id for c in cases]


def case_id(case):
    """For pytest.mark.parametrize(..., ids=case_id)."""
    return case.id


def half_ulp(y: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Half the spacing of `dtype` at |y| (float64 in and out): 2^(max(floor(log2 |y|), emin) - p)."""
    y = y.abs().double()
    e = torch.frexp(y)[1].to(torch.int64) - 1                      # y = m 2^ex, m in [0.5, 1)  =>  floor(log2 y) = ex - 1
    e = torch.where(y == 0, torch.full_like(e, EMIN[dtype]), e).clamp(min=EMIN[dtype])
    return torch.ldexp(torch.ones_like(y), (e - PREC[dtype]).to(torch.int32))


def out_bound(ref: torch.Tensor, b32: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The bound of an output stored in `dtype` from the bound `b32` of the fp32 value it is rounded from."""
    if dtype == F32:
        return b32 + SUB32
    return b32 + half_ulp(ref.abs() + b32, dtype)


def round_once(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """A float64 result as an exact kernel stores it: rounded to fp32 (the kernels' arithmetic type), then to the output type."""
    return ref.float().to(dtype)


def check(case, outputs, ref=None, bnd=None):
    """Compare `outputs` {name: CPU tensor} with ref64(case) within bound(case).  Returns the list of failures (empty = pass).
    An output whose bound is None must equal the reference rounded once, bit for bit (torch.equal; NaN never passes)."""
    ref = ref64(case) if ref is None else ref
    bnd = bound(case) if bnd is None else bnd
    fails = []
    assert set(outputs) == set(ref), (set(outputs), set(ref))
    for name, out in outputs.items():
        r, b = ref[name], bnd[name]
        if tuple(out.shape) != tuple(r.shape):
            fails.append(f"{case} {name}: shape {tuple(out.shape)} != {tuple(r.shape)}")
        elif b is None:
            want = r if r.dtype == out.dtype else round_once(r, out.dtype)
            if not torch.equal(out, want):
                bad = (out != want) | (out != out)
                fails.append(f"{case} {name}: {int(bad.sum())} of {out.numel()} elements differ from the reference (first at flat index "
                             f"{int(bad.flatten().nonzero()[0])})")
        else:
            err = (out.double() - r).abs()
            bad = ~(err <= b)                                      # NaN lands here
            if bool(bad.any()):
                i = int(torch.where(bad.flatten(), (err / b.clamp_min(1e-300)).flatten().nan_to_num(nan=math.inf), torch.zeros(())).argmax())
                fails.append(f"{case} {name}: {int(bad.sum())} of {out.numel()} elements outside the bound; worst at flat index {i}: "
                             f"got {out.flatten()[i].item()!r} ref {r.flatten()[i].item()!r} bound {b.flatten()[i].item():.3e}")
    return fails


def worst_ratio(case, outputs, ref=None, bnd=None):
    """max |out - ref| / bound over the bounded outputs (for printing next to an assertion)."""
    ref = ref64(case) if ref is None else ref
    bnd = bound(case) if bnd is None else bnd
    w = 0.0
    for name, out in outputs.items():
        if bnd[name] is not None:
            w = max(w, float(((out.double() - ref[name]).abs() / bnd[name].clamp_min(1e-300)).max()))
    return w


# ================================================================================================ cir_linear_f32
_LIN_SHAPES = [(1, 1, 1), (37, 9, 50), (63, 65, 17), (64, 64, 16), (65, 129, 15), (2, 256, 768), (64, 6346, 256), (4181, 2297, 256)]


def _linear_cases():
    out = []
    for i, mnk in enumerate(_LIN_SHAPES):
        big = mnk[0] * mnk[1] > 100000
        for mode in (0, 1, 2):
            if big:      # the two real distance matrices: once per mode, the flags alternating (the full grid runs on the six small shapes)
                out.append(Case("linear_f32", mnk=mnk, mode=mode, bias=int(mode == 0), strided=int((mode + i) % 2)))
            else:
                for bias, strided in itertools.product((0, 1), (0, 1)):
                    out.append(Case("linear_f32", mnk=mnk, mode=mode, bias=bias, strided=strided))
    return out


def _linear_inputs(c):
    (m, n, k), g = c.mnk, c.gen()
    h = torch.randn((m, 3, k) if c.strided else (m, k), generator=g)
    return dict(h=h, x=h[:, 0, :] if c.strided else h, w=torch.randn((n, k), generator=g),
                bias=torch.randn((n,), generator=g) if c.bias else None)


def linear_ref_bound(x, w, bias, mode, k=None):
    """(ref64, fp32 bound) of cir_linear_f32 on the given fp32 / 16-bit operands: shared with small_linear and rank_index."""
    x, w = x.double(), w.double()
    k = x.shape[1] if k is None else k
    v = x @ w.T
    b = (k + 2) * U * (x.abs() @ w.abs().T)                       # the dot product, any order
    if bias is not None:
        v = v + bias.double()
        b = b + U * (v.abs() + b)                                 # the bias add
    if mode == 1:
        v = 1.0 - v
        b = b + U * (v.abs() + b)                                 # 1 - v
    elif mode == 2:
        v = v - 1.0
        b = b + U * (v.abs() + b)
    return v, b + SUB32


def _linear_ref(c):
    i = inputs(c)
    return dict(y=linear_ref_bound(i["x"], i["w"], i["bias"], c.mode)[0])


def _linear_bound(c):
    i = inputs(c)
    return dict(y=linear_ref_bound(i["x"], i["w"], i["bias"], c.mode)[1])


# ================================================================================================ cir_l2_normalize
def _l2_cases():
    out = [Case("l2_normalize", rows=r, cols=n, special="none") for r, n in itertools.product((1, 3, 4, 5, 4099), (1, 63, 64, 65, 256, 1000))]
    out += [Case("l2_normalize", rows=r, cols=n, special=s) for s in ("zero_row", "tiny_row") for r, n in ((1, 256), (5, 65), (7, 1), (6, 1000))]
    return out


def _l2_inputs(c):
    x = torch.randn((c.rows, c.cols), generator=c.gen()) * 3.0
    r = c.rows // 2
    if c.special == "zero_row":
        x[r] = 0.0
    elif c.special == "tiny_row":                                   # norm 1e-20: F.normalize divides it by 1e-12 (its squares underflow in fp32)
        x[r] = (x[r].double() / x[r].double().norm() * 1e-20).float()
    return dict(x=x)


def _l2_ref(c):
    x = inputs(c)["x"].double()
    return dict(y=x / x.norm(dim=1, keepdim=True).clamp_min(1e-12))


def _l2_bound(c):
    return dict(y=(c.cols / 2 + 6) * U * _l2_ref(c)["y"].abs() + SUB32)


# ================================================================================================ cir_topk_desc
ARGSORT_KINDS = ("random", "all_equal", "levels8", "sorted_desc", "sorted_asc", "signed_zero", "inf", "nan")
_ARGSORT_K = (1, 2, 3, 255, 256, 257, 2047, 2048, 2297, 4096, 4097, 6346, 8191, 8192)       # one pair; 256 threads up to 1024 columns, 1024 above


def _argsort_cases():
    out = [Case("argsort_desc", q=3, k=k, kind=kind) for k in _ARGSORT_K for kind in ARGSORT_KINDS]
    out += [Case("argsort_desc", q=4181, k=2297, kind=kind) for kind in ("random", "levels8")]      # every query of the largest split
    return out


def _argsort_inputs(c):
    g, shape = c.gen(), (c.q, c.k)
    v = torch.randn(shape, generator=g)
    pick = torch.rand(shape, generator=g)
    if c.kind == "all_equal":
        v = torch.full(shape, 0.25)
    elif c.kind == "levels8":
        v = torch.randint(0, 8, shape, generator=g).float() / 8 - 0.5
    elif c.kind == "sorted_desc":
        v = v.sort(dim=1, descending=True).values
    elif c.kind == "sorted_asc":
        v = v.sort(dim=1).values
    elif c.kind == "signed_zero":
        v = torch.tensor([0.0, -0.0, 1.0, -1.0])[torch.randint(0, 4, shape, generator=g)]
    elif c.kind == "inf":
        v = torch.where(pick < 0.1, torch.tensor(math.inf), torch.where(pick > 0.9, torch.tensor(-math.inf), v))
    elif c.kind == "nan":
        v = torch.where(pick < 0.1, torch.tensor(math.nan), torch.where(pick > 0.95, torch.tensor(-math.inf), v))
        v = torch.where((pick > 0.45) & (pick < 0.5), torch.tensor(math.inf), v)
        v[:, 0] = math.nan
    return dict(logits=v.contiguous())


def argsort_ref(logits):
    """The contract of cir_topk_desc: NaN ranks as -inf; among equal values (NaN and -inf alike) the lower index comes first."""
    v = torch.where(logits != logits, torch.full_like(logits, -math.inf), logits)
    return torch.argsort(v, dim=-1, descending=True, stable=True)


def _argsort_ref(c):
    return dict(idx=argsort_ref(inputs(c)["logits"]))


# ================================================================================================ validate.rank_index at dataset scale
def _rank_cases():
    return [Case("rank_index", q=64, n=n) for n in (2297, 3817, 5373, 6346)]


def _rank_inputs(c):
    g = torch.Generator(device="cpu").manual_seed(c.n)             # seed = index size (6346 is the case the issue's figures were taken on)
    qf = F.normalize(torch.randn((c.q, 256), generator=g, dtype=torch.float64), dim=1).float()
    xf = F.normalize(torch.randn((c.n, 256), generator=g, dtype=torch.float64), dim=1).float()
    return dict(pred=qf, index=xf)


def _rank_ref(c):
    i = inputs(c)
    return dict(dist=linear_ref_bound(i["pred"], i["index"], None, 1)[0])


def _rank_bound(c):
    i = inputs(c)
    return dict(dist=linear_ref_bound(i["pred"], i["index"], None, 1)[1])


def rank_failures(case, order, neg_dist=None):
    """(a) `order` is bit for bit the stable descending argsort of `neg_dist`, the matrix the ranking was made from (the sort alone);
    (b) walking each row of `order`, the float64 distance never falls below the running maximum by more than 2 max(bound): two
    candidates may swap only when the fp32 matrix cannot tell them apart."""
    dist, bmax = ref64(case)["dist"], float(bound(case)["dist"].max())
    std = float(dist.std(dim=1).min())
    fails = []
    if not 2 * bmax < std / 100:                                    # the check would be vacuous: the inputs were changed
        fails.append(f"{case}: 2 max(bound) = {2 * bmax:.3e} is not far below the row spread {std:.3e}")
    if tuple(order.shape) != tuple(dist.shape) or not torch.equal(order.sort(dim=1).values, torch.arange(case.n).expand(case.q, -1)):
        return fails + [f"{case}: the ranking is not a permutation of the index"]
    if neg_dist is not None and not torch.equal(order, argsort_ref(neg_dist)):
        fails.append(f"{case}: the order is not the stable descending argsort of the kernel's own matrix")
    walked = torch.gather(dist, 1, order)
    drop = (torch.cummax(walked, dim=1).values - walked).max()
    if not float(drop) <= 2 * bmax:
        fails.append(f"{case}: a distance falls {float(drop):.3e} below the running maximum (allowed {2 * bmax:.3e})")
    return fails


# ================================================================================================ cir_gather_rows
GATHER_PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32), (BF16, F16), (F16, BF16)]
VIT_ROW = 197 * 768


def _gather_cases():
    out = []
    for s, d in GATHER_PAIRS:
        out.append(Case("gather_rows", src=s, dst=d, row_elems=8, src_rows=37, n_rows=300, index="clamp"))       # 300 threads: a partial 2nd block
        out.append(Case("gather_rows", src=s, dst=d, row_elems=VIT_ROW, src_rows=4, n_rows=5, index="clamp"))    # 94560 threads = 369.4 blocks
        out.append(Case("gather_rows", src=s, dst=d, row_elems=64, src_rows=37, n_rows=37, index="none"))
    return out


def _gather_inputs(c):
    g = c.gen()
    src = torch.randn((c.src_rows, c.row_elems), generator=g) * 8.0
    src[:, ::5] *= 2.0 ** -20                                        # fp16 subnormals on the way out
    index = None
    if c.index == "clamp":
        index = torch.randint(0, c.src_rows, (c.n_rows,), generator=g)       # repeats: n_rows > src_rows
        index[1], index[c.n_rows - 2], index[c.n_rows // 2] = -1, c.src_rows + 3, index[0]
    return dict(src=src.to(c.src), index=index)


def _gather_ref(c):
    i = inputs(c)
    rows = torch.arange(c.src_rows) if i["index"] is None else i["index"].clamp(0, c.src_rows - 1)   # the header: "clamped to [0, src_rows)"
    return dict(dst=i["src"].double()[rows])


# ================================================================================================ cir_patchify
PATCHIFY_PAIRS = [(F32, BF16), (F32, F16), (F32, F32), (BF16, BF16), (F16, F16)]


def _patchify_cases():
    out = [Case("patchify", px=px, src=s, dst=d, b=b, offset=0) for px in (224, 384) for s, d in PATCHIFY_PAIRS for b in (1, 2)]
    out += [Case("patchify", px=224, src=s, dst=d, b=1, offset=1) for s, d in PATCHIFY_PAIRS]     # image one element into its storage: scalar path
    return out


def _patchify_inputs(c):
    n = c.b * 3 * c.px * c.px
    store = (torch.randn((n + c.offset,), generator=c.gen()) * 2.0).to(c.src)
    return dict(storage=store, image=store[c.offset:].view(c.b, 3, c.px, c.px))


def _patchify_ref(c, patch=16):
    img = inputs(c)["image"].double()
    b, ch, h, w = img.shape
    gh, gw = h // patch, w // patch
    # patches[(b*gh+py)*gw+px][c*p*p + ky*p + kx] = image[b][c][py*p+ky][px*p+kx]
    return dict(patches=img.view(b, ch, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5).reshape(b * gh * gw, ch * patch * patch))


# ================================================================================================ cir_vit_assemble
def _assemble_cases():
    return [Case("vit_assemble", bpd=bpd, stream=s) for bpd in ((1, 196, 768), (3, 576, 768), (2, 196, 1024)) for s in (F32, F16)]


def _assemble_inputs(c):
    (b, p, d), g = c.bpd, c.gen()
    return dict(proj=torch.randn((b * p, d), generator=g).to(c.stream), cls=torch.randn((d,), generator=g), pos=torch.randn((p + 1, d), generator=g))


def _assemble_ref(c):
    """x[b][0] = cls + pos[0]; x[b][1+i] = proj[b*P+i] + pos[1+i]: ONE fp32 addition, then (fp16 stream) one rounding to fp16 -
    `check` rounds the float64 sum to fp32 and then to the stream type, i.e. (proj.float() + pos).half() and (cls + pos[0]).half()."""
    (b, p, d), i = c.bpd, inputs(c)
    tok = torch.cat([i["cls"].double().expand(b, 1, d), i["proj"].double().view(b, p, d)], dim=1)
    return dict(x=tok + i["pos"].double()[None])


# ================================================================================================ cir_small_linear
_SL_N, _SL_K, _SL_M = (1, 2, 3, 4, 5, 6, 7, 8), (8, 504, 512, 520, 768, 1024), (1, 3, 4, 5, 4099)


def _small_linear_cases():
    """Every (N, K) pair; M, the dtype, the bias and the row stride cycle with periods (5, 2, 2, 2) chosen so that every value of each
    meets every N and every K; then the full dtype x bias x stride grid on the product's own shape (N = 2, K = 768) and on the
    partial-last-pass shape (N = 8, K = 520), with the M % 4 tails 5 and 4099."""
    out, seen = [], set()
    for i, (ni, ki) in enumerate(itertools.product(range(8), range(6))):
        kw = dict(m=_SL_M[i % 5], n=_SL_N[ni], k=_SL_K[ki], dt=(BF16, F16)[(ni + ki) % 2], bias=(ni + ki // 2) % 2, strided=(ni // 2 + ki) % 2)
        out.append(Case("small_linear", **kw))
    for (n, k, m), dt, bias, strided in itertools.product(((2, 768, 4099), (8, 520, 5)), (BF16, F16), (0, 1), (0, 1)):
        out.append(Case("small_linear", m=m, n=n, k=k, dt=dt, bias=bias, strided=strided))
    return [c for c in out if not (c.id in seen or seen.add(c.id))]


def _small_linear_inputs(c):
    g = c.gen()
    h = torch.randn((c.m, 2, c.k) if c.strided else (c.m, c.k), generator=g).to(c.dt)       # strided: the CLS rows of an (M, L, K) tensor
    return dict(h=h, x=h[:, 0, :] if c.strided else h, w=torch.randn((c.n, c.k), generator=g).to(c.dt),
                bias=torch.randn((c.n,), generator=g) if c.bias else None)


def _small_linear_ref(c):
    i = inputs(c)
    return dict(y=linear_ref_bound(i["x"], i["w"], i["bias"], 0)[0])


def _small_linear_bound(c):
    i = inputs(c)
    return dict(y=linear_ref_bound(i["x"], i["w"], i["bias"], 0)[1])


# ================================================================================================ cir_embed_layernorm
EMBED_PAIRINGS = [(F32, BF16), (F32, F16), (F16, BF16), (F16, F16), (F32, F32)]      # (stream, 16-bit output); (f32, f32) = "exact" mode, no 16-bit copy
EMBED_EPS = 1e-12


def _embed_ln_cases():
    return [Case("embed_layernorm", cols=n, l=l, stream=s, dt16=d) for n in (128, 768, 1024) for l in (1, 32, 42, 512) for s, d in EMBED_PAIRINGS]


@functools.lru_cache(maxsize=1)
def embed_tables(cols):
    """(word (30524, cols), pos (512, cols), gamma, beta) fp32: BERT-like scales; shared by every case of one width."""
    g = torch.Generator(device="cpu").manual_seed(cols)
    return (torch.randn((VOCAB, cols), generator=g) * 0.05, torch.randn((512, cols), generator=g) * 0.02,
            1.0 + 0.1 * torch.randn((cols,), generator=g), 0.1 * torch.randn((cols,), generator=g))


def _embed_ln_inputs(c):
    word, pos, gamma, beta = embed_tables(c.cols)
    ids_ = torch.randint(0, VOCAB, (3, c.l), generator=c.gen())
    ids_[0, 0], ids_[2, c.l - 1] = 0, VOCAB - 1                     # the first and the last row of the table
    return dict(ids=ids_, word=word, pos=pos, gamma=gamma, beta=beta)


def _embed_ln_terms(c):
    i = inputs(c)
    n = c.cols
    x = i["word"][i["ids"]].double() + i["pos"][:c.l].double()[None]
    m = x.mean(-1, keepdim=True)
    d = x - m
    q = (d * d).mean(-1, keepdim=True)
    r = (q + EMBED_EPS) ** -0.5
    g, b = i["gamma"].double(), i["beta"].double()
    y = d * r * g + b
    a = x.abs().mean(-1, keepdim=True)
    e_d = U * x.abs() + (n + 3) * U * a + U * d.abs()
    e_q = (2 * d.abs() * e_d).mean(-1, keepdim=True) + (n + 3) * U * q
    e_r = e_q / (2 * (q + EMBED_EPS)) + 3 * U
    b32 = 2.0 * (g.abs() * r * e_d + (d * r * g).abs() * (e_r + 3 * U) + U * y.abs())          # see the module docstring
    return y, b32


def _embed_ln_ref(c):
    y = _embed_ln_terms(c)[0]
    return dict(stream=y) if c.dt16 == F32 else dict(stream=y, y16=y)


def _embed_ln_bound(c):
    y, b32 = _embed_ln_terms(c)
    out = dict(stream=out_bound(y, b32, c.stream))
    if c.dt16 != F32:
        out["y16"] = out_bound(y, b32, c.dt16)                      # rounded from the fp32 value, not from the 16-bit stream
    return out


# ================================================================================================ cir_eltwise
ELT_MODES = ("gelu", "gelu_bwd", "relu", "relu_bwd", "dropout", "add", "scale")        # = mode 0..6 of cir_eltwise
ELT_N = (1, 2, 3, 5, 1023, 1024, 1025, 37001)
ELT_P = {"dropout": 0.1, "scale": 0.37}                                                # the float argument (drop probability / scale factor)
ELT_SEED = 0x1234567


def _eltwise_cases():
    return [Case("eltwise", mode=m, z=z, out=o, n=n) for m in ELT_MODES for z in (F32, BF16, F16) for o in (F32, BF16, F16) for n in ELT_N]


def _eltwise_inputs(c):
    g = c.gen()
    z = (torch.randn((c.n,), generator=g) * 2.5).to(c.z)
    if c.n >= 1023:
        z[:7] = torch.tensor([0.0, -0.0, 6.0, -6.0, -9.5, 1e-4, -1e-4]).to(c.z)           # the flat tails of erf, and the origin
    return dict(z=z, dy=torch.randn((c.n,), generator=g))


def _erf_terms(x):
    t = x / math.sqrt(2.0)
    erf = torch.erf(t)
    e_erf = 16 * U * erf.abs() + (2 / math.sqrt(math.pi)) * torch.exp(-t * t) * t.abs() * 2 * U
    return erf, e_erf


def gelu_bwd_terms(x, d):
    """(float64 d * gelu'(x), its fp32 bound) on float64 operands: the gelu' terms of the module docstring (shared with tests/rowpass_cases.py)."""
    erf, e_erf = _erf_terms(x)
    a = 0.5 * x * x
    xphi = x.abs() * torch.exp(-a) / math.sqrt(2 * math.pi)
    gp = 0.5 * (1 + erf) + x * torch.exp(-a) / math.sqrt(2 * math.pi)
    e_gp = (e_erf + U * (1 + erf).abs()) / 2 + xphi * ((4 * a + 4) * U + 3 * U) + 2.0 ** -126 * x.abs() + U * gp.abs()
    y = d * gp
    return y, d.abs() * e_gp + U * y.abs()


def _eltwise_terms(c):
    """(float64 result, fp32 bound or None)."""
    i = inputs(c)
    x, d = i["z"].double(), i["dy"].double()
    if c.mode == "gelu":
        erf, e_erf = _erf_terms(x)
        y = 0.5 * x * (1 + erf)
        return y, x.abs() / 2 * (e_erf + U * (1 + erf).abs()) + 2 * U * y.abs()
    if c.mode == "gelu_bwd":
        return gelu_bwd_terms(x, d)
    if c.mode == "relu":
        return x.clamp_min(0.0), None
    if c.mode == "relu_bwd":
        return torch.where(x > 0, d, torch.zeros_like(d)), None
    if c.mode == "dropout":
        p = float(np.float32(ELT_P["dropout"]))
        keep = H.splitmix_keep(ELT_SEED, c.n, p)
        y = torch.where(keep, x / (1.0 - p), torch.zeros_like(x))
        return y, 4 * U * y.abs()
    if c.mode == "add":
        return x + d, None
    return x * float(np.float32(ELT_P["scale"])), None


def _eltwise_ref(c):
    return dict(out=_eltwise_terms(c)[0])


def _eltwise_bound(c):
    y, b32 = _eltwise_terms(c)
    return dict(out=None if b32 is None else out_bound(y, b32, c.out))


def dropout_interval(n, p, sigmas=5.0):
    """The kept count of n independent draws that keep with probability 1 - p: mean n (1 - p), variance n p (1 - p); the interval is
    `sigmas` standard deviations wide each way (5 sigma: a correct generator leaves it once in 1.7 million seeds)."""
    mean, sd = n * (1.0 - p), math.sqrt(n * p * (1.0 - p))
    return mean - sigmas * sd, mean + sigmas * sd


# ================================================================================================ cir_colsum
def _colsum_cases():
    out = [Case("colsum", rows=r, cols=n, pad=pad) for r in (1, 3, 4, 5, 31, 32, 33, 777) for n in (1, 255, 256, 257, 768, 3072) for pad in (0, 8)]
    # the product's 2R = 9232 rows: at the narrowest, a 256-tail and the widest extent (the other widths run at 777 rows above)
    out += [Case("colsum", rows=9232, cols=n, pad=pad) for n, pad in ((1, 0), (257, 0), (257, 8), (3072, 0))]
    return out


def _colsum_inputs(c):
    g = c.gen()
    buf = torch.randn((c.rows, c.cols + c.pad), generator=g)
    return dict(buf=buf, x=buf[:, :c.cols], out0=torch.randn((c.cols,), generator=g) * 4.0)


def _colsum_ref(c):
    i = inputs(c)
    return dict(out=i["out0"].double() + i["x"].double().sum(0))


def _colsum_bound(c):
    i = inputs(c)                                                    # R rows and the value already there: R + 1 terms, any order
    return dict(out=(c.rows + 3) * U * (i["x"].double().abs().sum(0) + i["out0"].double().abs()) + SUB32)


# ================================================================================================ cir_embed_bwd
def _embed_bwd_cases():
    return [Case("embed_bwd", cols=n, l=l, ids=k) for n in (64, 768, 1000) for l in (1, 32, 42) for k in ("equal", "distinct", "random")]


def _embed_bwd_inputs(c):
    g, rows = c.gen(), 3 * c.l
    if c.ids == "equal":
        ids_ = torch.full((rows,), VOCAB - 1, dtype=torch.int64)                          # worst-case collisions, on the last row of the table
    elif c.ids == "distinct":
        ids_ = torch.randperm(VOCAB, generator=g)[:rows]
    else:
        ids_ = torch.randint(0, VOCAB, (rows,), generator=g)
        ids_[0] = 0
        ids_[rows // 2] = ids_[rows - 1]                                                  # at least one collision
    return dict(ids=ids_, dy=torch.randn((rows, c.cols), generator=g))


def _embed_bwd_terms(c):
    """dword is compared on the rows the ids touch (`touched`, sorted); the rest of the table must stay as it was (checked by the callers)."""
    i = inputs(c)
    rows, dy = 3 * c.l, i["dy"].double()
    touched, inv = torch.unique(i["ids"], return_inverse=True)
    dword = torch.zeros((touched.numel(), c.cols), dtype=torch.float64).index_add_(0, inv, dy)
    aword = torch.zeros_like(dword).index_add_(0, inv, dy.abs())
    cnt = torch.zeros((touched.numel(), 1), dtype=torch.float64).index_add_(0, inv, torch.ones((rows, 1), dtype=torch.float64))
    pos = torch.arange(rows) % c.l
    dpos = torch.zeros((c.l, c.cols), dtype=torch.float64).index_add_(0, pos, dy)
    apos = torch.zeros_like(dpos).index_add_(0, pos, dy.abs())
    return touched, dict(dword=dword, dpos=dpos), dict(dword=(cnt + 2) * U * aword + SUB32, dpos=(3 + 2) * U * apos + SUB32)


def _embed_bwd_ref(c):
    return _embed_bwd_terms(c)[1]


def _embed_bwd_bound(c):
    return _embed_bwd_terms(c)[2]


def embed_bwd_touched(c):
    return _embed_bwd_terms(c)[0]


# ================================================================================================ registry
_EXACT = lambda name: (lambda c: {name: None})      # noqa: E731
_KERNELS = {
    "linear_f32": (_linear_cases, _linear_inputs, _linear_ref, _linear_bound),
    "l2_normalize": (_l2_cases, _l2_inputs, _l2_ref, _l2_bound),
    "argsort_desc": (_argsort_cases, _argsort_inputs, _argsort_ref, _EXACT("idx")),
    "rank_index": (_rank_cases, _rank_inputs, _rank_ref, _rank_bound),
    "gather_rows": (_gather_cases, _gather_inputs, _gather_ref, _EXACT("dst")),
    "patchify": (_patchify_cases, _patchify_inputs, _patchify_ref, _EXACT("patches")),
    "vit_assemble": (_assemble_cases, _assemble_inputs, _assemble_ref, _EXACT("x")),
    "small_linear": (_small_linear_cases, _small_linear_inputs, _small_linear_ref, _small_linear_bound),
    "embed_layernorm": (_embed_ln_cases, _embed_ln_inputs, _embed_ln_ref, _embed_ln_bound),
    "eltwise": (_eltwise_cases, _eltwise_inputs, _eltwise_ref, _eltwise_bound),
    "colsum": (_colsum_cases, _colsum_inputs, _colsum_ref, _colsum_bound),
    "embed_bwd": (_embed_bwd_cases, _embed_bwd_inputs, _embed_bwd_ref, _embed_bwd_bound),
}
CASES = {k: v[0]() for k, v in _KERNELS.items()}
_last = {}


def inputs(case):
    """The CPU tensors of a case (the last one asked for is kept: ref64 and bound read the same tensors)."""
    if _last.get("case") is not case:
        _last.clear()
        _last.update(case=case, inputs=_KERNELS[case.kernel][1](case))
    return _last["inputs"]


def ref64(case):
    return _KERNELS[case.kernel][2](case)


def bound(case):
    return _KERNELS[case.kernel][3](case)
