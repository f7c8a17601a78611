"""tests/rowpass_cases.py checked without a GPU.  For every case two fp32 stand-ins per kernel family, written with torch's CPU operators
and summing in different orders, must pass `rowpass_cases.check` - the comparison the GPU file applies - so that no GPU failure can be
blamed on a bound that a correct single-precision implementation breaks.  The bounds must not be vacuous either: on the row kinds randn,
vit, onehot and tiny every bounded output's largest bound stays under 1 % of its largest reference magnitude, the excluded (case, output)
pairs are exactly the listed ones, all on constant rows, and each of seventeen wrong stand-ins (eight forward, nine adjoint) leaves a
bound on a named case."""
import math

import pytest
import torch

from tests import helpers as H
from tests import rowpass_cases as R

F32 = R.F32
ORDERS = (0, 1)


def _case(kernel, case_id):
    return next(c for c in R.CASES[kernel] if c.id == case_id)


def _sum(t, dim, order):
    """order 0: torch's own sum; 1: four interleaved partial sums taken from the far end, added left to right."""
    if order == 0:
        return t.sum(dim, keepdim=True)
    t = t.flip(dim)
    parts = [t.index_select(dim, torch.arange(k, t.shape[dim], 4)).sum(dim, keepdim=True) for k in range(min(4, t.shape[dim]))]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def _colsum(t, order, block):
    """The column sums of `t` as the bounds assume them (rowpass_cases.depth): the rows of each block first, then the blocks."""
    rows, cols = t.shape
    nb = -(-rows // block)
    t = torch.cat([t, torch.zeros((nb * block - rows, cols), dtype=t.dtype)]).view(nb, block, cols)
    return _sum(_sum(t, 1, order)[:, 0], 0, order)[0]


def _k32(p):
    return torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=F32))


# ------------------------------------------------------------------------------------------------ forward stand-ins
def _ln_fwd32(pre, gamma, beta, eps, order, wrong=None, stats_of=None):
    n = pre.shape[-1]
    src = pre if stats_of is None else stats_of
    div = float(-(-n // 256) * 256) if wrong == "padded_width" else float(n)
    m = _sum(src, -1, order) / div
    if wrong == "one_pass":
        q = _sum(src * src, -1, order) / div - m * m
    else:
        ds = src - m
        q = _sum(ds * ds, -1, order) / (div - 1.0 if wrong == "unbiased" else div)
    r = 1.0 / (torch.sqrt(q) + eps) if wrong == "eps_outside" else torch.rsqrt(q + eps)
    return (pre - m) * r * gamma + beta


def _layernorm_standin(c, order, wrong=None):
    i = R.inputs(c)
    x = i["x"].float()
    pre = x + i["residual"].float() if c.res else x
    gamma, beta = (i["gamma"][:, None, :], i["beta"][:, None, :]) if c.twin else (i["gamma"], i["beta"])
    if c.twin:
        pre, x = pre.expand((2,) + tuple(c.shape)), x.expand((2,) + tuple(c.shape))
    y = _ln_fwd32(pre, gamma, beta, c.eps, order, wrong, stats_of=x if wrong == "residual_not_in_stats" else None)
    return {name: y.to(dt) for name, dt in (("stream", c.sdt), ("y16", c.dt16)) if dt is not None}


def _res_ln_standin(c, order, wrong=None):
    i = R.inputs(c)
    rows, cols = c.shape
    keep, _ = R._keep(c, rows, cols)
    if c.p > 0 and wrong == "mask_pitch":           # the mask read at row * pitch + col of a launch whose rows are `cols` long
        pitch = -(-cols // 256) * 256
        flat = torch.arange(rows)[:, None] * pitch + torch.arange(cols)[None, :]
        keep = H.pair_keep(R.drop_seed(c), rows * pitch // cols + 1, cols, R.f32(c.p))[flat // cols, flat % cols]
    if c.p > 0 and wrong == "mask_row":             # the row inside the 4-row block instead of the row
        keep = H.pair_keep(R.drop_seed(c), 4, cols, R.f32(c.p))[torch.arange(rows) % 4]
    s = i["t0"] + i["t1"] if c.t1 else i["t0"]
    k = _k32(c.p) if c.p > 0 else 1.0
    if wrong == "alpha_late":
        pre = (torch.where(keep, s * k, torch.zeros(())) + i["residual"]) * c.alpha
    else:
        pre = torch.where(keep, s * c.alpha * k, torch.zeros(())) + i["residual"]
    y = _ln_fwd32(pre, i["gamma"], i["beta"], c.eps, order, wrong)
    out = dict(pre=pre, y16=y.to(c.dt16))
    if c.want32:
        out["y32"] = y
    return out


# ------------------------------------------------------------------------------------------------ adjoint stand-ins
def _ln_bwd32(x, gamma, dy, eps, order, wrong=None):
    n = float(x.shape[-1])
    m = _sum(x, -1, order) / n
    d = x - m
    r = torch.rsqrt(_sum(d * d, -1, order) / n + (0.0 if wrong == "no_eps" else eps))
    xh, gq = d * r, dy * gamma
    a = torch.zeros(()) if wrong == "no_A" else _sum(gq, -1, order) / n
    b = torch.zeros(()) if wrong == "no_B" else _sum(gq * xh, -1, order) / n
    dx = r * (gq - a - xh * b)
    terms = dy * x if wrong == "dgamma_from_x" else (gq * xh if wrong == "dgamma_times_gamma" else dy * xh)
    dgamma = _colsum(terms, order, 32) + (0.0 if wrong == "dgamma_overwritten" else R.START)
    return dx, dgamma, _colsum(dy, order, 32) + R.START


def _ln_bwd_standin(c, order, wrong=None):
    i = R.inputs(c)
    dx, dgamma, dbeta = _ln_bwd32(i["x"], i["gamma"], i["dy"], c.eps, order, wrong)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def _ln_bwd_fused_standin(c, order, wrong=None):
    i = R.inputs(c)
    dx, dgamma, dbeta = _ln_bwd32(i["x"], i["gamma"], i["dy"], c.eps, order, wrong)
    out = dict(dgamma=dgamma, dbeta=dbeta)
    if c.outs != "dt_only":
        out["dx"] = dx
    if c.outs != "dx_only":
        keep, _ = R._keep(c, *c.shape)
        s = dx + i["t_add"] if (c.t_add and wrong != "no_t_add") else dx
        k = _k32(c.p) if (c.p > 0 and wrong != "no_keep_scale") else 1.0
        dt = torch.where(keep, s * c.alpha * k, torch.zeros(()))
        out["dt16"] = dt.to(c.dt16)
        bias = _colsum(s * c.alpha if wrong == "bias_before_dropout" else dt, order, 32) + R.START
        for name in ("dbias", "dbias2")[:c.nbias]:
            out[name] = bias
    return out


# ------------------------------------------------------------------------------------------------ the 16-bit rows, the scaled add
def _rows16_standin(c, order, wrong=None):
    i = R.inputs(c)
    a = i["a"].float()
    if c.mode == 0:
        return dict(sums=_colsum(a, order, 64) + R.START)
    z = i["z"].float()
    v = a * (0.5 * (1.0 + torch.erf(z * 0.70710678118654752)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z))
    out = dict(out=v.to(c.dt))
    if c.sums:
        out["sums"] = _colsum(v, order, 64) + R.START
    return out


def _rows_scale_add_standin(c, order, wrong=None):
    i = R.inputs(c)
    sc = i["scale"].repeat_interleave(i["rows_per_group"])[:, None]
    if not c.a:
        return dict(out=(sc * i["b"]).to(c.out))
    return dict(out=(i["a"] + sc * i["b"] if order == 0 else torch.addcmul(i["a"], sc.expand_as(i["b"]), i["b"])).to(c.out))


STANDIN = {"layernorm": _layernorm_standin, "res_ln_train": _res_ln_standin, "ln_bwd": _ln_bwd_standin, "ln_bwd_fused": _ln_bwd_fused_standin,
           "rows16_colsum": _rows16_standin, "rows_scale_add": _rows_scale_add_standin}
ALL = [c for k in STANDIN for c in R.CASES[k]]


def _full_id(c):
    return f"{c.kernel}-{c.id}"


def test_table_size_and_coverage():
    assert len(ALL) <= 400, len(ALL)
    for k, cases in R.CASES.items():
        if k != "rows16_colsum" and k != "rows_scale_add":
            left_out = {(R.NO_ADJOINT[0], R.NO_ADJOINT[1][0])} if k.startswith("ln_bwd") else set()
            assert {(c.kind, c.shape[0]) for c in cases} == {(kind, s[0]) for kind in R.KINDS for s in R.SHAPES} - left_out, k
    assert {c.p for c in R.CASES["res_ln_train"]} == set(R.P_DROP) == {c.p for c in R.CASES["ln_bwd_fused"]}
    assert {c.nbias for c in R.CASES["ln_bwd_fused"]} == {0, 1, 2} and {c.ordered for c in R.CASES["ln_bwd_fused"]} == {0, 1}
    assert {(c.xdt, c.sdt) for c in R.CASES["layernorm"] if c.sdt} == {(a, b) for a in (F32, R.F16) for b in (F32, R.F16)}
    assert {c.dt16 for c in R.CASES["layernorm"]} == {R.BF16, R.F16, None} and {c.twin for c in R.CASES["layernorm"]} == {0, 1}
    twins = [c for c in R.CASES["layernorm"] if c.twin and c.res]              # per-branch residuals: (2, rows, cols), a non-zero batch stride
    assert {c.xdt for c in twins} == {F32, R.F16} and {c.kind for c in twins} == set(R.KINDS)
    for c in twins:
        res = R.inputs(c)["residual"]
        assert tuple(res.shape) == (2,) + tuple(c.shape) and (c.kind in ("const", "zero", "onehot") or not torch.equal(res[0], res[1])), c
    assert {(c.kind, c.dt16) for c in R.CASES["ln_bwd_fused"]} >= {(k, d) for k in ("zero", "const") for d in (R.BF16, R.F16)}
    assert {(c.mode, c.ordered, bool(c.pad)) for c in R.CASES["rows16_colsum"]} == {(m, o, s) for m in (0, 1) for o in (0, 1) for s in (False, True)}
    assert {(c.a, c.out) for c in R.CASES["rows_scale_add"]} == {(a, o) for a in (0, 1) for o in (F32, R.BF16, R.F16)}


@pytest.mark.parametrize("c", ALL, ids=_full_id)
def test_correct_standins_are_inside_every_bound(c):
    for order in ORDERS:
        fails = R.check(c, STANDIN[c.kernel](c, order))
        assert not fails, (order, fails)


def test_bounds_say_something():
    """Kinds randn, vit, onehot, tiny: the largest bound of every bounded output is below 1 % of its largest reference magnitude."""
    worst = {}
    for c in ALL:
        if c.kind not in ("randn", "vit", "onehot", "tiny"):
            continue
        assert not R.excluded(c), c
        ref, bnd = R.ref64(c), R.bound(c)
        for name, b in bnd.items():
            if b is None or float(b.max()) == 0.0:
                continue
            ratio = float(b.max()) / float(ref[name].abs().max())
            assert ratio < 0.01, (c, name, ratio)
            key = (c.kernel, name, "16-bit" if b is not None and _is16(c, name) else "fp32")
            worst[key] = max(worst.get(key, 0.0), ratio)
    for key, v in sorted(worst.items()):
        print(f"largest bound / largest |reference|  {key[0]:15s} {key[1]:7s} {key[2]:6s} {v:.2e}")


def _is16(c, name):
    dt = {"stream": getattr(c, "sdt", None), "y16": getattr(c, "dt16", None), "dt16": getattr(c, "dt16", None),
          "out": getattr(c, "dt", None) or getattr(c, "out", None)}.get(name, F32)
    return dt is not None and dt != F32


def test_excluded_set():
    found = {(c.kernel, c.id, name) for c in ALL for name in R.says_nothing(c)}
    assert found == set(R.EXCLUDED), (sorted(found - set(R.EXCLUDED)), sorted(set(R.EXCLUDED) - found))
    for k, cid, name in R.EXCLUDED:
        assert _case(k, cid).kind == "const", (k, cid)
        assert name not in ("pre", "dbeta", "sums"), (k, cid, name)


# ------------------------------------------------------------------------------------------------ the wrong stand-ins
WRONG_FORWARD = [
    ("one_pass", "layernorm", "offset1000-203x768-xdt_f32-sdt_f32-dt16_f16-res1-twin0-eps1e-12"),
    ("unbiased", "layernorm", "randn-33x132-xdt_f32-sdt_f16-dt16_f16-res1-twin0-eps1e-12"),
    ("eps_outside", "res_ln_train", "tiny-203x768-eps1e-06-p0.1-alpha1.0-t11-dt16_f16-want321"),
    ("padded_width", "layernorm", "randn-33x132-xdt_f32-sdt_f16-dt16_f16-res1-twin0-eps1e-12"),
    ("mask_pitch", "res_ln_train", "randn-5x260-eps1e-12-p0.9-alpha0.5-t10-dt16_f16-want320"),
    ("mask_row", "res_ln_train", "randn-2100x768-eps1e-06-p0.9-alpha1.0-t11-dt16_bf16-want321"),
    ("alpha_late", "res_ln_train", "randn-203x768-eps1e-06-p0.0-alpha0.5-t11-dt16_f16-want320"),
    ("residual_not_in_stats", "layernorm", "randn-203x768-xdt_f32-sdt_f32-dt16_f16-res1-twin1-eps1e-12"),
]
WRONG_ADJOINT = [
    ("no_A", "ln_bwd", "randn-33x132-eps1e-06-ordered0"),
    ("no_B", "ln_bwd", "randn-5x260-eps1e-12-ordered0"),
    ("dgamma_from_x", "ln_bwd", "randn-33x132-eps1e-06-ordered0"),
    ("dgamma_times_gamma", "ln_bwd_fused", "randn-33x132-eps1e-12-p0.1-alpha1.0-t_add1-nbias0-dt16_bf16-both-ordered0"),
    ("no_eps", "ln_bwd", "tiny-70x1024-eps1e-06-ordered0"),
    ("no_t_add", "ln_bwd_fused", "randn-203x768-eps1e-06-p0.0-alpha0.5-t_add1-nbias1-dt16_f16-dt_only-ordered0"),
    ("no_keep_scale", "ln_bwd_fused", "randn-203x768-eps1e-12-p0.1-alpha0.5-t_add0-nbias1-dt16_bf16-both-ordered1"),
    ("bias_before_dropout", "ln_bwd_fused", "randn-2100x768-eps1e-06-p0.9-alpha1.0-t_add1-nbias2-dt16_f16-both-ordered0"),
    ("dgamma_overwritten", "ln_bwd", "randn-5x260-eps1e-12-ordered0"),
]


@pytest.mark.parametrize("wrong,kernel,case_id", WRONG_FORWARD + WRONG_ADJOINT, ids=[f"{w[0]}@{w[1]}[{w[2]}]" for w in WRONG_FORWARD + WRONG_ADJOINT])
def test_wrong_standin_leaves_a_bound(wrong, kernel, case_id):
    """The rejecting case of each wrong stand-in is part of the test's id (`pytest -v` lists the seventeen); the line printed below adds
    what the comparison said, and pytest shows it with `-rP` or `-s` only."""
    c = _case(kernel, case_id)
    assert not R.check(c, STANDIN[kernel](c, 0)), "the correct stand-in must pass where the wrong one is judged"
    fails = R.check(c, STANDIN[kernel](c, 0, wrong))
    assert fails, f"{wrong}: passed the comparison on {c}"
    print(f"wrong stand-in {wrong:22s} rejected by {c}: {fails[0].split(': ', 1)[1][:120]}")


def test_exact_expectations_are_in_the_table():
    """Bound None where the issue asks for bits: zero rows, pre without dropout / alpha / t1, the scaled add without `a`; bound 0 on dropped positions."""
    seen = set()
    for c in ALL:
        bnd = R.bound(c)
        if c.kind == "zero" and c.kernel in ("layernorm", "res_ln_train"):
            assert all(b is None for b in bnd.values()), c
            seen.add("zero")
        if c.kernel == "res_ln_train" and c.p == 0 and c.alpha == 1.0 and not c.t1:
            assert bnd["pre"] is None
            seen.add("pre")
        if c.kernel == "rows_scale_add" and not c.a:
            assert bnd["out"] is None
            seen.add("scale_add" + c.scale)
        if c.kernel in ("res_ln_train", "ln_bwd_fused") and c.p > 0 and c.kind != "zero":
            keep, _ = R._keep(c, *c.shape)
            name = "pre" if c.kernel == "res_ln_train" else "dt16"
            if name in bnd and not bool(keep.all()):
                assert float(bnd[name][~keep].max()) == 0.0 and (c.kernel == "res_ln_train" or float(R.ref64(c)[name][~keep].abs().max()) == 0.0)
                seen.add("dropped_" + name)
    assert seen >= {"zero", "pre", "scale_addzero_one", "scale_adddroppath", "scale_addrandn", "dropped_pre", "dropped_dt16"}, seen
    assert math.isclose(R.U, 2.0 ** -24)
