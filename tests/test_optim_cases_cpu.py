"""tests/optim_cases.py checked without a GPU.  Two correct fp32 stand-ins of the AdamW update - a numpy transcription of the kernels and
torch.optim.AdamW(foreach=False) on the CPU with its state injected and the fp32-rounded scalars - must pass `optim_cases.check`, the
comparison the GPU file applies, on every case; torch with the DOUBLE betas must leave the bound at t = 1 (the deviation the module
docstring names, not an error of the table); each of twelve wrong update rules must fail on a case named in the test id; the range rule
and the coverage of the index map are asserted on the whole table.  A Python stand-in of cir_grads_check must pass its table and seven
wrong forms must fail.  `train_core.loss_scale` is tested here as well: it needs no GPU."""
import math

import numpy as np
import pytest
import torch

from tests import optim_cases as O

ALL = O.CASES["adamw_dev"] + O.CASES["adamw"]
_full_id = lambda c: f"{c.kernel}[{c.id}]"      # noqa: E731


def _case(kernel, case_id):
    return next(c for c in O.CASES[kernel] if c.id == case_id)


# ------------------------------------------------------------------------------------------------ the update: stand-ins
def _numpy_step(i, hp, t, form, wrong=None):
    """The kernels' update in numpy fp32, operation by operation; `wrong` picks one of the wrong rules."""
    f = np.float32
    p, g, m, v = (i[k].numpy().copy() for k in "pgmv")
    lr, b1, b2, eps, wd = (f(x) for x in hp)
    one = f(1.0)
    tt = {"t_plus_1": t + 1, "t_minus_1": t - 1}.get(wrong, t)
    if form == "dev":
        bc1, bc2 = f(1.0 - float(b1) ** tt), f(1.0 - float(b2) ** tt)
    else:
        bc1, bc2 = one - f(float(b1) ** tt), one - f(float(b2) ** tt)          # (powf rounded once: inside its 16 ulp)
    out_bc = (bc1, bc2)
    if wrong == "no_correction":
        bc1 = bc2 = one
    if wrong == "swapped":
        bc1, bc2 = bc2, bc1
    with np.errstate(all="ignore"):
        ge = g + wd * p if wrong == "coupled_l2" else g
        m1 = b1 * m + (one if wrong == "no_one_minus_b1" else one - b1) * ge
        v1 = b2 * v + (one - b2) * (ge if wrong == "v_from_g" else ge * ge)
        mm, vv = (m, v) if wrong == "stale_moments" else (m1, v1)
        if wrong == "eps_inside":
            den = np.sqrt(vv / bc2 + eps)
        elif wrong == "eps_before_bc2":
            den = (np.sqrt(vv) + eps) / np.sqrt(bc2)
        elif wrong == "bc2_without_root":
            den = np.sqrt(vv) / bc2 + eps
        else:
            den = np.sqrt(vv / bc2) + eps
        upd = lr * (mm / bc1) / den
        if wrong == "coupled_l2":
            p1 = p - upd
        elif wrong == "decay_after":
            p1 = (p - upd) * (one - lr * wd)
        else:
            p1 = p * (one - lr * wd) - upd
    out = dict(p=torch.from_numpy(p1), m=torch.from_numpy(m1), v=torch.from_numpy(v1))
    assert all(x.dtype == torch.float32 for x in out.values())
    if form == "dev":
        out.update(bc1=torch.tensor([out_bc[0]]), bc2=torch.tensor([out_bc[1]]))
    return out


def _numpy_standin(c, wrong=None):
    return _numpy_step(O.inputs(c), O.hyper(c), c.t, c.form, wrong)


def _torch_standin(c, scalars=None):
    """torch.optim.AdamW's single-tensor CPU path from the injected state (step = t - 1, exp_avg, exp_avg_sq)."""
    i = O.inputs(c)
    lr, b1, b2, eps, wd = scalars or O.hyper(c)
    p = torch.nn.Parameter(i["p"].clone())
    p.grad = i["g"].clone()
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(c.t - 1)), exp_avg=i["m"].clone(), exp_avg_sq=i["v"].clone())
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == c.t
    return dict(p=p.detach(), m=st["exp_avg"], v=st["exp_avg_sq"])


def test_tables_are_what_the_issue_asks_for():
    assert O.N_REGIMES == 12 * 2 * 6 * 5
    want_dev = {(h, w, t, n) for h in range(3) for w in (0, 1) for t in O.STEPS for n in O.DEV_LENGTHS}
    for p16 in (O.F16, O.BF16):
        assert {(c.hp, c.wd, c.t, c.n) for c in O.CASES["adamw_dev"] if c.p16 == p16} == want_dev
    assert {(c.hp, c.wd, c.t, c.n) for c in O.CASES["adamw_dev"] if c.p16 is None} == {x for x in want_dev if x[0] == 0}
    assert {(c.hp, c.wd, c.t, c.n) for c in O.CASES["adamw"]} == {(h, w, t, n) for h in range(3) for w in (0, 1) for t in O.STEPS for n in O.HOST_LENGTHS}
    assert O.DEV_LENGTHS == (1, 3, 4, 7, 1027, 2048, 2051, 7175) and O.HOST_LENGTHS == (1, 255, 256, 257, 1027)
    assert O.HYPER[0] == (2e-5, 0.9, 0.999, 1e-8, 0.05) and O.STEPS == (1, 2, 10, 1000, 100000)
    assert math.isclose(O.U, 2.0 ** -24) and O.SUB32 == 2.0 ** -149


def test_range_rule_holds_on_every_case_and_drops_only_the_named_rows():
    p, g, m, v = O.REGIMES
    collapsed_1e15 = (g.abs() > 1e14) & (v > 1e35)
    assert int(collapsed_1e15.sum()) == 10
    for c in ALL:
        i, hp = O.inputs(c), O.hyper(c)
        assert bool(O.in_range(i["g"], i["v"], hp, c.t).all()), c
        ref = O.ref64(c)
        bc2 = float(ref["bc2"])
        assert float((ref["v"] / bc2).max()) < O.LIMIT and float((i["g"].double() ** 2).max()) < O.LIMIT, c
        assert all(bool(torch.isfinite(b).all()) and bool((b > 0).all()) for b in O.bound(c).values()), c
        dropped = set(range(O.N_REGIMES)) - set(O.kept(c).tolist())
        expect = set(torch.nonzero(collapsed_1e15).flatten().tolist()) if (c.t <= 2 and hp[2] > 0.99) else set()
        assert dropped == expect, (c, len(dropped))


def test_every_regime_lands_in_every_zone_of_the_index_map():
    seen = dict(first=set(), second=set(), tail=set())
    for c in O.CASES["adamw_dev"]:
        for zone, regimes in O.zones(c).items():
            seen[zone] |= regimes
    for zone, regimes in seen.items():
        assert regimes == set(range(O.N_REGIMES)), (zone, len(regimes))
    host = set()
    for c in O.CASES["adamw"]:
        host |= set(O.regime_of(c).tolist())
    assert host == set(range(O.N_REGIMES))
    # the elements that resolve the update: p = 0 and |p| = 1e-6 meet every |g| and every history
    p, g = O.REGIMES[0], O.REGIMES[1]
    assert int((p == 0).sum()) == O.N_REGIMES // 5 and int((p.abs() == np.float32(1e-6)).sum()) == O.N_REGIMES // 5


WORST = {}


@pytest.mark.parametrize("c", ALL, ids=_full_id)
def test_correct_standins_are_inside_every_bound(c):
    for name, out in (("numpy", _numpy_standin(c)), ("torch", _torch_standin(c))):
        fails = O.check(c, out)
        assert not fails, (name, fails)
        for k, w in O.worst(c, out).items():
            WORST[(name, c.form, k)] = max(WORST.get((name, c.form, k), 0.0), w)


def test_print_worst_standin_ratios():
    """Runs after the table (file order): what the correct stand-ins leave of the bounds, shown with -s / -rP."""
    for key, w in sorted(WORST.items()):
        print(f"correct stand-in {key[0]:5s} form {key[1]:4s} output {key[2]:3s} worst |error| / bound {w:.3f}")
    assert all(w <= 1.0 for w in WORST.values())


@pytest.mark.parametrize("hp", [0, 2])
def test_torch_with_double_betas_leaves_the_bound_at_t1(hp):
    """The deviation named in the module docstring: 1 - 0.999 against 1 - float32(0.999) is 1.3e-5 relative on bc2 at t = 1."""
    c = _case("adamw_dev", f"hp{hp}-wd1-t1-n7175-p16_f16")
    assert not O.check(c, _torch_standin(c))
    fails = O.check(c, _torch_standin(c, scalars=O.HYPER[hp]))
    assert fails and " p:" in fails[0], fails
    b2 = O.hyper(c)[2]
    assert math.isclose((1.0 - b2) / (1.0 - 0.999), 1.0 - 1.29e-5, rel_tol=2e-7)


WRONG = [
    ("eps_inside", "adamw_dev", "hp0-wd1-t1000-n7175-p16_f16"),
    ("eps_before_bc2", "adamw_dev", "hp0-wd1-t1-n7175-p16_f16"),
    ("no_correction", "adamw_dev", "hp0-wd1-t10-n7175-p16_bf16"),
    ("t_plus_1", "adamw_dev", "hp0-wd0-t1-n7175-p16_f16"),
    ("t_minus_1", "adamw_dev", "hp0-wd0-t2-n7175-p16_f16"),
    ("t_plus_1", "adamw", "hp1-wd1-t10-n1027"),
    ("t_minus_1", "adamw", "hp1-wd1-t10-n1027"),
    ("swapped", "adamw_dev", "hp0-wd1-t1-n2051-p16_bf16"),
    ("bc2_without_root", "adamw_dev", "hp0-wd1-t1-n2048-p16_f16"),
    ("coupled_l2", "adamw_dev", "hp0-wd1-t1000-n7175-p16None"),
    ("decay_after", "adamw_dev", "hp2-wd1-t1000-n7175-p16_f16"),
    ("no_one_minus_b1", "adamw_dev", "hp1-wd0-t10-n1027-p16_f16"),
    ("v_from_g", "adamw_dev", "hp1-wd1-t1000-n7175-p16_bf16"),
    ("stale_moments", "adamw_dev", "hp0-wd1-t100000-n7175-p16_f16"),
    ("stale_moments", "adamw", "hp0-wd1-t1000-n1027"),
]


@pytest.mark.parametrize("wrong,kernel,case_id", WRONG, ids=[f"{w[0]}@{w[1]}[{w[2]}]" for w in WRONG])
def test_wrong_update_rule_leaves_the_bound(wrong, kernel, case_id):
    c = _case(kernel, case_id)
    assert not O.check(c, _numpy_standin(c)), "the correct stand-in must pass where the wrong one is judged"
    fails = O.check(c, _numpy_standin(c, wrong))
    assert fails, f"{wrong}: passed the comparison on {c}"
    print(f"wrong rule {wrong:18s} rejected by {c}: {fails[0].split(': ', 1)[1][:120]}")


def test_wrong_rules_are_the_issues_list():
    assert {w[0] for w in WRONG} == {"eps_inside", "eps_before_bc2", "no_correction", "t_plus_1", "t_minus_1", "swapped", "bc2_without_root",
                                     "coupled_l2", "decay_after", "no_one_minus_b1", "v_from_g", "stale_moments"}


def test_step_terms_on_a_free_state_is_the_table():
    """`check_state` (the chained run and the class test go through it) is `check` on the same numbers."""
    c = _case("adamw_dev", "hp0-wd1-t10-n2051-p16_f16")
    i = O.inputs(c)
    out = _numpy_standin(c)
    fails, worst = O.check_state("free", {k: out[k] for k in "pmv"}, i["p"], i["g"], i["m"], i["v"], O.hyper(c), c.t)
    assert not fails and worst == {k: O.worst(c, out)[k] for k in "pmv"}
    bad = dict(out, p=out["p"] * (1 + 1e-5) + 1e-9)
    assert O.check_state("free", {k: bad[k] for k in "pmv"}, i["p"], i["g"], i["m"], i["v"], O.hyper(c), c.t)[0]


# ------------------------------------------------------------------------------------------------ cir_grads_check
CAP = 2                                                    # a two-block grid: the loop's trips at lengths a CPU test can afford
LONG = 4 * (CAP * 256 * 4 + CAP * 256 + 257) + 3           # GC_LONG_N's shape under that cap: trip 1, the u = 0 quarter, 257 float4 of u = 1, a tail


def _gc_standin(bits, scale, cap=O.GC_CAP, wrong=None):
    """cir_grads_check in numpy, following the kernel's loop: (int32 bits afterwards, the flag)."""
    n = bits.numel()
    a = bits.numpy().view(np.float32).copy()
    trip, _ = O.gc_quarter_of(n, cap)
    s = np.float32(scale)
    times = np.ones(n, dtype=np.int64)                     # how often an element is visited
    if wrong == "second_trip_skipped":
        times[trip >= 1] = 0
    elif wrong == "trip_twice":
        times[trip == 0] = 2
    elif wrong == "tail_ignored":
        times[trip < 0] = 0
    seen = times > 0
    before = a.copy()
    with np.errstate(all="ignore"):
        if s != 1.0:
            for k in (1, 2):
                a = np.where(times >= k, (a * s).astype(np.float32), a)
    x = (before if wrong == "check_before_scaling" else a)[seen]
    if wrong == "nan_only":
        bad = np.isnan(x)
    elif wrong == "inf_only":
        bad = np.isinf(x)
    elif wrong == "max_flagged":
        bad = ~(np.abs(x) < np.float32(3.4028234663852886e38))
    else:
        bad = (x.view(np.uint32) & 0x7F800000) == 0x7F800000
    return torch.from_numpy(a.view(np.int32).copy()), int(bool(bad.any()))


def test_grads_check_table_shape():
    names = {v[0] for v in O.GC_VALUES}
    assert names == {"+0", "-0", "sub_min", "sub_max", "norm_min", "+max", "-max", "+inf", "-inf", "qnan", "snan", "nan_ones"}
    assert {v[1] for v in O.GC_VALUES if v[2]} == {0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF}
    assert [s for _, s in O.GC_SCALES] == [1.0, 2.0 ** -10, 0.3, 2.0, 0.0] and math.frexp(0.3)[0] != 0.5
    # the long case, from the launch rule
    n4, blocks, stride = O.gc_grid(O.GC_LONG_N)
    assert (blocks, stride) == (8192, 8192 * 256) and 4 * stride * 4 == O.GC_TRIP == 33554432
    assert n4 == 4 * stride + stride + 257 and O.GC_LONG_N - 4 * n4 == 3
    assert O.gc_grid(O.GC_TRIP)[0] == 4 * stride                      # one float4 more enters the second trip
    # every short length stays inside one trip, and the positions reach every non-empty quarter
    for n in O.GC_LENGTHS:
        trip, u = O.gc_quarter_of(n)
        assert trip.max() <= 0
        pos = O.gc_positions(n)
        assert pos["first"] == 0 and pos["last"] == n - 1 and all(0 <= q < n for q in pos.values())
        assert {f"trip0_u{q}" for q in set(u[u >= 0].tolist())} == {k for k in pos if k.startswith("trip")}
        assert sum(k.startswith("tail") for k in pos) == n % 4
        for k, q in pos.items():
            if k.startswith("trip"):
                assert int(u[q]) == int(k[-1])
    assert {k for k in O.gc_positions(7175) if k.startswith("trip")} == {f"trip0_u{q}" for q in range(4)}
    # the scaled-down long case has the long case's structure
    trip, u = O.gc_quarter_of(LONG, CAP)
    assert {(int(a), int(b)) for a, b in zip(trip, u)} == {(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (-1, -1)}
    assert int(((trip == 1) & (u == 1)).sum()) == 4 * 257


def _gc_runs(n, cap):
    for pname, pos in O.gc_positions(n, cap).items():
        for (vname, vbits, _), (sname, scale) in ((v, s) for v in O.GC_VALUES for s in O.GC_SCALES):
            yield f"n{n}-{pname}-{vname}-x{sname}", O.gc_buffer(n, pos, vbits), scale


@pytest.mark.parametrize("n", O.GC_LENGTHS + (LONG,))
def test_grads_check_standin_passes_the_table(n):
    cap = CAP if n == LONG else O.GC_CAP
    count = 0
    for what, bits, scale in _gc_runs(n, cap):
        got, flag = _gc_standin(bits, scale, cap)
        assert not O.gc_check(what, bits, scale, got, flag), what
        assert not O.gc_check(what, bits, scale, got, 1, preset=1), what
        count += 1
    assert count == len(O.gc_positions(n, cap)) * len(O.GC_VALUES) * len(O.GC_SCALES)
    clean = O.gc_base(n).view(torch.int32)
    for _, scale in O.GC_SCALES:
        got, flag = _gc_standin(clean, scale, cap)
        assert flag == 0 and not O.gc_check("clean", clean, scale, got, flag)


def test_grads_check_expectations_by_hand():
    """The issue's statements, spelled out against gc_expected (which the table goes through)."""
    val = {v[0]: v[1] for v in O.GC_VALUES}
    for name, bits, nonfinite in O.GC_VALUES:
        buf = O.gc_buffer(7, 5, bits)
        out, flag = O.gc_expected(buf, 1.0)
        assert torch.equal(out, buf) and flag == int(nonfinite), name               # scale 1: bits untouched, payloads included
        out, flag = O.gc_expected(buf, 2.0 ** -10)
        assert flag == int(nonfinite), name
    for sign in ("+max", "-max"):
        buf = O.gc_buffer(7, 2, val[sign])
        assert O.gc_expected(buf, 2.0)[1] == 1 and O.gc_expected(buf, 0.3)[1] == 0    # the overflow the scaling makes
    buf = O.gc_buffer(7, 6, val["+inf"])
    out, flag = O.gc_expected(buf, 0.0)
    assert flag == 1 and bool(torch.isnan(out.view(torch.float32)[6]))                # inf * 0
    out, flag = O.gc_expected(O.gc_base(7).view(torch.int32), 0.0)
    assert flag == 0 and bool((out.view(torch.float32) == 0).all())
    base = O.gc_base(1027)
    out, _ = O.gc_expected(base.view(torch.int32), 0.3)
    assert torch.equal(out.view(torch.float32), base * torch.tensor(0.3, dtype=torch.float32))
    assert not torch.equal(out.view(torch.float32), (base.double() * 0.3).float())   # (the double product rounds differently somewhere)


GC_WRONG = [
    ("nan_only", 7, "tail1", "+inf", "one"),
    ("inf_only", 1027, "body_last", "snan", "one"),
    ("max_flagged", 2048, "trip0_u1", "-max", "one"),
    ("check_before_scaling", 2051, "last", "+max", "two"),
    ("check_before_scaling", 4, "first", "-max", "two"),
    ("second_trip_skipped", LONG, "trip1_u1", "+inf", "one"),
    ("second_trip_skipped", LONG, "trip1_u0", "+0", "0.3"),
    ("trip_twice", LONG, "trip0_u2", "+0", "0.3"),
    ("tail_ignored", 7175, "tail2", "qnan", "one"),
    ("tail_ignored", 3, "tail0", "+0", "2^-10"),
]


@pytest.mark.parametrize("wrong,n,pname,vname,sname", GC_WRONG, ids=[f"{w[0]}@n{w[1]}-{w[2]}-{w[3]}-x{w[4]}" for w in GC_WRONG])
def test_wrong_grads_check_fails(wrong, n, pname, vname, sname):
    cap = CAP if n == LONG else O.GC_CAP
    bits = O.gc_buffer(n, O.gc_positions(n, cap)[pname], {v[0]: v[1] for v in O.GC_VALUES}[vname])
    scale = dict(O.GC_SCALES)[sname]
    assert not O.gc_check("correct", bits, scale, *_gc_standin(bits, scale, cap))
    fails = O.gc_check(wrong, bits, scale, *_gc_standin(bits, scale, cap, wrong))
    assert fails, wrong
    print(fails[0])


def test_wrong_grads_check_forms_are_the_issues_list():
    assert {w[0] for w in GC_WRONG} == {"nan_only", "inf_only", "max_flagged", "check_before_scaling", "second_trip_skipped", "trip_twice", "tail_ignored"}


# ------------------------------------------------------------------------------------------------ train_core.loss_scale
def _amax_values():
    vals = [10.0 ** e for e in range(-30, 31)] + [3.0 * 10.0 ** e for e in range(-30, 30, 3)] + [2.0 ** e for e in range(-126, 100, 7)]
    vals += [2.0 ** -149, 2.0 ** -140, 1e-40, 1e-45, float(np.finfo(np.float32).max), 512.0, 1.0, 65504.0]
    return vals


def test_loss_scale_is_a_power_of_two_that_puts_amax_near_512():
    from candidate_reranking_cir_amd.train_core import loss_scale
    lo, hi = 512.0 / math.sqrt(2.0), 512.0 * math.sqrt(2.0)
    for amax in _amax_values():
        s = loss_scale(amax)
        assert s > 0 and math.frexp(s)[0] == 0.5, (amax, s)
        assert lo * (1 - 1e-12) <= amax * s <= hi * (1 + 1e-12), (amax, s, amax * s)
    for e in range(-60, 61):                               # exact powers of two land on 512 itself
        assert loss_scale(2.0 ** e) * 2.0 ** e == 512.0


def test_loss_scale_half_way_points_follow_pythons_round():
    """log2(512 / amax) = k + 1/2 exactly at amax = 512 / 2^(k + 1/2) only up to rounding; what IS exact: the scale is 2^round(x) for the x
    the function computes, so it sits on either side of the half-way point as Python's round (half to even) sends x."""
    from candidate_reranking_cir_amd.train_core import loss_scale
    for k in range(-20, 21):
        for amax in (512.0 / 2.0 ** (k + 0.5), np.nextafter(512.0 / 2.0 ** (k + 0.5), 0.0), np.nextafter(512.0 / 2.0 ** (k + 0.5), 1e9)):
            amax = float(amax)
            x = math.log2(512.0 / amax)
            assert loss_scale(amax) == 2.0 ** round(x), (k, amax)
            assert abs(x - (k + 0.5)) < 1e-9 and loss_scale(amax) in (2.0 ** k, 2.0 ** (k + 1))
            if x == k + 0.5:                               # an exact tie goes to the even exponent
                assert loss_scale(amax) == 2.0 ** (k if k % 2 == 0 else k + 1)
    assert round(0.5) == 0 and round(1.5) == 2 and round(-0.5) == 0


@pytest.mark.parametrize("amax", [0.0, -0.0, math.inf, -math.inf, math.nan, -1.0, -1e-30])
def test_loss_scale_of_a_useless_amax_is_one(amax):
    from candidate_reranking_cir_amd.train_core import loss_scale
    assert loss_scale(amax) == 1.0
