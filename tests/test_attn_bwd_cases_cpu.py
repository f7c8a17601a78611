"""tests/attn_bwd_cases.py checked without a GPU.  `attn_bwd_cases.emulate`, a torch fp32 model of tattn_fwd_kernel, tattn_bwd_dq_kernel
and tattn_bwd_dkv_kernel, stands in for the kernels: every correct form (the kernels as they are, fp16 subnormals flushed, the unrounded
p inside dS) must pass `attn_bwd_cases.check` on EVERY case - no GPU failure can be blamed on a bound that was too tight - and every wrong
form must fail it on named cases - the bounds are not so loose that a wrong row, column, mask or scale passes.  The case table is kept
honest: the dropout masks reach the ragged tiles, the idle-wave cases have idle waves, the loss-scaled case stays in fp16's range."""
import pytest
import torch

from tests import attn_bwd_cases as B

BF16, F16 = B.BF16, B.F16


# ------------------------------------------------------------------------------------------------ correct stand-ins pass everywhere
def test_correct_emulations_pass_every_case():
    worst = {}
    for c in B.CASES:
        e = float(B.second_order_ok(c).max())
        assert e <= 0.05, f"{c}: E = {e:.3g}: the second-order factor of the bound does not cover this case"
        for variant in B.CORRECT:
            out = B.emulate(c, variant)
            fails = B.check(c, out)
            assert not fails, (variant, fails)
            for name, w in B.worst_ratio(c, out).items():
                key = (variant, name, B.DT_NAME[c.dt], "p>0" if c.p > 0 else "p=0")
                worst[key] = max(worst.get(key, 0.0), w)
    print("\nlargest error / bound of the correct stand-ins:")
    for variant in B.CORRECT:
        for dt in ("bf16", "f16"):
            for p in ("p=0", "p>0"):
                print(f"  {variant:10s} {dt:4s} {p}: " + "  ".join(f"{n} {worst[(variant, n, dt, p)]:.2f}" for n in B.OUTPUTS))
    assert max(worst.values()) < 1.0


# ------------------------------------------------------------------------------------------------ wrong stand-ins are caught
# variant -> the case ids it must fail on (no_centre: EVERY case, below)
CAUGHT_ON = {
    "mask_shift": ["33x100-dt_bf16-tail-p0.0-t16", "70x197-dt_f16-front-p0.1-t16", "33x100-dt_f16-tail40-p0.1-t16", "9x9-dt_bf16-min_tail-p0.1-t16"],
    "drop_last": ["9x9-dt_bf16-none-p0.0-t16", "64x65-dt_f16-none-p0.1-t16", "70x197-dt_bf16-front-p0.1-t16"],
    "pad_query": ["33x100-dt_bf16-none-p0.0-t16", "9x9-dt_f16-tail-p0.1-t16", "70x197-dt_f16-none-p0.1-t16"],
    "pad_key": ["9x9-dt_bf16-none-p0.0-t16", "64x65-dt_f16-none-p0.1-t16", "70x197-dt_bf16-none-p0.1-t16", "33x100-dt_f16-front-p0.0-t16"],
    "dkv_row_slip": ["33x100-dt_bf16-none-p0.1-t16", "9x9-dt_f16-none-p0.1-t16", "70x197-dt_f16-tail-p0.1-t16", "32x32-dt_bf16-none-p0.1-t16"],
    "dq_col_parity": ["33x100-dt_bf16-none-p0.1-t16", "70x197-dt_f16-none-p0.1-t16", "9x9-dt_f16-none-p0.1-t16", "32x32-dt_bf16-tail-p0.1-t16"],
    "dropped_no_D": ["33x100-dt_bf16-none-p0.25-t16", "70x197-dt_f16-none-p0.1-t16", "9x9-dt_bf16-tail-p0.1-t16"],
    "dk_scale_twice": ["9x9-dt_bf16-none-p0.0-t16", "70x197-dt_f16-none-p0.1-t16"],
    "grad16_cols": ["9x9-dt_bf16-none-p0.0-t16", "33x100-dt_f16-none-p0.1-t16", "1x1-dt_f16-none-p0.0-t16"],
}


def test_every_wrong_variant_is_listed():
    assert set(CAUGHT_ON) | {"no_centre"} == set(B.WRONG)


@pytest.mark.parametrize("variant", list(CAUGHT_ON))
def test_wrong_emulations_fail(variant):
    for cid in CAUGHT_ON[variant]:
        c = B.case(cid)
        assert B.check(c, B.emulate(c, variant)), f"{c}: the wrong stand-in `{variant}` passed the comparison"


def test_missing_centre_correction_fails_on_every_case():
    """corr = 0 - the defect test_training_attention_backward_profiles found at norm granularity: key column 1 is the constant 1 on
    every key of every case, so the residue of sum_j ds16_j lands in dQ[:, 1] undiminished and every case notices, element by element."""
    for c in B.CASES:
        fails = B.check(c, B.emulate(c, "no_centre"))
        assert fails and all(" dq:" in f for f in fails), (c, fails)


def test_no_twin_form_under_the_twin_bound():
    """D = rowsum(dO * O) from the 16-bit O (`no_twin_as_twin` on a t32 case = the n32 case's computation, bit for bit) against the TWIN's
    bound.  The two forms have two bounds - the no-twin one is larger by the rounding of O in dD - but against float64 the twin is not
    the more accurate form: its O carries the forward's 16-bit rounding of P (r_f in b_O) either way, which is as large as the rounding
    of O itself; what the twin buys is that D equals sum_j pd16_ij G_ij term for term (zero row sums of dS), which the centre
    correction of the dQ kernel now supplies for dQ anyway.  So an elementwise float64 bound cannot tell the forms apart, and this test
    only pins the relation of the two bounds and prints how far inside the twin's bound the no-twin form stays (measured: <= 0.32)."""
    worst = 0.0
    for twin_case in [c for c in B.CASES if c.form == "t32"]:
        plain = B.case(twin_case.id.replace("t32", "n32"))
        out = B.emulate(plain, "kernel")
        assert not B.check(plain, out)
        same = B.emulate(twin_case, "no_twin_as_twin")
        assert all(torch.equal(out[n], same[n]) for n in B.OUTPUTS)
        wide = {n: b.clone() for n, b in B.bound(plain).items()}
        for n in ("dq", "dk"):
            assert bool((wide[n] >= B.bound(twin_case)[n]).all()) and (twin_case.shape == (1, 1) or bool((wide[n] > B.bound(twin_case)[n]).any()))
        w = B.worst_ratio(twin_case, same)
        worst = max(worst, w["dq"], w["dk"])
    print(f"\nno-twin D under the twin's bound: largest error / bound of dQ, dK {worst:.2f}")


# ------------------------------------------------------------------------------------------------ the case table reaches what it claims
def test_table_covers_the_axes():
    ids = [c.id for c in B.CASES]
    assert len(set(ids)) == len(ids)
    for form in B.FORMS:
        for s in B.SHAPES:
            for dt in (BF16, F16):
                assert {c.p for c in B.CASES if (c.form, c.shape, c.dt) == (form, s, dt)} >= {0.0, 0.1}, (form, s, dt)
    full = [c for c in B.CASES if c.form == "t16"]
    for s in B.SHAPES:
        for dt in (BF16, F16):
            for p in (0.0, 0.1):
                assert {c.mask for c in full if (c.shape, c.dt, c.p) == (s, dt, p)} >= set(B.masks_at(s[1])), (s, dt, p)
    assert {c.mask for c in full if c.shape == (33, 100)} >= {"tail40", "all10k"} and any(c.p == 0.25 for c in full if c.shape == (33, 100))
    assert any(c.shape == (32, 32) and c.mask == "none" for c in full)                  # the dQ kernel's edge == false branch
    seeds = {B.seed_of(c) for c in B.CASES if c.p > 0}
    assert len(seeds) == 2 and any(s >> 32 for s in seeds) and all(s < 2 ** 63 for s in seeds)
    for dt in (BF16, F16):
        assert {B.seed_of(c) for c in B.CASES if c.p > 0 and c.dt == dt} == seeds


def test_masks_mask_something_and_leave_something():
    for c in B.CASES:
        m = B.inputs(c)["mask"]
        if c.mask == "none":
            assert m is None
        elif c.mask == "all10k":
            rows = (m == -10000.0).all(-1)
            assert bool(rows.any()) and not bool(rows.all()) and bool((m[~rows] == 0).all())
        elif c.mask == "min_all":
            assert bool((m == torch.finfo(torch.float32).min).all())
        else:
            assert bool((m < 0).any(-1).all()) and bool((m == 0).any(-1).all()), c


def test_dropout_reaches_the_ragged_tiles():
    """Every case with p > 0 has a dropped AND a kept element in the last (ragged) key tile and in the last (ragged) query tile - the
    index formulas of the two backward kernels are exercised where they differ from a full tile."""
    for c in B.CASES:
        if c.p == 0:
            assert bool(B.inputs(c)["keep"].all())
            continue
        lq, lk = c.shape
        keep = B.inputs(c)["keep"]
        for name, part in (("key", keep[:, :, (lk - 1) // 32 * 32:]), ("query", keep[:, (lq - 1) // 32 * 32:, :])):
            assert bool(part.any()) and not bool(part.all()), f"{c}: the last {name} tile holds no dropped or no kept element"
        share = 1.0 - float(keep.double().mean())
        assert abs(share - c.p) < 5 * (c.p * (1 - c.p) / keep.numel()) ** 0.5 + 1e-9 or keep.numel() < 64, (c, share)


def test_idle_wave_cases_have_idle_waves():
    sub = [c for c in B.CASES if getattr(c, "items", "all") == "sub7"]
    assert {c.shape for c in sub} == {(33, 100), (9, 9)} and {c.dt for c in sub} == {BF16, F16}
    for c in B.CASES:
        g, h, idx = B.layout(c)
        nqt, nkt = (c.shape[0] + 31) // 32, (c.shape[1] + 31) // 32
        assert len(idx) == g * h and B.inputs(c)["q"].shape[0] == g * h
        if c in sub:
            assert (g * h * nqt) % 4 != 0, c                        # forward and dQ launches: the last workgroup has idle waves
            if c.shape == (9, 9):
                assert (g * h * nkt) % 4 != 0, c                    # and the dK / dV launch
        else:
            assert (g * h * nqt) % 4 == 0 and (g * h * nkt) % 4 == 0, c


def test_loss_scaled_case_stays_in_range():
    """fp16 with dO at the trainers' loss scale: max |dO| in [256, 512), and the REFERENCE's dS / scale and dO.V stay below 2^15, the
    gradients (with their bounds) below fp16's largest number - so the kernel has no excuse for an overflow."""
    loss = [c for c in B.CASES if getattr(c, "do", None) == "loss"]
    assert loss and all(c.dt == F16 for c in loss) and {c.p for c in loss} == {0.0, 0.1}
    for c in loss:
        top = float(B.inputs(c)["do"].double().abs().max())
        assert 256.0 <= top < 512.0, top
        t = B.terms(c)
        assert t["ds_max"] < 2.0 ** 15 and t["g_max"] < 2.0 ** 15, (t["ds_max"], t["g_max"])
        for n in ("dq", "dk", "dv"):
            assert float((t["ref"][n].abs() + t["bound"][n]).max()) < 65504.0, n


def test_single_element_and_dropped_rows():
    """(1, 1): P = 1, dS = 0 exactly, dV = w dO; with dropout some of the 16 rows lose their only key - the all-dropped row of the dQ
    kernel (no centre, corr = 0) is reached."""
    for c in B.CASES:
        if c.shape != (1, 1):
            continue
        r = B.ref64(c)
        assert float(r["dq"].abs().max()) < 1e-12 and float(r["dk"].abs().max()) < 1e-12        # (float64 rounding of w G - D)
        if c.p > 0:
            keep = B.inputs(c)["keep"]
            assert bool((~keep).any()) and bool(keep.any())
            assert bool((r["dv"][~keep[:, 0, 0]] == 0).all()) and bool((r["out"][~keep[:, 0, 0]] == 0).all())
