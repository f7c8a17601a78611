"""tests/attn_cases.py checked without a GPU.  `attn_cases.emulate`, a torch fp32 tile-by-tile model of the kernels' online softmax,
stands in for the kernels: both correct forms (the lazy vote of softmax_tile, the rescale on every tile of the other kernels) must pass
`attn_cases.check` on EVERY case - no GPU failure can be blamed on a bound that was too tight - and every wrong form must fail it on a
named case - the bounds are not so loose that the obvious mistakes pass.  The case table is kept honest: the random inputs of the older
attention tests never reach the late-rescale branch, the dialled profiles always do."""
import pytest
import torch

from tests import attn_cases as A

BF16, F16, F32 = A.BF16, A.F16, A.F32


def _case(kernel, case_id):
    return next(c for c in A.CASES[kernel] if c.id == case_id)


# ------------------------------------------------------------------------------------------------ correct stand-ins pass everywhere
@pytest.mark.parametrize("kernel", list(A.CASES))
def test_correct_emulations_pass_every_case(kernel):
    worst = {}
    for c in A.CASES[kernel]:
        e = float(A.second_order_ok(c).max())
        assert e <= 0.05, f"{c}: E = {e:.3g}: the second-order factor of the bound does not cover this case"
        for variant in A.CORRECT:
            out = A.emulate(c, variant)
            fails = A.check(c, out)
            assert not fails, (variant, fails)
            for name, w in A.worst_ratio(c, out).items():
                key = (variant, name, A.DT_NAME[c.dt])
                worst[key] = max(worst.get(key, 0.0), w)
    print(f"\n[{kernel}] largest error / bound of the correct stand-ins: " + "  ".join(f"{'/'.join(k)} {w:.2f}" for k, w in sorted(worst.items())))
    assert max(worst.values()) < 1.0


# ------------------------------------------------------------------------------------------------ wrong stand-ins are caught
# variant -> the cases (kernel, id) it must fail on
CAUGHT_ON = {
    "drop_last": [("attention", "shared_wide-dt_bf16-none"), ("attention", "stream_ragged-dt_f16-none"), ("cls", "d128-n197-dt_bf16-none"),
                  ("train", "9x9-dt_bf16-none")],
    "pad_key": [("attention", "shared_wide-dt_bf16-none"), ("attention", "shared_plain_lds-dt_f16-none"), ("attention_f32", "33x100-dt_f32-none")],
    "no_l_rescale": [("attention", "shared_wide-dt_bf16-none"), ("attention", "stream_long-dt_f16-tail")],
    "vote_rows_only": [("attention", "shared_wide-dt_bf16-none"), ("attention", "shared_2rounds-dt_f16-none")],
    "mask_shift": [("attention", "shared_wide-dt_bf16-tail"), ("attention", "stream_1tile-dt_f16-tail40"), ("train", "33x100-dt_f16-tail")],
    "alpha_after_move": [("attention", "shared_wide-dt_bf16-none"), ("train", "70x197-dt_bf16-none")],
    "mask_unclamped": [("attention", "shared_wide-dt_bf16-min_all"), ("attention_f32", "70x197-dt_f32-min_all")],
    "p_unscaled_tail": [("attention", "shared_wide-dt_f16-none")],
}


def test_every_wrong_variant_is_listed():
    assert set(CAUGHT_ON) | {"ge_no_move"} == set(A.WRONG)          # ge_no_move: test_ge_without_moving_the_reference_is_caught


@pytest.mark.parametrize("variant", list(CAUGHT_ON))
def test_wrong_emulations_fail(variant):
    for kernel, cid in CAUGHT_ON[variant]:
        c = _case(kernel, cid)
        assert A.check(c, A.emulate(c, variant)), f"{c}: the wrong stand-in `{variant}` passed the comparison"


def test_ge_without_moving_the_reference_is_caught():
    """The threshold itself: on `exact_step_inputs` the second tile's maximum exceeds the reference by exactly 6.  `>` does not rescale
    (no late rescale, P = 64 at the stale reference) and stays inside the bound; a vote on `>=` that multiplies by alpha without moving
    the reference of the rows on the equality is outside it."""
    for dt in (BF16, F16):
        q, k, v = A.exact_step_inputs(dt)
        t = A.core_terms(q, k, v, None, dt)
        b = A.out_bound(t["out"], t["b32"], dt)
        stats = {}
        good = A.emulate_core(q, k, v, None, dt, "lazy", stats)["out32"].to(dt).double()
        assert int(stats["late"].sum()) == 0 and abs(float(t["out"][0, 0, 0]) - 32.0 / 127.0) < 1e-6      # weights 32 x 1, 1 x 64, 31 x 1
        assert bool(((good - t["out"]).abs() <= b).all())
        bad = A.emulate_core(q, k, v, None, dt, "ge_no_move")["out32"].to(dt).double()
        assert not bool(((bad - t["out"]).abs() <= b).all())


# ------------------------------------------------------------------------------------------------ the case table reaches the branch
def test_random_inputs_never_rescale_late():
    """The inputs of test_ops_gpu.py::test_attention_shapes at 197 x 197 (randn q, k, v; seeds 1, 2, 3): behind the first key tile no
    32-row tile ever takes softmax_tile's rescale branch - which is why this file's profiles exist."""
    b1, b0, h, n = 3, 2, 2, 197
    for dt in (BF16, F16):
        q, k, v = (torch.randn((b1, b0, n, h * 64), generator=torch.Generator(device="cpu").manual_seed(s)).to(dt) for s in (1, 2, 3))
        items = lambda t: t.view(b1 * b0, n, h, 64).permute(0, 2, 1, 3).reshape(b1 * b0 * h, n, 64)      # noqa: E731
        stats = {}
        A.emulate_core(items(q), items(k), items(v), None, dt, "lazy", stats)
        assert int(stats["late"].sum()) == 0


def test_profiles_rescale_late_beside_a_uniform_row():
    """Every ramp, step, saw and spike_last item of every 16-bit cir_attention case with two tiles of valid keys takes the late
    rescale in EVERY 32-row query tile - and every query tile holds a gain-0 (uniform) row, which the vote drags along."""
    counts = {}
    for c in A.CASES["attention"]:
        if not A.late_rescale_expected(c):
            continue
        lq = A.shape(c)[0]
        stats = {}
        A.emulate(c, "lazy", stats)
        late = stats["late"]                                         # (NP * H, nqt)
        for n in range(late.shape[0]):
            name = A.PROFILES[n // A.H]
            gains = torch.tensor(A.GAINS)[(torch.arange(lq) + 4 * (n % A.H)) % 8]
            for qt in range(late.shape[1]):
                assert bool((gains[32 * qt:32 * qt + 32] == 0).any()), f"{c}: query tile {qt} holds no uniform row"
            if name in A.LATE_PROFILES or c.mask == "front":
                assert bool((late[n] >= 1).all()), f"{c} {name} head {n % A.H}: late rescales per query tile {late[n].tolist()}"
            if c.mask == "none":
                counts.setdefault((name, A.shape(c)[1]), set()).add(int(late[n].max()))
    print("\nlate rescales per profile (unmasked; Lk: largest count over query tiles): " +
          "  ".join(f"{p}@{lk}: {sorted(v)}" for (p, lk), v in sorted(counts.items())))


# ------------------------------------------------------------------------------------------------ the bound is not vacuous
def test_p_rounding_term_is_attained():
    """Two keys, v = (0, 1), random score gaps: the only error of the fp32 context is the rounding of P(key 1) to the operand type (l
    sums the unrounded values).  Over 512 rows the correct stand-in comes within a factor 2 of the P-rounding term of the bound - the
    term cannot be halved - and never exceeds the whole bound."""
    for dt in (BF16, F16):
        g = torch.Generator(device="cpu").manual_seed(A.PREC[dt])
        q = torch.zeros((1, 512, 64), dtype=torch.float64)
        q[0, :, 0] = torch.rand((512,), generator=g, dtype=torch.float64) * 16
        k = torch.zeros((1, 2, 64), dtype=torch.float64)
        k[0, 0, 0] = 1.0                                             # key 0 leads by up to 2 nats: P(key 1) in (2^-2.9, 1)
        v = torch.zeros((1, 2, 64), dtype=torch.float64)
        v[0, 1, :] = 1.0
        q, k, v = q.to(dt), k.to(dt), v.to(dt)
        t = A.core_terms(q, k, v, None, dt)
        err = (A.emulate_core(q, k, v, None, dt, "lazy")["out32"].double() - t["out"]).abs()
        assert bool((err <= t["b32"]).all())
        ratio = float((err / t["p_term"]).max())
        print(f"\n[{A.DT_NAME[dt]}] largest error / P-rounding term: {ratio:.3f}")
        assert 0.5 <= ratio <= 1.0 + 2.0 ** -10
