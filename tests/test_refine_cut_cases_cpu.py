"""The selective rank-refinement rule on the host (tests/refine_cut_cases.py): its two restatements agree, its guarantee - the first places
in order, the sets before every cut - holds on thousands of random rows whose fast values lie within the margin of the referee's, the full
rule is its special case and its superset, and on the separated-logit profile it selects a small share of what the full rule selects."""
import numpy as np
import pytest

from tests import refine_cases as R
from tests import refine_cut_cases as C

F32 = np.float32


def test_the_two_restatements_agree():
    rng = np.random.default_rng(11)
    rows = n_sel = n_partial = 0
    seen_first, seen_cuts = set(), set()
    while rows < 1500:
        k = int(rng.choice([1, 2, 3, 5, 8, 33, 100, 105]))
        margin = float(rng.choice([0.0, 1e-4, 3e-3, 0.05, 0.5]))
        scale = float(rng.choice([0.02, 0.3, 3.0]))
        offset = float(rng.choice([0.0, 0.0, 1e5, -1e5]))
        fast, _ = R.theorem_row(rng, k, margin, scale, offset, ties=int(rng.integers(3)), specials=int(rng.integers(2)))
        if rng.integers(20) == 0:
            fast[:] = fast[0]                                               # an all-equal row
        full = R.undecided_links(fast, margin)[0]
        grid = C.selection_grid(k)
        for first, cuts in grid:
            a = C.selected_links(fast, margin, first, cuts)
            b = C.selected_pairs(fast, margin, first, cuts)
            assert np.array_equal(a, b), (fast, margin, first, cuts)
            assert not (a & ~full).any()                                    # a subset of the full rule
            n_sel += int(a.sum())
            n_partial += int(0 < a.sum() < full.sum())
            seen_first.add(first - k)
            seen_cuts.add(len(cuts))
        rows += 1
    assert n_sel > 1000 and n_partial > 100
    assert {-1, 0, 7} <= seen_first and {0, 1, 2, 8} <= seen_cuts


@pytest.mark.parametrize("k", [1, 2, 5, 100])
def test_the_whole_grid_on_edge_rows(k):
    rng = np.random.default_rng(k)
    rows = [np.full(k, 0.25, dtype=F32), (0.01 * rng.standard_normal(k)).astype(F32), np.arange(k, dtype=F32)]
    special = (0.01 * rng.standard_normal(k)).astype(F32)
    special[::3] = np.nan
    special[1::5] = np.inf
    special[2::7] = -np.inf
    rows.append(special)
    for row in rows:
        for margin in (0.0, 0.004, 10.0):
            full = R.undecided_links(row, margin)[0]
            for first, cuts in C.selection_grid(k):
                a = C.selected_links(row, margin, first, cuts)
                assert np.array_equal(a, C.selected_pairs(row, margin, first, cuts)), (row, margin, first, cuts)
                assert not (a & ~full).any()
                if first >= k:
                    assert np.array_equal(a, full)                          # today's rule
                if first == 0 and all(c >= k for c in cuts):
                    assert not a.any()                                      # a cut at or beyond K selects nothing


def test_first_at_or_beyond_k_is_the_full_rule():
    for rng, k, margin, scale, offset in ((np.random.default_rng(s), k, m, 0.3, 0.0) for s, k, m in
                                          [(1, 1, 0.1), (2, 2, 0.1), (3, 33, 3e-3), (4, 100, 0.0), (5, 105, 0.05), (6, 100, 1e-3)]):
        for _ in range(50):
            fast, _ = R.theorem_row(rng, k, margin, scale, offset, ties=2 if k > 2 else 0, specials=1 if k > 2 else 0)
            want = R.undecided_links(fast, margin)[0]
            for first in (k, k + 7):
                assert np.array_equal(C.selected_links(fast, margin, first), want)
                assert np.array_equal(C.selected_links(fast, margin, first, (1, k + 9)), want)
            assert np.array_equal(C.hybrid(fast, fast + F32(1), margin, k).view(np.int32), R.hybrid(fast, fast + F32(1), margin).view(np.int32))


def test_guarantee_on_random_rows():
    partial = with_cuts = 0
    for rng, k, margin, scale, offset, first, cuts in C.theorem_rows(2, 4000):
        fast, ref = R.theorem_row(rng, k, margin, scale, offset, ties=int(rng.integers(3)), specials=int(rng.integers(3)) if k > 2 else 0)
        finite = np.isfinite(ref)
        assert np.all(np.abs(fast[finite].astype(np.float64) - ref[finite].astype(np.float64)) <= float(F32(margin)))     # the premise
        assert C.guarantee_holds(fast, ref, margin, first, cuts), (fast, ref, margin, first, cuts)
        sel, full = C.selected_links(fast, margin, first, cuts), R.undecided_links(fast, margin)[0]
        partial += int(0 < sel.sum() < full.sum())
        with_cuts += int(any(c < k for c in cuts))
    assert partial > 300 and with_cuts > 1000          # rows where the selection is neither empty nor the full rule: what the rule is for


@pytest.mark.parametrize("magnitude", [1e5, -1e5])
def test_guarantee_where_an_ulp_exceeds_the_margin(magnitude):
    """Near 1e5 an fp32 ulp is 0.0078: margins below, at and above it; many entries collide after rounding.  1000 rows per sign."""
    rng = np.random.default_rng(3)
    selections = [(0, (1, 5, 10, 50)), (10, (50,)), (50, ()), (5, (10,)), (0, (63,)), (1, ()), (63, (1, 2, 3, 4, 5, 6, 7, 8))]
    for margin in (0.0, 0.002, 0.0039, 0.0078125, 0.02):
        for i in range(200):
            fast, ref = R.theorem_row(rng, 64, margin, 0.05, magnitude)
            first, cuts = selections[i % len(selections)]
            assert C.guarantee_holds(fast, ref, margin, first, cuts), (fast, ref, margin, first, cuts)


def test_a_cluster_is_selected_by_where_it_starts_and_what_it_straddles():
    d = 0.125
    # sorted: 12 | 8 7.5 | 4 | 1 0.5 0 | -4 (times d; linked iff at most 2 d apart)    places: 0 | 1 2 | 3 | 4 5 6 | 7
    row = np.array([0.0, 8.0, 4.0, 12.0, 1.0, 7.5, -4.0, 0.5], dtype=F32) * F32(d)
    sel = lambda first, cuts=(): sorted(np.where(C.selected_links(row, d, first, cuts))[0].tolist())
    a, b = [1, 5], [0, 4, 7]
    assert sel(0) == [] and sel(1) == [] and sel(2) == a and sel(4) == a
    assert sel(5) == sorted(a + b) and sel(8) == sorted(a + b)
    assert sel(0, (1,)) == [] and sel(0, (2,)) == a and sel(0, (3,)) == [] and sel(0, (4,)) == []
    assert sel(0, (5,)) == b and sel(0, (6,)) == b and sel(0, (7,)) == [] and sel(0, (2, 6)) == sorted(a + b)
    assert sel(0, (8,)) == [] and sel(0, (1, 3, 4, 7, 8, 9, 10, 11)) == []


def test_shares_on_the_separated_logit_profile():
    """2000 rows of 100 fp32 N(0, 0.14^2) values, seed 0, at text32's margin with safety 2 (8.726e-4): the bands are set around the values the
    rule's first restatement gave when the feature was proposed (0.483 / 0.248 / 0.036; cuts 1, 5, 10, 50 alone: 0.020)."""
    rows = C.profile_rows()
    margin = 8.726e-4
    share = lambda first, cuts=(): float(np.mean([C.selected_links(r, margin, first, cuts).mean() for r in rows]))
    full = float(np.mean([R.undecided_links(r, margin)[0].mean() for r in rows]))
    first50, first10_cut50, cuts_only = share(50), share(10, (50,)), share(0, (1, 5, 10, 50))
    print(f"shares: full {full:.3f}  first=50 {first50:.3f}  first=10 cuts=(50,) {first10_cut50:.3f}  cuts (1, 5, 10, 50) {cuts_only:.3f}")
    assert 0.45 < full < 0.52
    assert 0.22 < first50 < 0.28
    assert first10_cut50 < 0.06
    assert 0 < cuts_only < first10_cut50 < first50 < full
