"""The rank-refinement rule on the host (tests/refine_cases.py): its two restatements agree, the theorem - if |fast - referee| <= margin on
every entry of a row, the refined row sorts exactly as the referee's - holds on thousands of random rows with the awkward cases in, and a
chain of gaps below 2 * margin is one cluster.  Also the argument contract of the two entry points, which needs no GPU."""
import numpy as np
import pytest

from tests import refine_cases as R

F32 = np.float32


def _rows(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        k = int(rng.choice([1, 2, 3, 5, 8, 33, 100, 105]))
        margin = float(rng.choice([0.0, 1e-4, 3e-3, 0.05, 0.5]))
        scale = float(rng.choice([0.02, 0.3, 3.0]))
        offset = float(rng.choice([0.0, 0.0, 1e5, -1e5]))
        yield rng, k, margin, scale, offset


def test_the_two_restatements_agree():
    n_und = 0
    for rng, k, margin, scale, offset in _rows(1, 1500):
        fast, _ = R.theorem_row(rng, k, margin, scale, offset, ties=int(rng.integers(3)), specials=int(rng.integers(2)))
        a, ca = R.undecided_links(fast, margin)
        b, cb = R.undecided_pairs(fast, margin)
        assert np.array_equal(a, b) and R.same_partition(ca, cb), (fast, margin)
        n_und += int(a.sum())
    assert n_und > 1000


def test_theorem_on_random_rows():
    mixed = 0
    for rng, k, margin, scale, offset in _rows(2, 4000):
        fast, ref = R.theorem_row(rng, k, margin, scale, offset, ties=int(rng.integers(3)), specials=int(rng.integers(3)) if k > 2 else 0)
        finite = np.isfinite(ref)
        assert np.all(np.abs(fast[finite].astype(np.float64) - ref[finite].astype(np.float64)) <= float(F32(margin)))     # the premise
        und = R.undecided_links(fast, margin)[0]
        mixed += int(0 < und.sum() < k)
        assert np.array_equal(R.order_desc(R.hybrid(fast, ref, margin)), R.order_desc(ref)), (fast, ref, margin)
    assert mixed > 500                      # rows with both decided and undecided entries: the case the rule exists for


@pytest.mark.parametrize("magnitude", [1e5, -1e5])
def test_theorem_where_an_ulp_exceeds_the_margin(magnitude):
    """Near 1e5 an fp32 ulp is 0.0078: margins below, at and above it; many entries collide after rounding."""
    assert float(np.spacing(F32(1e5))) == 0.0078125
    rng = np.random.default_rng(3)
    for margin in (0.0, 0.002, 0.0039, 0.0078125, 0.02):
        for _ in range(200):
            fast, ref = R.theorem_row(rng, 64, margin, 0.05, magnitude)
            assert np.array_equal(R.order_desc(R.hybrid(fast, ref, margin)), R.order_desc(ref))


def test_theorem_edge_rows():
    one = np.array([0.25], dtype=F32)
    assert not R.undecided_links(one, 0.5)[0].any() and np.array_equal(R.order_desc(R.hybrid(one, one + F32(0.5), 0.5)), [0])
    fast, ref = np.array([1.0, 1.5], dtype=F32), np.array([1.25, 1.25], dtype=F32)          # K = 2: the referee ties what fast ordered
    assert R.undecided_links(fast, 0.25)[0].all() and np.array_equal(R.order_desc(R.hybrid(fast, ref, 0.25)), [0, 1])
    assert not R.undecided_links(fast, 0.2)[0].any()
    same = np.full(7, -3.5, dtype=F32)                                                      # an all-equal row: one cluster at any margin, 0 included
    und, cluster = R.undecided_links(same, 0.0)
    assert und.all() and len(set(cluster)) == 1
    ref = same + np.array([0, 1, -1, 0, 2, 0, -2], dtype=F32) * F32(0.0)                    # margin 0: the referee equals the fast row
    assert np.array_equal(R.order_desc(R.hybrid(same, ref, 0.0)), np.arange(7))
    # margin 0: exact ties are undecided, everything else is decided
    row = np.array([2.0, 1.0, 2.0, 0.5, np.nan, -np.inf, np.inf, np.inf], dtype=F32)
    und = R.undecided_links(row, 0.0)[0]
    assert np.array_equal(und, [True, False, True, False, False, False, False, False])     # inf - inf and -inf - -inf are not numbers
    assert np.array_equal(R.order_desc(row), [6, 7, 0, 2, 1, 3, 4, 5])


def test_a_chain_is_one_cluster():
    d = 0.125
    row = np.array([0.0, 1.5 * d, 3.0 * d, 4.5 * d], dtype=F32)
    for und, cluster in (R.undecided_links(row, d), R.undecided_pairs(row, d)):
        assert und.all() and len(set(cluster.tolist())) == 1
    row = np.array([0.0, 1.5 * d, 3.75 * d, 4.5 * d, 9.0 * d], dtype=F32)                   # a gap of 2.25 d splits it; the last entry is decided
    und, cluster = R.undecided_links(row, d)
    assert np.array_equal(und, [True, True, True, True, False]) and cluster[0] == cluster[1] != cluster[2] == cluster[3] and cluster[4] == -1
    assert R.same_partition(cluster, R.undecided_pairs(row, d)[1])
    assert np.array_equal(R.undecided_positions(np.stack([row, row[::-1]]), d, active=[0, 1]), 5 + np.array([1, 2, 3, 4]))


def test_entry_points_check_their_arguments_before_any_launch():
    """Fake, never dereferenced device addresses: every refusal happens on the host (the error contract of include/cirrank.h)."""
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    EINVAL, ESHAPE, EALIGN = -1, -2, -3
    P = 0x10000
    ws = c.cir_rank_undecided_workspace
    assert ws(0, 8) == EINVAL and ws(3, 0) == EINVAL and ws(3, 8193) == ESHAPE
    assert ws(3, 5) == 16 + 16 + 4 * 8 and ws(65, 8192) == 65 * 8192 + 264 + 66 * 8

    def und(**over):
        a = dict(values=P, ld=100, active=None, margin=0.5, pos=P, count=P, Q=4, K=100, work=P, bytes=ws(4, 100), stream=None)
        a.update(over)
        return c.cir_rank_undecided(*[a[x] for x in ("values", "ld", "active", "margin", "pos", "count", "Q", "K", "work", "bytes", "stream")])

    assert und(values=None) == EINVAL and und(pos=None) == EINVAL and und(count=None) == EINVAL and und(ld=99) == EINVAL
    assert und(margin=-1e-6) == EINVAL and und(margin=float("nan")) == EINVAL and und(margin=float("inf")) == EINVAL
    assert und(K=8193, ld=8193) == ESHAPE and und(Q=0) == EINVAL
    assert und(work=None) == EINVAL and und(work=P + 4) == EINVAL and und(bytes=ws(4, 100) - 1) == EINVAL

    def app(**over):
        a = dict(values=P, ld=100, pos=P, referee=P, n=7, margin=0.5, stats=P, Q=4, K=100, stream=None)
        a.update(over)
        return c.cir_rank_refine_apply(*[a[x] for x in ("values", "ld", "pos", "referee", "n", "margin", "stats", "Q", "K", "stream")])

    assert app(values=None) == EINVAL and app(stats=None) == EINVAL and app(pos=None) == EINVAL and app(referee=None) == EINVAL
    assert app(n=-1) == EINVAL and app(ld=99) == EINVAL and app(margin=-1.0) == EINVAL and app(margin=float("nan")) == EINVAL
    assert app(stats=P + 4) == EALIGN and app(n=401) == ESHAPE


def test_ops_refuse_host_tensors_and_bad_layouts():
    import torch
    from candidate_reranking_cir_amd import ops
    from candidate_reranking_cir_amd.lib import CirrankError
    with pytest.raises(CirrankError):
        ops.rank_undecided(torch.zeros(3, 5), 0.1)
    with pytest.raises(CirrankError):
        ops.rank_refine_apply(torch.zeros(3, 5), torch.zeros(0, dtype=torch.int64), torch.zeros(0), 0.1)
