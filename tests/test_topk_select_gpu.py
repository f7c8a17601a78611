"""cir_topk_select / cir_rank_of (csrc/rank.hip) on a real MI355X: the first k columns of every row's descending order and the position of
given columns in it, for rows of any length - against `torch.argsort(stable=True, descending=True)` taken after the NaN -> -inf
substitution and after removing the excluded column.  The order is strict and total (value descending, then column ascending), so every
comparison is `torch.equal`: there are no tolerances.  Outputs sit inside canary allocations (tests/test_guard_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_guard_gpu import _flat_guard, _flat_intact

pytestmark = pytest.mark.gpu

KINDS = ("random", "levels8", "equal", "special")
BEYOND = [(3, 8193, 50), (3, 16385, 200), (3, 20000, 1), (3, 123403, 100), (2, 70000, 1024)]   # the last: 9 lists x 1024 > 8192 pairs, two merge rounds


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import lib, ops, validate

    class RT:
        pass
    r = RT()
    r.lib, r.c, r.ops, r.validate = lib, lib.load(), ops, validate
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _values(q, n, kind):
    """Seeded fp32 (q, n) rows; callers only read them."""
    g = torch.Generator().manual_seed(1000 * q + n)
    if kind == "equal":
        return torch.full((q, n), 0.25)
    if kind == "levels8":
        return torch.randint(0, 8, (q, n), generator=g).float() * 0.125 - 0.5
    v = torch.randn((q, n), generator=g)
    if kind == "special":
        v[0, ::7] = float("nan")
        v[1, 5] = v[1, n - 1] = float("inf")
        if q > 2:
            v[2, ::3] = float("-inf")
    return v


def _keys(v):
    return torch.where(torch.isnan(v), torch.full_like(v, float("-inf")), v)


def _ref_order(v, exclude=None):
    """Per row: the columns in the reference order (a list of 1-D int64 tensors; a row is one column shorter where a column is excluded)."""
    keys, out = _keys(v), []
    for r in range(v.shape[0]):
        cols = torch.arange(v.shape[1])
        if exclude is not None and int(exclude[r]) >= 0:
            cols = cols[cols != int(exclude[r])]
        out.append(cols[torch.argsort(keys[r, cols], stable=True, descending=True)])
    return out


@functools.lru_cache(maxsize=None)
def _ref_plain(q, n, kind):
    return _ref_order(_values(q, n, kind))


def _select(rt, vdev, n, k, exclude=None, want_val=True):
    """cir_topk_select through the C ABI on the (possibly row-strided) device rows `vdev`, outputs inside canaries -> (idx, val) on the host."""
    q = vdev.shape[0]
    need = rt.c.cir_topk_select_workspace(q, n, k)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    ibuf, idx = _flat_guard(q * k, torch.int64)
    vbuf, val = _flat_guard(q * k, torch.float32)
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64).cuda()
    rt.lib.check(rt.c.cir_topk_select(vdev.data_ptr(), vdev.stride(0), None if ex is None else ex.data_ptr(), idx.data_ptr(),
                                      val.data_ptr() if want_val else None, q, n, k, work.data_ptr(), need, _stream()), "cir_topk_select")
    torch.cuda.synchronize()
    assert _flat_intact(ibuf, q * k, torch.int64) and (_flat_intact(vbuf, q * k, torch.float32) or not want_val), "a store outside the output"
    return idx.view(q, k).cpu(), val.view(q, k).cpu()


def _check_select(rt, q, n, kind, k, exclude=None):
    v = _values(q, n, kind)
    ref = _ref_plain(q, n, kind) if exclude is None else _ref_order(v, exclude)
    idx, val = _select(rt, v.cuda(), n, k, exclude)
    want = torch.stack([r[:k] for r in ref])
    assert torch.equal(idx, want)
    assert torch.equal(val.view(torch.int32), torch.gather(_keys(v), 1, want).view(torch.int32))     # the keys as sorted, bit for bit
    return idx


# ------------------------------------------------------------------------------------------------ 1. where the full sort runs too
@pytest.mark.parametrize("kind", ["random", "levels8"])
@pytest.mark.parametrize("n", [2, 7, 200, 2297, 8192])
def test_same_answer_as_the_full_sort(rt, n, kind):
    v = _values(5, n, kind).cuda()
    k = min(n - 1, 50)
    assert torch.equal(rt.ops.topk_desc(v, k), rt.ops.argsort_desc(v)[:, :k])


# ------------------------------------------------------------------------------------------------ 2. beyond one segment
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("q,n,k", BEYOND, ids=lambda x: str(x))
def test_beyond_one_segment(rt, q, n, k, kind):
    idx = _check_select(rt, q, n, kind, k)
    if kind == "equal":
        assert torch.equal(idx, torch.arange(k).expand(q, k))


# ------------------------------------------------------------------------------------------------ 3. exclusion
@pytest.mark.parametrize("kind", ["random", "levels8"])
@pytest.mark.parametrize("q,n,k", BEYOND, ids=lambda x: str(x))
def test_exclusion_at_segment_seams(rt, q, n, k, kind):
    _check_select(rt, q, n, kind, k, [min(c, n - 1) for c in (8191, 8192, 0)][:q])


@pytest.mark.parametrize("q,n,k", BEYOND[:2] + [(3, 300, 299)], ids=lambda x: str(x))
def test_exclusion_of_the_best_column_and_whole_row(rt, q, n, k):
    for kind in ("random", "levels8", "equal"):
        best = [int(r[0]) for r in _ref_plain(q, n, kind)]
        idx = _check_select(rt, q, n, kind, k, best)
        assert not (idx == torch.tensor(best)[:, None]).any()
        if k == n - 1:                                                 # the whole row minus one column
            assert torch.equal(torch.sort(idx, dim=1).values, torch.stack([torch.tensor([c for c in range(n) if c != b]) for b in best]))


def test_exclude_minus_one_is_none(rt):
    v = _values(3, 16385, "levels8")
    a, av = _select(rt, v.cuda(), 16385, 200, None)
    b, bv = _select(rt, v.cuda(), 16385, 200, [-1, -1, -1])
    assert torch.equal(a, b) and torch.equal(av, bv)
    c = rt.ops.topk_desc(v.cuda(), 200, torch.tensor([-1, 8192, -1]).cuda()).cpu()          # mixed: only row 1 loses a column
    assert torch.equal(c[0], a[0]) and torch.equal(c[2], a[2]) and torch.equal(c[1], _ref_order(v[1:2], [8192])[0][:200])


# ------------------------------------------------------------------------------------------------ 4. strided rows
@pytest.mark.parametrize("q,n,k", [(5, 2297, 50), (3, 16385, 200)], ids=lambda x: str(x))
def test_strided_rows(rt, q, n, k):
    v = _values(q, n, "random")
    g = torch.Generator().manual_seed(n)
    buf = torch.randn((q, n + 37), generator=g)
    buf[:, :n] = v
    dbuf = buf.cuda()
    before = dbuf.clone()
    view = dbuf[:, :n]
    ex = [n - 1, 0, 5, 7, 9][:q]
    idx, val = _select(rt, view, n, k, ex)
    cidx, cval = _select(rt, v.cuda(), n, k, ex)
    assert torch.equal(idx, cidx) and torch.equal(val, cval)
    assert torch.equal(rt.ops.topk_desc(view, k, torch.tensor(ex).cuda()).cpu(), cidx)
    cols = torch.stack([torch.tensor([0, 1, n // 2, n - 1]) for _ in range(q)]).cuda()
    assert torch.equal(rt.ops.rank_of(view, cols, torch.tensor(ex).cuda()), rt.ops.rank_of(v.cuda(), cols, torch.tensor(ex).cuda()))
    assert torch.equal(dbuf.view(torch.int32), before.view(torch.int32))                     # values are never written


# ------------------------------------------------------------------------------------------------ 5. rank_of
def _rank_of(rt, vdev, n, cols, exclude):
    q, m = cols.shape
    rbuf, rank = _flat_guard(q * m, torch.int64)
    dcols = cols.cuda()
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64).cuda()
    rt.lib.check(rt.c.cir_rank_of(vdev.data_ptr(), vdev.stride(0), dcols.data_ptr(), None if ex is None else ex.data_ptr(), rank.data_ptr(),
                                  q, n, m, _stream()), "cir_rank_of")
    torch.cuda.synchronize()
    assert _flat_intact(rbuf, q * m, torch.int64), "a store outside the output"
    return rank.view(q, m).cpu()


def _want_ranks(v, cols, exclude):
    ref = _ref_order(v, exclude)
    want = torch.full(cols.shape, -1, dtype=torch.int64)
    for r, order in enumerate(ref):
        pos = torch.full((v.shape[1] + 1,), -1, dtype=torch.int64)
        pos[order] = torch.arange(len(order))
        inside = (cols[r] >= 0) & (cols[r] < v.shape[1])
        want[r] = torch.where(inside, pos[cols[r].clamp(0, v.shape[1])], torch.tensor(-1))
    return want


@pytest.mark.parametrize("kind", ["random", "levels8"])
@pytest.mark.parametrize("n", [8193, 20000])
def test_rank_of(rt, n, kind):
    q, k = 3, 100
    v = _values(q, n, kind).clone()
    v[:, 11] = float("nan")                                            # a NaN column: it ranks as -inf
    v[:, 4000] = v[:, 9]                                               # a tie across columns (levels8 is full of them anyway)
    exclude = [8192, 0, n - 1]
    ref = _ref_order(v, exclude)
    cols = torch.stack([torch.tensor([int(ref[r][0]), int(ref[r][k - 1]), 9, 4000, 11, exclude[r]]) for r in range(q)])
    want = _want_ranks(v, cols, exclude)
    assert (want[:, 0] == 0).all() and (want[:, 1] == k - 1).all() and (want[:, 5] == -1).all() and (want[:, 3] > want[:, 2]).all()
    assert torch.equal(_rank_of(rt, v.cuda(), n, cols, exclude), want)
    assert torch.equal(_rank_of(rt, v.cuda(), n, cols, None), _want_ranks(v, cols, None))
    assert torch.equal(rt.ops.rank_of(v.cuda(), cols.cuda(), torch.tensor(exclude).cuda()).cpu(), want)


def test_rank_of_columns_outside_the_row(rt):
    n = 301
    v = _values(2, n, "special")
    cols = torch.tensor([[0, 7, 14, n - 1, n, -1, 2 ** 40, 3], [5, n - 1, 6, 0, -7, n + 5, 1, 2]])
    got = _rank_of(rt, v.cuda(), n, cols, [3, -1])
    assert torch.equal(got, _want_ranks(v, cols, [3, -1]))
    assert got[0, 7] == -1 and (got[:, 4:6] == -1).all() and got[1, 0] == 0 and got[1, 1] == 1        # +inf at columns 5 and n - 1


# ------------------------------------------------------------------------------------------------ 6. validate.rank_index_topk
def test_rank_index_topk(rt):
    g = torch.Generator().manual_seed(64)
    pred = torch.nn.functional.normalize(torch.randn((64, 256), generator=g), dim=-1).cuda()
    index = torch.nn.functional.normalize(torch.randn((20000, 256), generator=g), dim=-1).cuda()
    k = 100
    mat = rt.ops.linear_f32(pred, index, None, mode=2).cpu()
    ref = _ref_order(mat)
    targets = torch.tensor([int(ref[r][(7 * r) % 20000]) for r in range(64)])
    topk, ranks = rt.validate.rank_index_topk(pred, index, k, cols=targets[:, None])
    assert topk.shape == (64, k) and topk.dtype == torch.int64 and ranks.shape == (64, 1) and ranks.dtype == torch.int64
    assert torch.equal(topk.cpu(), torch.stack([r[:k] for r in ref]))
    assert torch.equal(ranks.cpu()[:, 0], torch.tensor([(7 * r) % 20000 for r in range(64)]))
    topk7, ranks7 = rt.validate.rank_index_topk(pred, index, k, cols=targets[:, None], row_block=7)
    assert torch.equal(topk7, topk) and torch.equal(ranks7, ranks)
    only, none = rt.validate.rank_index_topk(pred, index, k)
    assert none is None and torch.equal(only, topk)
    refs = torch.tensor([int(ref[r][r % 3]) for r in range(64)])                             # drop one of each row's first three
    ex_topk, ex_ranks = rt.validate.rank_index_topk(pred, index, k, exclude=refs.numpy(), cols=torch.stack([targets, refs], 1), row_block=30)
    ex_ref = _ref_order(mat, refs)
    assert torch.equal(ex_topk.cpu(), torch.stack([r[:k] for r in ex_ref])) and (ex_ranks[:, 1] == -1).all()


# ------------------------------------------------------------------------------------------------ 7. pinned by the reference's files
def _same_top(a, b):
    assert set(a) == set(b)
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), key
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), key
        else:
            assert x == y, key


def test_reference_fixture_metrics_and_dicts(rt, tmp_path):
    V = rt.validate
    z = H.load("stage1_tiny.npz")
    names, k = [str(n) for n in z["index_names"]], int(z["k"])
    pooled = torch.tensor(z["pooled"]).cuda()
    group6 = np.concatenate([z["refs"][:, None], z["groups"]], axis=1)
    # CIRR
    pred = torch.tensor(z["cirr_pred"]).cuda()
    want_m, want_top = V.cirr_topk(V.rank_index(pred, pooled).cpu().numpy(), z["refs"], z["targets"], group6, names, k, "val")
    topk, ranks = V.rank_index_topk(pred, pooled, k, exclude=z["refs"], cols=V.cirr_rank_cols(z["refs"], z["targets"], group6))
    got_m, got_top = V.cirr_topk_from_ranks(topk.cpu().numpy(), ranks.cpu().numpy(), z["refs"], z["targets"], group6, names, k, "val")
    assert got_m == want_m
    _same_top(got_top, want_top)
    assert (got_top["sorted_index_names"] == z["cirr_file_names"]).all() and got_top["group_labels"].shape == (len(pred), 5)
    np.testing.assert_allclose(got_m, z["cirr_metrics"], atol=1e-4)
    path = str(tmp_path / "cirr_top.pt")
    V.save_topk(path, got_top)
    assert (V.load_topk(path, k, z["refs"]).labels == z["cirr_file_labels"]).all()
    # FashionIQ
    fpred = torch.tensor(z["fiq_pred"]).cuda()
    fwant_m, fwant_top = V.fiq_topk(V.rank_index(fpred, pooled).cpu().numpy(), z["targets"], names, k, "val", str(z["fiq_file_dress"]))
    ftopk, franks = V.rank_index_topk(fpred, pooled, k, cols=z["targets"][:, None])
    fgot_m, fgot_top = V.fiq_topk_from_ranks(ftopk.cpu().numpy(), franks.cpu().numpy(), z["targets"], names, k, "val", str(z["fiq_file_dress"]))
    assert fgot_m == fwant_m
    _same_top(fgot_top, fwant_top)
    assert (fgot_top["sorted_index_names"] == z["fiq_file_names"]).all()
