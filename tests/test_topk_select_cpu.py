"""Stage-I retrieval for indexes of any size, the parts that need no GPU: the host functions that turn (first k columns, ranks of a few
columns) into the metrics and top-K dicts of `fiq_topk` / `cirr_topk`, the error contract of cir_topk_select / cir_rank_of (fake, never
dereferenced device addresses, as tests/test_abi.py), the workspace size function, and the wrappers' refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from tests import helpers as H

EINVAL, ESHAPE = -1, -2
P = 0x10000          # 8-byte aligned fake device address


def _ranks_of(order: np.ndarray, cols: np.ndarray) -> np.ndarray:
    """Position of cols[q, t] in row q of a ranking; -1 where the ranking does not hold it (the excluded column)."""
    out = np.full(cols.shape, -1, dtype=np.int64)
    for q in range(order.shape[0]):
        pos = {int(c): j for j, c in enumerate(order[q])}
        out[q] = [pos.get(int(c), -1) for c in cols[q]]
    return out


def _same_top(a: dict, b: dict):
    assert set(a) == set(b)
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), key
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), key
        else:
            assert type(x) is type(y) and x == y, key


def _check_fiq(V, order, targets, names, k):
    want_m, want_top = V.fiq_topk(order, targets, names, k, "val", "dress")
    got_m, got_top = V.fiq_topk_from_ranks(order[:, :k], _ranks_of(order, targets[:, None]), targets, names, k, "val", "dress")
    assert got_m == want_m
    _same_top(got_top, want_top)
    return got_top


def _check_cirr(V, order, refs, targets, group6, names, k):
    want_m, want_top = V.cirr_topk(order, refs, targets, group6, names, k, "val")
    dropped = order[order != refs[:, None]].reshape(len(order), -1)                 # the ranking with the reference removed
    cols = V.cirr_rank_cols(refs, targets, group6)
    assert cols.shape == (len(order), 6) and (cols[:, 0] == targets).all()
    got_m, got_top = V.cirr_topk_from_ranks(dropped[:, :k], _ranks_of(dropped, cols), refs, targets, group6, names, k, "val")
    assert got_m == want_m
    _same_top(got_top, want_top)
    assert got_top["group_labels"].shape == (len(order), 5)
    return got_top


def test_from_ranks_on_the_reference_fixture(tmp_path):
    from candidate_reranking_cir_amd import validate as V
    z = H.load("stage1_tiny.npz")
    names, k = [str(n) for n in z["index_names"]], int(z["k"])
    group6 = np.concatenate([z["refs"][:, None], z["groups"]], axis=1)
    order = np.argsort(1 - z["cirr_pred"] @ z["pooled"].T, axis=1, kind="stable")
    top = _check_cirr(V, order, z["refs"], z["targets"], group6, names, k)
    assert (top["sorted_index_names"] == z["cirr_file_names"]).all() and (top["group_labels"].numpy() == z["cirr_file_group_labels"]).all()
    forder = np.argsort(1 - z["fiq_pred"] @ z["pooled"].T, axis=1, kind="stable")
    ftop = _check_fiq(V, forder, z["targets"], names, k)
    assert (ftop["sorted_index_names"] == z["fiq_file_names"]).all() and (ftop["labels"].numpy() == z["fiq_file_labels"]).all()
    # a file written from the new dicts loads through load_topk unchanged
    path = str(tmp_path / "top.pt")
    V.save_topk(path, top)
    ds = V.load_topk(path, k, z["refs"], group_index=z["groups"])
    assert (ds.labels == z["cirr_file_labels"]).all() and (ds.target_index == z["targets"]).all()
    assert (np.array(names)[ds.cand_index] == z["cirr_file_names"]).all()


def test_from_ranks_on_a_9000_image_index():
    """An index above the full sort's 8192 ceiling: numpy's stable argsort stands in for the device."""
    from candidate_reranking_cir_amd import validate as V
    rng = np.random.default_rng(5)
    n, q_n, k = 9000, 24, 100
    scores = np.round(rng.standard_normal((q_n, n)).astype(np.float32), 2)          # two decimals: plenty of ties
    order = np.argsort(-scores, axis=1, kind="stable")
    names = [f"im{i:05d}" for i in range(n)]
    group6 = np.stack([rng.choice(n, 6, replace=False) for _ in range(q_n)])
    refs = group6[:, 0].copy()
    targets = group6[np.arange(q_n), rng.integers(1, 6, q_n)]
    for q, ends in ((0, order[0, :2]), (1, order[1, :-3:-1])):                       # a first-place target and a last-place one
        col = ends[0] if ends[0] != refs[q] else ends[1]
        if col not in group6[q]:
            group6[q, 1] = col
        targets[q] = col
    for row in group6:
        assert len(set(row.tolist())) == 6
    group6 = group6[:, rng.permutation(6)]                                           # the reference sits anywhere in its group
    _check_cirr(V, order, refs, targets, group6, names, k)
    _check_fiq(V, order, targets, names, k)


def test_from_ranks_keep_the_references_asserts():
    from candidate_reranking_cir_amd import validate as V
    names = [f"i{i}" for i in range(12)]
    order = np.tile(np.arange(12), (2, 1))
    targets, refs = np.array([3, 4]), np.array([0, 1])
    group6 = np.array([[0, 3, 5, 6, 7, 8], [1, 4, 5, 6, 7, 8]])
    with pytest.raises(AssertionError):                                              # a target that is not in the ranking (rank -1)
        V.fiq_topk_from_ranks(order[:, :5], np.array([[-1], [4]]), targets, names, 5, "val", "shirt")
    dropped = order[order != refs[:, None]].reshape(2, -1)
    cols = V.cirr_rank_cols(refs, targets, group6)
    ranks = _ranks_of(dropped, cols)
    V.cirr_topk_from_ranks(dropped[:, :5], ranks, refs, targets, group6, names, 5, "val")
    with pytest.raises(AssertionError):                                              # a target outside its group
        V.cirr_topk_from_ranks(dropped[:, :5], ranks, refs, np.array([9, 4]), group6, names, 5, "val")
    with pytest.raises(AssertionError):                                              # a reference that is not in its group
        V.cirr_rank_cols(np.array([2, 1]), targets, group6)


def test_error_contract_before_any_launch():
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    ws = c.cir_topk_select_workspace

    def sel(**o):
        a = {**dict(values=P, ld=20000, exclude=None, idx=P, val=None, Q=4, n=20000, k=100, work=P, bytes=ws(4, 20000, 100), stream=None), **o}
        return c.cir_topk_select(*[a[x] for x in ("values", "ld", "exclude", "idx", "val", "Q", "n", "k", "work", "bytes", "stream")])

    assert sel(values=None) == EINVAL and sel(idx=None) == EINVAL and sel(Q=0) == EINVAL and sel(n=0) == EINVAL and sel(k=0) == EINVAL
    assert sel(Q=-3) == EINVAL and sel(ld=19999) == EINVAL
    assert sel(k=2049, bytes=1 << 40) == ESHAPE and sel(n=50, ld=50, k=50) == ESHAPE and sel(n=1, ld=1, k=1) == ESHAPE
    assert sel(work=None) == EINVAL and sel(bytes=ws(4, 20000, 100) - 1) == EINVAL and sel(bytes=0) == EINVAL
    assert sel(n=300, ld=300, k=299, bytes=0) == EINVAL                              # one segment: the workspace contract is the same

    def rk(**o):
        a = {**dict(values=P, ld=20000, cols=P, exclude=None, rank=P, Q=4, n=20000, m=6, stream=None), **o}
        return c.cir_rank_of(*[a[x] for x in ("values", "ld", "cols", "exclude", "rank", "Q", "n", "m", "stream")])

    assert rk(values=None) == EINVAL and rk(cols=None) == EINVAL and rk(rank=None) == EINVAL
    assert rk(Q=0) == EINVAL and rk(n=0) == EINVAL and rk(m=0) == EINVAL and rk(ld=19999) == EINVAL
    assert rk(m=9) == ESHAPE
    assert c.cir_version() == 15


def test_workspace_size():
    from candidate_reranking_cir_amd import lib
    ws = lib.load().cir_topk_select_workspace
    for q, n, k in ((1, 2, 1), (5, 8192, 50), (3, 8193, 50), (3, 123403, 100), (2, 70000, 1024), (4181, 123403, 100), (7, 2 ** 31 - 1, 2048)):
        need = ws(q, n, k)
        assert need >= q * -(-n // 8192) * min(k, 8192) * 8 > 0, (q, n, k)
        assert ws(q + 1, n, k) >= need and ws(2 * q, n, k) >= need                   # monotone in Q
    assert ws(0, 100, 5) == EINVAL and ws(4, 0, 5) == EINVAL and ws(4, 100, 0) == EINVAL and ws(-1, 100, 5) == EINVAL
    assert ws(4, 20000, 2049) == ESHAPE and ws(4, 100, 100) == ESHAPE and ws(4, 1, 1) == ESHAPE
    assert ws(2 ** 31 - 1, 20000, 5) == ESHAPE                                       # Q * segments is one grid dimension


def test_wrappers_refuse_cpu_tensors():
    from candidate_reranking_cir_amd import ops
    from candidate_reranking_cir_amd.lib import CirrankError
    v = torch.zeros(3, 40)
    with pytest.raises(CirrankError):
        ops.topk_desc(v, 5)
    with pytest.raises(CirrankError):
        ops.rank_of(v, torch.zeros(3, 2, dtype=torch.int64))
