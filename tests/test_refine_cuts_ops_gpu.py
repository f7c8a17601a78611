"""cir_rank_undecided_cuts (csrc/rank.hip) on a real MI355X against the numpy restatement of the selective rule
(tests/refine_cut_cases.py, selected_links).  Positions and counts are integers and the rule is stated in fp32, so every comparison is
equality.  Inputs with a row stride above K carry canary columns, `pos`, `count` and the workspace sit between canary bands, and `pos`
beyond `count` must stay unwritten."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import refine_cases as R
from tests import refine_cut_cases as C

pytestmark = pytest.mark.gpu

CANARY_F32, CANARY_I64, CANARY_U8 = 0x7FC0DEAD, 0x7EADBEEF7EADBEEF, 0xA5
BAND = 64


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import lib, ops

    class RT:
        pass
    r = RT()
    r.lib, r.c, r.ops = lib, lib.load(), ops
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype):
    """(whole buffer, the n elements between two canary bands)."""
    canary = {torch.float32: CANARY_F32, torch.int64: CANARY_I64, torch.uint8: CANARY_U8}[dtype]
    big = torch.empty(n + 2 * BAND, dtype=dtype, device="cuda")
    big.view(torch.int32 if dtype == torch.float32 else dtype).fill_(canary)
    return big, big[BAND:BAND + n]


def _bands_intact(big, n):
    canary = {torch.float32: CANARY_F32, torch.int64: CANARY_I64, torch.uint8: CANARY_U8}[big.dtype]
    bits = big.view(torch.int32) if big.dtype == torch.float32 else big
    return bool((bits[:BAND] == canary).all()) and bool((bits[BAND + n:] == canary).all())


def _wide(values: np.ndarray, pad: int):
    """The (Q, K) matrix as a view of a (Q, K + pad) device buffer whose extra columns hold the canary."""
    q, k = values.shape
    big = torch.empty((q, k + pad), dtype=torch.float32, device="cuda")
    big.view(torch.int32).fill_(CANARY_F32)
    view = big[:, :k]
    view.copy_(torch.from_numpy(values))
    return big, view


@functools.lru_cache(maxsize=None)
def _case(q, k):
    """(values (q, k) fp32, margin, active (q,) bool): clusters of a few entries at every K (the expected gap of neighbours is about the
    width), exact ties, a row with NaN / +-inf entries, an all-equal row, and inactive rows (which hold one fill value, like skipped queries)."""
    rng = np.random.default_rng(1000 * q + k)
    v = (0.3 * rng.standard_normal((q, k))).astype(np.float32)
    margin = float(np.float32(0.3 / k))
    for r in range(q):
        for _ in range(min(3, k // 2)):
            v[r, rng.integers(k)] = v[r, rng.integers(k)]
    active = np.ones(q, dtype=bool)
    if q > 1:
        v[1, ::3] = np.nan
        v[1, 1::5] = np.inf
        v[1, 2::7] = -np.inf
    if q > 2:
        v[2] = 0.25
        active[[0] if q == 3 else rng.integers(3, q, size=q // 8)] = False
        v[~active] = -99999.99
    return v, margin, active


def _selections(k):
    """The grid of the CPU test, plus the selections the consumers use."""
    return C.selection_grid(k) + [(50, ()), (10, (50,)), (0, (1, 5, 10, 50)), (k // 2, (k // 2 + 1, k // 2 + 2))]


def _undecided_cuts(rt, view, margin, active, first, cuts):
    q, k = view.shape
    need = rt.c.cir_rank_undecided_workspace(q, k)
    assert need > 0
    wbig, work = _guarded(need, torch.uint8)                               # BAND = 64 bytes: the workspace stays 8-byte aligned
    pbig, pos = _guarded(q * k, torch.int64)
    cbig, count = _guarded(1, torch.int64)
    act = None if active is None else torch.from_numpy(active.astype(np.uint8)).cuda()
    host = (ctypes.c_int * max(len(cuts), 1))(*cuts)
    rt.lib.check(rt.c.cir_rank_undecided_cuts(view.data_ptr(), view.stride(0), None if act is None else act.data_ptr(), margin, first, host, len(cuts),
                                              pos.data_ptr(), count.data_ptr(), q, k, work.data_ptr(), need, _stream()), "cir_rank_undecided_cuts")
    torch.cuda.synchronize()
    assert _bands_intact(pbig, q * k) and _bands_intact(cbig, 1), "a store outside pos / count"
    assert _bands_intact(wbig, need), "a store outside the workspace"
    return pbig.cpu(), int(count.cpu()[0])


@pytest.mark.parametrize("k", [1, 2, 5, 24, 100, 105, 257, 1024, 1025, 2047, 2048, 8192])
@pytest.mark.parametrize("q", [1, 3, 70])
def test_selected_against_the_restatement(rt, q, k):
    v, margin, active = _case(q, k)
    selections = _selections(k)
    if k > 2000:                                                            # the restatement walks rows in Python: fewer selections at 8192
        selections = [s for i, s in enumerate(selections) if i in (2, 3, 6, 11, 13, 14, 15)] if q < 70 else [(10, (50,)), (k, ()), (0, (k - 1,))]
    big, view = _wide(v, 3)
    full_pos, full_count = rt.ops.rank_undecided(view, margin, torch.from_numpy(active).cuda())
    n_full = int(full_count)
    partial = 0
    for first, cuts in selections:
        want = C.selected_positions(v, margin, first, cuts, active)
        whole, n = _undecided_cuts(rt, view, margin, active, first, cuts)
        assert n == len(want), (first, cuts)
        assert np.array_equal(whole[BAND:BAND + n].numpy(), want), (first, cuts)          # as sets and in order
        assert bool((whole[BAND + n:] == CANARY_I64).all()), "pos was written beyond count"
        partial += int(0 < n < n_full)
        if first >= k:                                                      # the full rule: the old entry point's result
            assert n == n_full and torch.equal(whole[BAND:BAND + n], full_pos[:n].cpu())
        again, n2 = _undecided_cuts(rt, view, margin, active, first, cuts)
        assert n2 == n and torch.equal(again, whole)                        # bit-identical, the unwritten tail included
        pos, count = rt.ops.rank_undecided(view, margin, torch.from_numpy(active).cuda(), first=first, cuts=cuts)
        assert int(count) == n and np.array_equal(pos[:n].cpu().numpy(), want)
    if k >= 24:
        assert partial >= 2                                                 # selections that take some clusters and leave others
    assert bool((big.view(torch.int32)[:, k:] == CANARY_F32).all())
    assert np.array_equal(big.cpu().view(torch.int32)[:, :k].numpy(), v.view(np.int32)), "the values are never written"


def test_front_end_defaults_and_refusals(rt):
    from candidate_reranking_cir_amd.lib import CirrankError
    v, margin, active = _case(3, 100)
    dev = torch.from_numpy(v).cuda()
    old = rt.ops.rank_undecided(dev, margin)
    for kw in (dict(first=100), dict(first=107), dict(first=100, cuts=(3, 200))):
        new = rt.ops.rank_undecided(dev, margin, **kw)
        assert torch.equal(new[1], old[1]) and torch.equal(new[0][:int(old[1])], old[0][:int(old[1])])
    pos, count = rt.ops.rank_undecided(dev, margin, cuts=(100, 150))         # first=None with cuts: first = 0; cuts at and beyond K
    assert int(count) == 0
    pos, count = rt.ops.rank_undecided(dev, margin, first=0)
    assert int(count) == 0
    pos, count = rt.ops.rank_undecided(dev, margin, cuts=(10,))
    assert np.array_equal(pos[:int(count)].cpu().numpy(), C.selected_positions(v, margin, 0, (10,)))
    for bad in (dict(first=-1), dict(cuts=(0,)), dict(cuts=(4, 4)), dict(cuts=tuple(range(1, 10)))):
        with pytest.raises(CirrankError):
            rt.ops.rank_undecided(dev, margin, **bad)
    with pytest.raises(CirrankError, match="(?i)extent"):
        rt.ops.rank_undecided(torch.zeros((2, 8193), device="cuda"), 0.1, first=3)
