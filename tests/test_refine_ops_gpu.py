"""cir_rank_undecided / cir_rank_refine_apply (csrc/rank.hip) on a real MI355X against the numpy restatement of the rule
(tests/refine_cases.py).  Positions and counts are integers and the rule is stated in fp32, so every comparison is equality.  Inputs with
a row stride above K carry canary columns (NaN patterns: a kernel that read them would link or sort them), outputs sit between canary
bands, and `pos` beyond `count` must stay unwritten."""
import functools

import numpy as np
import pytest
import torch

from tests import refine_cases as R

pytestmark = pytest.mark.gpu

CANARY_F32, CANARY_I64 = 0x7FC0DEAD, 0x7EADBEEF7EADBEEF
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
    canary, as_int = (CANARY_F32, torch.int32) if dtype == torch.float32 else (CANARY_I64, torch.int64)
    big = torch.empty(n + 2 * BAND, dtype=dtype, device="cuda")
    big.view(as_int).fill_(canary)
    return big, big[BAND:BAND + n]


def _bands_intact(big, n):
    bits = big.view(torch.int32 if big.dtype == torch.float32 else torch.int64)
    canary = CANARY_F32 if big.dtype == torch.float32 else CANARY_I64
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
    """(values (q, k) fp32, margin, active (q,) bool): a spread that leaves decided and undecided entries side by side at every K, exact
    ties, a row with NaN / +-inf entries, an all-equal row, and inactive rows (which hold one fill value, like skipped queries)."""
    rng = np.random.default_rng(100 * q + k)
    v = (0.3 * rng.standard_normal((q, k))).astype(np.float32)
    margin = float(np.float32(0.15 / k))
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


@functools.lru_cache(maxsize=None)
def _want(q, k):
    v, margin, active = _case(q, k)
    return R.undecided_positions(v, margin, active)


def _undecided(rt, view, margin, active):
    q, k = view.shape
    need = rt.c.cir_rank_undecided_workspace(q, k)
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    pbig, pos = _guarded(q * k, torch.int64)
    cbig, count = _guarded(1, torch.int64)
    act = None if active is None else torch.from_numpy(active.astype(np.uint8)).cuda()
    rt.lib.check(rt.c.cir_rank_undecided(view.data_ptr(), view.stride(0), None if act is None else act.data_ptr(), margin, pos.data_ptr(),
                                         count.data_ptr(), q, k, work.data_ptr(), need, _stream()), "cir_rank_undecided")
    torch.cuda.synchronize()
    assert _bands_intact(pbig, q * k) and _bands_intact(cbig, 1), "a store outside pos / count"
    return pbig.cpu(), int(count.cpu()[0])


@pytest.mark.parametrize("k", [1, 2, 5, 63, 64, 65, 100, 1025, 2047, 2048, 8192])
@pytest.mark.parametrize("q", [1, 3, 65])
def test_undecided_against_the_restatement(rt, q, k):
    v, margin, active = _case(q, k)
    want = _want(q, k)
    if k >= 5:
        assert 0 < len(want) < int(active.sum()) * k                      # the case exercises both outcomes
    big, view = _wide(v, 3)
    whole, n = _undecided(rt, view, margin, active)
    assert n == len(want)
    assert np.array_equal(whole[BAND:BAND + n].numpy(), want)             # as sets and in order
    assert bool((whole[BAND + n:] == CANARY_I64).all()), "pos was written beyond count"
    assert bool((big.view(torch.int32)[:, k:] == CANARY_F32).all())
    assert np.array_equal(big.cpu().view(torch.int32)[:, :k].numpy(), v.view(np.int32)), "the values are never written"
    again, n2 = _undecided(rt, view, margin, active)
    assert n2 == n and torch.equal(again, whole)                          # bit-identical, the unwritten tail included
    # the tensor front end on the same strided view, and on a dense copy without a mask
    pos, count = rt.ops.rank_undecided(view, margin, torch.from_numpy(active).cuda())
    assert int(count) == n and np.array_equal(pos[:n].cpu().numpy(), want)
    if active.all():
        pos, count = rt.ops.rank_undecided(view.contiguous(), margin)
        assert int(count) == n and np.array_equal(pos[:n].cpu().numpy(), want)


def test_undecided_margin_zero_and_a_margin_above_the_range(rt):
    v, _, _ = _case(3, 100)
    pos, count = rt.ops.rank_undecided(torch.from_numpy(v).cuda(), 0.0)
    want = R.undecided_positions(v, 0.0)                                                  # exact ties only: the two constant rows and a few pairs
    assert np.array_equal(pos[:int(count)].cpu().numpy(), want) and 200 <= len(want) < 300
    pos, count = rt.ops.rank_undecided(torch.linspace(-1.0, 1.0, 100).view(1, 100).cuda(), 10.0)
    assert int(count) == 100 and torch.equal(pos[:100].cpu(), torch.arange(100))


def test_refusals(rt):
    from candidate_reranking_cir_amd.lib import CirrankError
    with pytest.raises(CirrankError, match="(?i)extent"):
        rt.ops.rank_undecided(torch.zeros((2, 8193), device="cuda"), 0.1)
    ok = torch.zeros((2, 16), device="cuda")
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(CirrankError):
            rt.ops.rank_undecided(ok, bad)
        with pytest.raises(CirrankError):
            rt.ops.rank_refine_apply(ok, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, device="cuda"), bad)
    with pytest.raises(CirrankError):
        rt.ops.rank_undecided(ok.t(), 0.1)                                 # rows must be unit-stride: the matrix is written in place, never copied


@pytest.mark.parametrize("q,k,share", [(5, 37, 0.3), (65, 100, 0.6), (3, 8192, 0.2), (4, 9, 0.0), (1, 1, 1.0)])
def test_refine_apply(rt, q, k, share):
    rng = np.random.default_rng(q * 1000 + k)
    old = (0.5 * rng.standard_normal((q, k))).astype(np.float32)
    pos = np.sort(rng.choice(q * k, size=int(round(share * q * k)), replace=False)).astype(np.int64)
    n = len(pos)
    margin = np.float32(0.01)
    referee = (old.reshape(-1)[pos] + rng.uniform(-0.02, 0.02, n)).astype(np.float32)          # about half of them beyond the margin
    if n > 2:
        referee[0] = old.reshape(-1)[pos[0]]                                                    # deviation 0
        referee[1] = np.float32(old.reshape(-1)[pos[1]] + margin)                               # on or next to the boundary
    dev = np.abs(old.reshape(-1)[pos] - referee)                                                # fp32, as the kernel forms it
    want = old.copy()
    want.reshape(-1)[pos] = referee
    big, view = _wide(old, 5)
    rbig, rdev = _guarded(n, torch.float32)
    rdev.copy_(torch.from_numpy(referee))
    stats = rt.ops.rank_refine_apply(view, torch.from_numpy(pos).cuda(), rdev, float(margin))
    worst, bad = rt.ops.refine_stats(stats)
    assert torch.equal(view.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32))  # written values and untouched entries, bit for bit
    assert bool((big.view(torch.int32)[:, k:] == CANARY_F32).all()), "a store into the columns beyond K"
    assert _bands_intact(rbig, n) and torch.equal(rdev.cpu(), torch.from_numpy(referee))
    assert np.float32(worst) == (dev.max() if n else np.float32(0)) and bad == int((dev > margin).sum())
    if n > 2:
        assert 0 < bad < n
    # through the C ABI with the statistics between canaries
    big2, view2 = _wide(old, 5)
    sbig, sdev = _guarded(2, torch.int64)
    pdev = torch.from_numpy(pos).cuda()
    rt.lib.check(rt.c.cir_rank_refine_apply(view2.data_ptr(), view2.stride(0), pdev.data_ptr() if n else None, rdev.data_ptr() if n else None, n,
                                            float(margin), sdev.data_ptr(), q, k, _stream()), "cir_rank_refine_apply")
    torch.cuda.synchronize()
    raw = sdev.view(torch.uint8).cpu()
    assert _bands_intact(sbig, 2) and torch.equal(raw[:4], stats.cpu()[:4]) and torch.equal(raw[8:], stats.cpu()[8:])
    assert bool((raw[4:8].view(torch.int32) == CANARY_I64 >> 32).all()), "bytes 4 .. 7 of the statistics are padding: not written"
    assert torch.equal(big2.view(torch.int32), big.view(torch.int32))


def test_refine_apply_skips_positions_outside_the_matrix(rt):
    old = torch.arange(12, dtype=torch.float32).view(3, 4)
    big, view = _wide(old.numpy(), 2)
    pos = torch.tensor([-1, 5, 12, 1 << 40], dtype=torch.int64).cuda()
    stats = rt.ops.rank_refine_apply(view, pos, torch.full((4,), 100.0, device="cuda"), 1000.0)
    want = old.clone()
    want[1, 1] = 100.0
    assert torch.equal(view.cpu(), want) and bool((big.view(torch.int32)[:, 4:] == CANARY_F32).all())
    assert rt.ops.refine_stats(stats) == (95.0, 3)
