"""The training-side glue kernels (cir_eltwise, cir_colsum, cir_embed_bwd) on a real MI355X against the float64 references and the
a-priori bounds of tests/glue_cases.py: every mode x dtype pair of cir_eltwise at lengths around its 4-wide and 1024-wide steps, on
aligned allocations (16-byte accesses) and on views one element into their storage (the scalar path), bit for bit alike; the column
sums around the 32-row block and the 4-way unroll, with padded rows and into a non-zero output; the embedding scatter-add with
every id equal, on the real vocabulary."""
import numpy as np
import pytest
import torch

from tests import glue_cases as G
from tests import helpers as H
from tests.test_guard_gpu import CANARY, _INT, _flat_guard, _flat_intact

pytestmark = pytest.mark.gpu

BF16, F16, F32 = G.BF16, G.F16, G.F32


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import lib, train_ops

    class RT:
        pass
    r = RT()
    r.lib, r.c, r.T = lib, lib.load(), train_ops
    r.DT = {BF16: lib.CIR_BF16, F16: lib.CIR_F16, F32: lib.CIR_F32}
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _offset(t, k):
    """A copy of the 1-d tensor `t` that starts k elements into a fresh allocation (k = 0: aligned; k = 1: not 16-byte aligned)."""
    buf = torch.empty((t.numel() + 8,), dtype=t.dtype, device="cuda")
    buf[k:k + t.numel()].copy_(t)
    return buf[k:k + t.numel()]


def _eltwise(rt, c, i, k, seed=G.ELT_SEED):
    """One launch of case `c` on operands that all start `k` elements into their storage; returns (out, guard)."""
    mode = G.ELT_MODES.index(c.mode)
    z, dy = _offset(i["z"].cuda(), k), _offset(i["dy"].cuda(), k)
    buf = torch.empty((c.n + 2 * 4096,), dtype=c.out, device="cuda")
    buf.view(_INT[c.out]).fill_(CANARY[c.out])
    out = buf[4096 + k:4096 + k + c.n]
    assert (z.data_ptr() % 16 == 0) == (k == 0) and (out.data_ptr() % 16 == 0) == (k == 0) and (dy.data_ptr() % 16 == 0) == (k == 0)
    uses_dy = c.mode in ("gelu_bwd", "relu_bwd", "add")
    rt.lib.check(rt.c.cir_eltwise(z.data_ptr(), rt.DT[c.z], dy.data_ptr() if uses_dy else None, out.data_ptr(), rt.DT[c.out], c.n, mode,
                                  float(G.ELT_P.get(c.mode, 0.0)), seed, _stream()), "cir_eltwise")
    torch.cuda.synchronize()
    bits = buf.view(_INT[c.out])
    intact = bool((bits[:4096 + k] == CANARY[c.out]).all()) and bool((bits[4096 + k + c.n:] == CANARY[c.out]).all())
    return out, intact


@pytest.mark.parametrize("odt", [F32, BF16, F16], ids=lambda d: "out_" + G.DT_NAME[d])
@pytest.mark.parametrize("zdt", [F32, BF16, F16], ids=lambda d: "z_" + G.DT_NAME[d])
@pytest.mark.parametrize("mode", G.ELT_MODES)
def test_eltwise_grid(rt, mode, zdt, odt):
    cases = [c for c in G.CASES["eltwise"] if (c.mode, c.z, c.out) == (mode, zdt, odt)]
    assert [c.n for c in cases] == list(G.ELT_N)
    fails = []
    for c in cases:
        i = G.inputs(c)
        aligned, ok_a = _eltwise(rt, c, i, 0)
        shifted, ok_s = _eltwise(rt, c, i, 1)
        assert ok_a and ok_s, f"{c}: a store outside the output"
        a, s = aligned.cpu(), shifted.cpu()
        if not torch.equal(a.view(_INT[odt]), s.view(_INT[odt])):
            fails.append(f"{c}: the 16-byte path and the scalar path differ in {int((a.view(_INT[odt]) != s.view(_INT[odt])).sum())} elements")
        fails += G.check(c, dict(out=a)) + G.check(c, dict(out=s))
    assert not fails, fails


def test_eltwise_dropout_mask_is_a_function_of_seed_and_flat_index(rt):
    """The kept set of a launch of length m < n is the prefix of the kept set at length n (same seed) - on both paths; another seed
    keeps another set; the kept share lies in the binomial 5-sigma interval around 1 - p, computed from n and p
    (glue_cases.dropout_interval)."""
    n, p = 1 << 20, G.ELT_P["dropout"]
    long = G.Case("eltwise", mode="dropout", z=F32, out=F32, n=n)
    ones = dict(z=torch.ones((n,)), dy=torch.zeros((n,)))
    kept = {}
    for k in (0, 1):
        out, ok = _eltwise(rt, long, ones, k)
        assert ok
        kept[k] = (out != 0).cpu()
    assert torch.equal(kept[0], kept[1])
    assert torch.equal(kept[0], H.splitmix_keep(G.ELT_SEED, n, float(np.float32(p))))
    lo, hi = G.dropout_interval(n, p)
    assert lo <= int(kept[0].sum()) <= hi, (lo, int(kept[0].sum()), hi)
    for m in (1, 3, 1025, 37001):
        short = G.Case("eltwise", mode="dropout", z=F32, out=F32, n=m)
        for k in (0, 1):
            out, ok = _eltwise(rt, short, dict(z=torch.ones((m,)), dy=torch.zeros((m,))), k)
            assert ok and torch.equal((out != 0).cpu(), kept[0][:m]), (m, k)
    other, ok = _eltwise(rt, long, ones, 0, seed=G.ELT_SEED + 1)
    other = (other != 0).cpu()
    assert ok and lo <= int(other.sum()) <= hi
    # two independent masks agree on a share (1-p)^2 + p^2 of the elements: the same interval construction, around that share
    agree, q = int((other == kept[0]).sum()), (1 - p) ** 2 + p ** 2
    alo, ahi = G.dropout_interval(n, 1 - q)
    assert alo <= agree <= ahi, (alo, agree, ahi)


# ------------------------------------------------------------------------------------------------ colsum
@pytest.mark.parametrize("c", G.CASES["colsum"], ids=G.case_id)
def test_colsum(rt, c):
    i = G.inputs(c)
    x = i["buf"].cuda()[:, :c.cols]
    assert x.stride(0) == c.cols + c.pad
    buf, out = _flat_guard(c.cols, F32, slack=256)
    out.copy_(i["out0"])                                             # the contract is +=
    rt.lib.check(rt.c.cir_colsum(x.data_ptr(), x.stride(0), out.data_ptr(), c.rows, c.cols, _stream()), "cir_colsum")
    torch.cuda.synchronize()
    fails = G.check(c, dict(out=out.cpu()))
    assert not fails, fails
    assert _flat_intact(buf, c.cols, F32, slack=256)
    via = i["out0"].cuda()
    rt.T.colsum(x, via)
    torch.cuda.synchronize()
    assert not G.check(c, dict(out=via.cpu()))                       # the wrapper (the order of the atomics is free: not bit-equal)


def test_colsum_refuses_more_row_blocks_than_a_grid_dimension(rt):
    """rows > 65535 * 32 would need more than 65535 blocks in grid.y: CIR_ESHAPE before any launch (ld = 0: one real row)."""
    x, out = torch.zeros((8,), device="cuda"), torch.zeros((8,), device="cuda")
    assert rt.c.cir_colsum(x.data_ptr(), 0, out.data_ptr(), 65535 * 32 + 1, 8, _stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ------------------------------------------------------------------------------------------------ embed_bwd
@pytest.fixture(scope="module")
def dword_table():
    return {}


@pytest.mark.parametrize("c", G.CASES["embed_bwd"], ids=G.case_id)
def test_embed_bwd(rt, dword_table, c):
    i = G.inputs(c)
    ids, dy = i["ids"].cuda(), i["dy"].cuda()
    if dword_table.get("cols") != c.cols:                            # one zeroed (30524, cols) table per width, restored after each case
        dword_table.clear()
        dword_table.update(cols=c.cols, t=torch.zeros((G.VOCAB, c.cols), device="cuda"))
    dword = dword_table["t"]
    buf, dpos = _flat_guard(c.l * c.cols, F32)
    dpos.zero_()
    rt.T.embed_bwd(ids, dy, dword, dpos.view(c.l, c.cols), c.l)
    torch.cuda.synchronize()
    touched = G.embed_bwd_touched(c).cuda()
    got = dword[touched].cpu()
    dword[touched] = 0
    clean = not bool(dword.any())                                    # nothing outside the rows the ids name
    fails = G.check(c, dict(dword=got, dpos=dpos.view(c.l, c.cols).cpu()))
    assert not fails, fails
    assert clean and _flat_intact(buf, c.l * c.cols, F32)
