"""The fixed-order operators of the deterministic training mode (include/cirrank.h, "Fixed-order forms") on a real MI355X, through
`train_ops` with every destination and every workspace inside a canary-filled allocation.  For each operator: three calls on the same
inputs give the same bits; destinations that held a value come out as old + sum; the values agree with float64 within the a-priori
bound of a sum of that many fp32 terms (column sum, embedding adjoint) or with the default (atomic) operator's output within the
comparison tests/test_train_ops_gpu.py applies to that operator (LayerNorm adjoints, weight gradients); a workspace that is too small
is refused with CIR_ESHAPE before anything is written.

Shapes: the row counts sit around each kernel's rows per workgroup (32 for the LayerNorm adjoints, 64 for the 16-bit row kernel, 256 per
first-level block of the ordered column sum, 512 per chunk of the embedding adjoint, 64-row steps of the weight gradient): one row, exactly
one workgroup, one more, three workgroups and a ragged rest."""
import pytest
import torch

from tests import glue_cases as G
from tests.test_guard_gpu import _INT, _flat_guard, _flat_intact

pytestmark = pytest.mark.gpu
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
U, SUB32 = G.U, G.SUB32
ESHAPE = -2


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    return train_ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _r(shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).cuda()


class GuardedWork:
    """train_ops.Workspace whose buffers are EXACTLY as large as asked for and sit between canaries (a kernel that needs more than the
    wrapper sized would write into them)."""

    def __init__(self):
        self.bufs = []

    def _get(self, n, dtype):
        n = max(int(n), 1)
        buf, view = _flat_guard(n, dtype) if dtype == F32 else (None, None)
        if dtype != F32:
            buf = torch.full((n + 2 * 4096,), 0x7EADBEEF, dtype=torch.int32, device="cuda")
            view = buf[4096:4096 + n]
        self.bufs.append((buf, n, dtype))
        return view

    def f32(self, n, device):
        return self._get(n, F32)

    def i32(self, n, device):
        return self._get(n, torch.int32)

    def intact(self):
        torch.cuda.synchronize()
        ok = True
        for buf, n, dtype in self.bufs:
            if dtype == F32:
                ok = ok and _flat_intact(buf, n, F32)
            else:
                ok = ok and bool((buf[:4096] == 0x7EADBEEF).all()) and bool((buf[4096 + n:] == 0x7EADBEEF).all())
        return ok


def _vec(old):
    """A guarded fp32 vector holding `old` (the destinations are accumulated into)."""
    buf, v = _flat_guard(old.numel(), F32, slack=256)
    v.copy_(old)
    return buf, v


def _thrice(run):
    """run() -> (tuple of result tensors, list of guards); three calls, bit-equal results, guards intact; returns the first results."""
    first = None
    for _ in range(3):
        res, guards = run()
        torch.cuda.synchronize()
        for g in guards:
            assert g()
        res = [None if t is None else t.clone() for t in res]
        if first is None:
            first = res
        else:
            for a, b in zip(first, res):
                assert (a is None and b is None) or torch.equal(a.view(_INT.get(a.dtype, a.dtype)), b.view(_INT.get(b.dtype, b.dtype)))
    return first


LN_ROWS = (1, 32, 33, 101)            # 32 rows per workgroup: one row, one workgroup, one more, three workgroups + a ragged 5
R16_ROWS = (1, 64, 65, 197)           # 64 rows per workgroup
COLS = (64, 768, 1024)


# ------------------------------------------------------------------------------------------------ site 1: cir_layernorm_bwd_ordered
@pytest.mark.parametrize("cols", COLS)
def test_layernorm_bwd_ordered(T, cols):
    for rows in LN_ROWS:
        x, dy = _r((rows, cols), 8 + rows, 2.0) + 0.3, _r((rows, cols), 9 + rows)
        g = _r((cols,), 10) * 0.1 + 1.0
        old_g, old_b = _r((cols,), 11), _r((cols,), 12)

        def run():
            w = GuardedWork()
            (bg, dg), (bb, db) = _vec(old_g), _vec(old_b)
            dx = T.layernorm_bwd(x, g, dy, dg, db, 1e-12, work=w)
            return (dx, dg, db), [w.intact, lambda: _flat_intact(bg, cols, F32, slack=256), lambda: _flat_intact(bb, cols, F32, slack=256)]
        dx, dg, db = _thrice(run)
        rg, rb = old_g.clone(), old_b.clone()
        rx = T.layernorm_bwd(x, g, dy, rg, rb, 1e-12)                                # the default operator: same sums, free order
        assert torch.equal(dx, rx)
        torch.testing.assert_close(dg, rg, atol=2e-3, rtol=1e-4)                     # (tests/test_train_ops_gpu.py::test_layernorm_bwd's comparison)
        torch.testing.assert_close(db, rb, atol=2e-3, rtol=1e-4)
        # db is a plain column sum of dy on top of the old value: float64 within (rows + 3) u of the absolute sum
        ref = old_b.double() + dy.double().sum(0)
        assert bool(((db.double() - ref).abs() <= (rows + 3) * U * (dy.double().abs().sum(0) + old_b.double().abs()) + SUB32).all())


def test_ordered_row_kernels_refuse_a_small_workspace(T):
    """One element short of ceil(rows / 32) * 2 (or 3) * cols, ceil(rows / 64) * cols: CIR_ESHAPE, nothing written."""
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    rows, cols = 33, 64
    x, dy, g = _r((rows, cols), 1), _r((rows, cols), 2), _r((cols,), 3)
    dx = torch.zeros((rows, cols), device="cuda")
    dg, db, b1 = (torch.zeros((cols,), device="cuda") for _ in range(3))
    part = torch.zeros((2 * 3 * cols,), device="cuda")
    assert c.cir_layernorm_bwd_ordered(x.data_ptr(), g.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, cols, 1e-12,
                                       part.data_ptr(), 2 * 2 * cols - 1, _stream()) == ESHAPE
    dt16 = torch.zeros((rows, cols), dtype=BF, device="cuda")
    args = (x.data_ptr(), g.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), None, dt16.data_ptr())
    tail = (rows, cols, 1e-12, 1.0, 0.0, 0, lib.CIR_BF16, part.data_ptr())
    assert c.cir_layernorm_bwd_fused_ordered(*args, b1.data_ptr(), None, *tail, 2 * 3 * cols - 1, _stream()) == ESHAPE
    assert c.cir_layernorm_bwd_fused_ordered(*args, None, None, *tail, 2 * 2 * cols - 1, _stream()) == ESHAPE
    a16 = _r((65, cols), 4, dtype=BF)
    assert c.cir_rows16_colsum_ordered(a16.data_ptr(), cols, None, 0, None, 0, b1.data_ptr(), 65, cols, 0, lib.CIR_BF16, part.data_ptr(),
                                       2 * cols - 1, _stream()) == ESHAPE
    xs = torch.zeros((257, 8), device="cuda")
    assert c.cir_colsum_ordered(xs.data_ptr(), 8, dg.data_ptr(), 257, 8, part.data_ptr(), 2 * 8 - 1, _stream()) == ESHAPE
    assert c.cir_colsum_ordered(xs.data_ptr(), 7, dg.data_ptr(), 3, 8, part.data_ptr(), 64, _stream()) == ESHAPE          # ld < cols
    ids = torch.zeros((513,), dtype=torch.int64, device="cuda")
    dyw, table, dpos = torch.zeros((513, 8), device="cuda"), torch.zeros((50, 8), device="cuda"), torch.zeros((8,), device="cuda")
    big, index = torch.zeros((3 * 513 * 8,), device="cuda"), torch.zeros((128,), dtype=torch.int32, device="cuda")
    emb = (ids.data_ptr(), dyw.data_ptr(), table.data_ptr(), dpos.data_ptr(), 513, 1, 8, 50, big.data_ptr())
    assert c.cir_embed_bwd_ordered(*emb, 513 * 8 - 1, index.data_ptr(), 100, _stream()) == ESHAPE                          # fp32 partials short
    assert c.cir_embed_bwd_ordered(*emb, big.numel(), index.data_ptr(), 99, _stream()) == ESHAPE                           # index short (2 chunks x 50)
    torch.cuda.synchronize()
    for t in (dx, dg, db, b1, part, table, dpos, big):
        assert not bool(t.any())
    assert not bool(dt16.any()) and not bool(index.any())


# ------------------------------------------------------------------------------------------------ site 2: cir_layernorm_bwd_fused_ordered
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("variant", ["dx_only", "dt", "dt_b1", "dt_b1_b2_tadd"])
@pytest.mark.parametrize("cols", COLS)
def test_layernorm_bwd_fused_ordered(T, cols, variant, dtype):
    p, seed, eps = 0.1, 4242, 1e-12
    for rows in LN_ROWS:
        pre, dy = _r((rows, cols), 31 + rows, 2.0), _r((rows, cols), 36 + rows)
        gam = _r((cols,), 34) * 0.1 + 1.0
        t_add = _r((rows, cols), 37, 0.5) if variant == "dt_b1_b2_tadd" else None
        olds = [_r((cols,), 40 + i) for i in range(3)]
        olds.append(olds[2].clone())
        want_dt, n_bias = variant != "dx_only", {"dx_only": 0, "dt": 0, "dt_b1": 1, "dt_b1_b2_tadd": 2}[variant]

        def call(vecs, **kw):
            return T.layernorm_bwd_fused(pre, gam, dy, vecs[0], vecs[1], eps, dtype, t_add=t_add, dbias=vecs[2] if n_bias > 0 else None,
                                         dbias2=vecs[3] if n_bias > 1 else None, alpha=0.5, p_drop=p, seed=seed, want_dt=want_dt, **kw)

        def run():
            w = GuardedWork()
            gv = [_vec(o) for o in olds]
            dx, dt16 = call([v for _, v in gv], work=w)
            return (dx, dt16, *[v for _, v in gv]), [w.intact] + [(lambda b=b: _flat_intact(b, cols, F32, slack=256)) for b, _ in gv]
        dx, dt16, *vecs = _thrice(run)
        ref = [o.clone() for o in olds]
        rx, rt16 = call(ref)                                                         # the default operator
        assert torch.equal(dx, rx) and (dt16 is None) == (rt16 is None) and (dt16 is None or torch.equal(dt16.view(torch.int16), rt16.view(torch.int16)))
        torch.testing.assert_close(vecs[0], ref[0], atol=2e-3, rtol=1e-4)            # dgamma, dbeta: test_residual_layernorm_train_and_adjoint's
        torch.testing.assert_close(vecs[1], ref[1], atol=2e-3, rtol=1e-4)
        for i in range(2, 2 + n_bias):
            torch.testing.assert_close(vecs[i], ref[i], atol=3e-3, rtol=1e-4)        # ... and its bias-sum comparison
        for i in range(2 + n_bias, 4):
            assert torch.equal(vecs[i], olds[i])                                     # a destination that was not asked for is not touched
        if n_bias == 2:
            assert torch.equal(vecs[2], vecs[3])                                     # one sum, two destinations that held the same value


# ------------------------------------------------------------------------------------------------ site 3: cir_rows16_colsum_ordered
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["sums", "gelu_bwd"])
@pytest.mark.parametrize("cols", COLS)
def test_rows16_colsum_ordered(T, cols, mode, dtype):
    for rows in R16_ROWS:
        wide = _r((rows, cols + 8), 41 + rows, dtype=dtype)
        a, z = wide[:, :cols], _r((rows, cols), 42 + rows, 2.0, dtype=dtype)          # a: a strided view (row stride cols + 8)
        old = _r((cols,), 43)

        def run():
            w = GuardedWork()
            bs, sums = _vec(old)
            out = T.colsum16(a, sums, work=w) if mode == "sums" else T.gelu_bwd16(a, z, sums=sums, work=w)
            return ((None if mode == "sums" else out), sums), [w.intact, lambda: _flat_intact(bs, cols, F32, slack=256)]
        out, sums = _thrice(run)
        ref = old.clone()
        if mode == "sums":
            T.colsum16(a, ref)
            terms = a.double()
        else:
            rout = T.gelu_bwd16(a, z, sums=ref)
            assert torch.equal(out.view(torch.int16), rout.view(torch.int16))
            terms = None
        torch.testing.assert_close(sums, ref, atol=2e-3, rtol=1e-4)                  # (test_rows16_colsum_and_gelu_adjoint's column-sum comparison)
        if terms is not None:                                                        # a plain sum of 16-bit values: float64 within (rows + 3) u
            r64 = old.double() + terms.sum(0)
            assert bool(((sums.double() - r64).abs() <= (rows + 3) * U * (terms.abs().sum(0) + old.double().abs()) + SUB32).all())


# ------------------------------------------------------------------------------------------------ site 4: cir_colsum_ordered
CS_ROWS = (1, 3, 257, 1283)           # 256 rows per first-level block: one block + 1, five blocks + 3
CS_COLS = (1, 255, 256, 257, 3072)


@pytest.mark.parametrize("pad", [0, 8], ids=["dense", "ld_gt_cols"])
@pytest.mark.parametrize("cols", CS_COLS)
@pytest.mark.parametrize("rows", CS_ROWS)
def test_colsum_ordered(T, rows, cols, pad):
    """Against float64 within the bound tests/glue_cases.py derives for cir_colsum: R rows and the value already there are R + 1 terms
    summed in fp32 in some order, (R + 3) u * (sum |x| + |old|)."""
    g = torch.Generator().manual_seed(rows * 7919 + cols + pad)
    buf = torch.randn((rows, cols + pad), generator=g)
    old = torch.randn((cols,), generator=g) * 4.0
    x = buf.cuda()[:, :cols]
    assert x.stride(0) == cols + pad

    def run():
        w = GuardedWork()
        bo, out = _vec(old.cuda())
        T.colsum(x, out, work=w)
        return (out,), [w.intact, lambda: _flat_intact(bo, cols, F32, slack=256)]
    (out,) = _thrice(run)
    ref = old.double() + buf[:, :cols].double().sum(0)
    bound = (rows + 3) * U * (buf[:, :cols].double().abs().sum(0) + old.double().abs()) + SUB32
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ site 5: cir_embed_bwd_ordered
def _embed_case(kind, rows, table, cols, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "equal":
        ids = torch.full((rows,), table - 1, dtype=torch.int64)                      # every row on the LAST row of the table
    elif kind == "distinct":
        ids = torch.randperm(table, generator=g)[:rows]
    else:
        ids = torch.randint(0, table, (rows,), generator=g)
        ids[0] = 0
        ids[rows // 2] = ids[rows - 1]
    return ids, torch.randn((rows, cols), generator=g)


# (rows, L, table rows, cols, id pattern): 96 rows as one id / all distinct / mixed at L = 1 and 5 (96 = 19 sequences of 5 and one row: a
# ragged last sequence), a 50-row table; and 1100 rows - three 512-row chunks, 1100 sequences of one row (five 256-blocks of the dpos sum) and
# 220 of five - on the 50-row table, where every id recurs in every chunk
EMB_CASES = [(96, l, tb, 64, k) for l in (1, 5) for tb, k in ((30524, "equal"), (30524, "distinct"), (30524, "mixed"), (50, "equal"), (50, "mixed"))]
EMB_CASES += [(1100, 1, 50, 64, "mixed"), (1100, 5, 50, 72, "equal"), (1100, 5, 2000, 64, "mixed")]


@pytest.fixture(scope="module")
def tables():
    return {}


@pytest.mark.parametrize("rows,l,table,cols,kind", EMB_CASES, ids=lambda v: str(v))
def test_embed_bwd_ordered(T, tables, rows, l, table, cols, kind):
    """dword / dpos against float64: a destination that collects n rows on top of its old value is a sum of n + 1 fp32 terms in some order,
    (n + 3) u * (sum |dy| + |old|) - the bound tests/glue_cases.py derives for cir_embed_bwd, with the old value as one more term.  Rows of
    the table that no id names keep their bits."""
    ids, dy = _embed_case(kind, rows, table, cols, rows + l + table)
    key = (table, cols)
    if key not in tables:
        tables[key] = _r((table, cols), 77)
    old_w, old_p = tables[key], _r((l, cols), 78)
    ids_d, dy_d = ids.cuda(), dy.cuda()

    def run():
        w = GuardedWork()
        bw, dword = _flat_guard(table * cols, F32)
        dword.copy_(old_w.view(-1))
        bp, dpos = _vec(old_p.view(-1))
        T.embed_bwd(ids_d, dy_d, dword.view(table, cols), dpos.view(l, cols), l, work=w)
        return (dword.view(table, cols), dpos.view(l, cols)), [w.intact, lambda: _flat_intact(bw, table * cols, F32),
                                                               lambda: _flat_intact(bp, l * cols, F32, slack=256)]
    dword, dpos = _thrice(run)
    touched, inv = torch.unique(ids, return_inverse=True)
    d64 = dy.double()
    sw = torch.zeros((touched.numel(), cols), dtype=torch.float64).index_add_(0, inv, d64)
    aw = torch.zeros_like(sw).index_add_(0, inv, d64.abs())
    cnt = torch.zeros((touched.numel(), 1), dtype=torch.float64).index_add_(0, inv, torch.ones((rows, 1), dtype=torch.float64))
    oldw = old_w.cpu().double()[touched]
    err = (dword.cpu().double()[touched] - (oldw + sw)).abs()
    assert bool((err <= (cnt + 3) * U * (aw + oldw.abs()) + SUB32).all())
    rest = torch.ones((table,), dtype=torch.bool)
    rest[touched] = False
    assert torch.equal(dword.cpu()[rest], old_w.cpu()[rest])
    pos = torch.arange(rows) % l
    sp = torch.zeros((l, cols), dtype=torch.float64).index_add_(0, pos, d64)
    ap = torch.zeros_like(sp).index_add_(0, pos, d64.abs())
    npos = torch.zeros((l, 1), dtype=torch.float64).index_add_(0, pos, torch.ones((rows, 1), dtype=torch.float64))
    oldp = old_p.cpu().double()
    errp = (dpos.cpu().double() - (oldp + sp)).abs()
    assert bool((errp <= (npos + 3) * U * (ap + oldp.abs()) + SUB32).all())


def test_embed_bwd_ordered_skips_ids_outside_the_table(T):
    ids = torch.tensor([3, 50, -1, 3, 49, 10 ** 12], dtype=torch.int64).cuda()
    dy = torch.ones((6, 8), device="cuda")
    w = GuardedWork()
    bw, dword = _flat_guard(50 * 8, F32)
    dword.zero_()
    dpos = torch.zeros((2, 8), device="cuda")
    T.embed_bwd(ids, dy, dword.view(50, 8), dpos, 2, work=w)
    assert w.intact() and _flat_intact(bw, 50 * 8, F32)
    want = torch.zeros((50, 8))
    want[3], want[49] = 2.0, 1.0
    assert torch.equal(dword.view(50, 8).cpu(), want) and torch.equal(dpos.cpu(), torch.full((2, 8), 3.0))


# ------------------------------------------------------------------------------------------------ sites 6, 7: unsplit weight gradients
WG_ROWS = (37, 64, 320, 357)          # a tail alone; one 64-row step; five steps; five steps + a tail of 37


def _wgrad_close(dw, ref, old):
    """tests/test_train_ops_gpu.py::test_wgrad_kernel's comparison, here against the default (split, atomic) operator's output."""
    err = ((dw - old) - (ref - old)).abs().max().item()
    assert err < 2e-3 * max(1.0, (ref - old).abs().max().item()), err


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,k", [(128, 128), (256, 128)])
@pytest.mark.parametrize("rows", WG_ROWS)
def test_wgrad_unsplit_repeats(T, rows, n, k, dtype):
    wide_y, wide_x = _r((rows, n + 128), 51 + rows, dtype=dtype), _r((rows, k + 256), 52 + rows, dtype=dtype)
    dy, x = wide_y[:, 128:], wide_x[:, 128:128 + k]

    def run():
        buf, dw = _flat_guard(n * k, F32)
        dw.fill_(0.25)
        T.wgrad(dy, x, dw.view(n, k), splits=1)
        return (dw.view(n, k),), [lambda: _flat_intact(buf, n * k, F32)]
    (dw,) = _thrice(run)
    ref = torch.full((n, k), 0.25, device="cuda")
    T.wgrad(dy, x, ref)                                                              # splits chosen from the shape: atomics where it splits
    _wgrad_close(dw, ref, 0.25)
    _wgrad_close(dw, dy.float().t() @ x.float() + 0.25, 0.25)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_wgrad_grouped_unsplit_repeats(T, dtype):
    shapes = [(37, 128, 128), (320, 256, 128), (357, 128, 128)]
    ops_ = [(_r((r, n), 60 + i, dtype=dtype), _r((r, k), 70 + i, dtype=dtype)) for i, (r, n, k) in enumerate(shapes)]

    def run():
        guards, dws = [], []
        for i, (r, n, k) in enumerate(shapes):
            buf, dw = _flat_guard(n * k, F32)
            dw.fill_(float(i + 1))
            guards.append(lambda b=buf, m=n * k: _flat_intact(b, m, F32))
            dws.append(dw.view(n, k))
        T.wgrad_grouped([(dy, x, dw) for (dy, x), dw in zip(ops_, dws)], splits=1)
        return tuple(dws), guards
    dws = _thrice(run)
    refs = [torch.full((n, k), float(i + 1), device="cuda") for i, (r, n, k) in enumerate(shapes)]
    T.wgrad_grouped([(dy, x, dw) for (dy, x), dw in zip(ops_, refs)])
    for i, (dw, ref) in enumerate(zip(dws, refs)):
        _wgrad_close(dw, ref, float(i + 1))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_small_linear_weight_gradient_unsplit(T, dtype):
    """cls_head's 768 -> 2 Linear at 100 rows (off the 128 grid: cir_bmm): the deterministic route of `_Lin.bwd16` - one batch item,
    accumulate = 1 - against its default route (row chunks that share dW through atomics)."""
    rows, n, k = 100, 2, 768
    dy16, x16 = _r((rows, n), 81, dtype=dtype), _r((rows, k), 82, dtype=dtype)

    def run():
        buf, dw = _flat_guard(n * k, F32)
        dw.fill_(0.5)
        T.bmm(dy16.unsqueeze(0), x16.unsqueeze(0), True, False, out=dw.view(1, n, k), accumulate=True)
        return (dw.view(n, k),), [lambda: _flat_intact(buf, n * k, F32)]
    (dw,) = _thrice(run)
    ref = torch.full((n, k), 0.5, device="cuda")
    T.bmm(dy16.unflatten(0, (2, 50)), x16.unflatten(0, (2, 50)), True, False, out=ref.unsqueeze(0).expand(2, n, k), accumulate="atomic")
    _wgrad_close(dw, ref, 0.5)
    _wgrad_close(dw, dy16.float().t() @ x16.float() + 0.5, 0.5)
