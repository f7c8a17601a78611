"""The stage-I ranking kernels and the inference glue on a real MI355X, against the float64 references and the a-priori bounds of
tests/glue_cases.py (checked without a GPU by tests/test_glue_cases_cpu.py).  Every entry point is called through the C ABI with its
output inside a canary-filled allocation (tests/test_guard_gpu.py): the tail-shaped cases - a partial last block, a row count that
is not a multiple of the rows per workgroup - must leave every byte outside the output as it was."""
import pytest
import torch

from tests import glue_cases as G
from tests.test_guard_gpu import _flat_guard, _flat_intact

pytestmark = pytest.mark.gpu

BF16, F16, F32 = G.BF16, G.F16, G.F32


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import lib, ops, validate

    class RT:
        pass
    r = RT()
    r.lib, r.c, r.ops, r.validate = lib, lib.load(), ops, validate
    r.DT = {BF16: lib.CIR_BF16, F16: lib.CIR_F16, F32: lib.CIR_F32}
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.cuda()


def _strided_dev(i):
    """The operand x on the device with the strides of the case: a contiguous matrix, or the rows h[:, 0, :] of an (M, L, K) tensor."""
    h = i["h"].cuda()
    return h, (h[:, 0, :] if h.dim() == 3 else h)


def _assert_ok(case, outputs, guards):
    fails = G.check(case, {k: v.cpu() for k, v in outputs.items()})
    assert not fails, fails
    for buf, n, dtype, slack in guards:
        assert _flat_intact(buf, n, dtype, slack=slack), f"{case}: a store outside the output"


# ------------------------------------------------------------------------------------------------ linear_f32
def _linear(rt, x, w, bias, mode, guards=None):
    (m, k), n = x.shape, w.shape[0]
    buf, y = _flat_guard(m * n, F32)
    rt.lib.check(rt.c.cir_linear_f32(x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(bias), y.data_ptr(), m, n, k, mode, _stream()), "cir_linear_f32")
    torch.cuda.synchronize()
    if guards is not None:
        guards.append((buf, m * n, F32, 4096))
    return y.view(m, n)


@pytest.mark.parametrize("c", G.CASES["linear_f32"], ids=G.case_id)
def test_linear_f32(rt, c):
    i = G.inputs(c)
    _, x = _strided_dev(i)
    assert x.stride(0) == (3 if c.strided else 1) * c.mnk[2]
    guards = []
    y = _linear(rt, x, i["w"].cuda(), _dev(i["bias"]), c.mode, guards)
    _assert_ok(c, dict(y=y), guards)


@pytest.mark.parametrize("c", [c for c in G.CASES["linear_f32"] if c.mode == 2], ids=G.case_id)
def test_linear_f32_mode2_is_the_exact_negative_of_mode1(rt, c):
    """include/cirrank.h: mode 2 is 'the exact negative of mode 1' - bit for bit, so that ranking by descending mode 2 IS ranking by
    ascending distance, ties included."""
    i = G.inputs(c)
    _, x = _strided_dev(i)
    w, bias = i["w"].cuda(), _dev(i["bias"])
    assert torch.equal(_linear(rt, x, w, bias, 2), -_linear(rt, x, w, bias, 1))
    assert torch.equal(rt.ops.linear_f32(x, w, bias, mode=2), -rt.ops.linear_f32(x, w, bias, mode=1))      # and through the wrapper


def test_linear_f32_refuses_more_row_blocks_than_a_grid_dimension(rt):
    """M > 65535 * 64 rows would need more than 65535 blocks in grid.y: CIR_ESHAPE before any launch (the tensors here are one tile)."""
    x, w, y = torch.zeros((64, 16), device="cuda"), torch.zeros((1, 16), device="cuda"), torch.zeros((64,), device="cuda")
    code = rt.c.cir_linear_f32(x.data_ptr(), 16, w.data_ptr(), None, y.data_ptr(), 65535 * 64 + 1, 1, 16, 0, _stream())
    torch.cuda.synchronize()
    assert code == -2                                                # CIR_ESHAPE
    with pytest.raises(rt.lib.CirrankError, match="extent not supported"):
        rt.lib.check(code, "cir_linear_f32")


# ------------------------------------------------------------------------------------------------ l2_normalize
@pytest.mark.parametrize("c", G.CASES["l2_normalize"], ids=G.case_id)
def test_l2_normalize(rt, c):
    x = G.inputs(c)["x"].cuda()
    buf, y = _flat_guard(c.rows * c.cols, F32)
    rt.lib.check(rt.c.cir_l2_normalize(x.data_ptr(), y.data_ptr(), c.rows, c.cols, _stream()), "cir_l2_normalize")
    torch.cuda.synchronize()
    y = y.view(c.rows, c.cols)
    _assert_ok(c, dict(y=y), [(buf, c.rows * c.cols, F32, 4096)])
    if c.special == "zero_row":
        assert bool((y[c.rows // 2] == 0).all())                     # zeros, not 0 / 0
    assert torch.equal(rt.ops.l2_normalize(x), y)                    # the wrapper runs the same launch


# ------------------------------------------------------------------------------------------------ argsort_desc
@pytest.mark.parametrize("c", G.CASES["argsort_desc"], ids=G.case_id)
def test_argsort_desc(rt, c):
    logits = G.inputs(c)["logits"].cuda()
    buf, idx = _flat_guard(c.q * c.k, torch.int64, slack=512)
    rt.lib.check(rt.c.cir_topk_desc(logits.data_ptr(), idx.data_ptr(), c.q, c.k, _stream()), "cir_topk_desc")
    torch.cuda.synchronize()
    _assert_ok(c, dict(idx=idx.view(c.q, c.k)), [(buf, c.q * c.k, torch.int64, 512)])


def test_argsort_desc_refuses_more_than_8192_columns(rt):
    """8192 (value, index) pairs fill the 64 KiB of LDS one workgroup may ask for: K = 8193 is CIR_ESHAPE, returned before any launch."""
    logits = torch.zeros((1, 8193), device="cuda")
    with pytest.raises(rt.lib.CirrankError, match=r"extent not supported.*code -2"):
        rt.ops.argsort_desc(logits)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ rank_index at dataset scale
@pytest.mark.parametrize("c", G.CASES["rank_index"], ids=G.case_id)
def test_rank_index_dataset_scale(rt, c):
    """(a) the order is bit for bit the stable descending argsort of the kernel's own mode-2 matrix (the sort alone);
    (b) along every returned row the float64 distance never falls below its running maximum by more than 2 max(bound);
    and the matrix itself meets the float64 distances within the bound."""
    i = G.inputs(c)
    pred, index = i["pred"].cuda(), i["index"].cuda()
    order = rt.validate.rank_index(pred, index)
    neg = rt.ops.linear_f32(pred, index, None, mode=2)
    torch.cuda.synchronize()
    fails = G.check(c, dict(dist=-neg.cpu())) + G.rank_failures(c, order.cpu(), neg.cpu())
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ gather_rows
@pytest.mark.parametrize("c", G.CASES["gather_rows"], ids=G.case_id)
def test_gather_rows(rt, c):
    i = G.inputs(c)
    src, index = i["src"].cuda(), _dev(i["index"])
    n = c.n_rows * c.row_elems
    buf, dst = _flat_guard(n, c.dst)
    rt.lib.check(rt.c.cir_gather_rows(src.data_ptr(), rt.DT[c.src], _ptr(index), dst.data_ptr(), rt.DT[c.dst], c.n_rows, c.row_elems, c.src_rows,
                                      _stream()), "cir_gather_rows")
    torch.cuda.synchronize()
    _assert_ok(c, dict(dst=dst.view(c.n_rows, c.row_elems)), [(buf, n, c.dst, 4096)])
    assert torch.equal(rt.ops.gather_rows(src, index, c.dst), dst.view(c.n_rows, c.row_elems))


# ------------------------------------------------------------------------------------------------ patchify
def _patchify(rt, c, image, guards):
    b, ch, h, w = image.shape
    n = b * ch * h * w
    buf, out = _flat_guard(n, c.dst)
    rt.lib.check(rt.c.cir_patchify(image.data_ptr(), rt.DT[c.src], out.data_ptr(), rt.DT[c.dst], b, ch, h, w, 16, _stream()), "cir_patchify")
    torch.cuda.synchronize()
    guards.append((buf, n, c.dst, 4096))
    return out.view(-1, ch * 256)


@pytest.mark.parametrize("c", G.CASES["patchify"], ids=G.case_id)
def test_patchify(rt, c):
    i = G.inputs(c)
    store = i["storage"].cuda()
    image = store[c.offset:].view(i["image"].shape)
    assert image.data_ptr() % 16 == (c.offset * store.element_size()) % 16 and image.is_contiguous()
    guards = []
    out = _patchify(rt, c, image, guards)
    _assert_ok(c, dict(patches=out), guards)
    wrapped = rt.ops.patchify(image, 16, c.dst)                      # .contiguous() leaves a contiguous view where it is: same pointer, same path
    torch.cuda.synchronize()
    assert torch.equal(wrapped, out)
    if c.offset:                                                     # the scalar path against the vector path on an aligned copy, bit for bit
        assert torch.equal(out, _patchify(rt, c, image.clone(), guards))
        assert all(_flat_intact(b, n, d, slack=s) for b, n, d, s in guards)


# ------------------------------------------------------------------------------------------------ vit_assemble
@pytest.mark.parametrize("c", G.CASES["vit_assemble"], ids=G.case_id)
def test_vit_assemble(rt, c):
    (b, p, d), i = c.bpd, G.inputs(c)
    proj, cls, pos = i["proj"].cuda(), i["cls"].cuda(), i["pos"].cuda()
    n = b * (p + 1) * d
    buf, x = _flat_guard(n, c.stream)
    rt.lib.check(rt.c.cir_vit_assemble(proj.data_ptr(), cls.data_ptr(), pos.data_ptr(), x.data_ptr(), rt.DT[c.stream], b, p, d, _stream()), "cir_vit_assemble")
    torch.cuda.synchronize()
    x = x.view(b, p + 1, d)
    _assert_ok(c, dict(x=x), [(buf, n, c.stream, 4096)])
    if c.stream == F16:
        assert torch.equal(x[:, 1:], (proj.float().view(b, p, d) + pos[1:]).half())
        assert torch.equal(x[:, 0], (cls + pos[0]).half().expand(b, d))
    assert torch.equal(rt.ops.vit_assemble(proj, cls, pos, b), x)


# ------------------------------------------------------------------------------------------------ small_linear
@pytest.mark.parametrize("c", G.CASES["small_linear"], ids=G.case_id)
def test_small_linear(rt, c):
    i = G.inputs(c)
    _, x = _strided_dev(i)
    w, bias = i["w"].cuda(), _dev(i["bias"])
    assert x.stride(0) == (2 if c.strided else 1) * c.k
    buf, y = _flat_guard(c.m * c.n, F32, slack=256)
    rt.lib.check(rt.c.cir_small_linear(x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(bias), y.data_ptr(), c.m, c.n, c.k, rt.DT[c.dt], _stream()),
                 "cir_small_linear")
    torch.cuda.synchronize()
    _assert_ok(c, dict(y=y.view(c.m, c.n)), [(buf, c.m * c.n, F32, 256)])
    assert torch.equal(rt.ops.small_linear(x, w, bias), y.view(c.m, c.n))


# ------------------------------------------------------------------------------------------------ embed_layernorm
@pytest.fixture(scope="module")
def tables():
    cache = {}

    def get(cols):
        if cols not in cache:
            cache.clear()                                            # one width on the device at a time (the widest table is 125 MB)
            cache[cols] = tuple(t.cuda() for t in G.embed_tables(cols))
        return cache[cols]
    return get


@pytest.mark.parametrize("c", G.CASES["embed_layernorm"], ids=G.case_id)
def test_embed_layernorm(rt, tables, c):
    i = G.inputs(c)
    word, pos, gamma, beta = tables(c.cols)
    ids = i["ids"].cuda()
    rows, n = 3 * c.l, 3 * c.l * c.cols
    bs, ys = _flat_guard(n, c.stream)
    guards = [(bs, n, c.stream, 4096)]
    y16 = None
    if c.dt16 != F32:
        b16, y16 = _flat_guard(n, c.dt16)
        guards.append((b16, n, c.dt16, 4096))
    rt.lib.check(rt.c.cir_embed_layernorm(ids.data_ptr(), word.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ys.data_ptr(),
                                          rt.DT[c.stream], _ptr(y16), rows, c.l, c.cols, G.VOCAB, G.EMBED_EPS,
                                          rt.lib.CIR_F16 if y16 is None else rt.DT[c.dt16], _stream()), "cir_embed_layernorm")
    torch.cuda.synchronize()
    outs = dict(stream=ys.view(3, c.l, c.cols))
    if y16 is not None:
        outs["y16"] = y16.view(3, c.l, c.cols)
    _assert_ok(c, outs, guards)
    w_s, w_16 = rt.ops.embed_layernorm(ids, word, pos, gamma, beta, G.EMBED_EPS, dtype16=c.dt16, stream_dtype=c.stream)
    torch.cuda.synchronize()
    assert torch.equal(w_s, outs["stream"]) and torch.equal(w_16, outs.get("y16", outs["stream"]))
