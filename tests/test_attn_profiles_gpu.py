"""The online-softmax attention kernels on the MI355X against float64 within the a-priori bounds of tests/attn_cases.py, on inputs whose
scores are dialled so that the running maximum MOVES behind the first key tile (ramps, steps, a saw, spikes; uniform and reversed rows in
the same 32-row tile; -10000 and finfo.min masks on tails, on the whole first tile, on every key): cir_attention on every path of its
dispatch (16-bit: softmax_tile's lazy rescale; fp32: softmax_plain), cir_cls_cross_attention, cir_attention_train_fwd / _bwd.
One launch per case, its items carrying the eight profiles; every element of every output is compared, outputs are pre-filled with NaN
and sit between NaN canaries that must stay untouched.  tests/test_attn_cases_cpu.py shows what the comparison lets through."""
import pytest
import torch

from tests import attn_cases as A

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    return train_ops


def _framed(shape, dtype, pad_cols=0):
    """A NaN buffer with one canary row above and below (and `pad_cols` canary columns right of) the view that is returned with it."""
    *lead, rows, cols = shape
    buf = torch.full((*lead, rows + 2, cols + pad_cols), NAN, dtype=dtype, device="cuda")
    return buf, buf[..., 1:rows + 1, :cols]


def _gaps_untouched(buf, view):
    """Everything of `buf` outside `view` is still NaN, everything inside was written."""
    seen = torch.isnan(buf)
    inside = torch.zeros_like(seen)
    inside[..., 1:view.shape[-2] + 1, :view.shape[-1]] = True
    return bool(seen[~inside].all()) and not bool(torch.isnan(view).any())


def _report(case, outputs):
    fails = A.check(case, outputs)
    print(f"\n[{case}] largest error / bound: " + "  ".join(f"{n} {w:.3f}" for n, w in A.worst_ratio(case, outputs).items()))
    assert not fails, fails


def _attention(ops, c, lq, lk, pad_cols=0, forced_stream=False):
    from candidate_reranking_cir_amd import lib
    i = A.inputs(c)
    q, k, v = (A.to_launch(i[n]).cuda() for n in ("q", "k", "v"))
    mask = None if i["mask"] is None else i["mask"].view(A.NP, 1, lk).cuda()
    buf, out = _framed((A.NP, 1, lq, A.H * 64), c.dt, pad_cols)
    if forced_stream:
        lib.set_tuning(lib.TUNE_ATTN_SHARED_MAX, -1)
    try:
        ops.attention(q, k, v, out, A.SCALE, mask)
        torch.cuda.synchronize()
    finally:
        if forced_stream:
            lib.set_tuning(lib.TUNE_ATTN_SHARED_MAX, 0)
    assert _gaps_untouched(buf, out), f"{c}: a canary was overwritten or an output element was not written"
    _report(c, dict(out=A.from_launch(out.cpu())))


@pytest.mark.parametrize("case", A.CASES["attention"], ids=A.case_id)
def test_attention_profiles(ops, case):
    """cir_attention, 16-bit operands: stream kernel (one query tile; Lk > 608; forced), shared kernel with wide stores, with plain
    stores (by the LDS rule, by an output row stride of 132 elements), in two rounds (attn_cases.ATTN_PATHS)."""
    lq, lk, pad_cols, forced = A.ATTN_PATHS[case.path]
    _attention(ops, case, lq, lk, pad_cols, forced)


@pytest.mark.parametrize("case", A.CASES["attention_f32"], ids=A.case_id)
def test_attention_f32_profiles(ops, case):
    """cir_attention with fp32 tensors (attn_f32_kernel, softmax_plain)."""
    _attention(ops, case, *case.shape)


@pytest.mark.parametrize("case", A.CASES["cls"], ids=A.case_id)
def test_cls_cross_attention_profiles(ops, case):
    """cir_cls_cross_attention: the dial is on x[:, :, 0] (values = keys), the 32 query rows carry the gains."""
    i = A.inputs(case)
    buf = torch.full((A.NP + 2, 32, case.d), NAN, dtype=case.dt, device="cuda")
    out = buf[1:A.NP + 1]
    ops.cls_cross_attention(i["k"].cuda(), i["q"].cuda(), A.SCALE, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()) and not bool(torch.isnan(out).any())
    _report(case, dict(out=out.cpu()))


TRAIN_BWD_LIMIT = {A.BF16: 2e-2, A.F16: 3e-3}      # test_train_ops_gpu.py::test_fused_training_attention_matches_torch_autograd's


def _train_forward(T, case):
    """-> (q4, k4, v4, mask, out4, out32, lse) on the GPU; out4 / out32 inside NaN frames that are checked."""
    lq, lk = case.shape
    i = A.inputs(case)
    g, h = A.NP, A.H
    q4, k4, v4 = (i[n].view(g, h, -1, 64).cuda() for n in ("q", "k", "v"))
    mask = None if i["mask"] is None else i["mask"].cuda()
    buf, out4 = _framed((g, h, lq, 64), case.dt)
    buf32, out32 = _framed((g, h, lq, 64), torch.float32)
    lse = T.attention_train_fwd(q4, k4, v4, mask, out4, A.SCALE, 0.0, 1, out32=out32)
    torch.cuda.synchronize()
    assert _gaps_untouched(buf, out4) and _gaps_untouched(buf32, out32), f"{case}: a canary was overwritten or an element was not written"
    return q4, k4, v4, mask, out4, out32, lse


@pytest.mark.parametrize("case", A.CASES["train"], ids=A.case_id)
def test_training_attention_profiles(T, case):
    """cir_attention_train_fwd at p_drop = 0: out, its fp32 twin and the log2-domain log-sum-exp within their bounds."""
    lq = case.shape[0]
    *_, out4, out32, lse = _train_forward(T, case)
    flat = lambda t: t.reshape(A.NP * A.H, lq, -1).cpu()                                       # noqa: E731
    _report(case, dict(out=flat(out4), out32=flat(out32), lse=lse.reshape(A.NP * A.H, lq).cpu()))


@pytest.mark.parametrize("case", A.CASES["train"], ids=A.case_id)
def test_training_attention_backward_profiles(T, case):
    """cir_attention_train_bwd at p_drop = 0 with the fp32 twin of O against float64 autograd of the same expression: relative norms of
    dQ, dK, dV within the limits of test_fused_training_attention_matches_torch_autograd (2e-2 bf16, 3e-3 fp16).

    This test found dQ outside its limit at 33 x 100 and 70 x 197 (bf16 up to 5.1e-2, fp16 up to 6.8e-3; dK and dV inside): the dialled
    key column carries an offset of up to 33, ~50 times its spread over the keys a peaked row attends, and sum_j dS_j k_j multiplies what
    16-bit P and dS lose of sum_j dS_j = 0 by that offset.  tattn_bwd_dq_kernel now takes that residue out around the row's own centre of
    the keys (train_attn.hip); measured since: dQ <= 2.5e-3 bf16, <= 4.4e-4 fp16 on every case."""
    lq = case.shape[0]
    i = A.inputs(case)
    g, h = A.NP, A.H
    q4, k4, v4, mask, out4, out32, lse = _train_forward(T, case)
    gen = torch.Generator(device="cpu").manual_seed(case.seed)
    dout_cpu = (torch.randn((g, h, lq, 64), generator=gen) * 0.5).to(case.dt)
    dbuf, dout = _framed((g, h, lq, 64), case.dt)
    dout.copy_(dout_cpu)
    dq, dk, dv = (torch.full(t.shape, NAN, dtype=torch.float32, device="cuda") for t in (q4, k4, v4))
    T.attention_train_bwd(q4, k4, v4, mask, out4, dout, lse, dq, dk, dv, A.SCALE, 0.0, 1, out32=out32)
    torch.cuda.synchronize()
    qd, kd, vd = (i[n].double().view(g, h, -1, 64).requires_grad_(True) for n in ("q", "k", "v"))
    s = qd @ kd.transpose(-1, -2) * A.SCALE
    if i["mask"] is not None:
        s = s + i["mask"].double().clamp_min(-1e30)[:, None, None, :]
    (torch.softmax(s, -1) @ vd).backward(dout_cpu.double())
    rel = lambda a, b: float((a.cpu().double() - b).norm() / (b.norm() + 1e-300))              # noqa: E731
    e_q, e_k, e_v = rel(dq, qd.grad), rel(dk, kd.grad), rel(dv, vd.grad)
    print(f"\n[{case}] backward, relative norms: dq {e_q:.2e}  dk {e_k:.2e}  dv {e_v:.2e}  (limit {TRAIN_BWD_LIMIT[case.dt]:.0e})")
    assert max(e_q, e_k, e_v) < TRAIN_BWD_LIMIT[case.dt]                                       # NaN fails
