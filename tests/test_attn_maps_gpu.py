"""cir_attention_maps / cir_attention_gradcam on the MI355X against float64, ELEMENT BY ELEMENT within the a-priori bounds of
tests/attn_map_cases.py: every case of its table through both entry points (one forward launch for the lse, one launch each), operands
as the q / k / v slices of fused projection rows whose other slices are NaN, outputs with a row pitch of Lk rounded up to 4 (and once
more with a wider pitch) between NaN canary bands, pad columns zero, cam bit-identical over two launches, and the probabilities-only call
bit-identical to the full call's probs.  tests/test_attn_map_cases_cpu.py shows what the comparison lets through and what it catches."""
import pytest
import torch

from tests import attn_bwd_cases as B
from tests import attn_map_cases as M

pytestmark = pytest.mark.gpu
NAN = float("nan")
BAND = 64                                           # canary elements before and after every output
MEASURED = {}                                       # dtype -> {output: largest error / bound}


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    yield train_ops
    print("\nattention maps, largest error / bound over the cases run:")
    for dt, w in sorted(MEASURED.items()):
        print(f"  {dt:4s}: " + "  ".join(f"{n} {x:.3f}" for n, x in w.items()))


def _heads(x, g, h, part):
    """The (G, H, rows, 64) head view of slice `part` of fused rows (G rows, parts, H 64) - or of plain rows (G rows, H 64), part None."""
    x = x.view(g, x.shape[0] // g, -1, h, 64)
    return (x[:, :, 0] if part is None else x[:, :, part]).permute(0, 2, 1, 3)


def _banded(shape):
    """A NaN fp32 buffer with BAND canary elements on either side of the contiguous `shape` view returned with it."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * BAND,), NAN, dtype=torch.float32, device="cuda")
    return buf, buf[BAND:BAND + n].view(shape)


def _intact(buf):
    return bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all())


def _operands(T, case):
    lq, lk = case.shape
    g, h, _ = B.layout(case)
    i = B.inputs(case)
    hd = h * 64
    qkv = torch.full((g * lq, 3, hd), NAN, dtype=case.dt, device="cuda")
    kvx = torch.full((g * lk, 2, hd), NAN, dtype=case.dt, device="cuda")
    q4, k4, v4 = _heads(qkv, g, h, 0), _heads(kvx, g, h, 0), _heads(kvx, g, h, 1)
    for dst, name in ((q4, "q"), (k4, "k"), (v4, "v")):
        dst.copy_(i[name].view(g, h, -1, 64))
    mask = None if i["mask_g"] is None else i["mask_g"].cuda()
    ctx = torch.empty((g * lq, hd), dtype=case.dt, device="cuda")
    dctx = torch.empty_like(ctx)
    out4, dout4 = _heads(ctx, g, h, None), _heads(dctx, g, h, None)
    dout4.copy_(i["do"].view(g, h, lq, 64))
    lse = T.attention_train_fwd(q4, k4, v4, mask, out4, B.SCALE, 0.0, 0)
    return q4, k4, v4, mask, dout4, lse


def _launch(T, case, ops, ldk):
    """Both entry points through the C ABI into banded buffers of row pitch `ldk` -> (probs, dprobs, cam, probs of the probabilities-only
    call, cam of a second launch), each the full (.., ldk) tensor, after the canaries were checked."""
    from candidate_reranking_cir_amd import lib
    from candidate_reranking_cir_amd.ops import _DT, _ptr, _stream
    q4, k4, v4, mask, dout4, lse = ops
    g, h, lq, _ = q4.shape
    lk = k4.shape[2]
    c = lib.load()
    hv = T._hv
    (pb, probs), (gb, dprobs), (ob, only), (cb, cam), (c2b, cam2) = (_banded(s) for s in ((g, h, lq, ldk),) * 3 + ((g, lq, ldk),) * 2)
    tail = (g, h, lq, lk, 64, B.SCALE, M.dmul(case), _DT[q4.dtype], _stream())
    lib.check(c.cir_attention_maps(*hv(q4), *hv(k4), *hv(v4), _ptr(mask), *hv(dout4), lse.data_ptr(), probs.data_ptr(), dprobs.data_ptr(), ldk, *tail),
              "cir_attention_maps")
    lib.check(c.cir_attention_maps(*hv(q4), *hv(k4), None, 0, 0, 0, _ptr(mask), None, 0, 0, 0, lse.data_ptr(), only.data_ptr(), None, ldk, *tail),
              "cir_attention_maps")
    for dst in (cam, cam2):
        lib.check(c.cir_attention_gradcam(*hv(q4), *hv(k4), *hv(v4), _ptr(mask), *hv(dout4), lse.data_ptr(), dst.data_ptr(), ldk, *tail),
                  "cir_attention_gradcam")
    torch.cuda.synchronize()
    for name, buf in (("probs", pb), ("dprobs", gb), ("probs-only", ob), ("cam", cb), ("cam (second launch)", c2b)):
        assert _intact(buf), f"{case}: a canary band of {name} was overwritten"
    return probs, dprobs, cam, only, cam2


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_attention_maps_elementwise(T, case):
    lq, lk = case.shape
    g, h, _ = B.layout(case)
    ops = _operands(T, case)
    ldk = (lk + 3) // 4 * 4
    probs, dprobs, cam, only, cam2 = _launch(T, case, ops, ldk)
    for name, t in (("probs", probs), ("dprobs", dprobs), ("cam", cam)):
        assert not bool(torch.isnan(t).any()), f"{case}: an element of {name} was not written"
        assert bool((t[..., lk:] == 0).all()), f"{case}: a pad column of {name} is not 0"
    assert torch.equal(cam, cam2), f"{case}: cam differs between two launches"
    assert torch.equal(only, probs), f"{case}: the probabilities-only call differs from the full call's probs"
    outputs = dict(probs=probs[..., :lk].reshape(g * h, lq, lk).cpu(), dprobs=dprobs[..., :lk].reshape(g * h, lq, lk).cpu(), cam=cam[..., :lk].cpu())
    worst = M.worst_ratio(case, outputs)
    print(f"\n[{case}] largest error / bound: " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    seen = MEASURED.setdefault(B.DT_NAME[case.dt], dict.fromkeys(worst, 0.0))
    for n, w in worst.items():
        seen[n] = max(seen[n], w)
    assert all(bool(torch.isfinite(o).all()) for o in outputs.values())
    fails = M.check(case, outputs)
    assert not fails, fails
    # the operators: same launches behind train_ops, sliced to Lk
    p2, g2 = T.attention_maps(*ops, dmul=M.dmul(case), scale=B.SCALE)
    c2 = T.attention_gradcam(*ops, dmul=M.dmul(case), scale=B.SCALE)
    p3, none = T.attention_maps(*ops, dmul=M.dmul(case), grads=False, scale=B.SCALE)
    assert none is None and p2.shape == (g, h, lq, lk) and c2.shape == (g, lq, lk)
    assert torch.equal(p2, probs[..., :lk]) and torch.equal(g2, dprobs[..., :lk]) and torch.equal(c2, cam[..., :lk]) and torch.equal(p3, p2)


@pytest.mark.parametrize("which", [((9, 9), B.BF16, "none"), ((33, 100), B.F16, "tail")], ids=["9x9-bf16", "33x100-fp16-tail"])
def test_wide_row_pitch(T, which):
    """ldk beyond the last key tile (9 keys in rows of 72, 100 in rows of 136): the tail past 32 nkt is zeroed too, the values are the same
    bits, and nothing lands outside the buffers."""
    case = M.named(*which)
    lk = case.shape[1]
    ops = _operands(T, case)
    narrow = _launch(T, case, ops, (lk + 3) // 4 * 4)
    wide = _launch(T, case, ops, (lk + 31) // 32 * 32 + 40)
    for a, b in zip(narrow[:3], wide[:3]):
        assert torch.equal(a[..., :lk], b[..., :lk]) and bool((b[..., lk:] == 0).all())
