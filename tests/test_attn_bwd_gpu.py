"""cir_attention_train_fwd / cir_attention_train_bwd on the MI355X against float64, ELEMENT BY ELEMENT within the a-priori bounds of
tests/attn_bwd_cases.py: the dialled score profiles (peaked rows, a common key offset), six shapes from one element to ragged multi-tile,
-10000 and finfo.min masks, dropout 0 / 0.1 / 0.25 regenerated on the host, the three forms of the backward call (fp32 twin of O or not,
16-bit or fp32 gradients), launches whose last workgroup has idle waves, fp16 with dO at the loss scale.
One forward and one backward launch per case; every element of out, out32, lse, dQ, dK and dV is compared.  The operands are the q / k / v
slices of fused projection rows (rows, 3, H 64) and (rows, 2, H 64), the gradients go into the slices of such buffers as the trainers pass
them; every output is pre-filled with NaN and sits between NaN canary rows, and what the kernels must not touch is NaN afterwards.
tests/test_attn_bwd_cases_cpu.py shows what the comparison lets through and what it catches.

Measured on the MI355X, largest error / bound over all 144 cases (`pytest -s` prints them per case and in a final table):
                 out     out32   lse     dQ      dK      dV
    bf16 p = 0   0.744   0.682   0.274   0.258   0.249   0.796
    bf16 p > 0   0.923   0.874   0.274   0.312   0.302   0.788
    fp16 p = 0   0.780   0.830   0.268   0.300   0.241   0.622
    fp16 p > 0   0.913   0.941   0.268   0.911   0.228   0.823
every figure within 0.01 of what the CPU stand-in `kernel` gives on the same case, i.e. the kernels compute what was read from them.
What this file found, both fixed in train_attn.hip:
  * fp16, p = 0: dQ[:, 1] (every key is 1 there, the exact value is 0) up to 2.58 times its bound on four cases, 0.7 - 0.9 on others where
    the stand-in gives 0.2: ONE element of the row's dS16 differed by an fp16 ulp between the matrix operand and the row sum that feeds the
    centre correction (the compiler rounded the two copies differently: `opaque128`).  Since: 0.300.
  * finfo.min on every key (min_all): dQ was NaN - the lse of such a row is the clamp itself and cannot rebuild P (`kSatLse`).  Since:
    dQ 0.16, dK 0.16, dV 0.39."""
import pytest
import torch

from tests import attn_bwd_cases as B

pytestmark = pytest.mark.gpu
NAN = float("nan")
MEASURED = {}                                       # (dtype, "p=0" | "p>0") -> {output: largest error / bound}, filled as the cases run


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    yield train_ops
    print("\nfused training attention, largest error / bound over the cases run:")
    for (dt, p), w in sorted(MEASURED.items()):
        print(f"  {dt:4s} {p}: " + "  ".join(f"{n} {w[n]:.3f}" for n in B.OUTPUTS))


def _framed(rows, cols, dtype):
    """A NaN buffer (rows + 2, *cols) with one canary row above and below the (rows, *cols) view that is returned with it."""
    buf = torch.full((rows + 2, *cols), NAN, dtype=dtype, device="cuda")
    return buf, buf[1:rows + 1]


def _heads(x, g, h, part):
    """The (G, H, rows, 64) head view of slice `part` of fused rows (G rows, parts, H 64) - or of plain rows (G rows, H 64), part None."""
    x = x.view(g, x.shape[0] // g, -1, h, 64)
    return (x[:, :, 0] if part is None else x[:, :, part]).permute(0, 2, 1, 3)


def _items(t4):
    """(G, H, L, 64) -> the items layout (G H, L, 64) on the CPU."""
    return t4.reshape(t4.shape[0] * t4.shape[1], t4.shape[2], 64).cpu()


def _run(T, case):
    lq, lk = case.shape
    g, h, _ = B.layout(case)
    twin, g16 = B.FORMS[case.form]
    gdt = case.dt if g16 else torch.float32
    i = B.inputs(case)
    hd = h * 64
    # operands: slices of fused projection rows whose other slices are NaN
    qkv = torch.full((g * lq, 3, hd), NAN, dtype=case.dt, device="cuda")
    kvx = torch.full((g * lk, 2, hd), NAN, dtype=case.dt, device="cuda")
    q4, k4, v4 = _heads(qkv, g, h, 0), _heads(kvx, g, h, 0), _heads(kvx, g, h, 1)
    for dst, name in ((q4, "q"), (k4, "k"), (v4, "v")):
        dst.copy_(i[name].view(g, h, -1, 64))
    mask = None if i["mask_g"] is None else i["mask_g"].cuda()
    (obuf, ctx), (o32buf, ctx32), (dobuf, dctx) = (_framed(g * lq, (hd,), dt) for dt in (case.dt, torch.float32, case.dt))
    out4, out32, dout4 = _heads(ctx, g, h, None), _heads(ctx32, g, h, None), _heads(dctx, g, h, None)
    dout4.copy_(i["do"].view(g, h, lq, 64))
    seed = B.seed_of(case)
    lse = T.attention_train_fwd(q4, k4, v4, mask, out4, B.SCALE, case.p, seed, out32=out32)
    (dqbuf, dqkv), (dkbuf, dkv) = _framed(g * lq, (3, hd), gdt), _framed(g * lk, (2, hd), gdt)
    dq4, dk4, dv4 = _heads(dqkv, g, h, 0), _heads(dkv, g, h, 0), _heads(dkv, g, h, 1)
    T.attention_train_bwd(q4, k4, v4, mask, out4, dout4, lse, dq4, dk4, dv4, B.SCALE, case.p, seed, out32=out32 if twin else None)
    torch.cuda.synchronize()
    for name, buf in (("out", obuf), ("out32", o32buf), ("dout", dobuf), ("dq", dqbuf), ("dkv", dkbuf)):
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), f"{case}: a canary row of {name} was overwritten"
    assert bool(torch.isnan(dqkv[:, 1:]).all()), f"{case}: the k / v slices beside dQ were written"
    assert bool(torch.isnan(qkv[:, 1:]).all()) and torch.equal(dout4.cpu(), i["do"].view(g, h, lq, 64)), f"{case}: an input was overwritten"
    return dict(out=_items(out4), out32=_items(out32), lse=lse.reshape(g * h, lq).cpu(), dq=_items(dq4), dk=_items(dk4), dv=_items(dv4))


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_training_attention_elementwise(T, case):
    outputs = _run(T, case)
    worst = B.worst_ratio(case, outputs)
    print(f"\n[{case}] largest error / bound: " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    seen = MEASURED.setdefault((B.DT_NAME[case.dt], "p>0" if case.p > 0 else "p=0"), dict.fromkeys(B.OUTPUTS, 0.0))
    for n, w in worst.items():
        seen[n] = max(seen[n], w)
    if getattr(case, "do", None) == "loss":
        assert all(bool(torch.isfinite(o).all()) for o in outputs.values()), f"{case}: a non-finite value at the loss scale"
    fails = B.check(case, outputs)                                  # (an element that was not written is NaN: outside every bound)
    assert not fails, fails
