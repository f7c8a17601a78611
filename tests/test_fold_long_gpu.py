"""cir_cross_attention_folded_long: the query-side fold for captions of up to 64 tokens against up to 224 keys (csrc/xattn_fold_units.hip) -
against the fp64 restatement of the reference's arithmetic and the projected path of this library on the inputs of tests/test_fold_gpu.py
(q and x at sigma 1, weights at sigma 0.03, biases at sigma 0.5), with the bounds that file holds for the 32-token kernels: a row's error
does not depend on how many rows share its launch.  Then the properties a longer caption adds: the token-to-block and head-to-wave maps of
blocks 3 and 4, stores confined to rows < L, and one accumulation order per row whatever the block assignment (bit-identical rows across
L = 33 / 48 / 49 / 64, across T and across the candidate's place in the batch)."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
D, H = 768, 12
F16, BF16 = torch.float16, torch.bfloat16
CANARY = {BF16: 0x7FC1, F16: 0x7E01}        # NaN patterns


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import ops as _ops
    return _ops


def _rand(shape, scale, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _reference(q, x, wk, bk, wv, bv, l, mask=None):
    """fp64, as the reference writes it: per branch b and candidate t, heads of 64 (optionally with an additive key mask (T, N))."""
    t_n, n, _ = x.shape
    out = torch.empty((t_n, l, 2, D), dtype=torch.float64)
    for b in (0, 1):
        k = (x.double() @ wk[b].double().T + bk[b].double()).view(t_n, n, H, 64).permute(0, 2, 1, 3)
        v = (x.double() @ wv[b].double().T + bv[b].double()).view(t_n, n, H, 64).permute(0, 2, 1, 3)
        qq = q[b].double().view(t_n, l, H, 64).permute(0, 2, 1, 3)
        s = qq @ k.transpose(-1, -2) / 8.0
        if mask is not None:
            s = s + mask.double().clamp(min=-1e30)[:, None, None, :]
        out[:, :, b] = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(t_n, l, D)
    return out


def _long(ops, q, x, wk, wv, bv, l, mask=None, out=None):
    out = torch.empty((x.shape[0], l, 2, D), dtype=x.dtype, device="cuda") if out is None else out
    ops.cross_attention_folded_long(q.cuda(), x.cuda(), ops.fold_pack_key(wk).cuda(), ops.fold_pack_value(wv).cuda(), bv.cuda(), out, l, 0.125,
                                    mask=None if mask is None else mask.cuda())
    return out


SHAPES = [(3, 40, 197), (2, 33, 197), (2, 48, 224), (5, 49, 50), (1, 64, 197), (9, 47, 17), (2, 16, 197), (2, 1, 33)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("t_n,l,n", SHAPES)
def test_long_fold_against_fp64_and_projected_path(ops, dtype, t_n, l, n):
    q = _rand((2, t_n * l, D), 1.0, 1, dtype)
    x = _rand((t_n, n, D), 1.0, 2, dtype)
    wk, wv = _rand((2, D, D), 0.03, 3, dtype), _rand((2, D, D), 0.03, 4, dtype)
    bk, bv = _rand((2, D), 0.5, 5, torch.float32), _rand((2, D), 0.5, 6, torch.float32)
    ref = _reference(q, x, wk, bk, wv, bv, l)
    out = _long(ops, q, x, wk, wv, bv, l)
    torch.cuda.synchronize()
    err = (out.cpu().double() - ref).abs().max().item()
    # the projected path on the same inputs: [K0 V0 K1 V1] GEMM + attention
    wkv = torch.cat([wk[0], wv[0], wk[1], wv[1]]).cuda()
    bkv = torch.cat([bk[0], bv[0], bk[1], bv[1]]).cuda()
    kv = ops.gemm(x.cuda().view(t_n * n, D), wkv, bkv).view(t_n, n, 4, D)
    o2 = torch.empty((t_n, l, 2, D), dtype=dtype, device="cuda")
    qc = q.cuda().view(2, t_n, l, D).permute(1, 0, 2, 3)
    ops.attention(qc, kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3), o2.permute(0, 2, 1, 3), 0.125)
    err2 = (o2.cpu().double() - ref).abs().max().item()
    print(f"\n[long fold {dtype} T {t_n} L {l} N {n}] max|err| vs fp64: folded {err:.2e}, projected {err2:.2e} (|ctx| max {ref.abs().max():.2f})")
    tol = 4e-2 if dtype == BF16 else 6e-3
    assert err < tol and err < 2.5 * err2 + 1e-3


def test_long_fold_exact_small_integers(ops):
    """Attention over identical keys is the mean of the values whatever the scores: with integer X (all rows equal) and integer W_v the folded
    chain (P X, then W_v) is exact in fp16 - a k-slot / permutation slip in G3 / G4 of any of the three blocks shows up as a wrong integer."""
    t_n, l, n = 2, 40, 197
    g = torch.Generator().manual_seed(3)
    row = torch.randint(-2, 3, (t_n, 1, D), generator=g).float()
    x = row.expand(t_n, n, D).contiguous().half()
    q = _rand((2, t_n * l, D), 1.0, 1, F16)
    wk = _rand((2, D, D), 0.03, 2, F16)
    wv = torch.randint(-1, 2, (2, D, D), generator=g).half()
    bv = torch.randint(-3, 4, (2, D), generator=g).float()
    out = _long(ops, q, x, wk, wv, bv, l)
    want = torch.stack([row[:, 0].double() @ wv[b].double().T + bv[b].double() for b in (0, 1)], dim=1)      # (T, 2, D)
    err = (out.cpu().double() - want[:, None].expand(t_n, l, 2, D)).abs().max().item()
    print(f"\n[long fold, constant keys] max|err| {err:.2e} (values up to {want.abs().max():.0f})")
    assert err < 0.13          # sums of ~50 terms up to ~100: one fp16 ulp there is 0.06 (P X is exact, the row sum of P rounds)


def test_long_fold_scores_follow_the_keys(ops):
    """One-hot attention at L = 64: every (branch, token, head) is steered to a key of its own, so a wrong token-to-block or head-to-wave map
    in blocks 3 and 4 (two waves per head) returns another key's value."""
    t_n, l, n = 1, 64, 197
    x = _rand((t_n, n, D), 1.0, 7, F16)
    wk = _rand((2, D, D), 0.05, 8, F16)
    wv = _rand((2, D, D), 0.03, 9, F16)
    bv = _rand((2, D), 0.5, 10, torch.float32)
    k_all = [(x[0].double() @ wk[b].double().T).view(n, H, 64) for b in (0, 1)]
    q = torch.zeros((2, t_n * l, D), dtype=F16)
    for b in (0, 1):
        for tok in range(l):
            for h in range(H):
                kv = k_all[b][(37 * tok + 11 * h + 5 * b) % n, h]
                q[b, tok, h * 64:(h + 1) * 64] = (kv * (300.0 / (kv @ kv))).half()          # q . k_j = 300 -> score 37.5 after the 1/8
    ref = _reference(q, x, wk, torch.zeros((2, D)), wv, bv, l)
    out = _long(ops, q, x, wk, wv, bv, l)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"\n[long fold, steered heads] max|err| vs fp64 {err:.2e}")
    assert err < 2e-2


@pytest.mark.parametrize("t_n,l,n", [(3, 40, 197), (2, 64, 224)])
def test_long_fold_with_a_key_mask(ops, t_n, l, n):
    """The additive key mask of padded candidate token sets: fp64 with the same mask, an all-zero mask next to the unmasked launch, a fully
    masked candidate finite, and a mask whose rows are further apart than N."""
    q = _rand((2, t_n * l, D), 1.0, 11, F16)
    x = _rand((t_n, n, D), 1.0, 12, F16)
    wk, wv = _rand((2, D, D), 0.03, 13, F16), _rand((2, D, D), 0.03, 14, F16)
    bk, bv = _rand((2, D), 0.5, 15, torch.float32), _rand((2, D), 0.5, 16, torch.float32)
    keep = torch.rand((t_n, n), generator=torch.Generator().manual_seed(17)) > 0.3
    keep[:, 0] = True
    keep[0, n // 2:] = False                                             # a candidate padded to half its tokens
    mask = ((1.0 - keep.float()) * torch.finfo(torch.float32).min)
    ref = _reference(q, x, wk, bk, wv, bv, l, mask=mask)
    out = _long(ops, q, x, wk, wv, bv, l, mask=mask)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"\n[long fold, key mask, T {t_n} L {l} N {n}] max|err| vs fp64 {err:.2e}")
    assert err < 6e-3
    plain = _long(ops, q, x, wk, wv, bv, l)
    zero = _long(ops, q, x, wk, wv, bv, l, mask=torch.zeros((t_n, n)))
    assert (plain.float() - zero.float()).abs().max().item() < 2e-3      # (the masked form scales the scores before the maximum: one rounding apart)
    allm = _long(ops, q, x, wk, wv, bv, l, mask=torch.full((t_n, n), torch.finfo(torch.float32).min))
    assert bool(torch.isfinite(allm.float()).all())
    wide = torch.full((t_n, n + 27), float("nan"), device="cuda")        # rows n + 27 apart; what lies between the rows must not be read
    wide[:, :n] = mask.cuda()
    strided = _long(ops, q, x, wk, wv, bv, l, mask=wide[:, :n])
    assert torch.equal(strided, out)


class Guarded:
    """A (rows, cols) output view inside a canary-filled (rows + 2 pr, cols + 2 pc) allocation (as tests/test_guard_gpu.py)."""

    def __init__(self, rows, cols, dtype, pr=40, pc=64):
        self.dtype, self.pr, self.pc, self.rows, self.cols = dtype, pr, pc, rows, cols
        self.big = torch.empty((rows + 2 * pr, cols + 2 * pc), dtype=dtype, device="cuda")
        self.big.view(torch.int16).fill_(CANARY[dtype])
        self.view = self.big[pr:pr + rows, pc:pc + cols]

    def assert_intact(self, what=""):
        bits = self.big.view(torch.int16).clone()
        bits[self.pr:self.pr + self.rows, self.pc:self.pc + self.cols].fill_(CANARY[self.dtype])
        bad = bits != CANARY[self.dtype]
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} canary elements overwritten, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("t_n,l,n", [(3, 40, 197), (5, 33, 50), (2, 64, 224), (9, 47, 17)])
def test_long_fold_guard_bands(ops, dtype, t_n, l, n):
    """The kernel writes token rows < L of a (T, L, 2, 768) tensor from 16-row blocks (rows beyond L are computed on zero queries and must not be
    stored), reads X rows clamped to N - 1 and weight fragments through buffer descriptors: output inside canaries, and the tokens / weights sit
    at the END of their allocations (a read past them would meet the next allocation's canary NaNs and poison the result)."""
    g = torch.Generator(device="cpu").manual_seed(t_n * 31 + l)

    def at_end(shape, s):                                                 # the tensor is the tail of a NaN-filled allocation
        v = (torch.randn(shape, generator=g) * s).to(dtype)
        big = torch.full((v.numel() + 4096,), float("nan"), dtype=dtype, device="cuda")
        big[4096:] = v.flatten().cuda()
        return big[4096:].view(shape)

    q, x = at_end((2, t_n * l, D), 1.0), at_end((t_n, n, D), 1.0)
    wk, wv = (torch.randn((2, D, D), generator=g) * 0.03).to(dtype), (torch.randn((2, D, D), generator=g) * 0.03).to(dtype)
    wkt, wvp = at_end((2, D, D), 0.0), at_end((2, D, D), 0.0)
    wkt.copy_(ops.fold_pack_key(wk).cuda()); wvp.copy_(ops.fold_pack_value(wv).cuda())
    bv = torch.randn((2, D), generator=g).cuda()
    guard = Guarded(t_n * l, 2 * D, dtype)
    out = guard.view.unflatten(0, (t_n, l)).unflatten(2, (2, D))
    ops.cross_attention_folded_long(q, x, wkt, wvp, bv, out, l, 0.125)
    torch.cuda.synchronize()
    guard.assert_intact(f"long fold T {t_n} L {l} N {n}")
    assert torch.isfinite(out.float()).all()
    # against the projected path of the library on the same inputs
    wkv = torch.cat([wk[0], wv[0], wk[1], wv[1]]).cuda()
    bkv = torch.cat([torch.zeros(D, device="cuda"), bv[0], torch.zeros(D, device="cuda"), bv[1]])
    kv = ops.gemm(x.view(t_n * n, D), wkv, bkv).view(t_n, n, 4, D)
    o2 = torch.empty((t_n, l, 2, D), dtype=dtype, device="cuda")
    ops.attention(q.view(2, t_n, l, D).permute(1, 0, 2, 3), kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3), o2.permute(0, 2, 1, 3), 0.125)
    assert (out.float() - o2.float()).abs().max().item() < (6.5e-2 if dtype == BF16 else 4e-3)     # (two roundings: up to two bf16 ulps of 2^-5 at |ctx| ~ 4)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_long_fold_rows_do_not_depend_on_their_launch(ops, dtype):
    """"Tile choice never changes a bit": (a) a candidate's rows are the same in a batch of 7 and alone, (b) the first 33 token rows are the same
    whether the caption has 33, 48, 49 or 64 tokens (three blocks in one wave, or two waves of two blocks), (c) a launch repeats itself."""
    n, t7 = 197, 7
    wk, wv, bv = _rand((2, D, D), 0.03, 23, dtype), _rand((2, D, D), 0.03, 24, dtype), _rand((2, D), 0.5, 26, torch.float32)
    x = _rand((t7, n, D), 1.0, 22, dtype)
    q64 = _rand((2, t7, 64, D), 1.0, 21, dtype)                           # (branch, candidate, token, D)
    pack = lambda cands, l: q64[:, cands, :l].reshape(2, len(cands) * l, D).contiguous()
    # (a), (c)
    l = 40
    every = list(range(t7))
    batch = _long(ops, pack(every, l), x, wk, wv, bv, l)
    assert torch.equal(batch, _long(ops, pack(every, l), x, wk, wv, bv, l))
    alone = _long(ops, pack([3], l), x[3:4], wk, wv, bv, l)
    assert torch.equal(batch[3], alone[0])
    # (b): the same q rows repacked into each launch's (2, T L, D) layout
    outs = {l: _long(ops, pack([0, 1], l), x[:2], wk, wv, bv, l) for l in (33, 48, 49, 64)}
    for l in (48, 49, 64):
        assert torch.equal(outs[l][:, :33], outs[33]), l
    assert torch.equal(outs[64][:, :48], outs[48]) and torch.equal(outs[64][:, :49], outs[49])


# ------------------------------------------------------------------------------------------------ engine and model
@pytest.fixture(scope="module")
def tiny(ops):
    """The tiny BLIP_NLVR of the existing engine test: 3 fusion layers, 64-px ViT (17 tokens), fp16, 2 queries x 6 candidates."""
    from candidate_reranking_cir_amd import synthetic
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    dev = torch.device("cuda")
    vit = VitGeometry(image_size=64, patch_size=16, width=768, depth=1, num_heads=12)
    torch.manual_seed(0)
    m = BLIP_NLVR(BertGeometry(num_hidden_layers=3), vit_geometry=vit, tokenizer=synthetic.HashTokenizer()).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(5)
    q_n, k, n = 2, 6, vit.num_tokens

    def inputs(l):
        z = torch.randn((q_n, l, 768), generator=g).to(dev)
        ids = torch.randint(1000, 20000, (q_n, l), generator=g).to(dev)
        return ids, torch.ones_like(ids), z

    cand = (torch.randn((q_n * k, n, 768), generator=g) * 0.5).to(dev).half()
    qidx = torch.arange(q_n, device=dev).repeat_interleave(k)
    cmask = torch.ones((q_n * k, n), dtype=torch.int64, device=dev)
    cmask[::2, n - 4:] = 0
    return dict(m=m, vit=vit, cand=cand, qidx=qidx, cmask=cmask, i40=inputs(40), i65=inputs(65))


def test_engine_takes_the_long_fold_for_40_tokens(tiny):
    """`fold_long` on: 40-token captions take the long fold on the fusion layers below the last - no fallback counted, no warning - and the
    logits agree with the projected path within 3e-3, the bound tests/test_fold_gpu.py holds between the two paths at this geometry; with a
    candidate mask the same (measured: 4.5e-4 and 4.2e-4).  65 tokens keep the projected path and the counter."""
    m = tiny["m"]
    eng = m.engines()[1]
    cand, qidx = tiny["cand"], tiny["qidx"]
    eng.fold_long, eng.fold_fallbacks = True, 0
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            folded = eng.forward(*tiny["i40"], cand, qidx)
            folded_m = eng.forward(*tiny["i40"], cand, qidx, cand_mask=tiny["cmask"])
        assert eng.fold_fallbacks == 0 and not [x for x in w if "projected" in str(x.message)]
        eng.fold_cross_kv = False
        projected = eng.forward(*tiny["i40"], cand, qidx)
        projected_m = eng.forward(*tiny["i40"], cand, qidx, cand_mask=tiny["cmask"])
        eng.fold_cross_kv = True
        d, dm = (folded - projected).abs().max().item(), (folded_m - projected_m).abs().max().item()
        print(f"\n[engine, 40 tokens] long fold vs projected: {d:.2e}, with a candidate mask {dm:.2e}; the mask moves the logits by {(folded - folded_m).abs().max().item():.2e}")
        assert d < 3e-3 and dm < 3e-3 and (folded - folded_m).abs().max().item() > 1e-4
        eng.fold_long = False                                  # the switch decides: off, the same call is the projected path, counted
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            off = eng.forward(*tiny["i40"], cand, qidx)
            eng.fold_long = True
            long65 = eng.forward(*tiny["i65"], cand, qidx)
        assert eng.fold_fallbacks == 2 and torch.equal(off, projected) and sum("projected" in str(x.message) for x in w) == 1
        eng.fold_cross_kv = False
        assert eng.fold_fallbacks == 2 and torch.equal(long65, eng.forward(*tiny["i65"], cand, qidx))
    finally:
        eng.fold_cross_kv, eng.fold_long = True, False


def test_model_switch_reaches_the_engine_and_survives_repacks(tiny):
    from candidate_reranking_cir_amd import synthetic
    m = tiny["m"]
    try:
        assert m.engines()[1].fold_long is False
        assert m.set_long_caption_fold(True) is m and m.engines()[1].fold_long is True
        m.set_precision("text32")
        assert m.engines()[1].fold_long is True
        m.set_precision("f16")
        m.load_state_dict(m.state_dict())
        eng = m.engines()[1]
        assert eng.fold_long is True
        # one query of 40 tokens (38 words + [CLS] / [SEP]) against 6 candidates through the model's own call
        cap = [synthetic.caption_text(7, 38)]
        cand = tiny["cand"][:6]
        z = torch.randn((1, 40, 768), generator=torch.Generator().manual_seed(9)).cuda()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            direct = m.img_txt_fusion_val(z, cand, cap)
        assert m.engines()[1].fold_fallbacks == 0 and not [x for x in w if "projected" in str(x.message)]
        m.enable_graphs(64)
        first, again = m.img_txt_fusion_val(z, cand, cap), m.img_txt_fusion_val(z, cand, cap)
        assert torch.equal(first, direct) and torch.equal(again, direct) and len(m.engines()[1]._graphs) == 1
        m.set_long_caption_fold(False)                         # the switch is part of the plan key: a new capture, the projected path
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            off = m.img_txt_fusion_val(z, cand, cap)
        assert torch.allclose(off, direct, atol=3e-3) and len(m.engines()[1]._graphs) == 2
        assert m.engines()[1].fold_fallbacks > 0
    finally:
        m.enable_graphs(0)
        m.set_long_caption_fold(False)
