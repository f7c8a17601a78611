"""cir_cross_attention_folded_short: the query-side fold for captions of at most 16 tokens against up to 608 keys, one wave and one 16-row
block per head (csrc/xattn_fold_units.hip: the 14-key-block form at <= 224 keys, `xattn_fold16_short_kernel` - 4 waves, 10 phase-1 and 15
phase-2 DMA pieces per wave - above) - on the inputs of tests/test_fold_long_gpu.py (q and x at sigma 1, weights at sigma 0.03, biases at
sigma 0.5) with the bounds that file and tests/test_fold_gpu.py hold for the folded kernels.  Where the code promises the neighbours' bits
(one body, one accumulation order per row) the comparison is `torch.equal`, never a tolerance."""
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


def _fold(fn, ops, q, x, wk, wv, bv, l, mask=None, out=None):
    out = torch.empty((x.shape[0], l, 2, D), dtype=x.dtype, device="cuda") if out is None else out
    fn(q.cuda(), x.cuda(), ops.fold_pack_key(wk).cuda(), ops.fold_pack_value(wv).cuda(), bv.cuda(), out, l, 0.125,
       mask=None if mask is None else mask.cuda())
    return out


def _short(ops, *a, **k):
    return _fold(ops.cross_attention_folded_short, ops, *a, **k)


# <= 224 keys: the 14-block form; 225 .. 608: the new instantiation (225 = its first key count, 577 = the 384-px geometry, 608 = every key live)
SHAPES = [(3, 16, 197), (2, 1, 1), (5, 9, 50), (9, 13, 17), (2, 16, 224), (2, 16, 225), (3, 12, 577), (2, 16, 608), (1, 7, 300)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("t_n,l,n", SHAPES)
def test_short_fold_against_fp64_and_projected_path(ops, dtype, t_n, l, n):
    q = _rand((2, t_n * l, D), 1.0, 1, dtype)
    x = _rand((t_n, n, D), 1.0, 2, dtype)
    wk, wv = _rand((2, D, D), 0.03, 3, dtype), _rand((2, D, D), 0.03, 4, dtype)
    bk, bv = _rand((2, D), 0.5, 5, torch.float32), _rand((2, D), 0.5, 6, torch.float32)
    ref = _reference(q, x, wk, bk, wv, bv, l)
    out = _short(ops, q, x, wk, wv, bv, l)
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
    print(f"\n[short fold {dtype} T {t_n} L {l} N {n}] max|err| vs fp64: folded {err:.2e}, projected {err2:.2e} (|ctx| max {ref.abs().max():.2f})")
    tol = 4e-2 if dtype == BF16 else 6e-3
    assert err < tol and err < 2.5 * err2 + 1e-3


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_short_fold_has_the_bits_of_its_neighbours(ops, dtype):
    """A row is one column of every product and every unit instantiation runs units and key blocks in one order: at 225 .. 608 keys the rows
    are cir_cross_attention_folded's (same body, two waves per head), at <= 224 keys cir_cross_attention_folded_long's (the same launch) -
    unmasked and under a key mask."""
    wk, wv, bv = _rand((2, D, D), 0.03, 43, dtype), _rand((2, D, D), 0.03, 44, dtype), _rand((2, D), 0.5, 46, torch.float32)
    for n, other in [(225, ops.cross_attention_folded), (577, ops.cross_attention_folded), (608, ops.cross_attention_folded),
                     (17, ops.cross_attention_folded_long), (197, ops.cross_attention_folded_long), (224, ops.cross_attention_folded_long)]:
        for t_n, l in ((2, 16), (3, 11)):
            q, x = _rand((2, t_n * l, D), 1.0, 41 + l, dtype), _rand((t_n, n, D), 1.0, 42 + n, dtype)
            assert torch.equal(_short(ops, q, x, wk, wv, bv, l), _fold(other, ops, q, x, wk, wv, bv, l)), (n, t_n, l)
        keep = torch.rand((t_n, n), generator=torch.Generator().manual_seed(n)) > 0.3
        keep[:, 0] = True
        mask = (1.0 - keep.float()) * torch.finfo(torch.float32).min
        assert torch.equal(_short(ops, q, x, wk, wv, bv, l, mask=mask), _fold(other, ops, q, x, wk, wv, bv, l, mask=mask)), (n, "masked")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [197, 577])
def test_short_fold_rows_do_not_depend_on_their_launch(ops, dtype, n):
    """(a) a launch repeats itself, (b) a candidate's rows are the same alone (T = 1) and in a batch of 9, at two places in it, (c) row r of an
    L = 16 launch is the same row of an L = r + 1 launch."""
    t9 = 9
    wk, wv, bv = _rand((2, D, D), 0.03, 53, dtype), _rand((2, D, D), 0.03, 54, dtype), _rand((2, D), 0.5, 56, torch.float32)
    x = _rand((t9, n, D), 1.0, 52, dtype)
    q16 = _rand((2, t9, 16, D), 1.0, 51, dtype)                           # (branch, candidate, token, D)
    pack = lambda cands, l: q16[:, cands, :l].reshape(2, len(cands) * l, D).contiguous()
    every = list(range(t9))
    batch = _short(ops, pack(every, 16), x, wk, wv, bv, 16)
    assert torch.equal(batch, _short(ops, pack(every, 16), x, wk, wv, bv, 16))                       # (a)
    for c in (0, 4, 8):                                                                               # (b)
        assert torch.equal(batch[c], _short(ops, pack([c], 16), x[c:c + 1], wk, wv, bv, 16)[0]), c
    moved = [8, 3, 4, 0, 1, 2, 5, 6, 7]
    again = _short(ops, pack(moved, 16), x[moved], wk, wv, bv, 16)
    assert torch.equal(again[0], batch[8]) and torch.equal(again[1], batch[3]) and torch.equal(again[3], batch[0])
    for r in (0, 6, 12, 14):                                                                          # (c)
        shorter = _short(ops, pack([0, 1], r + 1), x[:2], wk, wv, bv, r + 1)
        assert torch.equal(shorter, batch[:2, :r + 1]), r


@pytest.mark.parametrize("t_n,l,n", [(2, 16, 577), (2, 11, 197)])
def test_short_fold_exact_small_integers(ops, t_n, l, n):
    """Attention over identical keys is the mean of the values whatever the scores: with integer X (all rows equal) and integer W_v the folded
    chain (P X, then W_v) is exact in fp16 - a k-slot / permutation slip in G3 / G4 of the new instantiation shows up as a wrong integer."""
    g = torch.Generator().manual_seed(3)
    row = torch.randint(-2, 3, (t_n, 1, D), generator=g).float()
    x = row.expand(t_n, n, D).contiguous().half()
    q = _rand((2, t_n * l, D), 1.0, 1, F16)
    wk = _rand((2, D, D), 0.03, 2, F16)
    wv = torch.randint(-1, 2, (2, D, D), generator=g).half()
    bv = torch.randint(-3, 4, (2, D), generator=g).float()
    out = _short(ops, q, x, wk, wv, bv, l)
    want = torch.stack([row[:, 0].double() @ wv[b].double().T + bv[b].double() for b in (0, 1)], dim=1)      # (T, 2, D)
    err = (out.cpu().double() - want[:, None].expand(t_n, l, 2, D)).abs().max().item()
    print(f"\n[short fold, constant keys, N {n}] max|err| {err:.2e} (values up to {want.abs().max():.0f})")
    assert err < 0.13          # sums of ~50 terms up to ~100: one fp16 ulp there is 0.06 (P X is exact, the row sum of P rounds)


@pytest.mark.parametrize("n", [577, 608])
def test_short_fold_scores_follow_the_keys(ops, n):
    """One-hot attention at L = 16: each of the 2 x 16 x 12 (branch, token, head) triples is steered to a key of its own - key (3 i + N - 1)
    mod N for triple i, so triple 0 takes the LAST key (576 of 577: the only live key of block 36; 607 of 608: block 37) and at 608 keys
    eleven triples land in blocks 36 and 37, some in each.  A wrong head-to-wave map or a key block staged by the wrong one of the 10 pieces per wave
    returns another key's value."""
    t_n, l = 1, 16
    x = _rand((t_n, n, D), 1.0, 7, F16)
    wk = _rand((2, D, D), 0.05, 8, F16)
    wv = _rand((2, D, D), 0.03, 9, F16)
    bv = _rand((2, D), 0.5, 10, torch.float32)
    k_all = [(x[0].double() @ wk[b].double().T).view(n, H, 64) for b in (0, 1)]
    q = torch.zeros((2, t_n * l, D), dtype=F16)
    picked = set()
    for b in (0, 1):
        for tok in range(l):
            for h in range(H):
                j = (3 * ((b * l + tok) * H + h) + n - 1) % n
                picked.add(j)
                kv = k_all[b][j, h]
                q[b, tok, h * 64:(h + 1) * 64] = (kv * (300.0 / (kv @ kv))).half()          # q . k_j = 300 -> score 37.5 after the 1/8
    assert len(picked) == 2 * l * H and n - 1 in picked and (n == 577 or (any(576 <= j < 592 for j in picked) and any(j >= 592 for j in picked)))
    ref = _reference(q, x, wk, torch.zeros((2, D)), wv, bv, l)
    out = _short(ops, q, x, wk, wv, bv, l)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"\n[short fold, steered heads, N {n}] max|err| vs fp64 {err:.2e}")
    assert err < 2e-2


@pytest.mark.parametrize("t_n,l,n", [(3, 12, 577), (2, 16, 197)])
def test_short_fold_with_a_key_mask(ops, t_n, l, n):
    """The additive key mask of padded candidate token sets against fp64 with the same mask: candidate 0 with a fully masked tail, candidate 1
    with a single open key (its rows are that key's value), the rest random; an all-zero mask next to the unmasked launch, a fully masked
    candidate finite, and a mask whose rows are further apart than N."""
    q = _rand((2, t_n * l, D), 1.0, 11, F16)
    x = _rand((t_n, n, D), 1.0, 12, F16)
    wk, wv = _rand((2, D, D), 0.03, 13, F16), _rand((2, D, D), 0.03, 14, F16)
    bk, bv = _rand((2, D), 0.5, 15, torch.float32), _rand((2, D), 0.5, 16, torch.float32)
    keep = torch.rand((t_n, n), generator=torch.Generator().manual_seed(17)) > 0.3
    keep[:, 0] = True
    keep[0, n // 2:] = False                                             # a candidate padded to half its tokens
    keep[1] = False
    keep[1, n - 3] = True                                                # one open key, in the last key block
    mask = ((1.0 - keep.float()) * torch.finfo(torch.float32).min)
    ref = _reference(q, x, wk, bk, wv, bv, l, mask=mask)
    out = _short(ops, q, x, wk, wv, bv, l, mask=mask)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"\n[short fold, key mask, T {t_n} L {l} N {n}] max|err| vs fp64 {err:.2e}")
    assert err < 6e-3
    plain = _short(ops, q, x, wk, wv, bv, l)
    zero = _short(ops, q, x, wk, wv, bv, l, mask=torch.zeros((t_n, n)))
    assert (plain.float() - zero.float()).abs().max().item() < 2e-3      # (the masked form scales the scores before the maximum: one rounding apart)
    allm = _short(ops, q, x, wk, wv, bv, l, mask=torch.full((t_n, n), torch.finfo(torch.float32).min))
    assert bool(torch.isfinite(allm.float()).all())
    wide = torch.full((t_n, n + 27), float("nan"), device="cuda")        # rows n + 27 apart; what lies between the rows must not be read
    wide[:, :n] = mask.cuda()
    strided = _short(ops, q, x, wk, wv, bv, l, mask=wide[:, :n])
    assert torch.equal(strided, out)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("t_n,l,n", [(3, 12, 577), (5, 16, 608), (9, 13, 17), (2, 1, 225)])
def test_short_fold_guard_bands(ops, dtype, t_n, l, n):
    """The kernel writes token rows < L from one 16-row block per head (rows beyond L are computed on zero queries and must not be stored), reads X
    rows clamped to N - 1 - the two surplus phase-1 pieces and the three surplus phase-2 pieces of a wave included - and weight fragments
    through buffer descriptors.  `out` is the first L rows per candidate of a (T, L + 20, 2, 768) buffer inside a canary frame: everything but
    rows < L and the addressed 2 x 768 columns keeps its canary; tokens and weights sit at the END of their allocations (a read past them would
    meet the next allocation's NaNs and poison the result)."""
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
    lw, pr, pc = l + 20, 40, 64
    big = torch.empty((t_n * lw + 2 * pr, 2 * D + 2 * pc), dtype=dtype, device="cuda")
    big.view(torch.int16).fill_(CANARY[dtype])
    wider = big[pr:pr + t_n * lw, pc:pc + 2 * D].unflatten(0, (t_n, lw)).unflatten(2, (2, D))
    out = wider[:, :l]
    ops.cross_attention_folded_short(q, x, wkt, wvp, bv, out, l, 0.125)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    result = out.clone()
    out.view(torch.int16).fill_(CANARY[dtype]) if out.is_contiguous() else out.copy_(torch.full((), float("nan"), dtype=dtype).expand_as(out))
    bits = big.view(torch.int16).clone()
    rows = torch.zeros(big.shape[0], dtype=torch.bool, device="cuda")
    for t in range(t_n):
        rows[pr + t * lw:pr + t * lw + l] = True
    bits[rows, pc:pc + 2 * D] = CANARY[dtype]                             # the addressed elements
    bad = bits != CANARY[dtype]
    assert not bool(bad.any()), f"short fold T {t_n} L {l} N {n}: {int(bad.sum())} canary elements overwritten, first at {bad.nonzero()[0].tolist()}"
    # against the projected path of the library on the same inputs
    wkv = torch.cat([wk[0], wv[0], wk[1], wv[1]]).cuda()
    bkv = torch.cat([torch.zeros(D, device="cuda"), bv[0], torch.zeros(D, device="cuda"), bv[1]])
    kv = ops.gemm(x.view(t_n * n, D), wkv, bkv).view(t_n, n, 4, D)
    o2 = torch.empty((t_n, l, 2, D), dtype=dtype, device="cuda")
    ops.attention(q.view(2, t_n, l, D).permute(1, 0, 2, 3), kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3), o2.permute(0, 2, 1, 3), 0.125)
    assert (result.float() - o2.float()).abs().max().item() < (6.5e-2 if dtype == BF16 else 4e-3)     # (two roundings: up to two bf16 ulps of 2^-5 at |ctx| ~ 4)


def test_short_fold_rejects_other_geometries(ops):
    from candidate_reranking_cir_amd.lib import CirrankError
    w, bv = torch.zeros((2, D, D), dtype=F16, device="cuda"), torch.zeros((2, D), device="cuda")
    for l, n in ((17, 197), (12, 609)):
        q, x = torch.zeros((2, 2 * l, D), dtype=F16, device="cuda"), torch.zeros((2, n, D), dtype=F16, device="cuda")
        with pytest.raises(CirrankError):
            ops.cross_attention_folded_short(q, x, w, w, bv, torch.empty((2, l, 2, D), dtype=F16, device="cuda"), l, 0.125)


# ------------------------------------------------------------------------------------------------ engine and model
@pytest.fixture(scope="module")
def tiny(ops):
    """The tiny BLIP_NLVR of tests/test_fold_long_gpu.py (3 fusion layers at D = 768, 12 heads, fp16), 12-token captions, 2 queries x 3
    candidates of 197 and of 577 image tokens (the engine takes any token count; the ViT is not run)."""
    from candidate_reranking_cir_amd import synthetic
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    dev = torch.device("cuda")
    vit = VitGeometry(image_size=64, patch_size=16, width=768, depth=1, num_heads=12)
    torch.manual_seed(0)
    m = BLIP_NLVR(BertGeometry(num_hidden_layers=3), vit_geometry=vit, tokenizer=synthetic.HashTokenizer()).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(5)
    q_n, k, l = 2, 3, 12
    z = torch.randn((q_n, l, 768), generator=g).to(dev)
    ids = torch.randint(1000, 20000, (q_n, l), generator=g).to(dev)
    cand = {n: (torch.randn((q_n * k, n, 768), generator=g) * 0.5).to(dev).half() for n in (197, 577)}
    cmask = {n: torch.ones((q_n * k, n), dtype=torch.int64, device=dev) for n in (197, 577)}
    for n in cmask:
        cmask[n][::2, n - 40:] = 0
    return dict(m=m, cand=cand, cmask=cmask, qidx=torch.arange(q_n, device=dev).repeat_interleave(k), i12=(ids, torch.ones_like(ids), z))


def test_engine_takes_the_short_fold_for_12_tokens(tiny):
    """`fold_short` on, 12-token captions: at 577 keys the kernel's bits are the 32-token kernel's, so the whole forward is (`torch.equal`); at
    197 keys the two kernels round differently and the logits stay within 3e-3, the bound tests/test_fold_gpu.py and test_fold_long_gpu.py hold
    between the fold and the projected path at this geometry.  With and without a candidate mask; no fallback counted, no warning."""
    eng = tiny["m"].engines()[1]
    qidx = tiny["qidx"]
    assert eng.fold_short is False
    try:
        for n in (197, 577):
            cand, cm = tiny["cand"][n], tiny["cmask"][n]
            eng.fold_short, eng.fold_fallbacks = False, 0
            off, off_m = eng.forward(*tiny["i12"], cand, qidx), eng.forward(*tiny["i12"], cand, qidx, cand_mask=cm)
            eng.fold_short = True
            assert [lp.cross for lp in eng.plan(12, n, 768, False).layers] == ["fold_short", "fold_short", "cls_fold"]
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                on, on_m = eng.forward(*tiny["i12"], cand, qidx), eng.forward(*tiny["i12"], cand, qidx, cand_mask=cm)
            assert eng.fold_fallbacks == 0 and not [x for x in w if "projected" in str(x.message)]
            d, dm, moved = (on - off).abs().max().item(), (on_m - off_m).abs().max().item(), (on - on_m).abs().max().item()
            print(f"\n[engine, 12 tokens, {n} keys] short fold vs 32-token fold: {d:.2e}, with a candidate mask {dm:.2e}; the mask moves the logits by {moved:.2e}")
            assert moved > 1e-4
            if n == 577:
                assert torch.equal(on, off) and torch.equal(on_m, off_m)
            else:
                assert d < 3e-3 and dm < 3e-3
    finally:
        eng.fold_short, eng.fold_fallbacks = False, 0


def test_model_switch_reaches_the_engine_survives_repacks_and_keys_the_graph(tiny):
    from candidate_reranking_cir_amd import synthetic
    m = tiny["m"]
    try:
        assert m.short_caption_fold is False and m.engines()[1].fold_short is False
        assert m.set_short_caption_fold(True) is m and m.engines()[1].fold_short is True
        m.set_precision("text32")
        assert m.engines()[1].fold_short is True
        m.set_precision("f16")
        m.load_state_dict(m.state_dict())
        assert m.engines()[1].fold_short is True and m.engines()[1].fold_long is False
        # one query of 12 tokens (10 words + [CLS] / [SEP]) against 3 candidates of 577 tokens through the model's own call
        cap = [synthetic.caption_text(7, 10)]
        cand = tiny["cand"][577][:3]
        z = torch.randn((1, 12, 768), generator=torch.Generator().manual_seed(9)).cuda()
        direct = m.img_txt_fusion_val(z, cand, cap)
        m.enable_graphs(64)
        graphs = lambda: len(m.engines()[1]._graphs)
        first, again = m.img_txt_fusion_val(z, cand, cap), m.img_txt_fusion_val(z, cand, cap)
        assert torch.equal(first, direct) and torch.equal(again, direct) and graphs() == 1
        m.set_short_caption_fold(False)                        # the switch is part of the plan key: a new capture, the 32-token kernel - same bits
        off = m.img_txt_fusion_val(z, cand, cap)
        assert graphs() == 2 and torch.equal(off, direct)
        m.set_short_caption_fold(True)                         # back: the first capture is replayed, none added
        assert torch.equal(m.img_txt_fusion_val(z, cand, cap), direct) and graphs() == 2
        cand197 = tiny["cand"][197][:3]                        # 197 keys: another kernel, another rounding
        on197 = m.img_txt_fusion_val(z, cand197, cap)
        m.set_short_caption_fold(False)
        off197 = m.img_txt_fusion_val(z, cand197, cap)
        assert graphs() == 4 and torch.allclose(on197, off197, atol=3e-3) and torch.equal(off197, m.img_txt_fusion_val(z, cand197, cap))
        assert m.engines()[1].fold_fallbacks == 0
    finally:
        m.enable_graphs(0)
        m.set_short_caption_fold(False)
