"""cir_cross_attention_folded_long_wide: the query-side fold for captions of 33-64 tokens against 225-608 keys (csrc/xattn_fold_units.hip, the
key-split instantiation: per head two token halves x two key halves of 20 16-key blocks) - against the fp64 restatement of the reference's
arithmetic and the projected path of this library on the inputs of tests/test_fold_long_gpu.py (q and x at sigma 1, weights at sigma 0.03,
biases at sigma 0.5) with the bounds the project holds for its 16-row folds.  Then what the key split adds: a second half with no key, exactly
one key or a mask over a whole half (maximum -inf, probability 0, nothing but finite numbers), the token / head / half-to-wave maps, stores
confined to rows < L, and one accumulation order per row whatever T, L or the candidate's place in the batch."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
D, H = 768, 12
F16, BF16 = torch.float16, torch.bfloat16
CANARY = {BF16: 0x7FC1, F16: 0x7E01}        # NaN patterns (as tests/test_fold_long_gpu.py)
FMIN = torch.finfo(torch.float32).min


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


def _wide(ops, q, x, wk, wv, bv, l, mask=None, out=None):
    out = torch.empty((x.shape[0], l, 2, D), dtype=x.dtype, device="cuda") if out is None else out
    ops.cross_attention_folded_long_wide(q.cuda(), x.cuda(), ops.fold_pack_key(wk).cuda(), ops.fold_pack_value(wv).cuda(), bv.cuda(), out, l, 0.125,
                                         mask=None if mask is None else mask.cuda())
    return out


def _projected(ops, q, x, wk, bk, wv, bv, l, mask=None):
    """The projected path on the same inputs: [K0 V0 K1 V1] GEMM + attention."""
    t_n, n, _ = x.shape
    wkv = torch.cat([wk[0], wv[0], wk[1], wv[1]]).cuda()
    bkv = torch.cat([bk[0], bv[0], bk[1], bv[1]]).cuda()
    kv = ops.gemm(x.cuda().view(t_n * n, D), wkv, bkv).view(t_n, n, 4, D)
    o2 = torch.empty((t_n, l, 2, D), dtype=x.dtype, device="cuda")
    qc = q.cuda().view(2, t_n, l, D).permute(1, 0, 2, 3)
    emask = None if mask is None else mask.cuda().view(t_n, 1, n).expand(t_n, 2, n)
    ops.attention(qc, kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3), o2.permute(0, 2, 1, 3), 0.125, emask)
    return o2


def _inputs(t_n, l, n, dtype, seed=0):
    q = _rand((2, t_n * l, D), 1.0, seed + 1, dtype)
    x = _rand((t_n, n, D), 1.0, seed + 2, dtype)
    wk, wv = _rand((2, D, D), 0.03, seed + 3, dtype), _rand((2, D, D), 0.03, seed + 4, dtype)
    bk, bv = _rand((2, D), 0.5, seed + 5, torch.float32), _rand((2, D), 0.5, seed + 6, torch.float32)
    return q, x, wk, bk, wv, bv


def _check_bounds(what, out, o2, ref, dtype):
    err = (out.cpu().double() - ref).abs().max().item()
    err2 = (o2.cpu().double() - ref).abs().max().item()
    print(f"\n[{what}] max|err| vs fp64: folded {err:.2e}, projected {err2:.2e} (|ctx| max {ref.abs().max():.2f})")
    assert bool(torch.isfinite(out.float()).all())
    tol = 4e-2 if dtype == BF16 else 6e-3
    assert err < tol and err < 2.5 * err2 + 1e-3


# 225 / 320 / 321 keys: no key, exactly the last key of half 0, and one key in the second half; 305 ends inside half 0's last block; 608 fills
# the last real block (blocks 38 and 39 of the 640-key capacity never hold a key)
SHAPES = [(2, 33, 577), (1, 64, 577), (2, 48, 608), (3, 49, 225), (2, 40, 320), (2, 40, 321), (1, 64, 305)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("t_n,l,n", SHAPES)
def test_wide_fold_against_fp64_and_projected_path(ops, dtype, t_n, l, n):
    q, x, wk, bk, wv, bv = _inputs(t_n, l, n, dtype)
    ref = _reference(q, x, wk, bk, wv, bv, l)
    out = _wide(ops, q, x, wk, wv, bv, l)
    o2 = _projected(ops, q, x, wk, bk, wv, bv, l)
    torch.cuda.synchronize()
    _check_bounds(f"wide fold {dtype} T {t_n} L {l} N {n}", out, o2, ref, dtype)


@pytest.mark.parametrize("t_n,l,n", [(2, 40, 577), (2, 64, 300)])
def test_wide_fold_exact_small_integers(ops, t_n, l, n):
    """Attention over identical keys is the mean of the values whatever the scores and however the keys are split: with integer X (all rows
    equal) and integer W_v the folded chain (P X, then W_v) is exact in fp16 - a k-slot / permutation slip in G3 / G4, or a half counted
    twice or not at all in the row sum, shows up as a wrong integer."""
    g = torch.Generator().manual_seed(3)
    row = torch.randint(-2, 3, (t_n, 1, D), generator=g).float()
    x = row.expand(t_n, n, D).contiguous().half()
    q = _rand((2, t_n * l, D), 1.0, 1, F16)
    wk = _rand((2, D, D), 0.03, 2, F16)
    wv = torch.randint(-1, 2, (2, D, D), generator=g).half()
    bv = torch.randint(-3, 4, (2, D), generator=g).float()
    out = _wide(ops, q, x, wk, wv, bv, l)
    want = torch.stack([row[:, 0].double() @ wv[b].double().T + bv[b].double() for b in (0, 1)], dim=1)      # (T, 2, D)
    err = (out.cpu().double() - want[:, None].expand(t_n, l, 2, D)).abs().max().item()
    print(f"\n[wide fold, constant keys, L {l} N {n}] max|err| {err:.2e} (values up to {want.abs().max():.0f})")
    assert err < 0.13          # sums of ~50 terms up to ~100: one fp16 ulp there is 0.06 (P X is exact, the row sum of P rounds)


def test_wide_fold_scores_follow_the_keys(ops):
    """One-hot attention at L = 64, N = 577: every (branch, token, head) is steered to a key of its own, spread over BOTH key halves, so a
    wrong token-to-wave, head-to-wave or half-to-wave map returns another key's value."""
    t_n, l, n = 1, 64, 577
    x = _rand((t_n, n, D), 1.0, 7, F16)
    wk = _rand((2, D, D), 0.05, 8, F16)
    wv = _rand((2, D, D), 0.03, 9, F16)
    bv = _rand((2, D), 0.5, 10, torch.float32)
    k_all = [(x[0].double() @ wk[b].double().T).view(n, H, 64) for b in (0, 1)]
    q = torch.zeros((2, t_n * l, D), dtype=F16)
    targets = []
    for b in (0, 1):
        for tok in range(l):
            for h in range(H):
                j = (37 * tok + 11 * h + 5 * b) % n
                targets.append(j)
                kv = k_all[b][j, h]
                q[b, tok, h * 64:(h + 1) * 64] = (kv * (300.0 / (kv @ kv))).half()          # q . k_j = 300 -> score 37.5 after the 1/8
    assert min(targets) < 16 and max(targets) >= 560 and sum(j >= 320 for j in targets) > 400 and sum(j < 320 for j in targets) > 400
    ref = _reference(q, x, wk, torch.zeros((2, D)), wv, bv, l)
    out = _wide(ops, q, x, wk, wv, bv, l)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"\n[wide fold, steered heads] max|err| vs fp64 {err:.2e}")
    assert err < 2e-2


def _masks(t_n, n):
    tail = torch.zeros((t_n, n))
    tail[0, n // 2:] = FMIN                                               # a candidate padded to half its tokens
    tail[1, n - 5:] = FMIN
    low = torch.zeros((t_n, n))
    low[:, :320] = FMIN                                                   # all of half 0: its maximum is the clamped mask value, not a key's score
    high = torch.zeros((t_n, n))
    high[:, 320:] = FMIN                                                  # all of half 1
    return {"tail": tail, "keys 0-319": low, "keys 320-": high}


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("which", ["tail", "keys 0-319", "keys 320-"])
def test_wide_fold_with_a_key_mask(ops, dtype, which):
    """The additive key mask of padded candidate token sets, removing a tail, the whole first key half or the whole second one: the fp64
    restatement with the same mask, the bounds of the unmasked test, every output finite."""
    t_n, l, n = 2, 40, 577
    q, x, wk, bk, wv, bv = _inputs(t_n, l, n, dtype, seed=10)
    mask = _masks(t_n, n)[which]
    ref = _reference(q, x, wk, bk, wv, bv, l, mask=mask)
    out = _wide(ops, q, x, wk, wv, bv, l, mask=mask)
    o2 = _projected(ops, q, x, wk, bk, wv, bv, l, mask=mask)
    torch.cuda.synchronize()
    _check_bounds(f"wide fold {dtype}, mask over {which}", out, o2, ref, dtype)
    if which == "tail" and dtype == F16:
        zero = _wide(ops, q, x, wk, wv, bv, l, mask=torch.zeros((t_n, n)))
        plain = _wide(ops, q, x, wk, wv, bv, l)
        assert (plain.float() - zero.float()).abs().max().item() < 2e-3      # (the masked form scales the scores before the maximum: one rounding apart)
        allm = _wide(ops, q, x, wk, wv, bv, l, mask=torch.full((t_n, n), FMIN))
        assert bool(torch.isfinite(allm.float()).all())
        wide = torch.full((t_n, n + 27), float("nan"), device="cuda")        # rows n + 27 apart; what lies between the rows must not be read
        wide[:, :n] = mask.cuda()
        assert torch.equal(_wide(ops, q, x, wk, wv, bv, l, mask=wide[:, :n]), out)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_wide_fold_rows_do_not_depend_on_their_launch(ops, dtype):
    """(a) a candidate's rows are the same alone and as member 0 / 2 of a batch of 3, (b) the common token rows are the same whether the
    caption has 33, 48, 49 or 64 tokens (one instantiation; rows >= L run on zero queries), (c) a launch repeats itself."""
    n, t3 = 577, 3
    wk, wv, bv = _rand((2, D, D), 0.03, 23, dtype), _rand((2, D, D), 0.03, 24, dtype), _rand((2, D), 0.5, 26, torch.float32)
    x = _rand((t3, n, D), 1.0, 22, dtype)
    q64 = _rand((2, t3, 64, D), 1.0, 21, dtype)                           # (branch, candidate, token, D)
    pack = lambda cands, l: q64[:, cands, :l].reshape(2, len(cands) * l, D).contiguous()
    l = 40
    batch = _wide(ops, pack([0, 1, 2], l), x, wk, wv, bv, l)
    assert torch.equal(batch, _wide(ops, pack([0, 1, 2], l), x, wk, wv, bv, l))
    for c in (0, 2):
        alone = _wide(ops, pack([c], l), x[c:c + 1], wk, wv, bv, l)
        assert torch.equal(batch[c], alone[0]), c
    outs = {l: _wide(ops, pack([0, 1], l), x[:2], wk, wv, bv, l) for l in (33, 48, 49, 64)}
    assert bool(torch.isfinite(outs[64].float()).all())
    for l in (48, 49, 64):
        assert torch.equal(outs[l][:, :33], outs[33]), l
    assert torch.equal(outs[64][:, :48], outs[48]) and torch.equal(outs[64][:, :49], outs[49]) and torch.equal(outs[49][:, :48], outs[48])
    assert torch.equal(outs[48][:, :40], batch[:2])


class Guarded:
    """A (rows, cols) output view inside a canary-filled (rows + 2 pr, cols + 2 pc) allocation (as tests/test_fold_long_gpu.py)."""

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
@pytest.mark.parametrize("t_n,l,n", [(2, 33, 577), (3, 49, 225)])
def test_wide_fold_guard_bands(ops, dtype, t_n, l, n):
    """The kernel writes token rows < L of a (T, L, 2, 768) tensor from four 16-row blocks per head (rows beyond L run on zero queries and
    must not be stored: with the candidates packed L rows apart such a store would land in the next candidate or in the guard rows), reads X
    rows clamped to N - 1 and weight fragments through buffer descriptors: output inside canaries, every element of it written (no canary NaN
    left), and the tokens / weights sit at the END of their allocations."""
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
    ops.cross_attention_folded_long_wide(q, x, wkt, wvp, bv, out, l, 0.125)
    torch.cuda.synchronize()
    guard.assert_intact(f"wide fold T {t_n} L {l} N {n}")
    assert torch.isfinite(out.float()).all()
    # only rows < L of each candidate change: candidates 2 L rows apart, the rows between them canaries before and after
    spaced = Guarded(t_n * 2 * l, 2 * D, dtype, pc=0)
    view = spaced.view.unflatten(0, (t_n, 2 * l)).unflatten(2, (2, D))
    ops.cross_attention_folded_long_wide(q, x, wkt, wvp, bv, view[:, :l], l, 0.125)
    torch.cuda.synchronize()
    spaced.assert_intact(f"wide fold, spaced candidates, T {t_n} L {l} N {n}")
    assert torch.equal(view[:, :l], out)
    assert bool((view[:, l:].contiguous().view(torch.int16) == CANARY[dtype]).all())
    zb = torch.zeros((2, D))
    o2 = _projected(ops, q.cpu(), x.cpu(), wk, zb, wv, bv.cpu(), l)
    assert (out.float() - o2.float()).abs().max().item() < (6.5e-2 if dtype == BF16 else 4e-3)     # (two roundings: up to two bf16 ulps of 2^-5 at |ctx| ~ 4)


# ------------------------------------------------------------------------------------------------ engine and model
@pytest.fixture(scope="module")
def tiny(ops):
    """A BLIP_NLVR at hidden 768 / 12 heads with a ViT of depth 1 at 256 px (257 image tokens: above the 224 of the other long-caption fold),
    fp16, 40-token captions.  Three fusion layers = two per-token layers and the CLS-only last one, as the tiny model of
    tests/test_fold_long_gpu.py: `fold_fallbacks` is counted on layer 1, which in a model of two layers is the CLS-only one and never counts."""
    from candidate_reranking_cir_amd import synthetic
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    dev = torch.device("cuda")
    vit = VitGeometry(image_size=256, patch_size=16, width=768, depth=1, num_heads=12)
    assert vit.num_tokens == 257
    torch.manual_seed(0)
    m = BLIP_NLVR(BertGeometry(num_hidden_layers=3), vit_geometry=vit, tokenizer=synthetic.HashTokenizer()).to(dev).eval()
    g = torch.Generator(device="cpu").manual_seed(5)
    q_n, k, n = 2, 3, vit.num_tokens
    z = torch.randn((q_n, 40, 768), generator=g).to(dev)
    ids = torch.randint(1000, 20000, (q_n, 40), generator=g).to(dev)
    cand = (torch.randn((q_n * k, n, 768), generator=g) * 0.5).to(dev).half()
    qidx = torch.arange(q_n, device=dev).repeat_interleave(k)
    cmask = torch.ones((q_n * k, n), dtype=torch.int64, device=dev)
    cmask[::2, n - 4:] = 0
    return dict(m=m, cand=cand, qidx=qidx, cmask=cmask, i40=(ids, torch.ones_like(ids), z))


def test_model_takes_the_wide_fold_for_40_tokens_at_257_keys(tiny):
    """`set_long_caption_fold_wide(True)`: the plan names the new path on the per-token layer, the logits agree with the switch-off logits
    (the projected path) within 3e-3 - the bound tests/test_fold_long_gpu.py holds for its on / off comparison -, with a candidate mask the
    same, and `fold_fallbacks` moves only with the switch off.  `fold_long` alone leaves the geometry projected."""
    m = tiny["m"]
    cand, qidx = tiny["cand"], tiny["qidx"]
    try:
        assert m.long_caption_fold_wide is False and m.engines()[1].fold_long_wide is False
        assert m.set_long_caption_fold_wide(True) is m
        eng = m.engines()[1]
        assert eng.fold_long_wide is True and eng.fold_long is False
        assert [lp.cross for lp in eng.plan(40, 257, 768, False).layers] == ["fold_long_wide", "fold_long_wide", "cls_fold"]
        eng.fold_fallbacks = 0
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            on = eng.forward(*tiny["i40"], cand, qidx)
            on_m = eng.forward(*tiny["i40"], cand, qidx, cand_mask=tiny["cmask"])
        assert eng.fold_fallbacks == 0 and not [x for x in w if "projected" in str(x.message)]
        assert [lp.cross for lp in eng.plan(40, 257, 768, True).layers] == ["fold_long_wide", "fold_long_wide", "projected"]
        m.set_long_caption_fold_wide(False)
        m.set_long_caption_fold(True)                          # the 224-key switch does not reach 257 keys
        assert [lp.cross for lp in eng.plan(40, 257, 768, False).layers] == ["projected", "projected", "cls_fold"]
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            off = eng.forward(*tiny["i40"], cand, qidx)
            off_m = eng.forward(*tiny["i40"], cand, qidx, cand_mask=tiny["cmask"])
        assert eng.fold_fallbacks == 2
        d, dm = (on - off).abs().max().item(), (on_m - off_m).abs().max().item()
        print(f"\n[model, 40 tokens x 257 keys] wide fold vs projected: {d:.2e}, with a candidate mask {dm:.2e}; the mask moves the logits by "
              f"{(on - on_m).abs().max().item():.2e}")
        assert bool(torch.isfinite(on).all()) and d < 3e-3 and dm < 3e-3 and (on - on_m).abs().max().item() > 1e-4
    finally:
        m.set_long_caption_fold(False)
        m.set_long_caption_fold_wide(False)
        m.engines()[1].fold_fallbacks = 0


def test_model_switch_survives_repacks_and_keys_the_graph(tiny):
    from candidate_reranking_cir_amd import synthetic
    m = tiny["m"]
    try:
        assert m.set_long_caption_fold_wide(True) is m and m.engines()[1].fold_long_wide is True
        m.set_precision("text32")
        assert m.engines()[1].fold_long_wide is True
        m.set_precision("f16")
        m.load_state_dict(m.state_dict())
        eng = m.engines()[1]
        assert eng.fold_long_wide is True
        # one query of 40 tokens (38 words + [CLS] / [SEP]) against 3 candidates through the model's own call
        cap = [synthetic.caption_text(7, 38)]
        cand = tiny["cand"][:3]
        z = torch.randn((1, 40, 768), generator=torch.Generator().manual_seed(9)).cuda()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            direct = m.img_txt_fusion_val(z, cand, cap)
        assert m.engines()[1].fold_fallbacks == 0 and not [x for x in w if "projected" in str(x.message)]
        m.enable_graphs(64)
        first, again = m.img_txt_fusion_val(z, cand, cap), m.img_txt_fusion_val(z, cand, cap)
        assert torch.equal(first, direct) and torch.equal(again, direct) and len(m.engines()[1]._graphs) == 1
        m.set_long_caption_fold_wide(False)                    # the switch is part of the plan key: a new capture, the projected path
        with warnings.catch_warnings(record=True):
            warnings.simplefilter("always")
            off = m.img_txt_fusion_val(z, cand, cap)
        assert torch.allclose(off, direct, atol=3e-3) and len(m.engines()[1]._graphs) == 2
        assert m.engines()[1].fold_fallbacks > 0
    finally:
        m.enable_graphs(0)
        m.set_long_caption_fold_wide(False)
        m.engines()[1].fold_fallbacks = 0
