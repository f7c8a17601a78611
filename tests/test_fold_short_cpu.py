"""cir_cross_attention_folded_short without a GPU: the entry point's host-side refusals (fake, never dereferenced device addresses, as
tests/test_fold_long_cpu.py), the unchanged limits of its two neighbours, and NlvrEngine's choice between the one-block fold and the
32-token kernels, with `ops` replaced by recording stubs (tests/engine_stub.py; the short fold is recorded by a subclass here)."""
import pytest
import torch

from tests.engine_stub import StubOps, run_forward

EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
P = 0x10000          # 16-byte aligned fake device address
BF16, F16, F32 = 0, 1, 2
D = 768
NAMES = ["q", "q_sb", "q_rs", "x", "x_s1", "wkt", "wvp", "w_sb", "bv", "key_mask", "mask_stride", "out", "o_st", "o_sr", "o_sb",
         "T", "L", "N", "D", "H", "scale", "dtype", "stream"]


def _ok(l=12, n=577, t=3):
    return dict(q=P, q_sb=t * l * D, q_rs=D, x=P, x_s1=n * D, wkt=P, wvp=P, w_sb=D * D, bv=P, key_mask=None, mask_stride=0, out=P,
                o_st=l * 2 * D, o_sr=2 * D, o_sb=D, T=t, L=l, N=n, D=D, H=12, scale=0.125, dtype=F16, stream=None)


def _call(fn, l=12, n=577, **over):
    a = _ok(l, n)
    a.update(over)
    return fn(*[a[k] for k in NAMES])


def test_short_fold_refuses_bad_arguments_before_any_launch():
    """The four error codes of include/cirrank.h in the header's order (pointers and extents, shape, dtype, alignment, mask stride): a call
    that is valid but for ONE later fault passes every earlier check, so the EDTYPE / EALIGN / mask-stride answers at L = 16, N = 608 show
    that the largest geometry is not refused by shape (a valid call cannot be launched without a device)."""
    from candidate_reranking_cir_amd import lib
    fn = lib.load().cir_cross_attention_folded_short
    for name in ("q", "x", "wkt", "wvp", "bv", "out"):
        assert _call(fn, **{name: None}) == EINVAL
    assert _call(fn, T=0) == EINVAL and _call(fn, L=0) == EINVAL and _call(fn, N=0) == EINVAL and _call(fn, T=-1) == EINVAL
    assert _call(fn, L=17) == ESHAPE and _call(fn, N=609) == ESHAPE and _call(fn, D=512) == ESHAPE and _call(fn, H=8) == ESHAPE
    assert _call(fn, l=32, n=197) == ESHAPE and _call(fn, l=17, n=1) == ESHAPE
    assert _call(fn, l=16, n=608, dtype=F32) == EDTYPE and _call(fn, l=16, n=608, dtype=7) == EDTYPE
    assert _call(fn, l=16, n=608, out=P + 4) == EALIGN
    assert _call(fn, l=16, n=608, key_mask=P, mask_stride=607) == ESHAPE
    for n in (1, 224, 225):                                          # either kernel's side of the 224-key threshold
        assert _call(fn, l=1, n=n, dtype=7) == EDTYPE and _call(fn, l=16, n=n, q=P + 2) == EALIGN
    assert _call(fn, x=P + 8) == EALIGN and _call(fn, wkt=P + 4) == EALIGN and _call(fn, wvp=P + 8) == EALIGN and _call(fn, bv=P + 4) == EALIGN
    assert _call(fn, q_rs=D + 4) == EALIGN and _call(fn, x_s1=577 * D + 4) == EALIGN and _call(fn, o_sr=2 * D + 2) == EALIGN and _call(fn, o_sb=D + 1) == EALIGN
    assert _call(fn, dtype=F32, out=P + 4, key_mask=P, mask_stride=1) == EDTYPE         # the order: dtype before alignment before the mask stride
    assert _call(fn, out=P + 4, key_mask=P, mask_stride=1) == EALIGN


def test_the_neighbours_keep_their_limits():
    from candidate_reranking_cir_amd import lib
    so = lib.load()
    assert _call(so.cir_cross_attention_folded_long, l=12, n=225) == ESHAPE and _call(so.cir_cross_attention_folded_long, l=65, n=197) == ESHAPE
    assert _call(so.cir_cross_attention_folded_long, l=64, n=224, dtype=F32) == EDTYPE
    assert _call(so.cir_cross_attention_folded, l=33, n=197) == ESHAPE and _call(so.cir_cross_attention_folded, l=12, n=609) == ESHAPE
    assert _call(so.cir_cross_attention_folded, l=32, n=608, dtype=F32) == EDTYPE
    assert so.cir_version() == 15


# ------------------------------------------------------------------------------------------------ engine dispatch
LAYERS = 4           # fusion layers 0 .. 2 run per-token cross-attention, the last one the CLS rows only (as tests/test_fold_long_cpu.py)


class ShortStub(StubOps):
    def cross_attention_folded_short(self, q, x, wkt, wvp, bv, out, l, scale, heads=12, mask=None):
        args = dict(locals()); del args["self"]
        self.calls.append(("folded_short", l, x.shape[1], mask is not None))
        return self._record("cross_attention_folded_short", args, out)


@pytest.fixture(scope="module")
def engine():
    from candidate_reranking_cir_amd import engine as E
    from candidate_reranking_cir_amd import weights
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    geo = BertGeometry(num_hidden_layers=LAYERS)
    vit = VitGeometry(image_size=64, patch_size=16, width=768, depth=1, num_heads=12)
    geo.encoder_width = vit.width
    try:
        sd = weights.synth_state_dict(weights.nlvr_param_spec(geo, vit), 1)
        return E.NlvrEngine(sd, geo, torch.float16, torch.device("cpu"))
    except (RuntimeError, AssertionError) as e:            # (packing that needs a device)
        pytest.skip(f"NlvrEngine cannot be packed without a device: {e}")


def _run(engine, monkeypatch, l, n, cand_mask=False, stub_cls=ShortStub):
    q_n, k = 1, 2
    stub, _, w = run_forward(engine, monkeypatch, l, n, q_n, k, cand_mask, stub=stub_cls(engine))
    kv_gemms = [c for c in stub.calls if c[0] == "gemm" and c[1] == (q_n * k * n, D) and c[2] == (4 * D, D)]
    return [c for c in stub.calls if c[0].startswith("folded")], kv_gemms, [x for x in w if "projected" in str(x.message)], stub


def test_engine_dispatch_for_short_captions(engine, monkeypatch):
    assert engine.fold_short is False and engine.fold_long is False and engine.fold_cross_kv
    try:
        # switch off, 12 tokens: exactly the parent's calls - on the parent's stub, which has no short fold to call
        for n in (197, 577):
            for masked in (False, True):
                folds, kv, warned, _ = _run(engine, monkeypatch, 12, n, masked, stub_cls=StubOps)
                assert folds == [("folded", 12, n, masked)] * (LAYERS - 1) and len(kv) == int(masked) and not warned
        # switch on, 1 / 12 / 16 tokens against 197 and 577 keys, with and without a candidate mask: one short fold per per-token layer
        engine.fold_short, engine.fold_fallbacks = True, 0
        for l in (1, 12, 16):
            for n in (197, 577):
                for masked in (False, True):
                    folds, kv, warned, stub = _run(engine, monkeypatch, l, n, masked)
                    assert folds == [("folded_short", l, n, masked)] * (LAYERS - 1), (l, n, masked)
                    assert len(kv) == int(masked) and not warned and engine.fold_fallbacks == 0     # (masked: the CLS-only last layer projects, as before)
                    assert [t[0] for t in stub.trace].count("cross_attention_folded_short") == LAYERS - 1
        # 17 and 32 tokens: the 32-token kernels
        for l in (17, 32):
            for n in (197, 577):
                folds, kv, warned, _ = _run(engine, monkeypatch, l, n)
                assert folds == [("folded", l, n, False)] * (LAYERS - 1) and not kv and not warned
        # 609 keys at 12 tokens: nothing folds, as in the parent (not a long caption: not counted)
        folds, kv, warned, _ = _run(engine, monkeypatch, 12, 609)
        assert not folds and len(kv) == LAYERS - 1 and engine.fold_fallbacks == 0
        # 40 tokens: what `fold_long` says, as before
        for long_on in (False, True):
            engine.fold_long, before = long_on, engine.fold_fallbacks
            folds, kv, warned, _ = _run(engine, monkeypatch, 40, 197)
            if long_on:
                assert folds == [("folded_long", 40, 197, False)] * (LAYERS - 1) and not kv and engine.fold_fallbacks == before
            else:
                assert not folds and len(kv) == LAYERS - 1 and engine.fold_fallbacks == before + 1
        engine.fold_long = False
        # without the fold at all the switch is inert
        engine.fold_cross_kv, before = False, engine.fold_fallbacks
        folds, kv, warned, _ = _run(engine, monkeypatch, 12, 197)
        assert not folds and len(kv) == LAYERS - 1 and not warned and engine.fold_fallbacks == before
    finally:
        engine.fold_cross_kv, engine.fold_long, engine.fold_short, engine.fold_fallbacks = True, False, False, 0


def test_plan_with_the_switch_off_is_the_parents_plan(engine):
    """Off, `plan` names no path the parent did not know; on, it differs from the off plan in the foldable layers of L <= 16, N <= 608 and
    nowhere else - so captured graphs of those calls get a key of their own and every other key is the parent's."""
    assert engine.fold_short is False
    cases = [(l, n, m) for l in (1, 12, 16, 17, 32, 33, 40, 64, 65) for n in (1, 197, 224, 225, 577, 608, 609) for m in (False, True)]
    off = {c: engine.plan(c[0], c[1], D, c[2]) for c in cases}
    for (l, n, m), p in off.items():
        assert all(lp.cross in ("cls_fold", "fold32", "fold_long", "projected") for lp in p.layers)
        want = "fold32" if (l <= 32 and n <= 608) else "projected"
        assert [lp.cross for lp in p.layers[:-1]] == [want] * (LAYERS - 1), (l, n, m)
    engine.fold_short = True
    try:
        for (l, n, m), p in off.items():
            on = engine.plan(l, n, D, m)
            if l <= 16 and n <= 608:
                assert [lp.cross for lp in on.layers] == ["fold_short"] * (LAYERS - 1) + [p.layers[-1].cross] and on != p
                assert on._replace(layers=tuple(lp._replace(cross=q.cross) for lp, q in zip(on.layers, p.layers))) == p
            else:
                assert on == p, (l, n, m)
        other_width = engine.plan(12, 197, 512, False)                     # candidate tokens of another width: untouched
        engine.fold_short = False
        assert other_width == engine.plan(12, 197, 512, False) and other_width.layers[0].cross == "projected"
    finally:
        engine.fold_short = False


def test_model_switch_is_off_by_default_and_survives_a_repack():
    from candidate_reranking_cir_amd import synthetic
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    g = BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, encoder_width=128)
    v = VitGeometry(image_size=64, width=128, depth=1, num_heads=2)
    m = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    assert m.short_caption_fold is False
    assert m.set_short_caption_fold() is m and m.short_caption_fold is True
    assert m.set_short_caption_fold(False).short_caption_fold is False
    m.set_short_caption_fold(True)
    sd = {k: p.detach() for k, p in m.state_dict().items()}
    first = m._text_engine(sd)
    assert first.fold_short is True and first.fold_long is False
    m.set_precision("bf16")                                       # a repack: the next engine is packed anew and gets the model's setting
    again = m._text_engine(sd)
    assert again is not first and again.fold_short is True
    m.set_short_caption_fold(False)
    assert m._text_engine(sd).fold_short is False
