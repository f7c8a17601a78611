"""cir_cross_attention_folded_long without a GPU: the entry point's host-side refusals (fake, never dereferenced device addresses, as
test_abi.py::test_argument_validation_happens_before_any_launch) and NlvrEngine's choice between the long-caption fold and the projected
path, with `ops` replaced by recording stubs that return tensors of the right shape (tests/engine_stub.py)."""
import pytest
import torch

from tests.engine_stub import run_forward

EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
P = 0x10000          # 16-byte aligned fake device address
BF16, F16, F32 = 0, 1, 2
D = 768
NAMES = ["q", "q_sb", "q_rs", "x", "x_s1", "wkt", "wvp", "w_sb", "bv", "key_mask", "mask_stride", "out", "o_st", "o_sr", "o_sb",
         "T", "L", "N", "D", "H", "scale", "dtype", "stream"]


def _ok(l=40, n=197, t=3):
    return dict(q=P, q_sb=t * l * D, q_rs=D, x=P, x_s1=n * D, wkt=P, wvp=P, w_sb=D * D, bv=P, key_mask=None, mask_stride=0, out=P,
                o_st=l * 2 * D, o_sr=2 * D, o_sb=D, T=t, L=l, N=n, D=D, H=12, scale=0.125, dtype=F16, stream=None)


def _call(fn, l=40, n=197, **over):
    a = _ok(l, n)
    a.update(over)
    return fn(*[a[k] for k in NAMES])


def test_long_fold_refuses_bad_arguments_before_any_launch():
    """The four error codes of include/cirrank.h, each from the host-side checks.  The checks come in the header's order (pointers and extents,
    shape, dtype, alignment, mask stride), so a call that is valid but for ONE later fault passes every earlier check: the EDTYPE / EALIGN /
    mask-stride answers at L = 64, N = 224 show that this geometry is not refused by shape (a valid call cannot be launched without a device)."""
    from candidate_reranking_cir_amd import lib
    fn = lib.load().cir_cross_attention_folded_long
    for name in ("q", "x", "wkt", "wvp", "bv", "out"):
        assert _call(fn, **{name: None}) == EINVAL
    assert _call(fn, T=0) == EINVAL and _call(fn, L=0) == EINVAL and _call(fn, N=0) == EINVAL and _call(fn, T=-1) == EINVAL
    assert _call(fn, D=512) == ESHAPE and _call(fn, H=8) == ESHAPE
    assert _call(fn, L=65) == ESHAPE and _call(fn, N=225) == ESHAPE and _call(fn, l=32, n=577) == ESHAPE
    assert _call(fn, key_mask=P, mask_stride=196) == ESHAPE
    assert _call(fn, dtype=F32) == EDTYPE and _call(fn, dtype=7) == EDTYPE
    assert _call(fn, q=P + 2) == EALIGN and _call(fn, x=P + 8) == EALIGN and _call(fn, wkt=P + 4) == EALIGN and _call(fn, wvp=P + 8) == EALIGN
    assert _call(fn, bv=P + 4) == EALIGN and _call(fn, out=P + 4) == EALIGN
    assert _call(fn, q_rs=D + 4) == EALIGN and _call(fn, x_s1=197 * D + 4) == EALIGN and _call(fn, o_sr=2 * D + 2) == EALIGN and _call(fn, o_sb=D + 1) == EALIGN
    # the largest geometry passes the shape check: its refusals are the LATER checks'
    assert _call(fn, l=64, n=224, dtype=F32) == EDTYPE
    assert _call(fn, l=64, n=224, out=P + 4) == EALIGN
    assert _call(fn, l=64, n=224, key_mask=P, mask_stride=223) == ESHAPE
    assert _call(fn, l=1, n=1, dtype=7) == EDTYPE


def test_short_fold_still_refuses_33_tokens():
    from candidate_reranking_cir_amd import lib
    fn = lib.load().cir_cross_attention_folded
    assert _call(fn, l=33) == ESHAPE and _call(fn, l=64, n=224) == ESHAPE
    assert _call(fn, l=32, dtype=F32) == EDTYPE                      # (32 tokens pass the shape check)


# ------------------------------------------------------------------------------------------------ engine dispatch
LAYERS = 4           # fusion layers 0 .. 2 run per-token cross-attention (the full model's 0 .. 10), the last one the CLS rows only; the choice of
                     # path does not look at the layer index, and packing 12 layers on the host takes 8 s


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


def _run(engine, monkeypatch, l, n, cand_mask=False):
    q_n, k = 1, 2
    stub, _, w = run_forward(engine, monkeypatch, l, n, q_n, k, cand_mask)
    kv_gemms = [c for c in stub.calls if c[0] == "gemm" and c[1] == (q_n * k * n, D) and c[2] == (4 * D, D)]
    return stub.calls, kv_gemms, [x for x in w if "projected" in str(x.message)]


def test_engine_dispatch_for_long_captions(engine, monkeypatch):
    assert engine.fold_long is False and engine.fold_cross_kv
    # flag off, 40 tokens: the projected path on every per-token layer and the counter, as before
    engine.fold_fallbacks = 0
    calls, kv, warned = _run(engine, monkeypatch, 40, 197)
    assert len(kv) == LAYERS - 1 and not [c for c in calls if c[0] in ("folded", "folded_long")]
    assert engine.fold_fallbacks == 1 and len(warned) == 1
    # flag off, 32 tokens: the 32-token fold, whatever the flag
    for flag in (False, True):
        engine.fold_long = flag
        calls, kv, warned = _run(engine, monkeypatch, 32, 197)
        assert [c for c in calls if c[0].startswith("folded")] == [("folded", 32, 197, False)] * (LAYERS - 1) and not kv and not warned
    # flag on, 33 / 40 / 64 tokens: one long fold per per-token layer, the counter does not move, no warning
    engine.fold_long = True
    before = engine.fold_fallbacks
    for l in (33, 40, 64):
        calls, kv, warned = _run(engine, monkeypatch, l, 197)
        assert [c for c in calls if c[0].startswith("folded")] == [("folded_long", l, 197, False)] * (LAYERS - 1)
        assert not kv and not warned and engine.fold_fallbacks == before
    calls, kv, warned = _run(engine, monkeypatch, 40, 224, cand_mask=True)             # the key mask goes with it
    assert [c for c in calls if c[0].startswith("folded")] == [("folded_long", 40, 224, True)] * (LAYERS - 1)
    assert len(kv) == 1                                                                # (the CLS-only last layer: masked, so projected as before)
    # 65 tokens, and 300 keys at 40 tokens: projected, counted
    calls, kv, _ = _run(engine, monkeypatch, 65, 197)
    assert len(kv) == LAYERS - 1 and not [c for c in calls if c[0].startswith("folded")] and engine.fold_fallbacks == before + 1
    calls, kv, _ = _run(engine, monkeypatch, 40, 300)
    assert len(kv) == LAYERS - 1 and not [c for c in calls if c[0].startswith("folded")] and engine.fold_fallbacks == before + 2
    # without the fold at all the flag changes nothing
    engine.fold_cross_kv = False
    calls, kv, _ = _run(engine, monkeypatch, 40, 197)
    assert len(kv) == LAYERS - 1 and not [c for c in calls if c[0].startswith("folded")] and engine.fold_fallbacks == before + 2
    engine.fold_cross_kv, engine.fold_long = True, False


def test_model_switch_is_off_by_default_and_stored_on_the_model():
    from candidate_reranking_cir_amd import synthetic
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    g = BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, encoder_width=128)
    v = VitGeometry(image_size=64, width=128, depth=1, num_heads=2)
    m = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    assert m.long_caption_fold is False
    assert m.set_long_caption_fold() is m and m.long_caption_fold is True
    assert m.set_long_caption_fold(False).long_caption_fold is False
