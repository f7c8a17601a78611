"""cir_cross_attention_folded_long_wide without a GPU: the symbol and its host-side refusals (fake, never dereferenced device addresses, as
tests/test_fold_long_cpu.py), the unchanged limit of cir_cross_attention_folded_long at 225 keys, NlvrEngine's plan with the second switch
(`fold_long_wide`: 33-64 caption tokens against 225-608 keys) off and on, its dispatch on recording stubs, and the model switch."""
import ctypes
import os
import re

import pytest
import torch

from tests.engine_stub import StubOps, run_forward

EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
P = 0x10000          # 16-byte aligned fake device address
BF16, F16, F32 = 0, 1, 2
D = 768
NAMES = ["q", "q_sb", "q_rs", "x", "x_s1", "wkt", "wvp", "w_sb", "bv", "key_mask", "mask_stride", "out", "o_st", "o_sr", "o_sb",
         "T", "L", "N", "D", "H", "scale", "dtype", "stream"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ok(l=40, n=577, t=3):
    return dict(q=P, q_sb=t * l * D, q_rs=D, x=P, x_s1=n * D, wkt=P, wvp=P, w_sb=D * D, bv=P, key_mask=None, mask_stride=0, out=P,
                o_st=l * 2 * D, o_sr=2 * D, o_sb=D, T=t, L=l, N=n, D=D, H=12, scale=0.125, dtype=F16, stream=None)


def _call(fn, l=40, n=577, **over):
    a = _ok(l, n)
    a.update(over)
    return fn(*[a[k] for k in NAMES])


def test_symbol_signature_and_refusals_before_any_launch():
    """The header declares the entry point with cir_cross_attention_folded_long's parameter list, lib.py carries the same ctypes signature, and
    every geometry outside D = 768, H = 12, 33 <= L <= 64, 225 <= N <= 608 is CIR_ESHAPE from the host-side checks.  The corners of the accepted
    range pass the shape check: their refusals are the LATER checks' (a valid call cannot be launched without a device)."""
    from candidate_reranking_cir_amd import lib
    with open(os.path.join(ROOT, "include", "cirrank.h")) as f:
        header = f.read()
    params = lambda name: re.sub(r"\s+", " ", re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)).strip()
    assert params("cir_cross_attention_folded_long_wide") == params("cir_cross_attention_folded_long")
    so = lib.load()
    fn = so.cir_cross_attention_folded_long_wide
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(so.cir_cross_attention_folded_long.argtypes) and len(fn.argtypes) == len(NAMES)
    assert lib.SIGNATURES["cir_cross_attention_folded_long_wide"] == lib.SIGNATURES["cir_cross_attention_folded_long"]
    assert so.cir_version() == 15
    for name in ("q", "x", "wkt", "wvp", "bv", "out"):
        assert _call(fn, **{name: None}) == EINVAL
    assert _call(fn, T=0) == EINVAL and _call(fn, L=0) == EINVAL and _call(fn, N=0) == EINVAL
    assert _call(fn, l=32) == ESHAPE and _call(fn, l=65) == ESHAPE and _call(fn, n=224) == ESHAPE and _call(fn, n=609) == ESHAPE
    assert _call(fn, l=16, n=197) == ESHAPE and _call(fn, l=40, n=197) == ESHAPE
    assert _call(fn, D=512) == ESHAPE and _call(fn, H=8) == ESHAPE
    assert _call(fn, key_mask=P, mask_stride=576) == ESHAPE
    for l, n in ((33, 225), (33, 608), (64, 225), (64, 608), (40, 577)):
        assert _call(fn, l=l, n=n, dtype=F32) == EDTYPE and _call(fn, l=l, n=n, dtype=7) == EDTYPE, (l, n)
        assert _call(fn, l=l, n=n, out=P + 4) == EALIGN and _call(fn, l=l, n=n, q=P + 2) == EALIGN, (l, n)
        assert _call(fn, l=l, n=n, key_mask=P, mask_stride=n - 1) == ESHAPE
    # the shape refusal comes before the dtype's, as for the siblings
    assert _call(fn, l=32, dtype=F32) == ESHAPE and _call(fn, n=224, dtype=F32) == ESHAPE


def test_neighbours_keep_their_limits():
    from candidate_reranking_cir_amd import lib
    so = lib.load()
    assert _call(so.cir_cross_attention_folded_long, l=40, n=225) == ESHAPE and _call(so.cir_cross_attention_folded_long, l=40, n=577) == ESHAPE
    assert _call(so.cir_cross_attention_folded_long, l=64, n=224, dtype=F32) == EDTYPE
    assert _call(so.cir_cross_attention_folded, l=33, n=577) == ESHAPE and _call(so.cir_cross_attention_folded, l=32, n=608, dtype=F32) == EDTYPE
    assert _call(so.cir_cross_attention_folded_short, l=17, n=577) == ESHAPE and _call(so.cir_cross_attention_folded_short, l=1, n=1, dtype=F32) == EDTYPE


# ------------------------------------------------------------------------------------------------ engine plan and dispatch
LAYERS = 4           # fusion layers 0 .. 2 run per-token cross-attention, the last one the CLS rows only (as tests/test_fold_long_cpu.py)


class WideStub(StubOps):
    def cross_attention_folded_long_wide(self, q, x, wkt, wvp, bv, out, l, scale, heads=12, mask=None):
        args = dict(locals()); del args["self"]
        self.calls.append(("folded_long_wide", l, x.shape[1], mask is not None))
        return self._record("cross_attention_folded_long_wide", args, out)


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


def _paths(engine, l, n, masked=False, bank=None):
    p = engine.plan(l, n, D, masked, bank)
    return [lp.cross for lp in p.layers[:-1]], p.fallback


def test_plan_with_and_without_the_switch(engine):
    assert engine.fold_long_wide is False and engine.fold_long is False and engine.fold_cross_kv
    cases = [(l, n, m) for l in (1, 16, 17, 32, 33, 40, 48, 49, 64, 65) for n in (1, 197, 224, 225, 300, 577, 608, 609) for m in (False, True)]
    try:
        # off: (40, 300) and (40, 577) are projected and counted, also with `fold_long` on; no plan names the new path
        for long_on in (False, True):
            engine.fold_long = long_on
            for n in (300, 577):
                assert _paths(engine, 40, n) == (["projected"] * (LAYERS - 1), True), (long_on, n)
            assert all(lp.cross != "fold_long_wide" for c in cases for lp in engine.plan(c[0], c[1], D, c[2]).layers)
        engine.fold_long = False
        off = {c: engine.plan(c[0], c[1], D, c[2]) for c in cases}
        # on: the new path for 33-64 tokens x 225-608 keys, masked or not, not counted - and the off plan everywhere else
        engine.fold_long_wide = True
        for l in (33, 48, 49, 64):
            for n in (225, 577, 608):
                for masked in (False, True):
                    assert _paths(engine, l, n, masked) == (["fold_long_wide"] * (LAYERS - 1), False), (l, n, masked)
        for (l, n, m), p in off.items():
            on = engine.plan(l, n, D, m)
            if 33 <= l <= 64 and 225 <= n <= 608:
                assert on != p and on.layers[-1] == p.layers[-1]
            else:
                assert on == p, (l, n, m)
        # (40, 197) follows `fold_long` only
        assert _paths(engine, 40, 197) == (["projected"] * (LAYERS - 1), True)
        engine.fold_long = True
        assert _paths(engine, 40, 197) == (["fold_long"] * (LAYERS - 1), False) and _paths(engine, 40, 577) == (["fold_long_wide"] * (LAYERS - 1), False)
        engine.fold_long = False
        assert _paths(engine, 32, 577) == (["fold32"] * (LAYERS - 1), False)
        assert _paths(engine, 65, 577) == (["projected"] * (LAYERS - 1), True)
        assert _paths(engine, 40, 609) == (["projected"] * (LAYERS - 1), True)
        bank = (False,) * (LAYERS - 1) + (True,)                          # a K/V bank keeps its own path
        assert _paths(engine, 40, 577, bank=bank) == (["bank"] * (LAYERS - 1), False)
        assert engine.plan(40, 577, 512, False).layers[0].cross == "projected"        # candidate tokens of another width: untouched
        engine.fold_cross_kv = False                                      # without the fold at all (the exact mode) the switch is inert
        assert _paths(engine, 40, 577) == (["projected"] * (LAYERS - 1), False)
    finally:
        engine.fold_cross_kv, engine.fold_long, engine.fold_long_wide = True, False, False


def test_engine_dispatch_at_577_keys(engine, monkeypatch):
    def run(l, n, masked=False, stub_cls=WideStub):
        stub, _, w = run_forward(engine, monkeypatch, l, n, 1, 2, masked, stub=stub_cls(engine))
        kv = [c for c in stub.calls if c[0] == "gemm" and c[1] == (2 * n, D) and c[2] == (4 * D, D)]
        return [c for c in stub.calls if c[0].startswith("folded")], kv, [x for x in w if "projected" in str(x.message)]
    try:
        # off: the parent's calls on the parent's stub, which has no such op to call; counted
        engine.fold_fallbacks = 0
        folds, kv, warned = run(40, 577, stub_cls=StubOps)
        assert not folds and len(kv) == LAYERS - 1 and engine.fold_fallbacks == 1 and len(warned) == 1
        engine.fold_long_wide = True
        for l, n, masked in ((33, 577, False), (40, 257, False), (64, 608, False), (40, 577, True)):
            folds, kv, warned = run(l, n, masked)
            assert folds == [("folded_long_wide", l, n, masked)] * (LAYERS - 1), (l, n, masked)
            assert len(kv) == int(masked) and not warned and engine.fold_fallbacks == 1      # (masked: the CLS-only last layer projects, as before)
        folds, kv, _ = run(40, 197)                                       # <= 224 keys: not this switch's
        assert not folds and len(kv) == LAYERS - 1 and engine.fold_fallbacks == 2
        folds, kv, _ = run(32, 577)
        assert folds == [("folded", 32, 577, False)] * (LAYERS - 1) and not kv
    finally:
        engine.fold_long_wide, engine.fold_fallbacks = False, 0


def test_model_switch_is_off_by_default_and_survives_repacks():
    from candidate_reranking_cir_amd import synthetic
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    g = BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, encoder_width=128)
    v = VitGeometry(image_size=64, width=128, depth=1, num_heads=2)
    m = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    assert m.long_caption_fold_wide is False
    assert m.set_long_caption_fold_wide() is m and m.long_caption_fold_wide is True
    assert m.set_long_caption_fold_wide(False).long_caption_fold_wide is False
    m.set_long_caption_fold_wide(True)
    assert m.long_caption_fold is False                               # a second switch: the 224-key one does not move with it
    sd = {k: p.detach() for k, p in m.state_dict().items()}
    first = m._text_engine(sd)
    assert first.fold_long_wide is True and first.fold_long is False and first.fold_short is False
    for mode in ("bf16", "f16"):                                      # repacks: the next engine is packed anew and gets the model's setting
        m.set_precision(mode)
        assert m.long_caption_fold_wide is True and m._text_engine(sd).fold_long_wide is True
    m.load_state_dict(m.state_dict())
    assert m.long_caption_fold_wide is True and m._text_engine(sd).fold_long_wide is True
    m.set_long_caption_fold_wide(False)
    assert m._text_engine(sd).fold_long_wide is False
