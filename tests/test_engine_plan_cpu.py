"""NlvrEngine's launch plan without a GPU: `plan` as a table of cases, and the soundness of `graph_key` - two calls with the same key issue
the same launches - with `ops` replaced by the recording stubs of tests/engine_stub.py."""
import itertools

import pytest
import torch

from tests.engine_stub import StubOps, run_forward

F16, F32 = torch.float16, torch.float32
SWITCHES = ("trim_last", "fold_cls_kv", "fold_cross_kv", "fold_long", "kv_chunk", "stream32_from")


def _engine(layers=4, dtype=F16, **kw):
    from candidate_reranking_cir_amd import engine as E
    from candidate_reranking_cir_amd import weights
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    geo = BertGeometry(num_hidden_layers=layers, merge_mlp_from_layer=2)
    vit = VitGeometry(image_size=64, patch_size=16, width=768, depth=1, num_heads=12)
    geo.encoder_width = vit.width
    return E.NlvrEngine(weights.synth_state_dict(weights.nlvr_param_spec(geo, vit), 1), geo, dtype, torch.device("cpu"), **kw)


@pytest.fixture(scope="module")
def packed():
    return _engine()


@pytest.fixture
def eng(packed):
    """the 4-layer 768-wide fp16 engine, its live switches restored after the test"""
    saved = {k: getattr(packed, k) for k in SWITCHES + ("fold_fallbacks",)}
    yield packed
    for k, v in saved.items():
        setattr(packed, k, v)


def _paths(e, l, n, dv=768, masked=False, bank=None):
    p = e.plan(l, n, dv, masked, bank)
    assert hash(p) == hash(e.plan(l, n, dv, masked, bank)) and p == e.plan(l, n, dv, masked, bank)      # hashable, a pure function
    assert p.kv_chunk == e.kv_chunk
    return [x.cross for x in p.layers], [x.cls_only for x in p.layers], p.fallback


def test_plan_defaults(eng):
    for n in (197, 577, 608):
        assert _paths(eng, 32, n) == (["fold32"] * 3 + ["cls_fold"], [False] * 3 + [True], False)
    assert _paths(eng, 32, 609) == (["projected"] * 3 + ["cls_fold"], [False] * 3 + [True], False)       # too many keys: projected, not counted
    assert _paths(eng, 1, 1)[0] == ["fold32"] * 3 + ["cls_fold"]
    p = eng.plan(32, 197, 768, False)
    assert all(x.sdt == F16 and x.sdt_out == F16 for x in p.layers)


def test_plan_long_captions(eng):
    assert eng.fold_long is False
    assert _paths(eng, 40, 197) == (["projected"] * 3 + ["cls_fold"], [False] * 3 + [True], True)        # switch off: projected, counted
    eng.fold_long = True
    for l, n in ((33, 197), (40, 197), (64, 224), (40, 1)):
        assert _paths(eng, l, n) == (["fold_long"] * 3 + ["cls_fold"], [False] * 3 + [True], False)
    assert _paths(eng, 40, 225) == (["projected"] * 3 + ["cls_fold"], [False] * 3 + [True], True)        # past the long fold's keys: counted
    assert _paths(eng, 32, 197)[0] == ["fold32"] * 3 + ["cls_fold"]                                      # 32 tokens: the short fold, whatever the switch
    for on in (False, True):
        eng.fold_long = on
        assert _paths(eng, 65, 197) == (["projected"] * 3 + ["cls_fold"], [False] * 3 + [True], True)


def test_plan_masks_and_switches(eng):
    assert _paths(eng, 32, 197, masked=True) == (["fold32"] * 3 + ["projected"], [False] * 3 + [True], False)   # the CLS fold takes no key mask
    assert _paths(eng, 32, 197, dv=512) == (["projected"] * 3 + ["cls_fold"], [False] * 3 + [True], False)
    eng.trim_last = False
    assert _paths(eng, 32, 197) == (["fold32"] * 4, [False] * 4, False)
    eng.trim_last, eng.fold_cls_kv = True, False
    assert _paths(eng, 32, 197) == (["fold32"] * 3 + ["projected"], [False] * 3 + [True], False)
    eng.fold_cls_kv, eng.fold_cross_kv = True, False
    assert _paths(eng, 32, 197) == (["projected"] * 3 + ["cls_fold"], [False] * 3 + [True], False)
    assert _paths(eng, 40, 197)[2] is False                                                             # no fold to fall back from: not counted
    eng.fold_cross_kv, eng.kv_chunk, eng.stream32_from = True, 2, 2
    p = eng.plan(32, 197, 768, False)
    assert p.kv_chunk == 2 and [x.sdt for x in p.layers] == [F16, F16, F32, F32] and [x.sdt_out for x in p.layers] == [F16, F32, F32, F32]


def test_plan_with_a_kv_bank(eng):
    folded, full = (False, False, False, True), (False,) * 4
    for l in (32, 40):
        assert _paths(eng, l, 197, bank=folded) == (["bank"] * 3 + ["cls_fold"], [False] * 3 + [True], False)
        assert _paths(eng, l, 197, bank=full) == (["bank"] * 4, [False] * 3 + [True], False)
    eng.fold_cls_kv = False
    assert _paths(eng, 32, 197, bank=full)[0] == ["bank"] * 4
    with pytest.raises(ValueError, match="built with the last layer folded"):
        eng.plan(32, 197, 768, False, folded)
    eng.fold_cls_kv = True
    with pytest.raises(ValueError, match="built with the last layer folded"):
        eng.plan(32, 197, 768, True, folded)                                                            # masked: the last layer needs its K|V


def test_bank_errors_come_before_the_first_launch(eng, monkeypatch):
    from candidate_reranking_cir_amd import engine as E
    second = _engine()                                                                                  # (packed with the real `ops`)
    monkeypatch.setattr(E, "ops", StubOps())
    bank, other = (e.build_kv_bank(torch.zeros((4, 5, 768), dtype=F16)) for e in (eng, second))
    assert [kv is None for kv in bank] == [False, False, False, True]
    rows = torch.tensor([0, 3])
    stub, out, _ = run_forward(eng, monkeypatch, 32, 5, kv_bank=bank, cand_rows=rows)
    assert [c for c in stub.calls if c[0] == "attention" and c[2][0] == 4]                               # (the bank is what the attention reads)
    eng.fold_cls_kv = False
    stub = StubOps(eng)
    with pytest.raises(ValueError, match="built with the last layer folded"):
        run_forward(eng, monkeypatch, 32, 5, stub=stub, kv_bank=bank, cand_rows=rows)
    assert stub.trace == []
    eng.fold_cls_kv = True
    assert other.engine() is second
    bank.engine = None
    for foreign in (other, bank):                                                                       # another engine's bank, one without an engine
        with pytest.raises(RuntimeError, match="not built by this engine"):
            run_forward(eng, monkeypatch, 32, 5, stub=stub, kv_bank=foreign, cand_rows=rows)
    with pytest.raises(RuntimeError, match="not built by this engine"):
        run_forward(eng, monkeypatch, 32, 5, stub=stub, kv_bank=list(bank), cand_rows=rows)
    assert stub.trace == []


def test_plan_of_other_geometries():
    one = _engine(layers=1)
    assert one.cls_fold is None and _paths(one, 32, 197) == (["fold32"], [False], False)                # one layer: no CLS-only layer, nothing counted
    assert _paths(one, 40, 197) == (["projected"], [False], False)
    exact = _engine(dtype=F32, stream_dtype=F32, fold_merge=False)
    assert not exact.fold_cross_kv and not exact.fold_cls_kv
    for l in (32, 40):
        assert _paths(exact, l, 197) == (["projected"] * 4, [False] * 3 + [True], False)                # fp32: no fold, the reference's order
    exact.stream32_from = 2
    assert all(x.sdt == F32 and x.sdt_out == F32 for x in exact.plan(32, 197, 768, False).layers)


def _trace(e, monkeypatch, l, n):
    stub, _, _ = run_forward(e, monkeypatch, l, n, q_n=2, k=3)
    return stub.trace


def test_equal_graph_keys_mean_equal_launches(eng, monkeypatch):
    """Every combination of the live switches at a short and a long caption: 128 stubbed forwards, grouped by `graph_key`."""
    seen, forwards = {}, 0
    for l, n in ((32, 197), (40, 197)):
        for values in itertools.product((True, False), (True, False), (True, False), (False, True), (0, 2), (None, 2)):
            for k, v in zip(SWITCHES, values):
                setattr(eng, k, v)
            key = eng.graph_key((2, l), (6, n, 768), F16)
            assert key[:3] == ((2, l), (6, n, 768), F16) and key[3] == eng.plan(l, n, 768, False)
            trace = _trace(eng, monkeypatch, l, n)
            forwards += 1
            assert seen.setdefault(key, trace) == trace, (l, n, values)
    assert forwards == 128 and 1 < len(seen) <= 128


@pytest.mark.parametrize("switch,value,l", [("trim_last", False, 32), ("fold_cls_kv", False, 32), ("fold_cross_kv", False, 32), ("fold_long", True, 40),
                                            ("kv_chunk", 2, 40), ("stream32_from", 2, 32)])
def test_a_switch_that_changes_the_launches_changes_the_key(eng, monkeypatch, switch, value, l):
    key, trace = eng.graph_key((2, l), (6, 197, 768), F16), _trace(eng, monkeypatch, l, 197)
    setattr(eng, switch, value)
    assert _trace(eng, monkeypatch, l, 197) != trace                                                    # (the shape is one where the switch matters)
    assert eng.graph_key((2, l), (6, 197, 768), F16) != key
