"""The staleness key of the packed weights (`_EngineHost.weights_key`) on CPU tensors: every torch-side write to the parameters that the
packed copies (inference engines, captured graphs, K/V banks, the trainers' 16-bit slabs) must follow moves it, for the part it touched.
The GPU side - that the packs really are rebuilt and equal a fresh model's - is tests/test_weight_coherence_gpu.py."""
import pytest
import torch

from candidate_reranking_cir_amd import synthetic
from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
from tests import helpers as H

PARTS = ("text", "vit", "all")


@pytest.fixture(scope="module")
def tiny():
    z, g, v, sd2, sd1 = H.tiny_setup()
    other = H.state_dicts(g, v, int(z["seed"]) + 1, str(z["profile"]))
    return g, v, sd2, other[0]


def _model(tiny):
    g, v, sd2, _ = tiny
    m = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m.load_state_dict(sd2)
    return m


def _keys(m):
    return {p: m.weights_key(p) for p in PARTS}


def _moved(m, before):
    after = _keys(m)
    return {p for p in PARTS if after[p] != before[p]}


def _param(m, name):
    return dict(m.named_parameters())[name]


def _grads(m, prefix):
    for n, p in m.named_parameters():
        p.grad = torch.full_like(p, 1e-2) if n.startswith(prefix) else None


@pytest.mark.parametrize("name, part", [("text_encoder.encoder.layer.0.crossattention.self0.key.weight", "text"),
                                        ("cls_head.0.weight", "text"),
                                        ("text_encoder.embeddings.word_embeddings.weight", "text"),
                                        ("visual_encoder.blocks.0.norm1.weight", "vit"),
                                        ("visual_encoder.blocks.0.mlp.fc1.weight", "vit")])
def test_inplace_edit_moves_its_part(tiny, name, part):
    m = _model(tiny)
    before = _keys(m)
    with torch.no_grad():
        p = _param(m, name)
        p.copy_(2 * p + 0.1)
    assert _moved(m, before) == {part, "all"}


@pytest.mark.parametrize("sub, part", [("text_encoder", "text"), ("visual_encoder", "vit"), ("cls_head", "text")])
def test_submodule_load_moves_its_part(tiny, sub, part):
    m = _model(tiny)
    other = {k[len(sub) + 1:]: t for k, t in tiny[3].items() if k.startswith(sub + ".")}
    before = _keys(m)
    getattr(m, sub).load_state_dict(other)
    assert part in _moved(m, before) and "all" in _moved(m, before)


def test_whole_load_and_assign_load_move_every_part(tiny):
    m = _model(tiny)
    before = _keys(m)
    m.load_state_dict(tiny[3])
    assert _moved(m, before) == set(PARTS)
    # assign=True replaces the Parameter objects of the submodule: the key follows the NEW ones afterwards
    sub = {k[len("cls_head."):]: t.clone() for k, t in tiny[2].items() if k.startswith("cls_head.")}
    m.cls_head.load_state_dict(sub, assign=True)
    before = _keys(m)
    with torch.no_grad():
        m.cls_head.get_submodule("0").weight.mul_(3.0)
    assert "text" in _moved(m, before)


@pytest.mark.parametrize("kind", ["foreach=False", "foreach=True", "fused=True", "GradScaler"])
def test_torch_optimizer_steps_move_the_key(tiny, kind):
    m = _model(tiny)
    params = [p for n, p in m.named_parameters() if n.startswith(("text_encoder.", "cls_head."))]
    _grads(m, ("text_encoder.", "cls_head."))
    before = _keys(m)
    if kind == "GradScaler":
        opt = torch.optim.AdamW(params, lr=1e-3)
        scaler = torch.amp.GradScaler("cpu", init_scale=1.0)
        scaler.scale(torch.ones(()))                          # (what scaler.scale(loss).backward() leaves: the scale exists)
        scaler.step(opt)
        scaler.update()
    else:
        opt = torch.optim.AdamW(params, lr=1e-3, **{kind.split("=")[0]: True if kind.endswith("True") else False})
        opt.step()
    assert "text" in _moved(m, before) and "all" in _moved(m, before)


def test_data_writes_need_the_documented_invalidation(tiny):
    """`.data` is a tensor with a version counter of its own: writes through it are invisible until `invalidate_packed_weights()`."""
    m = _model(tiny)
    before = _keys(m)
    _param(m, "text_encoder.encoder.layer.6.crossattention.output.merge_layer.weight").data.mul_(2.0)
    assert _moved(m, before) == set()
    m.invalidate_packed_weights()
    assert _moved(m, before) == set(PARTS)


def test_dtype_round_trip_moves_the_key(tiny):
    m = _model(tiny)
    before = _keys(m)
    m.half().float()
    assert _moved(m, before) == set(PARTS)


def test_stage1_model_key(tiny):
    g, v, _, _ = tiny
    m = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    k0 = m.weights_key()
    with torch.no_grad():
        _param(m, "text_encoder.embeddings.word_embeddings.weight").add_(1.0)
    k1 = m.weights_key()
    m.text_encoder.load_state_dict(m.text_encoder.state_dict())
    assert len({k0, k1, m.weights_key()}) == 3
