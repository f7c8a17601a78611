"""Packed weight copies follow every write to the parameters: a matrix of mutation x consumer.

The kernels never read the fp32 `nn.Parameter`s: they run on copies packed from them - the inference engines (16-bit weights, split8
rows, LayerNorm-folded packs, cross-attention fold packs, the merge-layer fold) with their captured HIP graphs, K/V banks, and the
trainers' 16-bit slabs (`train._Slab`: flat16 and its transposed twin).  Each cell mutates a model's weights by a lot, then compares
a consumer BIT FOR BIT with a fresh model of the same class, geometry and precision loaded with the mutated state dict: a stale or
half-stale pack misses by orders of magnitude, not by a tolerance.  Gradients, whose weight-gradient kernels may add in another order,
are held to 1e-5 relative per tensor.  Sequences: S1 pack, mutate, call; S2 training forward / backward, eval call, mutate, eval call;
S3 `train.AdamW` step, mutate, training forward / backward."""
import copy
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic, train_ops as T
from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
from candidate_reranking_cir_amd.train import AdamW, _Lin, fusion_train
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GRAD_REL = 1e-5
TEXT = ("text_encoder.", "cls_head.")


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    z, g, v, sd2, sd1 = H.tiny_setup()
    v = dataclasses.replace(v, drop_path_rate=0.0)                   # deterministic ViT training forward (fresh model: other step count)
    other2, other1 = H.state_dicts(g, v, int(z["seed"]) + 7, str(z["profile"]))
    return dict(g=g, v=v, sd2=sd2, sd1=sd1, other2=other2, other1=other1)


@pytest.fixture(scope="module")
def wide():
    """768 wide, 3 layers: the text32 mode's split8 rows (at hidden 128 it falls back to three products)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g, v = BertGeometry(num_hidden_layers=3), VitGeometry(image_size=64, patch_size=16, width=768, depth=1, num_heads=12)
    g.encoder_width = v.width
    torch.manual_seed(0)
    sd = BLIP_NLVR(g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).state_dict()
    torch.manual_seed(1)
    other = BLIP_NLVR(g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).state_dict()
    return dict(g=g, v=v, sd2=sd, other2=other)


def _nlvr(geo, sd, mode):
    m = BLIP_NLVR(med_config=copy.deepcopy(geo["g"]), vit_geometry=geo["v"], tokenizer=synthetic.HashTokenizer())
    m.load_state_dict(sd)
    return m.to(DEV).float().eval().set_precision(mode) or m


def _fresh(m, geo, mode):
    return _nlvr(geo, copy.deepcopy(m.state_dict()), mode)


def _inputs(geo, seed=3, q_n=2, k=3):
    g, v = geo["g"], geo["v"]
    gen = torch.Generator().manual_seed(seed)
    l = 9
    z = torch.randn((q_n, l, g.hidden_size), generator=gen).to(DEV)
    ids = torch.randint(1000, 20000, (q_n, l), generator=gen).to(DEV)
    mask = torch.ones_like(ids)
    mask[0, l - 2:] = 0
    cand = (torch.randn((q_n * k, v.num_tokens, v.width), generator=gen) * 0.5).to(DEV)
    qidx = torch.arange(q_n, device=DEV).repeat_interleave(k)
    images = torch.randn((2, 3, v.image_size, v.image_size), generator=gen).to(DEV)
    return dict(z=z, ids=ids, mask=mask, cand=cand, qidx=qidx, images=images)


def _param(m, name):
    return dict(m.named_parameters())[name]


def _set_grads(m, prefixes):
    gen = torch.Generator(device=DEV).manual_seed(5)
    for n, p in m.named_parameters():
        p.grad = torch.randn(p.shape, generator=gen, device=DEV) if n.startswith(prefixes) else None


def _torch_opt(kind):
    def run(m, geo):
        ps = [p for n, p in m.named_parameters() if p.requires_grad]
        if not any(p.grad is not None for p in ps):
            _set_grads(m, ("",))
        if kind == "scaler":
            opt = torch.optim.AdamW(ps, lr=0.05)
            scaler = torch.amp.GradScaler("cuda", init_scale=1.0)
            scaler.scale(torch.ones((), device=DEV))
            scaler.step(opt)
            scaler.update()
        else:
            torch.optim.AdamW(ps, lr=0.05, **{kind: True} if kind != "loop" else {"foreach": False}).step()
    return run


def _cir_adamw(with_model):
    def run(m, geo):
        ps = [p for p in m.parameters() if p.requires_grad]
        if not any(p.grad is not None for p in ps):
            _set_grads(m, ("",))
        AdamW(ps, lr=0.05, weight_decay=0.0, model=m if with_model else None).step()
    return run


def _load(sub=None):
    def run(m, geo):
        other = geo["other2"]
        if sub is None:
            m.load_state_dict(other)
        else:
            getattr(m, sub).load_state_dict({k[len(sub) + 1:]: t for k, t in other.items() if k.startswith(sub + ".")})
    return run


def _edit(name):
    def run(m, geo):
        with torch.no_grad():
            p = _param(m, name.format(**_names(geo)))
            p.copy_(2 * p + 0.1)
    return run


def _data_edit(m, geo):
    p = _param(m, "text_encoder.encoder.layer.0.crossattention.self1.value.weight")
    p.data.copy_(2 * p.data + 0.1)
    m.invalidate_packed_weights()


def _half_float(m, geo):
    m.half().float()


def _names(geo):
    n = geo["g"].num_hidden_layers
    return dict(last=n - 1, merge=n - 2 if n > 2 else n - 1)


MUTATIONS = {
    "cir_adamw": _cir_adamw(False), "cir_adamw_model": _cir_adamw(True),
    "torch_loop": _torch_opt("loop"), "torch_foreach": _torch_opt("foreach"), "torch_fused": _torch_opt("fused"), "gradscaler": _torch_opt("scaler"),
    "load": _load(), "load_text": _load("text_encoder"), "load_vit": _load("visual_encoder"), "load_cls": _load("cls_head"),
    "edit_cross_key": _edit("text_encoder.encoder.layer.{last}.crossattention.self0.key.weight"),
    "edit_cross_value": _edit("text_encoder.encoder.layer.0.crossattention.self1.value.weight"),
    "edit_merge": _edit("text_encoder.encoder.layer.{merge}.crossattention.output.merge_layer.weight"),
    "edit_norm1": _edit("visual_encoder.blocks.0.norm1.weight"),
    "edit_fc1": _edit("visual_encoder.blocks.0.mlp.fc1.weight"),
    "edit_cls0": _edit("cls_head.0.weight"),
    "edit_word": _edit("text_encoder.embeddings.word_embeddings.weight"),
    "data_invalidate": _data_edit,
    "half_float": _half_float,
}
SIDE = ["load", "load_text", "edit_cross_key", "torch_foreach"]       # text32 / exact rows
GRAPH = ["load", "edit_cross_value", "edit_merge", "torch_foreach", "torch_fused"]


def _score(m, x, bank=None):
    if bank is not None:
        return m.score(x["z"], x["ids"], x["mask"], None, x["qidx"], kv_bank=bank, cand_rows=torch.arange(x["cand"].shape[0], device=DEV))
    return m.score(x["z"], x["ids"], x["mask"], x["cand"], x["qidx"])


def _check_eval(m, geo, mode, x, graphs=False):
    f = _fresh(m, geo, mode)
    if graphs:
        f.enable_graphs(64)
    assert torch.equal(_score(m, x), _score(f, x)), "score: a packed copy of the text side is stale"
    assert torch.equal(m.img_embed(x["images"]), f.img_embed(x["images"])), "img_embed: the packed ViT is stale"
    assert torch.equal(m.img_txt_fusion(x["z"], x["cand"][:2], {"input_ids": x["ids"], "attention_mask": x["mask"]}),
                       f.img_txt_fusion(x["z"], x["cand"][:2], {"input_ids": x["ids"], "attention_mask": x["mask"]}))
    return f


# ------------------------------------------------------------------------------------------------ S1: pack, mutate, call
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_s1_tiny_f16(tiny, mut):
    m = _nlvr(tiny, tiny["sd2"], "f16")
    x = _inputs(tiny)
    _score(m, x), m.img_embed(x["images"])                           # pack both sides
    MUTATIONS[mut](m, tiny)
    _check_eval(m, tiny, "f16", x)


@pytest.mark.parametrize("mode", ["text32", "exact"])
@pytest.mark.parametrize("mut", SIDE)
def test_s1_wide_text_side(wide, mode, mut):
    m = _nlvr(wide, wide["sd2"], mode)
    if mode == "text32":
        assert m.engines()[1].split == 8                              # the split8 weight rows are what is checked
    x = _inputs(wide, q_n=1, k=2)
    _score(m, x)
    MUTATIONS[mut](m, wide)
    f = _fresh(m, wide, mode)
    assert torch.equal(_score(m, x), _score(f, x))


@pytest.mark.parametrize("mut", GRAPH)
def test_s1_graphs_and_bank(tiny, mut):
    """Captured HIP graphs follow a repacked engine; a K/V bank built before the write is refused (never silently used) and a rebuilt one
    scores like the fresh model's."""
    m = _nlvr(tiny, tiny["sd2"], "f16").enable_graphs(64)
    x = _inputs(tiny)
    bank = m.build_kv_bank(x["cand"])
    _score(m, x), _score(m, x, bank)
    MUTATIONS[mut](m, tiny)
    f = _fresh(m, tiny, "f16").enable_graphs(64)
    assert torch.equal(_score(m, x), _score(f, x))
    with pytest.raises(RuntimeError, match="kv_bank"):
        _score(m, x, bank)
    assert torch.equal(_score(m, x, m.build_kv_bank(x["cand"])), _score(f, x, f.build_kv_bank(x["cand"])))


@pytest.mark.parametrize("mut", ["load", "load_text", "edit_word"])
@pytest.mark.parametrize("mode", ["f16", "text32"])
def test_s1_stage1_z_t(tiny, wide, mode, mut):
    geo = tiny if mode == "f16" else wide
    g, v = geo["g"], geo["v"]

    def make(sd):
        m = BLIP_Retrieval(med_config=copy.deepcopy(g), vit_geometry=v, tokenizer=synthetic.HashTokenizer())
        m.load_state_dict(sd, strict=False)
        return m.to(DEV).float().eval().set_precision(mode) or m
    base = BLIP_Retrieval(med_config=copy.deepcopy(g), vit_geometry=v).state_dict() if mode == "text32" else geo["sd1"]
    m = make(base)
    if mode == "text32":
        assert m.engines()[0].split == 8
    other = {k: t * 1.5 + 0.01 if t.is_floating_point() else t for k, t in base.items()}
    x = _inputs(geo, q_n=2)
    tok = x["cand"][:2]
    m.z_t(tok, x["ids"], x["mask"])
    if mut == "load":
        m.load_state_dict(other, strict=False)
    elif mut == "load_text":
        m.text_encoder.load_state_dict({k[len("text_encoder."):]: t for k, t in other.items() if k.startswith("text_encoder.")})
    else:
        with torch.no_grad():
            p = _param(m, "text_encoder.embeddings.word_embeddings.weight")
            p.copy_(2 * p + 0.1)
    f = make(copy.deepcopy(m.state_dict()))
    assert torch.equal(m.z_t(tok, x["ids"], x["mask"]).last_hidden_state, f.z_t(tok, x["ids"], x["mask"]).last_hidden_state)


# ------------------------------------------------------------------------------------------------ training consumers
def _train_step(m, x, img_tune=False):
    """Training forward (dropout 0) + backward of `img_txt_fusion`; returns the logits."""
    m.train()
    feats = m.img_embed(x["images"]) if img_tune else x["cand"][:2]
    logits = fusion_train(m, x["z"], feats, x["ids"], x["mask"], 0.0, 0.0)
    F.cross_entropy(logits, torch.arange(2, device=DEV)).backward()
    m.eval()
    return logits.detach()


def _check_slab(tr):
    s = tr.slab
    assert torch.equal(s.flat16, s.flat32.to(s.dtype)), "slab.flat16 is not the 16-bit copy of the parameters"
    lins = [l for d in getattr(tr, "layers", getattr(tr, "blocks", [])) for l in d.values() if isinstance(l, _Lin)]
    lins += [l for l in (getattr(tr, "c0", None), getattr(tr, "c2", None), getattr(tr, "pe", None)) if l is not None]
    assert lins
    for l in lins:
        assert torch.equal(l.w16t, l.w16.t()), "slab.flat16t is not the transpose of flat16"


def _check_training(m, f, x, img_tune):
    for p in list(m.parameters()) + list(f.parameters()):
        p.grad = None
    la, lb = _train_step(m, x, img_tune), _train_step(f, x, img_tune)
    _check_slab(m._trainer)
    if img_tune:
        _check_slab(m._vit_trainer)
    assert torch.equal(la, lb), "training-forward logits differ from the fresh model's"
    pf = dict(f.named_parameters())
    worst = 0.0
    for n, p in m.named_parameters():
        if p.grad is None:
            continue
        q = pf[n].grad
        worst = max(worst, ((p.grad - q).norm() / q.norm().clamp_min(1e-30)).item())
    print(f"\n[gradients against the fresh model] worst relative error {worst:.2e} (bound {GRAD_REL:.0e})")
    assert worst <= GRAD_REL


@pytest.mark.parametrize("mut", list(MUTATIONS))
@pytest.mark.parametrize("img_tune", [False, True], ids=["nlvr", "vit"])
def test_s3_trainer_after_cir_step(tiny, mut, img_tune):
    """B1: after one `train.AdamW` step (which writes the 16-bit slab along), any later write reaches the next training step."""
    m = _nlvr(tiny, tiny["sd2"], "f16")
    if not img_tune:
        for n, p in m.named_parameters():
            p.requires_grad_(n.startswith(TEXT))
    x = _inputs(tiny)
    _train_step(m, x, img_tune)
    AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.0, model=m).step()
    MUTATIONS[mut](m, tiny)
    f = _fresh(m, tiny, "f16")
    for n, p in f.named_parameters():
        p.requires_grad_(_param(m, n).requires_grad)
    _check_training(m, f, x, img_tune)


@pytest.mark.parametrize("mut", ["torch_loop", "torch_foreach", "torch_fused", "gradscaler", "load", "edit_cls0", "edit_norm1"])
def test_s2_eval_between_backward_and_mutation(tiny, mut):
    """B3: training forward, backward, an eval call (packs), then a write: the next eval call scores with the written weights."""
    m = _nlvr(tiny, tiny["sd2"], "f16")
    x = _inputs(tiny)
    _train_step(m, x, img_tune=True)
    _score(m, x), m.img_embed(x["images"])
    MUTATIONS[mut](m, tiny)
    _check_eval(m, tiny, "f16", x)


def test_s2_strengthened_staleness(tiny):
    """test_train_gpu's engine-staleness check as an equality: eval between backward and `train.AdamW.step`, then the eval call equals a fresh
    model loaded with the stepped weights."""
    m = _nlvr(tiny, tiny["sd2"], "f16")
    x = _inputs(tiny)
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.0)
    _train_step(m, x, img_tune=True)
    before = _score(m, x).clone()
    opt.step()
    f = _check_eval(m, tiny, "f16", x)
    assert not torch.equal(before, _score(f, x))


# ------------------------------------------------------------------------------------------------ B2: no cast pass after our own step
def test_slab_cast_only_when_the_parameters_were_written(tiny, monkeypatch):
    """With two slabs (text side and fine-tuned ViT): after a `train.AdamW` step the next training step casts neither (the step wrote both
    16-bit copies); after a torch.optim step it casts each exactly once."""
    m = _nlvr(tiny, tiny["sd2"], "f16")
    x = _inputs(tiny)
    _train_step(m, x, img_tune=True)
    slabs = [m._trainer.slab, m._vit_trainer.slab]
    casts = []
    real = T.eltwise

    def spy(t, mode, *a, **k):
        if mode == T.MODE_SCALE:
            casts.extend(i for i, s in enumerate(slabs) if t.data_ptr() == s.flat32.data_ptr() and t.numel() == s.flat32.numel())
        return real(t, mode, *a, **k)
    monkeypatch.setattr(T, "eltwise", spy)
    AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.0, model=m).step()
    _train_step(m, x, img_tune=True)
    assert casts == [], f"cast passes after a cir step: {casts}"
    torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3).step()
    _train_step(m, x, img_tune=True)
    assert sorted(casts) == [0, 1], f"cast passes after a torch.optim step: {casts}"
    assert [m._trainer.slab, m._vit_trainer.slab] == slabs
