"""The deterministic training mode (train.set_deterministic) on a real MI355X, at step and loop level: with the mode on, the same
weights, inputs and dropout seed give the same logits and the same bits in every gradient - for the stage-II fusion pass (NlvrTrainer),
the stage-I pass (MedTrainer) and ViT fine-tuning (img_embed in train mode) -, and two training loops from one state dict end in the same
parameters and AdamW moments.  Against the default mode's gradients of the same seed every tensor stays within the fp32 reorder noise
tests/test_train_gpu.py::test_dropout_statistics_and_determinism allows two default backward passes (1e-4 of the tensor's norm): the
mode changes the order of the sums and nothing else.

Shapes.  Thirteen captions of 9 - 13 words tokenize to L = 15, so the text side has B L = 195 rows (stage I, and the embeddings of stage
II) and B^2 L = 2535 rows (stage II's encoder), the ViT 13 x 17 = 221: each at least three workgroups of the 32-row LayerNorm adjoints and
of the 64-row 16-bit row kernel with a ragged rest, and at least two 64-row steps plus a tail in every weight gradient (asserted below;
twelve captions would leave B L = 180 rows short of a third 64-row workgroup).
Dropout runs at the med_config probabilities (0.1 / 0.1) from `torch.manual_seed`."""
import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests.test_train_gpu import BF, HF, build, freeze_vit

pytestmark = pytest.mark.gpu
NOISE = 1e-4                        # relative norm: test_dropout_statistics_and_determinism's bound on two default backward passes
B = 13
CAPS = [synthetic.caption_text(300 + i, 9 + i % 5) for i in range(B)]


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture
def mode():
    from candidate_reranking_cir_amd import train
    assert train.deterministic() is False
    yield train.set_deterministic
    train.set_deterministic(False)


def _ragged(rows):
    """At least three workgroups of the 32- and 64-row kernels with a ragged rest; two 64-row weight-gradient steps and a tail."""
    return rows >= 3 * 64 and rows % 64 != 0 and rows % 32 != 0


def _length():
    ids, _ = H.tokenize(CAPS)
    return ids.shape[1]


def _rewind(model):
    """The fusion pass derives its dropout seeds, and the ViT pass its DropPath draw, from (the trainer's seed, its count of forward calls),
    not from torch's generator: the same seed means the same count."""
    for name in ("_trainer", "_vit_trainer"):
        tr = getattr(model, name, None)
        if tr is not None:
            tr.step_no = 0


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _check(runs_on, run_off):
    """runs_on: three (logits, grads) with the mode on; run_off: one with it off, same seed."""
    l0, g0 = runs_on[0]
    assert len(g0) > 0 and all(bool(torch.isfinite(t).all()) for t in g0.values())
    for lg, gr in runs_on[1:]:
        assert torch.equal(l0, lg)
        assert gr.keys() == g0.keys()
        diff = [n for n in g0 if not torch.equal(g0[n], gr[n])]
        assert not diff, diff
    l_off, g_off = run_off
    assert torch.equal(l0, l_off)                                   # the forward pass is the same code in both modes
    assert g_off.keys() == g0.keys()
    worst = (0.0, "")
    for n in g0:
        e = (g0[n] - g_off[n]).norm().item() / (g_off[n].norm().item() + 1e-12)
        worst = max(worst, (e, n))
        assert (g0[n] - g_off[n]).norm().item() <= NOISE * (g_off[n].norm().item() + 1e-12), (n, e)
    print(f"\n[deterministic vs default] worst relative difference {worst[0]:.2e} ({worst[1]})")


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_fusion_step_repeats(cuda, mode, dtype):
    zf, g, v, _, _ = H.tiny_setup()
    assert (g.hidden_dropout_prob, g.attention_probs_dropout_prob) == (0.1, 0.1)
    l = _length()
    assert _ragged(B * l) and _ragged(B * B * l)                   # (the embeddings' rows; one branch of the encoder)
    m2, _ = build(g, v, int(zf["seed"]), str(zf["profile"]), dtype)
    freeze_vit(m2)
    m2.train()
    rng = torch.Generator().manual_seed(3)
    z_t = torch.randn((B, l, g.hidden_size), generator=rng).cuda()
    feats = torch.randn((B, 17, g.encoder_width), generator=rng).cuda()
    dl = torch.randn((B, B), generator=rng).cuda()

    def step():
        torch.manual_seed(5)
        _rewind(m2)
        m2.zero_grad(set_to_none=True)
        logits = m2.img_txt_fusion(z_t, feats, CAPS)
        (logits * dl).sum().backward()
        return logits.detach().clone(), _grads(m2)
    mode(True)
    on = [step() for _ in range(3)]
    mode(False)
    _check(on, step())
    assert any(n.startswith("cls_head.") for n in on[0][1]) and "text_encoder.embeddings.word_embeddings.weight" in on[0][1]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_stage1_step_repeats(cuda, mode, dtype):
    from tests.test_train_stage1_gpu import TINY, TINY_VIT, build as build1
    g, v = H.geometry(dict(TINY, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), TINY_VIT)
    assert _ragged(B * _length())
    m1, _ = build1(g, v, 7, "test", dtype)
    m1.train()
    gen = torch.Generator().manual_seed(33)
    ref = torch.randn((B, 17, g.encoder_width), generator=gen).cuda()
    tgt = F.normalize(torch.randn((B + 2, 256), generator=gen), dim=-1).cuda()
    wl = torch.randn((B, B + 2), generator=gen).cuda()

    def step():
        torch.manual_seed(5)
        m1.zero_grad(set_to_none=True)
        logits = m1.img_txt_fusion(ref, tgt, CAPS)
        (logits * wl).sum().backward()
        return logits.detach().clone(), _grads(m1)
    mode(True)
    on = [step() for _ in range(3)]
    mode(False)
    _check(on, step())
    assert "temp" in on[0][1] and "text_encoder.embeddings.position_embeddings.weight" in on[0][1]


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_vit_fine_tuning_step_repeats(cuda, mode, dtype):
    """img_embed in train mode (64 px, depth 2: 17 tokens per image) feeding the fusion pass: the ViT's reverse pass continues from the
    fusion pass's gradient of the target tokens, so every gradient of both flat buffers is compared."""
    zf, g, v, _, _ = H.tiny_setup()
    assert _ragged(B * v.num_tokens)
    m2, _ = build(g, v, int(zf["seed"]), str(zf["profile"]), dtype)
    m2.train()
    l = _length()
    rng = torch.Generator().manual_seed(4)
    z_t = torch.randn((B, l, g.hidden_size), generator=rng).cuda()
    dl = torch.randn((B, B), generator=rng).cuda()
    images = synthetic.scene_images(range(40, 40 + B), v.image_size).cuda()

    def step():
        torch.manual_seed(6)
        _rewind(m2)
        m2.zero_grad(set_to_none=True)
        feats = m2.img_embed(images)
        assert feats.requires_grad
        logits = m2.img_txt_fusion(z_t, feats.float(), CAPS, train=True)
        (logits * dl).sum().backward()
        return logits.detach().clone(), _grads(m2)
    mode(True)
    on = [step() for _ in range(3)]
    mode(False)
    _check(on, step())
    vit = [n for n in on[0][1] if n.startswith("visual_encoder.")]
    assert len(vit) == 6 + 12 * v.depth


@pytest.mark.parametrize("micro", [1, 2], ids=["whole_batch", "two_micro_batches"])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_training_loops_end_in_the_same_bits(cuda, mode, dtype, micro):
    """The reference's loop (zero_grad, img_txt_fusion in train mode, cross-entropy, backward, AdamW.step) three steps long, twice from one
    state dict: every parameter and both AdamW moments agree bit for bit; `micro` = 2 accumulates two micro-batches per step."""
    from candidate_reranking_cir_amd.train import AdamW
    zf, g, v, _, _ = H.tiny_setup()
    l = _length()
    rng = torch.Generator().manual_seed(9)
    z_t = torch.randn((B, l, g.hidden_size), generator=rng).cuda()
    feats = torch.randn((B, 17, g.encoder_width), generator=rng).cuda()
    mode(True)

    def loop():
        m2, _ = build(g, v, int(zf["seed"]), str(zf["profile"]), dtype)
        freeze_vit(m2)
        m2.train()
        params = [p for p in m2.parameters() if p.requires_grad]
        opt = AdamW(params, lr=2e-5, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05, model=m2)
        n = B // micro
        for k in range(3):
            opt.zero_grad()
            torch.manual_seed(100 + k)
            for j in range(micro):
                s = slice(j * n, (j + 1) * n)
                loss = F.cross_entropy(m2.img_txt_fusion(z_t[s], feats[s], CAPS[s]), torch.arange(n, device=cuda)) / micro
                loss.backward()
            opt.step()
        assert opt.t == 3 and opt.skipped_steps == 0
        names = [nm for nm, p in m2.named_parameters() if p.requires_grad]
        return ({nm: p.detach().clone() for nm, p in zip(names, params)}, {nm: opt.m[id(p)].clone() for nm, p in zip(names, params)},
                {nm: opt.v[id(p)].clone() for nm, p in zip(names, params)})
    first, second = loop(), loop()
    for what, a, b_ in zip(("parameter", "first moment", "second moment"), first, second):
        assert a.keys() == b_.keys() and len(a) > 100
        diff = [nm for nm in a if not torch.equal(a[nm], b_[nm])]
        assert not diff, (what, diff[:5], len(diff))
    assert any(bool(t.any()) for t in first[1].values())
