"""ViT gradient checkpointing (`vit_grad_ckpt` / `vit_ckpt_layer`, `set_vit_checkpointing`; vit.py:103-105, :158) on a real MI355X.  A
checkpointed block keeps its two fp32 stream rows and the backward rebuilds the rest with the forward's own launches, so in the deterministic
mode NOTHING may move: tokens, logits and every gradient are compared with `torch.equal` against the unchecked pass; in the default mode
the gradients stay within the fp32 reorder noise tests/test_train_deterministic_gpu.py allows two default backward passes (NOISE = 1e-4 of
the tensor's norm).  The saved state is weighed (`train.vit_saved_bytes`), the peak of forward + backward is compared, and the guards of
tests/test_train_vit_gpu.py - several live calls, an optimizer step before the backward, a second backward - are driven with checkpointing on.

Shapes: tests/golden/train_imgtune.npz's ViT (64 px, 17 tokens, width 768, depth 2) and a depth-4 variant at batch 13 - 221 rows, ragged
against the 32- and 64-row kernels, more than one workgroup in each - with DropPath 0.6; tests/golden/train_imgtune224.npz (ViT-B/16, 197
tokens, depth 12, its own batch of 4) with `vit_ckpt_layer = 4`, the reference's configs/retrieval_coco.yaml."""
import json

import pytest
import torch
import torch.nn.functional as F

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests.test_train_deterministic_gpu import NOISE
from tests.test_train_gpu import BF, HF, build

pytestmark = pytest.mark.gpu
B = 13


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


def _grads(model, prefix=""):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None and n.startswith(prefix)}


def _unequal(a, b):
    assert a.keys() == b.keys() and len(a) > 0
    return [n for n in a if not torch.equal(a[n], b[n])]


def _saved_tensors(sv):
    """Every tensor of a call's saved state: the patch rows, each block's entry, the final stream, the DropPath scales."""
    out = [sv["patches"], sv["xf"]] + [t for s in sv["blocks"] for t in s.values()]
    assert all(torch.is_tensor(t) for t in out)
    return out + ([sv["dp"]] if sv["dp"] is not None else [])


def _tiny_vit(dtype, depth, drop_path=0.6):
    z = H.load("train_imgtune.npz")
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), dict(json.loads(str(z["vit_cfg"])), depth=depth, drop_path_rate=drop_path))
    assert (v.image_size, v.num_tokens, v.width) == (64, 17, 768)
    m2, _ = build(g, v, int(z["seed"]), str(z["profile"]), dtype)
    return v, m2.train()


# ---------------------------------------------------------------------------------------------------------------- the tiny ViT
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_tiny_vit_gradients_do_not_move(cuda, mode, dtype, depth):
    from candidate_reranking_cir_amd import train
    v, m2 = _tiny_vit(dtype, depth)
    rows = B * v.num_tokens
    assert rows == 221 and rows % 32 != 0 and rows % 64 != 0 and rows > 3 * 64
    images = synthetic.scene_images(range(40, 40 + B), v.image_size).cuda()
    dfe = (torch.randn((B, v.num_tokens, v.width), generator=torch.Generator().manual_seed(3)) * 1e-3).cuda()

    def run(blocks):
        m2.set_vit_checkpointing(blocks)
        if getattr(m2, "_vit_trainer", None) is not None:
            m2._vit_trainer.step_no = 0                         # the DropPath draw is a function of (seed, step): the same draw every run
        m2.zero_grad(set_to_none=True)
        feats = m2.img_embed(images)
        assert feats.requires_grad
        sv = m2._vit_trainer.sv
        assert sv["ckpt"] == [i >= depth - min(blocks, depth) for i in range(depth)]
        assert sum(t.nbytes for t in _saved_tensors(sv)) == train.vit_saved_bytes(m2, B)
        dp = sv["dp"].cpu()
        assert bool((dp == 0).any()) and bool((dp > 1).any())   # both DropPath outcomes occur
        feats.backward(dfe)
        return feats.detach().clone(), _grads(m2, "visual_encoder.")

    settings = (0, 1, 2, depth + 5)
    mode(True)
    det = {k: run(k) for k in settings}
    assert len(det[0][1]) == 6 + 12 * depth and all(bool(torch.isfinite(t).all()) for t in det[0][1].values())
    for k in settings[1:]:
        assert torch.equal(det[k][0], det[0][0]), k
        assert not _unequal(det[k][1], det[0][1]), (k, _unequal(det[k][1], det[0][1])[:5])
    mode(False)
    worst = (0.0, "")
    for k in settings:
        tokens, grads = run(k)
        assert torch.equal(tokens, det[0][0]), k
        for n, ref in det[0][1].items():
            e = (grads[n] - ref).norm().item()
            worst = max(worst, (e / (ref.norm().item() + 1e-12), n, k))
            assert e <= NOISE * (ref.norm().item() + 1e-12), (k, n, e / (ref.norm().item() + 1e-12))
    print(f"\n[depth {depth} {dtype}] default mode against the deterministic gradients: worst relative difference {worst[0]:.2e} ({worst[1]}, {worst[2]} blocks)")
    m2.eval()


def test_peak_memory_is_lower_with_every_block_checkpointed(cuda, mode):
    """Depth 4, all blocks against none, same process, same inputs, forward + backward after reset_peak_memory_stats.  An inequality: the
    derived live sets are about 0.2 * 4 + 1 blocks' worth of activations against 4."""
    from candidate_reranking_cir_amd import train
    mode(True)
    v, m2 = _tiny_vit(HF, 4, drop_path=0.0)
    images = synthetic.scene_images(range(40, 40 + B), v.image_size).cuda()
    dfe = (torch.randn((B, v.num_tokens, v.width), generator=torch.Generator().manual_seed(3)) * 1e-3).cuda()

    def peak(blocks):
        m2.set_vit_checkpointing(blocks)
        m2.zero_grad(set_to_none=True)
        m2._vit_trainer.sv = None                               # (the trainer's pointer to the previous call's state, kept for tools)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        feats = m2.img_embed(images)
        feats.backward(dfe)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, train.vit_saved_bytes(m2, B)
    m2.img_embed(images).backward(dfe)                          # builds the trainer, its slab and the deterministic workspace once
    p0, s0 = peak(0)
    p4, s4 = peak(4)
    p0b, _ = peak(0)
    print(f"\n[depth 4, batch {B}] peak above the resting allocation: unchecked {p0 / 2 ** 20:.1f} MiB (again {p0b / 2 ** 20:.1f}), all checkpointed "
          f"{p4 / 2 ** 20:.1f} MiB; saved bytes {s0 / 2 ** 20:.1f} -> {s4 / 2 ** 20:.1f} MiB")
    assert s4 < s0 and p4 < p0 and p4 < p0b
    m2.eval()


# ---------------------------------------------------------------------------------------------------------------- the real widths
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_real_widths_through_the_factory(cuda, mode, dtype):
    """ViT-B/16 at 224 px, depth 12, `vit_grad_ckpt=True, vit_ckpt_layer=4` GIVEN TO THE FACTORY, through img_embed -> img_txt_fusion ->
    backward: logits and all 150 + 572 gradients equal the unchecked run's bit for bit, and the saved state is what `vit_saved_bytes` says."""
    from candidate_reranking_cir_amd import train
    from candidate_reranking_cir_amd.blip_stage2 import blip_stage2
    z = H.load("train_imgtune224.npz")
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    assert (v.depth, v.num_tokens, v.width) == (12, 197, 768)
    sd2, _ = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    m2 = blip_stage2(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer(), vit_grad_ckpt=True, vit_ckpt_layer=4)
    m2.load_state_dict(sd2, strict=True)
    m2 = m2.cuda().float().set_compute_dtype(dtype).train()
    assert train.vit_checkpointed_blocks(m2) == 4
    images = synthetic.scene_images(z["image_ids"].tolist(), v.image_size).cuda()
    bsz = images.shape[0]
    caps, z_t = [str(c) for c in z["caps"]], torch.from_numpy(z["z_t"]).cuda()
    n, d = v.num_tokens, v.width
    mode(True)

    def run():
        m2.zero_grad(set_to_none=True)
        feats = m2.img_embed(images)
        sv = m2._vit_trainer.sv
        saved = sum(t.nbytes for t in _saved_tensors(sv))
        entries = [[t.nbytes for t in s.values()] for s in sv["blocks"]]
        logits = m2.img_txt_fusion(z_t, feats.float(), caps, train=True)
        F.cross_entropy(logits, torch.arange(bsz, device=cuda)).backward()
        return logits.detach().clone(), _grads(m2), saved, entries, list(sv["ckpt"])

    l4, g4, saved4, entries4, ck4 = run()                       # as the factory was told
    want4 = train.vit_saved_bytes(m2, bsz)
    m2.set_vit_checkpointing(0)
    l0, g0, saved0, entries0, ck0 = run()
    want0 = train.vit_saved_bytes(m2, bsz)
    assert ck4 == [False] * 8 + [True] * 4 and ck0 == [False] * 12
    assert sum(k.startswith("visual_encoder.") for k in g0) == 150 and len(g0) == 150 + 572
    assert torch.equal(l4, l0)
    assert not _unequal(g4, g0), _unequal(g4, g0)[:5]
    # the saved state: what the function says; a checkpointed entry is exactly the two fp32 stream rows
    assert (saved4, saved0) == (want4, want0) and want0 - want4 == 4 * bsz * n * (30768 - 6144)
    assert all(e == [bsz * n * d * 4] * 2 for e in entries4[8:]) and all(len(e) == 10 and sum(e) == bsz * n * 30768 for e in entries4[:8] + entries0)
    m2.eval()


# ---------------------------------------------------------------------------------------------------------------- live calls and guards
def test_live_calls_and_guards_with_checkpointing(cuda, mode, monkeypatch):
    """The reference's `blip_bs` pattern (stage2_train.py:191-199): three calls of 5 / 5 / 3 images live at once, checkpointed, differentiated
    together - the same bits as the same three calls unchecked.  An optimizer step between a forward and its backward is refused BEFORE any
    recompute launch; a second backward through one call raises."""
    from candidate_reranking_cir_amd import train_ops
    from candidate_reranking_cir_amd.train import AdamW
    mode(True)
    v, m2 = _tiny_vit(HF, 2)
    images = synthetic.scene_images(range(40, 40 + B), v.image_size).cuda()
    dfe = (torch.randn((B, v.num_tokens, v.width), generator=torch.Generator().manual_seed(11)) * 1e-3).cuda()
    pair_calls = []
    real_pair = train_ops.gelu_bwd16_pair
    monkeypatch.setattr(train_ops, "gelu_bwd16_pair", lambda *a, **kw: (pair_calls.append(1), real_pair(*a, **kw))[1])

    def three(blocks):
        m2.set_vit_checkpointing(blocks)
        if getattr(m2, "_vit_trainer", None) is not None:
            m2._vit_trainer.step_no = 0
        m2.zero_grad(set_to_none=True)
        parts = [m2.img_embed(images[a:b]) for a, b in ((0, 5), (5, 10), (10, 13))]
        both = torch.vstack(parts)
        both.backward(dfe)
        return both.detach().clone(), _grads(m2, "visual_encoder."), parts
    t0, g0, _ = three(0)
    assert not pair_calls
    t2, g2, parts = three(2)
    assert len(pair_calls) == 3 * 2                              # three calls x two checkpointed blocks
    assert torch.equal(t2, t0) and not _unequal(g2, g0), _unequal(g2, g0)[:5]
    with pytest.raises(RuntimeError, match="second backward"):
        parts[0].sum().backward()
    f3 = m2.img_embed(images[:2])
    AdamW([p for p in m2.parameters() if p.requires_grad], lr=1e-4, model=m2).step()
    before = len(pair_calls)
    with pytest.raises(RuntimeError, match="parameters were updated"):
        f3.sum().backward()
    assert len(pair_calls) == before                             # no recompute ran on the updated weights
    m2.eval()


# ---------------------------------------------------------------------------------------------------------------- stage I
def test_stage1_image_tuning_with_checkpointing(cuda, mode):
    """BLIP_Retrieval with set_image_tuning() and set_vit_checkpointing(depth) on the tiny stage-I setup of
    tests/test_train_stage1_imgtune_gpu.py: reference and target images both carry a graph through the ViT."""
    from tests.test_train_stage1_imgtune_gpu import embed, grads_of, tiny
    mode(True)
    g, v, m1, _ = tiny(HF, 768, depth=2, p_drop=0.1)
    gen = torch.Generator().manual_seed(12)
    imgs, timgs = torch.randn((3, 3, 64, 64), generator=gen).cuda(), torch.randn((3, 3, 64, 64), generator=gen).cuda()
    caps = [synthetic.caption_text(900 + i, w) for i, w in enumerate((5, 11, 3))]
    gt = torch.arange(3, device=cuda)
    m1.train()

    def step(blocks):
        assert m1.set_vit_checkpointing(blocks) is m1
        torch.manual_seed(9)
        m1.zero_grad(set_to_none=True)
        ref, tgt = embed(m1, imgs, timgs)
        assert ref.requires_grad and tgt.requires_grad and m1._vit_trainer.sv["ckpt"] == [blocks > 0] * 2
        logits = m1.img_txt_fusion(ref, tgt, caps, train=True)
        F.cross_entropy(logits, gt).backward()
        return logits.detach().clone(), grads_of(m1)
    l0, g0 = step(0)
    l2, g2 = step(v.depth)
    assert sum(n.startswith("visual_encoder.") for n in g0) == 6 + 12 * v.depth
    assert torch.equal(l2, l0) and not _unequal(g2, g0), _unequal(g2, g0)[:5]
    m1.eval()


# ---------------------------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "fp16"])
def test_run_with_checkpointing_resumes_bit_for_bit(cuda, mode, dtype, tmp_path):
    """tests/test_resume_gpu.py's ViT fine-tuning drive, 2 + 1 steps against 3, with every ViT block checkpointed: parameters and both
    moments agree bit for bit, and with the unchecked run's - the recompute draws nothing and counts nothing, so there is no state to save."""
    from candidate_reranking_cir_amd import train
    from tests.test_resume_gpu import CAPS, _differences, _geometry, _run_resumed, _stage2_inputs, _stage2_model
    mode(True)
    g, v = _geometry()
    z_t, _ = _stage2_inputs(g, seed=4)
    images = synthetic.scene_images(range(40, 40 + len(CAPS)), v.image_size).cuda()
    states = []

    def steps(m2, opt, k):
        for _ in range(k):
            opt.zero_grad()
            feats = m2.img_embed(images)
            assert feats.requires_grad and all(m2._vit_trainer.sv["ckpt"]) == (m2.vit_ckpt_blocks > 0)
            F.cross_entropy(m2.img_txt_fusion(z_t, feats.float(), CAPS, train=True), torch.arange(len(CAPS), device=cuda)).backward()
            opt.step()
        states.append(train.training_state(m2))
    new = lambda blocks: (lambda: _stage2_model(dtype, frozen=False).set_vit_checkpointing(blocks))
    a, b = _run_resumed(new(v.depth), steps, 2, 3, tmp_path / "ck.pt")
    assert not _differences(a, b), _differences(a, b)[:5]
    assert sum(n.startswith("visual_encoder.") for n in a[1]) == 6 + 12 * v.depth
    assert all(set(s) == {"format", "cpu_rng_state", "fusion", "vit"} for s in states)          # nothing added to the training state
    torch.manual_seed(77)
    m0 = new(0)()
    from tests.test_resume_gpu import _optimizer, _result
    o0 = _optimizer(m0)
    steps(m0, o0, 3)
    assert not _differences(a, _result(m0, o0))                                                  # ... and the unchecked run ends in the same bits
