"""Stage-I training-step fixtures WITH a trained image encoder (--blip-img-tune) from the REAL reference (CPU, fp32, ~10 s per case):

    python tools/make_stage1_imgtune_golden.py     # writes tests/golden/train_s1_imgtune.npz and tests/golden/train_s1_imgtune_577.npz

One step of stage1_train.py:169-190 with the full med_config and both dropout probabilities 0 (the stage-I ViT has no DropPath,
blip_stage1.py:34): the reference's BLIP_Retrieval in .train() mode with every parameter trainable,
    ref    = model.img_embed(ref_images)                                          (B, N, 768) tokens with a graph
    tgt    = model.img_embed(tgt_images, return_pool_and_normalized=True)[-1]     (B, 256) with a graph
    logits = model.img_txt_fusion(ref, tgt, captions, train=True)
cross-entropy against arange(B), loss.backward().  The images are seeded normal tensors the test regenerates; only the seed and a slice are
stored.  Ragged captions, one of 40 words (L = 42).
  train_s1_imgtune.npz      64 px, ViT depth 2, B = 4, N = 17:    351 tensors with a gradient = 319 text side + 30 ViT + vision_proj's two
  train_s1_imgtune_577.npz  384 px, ViT depth 1, B = 2, N = 577 (18 full 32-key tiles + 1):    339 = 319 + 18 + 2
Stored: ids / mask, logits, loss, the names of the parameters that received a gradient, per tensor its norm, sum and the 64 entries of
`grad_sample_index`, the full gradients of temp, vision_proj.bias and visual_encoder.cls_token, and a slice of the tokens and of the pooled
features (a forward mismatch is told apart from a backward one).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import OUT, _install_torchvision_stub, build_reference_models, grad_sample_index  # noqa: E402
from candidate_reranking_cir_amd import synthetic  # noqa: E402

FULL = ("temp", "vision_proj.bias", "visual_encoder.cls_token")


def imgtune_images(seed: int, b: int, image_size: int):
    """(reference images, target images), each (B, 3, S, S), of a fixture - the test regenerates them."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((b, 3, image_size, image_size), generator=gen), torch.randn((b, 3, image_size, image_size), generator=gen)


def make(R, full_bert, name, b, image_size, depth, n_words, seed, input_seed):
    cfg = dict(full_bert, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vit = dict(image_size=image_size, width=768, depth=depth, num_heads=12)
    _, m1, g, v = build_reference_models(R, cfg, vit, seed=seed, profile="test")
    caps = [synthetic.caption_text(700 + i, w) for i, w in enumerate(n_words)]
    ri, ti = imgtune_images(input_seed, b, image_size)
    m1.train()
    ref = m1.img_embed(ri)
    tgt = m1.img_embed(ti, return_pool_and_normalized=True)[-1]
    logits = m1.img_txt_fusion(ref, tgt, caps, train=True)
    loss = torch.nn.functional.cross_entropy(logits, torch.arange(b))
    loss.backward()
    tok = m1.tokenizer(caps, padding="longest", return_tensors="pt")
    ids = tok.input_ids.clone(); ids[:, 0] = m1.tokenizer.enc_token_id
    names, norms, sums, samples, full = [], [], [], [], {}
    for pname, p in m1.named_parameters():
        if p.grad is None:
            continue
        gq = p.grad.detach().flatten()
        names.append(pname); norms.append(gq.double().norm().item()); sums.append(gq.double().sum().item())
        samples.append(gq[torch.from_numpy(grad_sample_index(gq.numel()))].numpy())
        if pname in FULL:
            full["full__" + pname] = p.grad.detach().numpy()
    np.savez_compressed(os.path.join(OUT, name + ".npz"), bert_cfg=json.dumps(cfg), vit_cfg=json.dumps(vit), seed=seed, profile="test",
                        caps=np.array(caps), input_ids=ids.numpy(), attention_mask=tok.attention_mask.numpy(), input_seed=input_seed,
                        n_tok=ref.shape[1], ref_image_slice=ri[:, :, :2, :8].numpy(), tgt_image_slice=ti[:, :, :2, :8].numpy(),
                        tokens_slice=ref.detach()[:, :3, :16].numpy(), pooled_slice=tgt.detach()[:, :16].numpy(),
                        logits=logits.detach().numpy(), loss=loss.item(),
                        names=np.array(names), norms=np.array(norms), sums=np.array(sums), samples=np.stack(samples), **full)
    n_vit = sum(n.startswith("visual_encoder.") for n in names)
    print(f"{name}: tokens {tuple(ref.shape)} L {ids.shape[1]} loss {loss.item():.5f} logits sigma {logits.std().item():.4f} params with grad "
          f"{len(names)} (ViT {n_vit}) zero-gradient tensors {sum(x == 0.0 for x in norms)} norm range {min(norms):.3e} {max(norms):.3e}")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = ref_shim.load_reference_modules()
    _install_torchvision_stub()
    full_bert = json.load(open(os.path.join(ref_shim.REFERENCE_ROOT, "configs", "med_config.json")))
    make(R, full_bert, "train_s1_imgtune", 4, 64, 2, (5, 40, 3, 9), seed=31, input_seed=5)
    make(R, full_bert, "train_s1_imgtune_577", 2, 384, 1, (5, 40), seed=31, input_seed=5)


if __name__ == "__main__":
    main()
