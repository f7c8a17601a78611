"""Stage-I training-step fixtures from the REAL reference (CPU, fp32, seconds):

    python tools/make_stage1_train_golden.py          # writes tests/golden/train_s1.npz and tests/golden/train_s1_577.npz

One step of stage1_train.py:170-176 with the full med_config and both dropout probabilities 0: the reference's BLIP_Retrieval in
.train() mode, `logits = model.img_txt_fusion(ref_tokens, target_feats, captions, train=True)` (blip_stage1.py:67-92), cross-entropy
against arange(B), loss.backward().  The inputs of img_txt_fusion are seeded normal tensors the test regenerates (the targets L2-normalised,
as img_embed(..., return_pool_and_normalized=True)[-1] leaves them); only the seed and two slices are stored.  Ragged captions, one of 40
words (L = 42: the first end-to-end training fixture with more than 32 caption tokens).
  train_s1.npz      B = 4, N = 17 image tokens
  train_s1_577.npz  B = 8, N = 577 (the reference's 384-px token count: 18 full 32-key tiles + 1)
Stored: ids / mask, logits, loss, the names of the parameters that received a gradient, per tensor its norm, sum and the 64 entries of
`grad_sample_index`, and the full gradients of temp, text_proj.bias and one LayerNorm.
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

FULL = ("temp", "text_proj.bias", "text_encoder.encoder.layer.0.crossattention.output.LayerNorm.weight")


def stage1_inputs(seed: int, b: int, n_tok: int, width: int = 768, embed: int = 256):
    """(reference tokens (B, N, width), normalised target features (B, embed)) of a fixture - the test regenerates them."""
    gen = torch.Generator().manual_seed(seed)
    ref = torch.randn((b, n_tok, width), generator=gen)
    tgt = torch.nn.functional.normalize(torch.randn((b, embed), generator=gen), dim=-1)
    return ref, tgt


def make(R, full_bert, name, b, image_size, n_words, seed, input_seed):
    cfg = dict(full_bert, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    vit = dict(image_size=image_size, width=768, depth=1, num_heads=12)          # the ViT is not run: geometry only
    _, m1, g, v = build_reference_models(R, cfg, vit, seed=seed, profile="test")
    n_tok = (image_size // 16) ** 2 + 1
    caps = [synthetic.caption_text(400 + 10 * seed + i, w) for i, w in enumerate(n_words)]
    ref, tgt = stage1_inputs(input_seed, b, n_tok)
    m1.train()
    for p in m1.visual_encoder.parameters():                                     # --blip-img-tune off (stage1_train.py:72-74)
        p.requires_grad_(False)
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
                        caps=np.array(caps), input_ids=ids.numpy(), attention_mask=tok.attention_mask.numpy(), input_seed=input_seed, n_tok=n_tok,
                        ref_slice=ref[:, :2, :8].numpy(), target_slice=tgt[:, :8].numpy(), logits=logits.detach().numpy(), loss=loss.item(),
                        names=np.array(names), norms=np.array(norms), sums=np.array(sums), samples=np.stack(samples), **full)
    print(f"{name}: L {ids.shape[1]} loss {loss.item():.5f} logits sigma {logits.std().item():.4f} params with grad {len(names)} "
          f"temp grad {float(m1.temp.grad):.4f} norm range {min(norms):.3e} {max(norms):.3e}")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = ref_shim.load_reference_modules()
    _install_torchvision_stub()
    full_bert = json.load(open(os.path.join(ref_shim.REFERENCE_ROOT, "configs", "med_config.json")))
    make(R, full_bert, "train_s1", 4, 64, (5, 40, 3, 9), seed=21, input_seed=211)
    make(R, full_bert, "train_s1_577", 8, 384, (5, 12, 3, 40, 9, 4, 11, 6), seed=23, input_seed=577)


if __name__ == "__main__":
    main()
