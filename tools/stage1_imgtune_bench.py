"""Timing of one stage-I training step with the image encoder frozen against tuned (`BLIP_Retrieval.set_image_tuning()`,
stage1_train.py --blip-img-tune) at the reference's geometry (full med_config, dropout 0.1 / 0.1, ViT-B at 384 px: 577 tokens), one JSON line.

    python tools/stage1_imgtune_bench.py [--batch 64] [--blip-bs 32] [--length 32] [--dtype f16|bf16] [--steps 5] [--warmup 2]

Both steps start from pixels, as stage1_train.py:144-190 does: img_embed of B reference and B target images in `blip_bs` mini-batches, the
fusion forward, cross-entropy, backward, train.AdamW.step.  Device-event times per step, and the split of the tuned step:
  vit_forward_ms      the 2 B / blip_bs img_embed calls with a graph (the pooled head included)
  fusion_forward_ms   img_txt_fusion
  backward_ms         loss.backward(): the text side, the 12 added dgrad GEMMs, the heads and both ViT reverse passes
  input_grads_ms      what the fusion backward costs more when ref_tokens / target are leaves that require grad - the 12 dgrad GEMMs of B N
                      rows plus cir_contrastive_bwd_target - than when they carry no graph (the same tokens, no ViT behind them)
  heads_ms            cir_pooled_head_fwd + cir_pooled_head_bwd + cir_contrastive_bwd_target on the step's shapes, timed alone
The saved activations of the ViT's reverse pass are ~0.2 GiB per image at 384 px: the batch the reference defaults to (1024, i.e. 2048
images with a graph) does not fit one device's memory, here or in the reference - hence the smaller default batch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from candidate_reranking_cir_amd import config as cfgmod, synthetic, train, train_ops as T  # noqa: E402
from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--blip-bs", type=int, default=32)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=384)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--dtype", default="f16", choices=("f16", "bf16"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    b, l, bs = a.batch, a.length, a.blip_bs
    dev = torch.device("cuda")
    g = cfgmod.BertGeometry.from_dict(dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, layer_norm_eps=1e-12,
                                           vocab_size=30524, max_position_embeddings=512, encoder_width=768, hidden_dropout_prob=0.1,
                                           attention_probs_dropout_prob=0.1))
    v = cfgmod.VitGeometry(image_size=a.image_size, width=768, depth=a.depth, num_heads=12)
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).to(dev).float()
    m1.set_compute_dtype(torch.float16 if a.dtype == "f16" else torch.bfloat16)
    m1.train()
    caps = [synthetic.caption_text(i, (l - 2) if i == 0 else 6 + (i * 7) % (l - 8)) for i in range(b)]
    gen = torch.Generator(device=dev).manual_seed(0)
    ri = torch.randn((b, 3, a.image_size, a.image_size), generator=gen, device=dev)
    ti = torch.randn((b, 3, a.image_size, a.image_size), generator=gen, device=dev)
    gt = torch.arange(b, device=dev)
    opt = train.AdamW([p for p in m1.parameters() if p.requires_grad], lr=2e-5, weight_decay=0.05, model=m1)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = []

    def embed():
        ref = torch.vstack([m1.img_embed(x) for x in torch.split(ri, bs)])
        tgt = torch.vstack([m1.img_embed(x, return_pool_and_normalized=True)[-1] for x in torch.split(ti, bs)])
        return ref, tgt

    def step():
        es = [ev() for _ in range(4)]
        opt.zero_grad()
        es[0].record()
        ref, tgt = embed()
        es[1].record()
        loss = F.cross_entropy(m1.img_txt_fusion(ref, tgt, caps, train=True), gt)
        es[2].record()
        loss.backward()
        es[3].record()
        opt.step()
        marks.append(es)

    out = {"workload": "stage1_imgtune_step", "B": b, "blip_bs": bs, "L": l, "N": v.num_tokens, "vit_depth": a.depth, "dtype": a.dtype, "steps": a.steps,
           "warmup": a.warmup}
    for mode in ("frozen", "tuned"):
        m1.set_image_tuning(mode == "tuned")
        marks.clear()
        torch.cuda.reset_peak_memory_stats()
        out[mode + "_step_ms"] = round(timed(step, a.steps, a.warmup), 3)
        split = [sum(es[i].elapsed_time(es[i + 1]) for es in marks[a.warmup:]) / a.steps for i in range(3)]
        out[mode + "_split_ms"] = {"vit_forward_ms": round(split[0], 3), "fusion_forward_ms": round(split[1], 3), "backward_ms": round(split[2], 3)}
        out[mode + "_peak_mem_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    # the fusion backward alone: graph-free tokens against leaf tokens that require grad (no ViT behind either)
    with torch.no_grad():
        ref0, tgt0 = embed()
    for key, need in (("fusion_backward_ms", False), ("fusion_backward_with_input_grads_ms", True)):
        ms = []
        for i in range(a.warmup + a.steps):
            opt.zero_grad()
            r, t = ref0.clone().requires_grad_(need), tgt0.clone().requires_grad_(need)
            loss = F.cross_entropy(m1.img_txt_fusion(r, t, caps, train=True), gt)
            e0, e1 = ev(), ev()
            e0.record()
            loss.backward()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[key] = round(sum(ms[a.warmup:]) / a.steps, 3)
    out["input_grads_ms"] = round(out["fusion_backward_with_input_grads_ms"] - out["fusion_backward_ms"], 3)
    # the three new entry points alone
    w, bias = m1.vision_proj.weight.detach(), m1.vision_proj.bias.detach()
    tok = ref0[:bs].contiguous()
    dth, dl, ph = torch.randn((bs, 256), device=dev), torch.randn((b, b), device=dev), F.normalize(torch.randn((b, 256), device=dev), dim=-1)
    dw, db, dtok = torch.zeros_like(w), torch.zeros_like(bias), torch.zeros_like(tok)
    temp = m1.temp.detach().reshape(1)

    def heads():
        for _ in range(b // bs):
            th, inv = T.pooled_head_fwd(tok[:, 0], w, bias)
            T.pooled_head_bwd(dth, th, inv, tok[:, 0], w, dw, db, dtok[:, 0])
        T.contrastive_bwd_target(dl, ph, temp)
    out["heads_ms"] = round(timed(heads, 20, 3), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
