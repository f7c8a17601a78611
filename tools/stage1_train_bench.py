"""Timing of the stage-I training step (stage1_train.py:170-192 on BLIP_Retrieval.img_txt_fusion(..., train=True)): forward, cross-entropy,
backward and train.AdamW.step at the reference's geometry (full med_config, dropout 0.1 / 0.1, 577 image tokens), one JSON line.

    python tools/stage1_train_bench.py [--batch 1024] [--length 32] [--tokens 577] [--dtype f16|bf16] [--steps 10] [--warmup 3] [--deterministic]

ms per step from device events around the timed steps (after the warm-up); algorithmic FLOPs counted from the shapes below (the products
the reference computes - the attention backward's recomputed scores are not credited), and their share of the dense 16-bit MFMA peak.
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

from candidate_reranking_cir_amd import config as cfgmod, synthetic, train  # noqa: E402
from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval  # noqa: E402

PEAK_TFLOPS = 2516.6          # dense 16-bit MFMA peak of the MI355X (bench.PEAK_TFLOPS)


def step_flops(b: int, l: int, n: int, d: int = 768, f: int = 3072, dv: int = 768, layers: int = 12, e: int = 256):
    """(forward, backward) algorithmic FLOPs of one step: per layer the q|k|v, o, cross q, cross k|v (over B N image rows), cross o and
    FFN products, both attentions' two products each; backward = dgrad of every text-side product (none into the frozen image tokens) +
    every weight gradient + four products per attention; text_proj and the head on top."""
    r = b * l
    text = 2 * r * d * (3 * d + 3 * d + 2 * f)                       # qkv, o, cross q, cross o, FFN in / out
    kv = 2 * b * n * dv * 2 * d
    attn = 4 * b * l * l * d + 4 * b * l * n * d
    head = 2 * b * d * e + 2 * b * b * e
    fwd = layers * (text + kv + attn) + head
    bwd = layers * (2 * text + kv + 2 * attn) + 2 * head + 2 * b * d * e
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=577)
    ap.add_argument("--dtype", default="f16", choices=("f16", "bf16"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--deterministic", action="store_true", help="train.set_deterministic(True): the fixed-order forms of every cross-workgroup sum")
    a = ap.parse_args()
    train.set_deterministic(a.deterministic)
    b, l, n = a.batch, a.length, a.tokens
    dev = torch.device("cuda")
    g = cfgmod.BertGeometry.from_dict(dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, layer_norm_eps=1e-12,
                                           vocab_size=30524, max_position_embeddings=512, encoder_width=768, hidden_dropout_prob=0.1,
                                           attention_probs_dropout_prob=0.1))
    side = int(round((n - 1) ** 0.5)) * 16
    v = cfgmod.VitGeometry(image_size=side, width=768, depth=1, num_heads=12)           # the ViT is not run: the tokens are inputs
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).to(dev).float()
    m1.set_compute_dtype(torch.float16 if a.dtype == "f16" else torch.bfloat16)
    m1.train()
    caps = [synthetic.caption_text(i, (l - 2) if i == 0 else 6 + (i * 7) % (l - 8)) for i in range(b)]      # ragged, padded to L
    gen = torch.Generator(device=dev).manual_seed(0)
    ref = torch.randn((b, n, 768), generator=gen, device=dev)
    tgt = F.normalize(torch.randn((b, 256), generator=gen, device=dev), dim=-1)
    gt = torch.arange(b, device=dev)
    opt = train.AdamW([p for p in m1.parameters() if p.requires_grad], lr=2e-5, weight_decay=0.05, model=m1)

    def step():
        opt.zero_grad()
        loss = F.cross_entropy(m1.img_txt_fusion(ref, tgt, caps, train=True), gt)
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    fwd, bwd = step_flops(b, l, n)
    tflops = (fwd + bwd) / (ms * 1e-3) / 1e12
    print(json.dumps({"workload": "stage1_train_step", "B": b, "L": l, "N": n, "dtype": a.dtype, "deterministic": train.deterministic(), "steps": a.steps, "warmup": a.warmup,
                      "ms_per_step": round(ms, 3), "tflop_forward": round(fwd / 1e12, 3), "tflop_backward": round(bwd / 1e12, 3),
                      "achieved_tflops": round(tflops, 1), "peak_tflops": PEAK_TFLOPS, "frac_of_peak": round(tflops / PEAK_TFLOPS, 4),
                      "loss": round(float(loss.detach()), 5), "skipped_steps": opt.skipped_steps,
                      "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}))


if __name__ == "__main__":
    main()
