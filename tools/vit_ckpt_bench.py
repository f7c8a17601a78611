"""What ViT gradient checkpointing (`set_vit_checkpointing`; `vit_grad_ckpt` / `vit_ckpt_layer` of the factories) costs and saves at the
reference's geometry (ViT-B/16 at 384 px: 577 tokens, depth 12; full med_config), one JSON document.  Needs the GPU.

    python tools/vit_ckpt_bench.py [--batch 16] [--length 32] [--dtype f16|bf16] [--steps 5] [--warmup 2] [--blocks 0,4,12] [--out FILE]

For each number of checkpointed blocks:
  stage2   one stage-II image-tuning step from pixels (stage2_train.py:191-218 with --blip-img-tune): img_embed of `batch` target images
           with a graph, img_txt_fusion over batch^2 triplets, cross-entropy, backward, train.AdamW.step.  step_ms (device events over the
           whole step), peak_mem_bytes (torch.cuda.max_memory_allocated() over the timed steps), vit_saved_bytes (train.vit_saved_bytes).
  vit      the image encoder alone on the same images: forward_ms of img_embed with a graph and backward_ms of its reverse pass from a
           given token gradient; recompute_share = (backward_ms - backward_ms at 0 blocks) / backward_ms.
  stage1   one stage-I image-tuning forward and backward (stage1_train.py:144-190 with --blip-img-tune): reference and target images
           through img_embed with a graph (two live calls), the fusion forward, cross-entropy, backward.  step_ms, peak_mem_bytes and
           vit_saved_bytes (of both calls).
And once: `pair`, the backward's one pass over z16 (train_ops.gelu_bwd16_pair: dz and gelu(z) together, bias sums included) against the
two launches it replaces in a checkpointed block (train_ops.gelu_bwd16 + train_ops.eltwise GELU) at (batch * 577) x 3072, alternating.
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
from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR  # noqa: E402


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


def measured(fn, steps, warmup):
    """(ms per call, peak bytes over the timed calls); the warm-up calls have built the trainers and their buffers."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(fn, steps, 0)
    return round(ms, 3), int(torch.cuda.max_memory_allocated())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--image-size", type=int, default=384)
    ap.add_argument("--dtype", default="f16", choices=("f16", "bf16"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", default="0,4,12")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vit_ckpt_bench.py measures on the GPU; none is visible")
    b, l = a.batch, a.length
    dt = torch.float16 if a.dtype == "f16" else torch.bfloat16
    blocks = [int(x) for x in a.blocks.split(",")]
    dev = torch.device("cuda")
    g = cfgmod.BertGeometry.from_dict(dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, layer_norm_eps=1e-12,
                                           vocab_size=30524, max_position_embeddings=512, encoder_width=768, hidden_dropout_prob=0.1,
                                           attention_probs_dropout_prob=0.1))
    v = cfgmod.VitGeometry(image_size=a.image_size, width=768, depth=12, num_heads=12)
    caps = [synthetic.caption_text(i, (l - 2) if i == 0 else 6 + (i * 7) % (l - 8)) for i in range(b)]
    gen = torch.Generator(device=dev).manual_seed(0)
    images = torch.randn((b, 3, a.image_size, a.image_size), generator=gen, device=dev)
    images2 = torch.randn((b, 3, a.image_size, a.image_size), generator=gen, device=dev)
    gt = torch.arange(b, device=dev)
    out = {"workload": "vit_checkpointing", "batch": b, "L": l, "N": v.num_tokens, "image_size": a.image_size, "dtype": a.dtype, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "stage2": {}, "vit": {}, "stage1": {}}

    # ---- stage II: one image-tuning step; and the image encoder alone
    m2 = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).to(dev).float().set_compute_dtype(dt)
    m2.train()
    opt = train.AdamW([p for p in m2.parameters() if p.requires_grad], lr=2e-5, weight_decay=0.05, model=m2)
    z_t = torch.randn((b, l, 768), generator=gen, device=dev)
    dfe = torch.randn((b, v.num_tokens, 768), generator=gen, device=dev) * 1e-3

    def step2():
        opt.zero_grad()
        feats = m2.img_embed(images)
        F.cross_entropy(m2.img_txt_fusion(z_t, feats.float(), caps, train=True), gt).backward()
        opt.step()
    for k in blocks:
        m2.set_vit_checkpointing(k)
        ms, peak = measured(step2, a.steps, a.warmup)
        out["stage2"][str(k)] = {"step_ms": ms, "peak_mem_bytes": peak, "vit_saved_bytes": train.vit_saved_bytes(m2, b)}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for k in blocks:
        m2.set_vit_checkpointing(k)
        fw, bw = [], []
        for i in range(a.warmup + a.steps):
            m2.zero_grad(set_to_none=True)
            e = [ev() for _ in range(3)]
            e[0].record()
            feats = m2.img_embed(images)
            e[1].record()
            feats.backward(dfe)
            e[2].record()
            torch.cuda.synchronize()
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
        out["vit"][str(k)] = {"forward_ms": round(sum(fw[a.warmup:]) / a.steps, 3), "backward_ms": round(sum(bw[a.warmup:]) / a.steps, 3)}
    if "0" in out["vit"]:
        for k in blocks:
            r = out["vit"][str(k)]
            r["recompute_share"] = round((r["backward_ms"] - out["vit"]["0"]["backward_ms"]) / r["backward_ms"], 4)
    del m2, opt, feats
    torch.cuda.empty_cache()

    # ---- stage I: one image-tuning forward and backward, both image sides with a graph
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).to(dev).float().set_compute_dtype(dt)
    m1.set_image_tuning().train()

    def step1():
        m1.zero_grad(set_to_none=True)
        ref = m1.img_embed(images)
        tgt = m1.img_embed(images2, return_pool_and_normalized=True)[-1]
        F.cross_entropy(m1.img_txt_fusion(ref, tgt, caps, train=True), gt).backward()
    for k in blocks:
        m1.set_vit_checkpointing(k)
        ms, peak = measured(step1, a.steps, a.warmup)
        out["stage1"][str(k)] = {"step_ms": ms, "peak_mem_bytes": peak, "vit_saved_bytes": 2 * train.vit_saved_bytes(m1, b)}
    del m1
    torch.cuda.empty_cache()

    # ---- the pair kernel against the two launches it replaces
    rows, cols = b * v.num_tokens, 3072
    z = (torch.randn((rows, cols), generator=gen, device=dev) * 2.5).to(dt)
    df = torch.randn((rows, cols), generator=gen, device=dev).to(dt)
    sums = torch.zeros((cols,), device=dev)
    dz, f = torch.empty_like(z), torch.empty_like(z)
    two = lambda: (T.gelu_bwd16(df, z, sums=sums, out=dz), T.eltwise(z, T.MODE_GELU, out=f))
    one = lambda: T.gelu_bwd16_pair(df, z, sums=sums, out=dz, out_f=f)
    t_two, t_one = [], []
    for _ in range(3):                                          # alternating
        t_two.append(timed(two, 50, 5))
        t_one.append(timed(one, 50, 5))
    out["pair"] = {"rows": rows, "cols": cols, "gelu_bwd16_plus_eltwise_gelu_us": [round(1e3 * t, 2) for t in t_two],
                   "gelu_bwd16_pair_us": [round(1e3 * t, 2) for t in t_one], "bytes_two": 5 * rows * cols * 2, "bytes_pair": 4 * rows * cols * 2}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
