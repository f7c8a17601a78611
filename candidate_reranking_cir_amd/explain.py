"""What a stage-II score rests on: the cross-attention maps of the two-branch encoder and their Grad-CAM.

The reference's cross-attention modules carry `save_attention`, `get_attention_map()` and `get_attn_gradients()`
(nlvr_encoder.py:121-134, filled at :199-203 with the probabilities after the softmax and before the dropout, and a hook for their
gradient; med.py and vit.py have the same surface).  Here every attention kernel is fused - no probability tensor exists in memory - so the
maps come from a kernel of their own (csrc/attn_maps.hip: cir_attention_maps / cir_attention_gradcam), fed by the training pass:

    `NlvrTrainer` with p_hidden = p_attn = 0 is the dropout-free forward with every cross-attention's q, k | v and log-sum-exp saved, and
    its reverse pass forms the gradient of each cross-attention's context; an observer (train.NlvrTrainer.backward) taps it there and ends
    the pass at the lowest layer asked for.  The pairs (query i, candidate j) do not interact, so ONE reverse pass from dlogits = ones gives
    every pair the gradient of its own logit; the pass's fp16 loss scale S, a power of two, is removed exactly (dmul = 1 / S).

Contract.  The maps belong to the TRAINING arithmetic - 16-bit operands of `train_dtype(model)`, fp32 statistics, dropout off - not to the
model's inference precision mode; `logits` is returned so that a caller sees the distance to the engine's scores.  `model.training` is not
touched.  A call leaves a training run exactly as it found it: the `.grad` tensors, the optimizer state, the slab's tested-buffer mark, the
trainer's saved activations, step count, claim state, finite flag, loss scale and the pending counters - it re-uses the model's trainer and
slab (a second slab would re-point every parameter), works in a gradient buffer of its own that is never installed into `.grad`, and puts
every slot back.  Between a training forward and its backward a call raises RuntimeError (the saved activations are that forward's); the
backward still works afterwards.  Stage-I maps (the MED encoder) and ViT self-attention maps are not covered.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import train_ops as T

_SLOTS = ("sv", "step_no", "generation", "consumed", "grads_finite", "grad_scale", "dfeats", "dfeats_scale", "need_dfeats", "p_hidden", "p_attn")
_MISSING = object()


@dataclass
class CrossAttentionMaps:
    """logits (B, Bt): the pass's own logits.  probs[layer] (2, B, Bt, H, L, N) fp32: branch, query, candidate, head, caption token, image
    token - views of the kernel's output, not copies.  grads[layer]: the same shape, d logits[i, j] / d probs, or None."""
    logits: torch.Tensor
    probs: Dict[int, torch.Tensor]
    grads: Optional[Dict[int, torch.Tensor]]


def _trainer(model, device):
    """The model's trainer as it is - whatever its dropout probabilities: the pass below switches them off and puts them back - or, for a
    model that has not trained yet, the one `img_txt_fusion` would build."""
    from .train import model_trainer, train_dtype
    tr = getattr(model, "_trainer", None)
    if tr is not None and tr.dtype == train_dtype(model):
        return tr
    g = model.bert_geometry
    return model_trainer(model, g.hidden_dropout_prob, g.attention_probs_dropout_prob, 0, device)


def _run(model, z_t, feats, text, layers: Sequence[int], tap):
    """One dropout-free forward and the reverse pass from dlogits = ones down to min(layers) on the model's trainer, `tap(layer, q4, k4, v4,
    dout4, lse, dmul, b, bt, l, n)` called at each layer of `layers`; every slot of the trainer and the slab is restored.  -> logits."""
    from .blip_stage2 import encode_text
    z = z_t.last_hidden_state if hasattr(z_t, "last_hidden_state") else z_t
    dev = model.device
    if dev.type != "cuda":
        raise RuntimeError("attention maps run on an MI355X only: move the model to 'cuda' (no CPU path)")
    ids, mask = encode_text(model.tokenizer, text, dev)
    n_layers = model.bert_geometry.num_hidden_layers
    layers = sorted({int(x) for x in layers})
    if not layers or layers[0] < 0 or layers[-1] >= n_layers:
        raise ValueError(f"layers {layers}: the two-branch encoder has layers 0 .. {n_layers - 1}")
    tr = _trainer(model, dev)
    if getattr(tr, "generation", 0) and not tr.consumed:
        raise RuntimeError("attention maps asked for between a training-mode forward and its backward: the trainer's saved activations belong "
                           "to that forward.  Call backward() first (or run the forward under torch.no_grad() / in .eval() mode)")
    slab = getattr(tr, "slab", None)
    keep = {k: tr.__dict__.get(k, _MISSING) for k in _SLOTS}
    keep_slab = None if slab is None else (slab, slab.gflat, slab.checked, slab.work)
    b, bt = ids.shape[0], feats.shape[0]

    def observer(layer, dc16, q4, k4, v4, saved):
        if layer in layers:
            l, n = q4.shape[2] // b, k4.shape[2]
            tap(layer, q4, k4, v4, tr._heads(dc16.view(-1, dc16.shape[-1]), 2 * bt, b * l), saved[0], 1.0 / tr.grad_scale, b, bt, l, n)
        return layer <= layers[0]

    try:
        tr.p_hidden = tr.p_attn = 0.0
        tr.need_dfeats = False
        with torch.no_grad():
            logits = tr.forward(z.to(dev), feats.to(dev), ids, mask)
            tr.backward(torch.ones((b, bt), dtype=torch.float32, device=dev), observer=observer)
    finally:
        for k, v in keep.items():
            if v is _MISSING:
                tr.__dict__.pop(k, None)
            else:
                setattr(tr, k, v)
        if keep_slab is not None and keep_slab[0] is tr.slab:       # (a slab built by this call has nothing to put back)
            slab.gflat, slab.checked, slab.work = keep_slab[1:]
            if slab.gflat is not None:
                tr._bind_grads(slab)
    return logits


def cross_attention_maps(model, z_t, feats, text, layers: Sequence[int], grads: bool = True) -> CrossAttentionMaps:
    """Cross-attention probabilities - and, with `grads`, the gradient of each pair's logit w.r.t. them - of B queries (z_t (B, L, D), `text`:
    the caption list, tokenised as `img_txt_fusion` does it, [ENC] set) against Bt candidates (feats (Bt, N, Dv)) at the fusion layers
    `layers`: what `get_attention_map()` / `get_attn_gradients()` of crossattention.self0 / self1 return in the reference
    (nlvr_encoder.py:121-134, 199-203), for every pair at once."""
    probs: Dict[int, torch.Tensor] = {}
    dprobs: Dict[int, torch.Tensor] = {}

    def tap(layer, q4, k4, v4, dout4, lse, dmul, b, bt, l, n):
        p, g = T.attention_maps(q4, k4, v4, None, dout4, lse, dmul=dmul, grads=grads)
        shape = lambda x: x.unflatten(2, (b, l)).unflatten(0, (2, bt)).permute(0, 3, 1, 2, 4, 5)      # noqa: E731  (2, Bt, H, B, L, N) -> (2, B, Bt, H, L, N)
        probs[layer] = shape(p)
        if grads:
            dprobs[layer] = shape(g)

    logits = _run(model, z_t, feats, text, layers, tap)
    return CrossAttentionMaps(logits=logits, probs=probs, grads=dprobs if grads else None)


def gradcam(model, z_t, feats, text, layer: int) -> torch.Tensor:
    """Grad-CAM of fusion layer `layer`: (2, B, Bt, L, N) fp32, the mean over the heads of probs * max(grads, 0) of `cross_attention_maps`,
    summed inside the kernel (cir_attention_gradcam): no (.., H, L, N) tensor is made."""
    out = []

    def tap(_layer, q4, k4, v4, dout4, lse, dmul, b, bt, l, n):
        cam = T.attention_gradcam(q4, k4, v4, None, dout4, lse, dmul=dmul)                            # (2 Bt, B L, N)
        out.append(cam.unflatten(1, (b, l)).unflatten(0, (2, bt)).permute(0, 2, 1, 3, 4))

    _run(model, z_t, feats, text, (layer,), tap)
    return out[0]


def patch_grid(x: torch.Tensor) -> torch.Tensor:
    """Drop the CLS key and lay the image tokens out as the ViT's patch grid: (..., N) -> (..., g, g) with N - 1 = g * g."""
    n = x.shape[-1] - 1
    g = math.isqrt(n) if n > 0 else 0
    if n <= 0 or g * g != n:
        raise ValueError(f"patch_grid: {x.shape[-1]} keys are not a CLS token plus a square patch grid")
    return x[..., 1:].unflatten(-1, (g, g))
