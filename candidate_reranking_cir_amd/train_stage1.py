"""Stage-I training step: `BLIP_Retrieval.img_txt_fusion(r, t, text, train=True)` in `.train()` mode and its backward pass on the
libcirrank kernels.

What the reference does per step (stage1_train.py:144-190 FashionIQ, :383-425 CIRR; blip_stage1.py:67-92): reference-image tokens
`img_embed(ref)` (B, N, D) and normalised pooled target features `img_embed(tgt, return_pool_and_normalized=True)[-1]` (B, 256) under
no_grad (the ViT is frozen unless --blip-img-tune), then under autocast
    logits = F.normalize(text_proj(MED(ids with [ENC], mask, ref_tokens)[:, 0])) @ target^T / temp
cross-entropy against arange(B), `scaler.scale(loss).backward()`, `scaler.step(AdamW)`.  Trainable: the MED encoder layers, the word /
position embeddings and the embedding LayerNorm, text_proj and temp - 319 tensors at the real geometry.  vision_proj requires grad but only
runs under no_grad, so it receives none.

`MedTrainer` runs that forward with what the backward needs kept on the device and the backward as an explicit reverse pass, as
train.NlvrTrainer does for stage II (the shared machinery is in train_core.py: same parameter slab, dense layers, fused attention /
dropout + residual + LayerNorm kernels and their adjoints, one grouped weight-gradient launch per layer), with a single branch:
  - one attention group per query: the self-attention over its L caption rows with the key mask, the cross-attention of its L rows
    against the N tokens of ITS OWN reference image (no mask: the reference's image masks are all ones);
  - the cross K|V projection of all B * N reference tokens, cast to 16 bits once per step; its weight gradient contracts over B * N rows
    (18x the text-side products' rows at N = 577) and is split by the grouped planner; no gradient flows into the image tokens unless
    the model's `set_image_tuning()` switch is on and they require one (--blip-img-tune: `MedTrainer.backward`, `dinputs`);
  - the contrastive head on cir_contrastive_fwd / _bwd (fp32, fixed-order reductions: bit-reproducible), text_proj's forward on
    cir_linear_f32 reading the CLS rows of the fp32 stream in place and its adjoint inside cir_contrastive_bwd.
Dropout: the six sites of train_med.MedDropoutForward with the same site seeds (`train_med.site_seed`) and element numbering, one base
seed per forward drawn from torch's global CPU generator (`last_seed`): with the same base seed the masks are exactly the ones
MedDropoutForward draws.
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import ops, train_ops as T
from .engine import additive_self_mask
from .train_core import Trainer, _install_grads, draw_seed, loss_scale, train_dtype
from .train_med import SITE_CROSS_ATTN, SITE_CROSS_OUT, SITE_EMB, SITE_FFN_OUT, SITE_SELF_ATTN, SITE_SELF_OUT, site_seed

INDEX_LIMIT = 2 ** 31          # largest element count of one saved K|V / token tensor the int32-indexed paths accept


class MedTrainer(Trainer):
    """Forward (with saved activations) and backward of the stage-I MED encoder + text_proj + contrastive head for a B x Bt batch."""

    _KEY, _NAME = "stage1_train", "img_txt_fusion (stage-I train mode)"
    # Slab order (train_core.slab_order): the q, k, v weights (then biases) of each self-attention and the k, v weights (then biases) of
    # each cross-attention adjacent - ONE stacked Linear each; everything else in the model's own order
    _GROUPS = ([f"attention.self.{x}" for x in ("query", "key", "value")], [f"crossattention.self.{x}" for x in ("key", "value")])

    def __init__(self, model):
        self.model = model
        self.geo = geo = model.bert_geometry
        self.p_hidden, self.p_attn = float(geo.hidden_dropout_prob), float(geo.attention_probs_dropout_prob)
        self.dtype = train_dtype(model)
        self._nh, self._hd = geo.num_attention_heads, geo.hidden_size // geo.num_attention_heads
        self._scale = self._hd ** -0.5
        self.last_seed = None

    # ------------------------------------------------------------------------------------------------ parameters
    def _trained(self, name: str) -> bool:
        """The 319 tensors the reference's step gives a gradient (tests/golden/train_s1.npz): every encoder-layer tensor, word / position
        embeddings, the embedding LayerNorm, text_proj and temp."""
        e = self._EMB
        return name.startswith(("text_encoder.encoder.layer.", "text_proj.")) or name in (
            "temp", e + "word_embeddings.weight", e + "position_embeddings.weight", e + "LayerNorm.weight", e + "LayerNorm.bias")

    def _build_layers(self, slab, lin, ln):
        g, e = self.geo, self._EMB
        self.word, self.pos = slab.w32(e + "word_embeddings.weight"), slab.w32(e + "position_embeddings.weight")
        self.ln_e = ln(e + "LayerNorm")
        self.layers: List[Dict] = []
        for i in range(g.num_hidden_layers):
            p = f"text_encoder.encoder.layer.{i}."
            self.layers.append(dict(
                qkv=lin([p + f"attention.self.{n}" for n in ("query", "key", "value")], True),          # one 3D-wide Linear
                o=lin(p + "attention.output.dense"), ln1=ln(p + "attention.output.LayerNorm"),
                cq=lin(p + "crossattention.self.query"),
                ckv=lin([p + f"crossattention.self.{n}" for n in ("key", "value")], True),               # one 2D-wide Linear
                co=lin(p + "crossattention.output.dense"), ln2=ln(p + "crossattention.output.LayerNorm"),
                w1=lin(p + "intermediate.dense"), w2=lin(p + "output.dense"), ln3=ln(p + "output.LayerNorm")))
        self.tp_w, self.tp_b = slab.w32("text_proj.weight"), slab.w32("text_proj.bias")
        ot = slab.off["temp"]
        self.temp, self._temp_off = slab.flat32[ot:ot + 1], ot                      # (the scalar parameter's slice: read on the device)

    # ------------------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, ref_tokens: torch.Tensor, target: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                seed=None, need_dref: bool = False, need_dtarget: bool = False) -> torch.Tensor:
        """ref_tokens (B, N, Dv), target (Bt, E) normalised pooled features, ids / mask (B, L) with [ENC] set -> logits (B, Bt) fp32.
        `need_dref` / `need_dtarget`: the backward of this forward also forms the gradients of the two image-side inputs (`dinputs`)."""
        g, dt = self.geo, self.dtype
        q_n, l = input_ids.shape
        n, dv = ref_tokens.shape[1], ref_tokens.shape[2]
        d = g.hidden_size
        if ref_tokens.shape[0] != q_n:
            raise ValueError(f"img_txt_fusion: {ref_tokens.shape[0]} reference images for {q_n} captions")
        if q_n * n * max(2 * d, dv) >= INDEX_LIMIT or q_n * l * g.intermediate_size >= INDEX_LIMIT:
            raise ValueError(f"stage-I training batch too large: B * N * max(2 * hidden, width) = {q_n * n * max(2 * d, dv)} elements in one "
                             f"tensor (limit {INDEX_LIMIT - 1}: the kernels index with 32-bit offsets) - split the batch (micro-batches accumulate)")
        self._pack()
        self.last_seed = seed = draw_seed(seed)
        dev = self.word.device
        ph, pa, f32 = self.p_hidden, self.p_attn, torch.float32
        r = q_n * l
        ids = input_ids.to(dev).contiguous()
        pos = getattr(self, "_pos_idx", None)
        if pos is None or tuple(pos.shape) != (q_n, l):                             # position of every row (built once per batch shape)
            pos = self._pos_idx = torch.arange(l, device=dev).repeat(q_n, 1)
        pos = pos.view(-1)
        self.sv = sv = {"ids": ids, "q_n": q_n, "l": l, "n": n, "seed": seed, "need_dref": bool(need_dref), "need_dtarget": bool(need_dtarget)}
        # BertEmbeddings (med.py:87-108): LayerNorm(word + position), dropout
        pre_e = T.eltwise(ops.gather_rows(self.word, ids.view(-1), f32), T.MODE_ADD, ops.gather_rows(self.pos, pos, f32))
        h32, h16 = self.ln_e.fwd(pre_e, dt)
        if ph > 0:
            h32 = T.eltwise(h32, T.MODE_DROPOUT, p_drop=ph, seed=site_seed(seed, 0, SITE_EMB))
            h16 = T.eltwise(h32, T.MODE_SCALE, out_dtype=dt, p_drop=1.0)
        sv["pre_e"] = pre_e
        smask = additive_self_mask(attention_mask.to(dev)).view(q_n, l)
        enc = ref_tokens.to(dev).reshape(q_n * n, dv)
        enc16 = enc if enc.dtype == dt else ops.gather_rows(enc, None, dt)            # the image tokens in 16 bits, once per step
        sv.update(smask=smask, enc16=enc16, layers=[])
        for i, ly in enumerate(self.layers):
            s = {"h16": h16}
            # self-attention: group = query, its L caption rows, key mask (med.py:193-235, dropout :225)
            qkv = ly["qkv"].fwd(h16, dt)
            ctx, ctx32 = torch.empty((r, d), dtype=dt, device=dev), torch.empty((r, d), dtype=f32, device=dev)
            s["sa"] = T.attention_train_fwd(*(self._heads(qkv, q_n, l, j, 3) for j in range(3)), smask, self._heads(ctx, q_n, l), self._scale, pa,
                                            site_seed(seed, i, SITE_SELF_ATTN), out32=self._heads(ctx32, q_n, l))
            pre1, a32, a16 = ly["ln1"].fwd_res(ly["o"].fwd(ctx, f32), None, h32, dt, 1.0, ph, site_seed(seed, i, SITE_SELF_OUT))   # med.py:250-253
            # cross-attention: group = query, its L rows against the N tokens of its own reference image (med.py:361-376)
            cq = ly["cq"].fwd(a16, dt)
            kv = ly["ckv"].fwd(enc16, dt)                                               # (B N, 2D)
            cx, cx32 = torch.empty((r, d), dtype=dt, device=dev), torch.empty((r, d), dtype=f32, device=dev)
            s["ca"] = T.attention_train_fwd(self._heads(cq, q_n, l), self._heads(kv, q_n, n, 0, 2), self._heads(kv, q_n, n, 1, 2), None,
                                            self._heads(cx, q_n, l), self._scale, pa, site_seed(seed, i, SITE_CROSS_ATTN), out32=self._heads(cx32, q_n, l))
            pre2, c32, c16 = ly["ln2"].fwd_res(ly["co"].fwd(cx, f32), None, a32, dt, 1.0, ph, site_seed(seed, i, SITE_CROSS_OUT))
            # FFN (med.py:319-335): the dense output in the operand type, GELU, dense, dropout + residual + LayerNorm
            z16 = ly["w1"].fwd(c16, dt)
            f16 = T.eltwise(z16, T.MODE_GELU, out_dtype=dt)
            pre3, h32, h16 = ly["ln3"].fwd_res(ly["w2"].fwd(f16, f32), None, c32, dt, 1.0, ph, site_seed(seed, i, SITE_FFN_OUT))
            s.update(qkv=qkv, ctx=ctx, ctx32=ctx32, pre1=pre1, a16=a16, cq=cq, kv=kv, cx=cx, cx32=cx32, pre2=pre2, c16=c16, z16=z16, f16=f16, pre3=pre3)
            sv["layers"].append(s)
        # head (blip_stage1.py:83-91): text_proj of the CLS rows (read in place, row stride L * D), normalise, / temp
        cls = h32.view(q_n, l * d)[:, :d]
        p = ops.linear_f32(cls, self.tp_w, self.tp_b)
        tgt = target.to(dev)
        tgt = tgt if tgt.dtype == f32 and tgt.is_contiguous() else tgt.float().contiguous()
        p_hat, inv, logits = T.contrastive_fwd(p, tgt, self.temp)
        sv.update(cls=cls, p_hat=p_hat, inv=inv, target=tgt)
        return logits

    # ------------------------------------------------------------------------------------------------ backward
    @torch.no_grad()
    def backward(self, dlogits: torch.Tensor) -> Dict[str, torch.Tensor]:
        """dlogits (B, Bt) fp32 -> {parameter name: fp32 gradient} for the 319 trained tensors.  Where the forward asked for them, the
        gradients of the image-side inputs are left in `dinputs` = (d ref_tokens (B, N, Dv) | None, d target (Bt, E) | None), fp32 and
        UNSCALED: d ref_tokens = sum over the layers of dkv16_l W_ckv,l - the cross K|V dgrad product of every layer, layers 11 -> 0, each
        adding to the running fp32 sum in its GEMM epilogue (one adder per element, fixed order) -, d target from
        cir_contrastive_bwd_target (blip_stage1.py:91)."""
        sv, g, dt, slab = self.sv, self.geo, self.dtype, self.slab
        det = slab.read_mode()                                                      # {} or the fixed-order forms' workspace (deterministic mode)
        dev = dlogits.device
        q_n, l, n, d, seed = sv["q_n"], sv["l"], sv["n"], g.hidden_size, sv["seed"]
        r = q_n * l
        ph, pa = self.p_hidden, self.p_attn
        # the power-of-two loss scale of NlvrTrainer.backward (fp16 operands: intermediate gradients in fp16's normal range; bf16: none)
        self.grad_scale = loss_scale(float(dlogits.abs().max())) if dt == torch.float16 else 1.0
        dl = dlogits.contiguous().float()
        if self.grad_scale != 1.0:
            dl = T.eltwise(dl, T.MODE_SCALE, p_drop=self.grad_scale)
        # head adjoint: dtemp written into temp's slice, text_proj's gradients into theirs, dCLS into the CLS rows of the stream gradient
        dh = torch.zeros((r, d), dtype=torch.float32, device=dev)
        T.contrastive_bwd(dl, sv["target"], self.temp, sv["p_hat"], sv["inv"], slab.gflat[self._temp_off:self._temp_off + 1], x=sv["cls"], w=self.tp_w,
                          dx=dh.view(q_n, l * d)[:, :d], dw=slab.grad("text_proj.weight"), db=slab.grad("text_proj.bias"))
        enc16 = sv["enc16"]
        need_dref = sv["need_dref"]
        dtarget = T.contrastive_bwd_target(dl, sv["p_hat"], self.temp) if sv["need_dtarget"] else None
        dref = None                                                                 # running sum over the layers (B N, Dv) fp32
        for i in reversed(range(len(self.layers))):
            ly, s = self.layers[i], sv["layers"][i]
            wq: list = []                                                           # this layer's weight gradients: ONE launch at its end
            dpre3, do16 = ly["ln3"].bwd_res(s["pre3"], dh, dt, dbias=ly["w2"].db, p_drop=ph, seed=site_seed(seed, i, SITE_FFN_OUT))
            df16 = ly["w2"].bwd16(s["f16"], do16, dx_dtype=dt, queue=wq)
            dz16 = T.gelu_bwd16(df16, s["z16"], sums=ly["w1"].db, **det)
            dc = ly["w1"].bwd16(s["c16"], dz16, residual=dpre3, queue=wq)          # fp32: FFN branch + skip
            dpre2, dd16 = ly["ln2"].bwd_res(s["pre2"], dc, dt, dbias=ly["co"].db, p_drop=ph, seed=site_seed(seed, i, SITE_CROSS_OUT))
            dcx16 = ly["co"].bwd16(s["cx"], dd16, dx_dtype=dt, queue=wq)
            dcq16 = torch.empty((r, d), dtype=dt, device=dev)
            dkv16 = torch.empty((q_n * n, 2 * d), dtype=dt, device=dev)
            kv = s["kv"]
            T.attention_train_bwd(self._heads(s["cq"], q_n, l), self._heads(kv, q_n, n, 0, 2), self._heads(kv, q_n, n, 1, 2), None,
                                  self._heads(s["cx"], q_n, l), self._heads(dcx16, q_n, l), s["ca"], self._heads(dcq16, q_n, l),
                                  self._heads(dkv16, q_n, n, 0, 2), self._heads(dkv16, q_n, n, 1, 2), self._scale, pa,
                                  site_seed(seed, i, SITE_CROSS_ATTN), out32=self._heads(s["cx32"], q_n, l))
            if need_dref:                                                           # B N rows; dkv16 W_ckv joins the image tokens' gradient
                dref = ly["ckv"].bwd16(enc16, dkv16, need_dx=True, bias=True, residual=dref, queue=wq)
            else:                                                                   # no gradient into the (frozen) image tokens
                ly["ckv"].bwd16(enc16, dkv16, need_dx=False, bias=True, queue=wq)
            da = ly["cq"].bwd16(s["a16"], dcq16, bias=True, residual=dpre2, queue=wq)
            dpre1, dt16 = ly["ln1"].bwd_res(s["pre1"], da, dt, dbias=ly["o"].db, p_drop=ph, seed=site_seed(seed, i, SITE_SELF_OUT))
            dctx16 = ly["o"].bwd16(s["ctx"], dt16, dx_dtype=dt, queue=wq)
            qkv = s["qkv"]
            dqkv16 = torch.empty((r, 3 * d), dtype=dt, device=dev)
            T.attention_train_bwd(*(self._heads(qkv, q_n, l, j, 3) for j in range(3)), sv["smask"], self._heads(s["ctx"], q_n, l),
                                  self._heads(dctx16, q_n, l), s["sa"], *(self._heads(dqkv16, q_n, l, j, 3) for j in range(3)), self._scale, pa,
                                  site_seed(seed, i, SITE_SELF_ATTN), out32=self._heads(s["ctx32"], q_n, l))
            dh = ly["qkv"].bwd16(s["h16"], dqkv16, bias=True, residual=dpre1, queue=wq)
            self._wgrad_grouped(wq)
        de = dh if ph <= 0 else T.eltwise(dh, T.MODE_DROPOUT, p_drop=ph, seed=site_seed(seed, 0, SITE_EMB))
        T.embed_bwd(sv["ids"].view(-1), self.ln_e.bwd(sv["pre_e"], de), self.dword, self.dpos, l, **det)
        # the pass ran on grad_scale * dlogits (fp16 operands): the power of two is divided out of the input gradients as _finish_backward
        # divides it out of the parameters' before they return to autograd
        if self.grad_scale != 1.0:
            dref, dtarget = (None if x is None else T.eltwise(x, T.MODE_SCALE, p_drop=1.0 / self.grad_scale) for x in (dref, dtarget))
        self.dinputs = (None if dref is None else dref.view(q_n, n, -1), dtarget)
        self.sv = None                                                              # (the saved activations are released with the pass)
        return self._finish_backward()


class _Stage1TrainFn(torch.autograd.Function):
    """One autograd node around MedTrainer.forward / backward (train._FusionTrainFn's contract): the parameters' gradients are accumulated
    into `.grad` directly; `anchor` only makes the node differentiable."""

    @staticmethod
    def forward(ctx, anchor, trainer, ref_tokens, target, ids, mask):
        ctx.trainer = trainer
        need = ctx.needs_input_grad
        ctx.in_meta = [(t.dtype, t.device, tuple(t.shape)) for t in (ref_tokens, target)]
        out = trainer.forward(ref_tokens, target, ids, mask, need_dref=need[2], need_dtarget=need[3])
        trainer._claim(ctx)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        tr = ctx.trainer
        tr._consume(ctx)
        _install_grads(tr, tr.backward(dlogits.contiguous().float()))
        dins, tr.dinputs = tr.dinputs, (None, None)
        dins = [None if gq is None else gq.to(device=dev, dtype=dt).view(shape) for gq, (dt, dev, shape) in zip(dins, ctx.in_meta)]
        return None, None, dins[0], dins[1], None, None


class _PooledHeadFn(torch.autograd.Function):
    """One autograd node around cir_pooled_head_fwd / _bwd: F.normalize(vision_proj(tokens[:, 0])) (blip_stage1.py:57).  The CLS rows are
    read in place; the backward ADDS vision_proj's gradients into `.grad` directly (as the trainers' nodes do: the `blip_bs` mini-batches of
    a step each contribute) and returns the token gradient - zero but for the CLS rows, which the kernel writes."""

    @staticmethod
    def forward(ctx, tokens, weight, bias):
        t_hat, inv = T.pooled_head_fwd(tokens[:, 0], weight.detach(), bias.detach())
        ctx.weight, ctx.bias = weight, bias
        ctx.save_for_backward(tokens, t_hat, inv)
        return t_hat

    @staticmethod
    def backward(ctx, dt_hat):
        tokens, t_hat, inv = ctx.saved_tensors
        weight, bias = ctx.weight, ctx.bias
        sums = []
        for p in (weight, bias):                                                    # the kernel adds into .grad where it can
            ok = p.requires_grad and p.grad is not None and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.data_ptr() % 16 == 0
            sums.append(p.grad if ok else torch.zeros(p.shape, dtype=torch.float32, device=tokens.device))
        dtok = torch.zeros_like(tokens) if ctx.needs_input_grad[0] else None       # the rows the kernel does not write: zeroed here
        T.pooled_head_bwd(dt_hat.contiguous().float(), t_hat, inv, tokens[:, 0], weight.detach(), sums[0], sums[1], None if dtok is None else dtok[:, 0])
        for p, s in zip((weight, bias), sums):
            if p.requires_grad and p.grad is not s:
                p.grad = s if p.grad is None else T.eltwise(p.grad.contiguous().float(), T.MODE_ADD, s)
        return dtok, None, None


def pooled_head_train(tokens: torch.Tensor, weight: torch.nn.Parameter, bias: torch.nn.Parameter) -> torch.Tensor:
    """(Bt, E) normalised pooled features of (Bt, N, Dv) fp32 tokens with a graph into vision_proj and into the tokens' CLS rows."""
    if tokens.dtype != torch.float32 or not tokens.is_contiguous() or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError("pooled head (train mode): fp32 contiguous tokens and an fp32 vision_proj are required")
    return _PooledHeadFn.apply(tokens, weight, bias)


def _refuse_image_grads(*tensors):
    if any(torch.is_tensor(t) and t.requires_grad for t in tensors):
        raise NotImplementedError("stage-I training with image features that require a gradient (stage1_train.py --blip-img-tune) is not "
                                  "supported: the reverse pass stops at the frozen ViT's tokens and pooled features - compute them under "
                                  "torch.no_grad(), as the reference's default loop does (stage1_train.py:157-164)")


def stage1_train(model, ref_tokens, target, ids, mask) -> torch.Tensor:
    """(B, Bt) logits of `BLIP_Retrieval.img_txt_fusion(..., train=True)` in training mode, differentiable w.r.t. the 319 trained tensors -
    and, on a model with `set_image_tuning()` on, w.r.t. `ref_tokens` and `target` where they require a gradient."""
    if not getattr(model, "image_tuning", False):
        _refuse_image_grads(ref_tokens, target)
    tr = getattr(model, "_trainer", None)
    g = model.bert_geometry
    if (not isinstance(tr, MedTrainer) or tr.dtype != train_dtype(model)
            or (tr.p_hidden, tr.p_attn) != (float(g.hidden_dropout_prob), float(g.attention_probs_dropout_prob))):
        tr = model._trainer = MedTrainer(model)
        tr.anchor = torch.zeros((1,), device=model.device, requires_grad=True)
    return _Stage1TrainFn.apply(tr.anchor, tr, ref_tokens, target, ids, mask)
