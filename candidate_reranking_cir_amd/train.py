"""Training-mode `img_txt_fusion` and its backward pass on the libcirrank kernels.

What the reference does per step (stage2_train.py:202-216): z_t from the frozen stage-I model, image tokens from the (by default
frozen) ViT, then under autocast `logits = model.img_txt_fusion(z_t, target_feats, captions, train=True)` - the B x B surface of
blip_stage2.py:65-99: row i's caption / z_t expanded to B rows against all B targets - cross-entropy against arange(B),
`loss.backward()`, AdamW.  Trainable: the two-branch BERT (`text_encoder.*`) and `cls_head.*`.

`NlvrTrainer` runs that forward with every intermediate the backward needs kept on the device, and the backward as an explicit
reverse pass - no autograd graph over the kernels: each step of nlvr_encoder.BertLayer.forward (:414-476), BertSelfAttention
(:140-222), BertSelfOutput (:248-264, incl. the averaging / merge_layer variants), BertIntermediate / BertOutput (:383-409),
BertEmbeddings (:49-91) and cls_head (blip_stage2.py:50-54) has its hand-written adjoint below.  Arithmetic:
dense layers forward / dgrad on the MFMA GEMM (`ops.gemm`; dgrad over a transposed weight copy, the skip connection's fp32 gradient
added in its epilogue); the 13 weight gradients of a layer in ONE grouped launch (`train_ops.wgrad_grouped`: dy and x read as stored,
no row splits, no atomics); attention as one fused kernel with a log-sum-exp output and a recomputing adjoint whose dq | dk | dv come
out as the 16-bit operand of the fused projection's backward; each dense -> dropout -> + residual -> LayerNorm block as one pass per
direction (`residual_layernorm_train` / `layernorm_bwd_fused`, the latter also emitting the dense branch's 16-bit gradient and bias
sums); GELU's adjoint with the bias sums in one 16-bit pass.  Triplets are ordered candidate-major, so the cross-attention keys /
values of a target image are projected once per step and their gradients sum over the B queries inside the dK / dV kernel.
Precision: 16-bit MFMA operands (activations, weights, and every gradient between two dense layers), fp32 accumulation, fp32 residual
stream and its gradient, fp32 LayerNorm inputs, fp32 weight gradients.
Dropout is counter-based (seed per site); with p = 0 the pass has no random state - reproducible up to the order of the fp32 atomic adds in
the column sums / LayerNorm and embedding adjoints - and is what the reference-gradient fixtures pin.  `set_deterministic(True)` (process-wide,
off by default, read at the start of every backward of the three passes) replaces those atomics by the fixed-order forms of include/cirrank.h:
the gradients then repeat bit for bit.

`fusion_train(model, ...)` wraps the pair as ONE `torch.autograd.Function`, so the reference's training step runs unchanged:
`logits = model.img_txt_fusion(z_t, feats, captions)` in `.train()` mode, `loss = F.cross_entropy(logits, gt)`, `loss.backward()`
fills `.grad` of every trainable parameter (accumulating, as autograd does); `AdamW` (train_optim.py, re-exported here) is torch.optim.AdamW's
update on `cir_adamw_step`.  The slab, the layer views and the trainer base both other passes share are in train_core.py.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops, train_ops as T
from .train_core import (Trainer, _Lin, _Lin2, _cast, _install_grads, _row_split, apply_pending_counters, load_training_state,  # noqa: F401
                         loss_scale, train_dtype, training_state)                                                             # (re-exported)
from .train_optim import AdamW, cosine_lr_schedule, exp_lr_schedule, step_lr_schedule, warmup_lr_schedule  # noqa: F401  (re-exported)
from .train_ops import deterministic, set_deterministic  # noqa: F401  (re-exported: the deterministic training mode)
from .train_vit import vit_checkpointed_blocks, vit_saved_bytes  # noqa: F401  (re-exported: ViT gradient checkpointing)


class NlvrTrainer(Trainer):
    """Forward (with saved activations) and backward of the two-branch encoder + cls_head for a B x Bt training batch: B queries against Bt
    target images (Bt = B: the reference's step; Bt > B: extra negatives; B = 1: one query against its candidates, the shape of
    img_txt_fusion_val, which explain.py runs)."""

    _KEY, _NAME = "text", "img_txt_fusion (train mode)"
    # Slab order (train_core.slab_order): per layer the twin (branch 0 | branch 1) dense layers as adjacent groups - all weights of a group,
    # then its biases - so that (a) the q, k, v projections of one self-attention (k, v of one cross-attention) are ONE stacked Linear and
    # (b) the two branches' Linears of one kind sit a constant stride apart: one BATCHED GEMM serves both (`_Lin2`)
    _GROUPS = ([f"attention.self{b}.{x}" for b in (0, 1) for x in ("query", "key", "value")],
               [f"crossattention.self{b}.{x}" for b in (0, 1) for x in ("key", "value")],
               [f"crossattention.self{b}.query" for b in (0, 1)],
               [f"attention.output.dense{b}" for b in (0, 1)],
               [f"crossattention.output.dense{b}" for b in (0, 1)])

    def __init__(self, model, p_hidden: float = 0.1, p_attn: float = 0.1, seed: int = 0):
        self.model, self.p_hidden, self.p_attn, self.seed = model, float(p_hidden), float(p_attn), int(seed)
        self.geo = model.bert_geometry
        self.dtype = train_dtype(model)
        self.step_no = 0
        self._nh, self._hd = self.geo.num_attention_heads, self.geo.hidden_size // self.geo.num_attention_heads
        self.need_dfeats = False          # blip_img_tune (stage2_train.py:183-199): also return the gradient of the target image tokens
        self.dfeats = self.dfeats_scale = None
        self._scale = self._hd ** -0.5

    # ------------------------------------------------------------------------------------------------ parameters
    def _trained(self, name: str) -> bool:
        """The parameters the reference's step gives a gradient (tests/golden/train768.npz: 572 of them): every encoder-layer and
        cls_head tensor, word / position embeddings and the embedding LayerNorm (token-type embeddings and the pooler are unused)."""
        e = self._EMB
        return name.startswith(("text_encoder.encoder.layer.", "cls_head.")) or name in (
            e + "word_embeddings.weight", e + "position_embeddings.weight", e + "LayerNorm.weight", e + "LayerNorm.bias")

    def _build_layers(self, slab, lin, ln):
        grp = lambda names: lin(names, True)
        e = self._EMB
        self.word, self.pos = slab.w32(e + "word_embeddings.weight"), slab.w32(e + "position_embeddings.weight")
        self.ln_e = ln(e + "LayerNorm")
        self.layers: List[Dict] = []
        for i in range(self.geo.num_hidden_layers):
            p = f"text_encoder.encoder.layer.{i}."
            ly = {}
            for b in (0, 1):
                ly[f"qkv{b}"] = grp([p + f"attention.self{b}.{n}" for n in ("query", "key", "value")])     # one 2304-wide Linear
                ly[f"o{b}"] = lin(p + f"attention.output.dense{b}")
                ly[f"cq{b}"] = lin(p + f"crossattention.self{b}.query")
                ly[f"ckv{b}"] = grp([p + f"crossattention.self{b}.{n}" for n in ("key", "value")])           # one 1536-wide Linear
                ly[f"d{b}"] = lin(p + f"crossattention.output.dense{b}")
            for kind in ("qkv", "o", "cq", "ckv", "d"):                                # the twins as one batched GEMM each
                ly[kind] = _Lin2(ly[kind + "0"], ly[kind + "1"])
            for c, b in (("A", 0), ("B", 1)):
                ly[f"ln1{b}"] = ln(p + f"attention.output.LayerNorm{c}")
                ly[f"ln2{b}"] = ln(p + f"crossattention.output.LayerNorm{c}")
            mk = p + "crossattention.output.merge_layer"
            ly["merge"] = lin(mk) if (mk + ".weight") in slab.off else None
            ly["w1"], ly["w2"], ly["ln3"] = lin(p + "intermediate.dense"), lin(p + "output.dense"), ln(p + "output.LayerNorm")
            self.layers.append(ly)
        self.c0, self.c2 = lin("cls_head.0"), lin("cls_head.2")

    def _site(self, *ids) -> int:
        s = self.seed * 1000003 + self.step_no * 7919
        for v in ids:
            s = s * 131 + int(v) + 1
        return s & (2 ** 62 - 1)

    def _drop(self, x: torch.Tensor, site: int) -> torch.Tensor:
        return x if self.p_hidden <= 0 else T.eltwise(x, T.MODE_DROPOUT, p_drop=self.p_hidden, seed=site)

    # ------------------------------------------------------------------------------------------------ attention
    def _attn_fwd(self, q4, k4, v4, mask, site, ctx, ctx32):
        """q4 (G, H, mq, hd), k4 / v4 (G, H, mk, hd) head views of 16-bit projections: G groups of mq query rows and mk key rows;
        mask (groups, mk) additive fp32, one row per mq * H score rows, or None.  Self-attention: a group is a triplet;
        cross-attention: a group is a CANDIDATE with the B queries scored against it stacked in mq = B * L rows - its keys /
        values exist once.  ONE kernel - scores, mask, softmax, dropout, P.V tile by tile in registers - and a log-sum-exp per row
        for the recomputing backward; no score / probability tensor is materialised (cir_attention_train_fwd; head dimension 64,
        which config.BertGeometry enforces).  Writes the context into `ctx` (G*mq, D) 16-bit and its fp32 twin `ctx32` (the backward's
        D = rowsum(dO * O), cirrank.h); returns what the adjoint needs."""
        nb1, h_n, mq, _ = q4.shape
        lse = T.attention_train_fwd(q4, k4, v4, mask, self._heads(ctx, nb1, mq), self._scale, self.p_attn, site, out32=self._heads(ctx32, nb1, mq))
        return (lse, mask, site, ctx, ctx32)

    def _attn_bwd(self, dctx16, q4, k4, v4, saved, dq4, dk4, dv4):
        """dctx16 (G*mq, D) in the operand type -> dq4 / dk4 / dv4: head views (same type) of the buffer the fused projection's
        backward reads as its dy operand."""
        nb1, h_n, mq, _ = q4.shape
        lse, mask, site, ctx, ctx32 = saved
        T.attention_train_bwd(q4, k4, v4, mask, self._heads(ctx, nb1, mq), self._heads(dctx16, nb1, mq), lse, dq4, dk4, dv4,
                              self._scale, self.p_attn, site, out32=self._heads(ctx32, nb1, mq))

    # ------------------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, z_t: torch.Tensor, feats: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """z_t (B, L, D) fp32, feats (Bt, N, Dv), ids / mask (B, L) with [ENC] set -> logits (B, Bt) fp32; keeps what backward needs."""
        self._pack()
        self.step_no += 1
        g, dt, dev = self.geo, self.dtype, z_t.device
        b_n, l = input_ids.shape
        bt_n, n, d = feats.shape[0], feats.shape[1], g.hidden_size
        t_n = b_n * bt_n
        r = t_n * l
        ph = self.p_hidden
        f32 = torch.float32
        # triplet t = j * B + i scores query i (caption, z_t) against target j - candidate-major, so that the B queries of one
        # target are consecutive rows and its cross-attention keys / values are projected ONCE (the reference recomputes them
        # for every query, blip_stage2.py:80-92; same values); the (Bt_j, B_i) result is transposed on the way out
        qi = torch.arange(b_n, device=dev).repeat(bt_n)
        ids_t = input_ids.to(dev)[qi].contiguous()                                  # (T, L)
        self.sv = sv = {"ids": ids_t, "t_n": t_n, "l": l, "n": n, "b_n": b_n, "bt_n": bt_n}
        # embeddings (BertEmbeddings: LayerNorm(word + pos), dropout) -> branch 1; z_t -> branch 0 (nlvr_encoder.py:880-892)
        pos_idx = torch.arange(l, device=dev).repeat(t_n)
        pre_e = T.eltwise(ops.gather_rows(self.word, ids_t.view(-1), f32), T.MODE_ADD, ops.gather_rows(self.pos, pos_idx, f32))
        sv["pre_e"] = pre_e
        e32, _ = self.ln_e.fwd(pre_e, dt)
        e32 = self._drop(e32, self._site(9000))
        # Both branches live in ONE (2, R, .) tensor per activation: the twin dense layers are then one batched GEMM each (`_Lin2`), and the
        # shared FFN reads the same memory as its 2R stacked rows.
        h32 = torch.empty((2, r, d), dtype=f32, device=dev)
        h32[0].copy_(ops.gather_rows(z_t.to(dev).float().contiguous().view(b_n, l * d), qi, f32).view(r, d))
        h32[1].copy_(e32)
        h16 = _cast(h32, dt)
        cand16 = _cast(feats.to(dev).float().contiguous(), dt).view(bt_n * n, -1)                         # (Bt*N, Dv): each target once
        sv["cand16"] = cand16
        cand2 = cand16.unsqueeze(0).expand(2, bt_n * n, cand16.shape[1])                                   # one input, two branches (batch stride 0)
        smask = ((1.0 - attention_mask.to(dev).float()) * -10000.0)[qi].contiguous()                      # (T, L), nlvr_encoder.py:773-774
        smask2 = smask.repeat(2, 1)                                                                       # the same key masks for both branches' groups
        sv["layers"] = []
        for i, ly in enumerate(self.layers):
            s = {"h16": h16}
            qkv = ly["qkv"].fwd(h16, dt)                                              # (2, R, 3D): one batched GEMM for both branches
            ctx = torch.empty((2, r, d), dtype=dt, device=dev)
            ctx32 = torch.empty((2, r, d), dtype=f32, device=dev)                     # fp32 twin of the context: the backward's D = rowsum(dO * O)
            # both branches' self-attentions in ONE launch: group = (branch, triplet) - 2T groups of 32 x 32 one-tile problems fill the
            # chip better than T (3072 waves are 3 per SIMD), and the dropout rows of the two branches are distinct rows of one site
            s["sa"] = self._attn_fwd(*(self._heads(qkv.view(2 * r, 3 * d), 2 * t_n, l, j, 3) for j in range(3)), smask2, self._site(i, 0, 1),
                                     ctx.view(2 * r, d), ctx32.view(2 * r, d))
            # BertSelfOutput (nlvr_encoder.py:399-409): LayerNorm(dropout(dense(ctx)) + h) - dropout, sum and LayerNorm in one pass per branch
            t = ly["o"].fwd(ctx, f32)
            pre1, a32, a16 = torch.empty((2, r, d), dtype=f32, device=dev), torch.empty((2, r, d), dtype=f32, device=dev), torch.empty((2, r, d), dtype=dt, device=dev)
            for b in (0, 1):
                ly[f"ln1{b}"].fwd_res(t[b], None, h32[b], dt, 1.0, ph, self._site(i, b, 2), pre=pre1[b], y32=a32[b], y16=a16[b])
            cq = ly["cq"].fwd(a16, dt)
            ckv = ly["ckv"].fwd(cand2, dt)                                            # (2, B*N, 2D): each target's keys | values, once per branch
            c = torch.empty((2, r, d), dtype=dt, device=dev)
            c32 = torch.empty((2, r, d), dtype=f32, device=dev)
            # ... and both cross-attentions: group = (branch, target image), its B * L stacked query rows against the target's 577 keys
            kv2 = ckv.view(2 * bt_n * n, 2 * d)
            s["ca"] = self._attn_fwd(self._heads(cq.view(2 * r, d), 2 * bt_n, b_n * l), self._heads(kv2, 2 * bt_n, n, 0, 2), self._heads(kv2, 2 * bt_n, n, 1, 2),
                                     None, self._site(i, 0, 3), c.view(2 * r, d), c32.view(2 * r, d))
            if ly["merge"] is None:                                                 # layers < 6: average (nlvr_encoder.py:257-260)
                dd = ly["d"].fwd(c, f32)
                t0, t1, alpha = dd[0], dd[1], 0.5
            else:                                                                   # layers >= 6: merge_layer(cat) (:252-256): the operand is written
                cat16 = torch.empty((r, 2 * d), dtype=dt, device=dev)               # in place, 16-bit, branch b into columns [bD, (b+1)D)
                ly["d"].fwd(c, dt, out=cat16.view(r, 2, d).permute(1, 0, 2))
                s["cat16"] = cat16
                t0, t1, alpha = ly["merge"].fwd(cat16, f32), None, 1.0
            # BertSelfOutput of the cross-attention: m = dropout(average | merge) (ONE mask for both branches), LayerNormA / B (m + a_b).
            # FFN: the SAME weights serve both branches (nlvr_encoder.py:469-476) - one pass over the 2R stacked rows (one GEMM pair,
            # one GELU / LayerNorm launch, and in the backward one dgrad / wgrad product each instead of two half-sized ones)
            pre2 = torch.empty((2 * r, d), dtype=f32, device=dev)
            x32, x16 = torch.empty_like(pre2), torch.empty((2 * r, d), dtype=dt, device=dev)
            for b in (0, 1):
                rows = slice(b * r, (b + 1) * r)
                ly[f"ln2{b}"].fwd_res(t0, t1, a32[b], dt, alpha, ph, self._site(i, 2, 4), pre=pre2[rows], y32=x32[rows], y16=x16[rows])
            z16 = ly["w1"].fwd(x16, dt)                                             # the dense output in the operand type, as autocast leaves it
            f16 = T.eltwise(z16, T.MODE_GELU, out_dtype=dt)
            pre3, hn, hn16 = ly["ln3"].fwd_res(ly["w2"].fwd(f16, f32), None, x32, dt, 1.0, ph, self._site(i, 0, 5))
            s.update(qkv=qkv, ctx=ctx, pre1=pre1, a16=a16, cq=cq, ckv=ckv, c=c, pre2=pre2, x16=x16, z16=z16, f16=f16, pre3=pre3)
            sv["layers"].append(s)
            h32, h16 = hn.view(2, r, d), hn16.view(2, r, d)
        # cat(CLS_0, CLS_1) -> cls_head (nlvr_encoder.py:906-908, blip_stage2.py:50-54, 94-99)
        cls_rows = torch.arange(t_n, device=dev) * l
        hid16 = torch.cat([ops.gather_rows(h16[0], cls_rows, dt), ops.gather_rows(h16[1], cls_rows, dt)], dim=1).contiguous()
        z1 = self.c0.fwd(hid16, f32)
        y16 = T.eltwise(z1, T.MODE_RELU, out_dtype=dt)
        logits2 = self.c2.fwd(y16, f32)                                             # (T, 2)
        sv.update(hid16=hid16, z1=z1, y16=y16, cls_rows=cls_rows)
        return logits2[:, 0].contiguous().view(bt_n, b_n).t().contiguous()          # (Bt_j, B_i) -> (B_i, Bt_j)

    def head_mask(self) -> torch.Tensor:
        """(B*Bt, hidden) bool: which cls_head.0 units were active in the last forward, rows in the reference's order (i * Bt + j)."""
        b, bt = self.sv["b_n"], self.sv["bt_n"]
        return (self.sv["z1"] > 0).view(bt, b, -1).transpose(0, 1).reshape(b * bt, -1)

    # ------------------------------------------------------------------------------------------------ backward
    @torch.no_grad()
    def backward(self, dlogits: torch.Tensor, observer=None) -> Optional[Dict[str, torch.Tensor]]:
        """dlogits (B, Bt) fp32 -> {parameter name: fp32 gradient} for every text_encoder.* / cls_head.* parameter.

        `observer` (None by default: the pass is then the same launches with the same arguments) is called at the cross-attention adjoint
        of each layer, top layer first, as observer(layer, dc16, q4, k4, v4, saved): dc16 (2, R, D) the 16-bit gradient of the context
        (times `self.grad_scale`), q4 (2 Bt, H, B L, hd) / k4 / v4 (2 Bt, H, N, hd) the head views the adjoint is about to read (group =
        (branch, target), rows = (query, token)), saved = what `_attn_fwd` returned (lse first).  A true return value ends the reverse
        pass there - the observer needs nothing below that layer - and backward returns None: the gradient buffer is then incomplete."""
        sv, g, dt = self.sv, self.geo, self.dtype
        det = self.slab.read_mode()                                                 # {} or the fixed-order forms' workspace (deterministic mode)
        dev = dlogits.device
        t_n, l, n, d = sv["t_n"], sv["l"], sv["n"], g.hidden_size
        r = t_n * l
        # Gradient scaling (what the reference's GradScaler does for its fp16 autocast, stage2_train.py:215-218, done inside):
        # every adjoint below is linear in the incoming gradient, so the pass runs on S * dlogits with S a power of two that
        # puts the largest entry near 512 - the 16-bit copies fed to the dgrad / wgrad GEMMs then sit in fp16's normal range
        # (hidden-state gradients are ~1e-5 per element unscaled, fp16's smallest normal is 6e-5) - and `_finish_backward` divides
        # by S.  bf16 has fp32's exponent range and needs none of this: scale 1, no unscaling pass.
        self.grad_scale = loss_scale(float(dlogits.abs().max())) if dt == torch.float16 else 1.0
        dl2 = torch.zeros((t_n, 2), dtype=torch.float32, device=dev)
        dl2[:, 0] = T.eltwise(dlogits.float().t().contiguous().view(-1), T.MODE_SCALE, p_drop=self.grad_scale)
        dy1 = self.c2.bwd(sv["y16"], dl2)
        dz1 = T.eltwise(sv["z1"], T.MODE_RELU_BWD, dy1)
        dhid = self.c0.bwd(sv["hid16"], dz1)                                        # (T, 2D)
        # Between the dense layers every gradient is the 16-bit operand of the next product (written by the kernel that forms it -
        # a fused LayerNorm adjoint, the attention adjoint, a dgrad epilogue), bias gradients are summed where it is formed, and
        # the fp32 gradient of the residual stream joins in the dgrad GEMM's epilogue: no stand-alone cast / add / dropout pass.
        dh = torch.zeros((2 * r, d), dtype=torch.float32, device=dev)               # both branches stacked, as the FFN saw them
        dh[sv["cls_rows"]] = dhid[:, :d]
        dh[sv["cls_rows"] + r] = dhid[:, d:]
        ph, b_n, bt_n = self.p_hidden, sv["b_n"], sv["bt_n"]
        dfeats = torch.empty((bt_n * n, sv["cand16"].shape[1]), dtype=torch.float32, device=dev) if self.need_dfeats else None
        dfeats_live = False
        for i in reversed(range(len(self.layers))):
            ly, s = self.layers[i], sv["layers"][i]
            w1, w2 = ly["w1"], ly["w2"]
            wq: list = []                                                           # this layer's weight-gradient products: ONE launch at its end
            dpre3, do16 = ly["ln3"].bwd_res(s["pre3"], dh, dt, dbias=w2.db, p_drop=ph, seed=self._site(i, 0, 5))
            df16 = w2.bwd16(s["f16"], do16, dx_dtype=dt, queue=wq)
            dz16 = T.gelu_bwd16(df16, s["z16"], sums=w1.db, **det)
            dx = w1.bwd16(s["x16"], dz16, residual=dpre3, queue=wq)                 # (2R, D) fp32: FFN branch + skip
            # the two LayerNorms over m + a_b: d m = dropout'(d pre2_0 + d pre2_1) comes out of the second one's kernel
            merge = ly["merge"]
            dpre2 = torch.empty((2, r, d), dtype=torch.float32, device=dev)
            ly["ln20"].bwd_res(s["pre2"][:r], dx[:r], dt, want_dt=False, dx=dpre2[0])
            if merge is None:                                                       # average: both output denses see 0.5 * d m
                kw = dict(alpha=0.5, dbias=ly["d0"].db, dbias2=ly["d1"].db)
            else:
                kw = dict(alpha=1.0, dbias=merge.db)
            _, dm16 = ly["ln21"].bwd_res(s["pre2"][r:], dx[r:], dt, t_add=dpre2[0], p_drop=ph, seed=self._site(i, 2, 4), dx=dpre2[1], **kw)
            if merge is None:
                dd16 = dm16.unsqueeze(0).expand(2, r, d)                            # one gradient, two branches (batch stride 0)
            else:
                dcat16 = merge.bwd16(s["cat16"], dm16, dx_dtype=dt, queue=wq)       # (R, 2D)
                dd16 = dcat16.view(r, 2, d).permute(1, 0, 2)                        # branch b = columns [bD, (b+1)D)
            ly["d"].wgrad(s["c"], dd16, wq, bias=merge is not None)
            dc16 = ly["d"].dgrad(dd16, dt)                                          # (2, R, D): both branches' output-dense dgrads, one GEMM
            cq, ckv = s["cq"], s["ckv"]
            dcq16 = torch.empty((2, r, d), dtype=dt, device=dev)
            dckv16 = torch.empty((2, bt_n * n, 2 * d), dtype=dt, device=dev)
            kv2, dkv2 = ckv.view(2 * bt_n * n, 2 * d), dckv16.view(2 * bt_n * n, 2 * d)
            cq4, ck4, cv4 = self._heads(cq.view(2 * r, d), 2 * bt_n, b_n * l), self._heads(kv2, 2 * bt_n, n, 0, 2), self._heads(kv2, 2 * bt_n, n, 1, 2)
            if observer is not None and observer(i, dc16, cq4, ck4, cv4, s["ca"]):
                return None
            self._attn_bwd(dc16.view(2 * r, d), cq4, ck4, cv4, s["ca"], self._heads(dcq16.view(2 * r, d), 2 * bt_n, b_n * l),
                           self._heads(dkv2, 2 * bt_n, n, 0, 2), self._heads(dkv2, 2 * bt_n, n, 1, 2))
            cand2 = sv["cand16"].unsqueeze(0).expand(2, bt_n * n, sv["cand16"].shape[1])
            ly["ckv"].wgrad(cand2, dckv16, wq, bias=True)
            if dfeats is not None:                                                  # ViT fine-tuning: every layer and branch adds its share
                for b in (0, 1):                                                    # (image tokens are inputs otherwise: no gradient beyond the weights)
                    ops.gemm(dckv16[b], ly[f"ckv{b}"].w16t, None, residual=dfeats if dfeats_live else None, out_dtype=torch.float32, out=dfeats)
                    dfeats_live = True
            ly["cq"].wgrad(s["a16"], dcq16, wq, bias=True)
            da = ly["cq"].dgrad(dcq16, torch.float32, residual=dpre2)               # (2, R, D) fp32: cross-attention query branch + skip
            dpre1 = torch.empty((2, r, d), dtype=torch.float32, device=dev)
            dt16 = torch.empty((2, r, d), dtype=dt, device=dev)
            for b in (0, 1):
                ly[f"ln1{b}"].bwd_res(s["pre1"][b], da[b], dt, dbias=ly[f"o{b}"].db, p_drop=ph, seed=self._site(i, b, 2), dx=dpre1[b], dt16=dt16[b])
            ly["o"].wgrad(s["ctx"], dt16, wq)
            dctx16 = ly["o"].dgrad(dt16, dt)
            qkv = s["qkv"]
            dqkv16 = torch.empty((2, r, 3 * d), dtype=dt, device=dev)
            self._attn_bwd(dctx16.view(2 * r, d), *(self._heads(qkv.view(2 * r, 3 * d), 2 * t_n, l, j, 3) for j in range(3)), s["sa"],
                           *(self._heads(dqkv16.view(2 * r, 3 * d), 2 * t_n, l, j, 3) for j in range(3)))
            ly["qkv"].wgrad(s["h16"], dqkv16, wq, bias=True)
            dh = ly["qkv"].dgrad(dqkv16, torch.float32, residual=dpre1).view(2 * r, d)      # both branches stacked, as the layer below's FFN saw them
            self._wgrad_grouped(wq)
        # branch 1 entered through BertEmbeddings; branch 0 is z_t (frozen stage I)
        de = dh[r:] if ph <= 0 else T.eltwise(dh[r:], T.MODE_DROPOUT, p_drop=ph, seed=self._site(9000))
        dpre_e = self.ln_e.bwd(sv["pre_e"], de)
        T.embed_bwd(sv["ids"].view(-1), dpre_e, self.dword, self.dpos, l, **det)
        # the loss-scaled gradient of the target tokens, unscaled for the ViT's own (separately scaled) reverse pass
        self.dfeats = None if dfeats is None else (dfeats if self.grad_scale == 1.0 else T.eltwise(dfeats, T.MODE_SCALE, p_drop=1.0 / self.grad_scale))
        self.dfeats_scale = None if dfeats is None else self.grad_scale            # train_vit.VitTrainer.backward runs under the same scale
        return self._finish_backward()


class _FusionTrainFn(torch.autograd.Function):
    """One autograd node around NlvrTrainer.forward / backward: `loss.backward()` of the reference's training step reaches
    the hand-written reverse pass through it.  `anchor` is a one-element leaf that only makes the node differentiable; the
    parameters' gradients are accumulated into `.grad` directly, as autograd's AccumulateGrad would (a first gradient is the
    trainer's own slice of its flat gradient buffer - no copy; later ones are added)."""

    @staticmethod
    def forward(ctx, anchor, trainer, z_t, feats, ids, mask):
        ctx.trainer = trainer
        ctx.feats_shape = tuple(feats.shape)
        out = trainer.forward(z_t, feats, ids, mask)
        trainer._claim(ctx)
        return out

    @staticmethod
    def backward(ctx, dlogits):
        tr = ctx.trainer
        tr._consume(ctx)
        _install_grads(tr, tr.backward(dlogits.contiguous().float()))
        dfeats = None if tr.dfeats is None else tr.dfeats.view(ctx.feats_shape)
        tr.dfeats = None
        return None, None, None, dfeats, None, None


def model_trainer(model, p_hidden: float, p_attn: float, seed: int, device) -> NlvrTrainer:
    """The model's one NlvrTrainer (`model._trainer`: one slab - a second one would re-point every parameter), rebuilt when the dropout
    probabilities or the operand type changed."""
    tr = getattr(model, "_trainer", None)
    if tr is None or (tr.p_hidden, tr.p_attn) != (float(p_hidden), float(p_attn)) or tr.dtype != train_dtype(model):
        tr = model._trainer = NlvrTrainer(model, p_hidden, p_attn, seed)
        apply_pending_counters(model, "fusion", tr)           # (seed, step_no) a checkpoint left for this trainer (load_training_state)
        tr.anchor = torch.zeros((1,), device=device, requires_grad=True)
    return tr


def fusion_train(model, z_t, feats, ids, mask, p_hidden: float = 0.1, p_attn: float = 0.1, seed: int = 0) -> torch.Tensor:
    """(B, Bt) logits of `img_txt_fusion` in training mode (z_t / ids / mask: B queries; feats: Bt targets - Bt = B is the reference's step,
    Bt > B adds negatives), differentiable w.r.t. the model's text_encoder / cls_head parameters - and w.r.t. the target image tokens when
    they require a gradient (blip_img_tune, stage2_train.py:191-199: the tokens then come from `train_vit.vit_train`, whose reverse pass
    continues into the ViT)."""
    if torch.is_tensor(z_t) and z_t.requires_grad:
        raise NotImplementedError("z_t requires a gradient: the reference computes it from the frozen stage-I model under torch.no_grad() "
                                  "(stage2_train.py:201-203); the backward pass stops at the two-branch encoder's z_t input")
    tr = model_trainer(model, p_hidden, p_attn, seed, z_t.device)
    tr.need_dfeats = bool(torch.is_tensor(feats) and feats.requires_grad)
    return _FusionTrainFn.apply(tr.anchor, tr, z_t, feats, ids, mask)


_NO_DECAY_NAMES = ("visual_encoder.pos_embed", "visual_encoder.cls_token")


def param_groups(model, weight_decay: float, lr_scale: Dict[str, float] = None) -> List[Dict]:
    """Group dicts for `AdamW` (and torch.optim.AdamW) over the `requires_grad` parameters of `model`, in `named_parameters()` order:
    biases, LayerNorm weights and every other parameter with ndim <= 1, plus visual_encoder.pos_embed / cls_token, take weight_decay 0
    (the reference's single group, stage2_train.py:138, gives them the config's full 0.05); `lr_scale` = {name prefix: factor} - the first
    prefix a name starts with, in the dict's order - splits further, e.g. {"visual_encoder.": 0.1} for a ViT tuned at a tenth of the rate.
    A group carries "lr_scale" only when its factor is not 1; groups come in the order their first parameter appears; empty ones are left
    out.  At most 8 groups (cir_adamw_step_groups)."""
    scales = list((lr_scale or {}).items())
    groups: Dict[tuple, Dict] = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        scale = next((float(f) for prefix, f in scales if name.startswith(prefix)), 1.0)
        decay = 0.0 if p.ndim <= 1 or name in _NO_DECAY_NAMES else float(weight_decay)
        g = groups.get((decay, scale))
        if g is None:
            g = groups[(decay, scale)] = {"params": [], "weight_decay": decay}
            if scale != 1.0:
                g["lr_scale"] = scale
        g["params"].append(p)
    return list(groups.values())
