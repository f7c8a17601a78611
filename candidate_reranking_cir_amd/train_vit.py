"""ViT fine-tuning inside the stage-II training step (`--blip-img-tune`, stage2_train.py:87-92, 191-199; SURVEY section 8(f)-4, the part
round 3 refused): the target images' tokens come from `model.img_embed` in .train() mode WITH a graph, the loss's gradient reaches them
through the cross-attention K|V projections of all 12 two-branch layers (`NlvrTrainer.need_dfeats`), and continues through the patch
encoder (vit.py:113-194 + timm PatchEmbed).  The stage-II image encoder is built with drop_path_rate 0.1 (blip_stage2.py:37; vit.py:153:
block i drops each SAMPLE's attention / MLP branch with probability linspace(0, 0.1, depth)[i] and scales the kept ones by 1 / keep,
vit.py:98-109 with timm's DropPath); its dropout probabilities are 0.  DropPath here is counter-based like the text side's dropout: the
per-sample scales of a step come from a seeded host generator (depth x 2 x B numbers), the backward reuses them; with rate 0 the pass is
deterministic and is what tests/golden/train_imgtune.npz pins.

Same construction as `train.NlvrTrainer`: an explicit forward that keeps what the reverse pass needs and a hand-written reverse pass on the
libcirrank kernels - 16-bit MFMA operands, fp32 residual stream and gradients of it, the fused attention pair (197 / 577 keys, no mask, no
dropout: the dropout-free instantiations), the four weight gradients of a block in one grouped launch, parameters / 16-bit copies / gradients
in flat buffers (`train_core._Slab`; the machinery the passes share is in train_core.py) so that `train.AdamW` updates the ViT in one
launch.  Pre-LayerNorm blocks: x + f(LayerNorm(x)), so the LayerNorm adjoint's input is the saved residual stream itself and its result is
added to the skip gradient.

Gradient checkpointing (`vit_grad_ckpt` / `vit_ckpt_layer` of the factories, `set_vit_checkpointing`; fairscale's checkpoint_wrapper around
attn and mlp of block i >= depth - ckpt_layer in the reference, vit.py:103-105, :158): such a block keeps only x and x1, the two fp32 stream
rows its LayerNorm adjoints read, and `backward` rebuilds the rest by the forward's own launches (`_recompute`) before the block's adjoints;
gelu(fc1's output), the left operand of fc2's weight gradient, comes from the pass that reads fc1's output for dz (`gelu_bwd16_pair`).
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import lib as _lib
from . import ops, train_ops as T
from .train_core import _LN, Trainer, _cast, _install_grads, apply_pending_counters, loss_scale

_P = "visual_encoder."


def vit_checkpointed_blocks(model) -> int:
    """Number of trailing ViT blocks whose activations are recomputed in the backward: 0 unless the factory was given `vit_grad_ckpt`, else
    min(vit_ckpt_layer, depth) (`set_vit_checkpointing` changes it) - block i is checkpointed iff i >= depth - that number (vit.py:158)."""
    return max(0, min(int(getattr(model, "vit_ckpt_blocks", 0)), model.vit_geometry.depth))


def _block_saved_bytes(geo, ckpt: bool) -> int:
    """Bytes per token a block keeps for its backward: an unchecked block's ten tensors (x, x1, ctx32 fp32 and h16, ctx, h2 16-bit of width
    D; qkv 16-bit of 3 D; z16, f16 16-bit of the MLP width; lse fp32 per head - 30768 at width 768), a checkpointed block's x and x1 (6144)."""
    d = geo.width
    if ckpt:
        return 2 * 4 * d
    return 3 * 4 * d + 2 * (3 * d + 3 * d + 2 * geo.mlp_ratio * d) + 4 * geo.num_heads


def vit_saved_bytes(model, batch: int) -> int:
    """Bytes one `img_embed(image)` call of `batch` images in train mode keeps for its backward under the model's current checkpointing
    setting: the summed `nbytes` of the tensors of the call's saved state - the 16-bit patch rows, each block's entry (`VitTrainer.forward`),
    the final fp32 stream and, where the geometry has DropPath, the call's (depth, 2, batch) fp32 scales.  From the geometry and the operand
    type (16-bit in every mode, `vit_train_dtype`) alone: no device access."""
    geo = model.vit_geometry
    n, depth = geo.num_tokens, geo.depth
    ck = vit_checkpointed_blocks(model)
    patch_cols = geo.in_chans * geo.patch_size * geo.patch_size
    per_token = (depth - ck) * _block_saved_bytes(geo, False) + ck * _block_saved_bytes(geo, True) + 4 * geo.width
    drop_path = 4 * depth * 2 if float(getattr(geo, "drop_path_rate", 0.0)) > 0.0 and depth >= 2 else 0
    return int(batch) * ((n - 1) * patch_cols * 2 + n * per_token + drop_path)


def vit_train_dtype(model) -> torch.dtype:
    """Operand type of the ViT's training step: the model's token type when it is 16-bit, fp16 under the exact mode (fp32 tokens) - the
    same mapping `train_core.train_dtype` applies to the text side (the reference trains under fp16 autocast, stage2_train.py:210-218)."""
    return model.token_dtype if model.token_dtype in (torch.float16, torch.bfloat16) else torch.float16


class VitTrainer(Trainer):
    _KEY = "vit"

    def __init__(self, model):
        self.model, self.geo = model, model.vit_geometry
        self.dtype = vit_train_dtype(model)
        self._nh, self._hd = self.geo.num_heads, 64
        self._scale = 64 ** -0.5                                                    # vit.py:50 (head dimension 64)
        self.seed, self.step_no = 0, 0

    def _drop_path_scales(self, bsz: int, device):
        """(depth, 2, B) fp32: 0 for a dropped (block, branch, sample), 1 / keep for a kept one; None when the rate is 0 (vit.py:153)."""
        rate = float(getattr(self.geo, "drop_path_rate", 0.0))
        if rate <= 0.0 or self.geo.depth < 2:
            return None, [0.0] * self.geo.depth
        import random
        rng = random.Random(self.seed * 1000003 + self.step_no * 7919 + 17)
        ps = [rate * i / (self.geo.depth - 1) for i in range(self.geo.depth)]      # torch.linspace(0, rate, depth)
        rows = [[[0.0 if rng.random() < p else 1.0 / (1.0 - p) for _ in range(bsz)] for _ in (0, 1)] for p in ps]
        return torch.tensor(rows, dtype=torch.float32, device=device), ps

    def _trained(self, name: str) -> bool:
        return name.startswith(_P)

    def _build_layers(self, slab, lin, ln):
        self.pe = lin(_P + "patch_embed.proj")                                      # Conv2d(3, D, p, p, stride p) == Linear over flattened patches
        self.blocks: List[Dict] = []
        for i in range(self.geo.depth):
            b = f"{_P}blocks.{i}."
            self.blocks.append(dict(ln1=ln(b + "norm1"), qkv=lin(b + "attn.qkv"), proj=lin(b + "attn.proj"), ln2=ln(b + "norm2"),
                                    fc1=lin(b + "mlp.fc1"), fc2=lin(b + "mlp.fc2")))
        self.lnf = ln(_P + "norm")
        d = self.geo.width
        self.cls, self.pos = slab.w32(_P + "cls_token").view(d), slab.w32(_P + "pos_embed").view(-1, d)
        assert self.pos.shape[0] == self.geo.num_tokens, "pos_embed does not match the ViT geometry"

    def _bind_grads(self, slab):
        d = self.geo.width
        self.dcls, self.dpos = slab.grad(_P + "cls_token").view(d), slab.grad(_P + "pos_embed").view(-1, d)

    def _ln16(self, ln: _LN, x: torch.Tensor):
        """Pre-LayerNorm: only the 16-bit operand copy is needed (the fp32 input itself is the saved tensor of the adjoint)."""
        return ops.layernorm(x, ln.g, ln.b, ln.eps, want32=False, dtype16=self.dtype, stream_dtype=torch.float32)

    # ------------------------------------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, image: torch.Tensor) -> torch.Tensor:
        """(B, 3, H, W) -> (B, N, D) fp32 image tokens (VisionTransformer.forward, vit.py:180-194); keeps what backward needs."""
        self._pack()
        geo, dt = self.geo, self.dtype
        if image.shape[-1] != geo.image_size or image.shape[-2] != geo.image_size:
            raise ValueError(f"image size {tuple(image.shape[-2:])} != model image_size {geo.image_size}")
        if image.dtype not in (torch.float32, dt):
            image = image.float()
        bsz, d, n = image.shape[0], geo.width, geo.num_tokens
        f32 = torch.float32
        patches = ops.patchify(image.contiguous(), geo.patch_size, dt)              # PatchEmbed im2col (B * P, 3 p p)
        x = ops.vit_assemble(self.pe.fwd(patches, f32), self.cls, self.pos, bsz).view(bsz * n, d)      # vit.py:184-187, fp32 stream
        self.step_no += 1
        dp, dp_rates = self._drop_path_scales(bsz, x.device)
        # What the reverse pass needs travels WITH THE CALL (the autograd node keeps it), not on the trainer: the reference embeds the
        # reference and the target images in `blip_bs` mini-batches, every call with a graph (stage2_train.py:191-199) - several calls
        # are live at once, and each backward must find its own activations and its own DropPath draw (round-4 advisor finding).
        # Gradient checkpointing (vit.py:103-105, :158): the setting is read HERE, once per call, and the form each block saved is recorded
        # beside its entry - the backward follows the record, whatever the setting has become by then.
        first_ckpt = len(self.blocks) - vit_checkpointed_blocks(self.model)
        sv = {"patches": patches, "bsz": bsz, "blocks": [], "ckpt": [], "dp": dp, "dp_rates": dp_rates, "epoch": _lib.PARAM_EPOCH[0]}
        heads = lambda t, j: self._heads(t, bsz, n, j, 3)

        def branch(lin, a16, res, i, j):
            """res + DropPath(lin(a16)) (vit.py:108-109): the residual joins in the GEMM epilogue unless block i drops samples."""
            if dp is None or dp_rates[i] <= 0.0:
                return lin.fwd(a16, f32, residual=res)
            return T.rows_scale_add(res, lin.fwd(a16, f32), dp[i, j], n)
        for i, blk in enumerate(self.blocks):
            _, h16 = self._ln16(blk["ln1"], x)                                       # vit.py:108
            qkv = blk["qkv"].fwd(h16, dt)                                            # (B N, 3 D), vit.py:72
            ctx = torch.empty((bsz * n, d), dtype=dt, device=x.device)
            ctx32 = torch.empty((bsz * n, d), dtype=f32, device=x.device)
            c4, c32 = self._heads(ctx, bsz, n), self._heads(ctx32, bsz, n)
            lse = T.attention_train_fwd(heads(qkv, 0), heads(qkv, 1), heads(qkv, 2), None, c4, self._scale, 0.0, 0, out32=c32)    # vit.py:73-83
            x1 = branch(blk["proj"], ctx, x, i, 0)                                  # vit.py:84, :108
            _, h2 = self._ln16(blk["ln2"], x1)
            z16 = blk["fc1"].fwd(h2, dt)                                             # vit.py:36
            f16 = T.eltwise(z16, T.MODE_GELU, out_dtype=dt)                         # vit.py:37
            x2 = branch(blk["fc2"], f16, x1, i, 1)                                  # vit.py:39, :109
            ckpt = i >= first_ckpt
            sv["ckpt"].append(ckpt)
            if ckpt:                                                                 # the two fp32 stream rows the LayerNorm adjoints read; the rest goes now
                sv["blocks"].append(dict(x=x, x1=x1))
            else:
                sv["blocks"].append(dict(x=x, h16=h16, qkv=qkv, ctx=ctx, ctx32=ctx32, lse=lse, x1=x1, h2=h2, z16=z16, f16=f16))
            x = x2
        sv["xf"] = x
        y32, _ = self.lnf.fwd(x, dt)                                                 # vit.py:192
        self.sv = sv                                                                 # (the latest call's state: tests / tools read it)
        return y32.view(bsz, n, d), sv

    # ------------------------------------------------------------------------------------------------ recompute
    def _recompute(self, blk: Dict, s: Dict, bsz: int, n: int):
        """The activations of a checkpointed block from its saved x and x1, by the launches (kernels and arguments) `forward` made: both
        LayerNorms, the qkv and fc1 products, the attention.  The proj and fc2 products are not needed again (x1 and the next block's x
        are saved); no random number is drawn (DropPath acts outside the two sub-modules, its scales travel with the call).  f16 = gelu(z16)
        comes back EMPTY where fc2's weight gradient is a queued product: `gelu_bwd16_pair` fills it in the pass that reads z16 for dz,
        before the block's grouped weight-gradient launch reads it.  Returns (the full entry, whether f16 is still to be filled)."""
        dt, d, f32 = self.dtype, self.geo.width, torch.float32
        x, x1 = s["x"], s["x1"]
        heads = lambda t, j: self._heads(t, bsz, n, j, 3)
        _, h16 = self._ln16(blk["ln1"], x)
        qkv = blk["qkv"].fwd(h16, dt)
        ctx = torch.empty((bsz * n, d), dtype=dt, device=x.device)
        ctx32 = torch.empty((bsz * n, d), dtype=f32, device=x.device)
        lse = T.attention_train_fwd(heads(qkv, 0), heads(qkv, 1), heads(qkv, 2), None, self._heads(ctx, bsz, n), self._scale, 0.0, 0,
                                    out32=self._heads(ctx32, bsz, n))
        _, h2 = self._ln16(blk["ln2"], x1)
        z16 = blk["fc1"].fwd(h2, dt)
        # `_Lin.bwd16` reads its left operand at once unless it queues the product (both extents multiples of 128, train_wgrad.hip): then
        # - every real width - the pair kernel may deliver f16 later; otherwise it is recomputed here, by the forward's own launch
        pair = blk["fc2"].n % 128 == 0 and blk["fc2"].k % 128 == 0
        f16 = torch.empty_like(z16) if pair else T.eltwise(z16, T.MODE_GELU, out_dtype=dt)
        return dict(x=x, h16=h16, qkv=qkv, ctx=ctx, ctx32=ctx32, lse=lse, x1=x1, h2=h2, z16=z16, f16=f16), pair

    # ------------------------------------------------------------------------------------------------ backward
    @torch.no_grad()
    def backward(self, dfeats: torch.Tensor, sv: Dict = None) -> Dict[str, torch.Tensor]:
        """dfeats (B, N, D) fp32 -> {parameter name: fp32 gradient} for every visual_encoder.* parameter, from the saved state `sv` of
        the forward call being differentiated (default: the latest call's).  Every backward writes a FRESH flat gradient buffer
        (`train_core._install_grads` folds it into .grad with one flat add), so the mini-batches of one step - and their loss scales - do
        not meet inside a buffer."""
        sv = self.sv if sv is None else sv
        geo, dt = self.geo, self.dtype
        if sv["epoch"] != _lib.PARAM_EPOCH[0]:
            raise RuntimeError("img_embed (train mode): the parameters were updated (optimizer step) between this forward and its backward - "
                               "the reverse pass would run on other weights than the forward did")
        slab = self.slab
        det = slab.read_mode()                                                      # {} or the fixed-order forms' workspace (deterministic mode)
        slab.gflat = torch.zeros_like(slab.flat32)
        self._bind_grads(slab)
        d = geo.width
        bsz, n = sv["bsz"], geo.num_tokens
        dev = dfeats.device
        g = dfeats.contiguous().float().view(bsz * n, d)
        # fp16 operands: run the (linear) pass on S * dfeats, S a power of two putting the largest entry near 512 (train.NlvrTrainer.backward)
        # When the gradient comes out of the two-branch encoder's reverse pass (the normal case), that pass's scale is reused: its own
        # internal gradients - of which dfeats is a 24-term sum - sat in fp16's range under it, and reading max|dfeats| back would make the
        # host wait for the whole fusion backward before the first ViT launch.
        self.grad_scale = 1.0
        if dt == torch.float16:
            hint = getattr(getattr(self.model, "_trainer", None), "dfeats_scale", None)
            if hint is not None:
                self.grad_scale = float(hint)
                self.model._trainer.dfeats_scale = None
            else:
                self.grad_scale = loss_scale(float(g.abs().max()))
            if self.grad_scale != 1.0:
                g = T.eltwise(g, T.MODE_SCALE, p_drop=self.grad_scale)
        g = self.lnf.bwd(sv["xf"], g)
        heads = lambda t, j: self._heads(t, bsz, n, j, 3)
        dp, dp_rates = sv["dp"], sv["dp_rates"]

        def branch_grad(gq, i, j):
            """The stream gradient as the branch's 16-bit operand: scaled per sample where block i drops samples."""
            return _cast(gq, dt) if dp is None or dp_rates[i] <= 0.0 else T.rows_scale_add(None, gq, dp[i, j], n, out_dtype=dt)
        for i in reversed(range(len(self.blocks))):
            blk, s, pair = self.blocks[i], sv["blocks"][i], False
            wq: list = []
            if sv["ckpt"][i]:
                s, pair = self._recompute(blk, s, bsz, n)
            # x2 = x1 + DropPath(fc2(gelu(fc1(LayerNorm2(x1)))))
            g16 = branch_grad(g, i, 1)
            df16 = blk["fc2"].bwd16(s["f16"], g16, dx_dtype=dt, bias=True, queue=wq)
            if pair:                                                                 # dz and the f16 the queued fc2 weight gradient reads, one pass over z16
                dz16, _ = T.gelu_bwd16_pair(df16, s["z16"], sums=blk["fc1"].db, out_f=s["f16"], **det)
            else:
                dz16 = T.gelu_bwd16(df16, s["z16"], sums=blk["fc1"].db, **det)
            dh2 = blk["fc1"].bwd16(s["h2"], dz16, queue=wq)                         # (B N, D) fp32
            g = T.eltwise(blk["ln2"].bwd_res(s["x1"], dh2, dt, want_dt=False)[0], T.MODE_ADD, g)
            # x1 = x + DropPath(proj(attention(LayerNorm1(x))))
            g16 = branch_grad(g, i, 0)
            dctx16 = blk["proj"].bwd16(s["ctx"], g16, dx_dtype=dt, bias=True, queue=wq)
            dqkv16 = torch.empty((bsz * n, 3 * d), dtype=dt, device=dev)
            c4 = lambda t: self._heads(t, bsz, n)
            T.attention_train_bwd(heads(s["qkv"], 0), heads(s["qkv"], 1), heads(s["qkv"], 2), None, c4(s["ctx"]), c4(dctx16), s["lse"],
                                  heads(dqkv16, 0), heads(dqkv16, 1), heads(dqkv16, 2), self._scale, 0.0, 0, out32=c4(s["ctx32"]))
            dh = blk["qkv"].bwd16(s["h16"], dqkv16, bias=True, queue=wq)
            g = T.eltwise(blk["ln1"].bwd_res(s["x"], dh, dt, want_dt=False)[0], T.MODE_ADD, g)
            self._wgrad_grouped(wq)
            s = wq = None                                                            # a recomputed block's tensors go before the next block's arrive
        # x0 = cat(cls, patch_embed(image)) + pos_embed (vit.py:182-187)
        g3 = g.view(bsz, n, d)
        T.colsum(g.view(bsz, n * d), self.dpos.reshape(-1), **det)
        T.colsum(g3[:, 0], self.dcls, **det)
        dproj16 = _cast(g3[:, 1:].contiguous().view(bsz * (n - 1), d), dt)
        self.pe.bwd16(sv["patches"], dproj16, need_dx=False, bias=True)             # pixels are inputs
        return self._finish_backward()


class _VitTrainFn(torch.autograd.Function):
    """One autograd node around VitTrainer.forward / backward.  The node owns the saved state of ITS call, so any number of calls
    may be live between forward and backward - the reference's loop embeds reference and target images in `blip_bs` mini-batches,
    each with a graph (stage2_train.py:191-199); calls whose output never receives a gradient (the reference images: z_t is formed
    under no_grad) simply drop their state with their output.  A second backward through one call raises (its state is released)."""

    @staticmethod
    def forward(ctx, anchor, trainer, image):
        ctx.trainer = trainer
        out, ctx.sv = trainer.forward(image)
        return out

    @staticmethod
    def backward(ctx, dfeats):
        tr, sv = ctx.trainer, ctx.sv
        if sv is None:
            raise RuntimeError("img_embed (train mode): second backward through the same forward; run the forward again")
        ctx.sv = None
        _install_grads(tr, tr.backward(dfeats, sv))
        return None, None, None


def vit_train(model, image: torch.Tensor) -> torch.Tensor:
    """(B, N, D) fp32 image tokens of `img_embed` in training mode, differentiable w.r.t. the model's visual_encoder parameters."""
    tr = getattr(model, "_vit_trainer", None)
    if tr is None or tr.dtype != vit_train_dtype(model):
        tr = model._vit_trainer = VitTrainer(model)
        apply_pending_counters(model, "vit", tr)              # (seed, step_no) a checkpoint left for this trainer (load_training_state)
        tr.anchor = torch.zeros((1,), device=model.device, requires_grad=True)
    return _VitTrainFn.apply(tr.anchor, tr, image.to(model.device))
