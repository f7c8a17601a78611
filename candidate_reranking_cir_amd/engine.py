"""Kernel schedules for the three encoders on the path (Python host, HIP kernels via `ops`).

Each engine packs a reference-layout fp32 state dict once (16-bit weight matrices, fused QKV /
K|V concatenations, folded merge weights; fp32 biases and LayerNorm affines) and then issues a
fixed sequence of libcirrank launches per forward.  Precision plan: GEMM operands and attention
tiles are 16-bit (fp16 by default since round 4, or bf16; or fp32 - `dtype=torch.float32`, the "exact" mode of round 5: every tensor
fp32 like the reference's, products on the f32-input MFMA, exact-erf GELU, no algebraic folds); every accumulation, the softmax and the LayerNorm statistics are
fp32; the RESIDUAL STREAM (x + sublayer(x), and the LayerNorm outputs that feed one) is stored in
`stream_dtype`: fp16 by default (sum formed in fp32, rounded to 11 bits) or fp32.

MIXED operand precision (round 4; profiles/r4_precision_attribution_*.json): the text-side engines take a second operand
type `cross_dtype` for their image-facing block - cross-attention query / key|value projections, the cross-attention itself
and its output (merge) projection, all of which consume or meet the ViT's tokens - while the self-attention block, the FFN and
cls_head run in `dtype`.  The per-site rounding attribution shows the rank error of a bf16 run entering through the text-side
self-attention / FFN / cls_head ACTIVATIONS; the ViT and the cross-attention block are rank-neutral in bf16.  "mixed" =
ViT + cross block bf16 (77 % of the flops), text self-attention + FFN + cls_head fp16.

Reference arithmetic being scheduled (cited per method): vit.py:180-194, med.py:348-398 / 685-821,
nlvr_encoder.py:414-476 / 777-908, blip_stage2.py:101-136.
"""
from __future__ import annotations

import warnings
import weakref
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import ops
from .config import BertGeometry, VitGeometry

SD = Dict[str, torch.Tensor]

LN_FOLD_DEFAULT = 1   # VitEngine.ln_fold where the geometry allows it (bench.py's CIR_VIT_LNFOLD overrides for A/B runs)


def _w16(t: torch.Tensor, dtype, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).to(dtype).contiguous()


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _mark_split(mode: int, layers, *extra):
    """text32 mode: every fp32 weight matrix of the text side (keys w*) takes a multi-product path of `ops.gemm`: mode 3 = three fp16
    products on [hi | lo | hi] rows (ops.split_weight, round 5), mode 8 = one fp16 product + two block-scaled fp8 correction products on
    "split8" rows (ops.split_weight8, round 6: 2 instead of 3 fp16-equivalents of matrix-pipe time, operands produced by the LayerNorm /
    attention / fc1 kernels themselves)."""
    mark = ops.split_weight8 if mode == 8 else ops.split_weight
    for ly in layers:
        for k, v in ly.items():
            if k.startswith("w") and torch.is_tensor(v) and v.dtype == torch.float32 and v.dim() >= 2:
                mark(v)
    for w in extra:
        mark(w)


def _split_mode(split3, dtype, geo=None) -> int:
    """engine argument `split3` (kept name): False / 0 = the f32-input MFMA, True / 3 = three fp16 products, 8 = split8 rows.
    split8 needs whole K-tile pairs in each of its three K segments (every Linear's depth a multiple of 256: hidden 768 / 1024, FFN 3072 / 4096,
    cls_head 2 x hidden); a geometry outside that (the 128-wide test geometries) takes the three-product form instead."""
    if dtype != torch.float32 or not split3:
        return 0
    if split3 == 8 and geo is not None and (geo.hidden_size % 256 or geo.intermediate_size % 256):
        return 3
    return 8 if split3 == 8 else 3


def _auto_stream(dtype: torch.dtype, stream_dtype: Optional[torch.dtype]) -> torch.dtype:
    """Residual-stream storage: explicit, or fp16 (the sums are formed in fp32; DESIGN.md section 2 has what fp32 storage of
    the text-side stream buys - tau 0.91 -> 0.94 on the outlier fixture - and costs - 3.6 % of the step)."""
    return stream_dtype if stream_dtype is not None else torch.float16


def _ln(x, gamma, beta, eps, dt, sdt, residual=None, need_stream=True, split8=False):
    """LayerNorm -> (stream copy in `sdt` or None, operand copy in `dt`).  One tensor serves as both when dt == sdt.
    `split8`: fp32 stream copy + the operand as split8 rows, written by the LayerNorm kernel itself (text32 mode)."""
    if split8:
        return ops.layernorm_split8(x, gamma, beta, eps, residual=residual)
    if (dt == sdt and need_stream) or dt == torch.float32:      # fp32 operands ("exact" mode): the fp32 stream copy IS the operand
        y, _ = ops.layernorm(x, gamma, beta, eps, residual=residual, want32=True, dtype16=None, stream_dtype=sdt)
        return y, y
    return ops.layernorm(x, gamma, beta, eps, residual=residual, want32=need_stream, dtype16=dt, stream_dtype=sdt)


def _attend(q, k, v, scale, mask, dt, split8, lead):
    """Self-attention context as the output projection's A operand under the leading shape `lead`: split8 rows written by the fp32
    attention kernel itself (text32 mode), or a fresh `dt` tensor (*lead, D) filled by `ops.attention`."""
    if split8:
        return ops.attention_split8(q, k, v, scale, mask).view(*lead)
    ctx = torch.empty(q.shape, dtype=dt, device=q.device)
    ops.attention(q, k, v, ctx, scale, mask)
    return ctx.view(*lead, q.shape[-1])


def additive_self_mask(attention_mask: torch.Tensor) -> torch.Tensor:
    """(R, L) ones/zeros -> fp32 additive key mask (1 - m) * -10000 (nlvr_encoder.py:773-774)."""
    return ((1.0 - attention_mask.to(torch.float32)) * -10000.0).contiguous()


def additive_encoder_mask(attention_mask: torch.Tensor) -> torch.Tensor:
    """transformers' invert_attention_mask: (1 - m) * finfo(float32).min (called nlvr_encoder.py:863-868)."""
    return ((1.0 - attention_mask.to(torch.float32)) * torch.finfo(torch.float32).min).contiguous()


# =================================================================================================
class VitEngine:
    """ViT-B/16 patch encoder (vit.py:113-194 + timm PatchEmbed) as 7 launches per block."""

    def __init__(self, sd: SD, geo: VitGeometry, dtype: torch.dtype, device, prefix: str = "visual_encoder.",
                 stream_dtype: Optional[torch.dtype] = None):
        geo.validate()
        self.geo, self.dtype, self.device, self.stream_dtype = geo, dtype, device, _auto_stream(dtype, stream_dtype)
        d = geo.width
        p = prefix
        self.w_patch = _w16(sd[p + "patch_embed.proj.weight"].reshape(d, -1), dtype, device)
        self.b_patch = _f32(sd[p + "patch_embed.proj.bias"], device)
        self.cls = _f32(sd[p + "cls_token"].reshape(d), device)
        self.pos = _f32(sd[p + "pos_embed"].reshape(-1, d), device)
        self.blocks = []
        for i in range(geo.depth):
            b = f"{p}blocks.{i}."
            self.blocks.append(dict(
                g1=_f32(sd[b + "norm1.weight"], device), b1=_f32(sd[b + "norm1.bias"], device),
                wqkv=_w16(sd[b + "attn.qkv.weight"], dtype, device), bqkv=_f32(sd[b + "attn.qkv.bias"], device),
                wo=_w16(sd[b + "attn.proj.weight"], dtype, device), bo=_f32(sd[b + "attn.proj.bias"], device),
                g2=_f32(sd[b + "norm2.weight"], device), b2=_f32(sd[b + "norm2.bias"], device),
                w1=_w16(sd[b + "mlp.fc1.weight"], dtype, device), c1=_f32(sd[b + "mlp.fc1.bias"], device),
                w2=_w16(sd[b + "mlp.fc2.weight"], dtype, device), c2=_f32(sd[b + "mlp.fc2.bias"], device)))
        self.gf, self.bf = _f32(sd[p + "norm.weight"], device), _f32(sd[p + "norm.bias"], device)
        # LayerNorm folded into the GEMM behind it (cir_gemm_ln_bias_act, round 5): the rows must BE the operand type (fp16 operands on
        # the fp16 stream) and K a multiple of 128.  ln_fold: 0 off, 1 norm1 -> qkv, 2 also norm2 -> fc1 (measured: the fc1 GEMM with its
        # GELU epilogue loses in the statistics what the dropped pass saves - DESIGN section 4).  Geometry decides, never the batch size.
        self.ln_fold = 0
        if dtype == torch.float16 and self.stream_dtype == torch.float16 and d % 128 == 0:
            self.ln_fold = LN_FOLD_DEFAULT
            for i, blk in enumerate(self.blocks):
                b = f"{p}blocks.{i}."
                blk["qkv_f"] = ops.ln_fold_pack(sd[b + "attn.qkv.weight"].to(device), sd[b + "attn.qkv.bias"].to(device), blk["g1"], blk["b1"])
                if self.ln_fold >= 2:     # norm2 -> fc1 only on request (measured slower: 57 MB of packed weights nobody reads otherwise)
                    blk["fc1_f"] = ops.ln_fold_pack(sd[b + "mlp.fc1.weight"].to(device), sd[b + "mlp.fc1.bias"].to(device), blk["g2"], blk["b2"])

    def forward(self, image: Optional[torch.Tensor], want32: bool = False, chunk: int = 4096, out32: Optional[torch.Tensor] = None,
                out16: Optional[torch.Tensor] = None, patches: Optional[torch.Tensor] = None):
        """(B,3,H,W) fp32/16-bit -> tokens (B, N, D): 16-bit always, fp32 too if `want32`.  `out32` / `out16`: write the
        tokens there (contiguous (B, N, D) tensors) - the chunked path hands each chunk its slice of ONE result tensor, so
        no concatenation copy follows (2 GB per 6784 images at 224 px).  `patches` (default None): the patch operand rows
        (B * P, 3 p p) in the engine's operand type, as ops.patchify writes them - the device transform's direct output
        (preprocess.DeviceTransform.batch(..., patches=True)); `image` is then ignored and no patchify launch is issued."""
        if patches is not None:
            return self._forward_patches(patches, want32, chunk, out32, out16)
        geo, dt = self.geo, self.dtype
        bsz, d, n = image.shape[0], geo.width, geo.num_tokens
        if bsz > chunk:
            n_parts = -(-bsz // chunk)
            size = -(-bsz // n_parts)                                          # balanced chunks (no ragged tail)
            y16 = torch.empty((bsz, n, d), dtype=dt, device=image.device) if out16 is None else out16
            if dt == torch.float32 and want32 and out32 is None:
                y32 = y16                                                      # "exact" mode: one fp32 tensor is both results
            else:
                y32 = (torch.empty((bsz, n, d), dtype=torch.float32, device=image.device) if out32 is None else out32) if want32 else None
            for i in range(0, bsz, size):
                self.forward(image[i:i + size], want32, chunk, out32=None if y32 is None else y32[i:i + size], out16=y16[i:i + size])
            return y32, y16
        if image.shape[-1] != geo.image_size or image.shape[-2] != geo.image_size:
            raise ValueError(f"image size {tuple(image.shape[-2:])} != model image_size {geo.image_size}")
        if image.dtype not in (torch.float32, dt):
            image = image.float()
        return self._encode(ops.patchify(image, geo.patch_size, dt), bsz, want32, out32, out16)   # PatchEmbed im2col

    def _forward_patches(self, patches: torch.Tensor, want32: bool, chunk: int, out32: Optional[torch.Tensor], out16: Optional[torch.Tensor]):
        """`forward` from the patch operand rows: the same chunking, no patchify launch."""
        geo, dt = self.geo, self.dtype
        p, d, n = geo.num_tokens - 1, geo.width, geo.num_tokens
        if patches.dim() != 2 or patches.dtype != dt or patches.shape[1] != 3 * geo.patch_size ** 2 or patches.shape[0] % p or not patches.is_contiguous():
            raise ValueError(f"patch rows {tuple(patches.shape)} {patches.dtype}: expected contiguous (B * {p}, {3 * geo.patch_size ** 2}) {dt}")
        bsz = patches.shape[0] // p
        if bsz <= chunk:
            return self._encode(patches, bsz, want32, out32, out16)
        n_parts = -(-bsz // chunk)
        size = -(-bsz // n_parts)
        y16 = torch.empty((bsz, n, d), dtype=dt, device=patches.device) if out16 is None else out16
        if dt == torch.float32 and want32 and out32 is None:
            y32 = y16
        else:
            y32 = (torch.empty((bsz, n, d), dtype=torch.float32, device=patches.device) if out32 is None else out32) if want32 else None
        for i in range(0, bsz, size):
            self._encode(patches[i * p:(i + size) * p], min(size, bsz - i), want32, None if y32 is None else y32[i:i + size], y16[i:i + size])
        return y32, y16

    def _encode(self, patches: torch.Tensor, bsz: int, want32: bool, out32: Optional[torch.Tensor], out16: Optional[torch.Tensor]):
        """Patch rows (bsz * P, 3 p p) -> tokens: everything of `forward` behind the im2col."""
        geo, dt = self.geo, self.dtype
        d, n = geo.width, geo.num_tokens
        scale = 64 ** -0.5                                                     # vit.py:50
        sdt = self.stream_dtype
        proj = ops.gemm(patches, self.w_patch, self.b_patch, out_dtype=sdt)
        x = ops.vit_assemble(proj, self.cls, self.pos, bsz).view(bsz * n, d)   # vit.py:184-187 (residual stream, sdt)
        ctx = torch.empty((bsz, n, d), dtype=dt, device=x.device)
        for blk in self.blocks:
            if self.ln_fold >= 1:
                qkv = ops.gemm_ln(x, *blk["qkv_f"], geo.layer_norm_eps).view(bsz, n, 3, d)   # vit.py:107 + :72, no LayerNorm pass
            else:
                _, xb = _ln(x, blk["g1"], blk["b1"], geo.layer_norm_eps, dt, sdt, need_stream=False)
                qkv = ops.gemm(xb, blk["wqkv"], blk["bqkv"]).view(bsz, n, 3, d)    # vit.py:72
            ops.attention(qkv[:, :, 0].unsqueeze(1), qkv[:, :, 1].unsqueeze(1), qkv[:, :, 2].unsqueeze(1),
                          ctx.unsqueeze(1), scale)                             # vit.py:73-83
            ops.gemm(ctx.view(bsz * n, d), blk["wo"], blk["bo"], residual=x, out_dtype=sdt, out=x)  # :84,:108
            if self.ln_fold >= 2 and "fc1_f" in blk:
                f = ops.gemm_ln(x, *blk["fc1_f"], geo.layer_norm_eps, act=ops.ACT_GELU)   # vit.py:109 + :36-37
            else:
                _, xb = _ln(x, blk["g2"], blk["b2"], geo.layer_norm_eps, dt, sdt, need_stream=False)
                f = ops.gemm(xb, blk["w1"], blk["c1"], act=ops.ACT_GELU)       # vit.py:36-37
            ops.gemm(f, blk["w2"], blk["c2"], residual=x, out_dtype=sdt, out=x)  # vit.py:39, :109
        if dt == torch.float32:                                                # "exact" mode: one fp32 token tensor serves both roles
            o = out16 if out16 is not None else out32
            y32, _ = ops.layernorm(x, self.gf, self.bf, geo.layer_norm_eps, want32=True, dtype16=None, stream_dtype=torch.float32,
                                   out32=None if o is None else o.view(bsz * n, d))
            if out16 is not None and out32 is not None and out32.data_ptr() != out16.data_ptr():
                out32.copy_(out16)
            return (y32.view(bsz, n, d) if want32 else None), y32.view(bsz, n, d)
        y32, y16 = ops.layernorm(x, self.gf, self.bf, geo.layer_norm_eps, want32=want32, dtype16=dt, stream_dtype=torch.float32,
                                 out32=None if (out32 is None or not want32) else out32.view(bsz * n, d),
                                 out16=None if out16 is None else out16.view(bsz * n, d))                                       # vit.py:192
        return (y32.view(bsz, n, d) if want32 else None), y16.view(bsz, n, d)


    @torch.no_grad()
    def forward_drop_path(self, image: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
        """The same encoder with timm's DropPath around both residual branches of every block (vit.py:98-109; blip_stage2.py:37 builds the
        stage-II image encoder with drop_path_rate 0.1): `scales` (depth, 2, B) fp32 holds 0 for a dropped (block, branch, sample) and
        1 / keep for a kept one.  What `img_embed` runs in .train() mode WITHOUT a graph (frozen ViT, stage2_train.py:183-190 under
        torch.no_grad(): the reference's DropPath modules are active there) - round 6.  fp32 residual stream, the engine's 16-bit weights;
        returns fp32 tokens (B, N, D).  Not a benchmark path: the branch outputs take a separate scale-and-add pass."""
        from . import train_ops as T
        geo, dt = self.geo, self.dtype
        if dt == torch.float32:
            raise RuntimeError("DropPath embeds run on 16-bit operands: leave the exact mode for training")
        bsz, d, n = image.shape[0], geo.width, geo.num_tokens
        assert tuple(scales.shape) == (geo.depth, 2, bsz) and scales.dtype == torch.float32
        if image.dtype not in (torch.float32, dt):
            image = image.float()
        f32 = torch.float32
        patches = ops.patchify(image.contiguous(), geo.patch_size, dt)
        x = ops.vit_assemble(ops.gemm(patches, self.w_patch, self.b_patch, out_dtype=f32), self.cls, self.pos, bsz).view(bsz * n, d)
        ctx = torch.empty((bsz, n, d), dtype=dt, device=x.device)
        for i, blk in enumerate(self.blocks):
            _, xb = ops.layernorm(x, blk["g1"], blk["b1"], geo.layer_norm_eps, want32=False, dtype16=dt, stream_dtype=f32)
            qkv = ops.gemm(xb, blk["wqkv"], blk["bqkv"]).view(bsz, n, 3, d)
            ops.attention(qkv[:, :, 0].unsqueeze(1), qkv[:, :, 1].unsqueeze(1), qkv[:, :, 2].unsqueeze(1), ctx.unsqueeze(1), 64 ** -0.5)
            x = T.rows_scale_add(x, ops.gemm(ctx.view(bsz * n, d), blk["wo"], blk["bo"], out_dtype=f32), scales[i, 0].contiguous(), n)   # vit.py:108
            _, xb = ops.layernorm(x, blk["g2"], blk["b2"], geo.layer_norm_eps, want32=False, dtype16=dt, stream_dtype=f32)
            f = ops.gemm(xb, blk["w1"], blk["c1"], act=ops.ACT_GELU)
            x = T.rows_scale_add(x, ops.gemm(f, blk["w2"], blk["c2"], out_dtype=f32), scales[i, 1].contiguous(), n)                       # vit.py:109
        y32, _ = ops.layernorm(x, self.gf, self.bf, geo.layer_norm_eps, want32=True, dtype16=None, stream_dtype=f32)
        return y32.view(bsz, n, d)


# =================================================================================================
class KVBank(list):
    """Per-layer cross-attention K|V of an index-feature bank: entry i is (n_index, N, 4D) - or None for
    the last layer when its K / V projections are folded out of the token side, which then reads `tokens` (the 16-bit
    index features themselves) through cir_cls_cross_attention's row index.  `engine`: weak reference to the NlvrEngine that built it -
    a bank holds projections of that engine's weights, and `NlvrEngine.forward` refuses it from any other (a repacked engine: the
    parameters were written since the bank was built)."""
    tokens: Optional[torch.Tensor] = None
    engine = None


def _cat(sd: SD, keys, suffix: str) -> torch.Tensor:
    return torch.cat([sd[k + suffix].detach().float() for k in keys], dim=0)


class MedEngine:
    """Stage-I BERT/MED text encoder with image cross-attention (med.py:348-398, 685-821) -> z_t."""

    def __init__(self, sd: SD, geo: BertGeometry, dtype: torch.dtype, device, prefix: str = "text_encoder.",
                 stream_dtype: Optional[torch.dtype] = None, cross_dtype: Optional[torch.dtype] = None, split3: bool = False):
        geo.validate()
        self.geo, self.dtype, self.device, self.stream_dtype = geo, dtype, device, _auto_stream(dtype, stream_dtype)
        self.split = _split_mode(split3, dtype, geo)
        self.split3 = self.split != 0
        self.xdtype = xdt = cross_dtype or dtype       # operand type of the image-facing block (module docstring)
        e = prefix + "embeddings."
        self.word, self.posemb = _f32(sd[e + "word_embeddings.weight"], device), _f32(sd[e + "position_embeddings.weight"], device)
        self.ge, self.be = _f32(sd[e + "LayerNorm.weight"], device), _f32(sd[e + "LayerNorm.bias"], device)
        self.layers = []
        for i in range(geo.num_hidden_layers):
            p = f"{prefix}encoder.layer.{i}."
            sa, ca = p + "attention.self.", p + "crossattention.self."
            self.layers.append(dict(
                wqkv=_w16(_cat(sd, [sa + "query", sa + "key", sa + "value"], ".weight"), dtype, device),
                bqkv=_f32(_cat(sd, [sa + "query", sa + "key", sa + "value"], ".bias"), device),
                wo=_w16(sd[p + "attention.output.dense.weight"], dtype, device), bo=_f32(sd[p + "attention.output.dense.bias"], device),
                g1=_f32(sd[p + "attention.output.LayerNorm.weight"], device), b1=_f32(sd[p + "attention.output.LayerNorm.bias"], device),
                wq=_w16(sd[ca + "query.weight"], xdt, device), bq=_f32(sd[ca + "query.bias"], device),
                wkv=_w16(_cat(sd, [ca + "key", ca + "value"], ".weight"), xdt, device),
                bkv=_f32(_cat(sd, [ca + "key", ca + "value"], ".bias"), device),
                wco=_w16(sd[p + "crossattention.output.dense.weight"], xdt, device), bco=_f32(sd[p + "crossattention.output.dense.bias"], device),
                g2=_f32(sd[p + "crossattention.output.LayerNorm.weight"], device), b2=_f32(sd[p + "crossattention.output.LayerNorm.bias"], device),
                w1=_w16(sd[p + "intermediate.dense.weight"], dtype, device), c1=_f32(sd[p + "intermediate.dense.bias"], device),
                w2=_w16(sd[p + "output.dense.weight"], dtype, device), c2=_f32(sd[p + "output.dense.bias"], device),
                g3=_f32(sd[p + "output.LayerNorm.weight"], device), b3=_f32(sd[p + "output.LayerNorm.bias"], device)))
        if self.split:
            _mark_split(self.split, self.layers)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, enc16: torch.Tensor,
                enc_mask: Optional[torch.Tensor] = None):
        """ids/mask (Q, L), image tokens (Q, N, Dv) 16-bit (in `xdtype`) -> last hidden state (Q, L, D): (fp32, 16-bit)."""
        geo, dt, sdt, xdt = self.geo, self.dtype, self.stream_dtype, self.xdtype
        q_n, l = input_ids.shape
        d, n = geo.hidden_size, enc16.shape[1]
        r = q_n * l
        eps, scale = geo.layer_norm_eps, 64 ** -0.5
        hs, h16 = ops.embed_layernorm(input_ids, self.word, self.posemb, self.ge, self.be, eps, dt, stream_dtype=sdt)  # med.py:87-110
        hs, h16 = hs.view(r, d), h16.view(r, d)
        smask = additive_self_mask(attention_mask).view(q_n, 1, l)
        emask = additive_encoder_mask(enc_mask).view(q_n, 1, n) if enc_mask is not None else None
        enc2 = enc16.reshape(q_n * n, enc16.shape[2])
        s8 = self.split == 8       # text32 on split8 rows: the LayerNorm / attention / fc1 kernels write the next GEMM's operand themselves
        ctx_x = torch.empty((q_n, 1, l, d), dtype=xdt, device=hs.device)
        for ly in self.layers:
            qkv = ops.gemm(h16, ly["wqkv"], ly["bqkv"]).view(q_n, 1, l, 3 * d)
            ctx_op = _attend(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], scale, smask, dt, s8, (r,))   # med.py:158-240
            t = ops.gemm(ctx_op, ly["wo"], ly["bo"], residual=hs, out_dtype=sdt)
            a_s, a16 = _ln(t, ly["g1"], ly["b1"], eps, xdt, sdt)                                       # med.py:250-253 (operand copy feeds cross-Q only)
            qc = ops.gemm(a16, ly["wq"], ly["bq"]).view(q_n, 1, l, d)
            kv = ops.gemm(enc2, ly["wkv"], ly["bkv"]).view(q_n, 1, n, 2 * d)
            ops.attention(qc, kv[..., :d], kv[..., d:], ctx_x, scale, emask)                           # med.py:361-376
            t = ops.gemm(ctx_x.view(r, d), ly["wco"], ly["bco"], residual=a_s, out_dtype=sdt)
            c_s, c16 = _ln(t, ly["g2"], ly["b2"], eps, dt, sdt, split8=s8)
            f = ops.gemm(c16, ly["w1"], ly["c1"], act=ops.ACT_GELU)                                    # med.py:319-322
            t = ops.gemm(f, ly["w2"], ly["c2"], residual=c_s, out_dtype=sdt)
            hs, h16 = _ln(t, ly["g3"], ly["b3"], eps, dt, sdt, split8=s8)                              # med.py:331-335
        if s8:
            h16 = hs
        h32 = hs if hs.dtype == torch.float32 else ops.gather_rows(hs, None, torch.float32)            # API: fp32 last_hidden_state
        return h32.view(q_n, l, d), h16.view(q_n, l, d)


# =================================================================================================
class LayerPlan(NamedTuple):
    """One fusion layer of a `Plan`."""
    cls_only: bool          # per-token work on the CLS rows only (the trimmed last layer)
    cross: str              # cross-attention path: "cls_fold", "fold_short", "fold32", "fold_long", "fold_long_wide", "projected" or "bank"
    sdt: torch.dtype        # residual-stream type the layer receives ...
    sdt_out: torch.dtype    # ... and the one its last LayerNorm writes (the next layer's)


class Plan(NamedTuple):
    """What `NlvrEngine.plan` returns.  Hashable, no tensors: with the argument shapes it is the key of a captured graph."""
    layers: Tuple[LayerPlan, ...]
    kv_chunk: int           # candidates per K|V + cross-attention chunk of the "projected" layers (0 = all at once)
    fallback: bool          # the call counts in `fold_fallbacks`: long captions on the projected path although the fold is on


SCALE = 64 ** -0.5          # every attention head of the text side is 64 wide


class NlvrEngine:
    """Stage-II two-branch BERT + cls_head (nlvr_encoder.py:414-476, 777-908; blip_stage2.py:50-54, 101-136).

    Layout: hidden states are (branch, row, D) with row = candidate * L + token.  Per layer:
    batched(2) QKV GEMM -> self-attention -> batched out-proj(+residual) -> LayerNormA/B ->
    batched cross-Q GEMM; ONE K|V GEMM over the candidate tokens for both branches
    ([K0;V0;K1;V1] stacked, N = 4D); cross-attention writes [c0|c1] rows; the merge is a single
    K = 2D GEMM ([.5 W0 | .5 W1] for the averaging layers, [Wm_a W0 | Wm_b W1] folded for the
    merge_layer ones - `fold_merge=False` keeps dense0/dense1 and merge_layer as separate GEMMs);
    twin LayerNorm with the shared merged tensor; FFN on both branches as one M = 2R GEMM pair.
    Layer 0's self-attention block is candidate-independent and runs once per QUERY.

    Which of these launches a call issues is decided in one place: `plan` maps the call's sizes and the live switches (plain attributes,
    set between calls: `trim_last`, `kv_chunk`, `fold_cls_kv`, `fold_cross_kv`, `fold_long`, `fold_long_wide`, `fold_short`, `stream32_from`, `cls_fold`) to a `Plan` before
    the first launch; `forward` executes it and `forward_graphed` keys its captures with it.  A new host-side switch belongs in `plan`.
    """

    def __init__(self, sd: SD, geo: BertGeometry, dtype: torch.dtype, device, prefix: str = "text_encoder.", fold_merge: bool = True,
                 stream_dtype: Optional[torch.dtype] = None, cross_dtype: Optional[torch.dtype] = None, split3: bool = False):
        geo.validate()
        self.geo, self.dtype, self.device, self.fold_merge, self.stream_dtype = geo, dtype, device, fold_merge, _auto_stream(dtype, stream_dtype)
        self.split = _split_mode(split3, dtype, geo)
        self.split3 = self.split != 0
        self.xdtype = xdt = cross_dtype or dtype   # operand type of the cross-attention block = type of the candidate tokens (module docstring)
        self.trim_last = True   # last layer: per-token work on the CLS rows only (results identical for the rows that are used)
        self.kv_chunk = 0       # candidates per K|V + cross-attention chunk (0 = all at once; attribute, for A/B runs)
        self.fold_cls_kv = xdt != torch.float32  # last layer: fold the cross K / V projections out of the token side (False: K|V GEMM +
                                                 # attention; the "exact" fp32 mode keeps the reference's order of operations)
        # Round 5: the OTHER layers' cross-attention with the K / V projections folded to the query side (cir_cross_attention_folded:
        # S = (q W_k) X^T, ctx = (P X) W_v^T + b_v - 614 instead of 969 MFLOP per candidate and layer, and no (T N, 4 D) K|V tensor).
        # Taken when the geometry is the kernels' (D = Dv = 768, 12 heads, L <= 32, N <= 608: 224 px and the reference's 384 px), with or
        # without a key mask (round 6), no K/V bank; anything else keeps the projected path (captions of more than 32 tokens: `fold_fallbacks`
        # counts those calls - the kernels' 48-row-per-wave tiling would run them as two passes, which the projected path beats below ~56 tokens).
        self.fold_cross_kv = xdt != torch.float32 and geo.hidden_size == 768 and geo.encoder_width == 768 and geo.num_attention_heads == 12
        self.fold_fallbacks = 0      # forward calls whose captions (> 32 tokens) took the projected path although the fold is on: visible, not silent
        # Captions of 33 .. 64 tokens against at most 224 keys: with `fold_long` on they take cir_cross_attention_folded_long (one head and up to
        # three 16-token blocks per wave; cost in 16-token steps) instead of the projected path, and `fold_fallbacks` does not move.  Off by default:
        # it measures faster than the projected path at 33-48 tokens and slower at 49-64 (LABNOTES.md section 14); a default per length is a later
        # change (BLIP_NLVR.set_long_caption_fold).
        self.fold_long = False
        # Captions of at most 16 tokens: with `fold_short` on they take cir_cross_attention_folded_short (one 16-token block per head: 12 blocks
        # per candidate and branch where the 32-token kernels run 24) at up to 608 keys.  Off by default: per layer it measures 7-8 % faster than
        # fold16 at 577 keys and 19-28 % slower than the 224-key kernel at 197 (LABNOTES.md section 18) - worth turning on for 384-px runs only
        # (BLIP_NLVR.set_short_caption_fold).
        self.fold_short = False
        # Captions of 33 .. 64 tokens against 225 .. 608 keys (384 px: 577): with `fold_long_wide` on they take cir_cross_attention_folded_long_wide
        # (four waves per head: two token halves x two key halves) instead of the projected path, and `fold_fallbacks` does not move.  A second
        # switch: `fold_long` alone keeps sending this geometry to the projected path.  Off by default whatever it measures (LABNOTES.md
        # section 21; BLIP_NLVR.set_long_caption_fold_wide).
        self.fold_long_wide = False
        self.stream32_from = None    # layers >= this index keep their residual stream in fp32 (None: `stream_dtype` everywhere)
        self._graphs = {}            # graph_key -> ScoreGraph, in recency order (`forward_graphed`)
        e = prefix + "embeddings."
        self.word, self.posemb = _f32(sd[e + "word_embeddings.weight"], device), _f32(sd[e + "position_embeddings.weight"], device)
        self.ge, self.be = _f32(sd[e + "LayerNorm.weight"], device), _f32(sd[e + "LayerNorm.bias"], device)
        d = geo.hidden_size
        self.layers = []
        for i in range(geo.num_hidden_layers):
            p = f"{prefix}encoder.layer.{i}."
            ly = {}
            sa = [p + f"attention.self{b}." for b in (0, 1)]
            ca = [p + f"crossattention.self{b}." for b in (0, 1)]
            ly["wqkv"] = _w16(torch.stack([_cat(sd, [s + "query", s + "key", s + "value"], ".weight") for s in sa]), dtype, device)
            ly["bqkv"] = _f32(torch.stack([_cat(sd, [s + "query", s + "key", s + "value"], ".bias") for s in sa]), device)
            ly["wo"] = _w16(torch.stack([sd[p + f"attention.output.dense{b}.weight"].float() for b in (0, 1)]), dtype, device)
            ly["bo"] = _f32(torch.stack([sd[p + f"attention.output.dense{b}.bias"].float() for b in (0, 1)]), device)
            ly["g1"] = _f32(torch.stack([sd[p + f"attention.output.LayerNorm{c}.weight"] for c in "AB"]), device)
            ly["b1"] = _f32(torch.stack([sd[p + f"attention.output.LayerNorm{c}.bias"] for c in "AB"]), device)
            ly["wq"] = _w16(torch.stack([sd[c + "query.weight"].float() for c in ca]), xdt, device)
            ly["bq"] = _f32(torch.stack([sd[c + "query.bias"].float() for c in ca]), device)
            kv_keys = [ca[0] + "key", ca[0] + "value", ca[1] + "key", ca[1] + "value"]
            ly["wkv"] = _w16(_cat(sd, kv_keys, ".weight"), xdt, device)           # (4D, Dv)
            ly["bkv"] = _f32(_cat(sd, kv_keys, ".bias"), device)
            if self.fold_cross_kv:        # query-side fold: W_k^T per branch, W_v with its columns in MFMA k-slot order, b_v (b_k drops out of the softmax)
                ly["wkt"] = ops.fold_pack_key(_w16(torch.stack([sd[c + "key.weight"].detach().float() for c in ca]), xdt, device))
                ly["wvp"] = ops.fold_pack_value(_w16(torch.stack([sd[c + "value.weight"].detach().float() for c in ca]), xdt, device))
                ly["bvf"] = _f32(torch.stack([sd[c + "value.bias"].detach().float() for c in ca]), device)
            # one-time weight preparation in fp64 on the host (keeps library GEMMs out of the device timeline)
            w0 = sd[p + "crossattention.output.dense0.weight"].detach().cpu().double()
            w1 = sd[p + "crossattention.output.dense1.weight"].detach().cpu().double()
            c0 = sd[p + "crossattention.output.dense0.bias"].detach().cpu().double()
            c1 = sd[p + "crossattention.output.dense1.bias"].detach().cpu().double()
            mk = p + "crossattention.output.merge_layer"
            if mk + ".weight" in sd:                                               # layers >= 6: nlvr_encoder.py:252-256
                wm, bm = sd[mk + ".weight"].detach().cpu().double(), sd[mk + ".bias"].detach().cpu().double()
                if fold_merge:
                    ly["wm"] = _w16(torch.cat([wm[:, :d] @ w0, wm[:, d:] @ w1], dim=1).float(), xdt, device)
                    ly["bm"] = _f32((wm[:, :d] @ c0 + wm[:, d:] @ c1 + bm).float(), device)
                else:
                    ly["wd"] = _w16(torch.stack([w0, w1]).float(), xdt, device)
                    ly["bd"] = _f32(torch.stack([c0, c1]).float(), device)
                    ly["wm"] = _w16(wm.float(), xdt, device)
                    ly["bm"] = _f32(bm.float(), device)
            else:                                                                  # layers < 6: nlvr_encoder.py:257-260
                ly["wm"] = _w16(torch.cat([0.5 * w0, 0.5 * w1], dim=1).float(), xdt, device)
                ly["bm"] = _f32((0.5 * (c0 + c1)).float(), device)
            ly["g2"] = _f32(torch.stack([sd[p + f"crossattention.output.LayerNorm{c}.weight"] for c in "AB"]), device)
            ly["b2"] = _f32(torch.stack([sd[p + f"crossattention.output.LayerNorm{c}.bias"] for c in "AB"]), device)
            ly["w1"] = _w16(sd[p + "intermediate.dense.weight"], dtype, device)
            ly["c1"] = _f32(sd[p + "intermediate.dense.bias"], device)
            ly["w2"] = _w16(sd[p + "output.dense.weight"], dtype, device)
            ly["c2"] = _f32(sd[p + "output.dense.bias"], device)
            ly["g3"] = _f32(sd[p + "output.LayerNorm.weight"], device)
            ly["b3"] = _f32(sd[p + "output.LayerNorm.bias"], device)
            self.layers.append(ly)
        # Last layer, CLS rows only: the cross K / V projections fold out of the token side (cir_cls_cross_attention) -
        # per (branch, head) W_k^T as a (Dv, 64) GEMM weight for q -> qp, W_v rows as a (64, Dv) one for sum_j p_j x_j -> ctx
        h_n, dv = geo.num_attention_heads, geo.encoder_width
        self.cls_fold = None
        if geo.num_hidden_layers > 1 and 2 * h_n <= 32 and dv % 128 == 0 and dv <= 768 and d == h_n * 64:
            p = f"{prefix}encoder.layer.{geo.num_hidden_layers - 1}.crossattention."
            wk = [sd[p + f"self{b}.key.weight"].detach().float() for b in (0, 1)]                    # (D, Dv)
            wv = [sd[p + f"self{b}.value.weight"].detach().float() for b in (0, 1)]
            bv = [sd[p + f"self{b}.value.bias"].detach().float() for b in (0, 1)]
            self.cls_fold = dict(
                wkt=[_w16(w.view(h_n, 64, dv).transpose(1, 2).contiguous(), xdt, device) for w in wk],     # (H, Dv, 64) per branch
                wv=_w16(torch.cat(wv).view(2 * h_n, 64, dv), xdt, device),                                 # (2H, 64, Dv)
                bv=_f32(torch.cat(bv).view(2 * h_n, 64), device), qp={})
        self.wc0, self.bc0 = _w16(sd["cls_head.0.weight"], dtype, device), _f32(sd["cls_head.0.bias"], device)
        self.wc2, self.bc2 = _w16(sd["cls_head.2.weight"], dtype, device), _f32(sd["cls_head.2.bias"], device)
        if self.split:
            _mark_split(self.split, self.layers, self.wc0)

    # ---------------------------------------------------------------------------------------------
    def plan(self, l: int, n: int, dv: int, masked: bool, bank: Optional[Tuple[bool, ...]] = None) -> Plan:
        """Every host-side decision of a forward for captions of `l` tokens against `n` keys of width `dv`, with (`masked`) or without a
        candidate mask, on candidate tokens (`bank` None) or a K/V bank (`bank[i]`: the bank holds no K|V of layer i): a pure function of
        these and of the live switches (class docstring)."""
        d, dt, s32, last = self.geo.hidden_size, self.dtype, self.stream32_from, len(self.layers) - 1
        sd = lambda i: torch.float32 if (s32 is not None and i >= s32 and dt != torch.float32) else self.stream_dtype
        layers = []
        for i, ly in enumerate(self.layers):
            cls_only = self.trim_last and i == last and i > 0
            no_kv = bank is not None and bank[i]
            foldable = bank is None and self.fold_cross_kv and "wkt" in ly and not cls_only and dv == d
            if cls_only and not masked and self.cls_fold is not None and self.fold_cls_kv and (bank is None or no_kv):
                cross = "cls_fold"
            elif no_kv:
                raise ValueError("this K/V bank was built with the last layer folded (no K|V of that layer): rebuild it with fold_cls_kv = False")
            elif foldable and self.fold_short and l <= 16 and n <= 608:
                cross = "fold_short"
            elif foldable and l <= 32 and n <= 608:
                cross = "fold32"
            elif foldable and self.fold_long and 33 <= l <= 64 and n <= 224:
                cross = "fold_long"
            elif foldable and self.fold_long_wide and 33 <= l <= 64 and 225 <= n <= 608:
                cross = "fold_long_wide"
            else:
                cross = "projected" if bank is None else "bank"
            layers.append(LayerPlan(cls_only, cross, sd(i), sd(i + 1)))
        # counted where layer 1 projects although the engine folds.  Bookkeeping, not a launch: it makes the graph key finer than the
        # launches need (fold_cross_kv off at 40 tokens issues the default's launches under a key of its own - one slot of the LRU)
        fallback = last >= 1 and layers[1].cross == "projected" and self.fold_cross_kv and "wkt" in self.layers[1] and l > 32
        return Plan(tuple(layers), self.kv_chunk, fallback)

    def graph_key(self, ids_shape, cand_shape, cand_dtype) -> tuple:
        """What a captured graph of `forward` is valid for: the problem and its plan."""
        return (tuple(ids_shape), tuple(cand_shape), cand_dtype, self.plan(ids_shape[1], cand_shape[1], cand_shape[2], False))

    @torch.no_grad()
    def build_kv_bank(self, bank16: torch.Tensor, chunk: int = 512) -> list:
        """Cross-attention K|V of every index image for every layer and both branches:
        bank16 (n_index, N, Dv) 16-bit -> 12 tensors (n_index, N, 4D) = [K0 V0 K1 V1].  These projections are
        query-independent (45 % of the fusion flops at 224 px); a real dataset re-uses a few thousand index images
        across 1e5-1e6 candidate slots, and 288 GB of HBM holds the whole bank (CIRR val at 384 px: 98 GB)."""
        n_idx, n, dv = bank16.shape
        d = self.geo.hidden_size
        out = KVBank()
        out.tokens = bank16
        out.engine = weakref.ref(self)
        last = len(self.layers) - 1
        for i, ly in enumerate(self.layers):
            if i == last and self.trim_last and last > 0 and self.cls_fold is not None and self.fold_cls_kv:
                out.append(None)            # the folded last layer attends the raw tokens: no K|V of this layer is ever formed
                continue
            kv = torch.empty((n_idx, n, 4 * d), dtype=self.xdtype, device=bank16.device)
            for i0 in range(0, n_idx, chunk):
                rows = bank16[i0:i0 + chunk].reshape(-1, dv)
                ops.gemm(rows, ly["wkv"], ly["bkv"], out=kv[i0:i0 + chunk].view(-1, 4 * d))
            out.append(kv)
        return out

    def forward_graphed(self, input_ids, attention_mask, z_t32, cand16, qidx) -> torch.Tensor:
        """`forward` through a captured HIP graph per problem shape (ScoreGraph); at most 8 are kept (least recently used dropped).
        A capture freezes every host-side branch of `forward`.  Those branches are the plan's and nothing else's, and the plan is part of the
        key (`graph_key`): changing a live A/B switch takes a new capture where it changes the plan, instead of replaying the old path.
        `lib.set_tuning` is not in the plan: the kernel selection in force at capture time stays frozen into the graph.  Replays share the
        graph's static buffers: one stream at a time.  With bench.py's per-launch event profiling on (ops.PROFILE_*) nothing is captured -
        events would be recorded inside."""
        if ops.PROFILE_GEMM is not None or ops.PROFILE_ATTN is not None:
            return self.forward(input_ids, attention_mask, z_t32, cand16, qidx)
        graphs = self._graphs
        z_t32 = z_t32.float().contiguous()
        key = self.graph_key(input_ids.shape, cand16.shape, cand16.dtype)
        g = graphs.pop(key, None)
        if g is None:
            if len(graphs) >= 8:
                graphs.pop(next(iter(graphs)))
            g = ScoreGraph(self, input_ids.contiguous(), attention_mask.contiguous(), z_t32, cand16.contiguous(), qidx.contiguous())
        graphs[key] = g                                   # (re-)inserted last: the dict's order is the recency order
        return g(input_ids, attention_mask, z_t32, cand16, qidx)

    # --------------------------------------------------------------------------------------------- the blocks `forward` schedules
    def _self_block(self, ly, h32, h16, items, l, smask, sdt, lq=None):
        """Twin self-attention + LayerNormA/B on (2, items*L, D) hidden states (nlvr_encoder.py:427-433, 262-264).  The 16-bit
        copy of the result feeds the cross-attention query projection only: it is written in `xdtype`.  `lq = 1`: the CLS-only layer -
        every token is still a key / value, the query, the context and the residual are the CLS rows (a strided view of `h32`)."""
        d, eps, lq = self.geo.hidden_size, self.geo.layer_norm_eps, lq or l
        qkv = ops.gemm(h16, ly["wqkv"], ly["bqkv"]).view(2, items, l, 3 * d)
        ctx_op = _attend(qkv[:, :, :lq, :d], qkv[..., d:2 * d], qkv[..., 2 * d:], SCALE, smask.unsqueeze(0).expand(2, items, l), self.dtype,
                         self.split == 8, (2, items * lq))
        t = ops.gemm(ctx_op, ly["wo"], ly["bo"], residual=h32 if lq == l else h32.view(2, items, l, d)[:, :, 0, :], out_dtype=sdt)
        return _ln(t, ly["g1"], ly["b1"], eps, self.xdtype, sdt)

    def _query_block(self, input_ids, attention_mask, z_t32, qidx, t_n, sdt):
        """Embeddings and layer 0's self-attention block: they depend on (z_t, caption) only, so they run once per QUERY and are then
        expanded to the candidates -> (stream rows, cross-Q operand rows) (2, T L, D) and the (T, L) self-attention key mask."""
        geo, dt, xdt = self.geo, self.dtype, self.xdtype
        (q_n, l), d = input_ids.shape, geo.hidden_size
        emb32, _ = ops.embed_layernorm(input_ids, self.word, self.posemb, self.ge, self.be, geo.layer_norm_eps, dt)   # nlvr_encoder.py:880-886
        if tuple(z_t32.shape) != tuple(emb32.shape):
            raise AssertionError("left and right inputs shall be the same shape")                         # nlvr_encoder.py:891
        hq32 = torch.stack([z_t32.reshape(q_n * l, d).float(), emb32.view(q_n * l, d)])                   # (2, Q*L, D): [z_t, emb] :892
        hq_s = hq32 if sdt == torch.float32 else ops.gather_rows(hq32.view(2 * q_n * l, d), None, sdt).view(2, q_n * l, d)
        hq16 = hq_s if dt == sdt else ops.gather_rows(hq32.view(2 * q_n * l, d), None, dt).view(2, q_n * l, d)
        smask_q = additive_self_mask(attention_mask)                                                     # (Q, L)
        a_sq, a16q = self._self_block(self.layers[0], hq_s, hq16, q_n, l, smask_q, sdt)
        both = torch.cat([qidx, qidx + q_n])                                                              # rows of (2*Q, L*D)
        a32 = ops.gather_rows(a_sq.view(2 * q_n, l * d), both, sdt).view(2, t_n * l, d)
        a16 = a32 if xdt == sdt else ops.gather_rows(a16q.view(2 * q_n, l * d), both, xdt).view(2, t_n * l, d)
        return a32, a16, ops.gather_rows(_pad8(smask_q), qidx, torch.float32)[:, :l]

    def _cross_block(self, ly, lp: LayerPlan, a16, cc, tok, emask2d, rows, kv, kv_chunk):
        """Cross-attention query projection and the cross-attention on the layer's planned path -> [c0 | c1] rows (T, Lq, 2, D).  `tok`: the
        candidate tokens (T, N, Dv), or the bank's (n_index, N, Dv) with the bank rows `rows` and the layer's K|V `kv`."""
        d, (t_n, l), n = self.geo.hidden_size, cc.shape[:2], tok.shape[1]
        qraw = ops.gemm(a16, ly["wq"], ly["bq"])                                                        # (2, T Lq, D)
        qc = qraw.view(2, t_n, -1, d).permute(1, 0, 2, 3)                                                 # (T, 2, Lq, D) view
        ccl = cc if not lp.cls_only else torch.empty((t_n, 1, 2, d), dtype=self.xdtype, device=cc.device)
        emask = None if emask2d is None else emask2d.view(t_n, 1, n).expand(t_n, 2, n)
        if lp.cross == "cls_fold":
            self._cross_cls_fold(qc, ccl, tok, rows)
        elif lp.cross in ("fold_short", "fold32", "fold_long", "fold_long_wide"):
            fold = getattr(ops, {"fold_short": "cross_attention_folded_short", "fold32": "cross_attention_folded", "fold_long": "cross_attention_folded_long",
                                 "fold_long_wide": "cross_attention_folded_long_wide"}[lp.cross])
            fold(qraw, tok, ly["wkt"], ly["wvp"], ly["bvf"], ccl, l, SCALE, heads=self.geo.num_attention_heads, mask=emask2d)
        elif lp.cross == "projected":
            self._cross_projected(ly, qc, ccl, tok, emask, kv_chunk)
        else:                                                                                             # (n_index, N, 4, D) bank
            kv = kv.view(-1, n, 4, d)
            ops.attention(qc, kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3), ccl.permute(0, 2, 1, 3), SCALE, emask,
                          kv_index=rows)
        return ccl

    def _cross_cls_fold(self, qc, ccl, tok, rows):
        """One query row per (branch, head): scores = (W_k^T q) . x_j, context = W_v (sum_j p_j x_j) + b_v - the 4 D x Dv projection of all
        T * N candidate tokens of this layer is never formed (nlvr_encoder.py:321-344)."""
        f, h_n, t_n, dv = self.cls_fold, self.geo.num_attention_heads, ccl.shape[0], tok.shape[2]
        qp = f["qp"].get(t_n)
        if qp is None:                                                                                    # rows >= 2H stay zero
            qp = f["qp"][t_n] = torch.zeros((t_n, 32, dv), dtype=self.xdtype, device=ccl.device)
        q2 = qc.permute(1, 0, 2, 3).reshape(2, t_n, h_n, 64)                                              # view of the (2, T, D) GEMM result
        for b in (0, 1):
            ops.gemm(q2[b].permute(1, 0, 2), f["wkt"][b], None, out=qp[:, b * h_n:(b + 1) * h_n, :].permute(1, 0, 2))
        o = ops.cls_cross_attention(tok, qp, SCALE, x_index=rows)
        ops.gemm(o[:, :2 * h_n, :].permute(1, 0, 2), f["wv"], f["bv"], out=ccl.view(t_n, 2 * h_n, 64).permute(1, 0, 2))

    def _cross_projected(self, ly, qc, ccl, tok, emask, kv_chunk):
        """K|V projection + cross-attention, optionally in candidate chunks (`kv_chunk`; measured: no gain from keeping a chunk's K|V in
        the Infinity Cache, so the default is one launch each)."""
        d, (t_n, n, dv) = self.geo.hidden_size, tok.shape
        cand2 = tok.reshape(t_n * n, dv)
        step_c = kv_chunk if kv_chunk > 0 else t_n
        for c0 in range(0, t_n, step_c):
            c1 = min(c0 + step_c, t_n)
            kv = ops.gemm(cand2[c0 * n:c1 * n], ly["wkv"], ly["bkv"]).view(c1 - c0, n, 4, d)             # [K0 V0 K1 V1]
            ops.attention(qc[c0:c1], kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3),
                          ccl[c0:c1].permute(0, 2, 1, 3), SCALE, None if emask is None else emask[c0:c1])   # nlvr_encoder.py:321-344

    def _merge_ffn(self, ly, lp: LayerPlan, ccl, a32, rq):
        """Merge of the two branches' cross-attention outputs, LayerNormA/B(m + att_b), the shared FFN, the layer's last LayerNorm ->
        next hidden states (stream copy in `lp.sdt_out`, operand copy), each (2, rq, D)."""
        d, dt, eps, xdt, s8 = self.geo.hidden_size, self.dtype, self.geo.layer_norm_eps, self.xdtype, self.split == 8
        if "wd" in ly:                                                                                    # unfolded merge_layer
            dd = torch.empty((rq, 2, d), dtype=xdt, device=ccl.device)
            ops.gemm(ccl.view(rq, 2, d).permute(1, 0, 2), ly["wd"], ly["bd"], out=dd.permute(1, 0, 2))
            m = ops.gemm(dd.view(rq, 2 * d), ly["wm"], ly["bm"], out_dtype=lp.sdt)
        else:
            m = ops.gemm(ccl.view(rq, 2 * d), ly["wm"], ly["bm"], out_dtype=lp.sdt)                      # :252-260
        x32, x16 = _ln(m, ly["g2"], ly["b2"], eps, dt, lp.sdt, residual=a32, split8=s8)                  # LayerNormA/B(m + att_b)
        f = ops.gemm(x16.view(2 * rq, d) if not s8 else x16.view(2 * rq), ly["w1"], ly["c1"], act=ops.ACT_GELU)   # shared FFN :469-476
        t = ops.gemm(f, ly["w2"], ly["c2"], residual=x32.view(2 * rq, d), out_dtype=lp.sdt)
        h32, h16 = _ln(t, ly["g3"], ly["b3"], eps, dt, lp.sdt_out, split8=s8)
        return h32.view(2, rq, d), (h16.view(2, rq, d) if not s8 else h16.view(2, rq))

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, z_t32: torch.Tensor, cand16: Optional[torch.Tensor],
                qidx: torch.Tensor, cand_mask: Optional[torch.Tensor] = None, taps: Optional[list] = None,
                kv_bank: Optional[list] = None, cand_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids/mask (Q, L), z_t (Q, L, D) fp32, candidate tokens (T, N, Dv) 16-bit, qidx (T,) int64 = the
        query each candidate belongs to -> logits (T, 2) fp32 (column 0 is the score).
        With `kv_bank` (from build_kv_bank) and `cand_rows` (T,) int64 bank rows, the per-candidate K|V GEMM is
        skipped and cross-attention reads K/V straight from the bank (cand16 is not used).  Executes `plan`, made before the first launch."""
        d, l = self.geo.hidden_size, input_ids.shape[1]
        if kv_bank is not None:
            if getattr(kv_bank, "engine", None) is None or kv_bank.engine() is not self:
                raise RuntimeError("kv_bank was not built by this engine: the model's parameters were written (or its precision changed) since "
                                   "build_kv_bank - its K/V are projections of the old weights; build the bank again")
            bank, tok, cand_rows = tuple(kv is None for kv in kv_bank), kv_bank.tokens, cand_rows.to(torch.int64).contiguous()
            t_n, n = cand_rows.shape[0], kv_bank[0].shape[1]
        else:
            bank, tok, cand_rows, (t_n, n), kv_bank = None, cand16, None, cand16.shape[:2], [None] * len(self.layers)
        plan = self.plan(l, n, tok.shape[2], cand_mask is not None, bank)
        a32, a16, smask = self._query_block(input_ids, attention_mask, z_t32, qidx, t_n, plan.layers[0].sdt)
        self.fold_fallbacks += plan.fallback               # (counted once the inputs are accepted, as when the count sat in layer 1)
        if plan.fallback and self.fold_fallbacks == 1:
            warnings.warn(f"captions of {l} tokens (> 32): the cross-attention runs the projected K|V path for this batch (~8 % of a step slower than "
                          "the query-side fold at 224 px); NlvrEngine.fold_fallbacks counts such calls; 33-64 tokens against <= 224 keys can take the "
                          "long-caption fold instead: BLIP_NLVR.set_long_caption_fold(); against 225-608 keys (384 px) its key-split form: "
                          "BLIP_NLVR.set_long_caption_fold_wide()", stacklevel=3)
        emask2d = additive_encoder_mask(cand_mask).view(t_n, n) if cand_mask is not None else None       # (T, N): the folded kernels' form
        cc = torch.empty((t_n, l, 2, d), dtype=self.xdtype, device=z_t32.device)
        h32 = h16 = None
        for ly, lp, kv in zip(self.layers, plan.layers, kv_bank):
            lq = 1 if lp.cls_only else l
            if h32 is not None:                # (layer 0's self-attention block ran per query, above)
                a32, a16 = self._self_block(ly, h32, h16, t_n, l, smask, lp.sdt, lq)
            ccl = self._cross_block(ly, lp, a16, cc, tok, emask2d, cand_rows, kv, plan.kv_chunk)
            h32, h16 = self._merge_ffn(ly, lp, ccl, a32, t_n * lq)
            if taps is not None:
                hv = h32.view(2, t_n, lq, d)
                taps.append((hv[0, :, 0, :8].float(), hv[1, :, 0, :8].float()))
        lq = 1 if plan.layers[-1].cls_only else l
        hcls = h32 if self.split == 8 else h16                                                            # (split8: the fp32 stream copy holds the same values)
        hid = hcls.view(2, t_n, lq, d)[:, :, 0, :].permute(1, 0, 2).reshape(t_n, 2 * d)                   # cat(CLS_0, CLS_1) :906-908
        y = ops.gemm(hid, self.wc0, self.bc0, act=ops.ACT_RELU)                                           # blip_stage2.py:50-52
        return ops.small_linear(y, self.wc2, self.bc2)                                                    # blip_stage2.py:53


class ScoreGraph:
    """One captured HIP graph of `NlvrEngine.forward` for a fixed (Q, L, T, N) problem (round 5).  A single query against K = 100
    candidates is ~330 launches of a few microseconds each: issued from Python the call is bound by the host (~30 us per launch), not
    by the GPU.  The launch sequence has no host-side decision and every kernel takes its scalars by value, so it is captured once
    (torch.cuda.CUDAGraph: hipStreamBeginCapture on the stream the C ABI is handed) and replayed with one hipGraphLaunch; inputs are
    copied into the graph's static buffers (30 MB of tokens at K = 100).  Results are bit-identical to the direct call (same kernels,
    same order).  Lives and dies with its engine (a re-packed engine starts without graphs)."""

    def __init__(self, eng: "NlvrEngine", ids, mask, z32, cand16, qidx):
        self.ids, self.mask, self.z, self.cand, self.qidx = (t.clone() for t in (ids, mask, z32, cand16, qidx))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                          # warm-up off the capture: lazy caches (qp buffers, CU count) get built
            for _ in range(2):
                eng.forward(self.ids, self.mask, self.z, self.cand, self.qidx)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = eng.forward(self.ids, self.mask, self.z, self.cand, self.qidx)

    def __call__(self, ids, mask, z32, cand16, qidx) -> torch.Tensor:
        self.ids.copy_(ids); self.mask.copy_(mask); self.z.copy_(z32); self.cand.copy_(cand16); self.qidx.copy_(qidx)
        self.graph.replay()
        return self.out.clone()


def _pad8(m: torch.Tensor) -> torch.Tensor:
    """Pad the last dim of a small fp32 matrix to a multiple of 8 (vector width of cir_gather_rows)."""
    pad = (-m.shape[1]) % 8
    if pad == 0:
        return m.contiguous()
    return torch.cat([m, m.new_zeros((m.shape[0], pad))], dim=1).contiguous()
