"""Stage-I model surface used by the stage-II scoring loop: `BLIP_Retrieval.img_txt_fusion(...,
train=False, return_raw=True)` produces z_t (reference: blip_stage1.py:67-92; called at
validate_stage2.py:106, 244, 264).  State-dict layout = the reference's `["BLIP_Retrieval"]` entry
(472 keys).  The stage-II scripts feed the text encoder image tokens from the stage-II ViT
(validate_stage2.py:139, 293); stage-I retrieval (validate.py) additionally
uses this model's own ViT and the 256-d `vision_proj` / `text_proj` heads (blip_stage1.py:48-65, 83).
"""
from __future__ import annotations

import dataclasses
import os
from typing import Optional, Union

import torch

from . import ops
from .blip_stage2 import _EngineHost, default_tokenizer, encode_text, load_bert_geometry
from .config import BertGeometry, VitGeometry
from .engine import MedEngine, VitEngine
from .param_tree import populate
from .weights import retrieval_param_spec


class EncoderOutput:
    """What callers read from the HF output object: `.last_hidden_state` (blip_stage2.py:106)."""

    def __init__(self, last_hidden_state: torch.Tensor, last_hidden_state16: Optional[torch.Tensor] = None):
        self.last_hidden_state = last_hidden_state
        self.last_hidden_state16 = last_hidden_state16


class BLIP_Retrieval(_EngineHost):
    def __init__(self, med_config: Union[str, dict, BertGeometry] = "configs/med_config.json", image_size: int = 384,
                 vit: str = "base", vit_grad_ckpt: bool = False, vit_ckpt_layer: int = 0, embed_dim: int = 256, *,
                 vit_geometry: Optional[VitGeometry] = None, tokenizer=None):
        super().__init__()
        # blip_stage1.py:34 passes create_vit no drop_path_rate: the stage-I image encoder has no DropPath (the stage-II one has 0.1) - a
        # copy, so that a geometry object shared with a stage-II model keeps its rate
        self.vit_geometry = dataclasses.replace(vit_geometry or VitGeometry.named(vit, image_size), drop_path_rate=0.0)
        self._keep_vit_checkpointing(vit_grad_ckpt, vit_ckpt_layer)            # blip_stage1.py:34
        self.image_tuning = False              # `set_image_tuning`: image features with a graph in .train() mode (--blip-img-tune); off by default
        self.bert_geometry = load_bert_geometry(med_config)
        self.bert_geometry.encoder_width = self.vit_geometry.width
        self.tokenizer = tokenizer if tokenizer is not None else default_tokenizer()
        populate(self, retrieval_param_spec(self.bert_geometry, self.vit_geometry, embed_dim))
        self.text_encoder.config = self.bert_geometry

    def engines(self):
        key = self.weights_key()
        if self._engines is not None and key != self._packed_key:            # a parameter was written since the pack (`weights_key`)
            self._engines = None
        if self._engines is None:
            dev = self.device
            if dev.type != "cuda":
                raise RuntimeError("BLIP_Retrieval runs on an MI355X only: move the model to 'cuda' (no CPU path)")
            sd = self.state_dict()
            f32 = lambda k: sd[k].detach().to(device=dev, dtype=torch.float32).contiguous()
            self._engines = (MedEngine(sd, self.bert_geometry, self.compute_dtype, dev, stream_dtype=self.stream_dtype, cross_dtype=self.token_dtype,
                                       split3=self.text_split3 if self.precision == "text32" else 0),
                             VitEngine(sd, self.vit_geometry, self.token_dtype, dev, stream_dtype=self.vit_stream_dtype),
                             dict(vw=f32("vision_proj.weight"), vb=f32("vision_proj.bias"), tw=f32("text_proj.weight"), tb=f32("text_proj.bias"),
                                  temp=f32("temp").reshape(1)))
            self._packed_key = key
        return self._engines

    def set_image_tuning(self, on: bool = True):
        """Stage-I training with a trainable image encoder (stage1_train.py --blip-img-tune, :144-190 / :383-425).  On: in `.train()` mode
        with grad enabled, `img_embed` returns tokens with a graph through the ViT (`train_vit.vit_train`) where a `visual_encoder.*`
        parameter requires grad, its pooled features carry one into `vision_proj` (and the CLS row) through cir_pooled_head_fwd / _bwd, and
        `img_txt_fusion(..., train=True)` accepts image features that require a gradient and hands it back (`train_stage1.MedTrainer`:
        12 more dgrad GEMMs of B * N rows).  Off (the default): `img_embed` runs under no_grad and such inputs are refused, as before.  In
        `.eval()`, under no_grad or with a fully frozen image side the switch changes nothing.  The setting is a plain attribute of the
        model: it survives `.to()` and `.train()` / `.eval()`."""
        self.image_tuning = bool(on)
        return self

    def _image_side_trained(self, pooled: bool):
        """(ViT trained, pooled head trained) for an `img_embed` call that builds a graph; (False, False) otherwise."""
        if not (self.image_tuning and self.training and torch.is_grad_enabled()):
            return False, False
        vit = any(p.requires_grad for n, p in self.named_parameters() if n.startswith("visual_encoder."))
        head = pooled and (vit or self.vision_proj.weight.requires_grad or self.vision_proj.bias.requires_grad)
        return vit, head

    def img_embed(self, image, atts=False, return_pool_and_normalized=False):
        """blip_stage1.py:48-65: ViT tokens (B, N, D) fp32 [, normalised 256-d pooled features][, ones mask].  Without a graph, unless
        `set_image_tuning()` is on (see there)."""
        vit_on, head_on = self._image_side_trained(return_pool_and_normalized)
        if not (vit_on or head_on):
            return self._img_embed_frozen(image, atts, return_pool_and_normalized)
        if self.device.type != "cuda":
            raise RuntimeError("BLIP_Retrieval runs on an MI355X only: move the model to 'cuda' (no CPU path)")
        if vit_on:
            from .train_vit import vit_train
            y32 = vit_train(self, image)                                             # tokens with a graph (no DropPath: rate 0 here)
        else:
            with torch.no_grad():
                y32, _ = self.engines()[1].forward(image.to(self.device), want32=True)
        out = (y32,)
        if return_pool_and_normalized:
            from .train_stage1 import pooled_head_train
            out += (pooled_head_train(y32, self.vision_proj.weight, self.vision_proj.bias),)
        if atts:
            out += (torch.ones(y32.shape[:-1], dtype=torch.long, device=y32.device),)
        return out[0] if len(out) == 1 else out

    def img_embed_raw(self, images, transform, atts=False, return_pool_and_normalized=False):
        """`img_embed` from decoded uint8 RGB images of any sizes and a `preprocess.DeviceTransform` (data_utils.py:71-101 on the device).
        Without a graph the transform writes the ViT's patch operand rows directly (no fp32 image tensor, no patchify launch); the results
        are those of `img_embed(transform.batch(images))` bit for bit.  With `set_image_tuning()` building a graph, the normalised
        (B,3,H,W) tensor goes to `img_embed`."""
        if any(self._image_side_trained(return_pool_and_normalized)):
            return self.img_embed(transform.batch(images, dtype=torch.float32), atts, return_pool_and_normalized)
        return self._img_embed_frozen(None, atts, return_pool_and_normalized, patches=transform.batch(images, patches=True, dtype=self.token_dtype))

    @torch.no_grad()
    def _img_embed_frozen(self, image, atts=False, return_pool_and_normalized=False, patches=None):
        _, vit, heads = self.engines()
        if patches is not None:
            y32, _ = vit.forward(None, want32=True, patches=patches)
        else:
            y32, _ = vit.forward(image.to(self.device), want32=True)
        out = (y32,)
        if return_pool_and_normalized:
            out += (ops.l2_normalize(ops.linear_f32(y32[:, 0, :], heads["vw"], heads["vb"])),)
        if atts:
            out += (torch.ones(y32.shape[:-1], dtype=torch.long, device=y32.device),)
        return out[0] if len(out) == 1 else out

    @torch.no_grad()
    def z_t(self, ref_tokens: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> EncoderOutput:
        """Batched z_t: reference-image tokens (Q, N, D), ids/mask (Q, L) with [ENC] set."""
        t = ref_tokens.to(self.device)
        fwd = self._dropout_forward() if self.training else None
        if fwd is not None:
            # model_stage1.train() (stage2_train.py:166): the reference forms z_t with every nn.Dropout of the stage-I BERT active, under
            # no_grad (stage2_train.py:200-203) - train_med.py; .eval() (every validation script) takes the inference engine below
            dt = fwd.eng.dtype
            h32, h16 = fwd.forward(input_ids, attention_mask, t if t.dtype == dt else ops.gather_rows(t, None, dt))
            return EncoderOutput(h32, h16)
        if t.dtype != self.token_dtype:
            t = ops.gather_rows(t, None, self.token_dtype)
        h32, h16 = self.engines()[0].forward(input_ids, attention_mask, t)
        return EncoderOutput(h32, h16)

    def _dropout_forward(self):
        """The train-mode forward of the text encoder (train_med.MedDropoutForward), or None when the med_config probabilities are zero.
        Operands as the training plan has them (train.train_dtype): the model's 16-bit compute type, fp16 for the fp32 modes - the inference
        engine's packed weights are shared when they are of that type, otherwise a 16-bit twin is packed once per engine build."""
        geo = self.bert_geometry
        ph, pa = float(geo.hidden_dropout_prob), float(geo.attention_probs_dropout_prob)
        if ph <= 0.0 and pa <= 0.0:
            return None
        from .train_med import MedDropoutForward
        eng = self.engines()[0]
        cur = getattr(self, "_med_dropout", None)
        if cur is None or cur[0] is not self._engines or (cur[1].p_hidden, cur[1].p_attn) != (ph, pa):
            dt = self.compute_dtype if self.compute_dtype in (torch.float16, torch.bfloat16) else torch.float16
            if not (eng.dtype == dt and eng.xdtype == dt):
                eng = MedEngine(self.state_dict(), geo, dt, self.device, stream_dtype=torch.float32, cross_dtype=dt)
            cur = self._med_dropout = (self._engines, MedDropoutForward(eng, ph, pa))
        return cur[1]

    def img_txt_fusion(self, r_image_embeds, t_image_embeds, text, train=True, return_raw=False):
        """blip_stage1.py:67-92.  train=False: `return_raw` -> z_t object (stage-II input); otherwise the normalised 256-d query feature
        `F.normalize(text_proj(z_t[:, 0]))` used by stage-I retrieval.  train=True: logits = that feature @ t_image_embeds^T / temp (B, Bt),
        t_image_embeds the normalised pooled target features (B, 256).  In .train() mode with grad enabled that is the stage-I training step
        (stage1_train.py:170-172): the logits are differentiable w.r.t. the encoder layers, embeddings, text_proj and temp
        (train_stage1.MedTrainer); in .eval() mode or under no_grad the same head runs on this mode's z_t, without a graph.  Image
        features that require a gradient are refused unless `set_image_tuning()` is on; then their gradients are returned as well."""
        if not train:
            with torch.no_grad():
                ids, mask = encode_text(self.tokenizer, text, self.device)          # blip_stage1.py:72-73
                z = self.z_t(r_image_embeds, ids, mask)
                if return_raw:
                    return z
                heads = self.engines()[2]
                return ops.l2_normalize(ops.linear_f32(z.last_hidden_state[:, 0, :], heads["tw"], heads["tb"]))
        from . import train_ops as T
        from .train_stage1 import _refuse_image_grads, stage1_train
        if not self.image_tuning:
            _refuse_image_grads(r_image_embeds, t_image_embeds)
        ids, mask = encode_text(self.tokenizer, text, self.device)
        if self.training and torch.is_grad_enabled():
            return stage1_train(self, r_image_embeds, t_image_embeds, ids, mask)
        with torch.no_grad():
            z = self.z_t(r_image_embeds, ids, mask)
            heads = self.engines()[2]
            p = ops.linear_f32(z.last_hidden_state[:, 0, :], heads["tw"], heads["tb"])
            return T.contrastive_fwd(p, t_image_embeds.to(self.device).float().contiguous(), heads["temp"])[2]


def blip_stage1(pretrained: str = "", **kwargs) -> BLIP_Retrieval:
    model = BLIP_Retrieval(**kwargs)
    if pretrained:
        if model.tokenizer is None:
            raise RuntimeError("blip_stage1(pretrained=...): real weights need the real WordPiece tokenizer, and no bert-base-uncased "
                               "vocabulary was found - pass tokenizer=blip.init_tokenizer(vocab_file=...)")
        from .checkpoint import load_stage1_checkpoint
        model, msg = load_stage1_checkpoint(model, pretrained)      # blip.py:215-237 semantics
        print("missing keys:")
        print(msg.missing_keys)
        # Real weights: "text32" - the text side on fp32 rows as split8 operands (fp16 + two scaled-fp8 correction products), fp32 text
        # stream, fp32 self-attention, erf GELU; ViT and cross-attention block fp16 (blip_stage2.blip_stage2 has the numbers).
        model.set_precision("text32")
    return model
