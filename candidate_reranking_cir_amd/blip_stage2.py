"""Drop-in `blip_stage2` model surface on the MI355X kernel library.

Mirrors the public surface of the reference's src/blip_stage2.py (factory `blip_stage2(pretrained,
**kwargs)`, class `BLIP_NLVR` with `img_embed`, `img_txt_fusion_val`, `img_txt_fusion`, the
attributes `visual_encoder`, `text_encoder`, `tokenizer`, `cls_head`, and a `state_dict` with the
same 723 keys/shapes) so the reference's validate/test scripts can construct and call it unchanged
(validate_stage2.py:352-362, 118, 254, 268; cirr_test_submission_stage2.py:157, 168; utils.py:51).
Forward arithmetic runs in libcirrank's HIP kernels (`engine.NlvrEngine`, `engine.VitEngine`);
parameters stay fp32 `nn.Parameter`s (what `load_state_dict` fills) and are packed to 16-bit on
first use (`set_compute_dtype`: bf16 or fp16 operands; `set_stream_dtype`: storage of the residual
stream).  Inference only: no autograd graph is built.
"""
from __future__ import annotations

import operator
import os
from typing import Optional, Sequence, Union

import torch
from torch import nn
from torch.autograd.graph import increment_version
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import lib as _lib
from . import ops
from .config import BertGeometry, VitGeometry
from .engine import NlvrEngine, VitEngine
from .param_tree import ParamNode, populate
from .weights import nlvr_param_spec


def default_tokenizer():
    """What the reference's constructors do (blip_stage2.py:38-44, blip_stage1.py:34): the real WordPiece tokenizer with
    [DEC] / [ENC].  Offline there may be no vocabulary; the model then has NO tokenizer and refuses strings loudly
    (`encode_text`) instead of silently hashing words - pass `tokenizer=synthetic.HashTokenizer()` (tests, benchmark)
    or `tokenizer=blip.init_tokenizer(vocab_file=...)` explicitly.  Pre-tokenised ids always work."""
    from .blip import init_tokenizer
    try:
        return init_tokenizer()
    except RuntimeError:
        return None

def load_bert_geometry(med_config) -> BertGeometry:
    """`med_config` is a path to a JSON file with the reference's keys (blip_stage2.py:46-47 reads
    configs/med_config.json: hidden_size, num_attention_heads, num_hidden_layers, intermediate_size, layer_norm_eps,
    vocab_size, max_position_embeddings), a dict, or a BertGeometry.  When the reference's default relative path is
    given but no such file exists in the working directory, the built-in BERT-base/BLIP geometry is used."""
    if isinstance(med_config, BertGeometry):
        return med_config
    if isinstance(med_config, dict):
        return BertGeometry.from_dict(med_config)
    if not os.path.isfile(med_config) and med_config == "configs/med_config.json":
        g = BertGeometry()   # defaults = the reference's med_config.json values
        g.validate()
        return g
    return BertGeometry.from_json_file(med_config)


def encode_text(tokenizer, text, device):
    """`text` is a list of strings (tokenised like blip_stage2.py:113-114) or an already tokenised
    object/dict with `input_ids` and `attention_mask`.  Returns ids with ids[:,0] = [ENC]."""
    if isinstance(text, dict):
        ids, mask = text["input_ids"], text["attention_mask"]
    elif hasattr(text, "input_ids"):
        ids, mask = text.input_ids, text.attention_mask
    else:
        if tokenizer is None:
            raise RuntimeError("no tokenizer: the bert-base-uncased vocabulary is not available offline - assign model.tokenizer = "
                               "blip.init_tokenizer(vocab_file=...) (or synthetic.HashTokenizer() for synthetic data), or pass token ids")
        enc = tokenizer(text, padding="longest", return_tensors="pt")
        ids, mask = enc.input_ids, enc.attention_mask
    ids = ids.to(device=device, dtype=torch.int64).clone()
    ids[:, 0] = getattr(tokenizer, "enc_token_id", 30523)
    return ids, mask.to(device=device, dtype=torch.int64)


_VERSION = operator.attrgetter("_version")


def _on_optimizer_step(optimizer, args, kwargs):
    """Post-hook of every torch.optim step (foreach / fused kernels and GradScaler.step included): whatever the optimizer's kernels
    did to the parameters' version counters, the parameters it holds count as written - the packed copies compare those counters."""
    increment_version([p for group in optimizer.param_groups for p in group["params"]])
    _lib.PARAM_EPOCH[0] += 1


register_optimizer_step_post_hook(_on_optimizer_step)

_LOAD_EPOCH = [0]      # moved by every load_state_dict of a model or of one of its submodules (post-hook; module-level so that models pickle)


def _on_load_state_dict(module, incompatible_keys):
    """load_state_dict(assign=True) replaces Parameter objects, whose version counters start afresh: keys and parameter lists move."""
    _LOAD_EPOCH[0] += 1


class _EngineHost(nn.Module):
    """Shared plumbing: lazily packed engines, repacked when the parameters they were packed from are written (`weights_key`)."""

    _PARTS = {"text": ("text_encoder.", "cls_head."), "vit": ("visual_encoder.",),
              "stage1_train": ("text_encoder.", "text_proj.", "temp")}          # what the stage-I trainer's slab holds (train_stage1.py)

    def __init__(self):
        super().__init__()
        self._engines = None
        self._weights_epoch = 0                # moved by `invalidate_packed_weights`
        self._param_lists = None               # part -> the parameters `weights_key` reads (cached; rebuilt after a load_state_dict)
        self._lists_epoch = -1
        self._loads_hooked = False
        self.compute_dtype = torch.float16     # operand type of the text side (self-attention, FFN, cls_head); fp16 holds the
                                               # reference's rank order where bf16 does not - `set_precision`
        self.image_dtype = None                # operand type of the ViT and the cross-attention block (None: = compute_dtype)
        self._stream_dtype = None              # None = automatic (see `stream_dtype`)
        self._vit_stream_dtype = None          # the ViT's own residual-stream storage (None = automatic)
        self.text_split3 = 8                   # text32 mode, arithmetic of the text side's fp32 Linears: 8 = "split8" rows - one fp16 MFMA product + two
                                               # block-scaled fp8 correction products, operands written by the producing kernels (round 6;
                                               # cir_gemm_split8); 3 / True = three fp16 products on [hi | lo | hi] rows (round 5; cir_split16);
                                               # 0 / False = the f32-input MFMA
        self.text_stream32_from = None         # two-branch encoder: layers >= this index keep their residual stream in fp32 (None: `stream_dtype`
                                               # everywhere) - `set_text_stream32_from`
        self.long_caption_fold = False         # two-branch encoder: captions of 33-64 tokens take the long-caption query-side fold instead of the
                                               # projected K|V path (`set_long_caption_fold`; off by default)
        self.long_caption_fold_wide = False    # two-branch encoder: captions of 33-64 tokens against 225-608 image tokens (384 px) take the key-split
                                               # query-side fold instead of the projected K|V path (`set_long_caption_fold_wide`; off by default)
        self.short_caption_fold = False        # two-branch encoder: captions of at most 16 tokens take the one-block query-side fold instead of the
                                               # 32-token kernels (`set_short_caption_fold`; off by default)
        self.vit_grad_ckpt, self.vit_ckpt_layer = False, 0      # what the factory was given (blip.py:194-209 hands them to the ViT)
        self.vit_ckpt_blocks = 0               # trailing ViT blocks whose activations the training backward recomputes (`set_vit_checkpointing`)
        self.graph_candidates = 0              # `score` calls with at most this many candidate rows replay a captured HIP graph per
                                               # shape (0 = off; `enable_graphs`): single-query serving is launch-bound from the host

    def _keep_vit_checkpointing(self, vit_grad_ckpt, vit_ckpt_layer):
        """The factory's two arguments (vit.py:158: block i is wrapped iff use_grad_checkpointing and i >= depth - ckpt_layer)."""
        self.vit_grad_ckpt, self.vit_ckpt_layer = bool(vit_grad_ckpt), int(vit_ckpt_layer)
        return self.set_vit_checkpointing(self.vit_ckpt_layer if self.vit_grad_ckpt else 0)

    def set_vit_checkpointing(self, n: int):
        """Gradient checkpointing of the image encoder's training pass (`vit_grad_ckpt` / `vit_ckpt_layer` of the factories; fairscale's
        checkpoint_wrapper around attn and mlp of the last `ckpt_layer` blocks in the reference, vit.py:103-105, :158): the last
        min(n, depth) blocks keep only their two fp32 stream rows for the backward (6144 of 30768 bytes per token and block at width 768),
        which rebuilds their activations with the forward's own launches before their adjoints (`train_vit.VitTrainer`).  Tokens and, in the
        deterministic mode, gradients are bit-identical to the unchecked pass.  0 (the default) checkpoints nothing.  Read at every
        train-mode `img_embed` call; a call already made keeps the form it saved.  `train.vit_saved_bytes` gives the bytes per call."""
        n = int(n)
        if n < 0:
            raise ValueError(f"set_vit_checkpointing: {n} blocks")
        self.vit_ckpt_blocks = min(n, self.vit_geometry.depth)
        return self

    @property
    def stream_dtype(self) -> torch.dtype:
        """Storage of the text-side residual stream: fp16 unless `set_stream_dtype` says otherwise (the sums are formed in fp32).
        Measured against the reference's fp32 outputs (profiles/r4_precision_modes.json): with fp16
        operands, fp32 storage of the text-side stream moves Kendall's tau on the outlier fixture 0.91 -> 0.94 and the exact
        positions on rank224 0.93 -> 0.96 for 3.6 % of the step; the ViT's stream is rank-neutral in fp16."""
        if self.compute_dtype == torch.float32:
            return torch.float32
        return self._stream_dtype if self._stream_dtype is not None else torch.float16

    def set_stream_dtype(self, dtype: Optional[torch.dtype], vit: Optional[torch.dtype] = "same"):
        """Storage of the residual stream: fp16, fp32 or None (default: fp16).  `vit` gives the ViT its own choice (its stream
        is 6x the text side's rows: the bytes are there, the rank sensitivity is on the text side - DESIGN.md section 2);
        `set_stream_dtype(torch.float32, vit=torch.float16)` is the strictest mode that is still fast."""
        for d in (dtype,) + (() if vit == "same" else (vit,)):
            if d not in (None, torch.float16, torch.float32):
                raise ValueError("residual-stream dtype must be torch.float16, torch.float32 or None (automatic)")
        self._stream_dtype = dtype
        self._vit_stream_dtype = dtype if vit == "same" else vit
        self._engines = None
        return self

    @property
    def vit_stream_dtype(self) -> torch.dtype:
        if self.token_dtype == torch.float32:
            return torch.float32
        return self._vit_stream_dtype if self._vit_stream_dtype is not None else torch.float16

    def set_compute_dtype(self, dtype: torch.dtype, image_dtype: Optional[torch.dtype] = None):
        """Operand type of every MFMA product (bf16 or fp16; fp32 accumulate either way).  `image_dtype` gives the ViT and the
        image-facing cross-attention block of the text encoders their own operand type (engine.py, "MIXED")."""
        for d in (dtype, image_dtype):
            if d not in (None, torch.bfloat16, torch.float16, torch.float32) or dtype is None:
                raise ValueError("compute dtype must be torch.bfloat16, torch.float16 (fp32 accumulate either way) or torch.float32 (exact mode)")
        if image_dtype == torch.float32 and dtype != torch.float32:
            raise ValueError("an fp32 ViT under a 16-bit text side is not a mode: set_precision('exact') or ('text32')")
        self.compute_dtype = dtype
        self.image_dtype = None if image_dtype == dtype else image_dtype
        self._engines = None
        return self

    def set_text_stream32_from(self, layer: Optional[int]):
        """fp32 storage of the two-branch encoder's residual stream from fusion layer `layer` on (the layers nearest the logits), the
        layers below it in `stream_dtype`; None = `stream_dtype` everywhere.  A point between the all-fp16 default and the split mode."""
        self.text_stream32_from = None if layer is None else int(layer)
        self._engines = None
        return self

    def enable_graphs(self, max_candidates: int = 512):
        """Serve small `score` calls (<= max_candidates candidate rows: img_txt_fusion_val, small query batches) from captured HIP
        graphs - one hipGraphLaunch instead of ~330 launches issued from Python.  Bit-identical results; 0 switches it off."""
        self.graph_candidates = int(max_candidates)
        return self

    PRECISIONS = ("bf16", "f16", "mixed", "text32", "text32x3", "exact")

    def set_precision(self, mode: str):
        """"bf16" / "f16": one operand type everywhere.  "mixed": bf16 operands for the ViT and the cross-attention block
        (cross Q / K|V projections, cross-attention, merge projection: 77 % of the path's flops), fp16 operands for the
        text-side self-attention, FFN and cls_head - where a bf16 run loses the reference's rank order
        (profiles/r4_precision_attribution_*.json)."""
        if mode not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}")
        if mode == "exact":
            # Round 5: the reference's own precision (validate_stage2.py:140-141, 288-289: model.float()) - fp32 weights, activations,
            # attention operands and residual streams, every product on the f32-input MFMA (IEEE fmaf chains), erf GELU as written,
            # the merge layers and the last layer's K / V projections un-folded.  The mode that holds the reference's rank order
            # (north_star: "identical top-K rank order"), and the on-device referee for sizes the CPU reference cannot reach; ~1/9 of
            # the default mode's throughput.
            self.set_compute_dtype(torch.float32)
            return self.set_stream_dtype(torch.float32)
        if self.compute_dtype == torch.float32:        # leaving exact / text32: back to the automatic stream storage
            self.set_stream_dtype(None)
        if mode in ("text32", "text32x3"):
            # Rounds 5-6 (tools/text_fp32_probe.py): the TEXT side alone at fp32-like precision - fp32 rows and weights as multi-term 16 / 8-bit
            # operands, fp32 stream, fp32 self-attention, erf GELU for self-attention / FFN / cls_head of both text encoders - over the fp16
            # ViT and fp16 cross-attention block (folds kept).  The rank error of a 16-bit run enters through the text side: this mode holds
            # 0.97 / 0.95 / 0.98 of the K = 100 / 200 / 50 positions of the reference's order where the all-fp16 default holds 0.90 / 0.81 / 0.95.
            # "text32" (round 6): "split8" rows - one fp16 MFMA product + two block-scaled fp8 correction products per Linear, operand rows
            # written by the producing kernels; "text32x3" (round 5): three fp16 products on [hi | lo | hi] rows (the last ~2 % of the order
            # on outlier-channel weights, at 0.85 x the throughput).  `text_split3` holds the choice (8 / 3; 0 = the f32-input MFMA).
            self.text_split3 = 8 if mode == "text32" else 3
            self.set_compute_dtype(torch.float32, torch.float16)
            return self.set_stream_dtype(None, vit=None)
        if mode == "mixed":
            return self.set_compute_dtype(torch.float16, torch.bfloat16)
        return self.set_compute_dtype(torch.bfloat16 if mode == "bf16" else torch.float16)

    @property
    def precision(self) -> str:
        if self.image_dtype is not None:
            if (self.compute_dtype, self.image_dtype) == (torch.float32, torch.float16):
                return "text32"            # (either arithmetic: `text_arithmetic` tells them apart)
            return "mixed" if (self.compute_dtype, self.image_dtype) == (torch.float16, torch.bfloat16) else \
                f"{str(self.compute_dtype)[6:]}+{str(self.image_dtype)[6:]}"
        return {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "exact"}[self.compute_dtype]

    @property
    def text_arithmetic(self) -> str:
        """how the text side's Linears multiply in this mode (reporting)"""
        if self.precision != "text32":
            return {"exact": "f32-input MFMA"}.get(self.precision, "one 16-bit MFMA product")
        return {8: "split8: fp16 MFMA + 2 block-scaled fp8 correction products", 3: "three fp16 MFMA products", True: "three fp16 MFMA products"}.get(
            self.text_split3, "f32-input MFMA")

    @property
    def token_dtype(self) -> torch.dtype:
        """16-bit type of image tokens on this model's path (ViT output = cross-attention operand)."""
        return self.image_dtype or self.compute_dtype

    def _apply(self, fn, *a, **k):
        self._engines = None
        self.invalidate_packed_weights()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._engines = None
        return super().load_state_dict(*a, **k)

    # ---------------------------------------------------------------------------------------------- packed-weight coherence
    def invalidate_packed_weights(self):
        """Every packed copy of the parameters - inference engines with their captured graphs and K/V banks, the trainers' 16-bit
        slabs - is rebuilt on its next use.  Needed after writes no version counter sees: `p.data.copy_(...)`, `p.data = ...` of a
        single submodule, a raw kernel on the parameters' memory.  In-place torch ops on the parameters, torch.optim steps,
        `train.AdamW.step` and `load_state_dict` of the model or any submodule are followed without it."""
        self._weights_epoch += 1
        self._param_lists = None
        for twin in tuple(self.__dict__.get("_twins") or ()):
            twin.invalidate_packed_weights()
        return self

    _TWIN_FRESH = ("_trainer", "_vit_trainer", "_med_dropout", "_packed_key", "_packed_keys", "_twins", "_pending_counters")    # per-model caches a twin starts without

    def referee(self):
        """A model of the same class and geometry over the SAME `Parameter` objects, in the "exact" precision with packed engines of its
        own: the referee of rank refinement (`validate_stage2.refine_predictions`).  No second fp32 copy of the weights exists, and the
        twin's `weights_key` reads the same version counters, so every write the primary's packed copies follow - in-place torch ops,
        optimizer steps, `train.AdamW.step`, a copying `load_state_dict` - repacks the twin as well; `invalidate_packed_weights()` and
        `.to()` / `.float()` on the primary reach its live twins (held weakly).  The primary's precision, engines, graphs and switches
        are untouched; the twin's switches are its own.  The module tree is the twin's own, so `load_state_dict(assign=True)` on either
        side - which replaces Parameter objects - BREAKS the sharing: build a new referee afterwards.  Every call returns a new twin."""
        import weakref

        def clone(mod):
            new = mod.__class__.__new__(mod.__class__)
            for k, val in mod.__dict__.items():                      # containers (parameters, buffers, hooks) are the twin's own; what they hold is shared
                new.__dict__[k] = type(val)(val) if isinstance(val, dict) else val
            new.__dict__["_modules"] = type(mod._modules)((name, clone(child)) for name, child in mod._modules.items())
            return new

        twin = clone(self)
        for k in self._TWIN_FRESH:
            twin.__dict__.pop(k, None)
        twin._engines, twin._param_lists, twin._lists_epoch, twin.graph_candidates = None, None, -1, 0
        twin.set_precision("exact")
        if self.__dict__.get("_twins") is None:
            self.__dict__["_twins"] = weakref.WeakSet()
        self._twins.add(twin)
        return twin

    def _part_params(self, part: str):
        if not self._loads_hooked:                 # load_state_dict(assign=True) of a submodule replaces Parameter objects: new list
            for mod in self.modules():
                mod.register_load_state_dict_post_hook(_on_load_state_dict)
            self._loads_hooked = True
        if self._param_lists is None or self._lists_epoch != _LOAD_EPOCH[0]:
            self._param_lists, self._lists_epoch = {}, _LOAD_EPOCH[0]
        ps = self._param_lists.get(part)
        if ps is None:
            pre = self._PARTS.get(part)
            ps = self._param_lists[part] = [p for n, p in self.named_parameters() if pre is None or n.startswith(pre)]
        return ps

    def weights_key(self, part: str = "all") -> tuple:
        """Staleness key of the parameters of `part` ("text": text_encoder + cls_head, "vit": visual_encoder, "all"): what a packed copy
        records when it is written and compares before it is used.  (epoch, sum of the parameters' version counters): every in-place
        torch op moves a counter, torch.optim steps and train.AdamW.step move them explicitly (their kernels write through pointers)."""
        ps = self._part_params(part)
        return (self._weights_epoch, _LOAD_EPOCH[0], sum(map(_VERSION, ps)))

    @property
    def device(self):
        return next(self.parameters()).device


class BLIP_NLVR(_EngineHost):
    """Stage-II re-ranker: ViT-B/16 + two-branch BERT + cls_head (reference: blip_stage2.py:19-136)."""

    def __init__(self, med_config: Union[str, dict, BertGeometry] = "configs/med_config.json", image_size: int = 480,
                 vit: str = "base", vit_grad_ckpt: bool = False, vit_ckpt_layer: int = 0, *,
                 vit_geometry: Optional[VitGeometry] = None, tokenizer=None, fold_merge: bool = True):
        super().__init__()
        self.vit_geometry = vit_geometry or VitGeometry.named(vit, image_size)
        self._keep_vit_checkpointing(vit_grad_ckpt, vit_ckpt_layer)         # blip_stage2.py:37
        self.bert_geometry = load_bert_geometry(med_config)
        self.bert_geometry.encoder_width = self.vit_geometry.width          # blip_stage2.py:47
        self.fold_merge = fold_merge
        self.tokenizer = tokenizer if tokenizer is not None else default_tokenizer()
        populate(self, nlvr_param_spec(self.bert_geometry, self.vit_geometry))
        self.text_encoder.config = self.bert_geometry                        # callers read .config.hidden_size

    # ------------------------------------------------------------------------------------------
    def _text_engine(self, sd) -> NlvrEngine:
        e = NlvrEngine(sd, self.bert_geometry, self.compute_dtype, self.device, fold_merge=self.fold_merge and self.compute_dtype != torch.float32,
                       stream_dtype=self.stream_dtype, cross_dtype=self.token_dtype, split3=self.text_split3 if self.precision == "text32" else 0)
        e.stream32_from = self.text_stream32_from
        e.fold_long = self.long_caption_fold
        e.fold_short = self.short_caption_fold
        e.fold_long_wide = self.long_caption_fold_wide
        return e

    def set_long_caption_fold(self, on: bool = True):
        """Captions of 33-64 tokens (the reference tokenises with padding='longest' and no 32-token cut, blip_stage2.py:113; FashionIQ joins two
        captions) against at most 224 image tokens: run the cross-attention of fusion layers 0-10 through the long-caption query-side fold
        (cir_cross_attention_folded_long) instead of the projected K|V path.  Off by default; `NlvrEngine.fold_fallbacks` stays at 0 for such
        batches when it is on.  The setting lives on the model and is re-applied to every engine packed from it."""
        self.long_caption_fold = bool(on)
        if self._engines is not None:
            self._engines[1].fold_long = self.long_caption_fold
        return self

    def set_long_caption_fold_wide(self, on: bool = True):
        """Captions of 33-64 tokens against 225-608 image tokens (the reference's 384 px: 577 tokens, validate_stage2.py:327; captions are never
        cut to 32 tokens, blip_stage2.py:113): run the cross-attention of fusion layers 0-10 through cir_cross_attention_folded_long_wide - the
        keys of a head split over two waves - instead of the projected K|V path.  A switch of its own: `set_long_caption_fold` covers at most
        224 image tokens and leaves this geometry projected.  Off by default (LABNOTES.md section 21); `NlvrEngine.fold_fallbacks` stays at 0
        for such batches when it is on.  The setting lives on the model and is re-applied to every engine packed from it."""
        self.long_caption_fold_wide = bool(on)
        if self._engines is not None:
            self._engines[1].fold_long_wide = self.long_caption_fold_wide
        return self

    def set_short_caption_fold(self, on: bool = True):
        """Captions of at most 16 tokens (the reference never pads a query: batch 1, padding='longest', blip_stage2.py:113; CIRR and FashionIQ
        modification sentences are short) against up to 608 image tokens: run the cross-attention of fusion layers 0-10 through
        cir_cross_attention_folded_short - one 16-token block per head - instead of the 32-token kernels, which compute a second block on zero
        queries.  Off by default: it measures faster at 225-608 image tokens (384 px) and slower at up to 224 (LABNOTES.md section 18).  The setting lives on the model and is re-applied to every
        engine packed from it."""
        self.short_caption_fold = bool(on)
        if self._engines is not None:
            self._engines[1].fold_short = self.short_caption_fold
        return self

    def _vit_engine(self, sd) -> VitEngine:
        return VitEngine(sd, self.vit_geometry, self.token_dtype, self.device, stream_dtype=self.vit_stream_dtype)

    def engines(self, text: bool = True, vit: bool = True):
        """(VitEngine, NlvrEngine) packed from the parameters.  A part whose `weights_key` moved since it was packed is repacked before it
        is returned - the text side when `text`, the ViT when `vit` (callers that use one engine only skip the other's check)."""
        if self._engines is None:
            if self.device.type != "cuda":
                raise RuntimeError("BLIP_NLVR runs on an MI355X only: move the model to 'cuda' (no CPU path)")
            self._packed_keys = [self.weights_key("vit"), self.weights_key("text")]
            sd = self.state_dict()
            self._engines = (self._vit_engine(sd), self._text_engine(sd))
            return self._engines
        if vit:
            k = self.weights_key("vit")
            if k != self._packed_keys[0]:
                self._packed_keys[0] = k
                self._engines = (self._vit_engine(self.state_dict()), self._engines[1])
        if text:
            k = self.weights_key("text")
            if k != self._packed_keys[1]:
                self._packed_keys[1] = k
                self._engines = (self._engines[0], self._text_engine(self.state_dict()))
        return self._engines

    def img_embed(self, image, train=True, atts=False):
        """(B,3,H,W) -> (B, N, D) fp32 image tokens [+ ones (B, N) int64], blip_stage2.py:57-63.  In `.train()` mode with autograd enabled and
        a trainable ViT (`--blip-img-tune`, stage2_train.py:87-92, 191-199) the tokens carry a graph: `train_vit.vit_train`, whose reverse
        pass fills `.grad` of every visual_encoder parameter; in `.train()` mode without a graph (frozen ViT / torch.no_grad(),
        stage2_train.py:183-190) the encoder still draws DropPath like the reference's (`VitEngine.forward_drop_path`); in eval mode the
        inference engine."""
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for n, p in self.named_parameters() if n.startswith("visual_encoder.")):
            if self.device.type != "cuda":
                raise RuntimeError("BLIP_NLVR runs on an MI355X only: move the model to 'cuda' (no CPU path)")
            from .train_vit import vit_train
            y32 = vit_train(self, image)
        elif self.training and float(getattr(self.vit_geometry, "drop_path_rate", 0.0)) > 0.0 and self.vit_geometry.depth > 1 and self.token_dtype != torch.float32:
            # .train() mode without a graph (frozen ViT, or under torch.no_grad(): stage2_train.py:183-190): the reference's DropPath modules
            # are in training mode there and drop each sample's residual branches (vit.py:98-109, rate linspace(0, 0.1, depth)[i]) - so do we
            # (round 6; rounds 3-5 ran the inference engine here).  The draws come from torch's global generator, like timm's.
            with torch.no_grad():
                geo = self.vit_geometry
                rates = torch.linspace(0.0, float(geo.drop_path_rate), geo.depth)                       # vit.py:153
                keep = 1.0 - rates
                draw = torch.rand((geo.depth, 2, image.shape[0]))
                scales = (draw < keep[:, None, None]).float() / keep[:, None, None]                     # timm drop_path: floor(keep + U) / keep
                y32 = self.engines(text=False)[0].forward_drop_path(image.to(self.device), scales.to(self.device))
        else:
            with torch.no_grad():
                y32, _ = self.engines(text=False)[0].forward(image.to(self.device), want32=True)
        if atts:
            return y32, torch.ones(y32.shape[:-1], dtype=torch.long, device=y32.device)
        return y32

    @torch.no_grad()
    def img_embed16(self, image) -> torch.Tensor:
        """Same tokens in the 16-bit `token_dtype` (what the cross-attention K|V GEMMs consume)."""
        return self.engines(text=False)[0].forward(image.to(self.device), want32=False)[1]

    def img_embed_raw(self, images, transform, train=True, atts=False):
        """`img_embed` from decoded uint8 RGB images of any sizes (arrays / tensors / PIL images) and a `preprocess.DeviceTransform`
        (the reference's `preprocess`, data_utils.py:71-101, on the device).  Eval mode: the transform writes the ViT's patch operand
        rows directly - no fp32 image tensor, no patchify launch - and the tokens are those of `img_embed(transform.batch(images))` bit
        for bit.  In `.train()` mode (a ViT with a graph, or DropPath draws) the normalised (B,3,H,W) tensor goes to `img_embed`."""
        if self.training:
            return self.img_embed(transform.batch(images, dtype=torch.float32), train=train, atts=atts)
        with torch.no_grad():
            rows = transform.batch(images, patches=True, dtype=self.token_dtype)
            y32, _ = self.engines(text=False)[0].forward(None, want32=True, patches=rows)
        if atts:
            return y32, torch.ones(y32.shape[:-1], dtype=torch.long, device=y32.device)
        return y32

    def _cand16(self, t_image_embeds: torch.Tensor) -> torch.Tensor:
        t = t_image_embeds.to(self.device)
        if t.dtype == self.token_dtype:
            return t
        return ops.gather_rows(t, None, self.token_dtype)

    @torch.no_grad()
    def score(self, z_t: torch.Tensor, input_ids: torch.Tensor, attention_mask: torch.Tensor, cand: Optional[torch.Tensor],
              qidx: torch.Tensor, taps: Optional[list] = None, kv_bank: Optional[list] = None,
              cand_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Batched scoring: z_t (Q,L,D), ids/mask (Q,L) with [ENC] already set, cand (T,N,D),
        qidx (T,) -> (T,) fp32 logits (column 0 of cls_head).  `kv_bank` + `cand_rows` score candidates
        straight out of a per-image cross-attention K/V bank (`build_kv_bank`)."""
        eng = self.engines(vit=False)[1]
        if self.graph_candidates and kv_bank is None and taps is None and cand.shape[0] <= self.graph_candidates:
            # small problems are bound by launch issue from the host: one captured HIP graph per shape (engine.ScoreGraph)
            return eng.forward_graphed(input_ids.to(self.device), attention_mask.to(self.device), z_t.to(self.device), self._cand16(cand),
                                       qidx.to(self.device))[:, 0]
        out = eng.forward(input_ids, attention_mask, z_t.to(self.device),
                          self._cand16(cand) if kv_bank is None else None, qidx.to(self.device), taps=taps,
                          kv_bank=kv_bank, cand_rows=None if cand_rows is None else cand_rows.to(self.device))
        return out[:, 0]

    @torch.no_grad()
    def build_kv_bank(self, bank: torch.Tensor) -> list:
        """Per-image, per-layer cross-attention K|V of an index-feature bank (n_index, N, D)."""
        return self.engines(vit=False)[1].build_kv_bank(self._cand16(bank))

    @torch.no_grad()
    def img_txt_fusion_val(self, r_image_embeds, t_image_embeds, text):
        """One query, K candidates -> (K,) logits (blip_stage2.py:101-136)."""
        z = r_image_embeds.last_hidden_state if hasattr(r_image_embeds, "last_hidden_state") else r_image_embeds
        assert z.shape[0] == 1                                               # blip_stage2.py:108
        ids, mask = encode_text(self.tokenizer, text, self.device)
        k = t_image_embeds.shape[0]
        qidx = torch.zeros((k,), dtype=torch.int64, device=self.device)
        return self.score(z, ids, mask, t_image_embeds, qidx)

    def img_txt_fusion(self, r_image_embeds, t_image_embeds, text, train=True):
        """B queries x B candidates -> (B, B) logits (blip_stage2.py:65-99): row i scores caption i / z_t i against all B
        candidates; ragged captions are padded to the longest (real attention masks inside the batch).

        As in the reference the `train` argument itself is unused - the mode is the module's.  In `.eval()` this is the
        inference engine (no graph; pinned by tests/golden/bxb224.npz).  In `.train()` mode it is the training step's forward
        (stage2_train.py:210-212) on `train.fusion_train`: dropout with the config's probabilities, fp32 residual stream, and
        a result that `loss.backward()` differentiates w.r.t. every `text_encoder.*` / `cls_head.*` parameter (pinned by
        tests/golden/train768.npz).  The image tokens and z_t are inputs there, as with the reference's frozen ViT."""
        z = r_image_embeds.last_hidden_state if hasattr(r_image_embeds, "last_hidden_state") else r_image_embeds
        ids, mask = encode_text(self.tokenizer, text, self.device)
        if self.training and torch.is_grad_enabled():
            from .train import fusion_train
            g = self.bert_geometry
            return fusion_train(self, z, t_image_embeds, ids, mask, g.hidden_dropout_prob, g.attention_probs_dropout_prob)
        with torch.no_grad():
            b = z.shape[0]
            cand = self._cand16(t_image_embeds)
            qidx = torch.arange(b, device=self.device).repeat_interleave(b)
            rows = torch.arange(b, device=self.device).repeat(b)
            logits = self.score(z, ids, mask, ops.gather_rows(cand, rows), qidx)
            return logits.view(b, b)

    # ---- what a score rests on (explain.py; the reference's save_attention / get_attention_map / get_attn_gradients, nlvr_encoder.py:121-134)
    def cross_attention_maps(self, r_image_embeds, t_image_embeds, text, layers, grads=True):
        """`explain.cross_attention_maps`: B queries x Bt candidates -> CrossAttentionMaps(logits (B, Bt), probs / grads {layer: (2, B, Bt, H, L, N)})."""
        from .explain import cross_attention_maps
        return cross_attention_maps(self, r_image_embeds, t_image_embeds, text, layers, grads)

    def gradcam(self, r_image_embeds, t_image_embeds, text, layer):
        """`explain.gradcam`: (2, B, Bt, L, N) fp32, the head mean of probs * max(grads, 0) at fusion layer `layer`."""
        from .explain import gradcam
        return gradcam(self, r_image_embeds, t_image_embeds, text, layer)

    @staticmethod
    def patch_grid(x):
        """`explain.patch_grid`: (..., N) -> (..., g, g) without the CLS key."""
        from .explain import patch_grid
        return patch_grid(x)


def blip_stage2(pretrained: str = "", **kwargs) -> BLIP_NLVR:
    """Factory with the reference's signature (blip_stage2.py:139-145).  `pretrained` names a local BLIP base
    checkpoint ({'model': ...}: position embedding resized, single-branch BERT weights copied to both branches, as
    blip_stage2.py:148-190 does), or a file holding {'BLIP_NLVR': state_dict} (utils.py:145-150) / a plain state dict."""
    model = BLIP_NLVR(**kwargs)
    if pretrained:
        if model.tokenizer is None:
            raise RuntimeError("blip_stage2(pretrained=...): real weights need the real WordPiece tokenizer, and no bert-base-uncased "
                               "vocabulary was found - pass tokenizer=blip.init_tokenizer(vocab_file=...)")
        from .checkpoint import load_stage2_checkpoint
        model, msg = load_stage2_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
        # Real weights: "text32" - the text side on fp32 rows as split8 operands (fp16 + two scaled-fp8 correction products, ~16 bits), fp32
        # text stream, fp32 self-attention, erf GELU; ViT and cross-attention block fp16.  Pretrained checkpoints carry outlier channels: on
        # the fixture that mimics them the all-fp16 path holds tau 0.68 of the reference's order, this mode 0.985 (0.97 / 0.95 / 0.98 of the
        # K = 100 / 200 / 50 positions exactly on well-conditioned weights) at 0.8 x the default's throughput.
        # `set_precision("text32x3")` is round 5's three-product form (tau 0.986, 0.85 x this mode's speed); random-init models and the
        # benchmark's headline keep the all-fp16 default; `set_precision("f16")` returns to it.
        model.set_precision("text32")
    return model
