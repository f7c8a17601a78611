"""What the hand-written training passes share (train.py: the stage-II two-branch encoder, train_stage1.py: the stage-I MED encoder,
train_vit.py: ViT fine-tuning; train_med.py: the dropout draw): the flat parameter slab with its 16-bit copy and transposed twin (`_Slab`),
the layer views over it (`_Lin`, `_Lin2`, `_LN`), the slab order (`slab_order`), the head views of the attention kernels (`head_view`), the
fp16 loss scale (`loss_scale`), the per-forward dropout seed (`draw_seed`), the random state a checkpoint carries (`training_state` /
`load_training_state`), the installation of flat gradient slices into `.grad` (`_install_grads`), and `Trainer`: the per-step packing, the end of a backward and the one-slot guard of the autograd nodes.  A pass module
keeps its group table, `_trained`, `_build_layers`, `forward`, `backward` and its entry function.
"""
from __future__ import annotations

import math
import weakref
from typing import Callable, Dict, List, Optional, Sequence

import torch

from . import ops, train_ops as T


def _cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return T.eltwise(x.contiguous(), T.MODE_SCALE, out_dtype=dtype, p_drop=1.0)


def _row_split(rows: int, n: int, k: int) -> int:
    """Number of row chunks of a weight-gradient product dW (n, k) over `rows` rows: enough 128 x 128 tiles x chunks for two
    waves of workgroups on 256 CUs (measured, tools/bmm_bench.py: 16 chunks for a 768 x 768 weight, 8 for the 3072-wide ones;
    32 is slower again), as a divisor of `rows` that leaves >= 128 rows per chunk."""
    tiles = ((n + 127) // 128) * ((k + 127) // 128)
    want = min(16, max(8, 576 // tiles))
    best = 1
    for nb in range(2, want + 1):
        if rows % nb == 0 and rows // nb >= 128:
            best = nb
    return best


def _gemm_ok(m: int, n: int, k: int) -> bool:
    return k % 64 == 0 and n % 16 == 0


_SLABS: Dict[int, "weakref.ref"] = {}     # flat32 base pointer -> the slab that owns it (AdamW.step finds the 16-bit copy to write along)


class _Slab:
    """The trained parameters as ONE flat fp32 buffer (each nn.Parameter's `.data` re-pointed to its slice: optimizers update the
    buffer in place), their 16-bit operand copies as one flat buffer refreshed by one cast when the parameters were written, and their
    gradients as one flat fp32 buffer zeroed once per step - three launches where per-tensor copies took ~900.  Slices start at multiples
    of 8 elements (16-byte rows for the 16-bit views).  `key`: the model's staleness key of these parameters (`_EngineHost.weights_key`):
    each Parameter keeps its own version counter after `p.data = view`, so the flat buffer's own counter sees none of their writes."""

    def __init__(self, params: Dict[str, torch.nn.Parameter], names: List[str], dtype: torch.dtype, key: Callable[[], tuple]):
        self.params, self.names, self.dtype, self.key = params, names, dtype, key
        self.off, o = {}, 0
        for n in names:
            self.off[n] = o
            o += (params[n].numel() + 7) // 8 * 8
        self.total = o
        dev = params[names[0]].device
        self.flat32 = torch.zeros((o,), dtype=torch.float32, device=dev)
        for n in names:
            p = params[n]
            v = self._view(self.flat32, n)
            v.copy_(p.data)
            p.data = v
        _SLABS[self.flat32.data_ptr()] = weakref.ref(self)
        self.flat16 = self.flat16t = self.gflat = self.plan = None
        self.checked = None                                                         # (gradient buffer pointer, its "all finite" device flag)
        self._fresh16 = None                                                        # the `key` flat16 was written for
        self.work = None                  # deterministic mode: the workspace of the fixed-order operators for the backward in flight (else None)
        self._workspace = None            # ... kept between steps

    def read_mode(self) -> dict:
        """Read the process-wide deterministic switch (train_ops.set_deterministic) for the backward that starts now.  Returns the keyword
        the pass and the layer views hand to the train_ops operators that sum across workgroups: {} - the default, atomic forms - or
        {"work": the trainer's reusable workspace}, which selects their fixed-order forms."""
        if T.deterministic():
            if self._workspace is None:
                self._workspace = T.Workspace()
            self.work = self._workspace
        else:
            self.work = None
        return self.det_kw()

    def det_kw(self) -> dict:
        return {} if self.work is None else {"work": self.work}

    def _view(self, flat: torch.Tensor, n: str) -> torch.Tensor:
        p = self.params[n]
        return flat[self.off[n]:self.off[n] + p.numel()].view(p.shape)

    def valid(self) -> bool:
        base = self.flat32.data_ptr()
        return all(self.params[n].data_ptr() == base + 4 * self.off[n] for n in self.names)

    def begin_step(self):
        """One cast launch refreshes the persistent 16-bit copy (when the parameters were written since it was), one multi-transpose launch
        the dgrad operands (`plan`, built by the trainer from its dense layers), one fill the fresh gradient buffer."""
        if self.flat16 is None:
            self.flat16 = torch.empty(self.flat32.shape, dtype=self.dtype, device=self.flat32.device)
            self.flat16t = torch.zeros_like(self.flat16)
        key = self.key()
        if self._fresh16 != key:                                                    # (AdamW.step below writes flat16 in its own pass)
            T.eltwise(self.flat32, T.MODE_SCALE, p_drop=1.0, out=self.flat16)
            self._fresh16 = key
        if self.plan is not None:
            self.plan.run(self.flat16, self.flat16t)
        self.gflat = torch.zeros_like(self.flat32)

    def mark_fresh16(self):
        """flat16 holds the 16-bit copy of flat32 AS IT IS NOW (the optimizer wrote both; called once the step has moved the key): the next
        begin_step skips its cast unless the parameters are written first (an in-place torch op, torch.optim, load_state_dict,
        `invalidate_packed_weights`)."""
        self._fresh16 = self.key()

    def w32(self, n): return self._view(self.flat32, n)
    def w16(self, n): return self._view(self.flat16, n)
    def grad(self, n): return self._view(self.gflat, n)

    def span_range(self, names: List[str]):
        """(offset, rows, trailing shape) of the slices of `names` stacked along dim 0 (they must be adjacent in the buffer: `NlvrTrainer._order`
        lays the q / k / v weights - and biases - of one attention out that way, so the three projections are one 2304-wide Linear)."""
        o = self.off[names[0]]
        rows = 0
        for n in names:
            assert self.off[n] == o + rows * (self.params[n].numel() // self.params[n].shape[0]), "group not adjacent in the slab"
            rows += self.params[n].shape[0]
        return o, rows, tuple(self.params[names[0]].shape[1:])

    def span(self, flat: torch.Tensor, names: List[str]) -> torch.Tensor:
        o, rows, tail = self.span_range(names)
        numel = rows
        for t in tail:
            numel *= t
        return flat[o:o + numel].view((rows,) + tail)


class _Lin:
    """One nn.Linear of the reference (weight (N, K), bias (N)) - or several of one input stacked -: views of the slab's persistent 16-bit
    weights, their transposed copy (the dgrad GEMM's operand; refreshed by the slab's one multi-transpose launch per step) and fp32 bias,
    built ONCE; the gradient views follow the slab's per-step gradient buffer lazily."""

    def __init__(self, slab: _Slab, name, group: bool = False):
        names = list(name) if group else [name]                                     # a group: several Linears of one input, stacked
        has_bias = (names[0] + ".bias") in slab.off
        self.slab = slab
        self.ws, self.bs = [n + ".weight" for n in names], ([n + ".bias" for n in names] if has_bias else None)
        off, n, tail = slab.span_range(self.ws)
        k = 1
        for t in tail:                                                              # a conv kernel (N, C, p, p) is the (N, C p p) Linear over patches
            k *= t
        self.n, self.k, self.off_w = n, k, off
        self.w16 = slab.flat16[off:off + n * k].view(n, k)                          # (N, K): forward operand
        self.w16t = slab.flat16t[off:off + n * k].view(k, n)                        # (K, N): dgrad operand
        self.transpose_entry = (off, n, k)
        self.bias = slab.span(slab.flat32, self.bs) if has_bias else None
        self._g = None

    def _grads(self):
        g = self.slab.gflat
        if self._g is not g:
            self._g, self._dw = g, g[self.off_w:self.off_w + self.n * self.k].view(self.n, self.k)
            self._db = self.slab.span(g, self.bs) if self.bs is not None else None

    @property
    def dw(self):
        self._grads()
        return self._dw

    @property
    def db(self):
        self._grads()
        return self._db

    def fwd(self, x16: torch.Tensor, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        m, k = x16.shape
        n = self.w16.shape[0]
        if _gemm_ok(m, n, k):
            return ops.gemm(x16, self.w16, self.bias, residual=residual, out_dtype=out_dtype, out=out)
        assert out is None and residual is None
        y = T.bmm(x16.unsqueeze(0), self.w16.unsqueeze(0), False, True, out_dtype=torch.float32)[0]
        if self.bias is not None:
            y = T.eltwise(y, T.MODE_ADD, self.bias.unsqueeze(0).expand(m, n).contiguous())
        return y if out_dtype == torch.float32 else _cast(y, out_dtype)

    def bwd(self, x16: torch.Tensor, dy: torch.Tensor, need_dx: bool = True) -> Optional[torch.Tensor]:
        """dy fp32 (M, N): accumulates dW, db; returns dx fp32 (M, K)."""
        m, k = x16.shape
        n = self.w16.shape[0]
        dy16 = _cast(dy, x16.dtype)
        det = self.slab.det_kw()
        if self.db is not None:
            T.colsum(dy, self.db, **det)
        # dW (N, K) = dy^T x on cir_bmm (operands read as stored: trans_a), split over row chunks into partial sums so that the
        # 36-tile products of a 768 x 768 weight fill the chip; the partials are summed into dW by the column-sum kernel
        nb = _row_split(m, n, k)
        if nb == 1:
            T.bmm(dy16.unsqueeze(0), x16.unsqueeze(0), True, False, out=self.dw.unsqueeze(0), accumulate=True)
        else:
            part = T.bmm(dy16.view(nb, m // nb, n), x16.view(nb, m // nb, k), True, False, out_dtype=torch.float32)
            T.colsum(part.view(nb, n * k), self.dw.view(-1), **det)
        if not need_dx:
            return None
        if _gemm_ok(m, k, n):                                                       # dx (M, K) = dy (M, N) . (W^T (K, N))^T
            return ops.gemm(dy16, self.w16t, None, out_dtype=torch.float32)
        return T.bmm(dy16.unsqueeze(0), self.w16.unsqueeze(0), False, False, out_dtype=torch.float32)[0]


    def bwd16(self, x16: torch.Tensor, dy16: torch.Tensor, need_dx: bool = True, dx_dtype: torch.dtype = torch.float32,
              residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, bias: bool = False,
              queue: Optional[list] = None) -> Optional[torch.Tensor]:
        """dy16 (M, N) ALREADY the 16-bit operand (any row stride: written by the fused row kernels, the attention adjoint or the dgrad
        product before): accumulates dW - and db when `bias` (otherwise the producer of dy16 summed it) -; returns
        dx = dy . W (+ residual: the fp32 gradient arriving over the skip connection, added in the GEMM epilogue) in `dx_dtype`."""
        m, k = x16.shape
        n = self.w16.shape[0]
        det = self.slab.det_kw()
        if bias and self.db is not None:
            T.colsum16(dy16, self.db, **det)
        # dW (N, K) += dy^T x with both operands read as stored, the rows split over workgroups so that the 36-tile product of a
        # 768 x 768 weight fills the chip; every workgroup adds its partial tile straight into dW (atomics: no partial tensor)
        if n % 128 == 0 and k % 128 == 0:
            # LDS-DMA / transposing-read kernel (train_wgrad.hip).  `queue` (a list): the product is deferred and launched together with
            # the layer's other weight gradients - ~940 output tiles fill the chip without splitting any tile's rows over workgroups
            if queue is not None:
                queue.append((dy16, x16, self.dw))
            elif det:
                T.wgrad(dy16, x16, self.dw, splits=1)                               # one workgroup per tile: plain adds
            else:
                T.wgrad(dy16, x16, self.dw)
        elif det:                                                                   # unsplit: every dW element has one adder
            T.bmm(dy16.unsqueeze(0), x16.unsqueeze(0), True, False, out=self.dw.unsqueeze(0), accumulate=True)
        else:
            nb = _row_split(m, n, k)
            T.bmm(dy16.unflatten(0, (nb, m // nb)), x16.unflatten(0, (nb, m // nb)), True, False, out=self.dw.unsqueeze(0).expand(nb, n, k),
                  accumulate="atomic")
        if not need_dx:
            return None
        return ops.gemm(dy16, self.w16t, None, residual=residual, out_dtype=dx_dtype, out=out)


class _Lin2:
    """The two branches' Linears of one kind (adjacent in the slab, `NlvrTrainer._order`): forward and dgrad of BOTH as one batched GEMM
    (batch 2; measured on the 8192-row shapes of the step: 22 against 35 us for the 768 x 768 products, 60 against 88 us for the stacked
    q|k|v dgrad - a 9.7-GFLOP product is mostly launch, prologue and epilogue).  Weight / bias gradients stay per branch (`.l[b]`)."""

    def __init__(self, l0: _Lin, l1: _Lin):
        slab, n, k = l0.slab, l0.n, l0.k
        assert l1.n == n and l1.k == k and l1.off_w == l0.off_w + n * k, "branch twins not adjacent in the slab"
        self.l = (l0, l1)
        self.w16 = slab.flat16[l0.off_w:l0.off_w + 2 * n * k].view(2, n, k)
        self.w16t = slab.flat16t[l0.off_w:l0.off_w + 2 * n * k].view(2, k, n)
        ob = slab.off[l0.bs[0]]
        assert slab.off[l1.bs[0]] == ob + n
        self.bias = slab.flat32[ob:ob + 2 * n].view(2, n)

    BATCHED = True        # False: the same products as two launches into the same tensors (A/B: tools/train_dbg.py, CIR_TRAIN_PAIRS=0)

    def _gemm(self, a3, w3, bias, residual, out_dtype, out):
        if self.BATCHED:
            return ops.gemm(a3, w3, bias, residual=residual, out_dtype=out_dtype, out=out)
        if out is None:
            out = torch.empty((2, a3.shape[1], w3.shape[1]), dtype=out_dtype, device=a3.device)
        for b in (0, 1):
            ops.gemm(a3[b], w3[b], None if bias is None else bias[b], residual=None if residual is None else residual[b], out_dtype=out_dtype, out=out[b])
        return out

    def fwd(self, x3: torch.Tensor, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x3 (2, M, K) (a stride-0 batch dimension shares one input) -> (2, M, N)."""
        return self._gemm(x3, self.w16, self.bias, residual, out_dtype, out)

    def dgrad(self, dy3: torch.Tensor, dx_dtype: torch.dtype, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dy3 (2, M, N) -> dx (2, M, K) = dy . W (+ residual) per branch."""
        return self._gemm(dy3, self.w16t, None, residual, dx_dtype, out)

    def wgrad(self, x3: torch.Tensor, dy3: torch.Tensor, queue: list, bias: bool = False):
        for b in (0, 1):
            self.l[b].bwd16(x3[b], dy3[b], need_dx=False, bias=bias, queue=queue)


class _LN:
    def __init__(self, slab: _Slab, name: str, eps: float):
        self.eps, self.slab, self.name = eps, slab, name
        self.g, self.b = slab.w32(name + ".weight"), slab.w32(name + ".bias")
        self._g = None

    def _grads(self):
        g = self.slab.gflat
        if self._g is not g:
            self._g, self._dg, self._db = g, self.slab.grad(self.name + ".weight"), self.slab.grad(self.name + ".bias")

    @property
    def dg(self):
        self._grads()
        return self._dg

    @property
    def db(self):
        self._grads()
        return self._db

    def fwd(self, pre: torch.Tensor, dtype: torch.dtype):
        return ops.layernorm(pre, self.g, self.b, self.eps, want32=True, dtype16=dtype, stream_dtype=torch.float32)

    def bwd(self, pre: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
        return T.layernorm_bwd(pre, self.g, dy, self.dg, self.db, self.eps, **self.slab.det_kw())

    def fwd_res(self, t0, t1, res, dtype, alpha=1.0, p_drop=0.0, seed=0, **out):
        """(pre, y32, y16) of LayerNorm(dropout(alpha * (t0 + t1)) + res): one launch (cir_residual_layernorm_train)."""
        return T.residual_layernorm_train(t0, t1, res, self.g, self.b, self.eps, dtype, alpha, p_drop, seed, **out)

    def bwd_res(self, pre, dy, dtype, **kw):
        """(d pre fp32, 16-bit gradient of the dense branch behind the dropout) - cir_layernorm_bwd_fused."""
        return T.layernorm_bwd_fused(pre, self.g, dy, self.dg, self.db, self.eps, dtype, **kw, **self.slab.det_kw())


def train_dtype(model) -> torch.dtype:
    """Operand type of the training step: the model's own when it is 16-bit; fp16 under the inference-only modes with an fp32 text side
    ("text32" - what the factories set for real weights - and "exact"): the reference trains under fp16 autocast (stage2_train.py:210-218)."""
    return model.compute_dtype if model.compute_dtype in (torch.float16, torch.bfloat16) else torch.float16


def _unscale_and_check(gflat: torch.Tensor, grad_scale: float) -> torch.Tensor:
    """gflat /= grad_scale in place; returns a 0-dim bool tensor "all finite" (no host read)."""
    st = torch.zeros((8,), dtype=torch.int32, device=gflat.device)
    T.grads_check(gflat, st, 1.0 / grad_scale)
    return st[0] == 0


def _install_grads(tr, grads: Dict[str, torch.Tensor]):
    """Accumulate a trainer's gradients into `.grad` as autograd's AccumulateGrad would (a first gradient is the trainer's own slice of its
    flat gradient buffer - no copy).  Gradient accumulation over micro-batches (stage2_train.py's grad_accumulation_step): when every .grad
    is still a slice of the flat buffer a previous backward installed, ONE flat add folds it into the new buffer and .grad is re-pointed to
    the new slices - so the optimizer keeps its one-launch flat path (per-tensor adds: ~570 launches, and AdamW falls back to 570 more)."""
    slab = tr.slab
    live = [(n, slab.params[n]) for n in slab.names if n in grads and slab.params[n].requires_grad]
    prev = getattr(tr, "acc_gflat", None)
    if (prev is not None and prev is not slab.gflat and prev.numel() == slab.gflat.numel()
            and all(p.grad is not None and p.grad.data_ptr() == prev.data_ptr() + 4 * slab.off[n] and p.grad.is_contiguous() for n, p in live)):
        slab.gflat = T.eltwise(slab.gflat, T.MODE_ADD, prev)
        slab.checked = None                                   # (the sum is a buffer nobody has tested: AdamW.step tests it)
        for n, p in live:
            p.grad = slab.grad(n)
    else:
        for n, p in live:
            gq = grads[n]
            p.grad = gq if p.grad is None else T.eltwise(p.grad.contiguous(), T.MODE_ADD, gq.contiguous())
    tr.acc_gflat = slab.gflat


def slab_order(names: List[str], groups: Sequence[Sequence[str]]) -> List[str]:
    """Slab order of the parameters `names`.  `groups`: lists of module paths relative to their common parent (an encoder layer), the first
    one the group's head: where `<stem>.<head>.weight` stands in `names`, all weights of the group, then all its biases, are laid out there
    (`_Slab.span` then reads them as ONE stacked Linear; the twins of two branches sit a constant stride apart for `_Lin2`).  Everything
    else keeps its place.  The head is matched with its leading '.': `crossattention.self.query` ends in `attention.self.query`."""
    heads = {}
    for n in names:
        for members in groups:
            tail = members[0] + ".weight"
            if n.endswith("." + tail):
                heads[n] = [n[:-len(tail)] + m + "." + y for y in ("weight", "bias") for m in members]
    grouped = {m for g in heads.values() for m in g}
    out, seen = [], set()
    for n in names:
        if n in seen:
            continue
        if n in heads:
            for m in heads[n]:
                out.append(m); seen.add(m)
        elif n not in grouped:
            out.append(n); seen.add(n)
    for n in names:                                                                 # (a grouped name whose group head is missing: keep it)
        if n not in seen:
            out.append(n); seen.add(n)
    assert sorted(out) == sorted(names)
    return out


def head_view(x: torch.Tensor, groups: int, rows: int, heads: int, head_dim: int, part: int = 0, parts: int = 1) -> torch.Tensor:
    """(groups * rows, parts * heads * head_dim) projection(s) -> (groups, heads, rows, head_dim) view of the head slices of projection
    `part` (no copy)."""
    return x.view(groups, rows, parts, heads, head_dim)[:, :, part].permute(0, 2, 1, 3)


def loss_scale(amax: float) -> float:
    """The power of two S that puts the largest entry `amax` of the incoming gradient near 512: every adjoint is linear in it, so an fp16
    pass runs on S * gradient - its 16-bit intermediate gradients then sit in fp16's normal range - and `_finish_backward` divides by S."""
    return 2.0 ** round(math.log2(512.0 / amax)) if amax > 0 and math.isfinite(amax) else 1.0


def draw_seed(seed: Optional[int] = None) -> int:
    """The base seed of one forward's dropout sites: `seed`, or one 62-bit draw from torch's global CPU generator (`torch.manual_seed`
    governs it, as it governs the reference's dropout; no device read)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if seed is None else seed


# ---- the resumable part of the training state that is neither a parameter nor an optimizer moment ---------------------------------------
# Two passes number their random draws themselves: train.NlvrTrainer's dropout sites and train_vit.VitTrainer's DropPath draw are functions
# of the trainer's (seed, step_no).  Everything else that is random in a training-mode pass - `draw_seed` above (the stage-I trainer and the
# train-mode z_t of train_med.py) and the frozen ViT's DropPath draw (BLIP_NLVR.img_embed) - reads torch's global CPU generator; none reads
# a device generator.
_COUNTED = {"fusion": "_trainer", "vit": "_vit_trainer"}     # key in the state -> the model attribute that holds the trainer
_PENDING = "_pending_counters"                                # counters loaded before their trainer exists (trainers are built lazily)


def training_state(model) -> dict:
    """What a checkpoint needs besides `model.state_dict()` and `AdamW.state_dict()` for the run to continue with the random draws it
    would have made (BLIP_NLVR and BLIP_Retrieval): the (seed, step_no) of the fusion and the ViT trainer where the model has them (or has
    them pending from `load_training_state`), and the state of torch's global CPU generator.  Plain values and one uint8 tensor: it sits
    in the same file and loads under torch.load(weights_only=True)."""
    state = {"format": 1, "cpu_rng_state": torch.get_rng_state()}
    pending = getattr(model, _PENDING, None) or {}
    for key, attr in _COUNTED.items():
        tr = getattr(model, attr, None)
        if tr is not None and hasattr(tr, "step_no"):         # (the stage-I trainer keeps no count: it draws from the generator)
            state[key] = {"seed": int(tr.seed), "step_no": int(tr.step_no)}
        elif key in pending:
            state[key] = dict(pending[key])
    return state


def load_training_state(model, state: dict):
    """Restore `training_state`'s result.  Counters of a trainer that exists are set on it; those of one that does not exist yet - a fresh
    model builds its trainers at the first training-mode forward - wait on the model until `apply_pending_counters` hands them to the new
    trainer, once.  A trainer rebuilt after that (other dropout probabilities, other operand type) starts from 0, as ever."""
    if state.get("format") != 1:
        raise ValueError(f"load_training_state: format {state.get('format')!r}; this build reads format 1")
    counters = {key: {"seed": int(state[key]["seed"]), "step_no": int(state[key]["step_no"])} for key in _COUNTED if key in state}
    rng = state["cpu_rng_state"]
    pending = {}
    for key, attr in _COUNTED.items():
        tr = getattr(model, attr, None)
        if key not in counters:
            continue
        if tr is not None and hasattr(tr, "step_no"):
            tr.seed, tr.step_no = counters[key]["seed"], counters[key]["step_no"]
        else:
            pending[key] = counters[key]
    setattr(model, _PENDING, pending)
    torch.set_rng_state(rng.cpu())


def apply_pending_counters(model, key: str, trainer):
    """Called where a counted trainer is constructed (train.fusion_train, train_vit.vit_train): hand it the counters a checkpoint left on
    the model, and forget them."""
    pending = getattr(model, _PENDING, None)
    if pending and key in pending:
        c = pending.pop(key)
        trainer.seed, trainer.step_no = c["seed"], c["step_no"]


class Trainer:
    """Base of the three passes.  A subclass sets `model`, `dtype`, `geo` (with `layer_norm_eps`) and `_nh` / `_hd` (heads, head dimension),
    and provides `_GROUPS` (slab_order's table), `_KEY` (the part of `model.weights_key` its parameters belong to), `_NAME` (for messages),
    `_trained(name)`, `_build_layers(slab, lin, ln)` and `_bind_grads(slab)`."""

    _GROUPS: Sequence[Sequence[str]] = ()
    _KEY = _NAME = ""
    _EMB = "text_encoder.embeddings."
    grads_finite = None                   # fp16: 0-dim device bool "the last backward's gradients are all finite" (AdamW.step consumes it)
    grad_scale = 1.0

    @classmethod
    def _order(cls, names: List[str]) -> List[str]:
        return slab_order(names, cls._GROUPS)

    def _pack(self):
        """Per step: refresh the 16-bit parameter copies and a zeroed gradient buffer (three launches).  The layer objects - views of the
        persistent buffers - are built once and rebuilt only when the model was moved / re-cast."""
        slab = getattr(self, "slab", None)
        if slab is None or slab.dtype != self.dtype or not slab.valid():           # first step, or the model was moved / re-cast
            P = dict(self.model.named_parameters())
            slab = self.slab = _Slab(P, self._order([n for n in P if self._trained(n)]), self.dtype, key=lambda: self.model.weights_key(self._KEY))
            slab.begin_step()                                                       # allocates the 16-bit buffers the views below slice
            lins: List[_Lin] = []

            def lin(name, group=False):
                lins.append(_Lin(slab, name, group))
                return lins[-1]
            self._build_layers(slab, lin, lambda name: _LN(slab, name, self.geo.layer_norm_eps))
            slab.plan = T.TransposePlan([l.transpose_entry for l in lins], slab.flat32.device)
        slab.begin_step()
        self._bind_grads(slab)

    def _bind_grads(self, slab: _Slab):
        """Views of the step's gradient buffer that the pass writes directly (here: the BERT embeddings' of both text passes)."""
        self.dword, self.dpos = slab.grad(self._EMB + "word_embeddings.weight"), slab.grad(self._EMB + "position_embeddings.weight")

    def _wgrad_grouped(self, queue: list):
        """The layer's queued weight gradients in one launch; deterministic mode: one workgroup per output tile (splits = 1, plain adds)."""
        if self.slab.work is None:
            T.wgrad_grouped(queue)
        else:
            T.wgrad_grouped(queue, splits=1)

    def _heads(self, x: torch.Tensor, groups: int, rows: int, part: int = 0, parts: int = 1) -> torch.Tensor:
        return head_view(x, groups, rows, self._nh, self._hd, part, parts)

    def _finish_backward(self) -> Dict[str, torch.Tensor]:
        """{name: gradient}: views of the flat gradient buffer.  fp16 operands: an intermediate gradient above 65504 turns into inf -> NaN in
        the weight gradients.  What GradScaler's unscale_ / found_inf do for the reference (stage2_train.py:215-218) in ONE pass over the
        buffer: divide by the loss scale and note any non-finite element in a device flag that AdamW.step consumes on the device.  bf16 has
        fp32's exponent range: no scale, no pass."""
        slab = self.slab
        self.grads_finite = _unscale_and_check(slab.gflat, self.grad_scale) if self.dtype == torch.float16 else None
        slab.checked = None if self.grads_finite is None else (slab.gflat.data_ptr(), self.grads_finite, slab.gflat._version)     # (AdamW.step: this buffer is tested)
        return {n: slab.grad(n) for n in slab.names}

    # The saved activations, the dropout seed and the flat gradient buffer are single slots on the trainer: an autograd node may only be
    # differentiated while they still belong to ITS forward, and only once.
    def _claim(self, ctx):
        self.generation = ctx.generation = getattr(self, "generation", 0) + 1
        self.consumed = False

    def _consume(self, ctx):
        if self.generation != ctx.generation:
            raise RuntimeError(f"{self._NAME}: another training-mode forward ran before this one's backward - the saved activations belong "
                               "to the later forward.  Call backward() after each forward (gradients accumulate in .grad across steps), or "
                               "run the other forward under torch.no_grad() / in .eval() mode")
        if self.consumed:
            raise RuntimeError(f"{self._NAME}: second backward through the same forward (retain_graph): the hand-written reverse pass keeps "
                               "one gradient buffer and one set of saved activations per forward; run the forward again")
        self.consumed = True
