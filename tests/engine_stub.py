"""`candidate_reranking_cir_amd.ops` as recording stubs, for running `NlvrEngine.forward` on a CPU: every kernel call is answered with an
uninitialised tensor (or split-operand stand-in) of the shape, strides and type the real call returns, and recorded twice -
  `calls`: the short tuples tests/test_fold_long_cpu.py asserts on (gemm / attention shapes, which fold ran);
  `trace`: the launch trace - per call the op name and every argument and result: tensors as (shape, strides, dtype, storage offset,
           identity token), the engine's weights by their name, scalars by value.  The identity token of a tensor is the order in which its
           storage was first seen, so "reads what call 17 wrote" and "writes into a view of that buffer" are part of the trace.
Two forwards issue the same launches on the same views exactly when their traces are equal."""
import warnings

import torch


class Rows:
    """Stand-in for ops.Split8Operand (`width` 4: uint8 rows (..., 4K)) and ops.SplitOperand (`width` 3: fp16 rows (..., 3K))."""
    dtype = torch.float32

    def __init__(self, rows, k, width):
        assert rows.shape[-1] == width * k
        self.rows, self.k, self.width, self.shape, self.device = rows, k, width, rows.shape[:-1] + (k,), rows.device

    def dim(self):
        return self.rows.dim()

    def view(self, *lead):
        return Rows(self.rows.view(*lead, self.width * self.k), self.k, self.width)


def weight_names(engine) -> dict:
    """storage address -> name, for every tensor the engine packed"""
    named = {f"layers[{i}].{k}": v for i, ly in enumerate(engine.layers) for k, v in ly.items()}
    named.update({k: getattr(engine, k) for k in ("word", "posemb", "ge", "be", "wc0", "bc0", "wc2", "bc2")})
    if engine.cls_fold is not None:
        named.update({"cls_fold.wkt[0]": engine.cls_fold["wkt"][0], "cls_fold.wkt[1]": engine.cls_fold["wkt"][1],
                      "cls_fold.wv": engine.cls_fold["wv"], "cls_fold.bv": engine.cls_fold["bv"]})
    return {t.untyped_storage().data_ptr(): name for name, t in named.items() if torch.is_tensor(t)}


class StubOps:
    ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2
    PROFILE_GEMM = PROFILE_ATTN = None

    def __init__(self, engine=None):
        self.calls, self.trace = [], []
        self._weights = weight_names(engine) if engine is not None else {}
        self._tokens, self._alive = {}, []          # (`_alive` keeps every storage seen, so that no address is handed out twice)

    # ---------------------------------------------------------------------------------------- recording
    def _describe(self, x):
        if isinstance(x, Rows):
            return ("rows", x.width, x.k, self._describe(x.rows))
        if torch.is_tensor(x):
            ptr = x.untyped_storage().data_ptr()
            view = (tuple(x.shape), tuple(x.stride()), str(x.dtype), x.storage_offset())
            if ptr in self._weights:
                return ("weight", self._weights[ptr]) + view
            if ptr not in self._tokens:
                self._tokens[ptr] = len(self._tokens)
                self._alive.append(x)
            return ("tensor",) + view + (self._tokens[ptr],)
        if isinstance(x, (tuple, list)):
            return tuple(self._describe(v) for v in x)
        return str(x) if isinstance(x, torch.dtype) else x

    def _record(self, name, args, result):
        self.trace.append((name, tuple((k, self._describe(v)) for k, v in args.items()), self._describe(result)))
        return result

    # ---------------------------------------------------------------------------------------- the ops NlvrEngine.forward calls
    def embed_layernorm(self, ids, word, pos, gamma, beta, eps, dtype16=torch.bfloat16, stream_dtype=torch.float32):
        args = dict(locals()); del args["self"]
        y = torch.empty(tuple(ids.shape) + (word.shape[1],), dtype=stream_dtype)
        return self._record("embed_layernorm", args, (y, y if dtype16 == torch.float32 else torch.empty(y.shape, dtype=dtype16)))

    def gather_rows(self, src, index, dtype=None):
        args = dict(locals()); del args["self"]
        n = src.shape[0] if index is None else index.numel()
        return self._record("gather_rows", args, torch.empty((n,) + tuple(src.shape[1:]), dtype=dtype or src.dtype))

    def gemm(self, a, w, bias=None, residual=None, act=0, out_dtype=None, out=None):
        args = dict(locals()); del args["self"]
        self.calls.append(("gemm", tuple(a.shape), tuple(w.shape)))
        lead, n = tuple(a.shape[:-1]), w.shape[-2]
        split = 4 if (isinstance(a, Rows) and a.width == 4) or (not isinstance(a, Rows) and a.dtype == torch.float32 and hasattr(w, "_split8")) else \
            3 if isinstance(a, Rows) or (a.dtype == torch.float32 and hasattr(w, "_split3")) else 0
        if out is not None:
            y = out
        elif split and act == self.ACT_GELU:             # fc1 on a multi-product path: the GELU output is the next GEMM's operand rows
            y = Rows(torch.empty(lead + (split * n,), dtype=torch.uint8 if split == 4 else torch.float16), n, split)
        else:
            y = torch.empty(lead + (n,), dtype=torch.float32 if split else (out_dtype or a.dtype))
        return self._record("gemm", args, y)

    def attention(self, q, k, v, out, scale, mask=None, kv_index=None):
        args = dict(locals()); del args["self"]
        self.calls.append(("attention", tuple(q.shape), tuple(k.shape)))
        assert out.shape == q.shape and out.dtype == q.dtype
        return self._record("attention", args, out)

    def attention_split8(self, q, k, v, scale, mask=None):
        args = dict(locals()); del args["self"]
        b1, b0, lq, d = q.shape
        return self._record("attention_split8", args, Rows(torch.empty((b1, b0, lq, 4 * d), dtype=torch.uint8), d, 4))

    @staticmethod
    def _ln_lead(x, gamma, residual):                    # (ops._ln_views' batch broadcast)
        nb = max(x.shape[0] if x.dim() == 3 else 1, gamma.shape[0] if gamma.dim() == 2 else 1,
                 residual.shape[0] if residual is not None and residual.dim() == 3 else 1)
        return (nb, x.shape[-2]) if (x.dim() == 3 or nb > 1) else (x.shape[-2],)

    def layernorm(self, x, gamma, beta, eps, residual=None, want32=True, dtype16=None, stream_dtype=torch.float32):
        args = dict(locals()); del args["self"]
        shape = self._ln_lead(x, gamma, residual) + (x.shape[-1],)
        return self._record("layernorm", args, (torch.empty(shape, dtype=stream_dtype) if want32 else None,
                                                torch.empty(shape, dtype=dtype16) if dtype16 is not None else None))

    def layernorm_split8(self, x, gamma, beta, eps, residual=None, want_stream=True):
        args = dict(locals()); del args["self"]
        lead, cols = self._ln_lead(x, gamma, residual), x.shape[-1]
        return self._record("layernorm_split8", args, (torch.empty(lead + (cols,), dtype=torch.float32) if want_stream else None,
                                                       Rows(torch.empty(lead + (4 * cols,), dtype=torch.uint8), cols, 4)))

    def cls_cross_attention(self, x, qp, scale, out=None, x_index=None):
        args = dict(locals()); del args["self"]
        return self._record("cls_cross_attention", args, torch.empty((qp.shape[0], 32, x.shape[2]), dtype=x.dtype))

    def cross_attention_folded(self, q, x, wkt, wvp, bv, out, l, scale, heads=12, mask=None):
        args = dict(locals()); del args["self"]
        self.calls.append(("folded", l, x.shape[1], mask is not None))
        return self._record("cross_attention_folded", args, out)

    def cross_attention_folded_long(self, q, x, wkt, wvp, bv, out, l, scale, heads=12, mask=None):
        args = dict(locals()); del args["self"]
        self.calls.append(("folded_long", l, x.shape[1], mask is not None))
        return self._record("cross_attention_folded_long", args, out)

    def small_linear(self, x, w, bias):
        args = dict(locals()); del args["self"]
        return self._record("small_linear", args, torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32))


def run_forward(engine, monkeypatch, l, n, q_n=1, k=2, cand_mask=False, dv=None, stub=None, **kw):
    """One stubbed `engine.forward` of `q_n` queries x `k` candidates each -> (stub, logits, the warnings raised).  `stub`: record into this
    one (a caller that expects the forward to raise keeps it to see what ran before); `kw`: further arguments of `forward`."""
    from candidate_reranking_cir_amd import engine as E
    stub = stub or StubOps(engine)
    monkeypatch.setattr(E, "ops", stub)
    d = engine.geo.hidden_size
    ids = torch.ones((q_n, l), dtype=torch.int64)
    cand = torch.zeros((q_n * k, n, dv or engine.geo.encoder_width), dtype=engine.xdtype)
    cm = torch.ones((q_n * k, n), dtype=torch.int64) if cand_mask else None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = engine.forward(ids, torch.ones_like(ids), torch.zeros((q_n, l, d)), cand, torch.arange(q_n).repeat_interleave(k), cand_mask=cm, **kw)
    assert tuple(out.shape) == (q_n * k, 2)
    return stub, out, list(w)
