"""ViT gradient checkpointing (`vit_grad_ckpt` / `vit_ckpt_layer`, `set_vit_checkpointing`) without a GPU: which blocks are checkpointed
(vit.py:158), what `train.vit_saved_bytes` says, the argument checks of cir_rows16_gelu_pair[_ordered] on fake addresses, and the list of
operators a `VitTrainer` forward and backward call with 0 and with 1 checkpointed block (recording stubs in the style of
tests/test_train_deterministic_cpu.py's `Recorder`; CPU tensors of the right shapes)."""
import pytest
import torch

from candidate_reranking_cir_amd import config, ops, synthetic, train, train_ops, train_vit
from candidate_reranking_cir_amd.blip import create_vit
from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval, blip_stage1
from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR, blip_stage2

BF = torch.bfloat16


def _tiny(depth=2, **kw):
    g = config.BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, encoder_width=128)
    v = config.VitGeometry(image_size=64, width=128, depth=depth, num_heads=2, drop_path_rate=0.0)
    return dict(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer(), **kw)


def _checkpointed(model):
    depth = model.vit_geometry.depth
    first = depth - train.vit_checkpointed_blocks(model)
    return {i for i in range(depth) if i >= first}


# ---------------------------------------------------------------------------------------------------------------- block selection
SETTINGS = [(False, 4), (True, 0), (True, 4), (True, 12), (True, 40)]


@pytest.mark.parametrize("factory", [blip_stage1, blip_stage2, BLIP_Retrieval, BLIP_NLVR], ids=lambda f: f.__name__)
@pytest.mark.parametrize("grad_ckpt,ckpt_layer", SETTINGS)
def test_block_selection_follows_the_reference(factory, grad_ckpt, ckpt_layer):
    depth = 12
    m = factory(**_tiny(depth=depth, vit_grad_ckpt=grad_ckpt, vit_ckpt_layer=ckpt_layer))
    want = {i for i in range(depth) if grad_ckpt and i >= depth - ckpt_layer}                 # vit.py:158 (with vit.py:103-105)
    assert _checkpointed(m) == want
    assert (m.vit_grad_ckpt, m.vit_ckpt_layer) == (grad_ckpt, ckpt_layer)                    # the model keeps what it was given
    # the setter reaches the same sets from any start, returns the model, and refuses a negative count
    other = factory(**_tiny(depth=depth))
    assert _checkpointed(other) == set() and other.vit_ckpt_blocks == 0                      # the default
    assert other.set_vit_checkpointing(ckpt_layer if grad_ckpt else 0) is other
    assert _checkpointed(other) == want
    assert _checkpointed(other.set_vit_checkpointing(0)) == set()
    with pytest.raises(ValueError):
        other.set_vit_checkpointing(-1)


def test_create_vit_keeps_its_return_value():
    g, width = create_vit("base", 384, use_grad_checkpointing=True, ckpt_layer=4, drop_path_rate=0.1)
    assert (width, g.depth, g.num_tokens) == (768, 12, 577) and not hasattr(g, "ckpt_layer")
    assert "carried by the MODEL" in create_vit.__doc__


# ---------------------------------------------------------------------------------------------------------------- vit_saved_bytes
PER_TOKEN = dict(x=3072, h16=1536, qkv=4608, ctx=1536, ctx32=3072, lse=48, x1=3072, h2=1536, z16=6144, f16=6144)      # width 768, 16-bit operands


def test_saved_bytes_at_the_reference_geometry():
    class M:                                                   # the function reads the geometry and the setting, nothing else
        vit_geometry = config.VitGeometry.named("base", 384)
        vit_ckpt_blocks = 0
    geo = M.vit_geometry
    assert (geo.width, geo.num_tokens, geo.depth) == (768, 577, 12) and geo.drop_path_rate > 0
    assert sum(PER_TOKEN.values()) == 30768 and PER_TOKEN["x"] + PER_TOKEN["x1"] == 6144
    assert train.vit_saved_bytes is train_vit.vit_saved_bytes
    batch, n = 16, 577
    patches = batch * (n - 1) * 3 * 16 * 16 * 2                # the 16-bit patch rows
    final = batch * n * 768 * 4                                # the fp32 stream the last LayerNorm's adjoint reads
    drop_path = 12 * 2 * batch * 4                             # the call's (depth, 2, batch) fp32 DropPath scales
    sizes = []
    for k in range(13):
        M.vit_ckpt_blocks = k
        sizes.append(train.vit_saved_bytes(M, batch))
        assert sizes[-1] == batch * n * ((12 - k) * 30768 + k * 6144) + patches + final + drop_path
    assert all(a > b for a, b in zip(sizes, sizes[1:]))                                        # strictly decreasing
    assert {a - b for a, b in zip(sizes, sizes[1:])} == {batch * n * (30768 - 6144)}          # per block, exactly
    M.vit_ckpt_blocks = 40
    assert train.vit_saved_bytes(M, batch) == sizes[12]                                       # more than depth: depth
    # the derived table: 213 MB per image unchecked, ~156 with 4 blocks, ~43 with all 12
    per_image = [s / batch / 1e6 for s in sizes]
    assert 212 < per_image[0] < 216 and 155 < per_image[4] < 160 and 43 < per_image[12] < 46
    geo0 = config.VitGeometry(image_size=64, width=128, depth=2, num_heads=2, drop_path_rate=0.0)
    M.vit_geometry, M.vit_ckpt_blocks = geo0, 0
    assert train.vit_saved_bytes(M, 3) == 3 * (16 * 768 * 2 + 17 * (2 * (3 * 512 + 2 * (3 * 128 + 3 * 128 + 2 * 512) + 8) + 512))


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_pair_entry_points_validate_before_any_launch():
    """Fake, never dereferenced, 16-byte aligned addresses (tests/test_abi.py): a valid argument list would launch, so only refusals."""
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    assert hasattr(c, "cir_rows16_gelu_pair") and hasattr(c, "cir_rows16_gelu_pair_ordered") and c.cir_version() == 15
    EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
    P, BF16, F16, F32 = 0x10000, 0, 1, 2
    names = ("a", "lda", "z", "ldz", "out", "ldo", "out_f", "ldf", "sums", "rows", "cols", "dtype")
    ok = dict(a=P, lda=64, z=P, ldz=64, out=P, ldo=64, out_f=P, ldf=64, sums=P, rows=4, cols=64, dtype=BF16)

    def plain(**over):
        a = {**ok, **over}
        return c.cir_rows16_gelu_pair(*[a[k] for k in names], None)

    def ordered(partials=P, partial_elems=64, **over):
        a = {**ok, **over}
        return c.cir_rows16_gelu_pair_ordered(*[a[k] for k in names], partials, partial_elems, None)

    for call in (plain, ordered):
        for ptr in ("a", "z", "out", "out_f"):
            assert call(**{ptr: None}) == EINVAL, (call.__name__, ptr)
            assert call(**{ptr: P + 2}) == EALIGN, (call.__name__, ptr)
        assert call(rows=0) == EINVAL and call(rows=-3) == EINVAL and call(cols=0) == EINVAL
        assert call(cols=12) == ESHAPE
        for ld in ("lda", "ldz", "ldo", "ldf"):
            assert call(**{ld: 60}) == EALIGN, (call.__name__, ld)
        assert call(dtype=F32) == EDTYPE and call(dtype=7) == EDTYPE
        assert call(dtype=F16, cols=12) == ESHAPE
        assert call(rows=65536 * 64) == ESHAPE                                                # more row blocks than a grid dimension takes
    # the ordered form: a workspace, large enough for ceil(rows / 64) * cols partial sums
    assert ordered(partials=None) == EINVAL
    assert ordered(partial_elems=63) == ESHAPE and ordered(partial_elems=0) == ESHAPE
    assert ordered(rows=65, partial_elems=127) == ESHAPE and ordered(rows=65, partial_elems=127, a=None) == EINVAL


# ---------------------------------------------------------------------------------------------------------------- launch list
class Recorder:
    """Recording stand-ins for every ops / train_ops entry point a VitTrainer calls, returning CPU tensors of the right shapes.  An
    `eltwise` call is recorded with its mode ("eltwise.gelu", ".add", ".scale")."""

    OPS = ("patchify", "vit_assemble", "gemm", "layernorm")
    TRAIN_OPS = ("eltwise", "attention_train_fwd", "attention_train_bwd", "gelu_bwd16", "gelu_bwd16_pair", "layernorm_bwd", "layernorm_bwd_fused",
                 "colsum", "colsum16", "wgrad", "wgrad_grouped", "rows_scale_add", "bmm", "grads_check")
    MODES = {train_ops.MODE_GELU: "gelu", train_ops.MODE_ADD: "add", train_ops.MODE_SCALE: "scale"}

    def __init__(self, monkeypatch):
        self.calls = []
        rec = self

        class Plan:
            def __init__(self, entries, device):
                self.entries = list(entries)

            def run(self, src, dst):
                rec.calls.append("transpose16_multi")
        for name in self.OPS:
            monkeypatch.setattr(ops, name, getattr(self, "_" + name))
        for name in self.TRAIN_OPS:
            monkeypatch.setattr(train_ops, name, getattr(self, "_" + name, None) or self._plain(name))
        monkeypatch.setattr(train_ops, "TransposePlan", Plan)

    def _plain(self, name):
        def fn(*a, **kw):
            self.calls.append(name)
        return fn

    def _patchify(self, image, patch, dt):
        self.calls.append("patchify")
        b, c, h, w = image.shape
        return torch.zeros((b * (h // patch) * (w // patch), c * patch * patch), dtype=dt)

    def _vit_assemble(self, pe, cls, pos, bsz):
        self.calls.append("vit_assemble")
        return torch.zeros((bsz, pos.shape[0], pos.shape[1]))

    def _gemm(self, a, w, bias=None, residual=None, out_dtype=torch.float32, out=None):
        self.calls.append("gemm")
        return out if out is not None else torch.zeros((a.shape[0], w.shape[0]), dtype=out_dtype)

    def _layernorm(self, x, g, b, eps, want32=True, dtype16=BF, stream_dtype=torch.float32):
        self.calls.append("layernorm")
        return (torch.zeros_like(x) if want32 else None), torch.zeros(x.shape, dtype=dtype16)

    def _eltwise(self, z, mode, dy=None, out_dtype=None, p_drop=0.0, seed=0, out=None):
        self.calls.append("eltwise." + self.MODES[mode])
        return out if out is not None else torch.zeros(z.shape, dtype=out_dtype or z.dtype)

    def _attention_train_fwd(self, q4, k4, v4, mask, out4, scale, p_drop, seed, out32=None):
        self.calls.append("attention_train_fwd")
        return torch.zeros(q4.shape[:3])

    def _gelu_bwd16(self, df, z, sums=None, work=None, out=None):
        self.calls.append("gelu_bwd16")
        return torch.zeros_like(df)

    def _gelu_bwd16_pair(self, df, z, sums=None, work=None, out=None, out_f=None):
        self.calls.append("gelu_bwd16_pair")
        assert out_f is not None and out_f.shape == z.shape          # the buffer fc2's queued weight gradient was handed
        self.pair_out_f = out_f
        return torch.zeros_like(df), out_f

    def _layernorm_bwd(self, x, gamma, dy, dgamma, dbeta, eps, work=None, dx=None):
        self.calls.append("layernorm_bwd")
        return torch.zeros_like(x)

    def _layernorm_bwd_fused(self, x, gamma, dy, dgamma, dbeta, eps, dtype16, **kw):
        self.calls.append("layernorm_bwd_fused")
        return torch.zeros_like(x), None

    def _wgrad_grouped(self, queue, splits=0):
        self.calls.append("wgrad_grouped")
        self.queues = getattr(self, "queues", []) + [list(queue)]


# What the parent commit's VitTrainer calls for a 2-block ViT (bf16 operands, no DropPath, default mode), written down from its code:
# `_pack` (the first call casts the slab and transposes the dgrad operands), then forward and backward.
FWD_BLOCK = ["layernorm", "gemm", "attention_train_fwd", "gemm", "layernorm", "gemm", "eltwise.gelu", "gemm"]
PARENT_FORWARD = ["eltwise.scale", "transpose16_multi", "patchify", "gemm", "vit_assemble"] + 2 * FWD_BLOCK + ["layernorm"]
BWD_BLOCK = ["eltwise.scale", "colsum16", "gemm", "gelu_bwd16", "gemm", "layernorm_bwd_fused", "eltwise.add",          # the MLP branch
             "eltwise.scale", "colsum16", "gemm", "attention_train_bwd", "colsum16", "gemm", "layernorm_bwd_fused", "eltwise.add",   # attention
             "wgrad_grouped"]
PARENT_BACKWARD = ["layernorm_bwd"] + 2 * BWD_BLOCK + ["colsum", "colsum", "eltwise.scale", "colsum16", "wgrad"]
RECOMPUTE = ["layernorm", "gemm", "attention_train_fwd", "layernorm", "gemm"]


def _run(monkeypatch, blocks):
    rec = Recorder(monkeypatch)
    m = BLIP_NLVR(**_tiny(depth=2)).set_compute_dtype(BF).set_vit_checkpointing(blocks)
    tr = train_vit.VitTrainer(m)
    assert tr.dtype == BF
    feats, sv = tr.forward(torch.zeros((3, 3, 64, 64)))
    fwd, rec.calls = rec.calls, []
    m.set_vit_checkpointing(2 - blocks)                          # changed between forward and backward: the backward follows the record
    tr.backward(torch.zeros_like(feats), sv)
    return fwd, rec.calls, sv, rec


def test_default_calls_what_the_parent_called(monkeypatch):
    fwd, bwd, sv, _ = _run(monkeypatch, 0)
    assert fwd == PARENT_FORWARD
    assert bwd == PARENT_BACKWARD
    assert sv["ckpt"] == [False, False] and all(len(s) == 10 for s in sv["blocks"])


def test_one_checkpointed_block_adds_the_recompute_and_the_pair(monkeypatch):
    fwd, bwd, sv, rec = _run(monkeypatch, 1)
    assert fwd == PARENT_FORWARD                                 # the forward launches what it launched
    assert sv["ckpt"] == [False, True] and sorted(sv["blocks"][1]) == ["x", "x1"] and len(sv["blocks"][0]) == 10
    # block 1 (differentiated first) is recomputed: layernorm x 2, gemm x 2, attention_train_fwd x 1, the pair kernel instead of gelu_bwd16,
    # and no GELU eltwise; block 0 as ever
    ckpt_block = RECOMPUTE + [("gelu_bwd16_pair" if c == "gelu_bwd16" else c) for c in BWD_BLOCK]
    assert bwd == ["layernorm_bwd"] + ckpt_block + BWD_BLOCK + PARENT_BACKWARD[-5:]
    mine = bwd[1:1 + len(ckpt_block)]
    assert "gelu_bwd16" not in mine and "eltwise.gelu" not in mine and mine.count("gelu_bwd16_pair") == 1
    extra = list(mine)
    for c in BWD_BLOCK:
        extra.remove("gelu_bwd16_pair" if c == "gelu_bwd16" else c)
    assert sorted(extra) == sorted(RECOMPUTE)
    # the buffer the pair kernel fills is the left operand of fc2's queued weight gradient, launched after it
    fc2 = [x16 for dy16, x16, dw in rec.queues[0] if x16.shape[1] == 512]
    assert len(fc2) == 1 and fc2[0] is rec.pair_out_f and bwd.index("gelu_bwd16_pair") < bwd.index("wgrad_grouped")


def test_off_the_128_grid_the_forward_kernels_recompute_gelu(monkeypatch):
    """Width 64: fc2's weight gradient (64 x 256) is not a queued product - `_Lin.bwd16` reads its left operand at once - so a checkpointed
    block recomputes gelu(z) up front with the forward's own launch and takes `gelu_bwd16`; the pair kernel is not called."""
    rec = Recorder(monkeypatch)
    kw = _tiny(depth=2)
    kw["vit_geometry"] = config.VitGeometry(image_size=64, width=64, depth=2, num_heads=1, drop_path_rate=0.0)
    m = BLIP_NLVR(**kw).set_compute_dtype(BF).set_vit_checkpointing(1)
    tr = train_vit.VitTrainer(m)
    feats, sv = tr.forward(torch.zeros((3, 3, 64, 64)))
    rec.calls = []
    tr.backward(torch.zeros_like(feats), sv)
    assert sv["ckpt"] == [False, True] and "gelu_bwd16_pair" not in rec.calls and rec.calls.count("gelu_bwd16") == 2
    assert rec.calls[1:7] == RECOMPUTE + ["eltwise.gelu"] and rec.calls.count("eltwise.gelu") == 1


def test_optimizer_step_is_refused_before_any_recompute(monkeypatch):
    from candidate_reranking_cir_amd import lib
    rec = Recorder(monkeypatch)
    m = BLIP_NLVR(**_tiny(depth=2)).set_compute_dtype(BF).set_vit_checkpointing(2)
    tr = train_vit.VitTrainer(m)
    feats, sv = tr.forward(torch.zeros((2, 3, 64, 64)))
    rec.calls = []
    monkeypatch.setattr(lib, "PARAM_EPOCH", [lib.PARAM_EPOCH[0] + 1])                         # what an optimizer step does
    with pytest.raises(RuntimeError, match="parameters were updated"):
        tr.backward(torch.zeros_like(feats), sv)
    assert rec.calls == []
