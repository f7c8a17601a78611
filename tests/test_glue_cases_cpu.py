"""tests/glue_cases.py checked without a GPU.  For every case torch's own CPU operator in the kernel's precision stands in for the
kernel and must pass `glue_cases.check`, the comparison the GPU tests apply: a correct single-precision implementation stays inside
every bound, so no GPU failure can be blamed on a bound that was too tight.  For every kernel at least one stand-in that is wrong in
VALUE only (bias dropped, K-tail skipped, tie-break reversed, clamp removed, modes swapped ...) must fail the same comparison: the
bounds are not so loose that the obvious mistakes pass."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_cases as G
from tests import helpers as H

BF16, F16, F32 = G.BF16, G.F16, G.F32


def _case(kernel, case_id):
    return next(c for c in G.CASES[kernel] if c.id == case_id)


def _passes(case, outputs):
    fails = G.check(case, outputs)
    assert not fails, fails


def _fails(case, outputs):
    assert G.check(case, outputs), f"{case}: a wrong stand-in passed the comparison"


# ------------------------------------------------------------------------------------------------ the rounding term
def test_half_ulp_is_attained():
    """half_ulp is the exact half spacing: torch's own rounding reaches it (so nothing smaller can be asked of a correct kernel) and
    never exceeds it.  bf16 just above a power of two errs by 2^-8 |y| - twice the flat 2^-9 |y|."""
    for dtype, p in ((BF16, 8), (F16, 11)):
        y = torch.tensor([1.0 + 2.0 ** -p, 3.0 + 2.0 ** (1 - p), 2.0 ** -5 * (1 + 2.0 ** -p)], dtype=torch.float64)      # rounding ties
        err = (y.float().to(dtype).double() - y).abs()
        assert torch.equal(err, G.half_ulp(y, dtype))
        g = torch.Generator().manual_seed(int(p))
        y = torch.randn((100000,), generator=g, dtype=torch.float64) * torch.logspace(-30, 3, 100000, dtype=torch.float64)
        assert bool(((y.float().to(dtype).double() - y).abs() <= G.half_ulp(y, dtype) + y.abs() * G.U).all())
    y = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
    assert float((y.float().bfloat16().double() - y).abs()) > 2.0 ** -9 * float(y)
    assert float(G.half_ulp(torch.tensor([0.0]), F16)) == 2.0 ** -25 and float(G.half_ulp(torch.tensor([1e-7]), F16)) == 2.0 ** -25


# ------------------------------------------------------------------------------------------------ linear_f32
def _linear_standin(c, wrong=None):
    i = G.inputs(c)
    x, w, bias, mode = i["x"], i["w"], i["bias"], c.mode
    if wrong == "k_tail":
        kk = (x.shape[1] // 16) * 16
        x, w = x[:, :kk], w[:, :kk]
    if wrong == "swap_modes":
        mode = {0: 0, 1: 2, 2: 1}[mode]
    v = x @ w.T
    if bias is not None and wrong != "no_bias":
        v = v + bias
    return dict(y=1.0 - v if mode == 1 else (v - 1.0 if mode == 2 else v))


@pytest.mark.parametrize("c", G.CASES["linear_f32"], ids=G.case_id)
def test_linear_f32_standin(c):
    _passes(c, _linear_standin(c))


@pytest.mark.parametrize("case_id,wrong", [("37x9x50-mode0-bias1-strided0", "no_bias"), ("37x9x50-mode0-bias0-strided1", "k_tail"),
                                           ("65x129x15-mode1-bias0-strided0", "k_tail"), ("64x6346x256-mode1-bias0-strided1", "swap_modes"),
                                           ("63x65x17-mode2-bias1-strided1", "swap_modes")])
def test_linear_f32_wrong(case_id, wrong):
    c = _case("linear_f32", case_id)
    _fails(c, _linear_standin(c, wrong))


def test_linear_f32_mode2_is_negative_of_mode1_standin():
    for c in G.CASES["linear_f32"]:
        if c.mode == 2 and c.mnk[0] <= 65:
            i = G.inputs(c)
            v = i["x"] @ i["w"].T + (i["bias"] if i["bias"] is not None else 0.0)
            assert torch.equal(v - 1.0, -(1.0 - v))                  # fp32 subtraction is antisymmetric: the header's promise is attainable


# ------------------------------------------------------------------------------------------------ l2_normalize
@pytest.mark.parametrize("c", G.CASES["l2_normalize"], ids=G.case_id)
def test_l2_normalize_standin(c):
    y = F.normalize(G.inputs(c)["x"], dim=1)
    _passes(c, dict(y=y))
    if c.special == "zero_row":
        assert bool((y[c.rows // 2] == 0).all())
    if c.special == "tiny_row":                                      # divided by the clamp (norm 1e-8 comes out), not by its own norm (1 would)
        assert float(y[c.rows // 2].double().norm()) < 0.5


@pytest.mark.parametrize("special,wrong", [("zero_row", "no_clamp"), ("tiny_row", "no_clamp"), ("tiny_row", "eps_added"),
                                           ("none", "l1_norm")])
def test_l2_normalize_wrong(special, wrong):
    c = _case("l2_normalize", f"rows5-cols65-{special}" if special != "none" else "rows5-cols65-none")
    x = G.inputs(c)["x"]
    n = x.double().norm(dim=1, keepdim=True).float()          # no_clamp: 0 / 0 on the zero row, a unit vector where 1e-8 is due on the tiny one
    _fails(c, dict(y=x / n if wrong == "no_clamp" else (x / (n + 1e-6) if wrong == "eps_added" else x / x.abs().sum(1, keepdim=True))))


# ------------------------------------------------------------------------------------------------ argsort_desc
def _argsort_standin(logits, wrong=None):
    """An argsort that shares nothing with the reference's: numpy's lexsort on (-value, index)."""
    v = logits.numpy().astype(np.float64)
    if wrong != "nan_kept":
        v = np.where(np.isnan(v), -np.inf, v)
    idx = np.broadcast_to(np.arange(v.shape[1]), v.shape)
    rows = [np.lexsort((-idx[r] if wrong == "tie_reversed" else idx[r], -v[r])) for r in range(v.shape[0])]
    return dict(idx=torch.from_numpy(np.stack(rows).astype(np.int64)))


@pytest.mark.parametrize("c", G.CASES["argsort_desc"], ids=G.case_id)
def test_argsort_desc_standin(c):
    _passes(c, _argsort_standin(G.inputs(c)["logits"]))


@pytest.mark.parametrize("case_id,wrong", [("q3-k257-levels8", "tie_reversed"), ("q3-k2-all_equal", "tie_reversed"), ("q3-k6346-signed_zero", "tie_reversed"),
                                           ("q3-k8192-inf", "tie_reversed"), ("q3-k255-nan", "tie_reversed"), ("q3-k255-nan", "nan_kept"),
                                           ("q3-k1-nan", None)])
def test_argsort_desc_wrong(case_id, wrong):
    c = _case("argsort_desc", case_id)
    if wrong is None:                                                # K = 1 has one answer; a NaN there must not derail the reference
        assert torch.equal(G.ref64(c)["idx"], torch.zeros((3, 1), dtype=torch.int64))
        return
    _fails(c, _argsort_standin(G.inputs(c)["logits"], wrong))


def test_argsort_desc_nan_contract():
    """NaN ranks with -inf, by index: [nan, 1, -inf, nan, +inf, 1] -> [4, 1, 5, 0, 2, 3]."""
    v = torch.tensor([[math.nan, 1.0, -math.inf, math.nan, math.inf, 1.0]])
    assert G.argsort_ref(v).tolist() == [[4, 1, 5, 0, 2, 3]]
    assert _argsort_standin(v)["idx"].tolist() == [[4, 1, 5, 0, 2, 3]]


# ------------------------------------------------------------------------------------------------ rank_index
@pytest.mark.parametrize("c", G.CASES["rank_index"], ids=G.case_id)
def test_rank_index_standin(c):
    i = G.inputs(c)
    neg = i["pred"] @ i["index"].T - 1.0
    order = torch.argsort(neg, dim=1, descending=True, stable=True)
    assert not G.check(c, dict(dist=-neg))
    fails = G.rank_failures(c, order, neg)
    assert not fails, fails
    dist, bmax = G.ref64(c)["dist"], float(G.bound(c)["dist"].max())
    gaps = dist.sort(dim=1).values.diff(dim=1)
    print(f"{c}: max(bound) {bmax:.3e}, min row std {float(dist.std(dim=1).min()):.3f}, adjacent gaps above 2 max(bound): "
          f"{float((gaps > 2 * bmax).double().mean()):.2f}")
    # (about half of the adjacent float64 gaps exceed 2 max(bound): the walk pins those pairs - test_rank_index_wrong[one_swap] shows it bite)


@pytest.mark.parametrize("wrong", ["descending_distance", "bf16_features", "one_swap"])
def test_rank_index_wrong(wrong):
    c = _case("rank_index", "q64-n6346")
    i = G.inputs(c)
    neg = i["pred"] @ i["index"].T - 1.0
    if wrong == "descending_distance":                               # mode 1 where mode 2 was meant
        order = torch.argsort(-neg, dim=1, descending=True, stable=True)
    elif wrong == "bf16_features":
        order = torch.argsort(i["pred"].bfloat16().float() @ i["index"].bfloat16().float().T, dim=1, descending=True, stable=True)
    else:                                                            # two well-separated neighbours exchanged in one row
        order = torch.argsort(neg, dim=1, descending=True, stable=True)
        order[17, [100, 140]] = order[17, [140, 100]]
    assert G.rank_failures(c, order, None if wrong == "bf16_features" else neg)


# ------------------------------------------------------------------------------------------------ gather_rows
def _gather_standin(c, wrong=None):
    i = G.inputs(c)
    src, index = i["src"], i["index"]
    if index is None:
        return dict(dst=src.to(c.dst))
    rows = index % c.src_rows if wrong == "wrap" else index.clamp(0, c.src_rows - 1)
    if wrong == "off_by_one":
        rows = (rows + 1).clamp(max=c.src_rows - 1)
    return dict(dst=src.index_select(0, rows).to(c.dst))


@pytest.mark.parametrize("c", G.CASES["gather_rows"], ids=G.case_id)
def test_gather_rows_standin(c):
    _passes(c, _gather_standin(c))


@pytest.mark.parametrize("wrong", ["wrap", "off_by_one"])
@pytest.mark.parametrize("row_elems,src_rows,n_rows", [(8, 37, 300), (G.VIT_ROW, 4, 5)])
def test_gather_rows_wrong(row_elems, src_rows, n_rows, wrong):
    c = _case("gather_rows", f"src_f32-dst_bf16-row_elems{row_elems}-src_rows{src_rows}-n_rows{n_rows}-clamp")
    _fails(c, _gather_standin(c, wrong))


# ------------------------------------------------------------------------------------------------ patchify
def _patchify_standin(c, wrong=None):
    img = G.inputs(c)["image"].float()
    cols = F.unfold(img, kernel_size=16, stride=16).transpose(1, 2).reshape(-1, 768)           # (c, ky, kx) column order, like the kernel's
    if wrong == "kx_ky":
        cols = cols.view(-1, 3, 16, 16).transpose(2, 3).reshape(-1, 768)
    return dict(patches=cols.to(c.dst))


@pytest.mark.parametrize("c", G.CASES["patchify"], ids=G.case_id)
def test_patchify_standin(c):
    _passes(c, _patchify_standin(c))


def test_patchify_wrong():
    for case_id in ("px224-src_f32-dst_bf16-b1-offset0", "px384-src_f16-dst_f16-b2-offset0"):
        c = _case("patchify", case_id)
        _fails(c, _patchify_standin(c, "kx_ky"))


# ------------------------------------------------------------------------------------------------ vit_assemble
def _assemble_standin(c, wrong=None):
    (b, p, d), i = c.bpd, G.inputs(c)
    pos = i["pos"]
    if wrong == "cls_without_pos":
        pos = torch.cat([torch.zeros((1, d)), pos[1:]])
    if wrong == "pos_shifted":
        pos = torch.cat([pos[:1], pos[:-1]])
    x = torch.cat([i["cls"].expand(b, 1, d), i["proj"].float().view(b, p, d)], dim=1) + pos[None]
    return dict(x=x.to(c.stream))


@pytest.mark.parametrize("c", G.CASES["vit_assemble"], ids=G.case_id)
def test_vit_assemble_standin(c):
    out = _assemble_standin(c)
    _passes(c, out)
    if c.stream == F16:                                              # the two statements of the issue, literally
        (b, p, d), i = c.bpd, G.inputs(c)
        assert torch.equal(out["x"][:, 1:], (i["proj"].float().view(b, p, d) + i["pos"][1:]).half())
        assert torch.equal(out["x"][:, 0], (i["cls"] + i["pos"][0]).half().expand(b, d))


@pytest.mark.parametrize("wrong", ["cls_without_pos", "pos_shifted"])
@pytest.mark.parametrize("stream", ["f32", "f16"])
def test_vit_assemble_wrong(stream, wrong):
    c = _case("vit_assemble", f"1x196x768-stream_{stream}")
    _fails(c, _assemble_standin(c, wrong))


# ------------------------------------------------------------------------------------------------ small_linear
def _small_linear_standin(c, wrong=None):
    i = G.inputs(c)
    x, w = i["x"].float(), i["w"].float()
    if wrong == "last_pass":                                         # the partial last 512-wide pass skipped
        x = x.clone()
        x[:, (c.k // 512) * 512:] = 0
    y = x @ w.T
    if i["bias"] is not None and wrong != "no_bias":
        y = y + i["bias"]
    return dict(y=y)


@pytest.mark.parametrize("c", G.CASES["small_linear"], ids=G.case_id)
def test_small_linear_standin(c):
    _passes(c, _small_linear_standin(c))


@pytest.mark.parametrize("case_id,wrong", [("m5-n8-k520-dt_bf16-bias0-strided0", "last_pass"), ("m5-n8-k520-dt_f16-bias1-strided1", "last_pass"),
                                           ("m5-n8-k520-dt_f16-bias1-strided1", "no_bias"), ("m4099-n2-k768-dt_bf16-bias1-strided1", "no_bias"),
                                           ("m4099-n2-k768-dt_bf16-bias0-strided0", "last_pass")])
def test_small_linear_wrong(case_id, wrong):
    c = _case("small_linear", case_id)
    _fails(c, _small_linear_standin(c, wrong))


def test_small_linear_case_table_covers_the_grid():
    cs = G.CASES["small_linear"]
    for key, values in (("n", range(1, 9)), ("k", (8, 504, 512, 520, 768, 1024)), ("m", (1, 3, 4, 5, 4099)), ("dt", (BF16, F16)), ("bias", (0, 1)),
                        ("strided", (0, 1))):
        for v in values:
            assert any(getattr(c, key) == v for c in cs), (key, v)
            for k in (8, 504, 512, 520, 768, 1024):                  # every value of every axis meets every K (the 512-wide passes)
                assert key in ("m", "k") or any(getattr(c, key) == v and c.k == k for c in cs), (key, v, k)


# ------------------------------------------------------------------------------------------------ embed_layernorm
def _embed_ln_standin(c, wrong=None):
    i = G.inputs(c)
    pos = i["pos"][1:c.l + 1] if wrong == "pos_shifted" and c.l < 512 else i["pos"][:c.l]
    x = i["word"][i["ids"]] + pos[None]
    if wrong == "unbiased_var":
        y = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, keepdim=True, unbiased=True) + G.EMBED_EPS) * i["gamma"] + i["beta"]
    else:
        y = F.layer_norm(x, (c.cols,), i["gamma"], i["beta"], 1e-5 if wrong == "eps" else G.EMBED_EPS)
    return dict(stream=y.to(c.stream)) if c.dt16 == F32 else dict(stream=y.to(c.stream), y16=y.to(c.dt16))


@pytest.mark.parametrize("c", G.CASES["embed_layernorm"], ids=G.case_id)
def test_embed_layernorm_standin(c):
    _passes(c, _embed_ln_standin(c))


@pytest.mark.parametrize("case_id,wrong", [("cols768-l42-stream_f32-dt16_bf16", "pos_shifted"), ("cols128-l1-stream_f16-dt16_f16", "pos_shifted"),
                                           ("cols1024-l32-stream_f32-dt16_f32", "eps"), ("cols768-l512-stream_f32-dt16_f16", "unbiased_var"),
                                           ("cols128-l32-stream_f16-dt16_bf16", "unbiased_var")])
def test_embed_layernorm_wrong(case_id, wrong):
    c = _case("embed_layernorm", case_id)
    _fails(c, _embed_ln_standin(c, wrong))


# ------------------------------------------------------------------------------------------------ eltwise
def _eltwise_standin(c, wrong=None):
    i = G.inputs(c)
    z, d = i["z"].float(), i["dy"]
    if c.mode == "gelu":             # the erf form spelled out in fp32 operators (F.gelu may take a vendor path with an approximated erf)
        y = F.gelu(z, approximate="tanh") if wrong else 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))
    elif c.mode == "gelu_bwd":
        if wrong:
            zz = z.clone().requires_grad_(True)
            F.gelu(zz, approximate="tanh").backward(d)
            y = zz.grad
        else:
            y = d * (0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z))
    elif c.mode == "relu":
        y = torch.where(z > (0.5 if wrong else 0.0), z, torch.zeros_like(z))
    elif c.mode == "relu_bwd":
        y = torch.where(z >= 0, d, torch.zeros_like(d)) if wrong else torch.where(z > 0, d, torch.zeros_like(d))
    elif c.mode == "dropout":
        p = np.float32(G.ELT_P["dropout"])
        keep = H.splitmix_keep(G.ELT_SEED + (1 if wrong == "seed" else 0), c.n, float(p))
        y = torch.where(keep, z * (1.0 if wrong == "unscaled" else float(np.float32(1.0) / (np.float32(1.0) - p))), torch.zeros_like(z))
    elif c.mode == "add":
        y = z - d if wrong else z + d
    else:
        y = z * float(np.float32(G.ELT_P["scale"])) * (1.001 if wrong else 1.0)
    return dict(out=y.to(c.out))


@pytest.mark.parametrize("c", G.CASES["eltwise"], ids=G.case_id)
def test_eltwise_standin(c):
    _passes(c, _eltwise_standin(c))


@pytest.mark.parametrize("mode,wrong", [(m, "value") for m in G.ELT_MODES if m != "dropout"] + [("dropout", "seed"), ("dropout", "unscaled")])
def test_eltwise_wrong(mode, wrong):
    for z, o in ((F32, F32), (F16, BF16)):
        c = _case("eltwise", f"{mode}-z_{G.DT_NAME[z]}-out_{G.DT_NAME[o]}-n37001")
        _fails(c, _eltwise_standin(c, wrong))


def test_dropout_interval():
    lo, hi = G.dropout_interval(1 << 20, 0.1)
    assert lo < (1 << 20) * 0.9 < hi and math.isclose(hi - lo, 10 * math.sqrt((1 << 20) * 0.09))
    kept = int(H.splitmix_keep(G.ELT_SEED, 1 << 20, 0.1).sum())
    assert lo <= kept <= hi
    assert not lo <= int(H.splitmix_keep(G.ELT_SEED, 1 << 20, 0.11).sum()) <= hi         # a 1 % slip of p is outside the interval


# ------------------------------------------------------------------------------------------------ colsum
def _colsum_standin(c, wrong=None):
    i = G.inputs(c)
    x = i["x"][:-1] if wrong == "last_row" else i["x"]
    s = x.sum(0)
    return dict(out=s if wrong == "overwrite" else i["out0"] + s)


@pytest.mark.parametrize("c", G.CASES["colsum"], ids=G.case_id)
def test_colsum_standin(c):
    _passes(c, _colsum_standin(c))


@pytest.mark.parametrize("case_id,wrong", [("rows33-cols257-pad8", "last_row"), ("rows5-cols1-pad0", "last_row"), ("rows777-cols3072-pad0", "last_row"),
                                           ("rows33-cols257-pad8", "overwrite"), ("rows9232-cols3072-pad0", "overwrite")])
def test_colsum_wrong(case_id, wrong):
    """(At 9232 rows the worst-case bound, 9235 u sum |x|, is wider than one element: the row tails are pinned by the small row counts.)"""
    c = _case("colsum", case_id)
    _fails(c, _colsum_standin(c, wrong))


# ------------------------------------------------------------------------------------------------ embed_bwd
def _embed_bwd_standin(c, wrong=None):
    i = G.inputs(c)
    rows = 3 * c.l
    touched, inv = torch.unique(i["ids"], return_inverse=True)
    dword = torch.zeros((touched.numel(), c.cols))
    if wrong == "no_accumulate":
        dword[inv] = i["dy"]
    else:
        dword.index_add_(0, inv, i["dy"])
    pos = torch.arange(rows) // 3 if wrong == "pos_div" else torch.arange(rows) % c.l
    return dict(dword=dword, dpos=torch.zeros((c.l, c.cols)).index_add_(0, pos, i["dy"]))


@pytest.mark.parametrize("c", G.CASES["embed_bwd"], ids=G.case_id)
def test_embed_bwd_standin(c):
    _passes(c, _embed_bwd_standin(c))


@pytest.mark.parametrize("case_id,wrong", [("cols768-l42-equal", "no_accumulate"), ("cols1000-l32-random", "no_accumulate"),
                                           ("cols64-l32-distinct", "pos_div"), ("cols1000-l42-equal", "pos_div")])
def test_embed_bwd_wrong(case_id, wrong):
    c = _case("embed_bwd", case_id)
    _fails(c, _embed_bwd_standin(c, wrong))
