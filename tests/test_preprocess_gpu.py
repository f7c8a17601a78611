"""The device image transform on a real MI355X (cir_preprocess_images, candidate_reranking_cir_amd/preprocess.py): every output layout
bit for bit against the PIL-made fixture of tests/preprocess_cases.py (needs neither PIL nor the reference), independence of the batch
position, canary guard bands around all three layouts, and the model entry points against the existing ones on the host-side tensor."""
import numpy as np
import pytest
import torch

from tests import preprocess_cases as P

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
CANARY = {torch.float32: 0x7FC0DEAD, torch.bfloat16: 0x7FC1, torch.float16: 0x7E01, torch.uint8: 0xA5}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.uint8: torch.uint8}


def _t(a):
    return torch.from_numpy(np.array(a))                      # (a copy: the fixture's arrays are read-only)


class _Rt:
    def __init__(self):
        from candidate_reranking_cir_amd import ops, preprocess
        self.ops, self.PP = ops, preprocess
        self.table = preprocess.value_table()                 # fp32, CPU: test_preprocess_cpu.py pins it to torch's ToTensor + Normalize
        self._tr = {}

    def transform(self, dim, ratio):
        key = (dim, ratio)
        if key not in self._tr:
            self._tr[key] = self.PP.DeviceTransform(dim, ratio, "cuda")
        return self._tr[key]

    def normalised(self, u8, dtype=torch.float32):
        """(dim, dim, 3) uint8 -> (3, dim, dim): the value table (in `dtype`) applied to an image."""
        idx = _t(u8).long().permute(2, 0, 1) + 256 * torch.arange(3)[:, None, None]
        return self.table.to(dtype)[idx]


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _Rt()


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_raw_and_fp32_outputs_equal_the_fixture(rt, c):
    src, want = P.fixture()[c.name]
    tr = rt.transform(c.dim, c.ratio)
    raw = tr.batch([src], raw=True)
    assert raw.dtype == torch.uint8 and tuple(raw.shape) == (1, c.dim, c.dim, 3)
    assert torch.equal(raw[0].cpu(), _t(want))
    chw = tr.batch([src])
    assert chw.dtype == torch.float32 and torch.equal(chw[0].cpu(), rt.normalised(want))
    assert torch.equal(tr(src), chw[0])                                   # the reference's preprocess(img) call form


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_patch_rows_and_16bit_outputs(rt, dtype):
    for c in P.CASES:
        src, want = P.fixture()[c.name]
        tr = rt.transform(c.dim, c.ratio)
        chw32 = tr.batch([src])
        rows = tr.batch([src], patches=True, dtype=dtype)
        assert rows.dtype == dtype and tuple(rows.shape) == ((c.dim // 16) ** 2, 768)
        assert torch.equal(rows, rt.ops.patchify(chw32, 16, dtype)), c.name
        assert torch.equal(tr.batch([src], dtype=dtype)[0].cpu(), rt.normalised(want, dtype)), c.name


@pytest.mark.parametrize("dim", [32, 64])
def test_mixed_batch_equals_single_launches(rt, dim):
    """All sources of the cases of one dim in ONE launch (sizes from 1 x 7 to 40 x 520 under one TargetPad transform): every image equals
    its single-image launch, wherever it sits in the batch - and the fixture where the case's own transform is this one."""
    cases = [c for c in P.CASES if c.dim == dim]
    srcs = [P.fixture()[c.name][0] for c in cases]
    tr = rt.transform(dim, 1.25)
    single = [tr.batch([s], raw=True)[0] for s in srcs]
    for order in (list(range(len(cases))), list(reversed(range(len(cases))))):
        got = tr.batch([srcs[i] for i in order], raw=True)
        rows = tr.batch([srcs[i] for i in order], patches=True, dtype=torch.bfloat16).view(len(order), -1, 768)
        for pos, i in enumerate(order):
            assert torch.equal(got[pos], single[i]), (cases[i].name, pos)
            assert torch.equal(rows[pos], tr.batch([srcs[i]], patches=True, dtype=torch.bfloat16)), (cases[i].name, pos)
            if cases[i].ratio == 1.25:
                assert torch.equal(got[pos].cpu(), _t(P.fixture()[cases[i].name][1])), cases[i].name


def _guarded(shape, dtype, slack=4096):
    n = int(np.prod(shape))
    big = torch.empty(n + 2 * slack, dtype=dtype, device="cuda")
    big.view(_INT[dtype]).fill_(CANARY[dtype])
    return big, big[slack:slack + n].view(shape)


def _assert_intact(big, n, dtype, slack=4096, what=""):
    bits = big.view(_INT[dtype])
    outside = torch.cat([bits[:slack], bits[slack + n:]])
    bad = outside != CANARY[dtype]
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} canary elements overwritten"
    assert bool((bits[slack:slack + n] != CANARY[dtype]).any())


@pytest.mark.parametrize("layout,dim,dtype", [("raw", 40, torch.uint8), ("chw", 40, torch.float32), ("chw", 40, torch.bfloat16),
                                              ("patches", 48, torch.bfloat16), ("patches", 48, torch.float32)],
                         ids=["raw40", "chw40-fp32", "chw40-bf16", "patches48-bf16", "patches48-fp32"])
def test_guard_bands(rt, layout, dim, dtype):
    """Outputs inside canary-filled allocations: a ragged last band (40 = 2.5 bands of 16 rows) and a ragged column chunk (40, 48 < 64),
    three images of different sizes; the values against the restatement (no fixture exists at these sizes)."""
    names = ["33x47", "97x41", "161x333"]
    srcs = [P.fixture()[n][0] for n in names]
    want = [P.ref_transform(s, dim, 1.25) for s in srcs]
    tr = rt.transform(dim, 1.25)
    shape = {"raw": (3, dim, dim, 3), "chw": (3, 3, dim, dim), "patches": (3 * (dim // 16) ** 2, 768)}[layout]
    big, view = _guarded(shape, dtype)
    out = tr.batch(srcs, patches=layout == "patches", raw=layout == "raw", dtype=dtype, out=view)
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    _assert_intact(big, view.numel(), dtype, what=layout)
    if layout == "raw":
        assert torch.equal(view.cpu(), _t(np.stack(want)))
    else:
        chw = torch.stack([rt.normalised(w, dtype) for w in want])
        if layout == "chw":
            assert torch.equal(view.cpu(), chw)
        else:
            g = dim // 16
            rows = chw.view(3, 3, g, 16, g, 16).permute(0, 2, 4, 1, 3, 5).reshape(3 * g * g, 768)      # (b, py, px | c, ky, kx)
            assert torch.equal(view.cpu(), rows)


def test_windows_wider_than_the_stage(rt):
    """8 x 2100 square-padded to 32 px is a 65.6-fold downscale: a column's window is 263 source pixels, the 32 columns span 6300 bytes of a
    source row - more than the kernel's 3072-byte LDS stage, so the right-hand columns read their pixels from global memory while the
    left-hand ones read the stage, and both coefficient sets overflow their register / LDS copies.  Against the restatement."""
    src = np.random.RandomState(2100).randint(0, 256, size=(8, 2100, 3)).astype(np.uint8)
    want = P.ref_transform(src, 32, None)
    assert int(want.max()) > int(want.min())
    got = rt.transform(32, None).batch([src, src[:, ::-1].copy()], raw=True)
    assert torch.equal(got[0].cpu(), _t(want))
    assert torch.equal(got[1].cpu(), _t(P.ref_transform(src[:, ::-1], 32, None)))


# ------------------------------------------------------------------------------------------------ model entry points
@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import config, synthetic, weights
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    from candidate_reranking_cir_amd.preprocess import targetpad_transform
    g = config.BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=8, intermediate_size=256, encoder_width=128)
    v = config.VitGeometry(image_size=64, width=128, depth=2, num_heads=2)
    m2 = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m2.load_state_dict(weights.synth_state_dict(weights.nlvr_param_spec(g, v), 3, "spread"))
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m1.load_state_dict(weights.synth_state_dict(weights.retrieval_param_spec(g, v), 4, "spread"))
    images = [P.fixture()[n][0] for n in ("33x47", "47x33", "97x41", "161x333", "64x80", "1x7", "20x90")]
    return m2.to("cuda").eval(), m1.to("cuda").eval(), targetpad_transform(1.25, 64), images


def test_img_embed_raw_equals_img_embed(tiny):
    m2, m1, tr, images = tiny
    chw = tr.batch(images)
    assert tuple(chw.shape) == (len(images), 3, 64, 64) and chw.dtype == torch.float32
    want = m2.img_embed(chw)
    got, atts = m2.img_embed_raw(images, tr, atts=True)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and tuple(atts.shape) == tuple(got.shape[:2])
    assert float((want[0] - want[1]).abs().max()) > 0                    # the images differ, and so do their tokens
    w_tok, w_pool = m1.img_embed(chw, return_pool_and_normalized=True)
    g_tok, g_pool = m1.img_embed_raw(images, tr, return_pool_and_normalized=True)
    assert torch.equal(g_tok, w_tok) and torch.equal(g_pool, w_pool)
    assert torch.equal(m1.img_embed_raw(images, tr), w_tok)


def test_extract_index_features_raw_equal_the_existing_functions(tiny):
    from candidate_reranking_cir_amd import validate, validate_stage2
    m2, m1, tr, images = tiny
    chw = tr.batch(images)
    for dtype in (None, torch.float32):
        want = validate_stage2.extract_index_features(chw, m2, batch_size=3, dtype=dtype)
        got = validate_stage2.extract_index_features_raw(images, m2, tr, batch_size=3, dtype=dtype)
        assert got.dtype == want.dtype and torch.equal(got, want)
    w_tok, w_pool = validate.extract_index_features(chw, m1, batch_size=3)
    g_tok, g_pool = validate.extract_index_features_raw(images, m1, tr, batch_size=3)
    assert g_tok.dtype == w_tok.dtype and torch.equal(g_tok, w_tok) and torch.equal(g_pool, w_pool)
