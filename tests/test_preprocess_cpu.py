"""Host side of the device image transform (candidate_reranking_cir_amd/preprocess.py, cir_preprocess_images), without a GPU: the
geometry and the coefficient tables against hand-derived values, the numpy restatement against the PIL-made fixture (and against PIL run
live where it is installed), the value table against torch's own fp32 ops, the entry point's argument errors, and the `patches=` keyword of
VitEngine.forward on recording stubs."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import preprocess_cases as P
from tests.engine_stub import StubOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (hp, vp, rw, rh, left, top) by hand from data_utils.py:36-42 / 59-68, Resize(int) and CenterCrop
GEOMETRY = {
    "33x47": (0, 2, 40, 32, 4, 0),            # 47/33 = 1.42 >= 1.25: s = 37.6, hp = max(int(-4.7), 0) = 0, vp = int(2.3) = 2 -> 37 x 47; rw = int(32 * 47 / 37) = int(40.6)
    "47x33": (2, 0, 32, 40, 0, 4),
    "40x50": (0, 0, 40, 32, 4, 0),            # 50/40 = 1.25 is NOT < 1.25: pad branch, s = 40, hp = max(int(-5.0), 0) = 0, vp = int(0.0) = 0
    "20x90": (0, 26, 40, 32, 4, 0),           # s = 72, vp = int(26.0) = 26 -> 72 x 90 padded; rw = int(32 * 90 / 72) = 40
    "90x20": (26, 0, 32, 40, 0, 4),
    "17x23": (0, 0, 43, 32, 6, 0),            # 23/17 = 1.35: s = 18.4, vp = int(0.7) = 0; rw = int(32 * 23 / 17) = int(43.29) = 43; left = round(5.5) = 6
    "64x64": (0, 0, 64, 64, 0, 0),
    "64x80": (0, 0, 80, 64, 8, 0),            # 80/64 = 1.25: s = 64, no pad
    "97x41": (0, 0, 48, 113, 0, 32),          # ratio 2.5: no pad; rh = int(48 * 97 / 41) = int(113.56); top = round(32.5) = 32 (ties to even)
    "161x333": (0, 52, 80, 64, 8, 0),         # s = 266.4, vp = int(52.7) = 52 -> 265 x 333; rw = int(64 * 333 / 265) = int(80.4)
    "40x520sq": (0, 240, 32, 32, 0, 0),       # square pad: vp = int(480 / 2)
    "1x7": (0, 2, 44, 32, 6, 0),              # s = 5.6, vp = int(2.3) = 2 -> 5 x 7; rw = int(32 * 7 / 5) = 44
    "ones": (0, 16, 40, 32, 4, 0),            # 24 x 70: s = 56, vp = 16 -> 56 x 70; rw = 40
    "blocks": (0, 1, 41, 32, 4, 0),           # 45 x 61: s = 48.8, vp = int(1.9) = 1 -> 47 x 61; rw = int(41.53); left = round(4.5) = 4
    "375x500@384": (0, 12, 481, 384, 48, 0),  # s = 400, vp = int(12.5) = 12 -> 399 x 500; rw = int(384 * 500 / 399) = int(481.2); left = round(48.5) = 48
    "375x500@224": (0, 12, 280, 224, 28, 0),  # rw = int(224 * 500 / 399) = int(280.7)
}


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_geometry_by_hand(c):
    from candidate_reranking_cir_amd import preprocess as PP
    assert PP.geometry(c.h, c.w, c.dim, c.ratio) == GEOMETRY[c.name]
    assert P.ref_geometry(c.h, c.w, c.dim, c.ratio) == GEOMETRY[c.name]


def test_geometry_refuses_empty_images():
    from candidate_reranking_cir_amd import preprocess as PP
    for bad in ((0, 4, 32), (4, 0, 32), (4, 4, 0)):
        with pytest.raises(ValueError):
            PP.geometry(*bad)


def _fix(fr):
    """libImaging's rounding of an exact coefficient: (int)(w 2^22 +- 0.5), truncation toward zero."""
    v = fr * (1 << 22)
    return int(v + Fraction(1, 2)) if fr >= 0 else -int(-v + Fraction(1, 2))


def test_resample_taps_by_hand():
    from candidate_reranking_cir_amd import preprocess as PP
    # 4 -> 2: scale 2 = fs, support 4.  Output 0: center 1, window [max(int(-2.5), 0), min(int(5.5), 4)) = [0, 4), arguments
    # (x - 0.5) / 2 = -0.25, 0.25, 0.75, 1.25 -> bicubic 111/128, 111/128, 29/128, -9/128 (a = -0.5), sum 242/128.  Output 1 mirrors it.
    want = [Fraction(111, 242), Fraction(111, 242), Fraction(29, 242), Fraction(-9, 242)]
    t = PP.resample_taps(4, 2)
    assert t.dtype == np.int32 and t.shape == (2, 6)
    assert t[0].tolist() == [0, 4] + [_fix(f) for f in want]
    assert t[1].tolist() == [0, 4] + [_fix(f) for f in reversed(want)]
    assert abs(int(t[0, 2:].sum()) - (1 << 22)) <= 2                      # rounded one by one: the sum may miss 2^22 by a unit or two
    # 2 -> 4 (upscale: fs = 1, support 2).  Output 0: center 0.25, window [max(int(-1.25), 0), min(int(2.75), 2)) = [0, 2), arguments
    # 0.25, 1.25 -> 111/128, -9/128 -> normalised 111/102, -9/102
    u = PP.resample_taps(2, 4)
    assert u[0].tolist()[:4] == [0, 2, _fix(Fraction(111, 102)), _fix(Fraction(-9, 102))]
    # a pass PIL skips: the identity in the kernel's arithmetic, for the surviving window only
    assert PP.resample_taps(80, 80, 8, 64).tolist() == [[x, 1, 1 << 22] for x in range(8, 72)]
    # the 16.25-fold downscale of the square-padded case: support 32.5, libImaging allocates ksize = 2 ceil(32.5) + 1 = 67 per output; a
    # window is [int(c - 32), int(c + 33)) with c = 8.125 + 16.25 i: 65 taps inside the image, int(41.125) = 41 for output 0
    big = PP.resample_taps(520, 32)
    assert big.shape == (32, 2 + 65) and int(big[:, 1].max()) == 65 and big[0, :2].tolist() == [0, 41] and big[5, :2].tolist() == [57, 65]
    # a window is the rows of the whole table
    assert np.array_equal(PP.resample_taps(500, 481, 48, 384), PP.resample_taps(500, 481)[48:48 + 384])
    with pytest.raises(ValueError):
        PP.resample_taps(10, 4, 2, 3)


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_resample_taps_equal_the_restatements_coefficients(c):
    """Two statements of precompute_coeffs - the package's vectorised one and the scalar one of the restatement - give the same integers."""
    from candidate_reranking_cir_amd import preprocess as PP
    hp, vp, rw, rh, left, top = GEOMETRY[c.name]
    for n_in, n_out, first in ((c.w + 2 * hp, rw, left), (c.h + 2 * vp, rh, top)):
        if n_in == n_out:
            continue
        t = PP.resample_taps(n_in, n_out, first, c.dim)
        ref = P.ref_coeffs(n_in, n_out)[first:first + c.dim]
        for row, (xmin, kk) in zip(t, ref):
            assert row[0] == xmin and row[1] == len(kk) and row[2:2 + len(kk)].tolist() == kk and not row[2 + len(kk):].any()
            assert sum(abs(k) for k in kk) * 255 < (1 << 31)               # int32 is enough, as in PIL


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_restatement_equals_fixture(c):
    src, want = P.fixture()[c.name]
    assert np.array_equal(src, P.make_source(c))                           # the fixture's sources are the generator's
    assert want.shape == (c.dim, c.dim, 3) and want.dtype == np.uint8
    assert np.array_equal(P.ref_transform(src, c.dim, c.ratio), want)


def test_fixture_is_small():
    assert os.path.getsize(P.GOLDEN) < 300 * 1024


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_restatement_equals_pil_live(c):
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_preprocess_golden", os.path.join(ROOT, "tools", "make_preprocess_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    src = P.fixture()[c.name][0]
    assert np.array_equal(P.ref_transform(src, c.dim, c.ratio), gen.pil_transform(src, c.dim, c.ratio))


def test_value_table():
    from candidate_reranking_cir_amd import preprocess as PP
    u8 = torch.arange(256, dtype=torch.uint8)
    mean = torch.tensor((0.48145466, 0.4578275, 0.40821073), dtype=torch.float32)      # data_utils.py:83 / :100
    std = torch.tensor((0.26862954, 0.26130258, 0.27577711), dtype=torch.float32)
    want = ((u8.to(torch.float32).div(255)[None, :] - mean[:, None]) / std[:, None]).reshape(768)     # ToTensor, Normalize
    t = PP.value_table()
    assert t.dtype == torch.float32 and torch.equal(t, want)
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(PP.value_table(dt), want.to(dt))


def test_pack_layout():
    """Descriptors, shared tap tables and 16-byte aligned pixels in one buffer; two images of one size share their tables."""
    from candidate_reranking_cir_amd import preprocess as PP
    fx = P.fixture()
    imgs = [fx["33x47"][0], fx["47x33"][0], torch.from_numpy(fx["33x47"][0].copy())]
    tr = PP.DeviceTransform(32, 1.25, device="cpu")
    buf, o_desc, o_taps, n_taps, o_pix, n_pix = tr.pack(imgs)
    assert o_desc % 16 == 0 and o_taps % 16 == 0 and o_pix % 16 == 0 and buf.size == o_pix + n_pix
    desc = buf[o_desc:o_desc + 3 * 64].view(np.int32).reshape(3, 16)
    taps = buf[o_taps:o_taps + 4 * n_taps].view(np.int32)
    assert desc[0].tolist()[1:9] == [33, 47, 0, 2, 47, 37, 4, 0] and desc[0].tolist()[13:] == [40, 32, 0]
    assert desc[2].tolist()[1:] == desc[0].tolist()[1:] and desc[2, 0] != desc[0, 0]
    for i, im in enumerate(imgs):
        a = np.asarray(im)
        s = o_pix + int(desc[i, 0]) * 16
        assert np.array_equal(buf[s:s + a.size], a.reshape(-1))
        off, stride = int(desc[i, 9]), int(desc[i, 10])
        hp, left, rw = int(desc[i, 3]), int(desc[i, 7]), int(desc[i, 13])
        assert np.array_equal(taps[off:off + 32 * stride].reshape(32, stride), PP.resample_taps(a.shape[1] + 2 * hp, rw, left, 32))
    with pytest.raises(ValueError):
        tr.pack([np.zeros((4, 4), dtype=np.uint8)])
    with pytest.raises(ValueError):
        tr.pack([np.zeros((4, 4, 3), dtype=np.float32)])


def test_pil_images_by_duck_typing():
    from candidate_reranking_cir_amd import preprocess as PP

    class FakePil:
        def __init__(self, a): self.a = a
        def convert(self, mode):
            assert mode == "RGB"
            return self.a                     # (np.asarray of a PIL image is its (h, w, 3) array)

    a = P.fixture()["17x23"][0]
    assert np.array_equal(PP.as_rgb_array(FakePil(a)), a)
    # the module imports neither PIL nor torchvision, at any level
    src = open(os.path.join(ROOT, "candidate_reranking_cir_amd", "preprocess.py")).read()
    imports = [ln.strip() for ln in src.splitlines() if ln.strip().startswith(("import ", "from "))]
    assert imports and not [ln for ln in imports if "PIL" in ln or "torchvision" in ln]


def test_argument_errors_before_any_launch():
    """Fake, never dereferenced addresses stand in for device pointers, as in test_abi.py."""
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
    P16 = 0x10000
    CHW, PATCHES, RAW = 0, 1, 2
    names = ["src", "src_bytes", "desc", "taps", "taps_len", "table", "out", "B", "dim", "layout", "dtype", "stream"]
    ok = dict(src=P16, src_bytes=4096, desc=P16, taps=P16, taps_len=64, table=P16, out=P16, B=1, dim=32, layout=CHW, dtype=lib.CIR_F32, stream=None)
    call = lambda **o: c.cir_preprocess_images(*[{**ok, **o}[k] for k in names])       # (the valid list itself is never passed: it would launch)
    for p in ("src", "desc", "taps", "table", "out"):
        assert call(**{p: None}) == EINVAL, p
    assert call(B=0) == EINVAL and call(dim=0) == EINVAL and call(dim=-16) == EINVAL and call(src_bytes=0) == EINVAL and call(taps_len=0) == EINVAL
    assert call(layout=3) == EINVAL and call(layout=-1) == EINVAL
    assert call(dtype=3) == EDTYPE and call(dtype=-1) == EDTYPE and call(layout=PATCHES, dtype=7) == EDTYPE
    assert call(layout=PATCHES, dim=40) == ESHAPE and call(dim=8192) == ESHAPE
    assert call(B=1 << 30, dim=4096) == ESHAPE                                           # one-dimensional grid
    for p in ("src", "desc", "taps", "table", "out"):
        assert call(**{p: P16 + 4}) == EALIGN, p
    assert call(layout=RAW, out=P16 + 8, table=None) == EALIGN                           # the raw layout takes no table, but an aligned output


# ------------------------------------------------------------------------------------------------ VitEngine.forward(patches=...)
class VitStubOps(StubOps):
    """engine_stub.StubOps plus the three ops only the ViT calls."""

    def patchify(self, image, patch, dtype16=torch.bfloat16):
        args = dict(locals()); del args["self"]
        b, ch, h, w = image.shape
        return self._record("patchify", args, torch.empty((b * (h // patch) * (w // patch), ch * patch * patch), dtype=dtype16))

    def vit_assemble(self, proj, cls, pos, batch):
        args = dict(locals()); del args["self"]
        return self._record("vit_assemble", args, torch.empty((batch, proj.shape[0] // batch + 1, proj.shape[1]), dtype=proj.dtype))

    def layernorm(self, x, gamma, beta, eps, residual=None, want32=True, dtype16=None, stream_dtype=torch.float32, out32=None, out16=None):
        args = dict(locals()); del args["self"]
        y32 = (out32 if out32 is not None else torch.empty(x.shape, dtype=stream_dtype)) if want32 else None
        y16 = (out16 if out16 is not None else torch.empty(x.shape, dtype=dtype16)) if dtype16 is not None else None
        return self._record("layernorm", args, (y32, y16))


def _vit_engine():
    from candidate_reranking_cir_amd import engine as E
    from candidate_reranking_cir_amd import weights
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    geo = BertGeometry(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256, encoder_width=128)
    vit = VitGeometry(image_size=64, patch_size=16, width=128, depth=2, num_heads=2)
    sd = weights.synth_state_dict(weights.nlvr_param_spec(geo, vit), 1)
    return E.VitEngine(sd, vit, torch.bfloat16, torch.device("cpu")), vit


def _trace(eng, monkeypatch, **kw):
    from candidate_reranking_cir_amd import engine as E
    stub = VitStubOps()
    monkeypatch.setattr(E, "ops", stub)
    y32, y16 = eng.forward(want32=True, **kw)
    return stub.trace, y32, y16


def test_patches_keyword_skips_only_the_patchify_launch(monkeypatch):
    eng, geo = _vit_engine()
    p = geo.num_tokens - 1
    base, y32, y16 = _trace(eng, monkeypatch, image=torch.zeros((3, 3, 64, 64)))
    assert [t[0] for t in base].count("patchify") == 1 and base[0][0] == "patchify"
    assert tuple(y32.shape) == (3, geo.num_tokens, 128) and y16.dtype == torch.bfloat16
    rows = torch.zeros((3 * p, 768), dtype=torch.bfloat16)
    direct, z32, z16 = _trace(eng, monkeypatch, image=None, patches=rows)
    assert "patchify" not in [t[0] for t in direct] and z32.shape == y32.shape and z16.shape == y16.shape
    # every other launch is the same launch: same ops in the same order on the same shapes, strides and types (the first GEMM reads the
    # caller's rows where it read patchify's result: both are the first storage the trace meets)
    assert [t[0] for t in direct] == [t[0] for t in base[1:]]
    strip = lambda tr: [(name, tuple((k, v[:5] if isinstance(v, tuple) and v and v[0] == "tensor" else v) for k, v in args)) for name, args, _ in tr]
    assert strip(direct) == strip(base[1:])
    # chunked: the same chunk boundaries as the image path, still no patchify
    chunked, _, _ = _trace(eng, monkeypatch, image=None, patches=rows, chunk=2)
    by_image, _, _ = _trace(eng, monkeypatch, image=torch.zeros((3, 3, 64, 64)), chunk=2)
    assert [t[0] for t in chunked] == [t[0] for t in by_image if t[0] != "patchify"] and [t[0] for t in by_image].count("patchify") == 2
    for bad in (torch.zeros((3 * p, 768)), torch.zeros((3 * p + 1, 768), dtype=torch.bfloat16), torch.zeros((3 * p, 512), dtype=torch.bfloat16)):
        with pytest.raises(ValueError):
            eng.forward(None, patches=bad)


def test_forward_without_patches_is_unchanged(monkeypatch):
    """The default (patches=None) issues patchify first and then exactly the launches it always did (positional call form included)."""
    eng, geo = _vit_engine()
    from candidate_reranking_cir_amd import engine as E
    stub = VitStubOps()
    monkeypatch.setattr(E, "ops", stub)
    eng.forward(torch.zeros((2, 3, 64, 64)), True)
    names = [t[0] for t in stub.trace]
    assert names[:3] == ["patchify", "gemm", "vit_assemble"] and names.count("attention") == geo.depth and names[-1] == "layernorm"
    with pytest.raises(ValueError, match="image size"):
        eng.forward(torch.zeros((2, 3, 32, 32)))
