"""Cases, the numpy restatement and the fixture loader for the device image transform (cir_preprocess_images,
candidate_reranking_cir_amd/preprocess.py).  A plain module, imported by tests/test_preprocess_cpu.py, tests/test_preprocess_gpu.py and
tools/make_preprocess_golden.py.

The restatement (`ref_transform`) is the reference's TargetPad | SquarePad -> Resize(dim, BICUBIC) -> CenterCrop(dim) on an 8-bit RGB image
(data_utils.py:23-101) written out the long way, independent of the package: the pad IS materialised, both resize passes run over the whole
image, the crop comes last, one output coordinate at a time.  The fixture tests/golden/preprocess.npz holds each case's source and the
output PIL itself gave (tools/make_preprocess_golden.py: ImageOps.expand, Image.resize(BICUBIC), crop); every comparison is bit-exact -
all the arithmetic between the source bytes and the output bytes is integer, and the float64 coefficients are rounded to 22-bit integers
by one stated rule.

Cases are (h, w, dim, ratio); ratio None = SquarePad.  1.25 is the ratio of every reference script (validate_stage2.py:327-331).
`97x41` uses 2.5: 97 / 41 = 2.37 stays under it, so there is NO pad and Resize gives int(48 * 97 / 41) = 113 rows (3 x 3 patches survive)."""
import os
from typing import NamedTuple, Optional

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess.npz")


class Case(NamedTuple):
    name: str
    h: int
    w: int
    dim: int
    ratio: Optional[float]
    source: str = "noise"          # noise | noise4 | ones (all 255) | blocks (0 / 255 blocks) | smooth


CASES = [
    Case("33x47", 33, 47, 32, 1.25),                      # no pad, landscape
    Case("47x33", 47, 33, 32, 1.25),                      # no pad, portrait
    Case("40x50", 40, 50, 32, 1.25),                      # ratio exactly 1.25: the pad branch with zero pad
    Case("20x90", 20, 90, 32, 1.25),                      # pad with int() truncation: vp = int(26.0) = 26
    Case("90x20", 90, 20, 32, 1.25),
    Case("17x23", 17, 23, 32, 1.25),                      # upscale: fs = 1
    Case("64x64", 64, 64, 64, 1.25),                      # both passes skipped
    Case("64x80", 64, 80, 64, 1.25),                      # both passes skipped, crop only (left = 8)
    Case("97x41", 97, 41, 48, 2.5),                       # int(48 * 97 / 41) = 113, 9 patches
    Case("161x333", 161, 333, 64, 1.25, "noise4"),                # general downscale
    Case("40x520sq", 40, 520, 32, None, "noise4"),                # square pad, 16.25-fold downscale, 67 taps
    Case("1x7", 1, 7, 32, 1.25),                          # one-pixel side
    Case("ones", 24, 70, 32, 1.25, "ones"),               # all 255, padded: coefficient normalisation and edge windows
    Case("blocks", 45, 61, 32, 1.25, "blocks"),           # 0 / 255 blocks: overshoot clipped at both ends
    Case("375x500@384", 375, 500, 384, 1.25, "smooth"),   # the reference's geometries (CIRR images, validate_stage2.py:327-331)
    Case("375x500@224", 375, 500, 224, 1.25, "smooth"),
]


def case_id(c: Case) -> str:
    return c.name


def source_key(c: Case) -> str:
    """Fixture key of a case's source (the two 375 x 500 cases share one)."""
    return f"{c.source}_{c.h}x{c.w}_src"


def make_source(c: Case) -> np.ndarray:
    """The (h, w, 3) uint8 source of a case (what the generator stores in the fixture)."""
    if c.source == "ones":
        return np.full((c.h, c.w, 3), 255, dtype=np.uint8)
    if c.source == "blocks":
        y, x = np.mgrid[0:c.h, 0:c.w]
        a = (((y // 5) + (x // 7)) % 2 * 255).astype(np.uint8)
        return np.stack([a, 255 - a, np.roll(a, 3, axis=1)], axis=2)
    if c.source == "smooth":      # flat blocks on an irregular grid: resampled runs and rows repeat, so the 384-px fixture compresses
        rs = np.random.RandomState(375500)
        ys, xs = [0, 30, 70, 75, 140, 200, 260, 330, c.h], [0, 41, 90, 97, 160, 230, 301, 340, 420, 470, c.w]
        img = np.empty((c.h, c.w, 3), dtype=np.uint8)
        for y0, y1 in zip(ys[:-1], ys[1:]):
            for x0, x1 in zip(xs[:-1], xs[1:]):
                img[y0:y1, x0:x1] = rs.randint(0, 256, size=3)
        return img
    seed = (c.h * 1000003 + c.w * 1009) % (1 << 31)
    if c.source == "noise4":      # four levels only (the two large noise sources: a quarter of the entropy in the fixture)
        return (np.random.RandomState(seed).randint(0, 4, size=(c.h, c.w, 3)) * 85).astype(np.uint8)
    return np.random.RandomState(seed).randint(0, 256, size=(c.h, c.w, 3)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the restatement
def ref_geometry(h, w, dim, ratio):
    """(hp, vp, rw, rh, left, top): data_utils.py:36-42 / 59-68, torchvision's Resize(int) and CenterCrop."""
    big = max(w, h)
    if ratio is None:
        hp, vp = int((big - w) / 2), int((big - h) / 2)
    elif big / min(w, h) < ratio:
        hp, vp = 0, 0
    else:
        s = big / ratio
        hp, vp = max(int((s - w) / 2), 0), max(int((s - h) / 2), 0)
    pw, ph = w + 2 * hp, h + 2 * vp
    if pw <= ph:
        rw, rh = dim, int(dim * ph / pw)
    else:
        rw, rh = int(dim * pw / ph), dim
    return hp, vp, rw, rh, int(round((rw - dim) / 2.0)), int(round((rh - dim) / 2.0))


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def ref_coeffs(n_in, n_out):
    """libImaging's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter: [(xmin, [kk ...])] per output, Python floats."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        ws = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in ws:
            ww += v
        if ww != 0.0:
            ws = [v / ww for v in ws]
        out.append((xmin, [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in ws]))
    return out


def ref_pass(img, n_out, axis):
    """One resize pass of an (H, W, 3) uint8 image along `axis` (1 = horizontal), uint8 out; PIL skips a pass that keeps the extent."""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i, (xmin, kk) in enumerate(ref_coeffs(n_in, n_out)):
        acc = (1 << 21) + np.tensordot(np.asarray(kk, dtype=np.int64), src[xmin:xmin + len(kk)], axes=(0, 0))
        assert np.abs(acc).max() < (1 << 31)                              # int32 throughout in libImaging: no wrap to reproduce
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def ref_transform(src, dim, ratio):
    """(dim, dim, 3) uint8: pad -> horizontal pass -> vertical pass -> centre crop."""
    h, w = src.shape[:2]
    hp, vp, rw, rh, left, top = ref_geometry(h, w, dim, ratio)
    img = np.pad(src, ((vp, vp), (hp, hp), (0, 0)))
    img = ref_pass(ref_pass(img, rw, 1), rh, 0)
    return np.ascontiguousarray(img[top:top + dim, left:left + dim])


# ------------------------------------------------------------------------------------------------ the fixture
_FIXTURE = None


def fixture():
    """{case name: (source (h, w, 3) uint8, PIL's output (dim, dim, 3) uint8)}, loaded once."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(GOLDEN) as z:
            _FIXTURE = {c.name: (z[source_key(c)], z[c.name + "_out"]) for c in CASES}
        for a, b in _FIXTURE.values():
            a.setflags(write=False)
            b.setflags(write=False)
    return _FIXTURE
