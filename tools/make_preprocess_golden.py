"""Writes tests/golden/preprocess.npz: for every case of tests/preprocess_cases.py the uint8 source and the output PIL gives for the
reference's transform up to the crop (data_utils.py:23-101: pad -> Resize(dim, BICUBIC) -> CenterCrop(dim)).  The only file of the project
that imports PIL; the tests read the fixture and need neither PIL nor torchvision.

    python tools/make_preprocess_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import preprocess_cases as P  # noqa: E402


def pil_transform(src: np.ndarray, dim: int, ratio) -> np.ndarray:
    h, w = src.shape[:2]
    hp, vp, rw, rh, left, top = P.ref_geometry(h, w, dim, ratio)
    img = Image.fromarray(src, "RGB")
    if hp or vp:
        img = ImageOps.expand(img, border=(hp, vp, hp, vp), fill=0)
    if img.size != (rw, rh):                                  # torchvision's Resize returns the image itself when the size is kept
        img = img.resize((rw, rh), Image.BICUBIC)
    return np.asarray(img.crop((left, top, left + dim, top + dim)))


def main():
    out = {}
    for c in P.CASES:
        src = P.make_source(c)
        out[P.source_key(c)], out[c.name + "_out"] = src, pil_transform(src, c.dim, c.ratio)
    np.savez_compressed(P.GOLDEN, **out)
    print(f"{P.GOLDEN}: {len(P.CASES)} cases, {os.path.getsize(P.GOLDEN)} bytes (PIL {Image.__version__})")


if __name__ == "__main__":
    main()
