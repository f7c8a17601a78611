"""The reference's image transforms on the device (data_utils.py:23-101): TargetPad | SquarePad -> Resize(dim, BICUBIC) -> CenterCrop(dim)
-> ToTensor -> Normalize, from decoded uint8 RGB images of any sizes, one cir_preprocess_images launch per batch (csrc/preprocess.hip).

The host side is geometry and coefficient tables only; every pixel is computed by the kernel, bit for bit as PIL's 8-bit resize does:

1. Pad (never materialised).  TargetPad (data_utils.py:59-68): `max(w,h)/min(w,h) < ratio` (Python float division) -> no pad; otherwise
   `s = max(w,h)/ratio`, `hp = max(int((s-w)/2), 0)`, `vp = max(int((s-h)/2), 0)`.  SquarePad (:36-42): `hp = int((max-w)/2)`,
   `vp = int((max-h)/2)`.  Zeros, hp left and right, vp top and bottom.
2. Resize(dim, BICUBIC) on a PIL image: torchvision's rule - the shorter padded side becomes dim, the longer `int(dim * long / short)`, ties
   `w <= h` -> the width is the short side - then PIL's Image.resize: horizontal pass (skipped when the width does not change), uint8
   intermediate, vertical pass (skipped likewise).  One pass n_in -> n_out in float64 as libImaging's precompute_coeffs (`resample_taps`).
3. CenterCrop(dim): `top = int(round((rh-dim)/2.0))`, `left = int(round((rw-dim)/2.0))` (Python's round).  Only surviving rows / columns
   get a table row.
4. ToTensor + Normalize (data_utils.py:82-83 / 99-100): a 768-entry table built with torch's own CPU fp32 ops (`value_table`).

No PIL or torchvision import: a PIL image is taken by duck typing (`np.asarray(img.convert("RGB"))`).  DataLoader workers cannot open the
GPU, so the transform is a batch-level call on the model side (`DeviceTransform.batch`), not a per-item one: a dataset hands out raw arrays.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from . import ops

MEAN = (0.48145466, 0.4578275, 0.40821073)            # data_utils.py:83 / :100
STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22                                   # libImaging Resample.c: 32 - 8 - 2
DESC_INTS = 16
LAYOUT_CHW, LAYOUT_PATCHES, LAYOUT_RAW = 0, 1, 2


def geometry(h: int, w: int, dim: int, target_ratio: Optional[float] = None):
    """(hp, vp, rw, rh, left, top) for an (h, w) image: the pad (target_ratio None = SquarePad), the size Resize(dim) gives the padded
    image and the offsets of CenterCrop(dim) in it."""
    h, w, dim = int(h), int(w), int(dim)
    if h <= 0 or w <= 0 or dim <= 0:
        raise ValueError(f"non-positive extent: image {h} x {w}, dim {dim}")
    big = max(w, h)
    if target_ratio is None:                                              # SquarePad, data_utils.py:36-42
        hp, vp = int((big - w) / 2), int((big - h) / 2)
    elif big / min(w, h) < target_ratio:                                  # TargetPad, data_utils.py:59-68
        hp = vp = 0
    else:
        s = big / target_ratio
        hp, vp = max(int((s - w) / 2), 0), max(int((s - h) / 2), 0)
    pw, ph = w + 2 * hp, h + 2 * vp
    if pw <= ph:                                                          # torchvision Resize(int): the short side becomes dim
        rw, rh = dim, int(dim * ph / pw)
    else:
        rw, rh = int(dim * pw / ph), dim
    top, left = int(round((rh - dim) / 2.0)), int(round((rw - dim) / 2.0))   # torchvision center_crop
    return hp, vp, rw, rh, left, top


def _bicubic(x: np.ndarray) -> np.ndarray:
    """libImaging's bicubic_filter (a = -0.5), operation for operation in float64."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


_TAPS = {}


def resample_taps(n_in: int, n_out: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
    """The int32 tap table of one resize pass n_in -> n_out for the outputs [first, first + count): (count, 2 + kmax) rows
    {xmin, taps, kk[0 .. taps), 0 ..}.  libImaging's precompute_coeffs + normalize_coeffs_8bpc in float64:
        scale = n_in / n_out, fs = max(scale, 1.0), support = 2.0 * fs
        center = (i + 0.5) * scale;  xmin = max(int(center - support + 0.5), 0);  xmax = min(int(center + support + 0.5), n_in)
        w_x = bicubic((x + xmin - center + 0.5) * (1.0 / fs)),  x in [0, xmax - xmin)      (libImaging multiplies by the reciprocal)
        normalised by the sum taken in index order;  kk = (int)(w * 2^22 +- 0.5)  (+ for w >= 0, - for w < 0; truncation toward zero)
    n_in == n_out is the pass PIL skips: {x, 1, 1 << 22} - the identity in the kernel's arithmetic.  Cached per argument tuple."""
    count = n_out - first if count is None else count
    key = (int(n_in), int(n_out), int(first), int(count))
    hit = _TAPS.get(key)
    if hit is not None:
        return hit
    n_in, n_out, first, count = key
    if n_in <= 0 or n_out <= 0 or first < 0 or count <= 0 or first + count > n_out:
        raise ValueError(f"resample_taps{key}: empty or out-of-range window")
    if n_in == n_out:
        t = np.empty((count, 3), dtype=np.int32)
        t[:, 0] = np.arange(first, first + count)
        t[:, 1] = 1
        t[:, 2] = 1 << PRECISION_BITS
    else:
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = 2.0 * fs
        ss = 1.0 / fs
        center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
        xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
        xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
        n = xmax - xmin
        kmax = int(n.max())
        x = np.arange(kmax, dtype=np.int64)[None, :]
        w = _bicubic((x + xmin[:, None] - center[:, None] + 0.5) * ss)
        w[x >= n[:, None]] = 0.0
        ww = np.zeros(count, dtype=np.float64)
        for j in range(kmax):                                             # the sum in index order (trailing zeros change nothing)
            ww = ww + w[:, j]
        ww[ww == 0.0] = 1.0
        w = w / ww[:, None]
        kk = np.trunc(np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS))).astype(np.int64)
        t = np.zeros((count, 2 + kmax), dtype=np.int32)
        t[:, 0], t[:, 1] = xmin, n
        t[:, 2:] = np.where(x < n[:, None], kk, 0)
    t.setflags(write=False)
    if len(_TAPS) > 4096:
        _TAPS.clear()
    _TAPS[key] = t
    return t


def value_table(dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(768,) CPU tensor: table[c * 256 + u] = ToTensor + Normalize of the byte u in channel c, with torch's own fp32 ops
    (`pic.to(float32).div(255)`, `tensor.sub_(mean).div_(std)`), then `.to(dtype)`."""
    u = torch.arange(256).float().div(255)
    rows = [u.sub(torch.tensor(m, dtype=torch.float32)).div(torch.tensor(s, dtype=torch.float32)) for m, s in zip(MEAN, STD)]
    return torch.cat(rows).to(dtype).contiguous()


def as_rgb_array(image) -> np.ndarray:
    """(h, w, 3) contiguous uint8 from a numpy array, a torch uint8 tensor or anything with PIL's `.convert` (duck typing)."""
    if hasattr(image, "convert"):
        image = np.asarray(image.convert("RGB"))
    elif torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"expected a decoded (h, w, 3) uint8 RGB image, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _align16(n: int) -> int:
    return (n + 15) & ~15


class DeviceTransform:
    """`preprocess` of the reference on the device.  `transform(image)` -> (3, dim, dim) like the reference's `preprocess(img)`;
    `transform.batch(images, ...)` for a list of images of mixed sizes: one pinned packed host buffer (descriptors, tap tables, pixels),
    one asynchronous copy, one launch."""

    def __init__(self, dim: int, target_ratio: Optional[float] = None, device="cuda", dtype: torch.dtype = torch.float32):
        self.dim, self.target_ratio, self.device, self.dtype = int(dim), target_ratio, torch.device(device), dtype
        self._tables = {}
        self._pinned = None
        self._copied = None                      # event: the last copy out of `_pinned` has finished

    def _table(self, dtype: torch.dtype) -> torch.Tensor:
        t = self._tables.get(dtype)
        if t is None:
            t = self._tables[dtype] = value_table(dtype).to(self.device)
        return t

    def pack(self, images: Sequence):
        """Host half of `batch`: (packed uint8 numpy array, descriptor offset, tap offset, tap count, pixel offset, pixel bytes)."""
        arrs = [as_rgb_array(im) for im in images]
        if not arrs:
            raise ValueError("empty batch")
        dim = self.dim
        desc = np.zeros((len(arrs), DESC_INTS), dtype=np.int32)
        tables, table_off, n_taps, off = [], {}, 0, 0
        for i, a in enumerate(arrs):
            h, w = a.shape[:2]
            hp, vp, rw, rh, left, top = geometry(h, w, dim, self.target_ratio)
            slots = []
            for key in ((w + 2 * hp, rw, left, dim), (h + 2 * vp, rh, top, dim)):
                if key not in table_off:
                    t = resample_taps(*key)
                    table_off[key] = (n_taps, t.shape[1])
                    tables.append(t)
                    n_taps += t.size
                slots.append(table_off[key])
            desc[i] = (off // 16, h, w, hp, vp, w + 2 * hp, h + 2 * vp, left, top, slots[0][0], slots[0][1], slots[1][0], slots[1][1], rw, rh, 0)
            off += _align16(a.size)
        o_desc, o_taps = 0, _align16(desc.nbytes)
        o_pix = o_taps + _align16(4 * n_taps)
        buf = self._host(o_pix + off)
        buf[o_desc:o_desc + desc.nbytes] = desc.reshape(-1).view(np.uint8)
        p = o_taps
        for t in tables:
            buf[p:p + t.nbytes] = t.reshape(-1).view(np.uint8)
            p += t.nbytes
        for i, a in enumerate(arrs):
            s = o_pix + int(desc[i, 0]) * 16
            buf[s:s + a.size] = a.reshape(-1)
        return buf, o_desc, o_taps, n_taps, o_pix, off

    def _host(self, nbytes: int) -> np.ndarray:
        if self.device.type != "cuda":                                   # (`pack` alone runs anywhere: the CPU tests read its tables)
            return np.zeros(nbytes, dtype=np.uint8)
        if self._copied is not None:
            self._copied.synchronize()                                   # the previous batch's copy still reads the buffer
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return self._pinned.numpy()[:nbytes]

    @torch.no_grad()
    def batch(self, images: Sequence, patches: bool = False, dtype: Optional[torch.dtype] = None, raw: bool = False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images: uint8 (h, w, 3) arrays / tensors / PIL images of mixed sizes -> (B, 3, dim, dim) in `dtype` (default: the transform's);
        `patches`: the ViT's patch operand rows (B (dim / 16)^2, 768) in ops.patchify's column order instead; `raw`: the resized and
        cropped uint8 image (B, dim, dim, 3).  `out`: write there (a contiguous device tensor of that shape and type, 16-byte aligned)."""
        if self.device.type != "cuda":
            raise _lib.CirrankError("the device transform runs on an MI355X only (no CPU fallback exists)")
        n, dim = len(images), self.dim
        dtype = torch.uint8 if raw else (dtype or self.dtype)
        if raw:
            layout, shape = LAYOUT_RAW, (n, dim, dim, 3)
        elif patches:
            layout, shape = LAYOUT_PATCHES, (n * (dim // 16) ** 2, 768)
        else:
            layout, shape = LAYOUT_CHW, (n, 3, dim, dim)
        if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or not out.is_cuda):
            raise ValueError(f"out: expected a contiguous {shape} {dtype} tensor on {self.device}")
        buf, o_desc, o_taps, n_taps, o_pix, n_pix = self.pack(images)
        with torch.cuda.device(self.device):
            dev = self._pinned[:buf.size].to(self.device, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            if out is None:
                out = torch.empty(shape, dtype=dtype, device=self.device)
            ops.preprocess_images(dev[o_pix:], n_pix, dev[o_desc:], dev[o_taps:], n_taps, None if raw else self._table(dtype), out, n, dim, layout)
        return out

    def __call__(self, image) -> torch.Tensor:
        return self.batch([image])[0]


def targetpad_transform(target_ratio: float, dim: int, device="cuda") -> DeviceTransform:
    """data_utils.py:87-101 under the reference's name."""
    return DeviceTransform(dim, float(target_ratio), device)


def squarepad_transform(dim: int, device="cuda") -> DeviceTransform:
    """data_utils.py:71-84 under the reference's name."""
    return DeviceTransform(dim, None, device)
