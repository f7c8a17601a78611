"""The device image transform (cir_preprocess_images) at the reference's two index geometries: 2297 synthetic 500 x 375 images to 384 px
(the CIRR validation index) and 6784 to 224 px (the benchmark's image count), in batches.  Per geometry, one JSON line with
  * the kernel time from HIP events (patch-row layout in the engine's 16-bit type), per image, and the effective GB/s against the byte
    floor `source bytes + output bytes`;
  * the source-row redundancy of the band tiling (rows read by more than one band of 16 output rows), from the tap tables;
  * the wall time of DeviceTransform.batch including packing and the pinned copy;
  * beside it the ViT-B/16 forward of the same images from those patch rows, on the unchanged engine;
  * PIL's time for the same transform on the host cores (ImageOps.expand / resize / crop + the numpy normalisation), where PIL imports.

    python tools/preprocess_bench.py [--batch 256] [--pil-images 64]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from candidate_reranking_cir_amd import config, engine, ops, weights
from candidate_reranking_cir_amd import preprocess as PP


def band_redundancy(h, w, dim, ratio):
    """Source rows read / source rows of the image, summed over the bands of 16 output rows (pad rows are never read)."""
    hp, vp, rw, rh, left, top = PP.geometry(h, w, dim, ratio)
    vt = PP.resample_taps(h + 2 * vp, rh, top, dim)
    rows = 0
    for b in range(0, dim, 16):
        t = vt[b:b + 16]
        y0, y1 = int(t[:, 0].min()) - vp, int((t[:, 0] + t[:, 1]).max()) - vp
        rows += max(min(y1, h) - max(y0, 0), 0)
    return rows / h


def pil_seconds(images, dim, ratio, workers):
    try:
        from PIL import Image, ImageOps
    except ImportError:
        return None
    from concurrent.futures import ThreadPoolExecutor
    table = PP.value_table().view(3, 256).numpy()

    def one(a):
        h, w = a.shape[:2]
        hp, vp, rw, rh, left, top = PP.geometry(h, w, dim, ratio)
        img = ImageOps.expand(Image.fromarray(a, "RGB"), border=(hp, vp, hp, vp), fill=0).resize((rw, rh), Image.BICUBIC)
        u8 = np.asarray(img.crop((left, top, left + dim, top + dim)))
        return np.stack([table[c][u8[:, :, c]] for c in range(3)])

    t0 = time.perf_counter()
    with ThreadPoolExecutor(workers) as ex:                    # PIL releases the GIL inside resize
        list(ex.map(one, images))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pil-images", type=int, default=64)
    ap.add_argument("--cases", default="2297x384,6784x224")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rs = np.random.RandomState(0)
    pool = [rs.randint(0, 256, size=(375, 500, 3)).astype(np.uint8) for _ in range(8)]       # h = 375, w = 500
    workers = min(16, len(os.sched_getaffinity(0)))
    for case in args.cases.split(","):
        n, dim = (int(x) for x in case.split("x"))
        v = config.VitGeometry(image_size=dim)
        vit = engine.VitEngine(weights.synth_state_dict(weights._vit_spec(v), 0, "test"), v, torch.float16, dev)
        tr = PP.DeviceTransform(dim, 1.25, dev)
        table = PP.value_table(torch.float16).to(dev)
        k_ms = wall = vit_ms = 0.0
        for rep in range(2):                                   # the second pass is the measurement
            k_ms = wall = vit_ms = 0.0
            for s in range(0, n, args.batch):
                imgs = [pool[i % len(pool)] for i in range(s, min(s + args.batch, n))]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = tr.batch(imgs, patches=True, dtype=torch.float16)
                torch.cuda.synchronize()
                wall += time.perf_counter() - t0
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                buf, o_desc, o_taps, n_taps, o_pix, n_pix = tr.pack(imgs)
                d = torch.from_numpy(buf.copy()).to(dev)
                e0.record()
                ops.preprocess_images(d[o_pix:], n_pix, d[o_desc:], d[o_taps:], n_taps, table, rows, len(imgs), dim, PP.LAYOUT_PATCHES)
                e1.record()
                vit.forward(None, patches=rows)
                e2.record()
                torch.cuda.synchronize()
                k_ms += e0.elapsed_time(e1)
                vit_ms += e1.elapsed_time(e2)
        src_b, out_b = 375 * 500 * 3, dim * dim * 3 * 2
        pil = pil_seconds([pool[i % len(pool)] for i in range(args.pil_images)], dim, 1.25, workers)
        print(json.dumps({
            "images": n, "dim": dim, "batch": args.batch, "kernel_ms": round(k_ms, 3), "kernel_us_per_image": round(1e3 * k_ms / n, 3),
            "floor_bytes_per_image": src_b + out_b, "effective_GBps": round(n * (src_b + out_b) / (k_ms * 1e-3) / 1e9, 1),
            "band_row_redundancy": round(band_redundancy(375, 500, dim, 1.25), 3),
            "wall_ms_pack_copy_kernel": round(1e3 * wall, 1), "vit_forward_ms": round(vit_ms, 1),
            "pil_ms_per_image_%d_threads" % workers: None if pil is None else round(1e3 * pil / args.pil_images, 3),
            "pil_ms_for_all_images_extrapolated": None if pil is None else round(1e3 * pil / args.pil_images * n, 1)}), flush=True)


if __name__ == "__main__":
    main()
