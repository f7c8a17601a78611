"""Bit-for-bit A/B of two builds of the attention kernels (attention.hip, attention_f32.hip, train_attn.hip; GPU box only):
   CIR_LIB=build/libcirrank_a.so python tools/attn_ab.py dump a.pt
   CIR_LIB=build/libcirrank_b.so python tools/attn_ab.py dump b.pt
   python tools/attn_ab.py compare a.pt b.pt
`dump` runs the smallest shapes that reach every branch of every kernel (inputs from a seeded CPU generator) and saves every output tensor;
each dump is its own process because the library is chosen at import.  None of these kernels uses atomics, so their outputs repeat from
run to run and `compare` asks for torch.equal on every entry; it prints the first mismatch and exits 1."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

f16, bf, f32 = torch.float16, torch.bfloat16, torch.float32
H, D = 2, 128


def _mask(g, shape, lk):
    """additive key mask: a tail of -10000, one finfo.min entry (the kernels clamp it), small noise elsewhere"""
    m = torch.randn(shape + (lk,), generator=g) * 0.5
    m[..., lk - max(1, lk // 4):] = -10000.0
    m[..., lk // 2] = torch.finfo(f32).min
    return m.cuda()


def _qkv(g, b1, b0, lq, lk, dtype, bank_rows=None):
    q = torch.randn((b1, b0, lq, D), generator=g).to(dtype).cuda()
    k = torch.randn((bank_rows or b1, b0, lk, D), generator=g).to(dtype).cuda()
    v = torch.randn((bank_rows or b1, b0, lk, D), generator=g).to(dtype).cuda()
    return q, k, v


def dump(path):
    from candidate_reranking_cir_amd import lib, ops, train_ops
    res = {}

    def attention(name, dtype, lq, lk, masked, b1=3, b0=2, pad=0, bank=False):
        g = torch.Generator(device="cpu").manual_seed(lq * 1000 + lk)
        q, k, v = _qkv(g, b1, b0, lq, lk, dtype, bank_rows=2 if bank else None)
        mask = _mask(g, (b1, b0), lk) if masked else None
        idx = (torch.arange(b1) % 2).flip(0).contiguous().cuda() if bank else None
        buf = torch.zeros((b1, b0, lq, D + pad), dtype=dtype, device="cuda")
        ops.attention(q, k, v, buf[..., :D], 0.125, mask, kv_index=idx)
        res[f"{name} {dtype} ({lq},{lk}) masked={masked}"] = buf.cpu()

    # cir_attention, 16-bit: stream / shared (wide and direct store, one and two rounds, 4- and 5-chunk stage) / stream above 608 keys / K-V bank
    for dtype in (f16, bf):
        for masked in (True, False):
            attention("attention", dtype, 5, 7, masked)
            attention("attention", dtype, 33, 70, masked)
            attention("attention", dtype, 197, 197, masked)
            attention("attention odd-stride", dtype, 197, 197, masked, pad=4)
            attention("attention", dtype, 577, 577, masked, b1=1)
            attention("attention", dtype, 32, 640, masked)
            attention("attention bank", dtype, 33, 70, masked, bank=True)
            attention("attention bank", dtype, 5, 7, masked, bank=True)
    # fp32 ("exact" mode)
    attention("attention", f32, 33, 65, True)
    attention("attention", f32, 1, 9, False)

    def split8(name, items, lq, lk, masked):
        g = torch.Generator(device="cpu").manual_seed(items * 100 + lk)
        q, k, v = _qkv(g, 2, items, lq, lk, f32)
        mask = _mask(g, (2, items), lk) if masked else None
        res[f"{name} ({items},{lq},{lk}) masked={masked}"] = ops.attention_split8(q, k, v, 0.125, mask).rows.cpu()

    split8("split8", 37, 1, 32, True)
    split8("split8", 5, 40, 77, False)
    split8("split8", 9, 32, 32, True)
    lib.set_tuning(lib.TUNE_ATTN_SHARED_MAX, -2)       # the f32-input MFMA form of the same op
    try:
        split8("split8 f32-kernel", 5, 40, 77, False)
        split8("split8 f32-kernel", 5, 40, 77, True)
    finally:
        lib.set_tuning(lib.TUNE_ATTN_SHARED_MAX, 0)

    for dtype in (f16, bf):
        for t, n, d in ((3, 17, 128), (4, 33, 256), (2, 577, 768)):
            g = torch.Generator(device="cpu").manual_seed(t + n)
            x = torch.randn((t, n, d), generator=g).to(dtype).cuda()
            qp = (torch.randn((t, 32, d), generator=g) * 0.3).to(dtype).cuda()
            res[f"cls {dtype} ({t},{n},{d})"] = ops.cls_cross_attention(x, qp, 0.125).cpu()

    def train(name, dtype, gr, h, lq, lk, masked, p, twin16):
        g = torch.Generator(device="cpu").manual_seed(lq * 100 + lk)
        q, k, v, do = (torch.randn((gr, h, n, 64), generator=g).to(dtype).cuda() for n in (lq, lk, lk, lq))
        mask = _mask(g, (gr,), lk) if masked else None
        out = torch.zeros_like(q)
        o32 = torch.zeros(q.shape, dtype=f32, device="cuda") if twin16 else None
        lse = train_ops.attention_train_fwd(q, k, v, mask, out, 0.125, p, 1234, out32=o32)
        gdt = dtype if twin16 else f32
        dq, dk, dv = (torch.zeros(t.shape, dtype=gdt, device="cuda") for t in (q, k, v))
        train_ops.attention_train_bwd(q, k, v, mask, out, do, lse, dq, dk, dv, 0.125, p, 1234, out32=o32)
        for label, t in (("O", out), ("o32", o32), ("LSE", lse), ("dQ", dq), ("dK", dk), ("dV", dv)):
            if t is not None:
                res[f"{name} {dtype} ({gr},{h},{lq},{lk}) masked={masked} p={p} {label}"] = t.cpu()

    for dtype in (f16, bf):
        train("train", dtype, 5, 2, 9, 9, True, 0.0, False)
        train("train", dtype, 2, 3, 70, 45, False, 0.1, False)
        train("train grad16+out32", dtype, 2, 3, 70, 45, False, 0.1, True)

    torch.cuda.synchronize()
    bad = [k for k, t in res.items() if t.dtype != torch.uint8 and not torch.isfinite(t.float()).all()]
    assert not bad, f"non-finite outputs: {bad}"
    torch.save(res, path)
    print(f"{lib.LIB_PATH}: {len(res)} tensors -> {path}")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert list(a) == list(b), f"different case lists: {sorted(set(a) ^ set(b))}"
    for name in a:
        x, y = a[name], b[name]
        if x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x, y):
            ne = (x != y).nonzero() if x.shape == y.shape else None
            where = tuple(ne[0].tolist()) if ne is not None and len(ne) else None
            print(f"MISMATCH {name}: {x.shape} {x.dtype} vs {y.shape} {y.dtype}; {0 if ne is None else len(ne)} elements differ, first at {where}"
                  + (f": {x[where].item()} vs {y[where].item()}" if where is not None else ""))
            sys.exit(1)
    print(f"{len(a)} tensors bit-identical")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
