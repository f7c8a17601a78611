"""Long-caption query-side fold (cir_cross_attention_folded_long, 33-64 caption tokens) against the projected path (K|V GEMM + cir_attention)
on the same tensors; with `--fold short`, the one-block fold for captions of at most 16 tokens (cir_cross_attention_folded_short) against the
32-token kernels (cir_cross_attention_folded) on the same tensors; with `--fold wide`, the key-split fold for 33-64 caption tokens against
225-608 keys (cir_cross_attention_folded_long_wide) against the projected path.  GPU box only.

  python tools/fold_long_bench.py                       one fusion layer: L in {33, 40, 48, 49, 64}, N = 197, T = 6720, fp16 and bf16
  python tools/fold_long_bench.py --mode step --tokens 40
                                                        a whole scoring step (64 queries x 105 candidates, 224 px: ViT, stage-I z_t, fusion) with
                                                        BLIP_NLVR.set_long_caption_fold on and off
  python tools/fold_long_bench.py --fold short          one fusion layer: L in {8, 12, 16} at (N, T) = (197, 6720) and (577, 1680), fp16 and bf16
  python tools/fold_long_bench.py --fold short --mode step --tokens 12 [--px 384 --queries 16]
                                                        the scoring step with BLIP_NLVR.set_short_caption_fold on and off
  python tools/fold_long_bench.py --fold wide           one fusion layer: L in {33, 40, 48, 49, 56, 64}, N = 577, T = 1680, fp16 and bf16
  python tools/fold_long_bench.py --fold wide --mode step --tokens 40 [--queries 16]
                                                        the 384-px scoring step with BLIP_NLVR.set_long_caption_fold_wide on and off
  options: --t T  --n N (= --keys N)  --lengths 33,40,..  --dtypes fp16,bf16  --rounds R  --px 224|384  --json out.json

Method: every shape is launched before it is timed and the part is warmed for 1.5 s on the work it is about to time; the two forms ALTERNATE
inside a round (device events around `inner` back-to-back launches each), and the figure is the MEDIAN over the rounds, with the spread
(min .. max) beside it.  Flops are the ones each form executes, computed from the shapes: the fold 2 T (2 H Lp 64 D + 2 H Lp D Np) with
Lp = 16 ceil(L / 16) rows and Np = 224 keys as the kernel runs them (`--fold wide`: Lp = 64 rows and Np = 640 keys whatever L and N), the projected path 2 T N D 4 D + 4 T 2 L N D; with `--fold short` both
forms are folds: Lp = 16 rows against 32, Np = 224 keys up to 224 and 608 above."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from candidate_reranking_cir_amd import ops

D, H = 768, 12


def _timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def _alternate(forms, rounds, inner, warm_s=1.5):
    """forms: {name: fn}.  -> {name: [ms per call, one per round]}"""
    for fn in forms.values():                                  # first launches: code objects, lazy caches
        fn(); fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:                    # power / clocks as in steady state
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            out[k].append(_timed(fn, inner))
    return out


def _stat(v):
    return statistics.median(v), min(v), max(v)


def layer_mode(a):
    rows = []
    for dname in a.dtypes.split(","):
        dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
        g = torch.Generator(device="cuda").manual_seed(0)
        r = lambda shape, s: (torch.randn(shape, generator=g, device="cuda") * s).to(dt)
        t_n, n = a.t, a.n
        x = r((t_n, n, D), 1.0)
        wk, wv = r((2, D, D), 0.03), r((2, D, D), 0.03)
        bk, bv = torch.randn((2, D), device="cuda") * 0.5, torch.randn((2, D), device="cuda") * 0.5
        wkt, wvp = ops.fold_pack_key(wk), ops.fold_pack_value(wv)
        wkv, bkv = torch.cat([wk[0], wv[0], wk[1], wv[1]]), torch.cat([bk[0], bv[0], bk[1], bv[1]])
        for l in [int(s) for s in a.lengths.split(",")]:
            q = r((2, t_n * l, D), 1.0)
            out = torch.empty((t_n, l, 2, D), dtype=dt, device="cuda")
            o2 = torch.empty((t_n, l, 2, D), dtype=dt, device="cuda")

            fold = ops.cross_attention_folded_long_wide if a.fold == "wide" else ops.cross_attention_folded_long

            def folded():
                fold(q, x, wkt, wvp, bv, out, l, 0.125)

            def projected():
                kv = ops.gemm(x.view(t_n * n, D), wkv, bkv).view(t_n, n, 4, D)
                ops.attention(q.view(2, t_n, l, D).permute(1, 0, 2, 3), kv[:, :, 0::2].permute(0, 2, 1, 3), kv[:, :, 1::2].permute(0, 2, 1, 3),
                              o2.permute(0, 2, 1, 3), 0.125)

            ms = _alternate({"folded_long": folded, "projected": projected}, a.rounds, a.inner)
            (tf, tf0, tf1), (tp, tp0, tp1) = _stat(ms["folded_long"]), _stat(ms["projected"])
            lp, np_ = (64, 640) if a.fold == "wide" else (16 * -(-l // 16), 224)
            fl_f = 2.0 * t_n * 2 * (2 * H * lp * 64 * D + 2 * H * lp * D * np_)
            fl_p = 2.0 * t_n * n * D * 4 * D + 4.0 * t_n * 2 * l * n * D
            diff = (out.float() - o2.float()).abs().max().item()
            print(f"{dname} T {t_n} L {l} N {n}: folded_long {tf * 1e3:.0f} us [{tf0 * 1e3:.0f} .. {tf1 * 1e3:.0f}] ({fl_f / tf / 1e9:.0f} TFLOP/s of its "
                  f"{fl_f / 1e6 / t_n:.0f} MFLOP per candidate)   projected {tp * 1e3:.0f} us [{tp0 * 1e3:.0f} .. {tp1 * 1e3:.0f}] ({fl_p / tp / 1e9:.0f} TFLOP/s of "
                  f"its {fl_p / 1e6 / t_n:.0f} MFLOP)   ratio {tf / tp:.3f}   max|folded - projected| {diff:.2e}", flush=True)
            rows.append(dict(dtype=dname, T=t_n, L=l, N=n, folded_long_us=round(tf * 1e3, 1), folded_long_us_min_max=[round(tf0 * 1e3, 1), round(tf1 * 1e3, 1)],
                             projected_us=round(tp * 1e3, 1), projected_us_min_max=[round(tp0 * 1e3, 1), round(tp1 * 1e3, 1)], ratio=round(tf / tp, 4),
                             folded_long_mflop_per_candidate=round(fl_f / 1e6 / t_n, 1), projected_mflop_per_candidate=round(fl_p / 1e6 / t_n, 1),
                             folded_long_tflops=round(fl_f / tf / 1e9, 1), projected_tflops=round(fl_p / tp / 1e9, 1), max_abs_diff=diff))
            del q, out, o2
    return dict(mode="layer", fold=a.fold, rounds=a.rounds, inner=a.inner, rows=rows)


def short_layer_mode(a):
    """cir_cross_attention_folded_short against cir_cross_attention_folded (the path the engine takes with the switch off) on the same tensors."""
    rows = []
    shapes = [(a.n, a.t)] if a.n or a.t else [(197, 6720), (577, 1680)]
    for dname in a.dtypes.split(","):
        dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
        g = torch.Generator(device="cuda").manual_seed(0)
        r = lambda shape, s: (torch.randn(shape, generator=g, device="cuda") * s).to(dt)
        wkt, wvp, bv = ops.fold_pack_key(r((2, D, D), 0.03)), ops.fold_pack_value(r((2, D, D), 0.03)), torch.randn((2, D), device="cuda") * 0.5
        for n, t_n in shapes:
            n, t_n = n or 197, t_n or 6720
            x = r((t_n, n, D), 1.0)
            for l in [int(s) for s in (a.lengths or "8,12,16").split(",")]:
                q = r((2, t_n * l, D), 1.0)
                out, o2 = (torch.empty((t_n, l, 2, D), dtype=dt, device="cuda") for _ in range(2))
                ms = _alternate({"short": lambda: ops.cross_attention_folded_short(q, x, wkt, wvp, bv, out, l, 0.125),
                                 "fold32": lambda: ops.cross_attention_folded(q, x, wkt, wvp, bv, o2, l, 0.125)}, a.rounds, a.inner)
                (ts, ts0, ts1), (tp, tp0, tp1) = _stat(ms["short"]), _stat(ms["fold32"])
                np_ = 224 if n <= 224 else 608
                fl = lambda lp: 2.0 * t_n * 2 * (2 * H * lp * 64 * D + 2 * H * lp * D * np_)
                diff = (out.float() - o2.float()).abs().max().item()
                print(f"{dname} T {t_n} L {l} N {n}: folded_short {ts * 1e3:.0f} us [{ts0 * 1e3:.0f} .. {ts1 * 1e3:.0f}] ({fl(16) / ts / 1e9:.0f} TFLOP/s executed)   "
                      f"folded {tp * 1e3:.0f} us [{tp0 * 1e3:.0f} .. {tp1 * 1e3:.0f}] ({fl(32) / tp / 1e9:.0f} TFLOP/s executed)   ratio {ts / tp:.3f}   "
                      f"max|short - folded| {diff:.2e}", flush=True)
                rows.append(dict(dtype=dname, T=t_n, L=l, N=n, folded_short_us=round(ts * 1e3, 1), folded_short_us_min_max=[round(ts0 * 1e3, 1), round(ts1 * 1e3, 1)],
                                 folded_us=round(tp * 1e3, 1), folded_us_min_max=[round(tp0 * 1e3, 1), round(tp1 * 1e3, 1)], ratio=round(ts / tp, 4),
                                 folded_short_tflops=round(fl(16) / ts / 1e9, 1), folded_tflops=round(fl(32) / tp / 1e9, 1), max_abs_diff=diff))
                del q, out, o2
            del x
    return dict(mode="layer", fold="short", rounds=a.rounds, inner=a.inner, rows=rows)


def step_mode(a):
    from candidate_reranking_cir_amd import config, synthetic
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    q_n, k, l = a.queries, a.k, a.tokens
    dev = torch.device("cuda")
    g, v = config.BertGeometry(), config.VitGeometry(image_size=a.px)
    m2 = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).to(dev).eval()
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer()).to(dev).eval()
    images = torch.randn((q_n + q_n * k, 3, a.px, a.px), device=dev).half()
    ids = torch.stack([synthetic.caption_ids(q, l) for q in range(q_n)]).to(dev)
    mask = torch.ones_like(ids)
    qidx = torch.arange(q_n, device=dev).repeat_interleave(k)

    def step():
        toks = m2.img_embed16(images)
        z = m1.z_t(toks[:q_n], ids, mask)
        return m2.score(z.last_hidden_state, ids, mask, toks[q_n:], qidx)

    import warnings
    warnings.simplefilter("ignore")                             # (the switch-off form reports its projected path once)

    switch = {"long": m2.set_long_caption_fold, "wide": m2.set_long_caption_fold_wide, "short": m2.set_short_caption_fold}[a.fold]

    def form(on):
        def run():
            switch(on)
            return step()
        return run

    name = f"fold_{a.fold}"
    ms = _alternate({name + "_on": form(True), name + "_off": form(False)}, a.rounds, 1, warm_s=3.0)
    switch(True); lon = step()
    switch(False); loff = step()
    (t1, a1, b1), (t0, a0, b0) = _stat(ms[name + "_on"]), _stat(ms[name + "_off"])
    diff = (lon - loff).abs().max().item()
    print(f"step {q_n} x {k}, {l} caption tokens, {a.px} px, {name}: switch on {t1:.1f} ms [{a1:.1f} .. {b1:.1f}]   off {t0:.1f} ms [{a0:.1f} .. {b0:.1f}]   "
          f"ratio {t1 / t0:.3f}   fold_fallbacks {m2.engines()[1].fold_fallbacks}   max|logit difference| {diff:.2e}", flush=True)
    return dict(mode="step", fold=a.fold, px=a.px, queries=q_n, k=k, tokens=l, rounds=a.rounds, on_ms=round(t1, 2), on_ms_min_max=[round(a1, 2), round(b1, 2)],
                off_ms=round(t0, 2), off_ms_min_max=[round(a0, 2), round(b0, 2)], ratio=round(t1 / t0, 4), max_abs_logit_diff=diff)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=["layer", "step"], default="layer")
    p.add_argument("--fold", choices=["long", "short", "wide"], default="long")
    p.add_argument("--px", type=int, choices=[224, 384], default=None)
    p.add_argument("--t", type=int, default=None)
    p.add_argument("--n", "--keys", dest="n", type=int, default=None)
    p.add_argument("--lengths", default=None)
    p.add_argument("--dtypes", default="fp16,bf16")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--inner", type=int, default=5)
    p.add_argument("--tokens", type=int, default=None)
    p.add_argument("--queries", type=int, default=None)
    p.add_argument("--k", type=int, default=105)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fold_long_bench.py measures on an MI355X: no GPU found")
    if args.tokens is None:
        args.tokens = 12 if args.fold == "short" else 40
    args.px = args.px or (384 if args.fold == "wide" else 224)
    args.queries = args.queries or (16 if args.fold == "wide" else 64)         # (384 px: 16 x 105 = 1680 candidates)
    if args.fold == "long":
        args.t, args.n, args.lengths = args.t or 6720, args.n or 197, args.lengths or "33,40,48,49,64"
    if args.fold == "wide":
        args.t, args.n, args.lengths = args.t or 1680, args.n or 577, args.lengths or "33,40,48,49,56,64"
    res = step_mode(args) if args.mode == "step" else short_layer_mode(args) if args.fold == "short" else layer_mode(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
