"""Stage-I retrieval: validate.rank_index_topk (cir_topk_select + cir_rank_of, any index size) against validate.rank_index (the full sort,
at most 8192 images) on the same tensors, and the CIRCO-scale points the full sort cannot run.  GPU box only.

  python tools/topk_bench.py                            both parts
  python tools/topk_bench.py --part small               Q in {64, 4181} x n in {2297, 6346, 8192}, k = 100: rank_index_topk vs rank_index
  python tools/topk_bench.py --part large               Q in {800, 4181}, n = 123403, k = 100: the matrix, the selection and the rank kernel apart
  options: --rounds R  --k K  --json out.json

Method: every form is launched before it is timed and warmed on the work it is about to time; the forms of a point ALTERNATE inside a round
(device events around `inner` back-to-back calls each) and the figure is the MEDIAN over the rounds with the spread (min .. max) beside it.
Both forms include what a caller pays: the distance matrix, torch's allocations of outputs and workspace.  The shader clock is read
(rocm-smi, read only) while the point's work is in flight.  Before timing, the two forms' first k columns are compared (they must be equal)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from candidate_reranking_cir_amd import ops, validate as V


def _timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def _sclk():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--csv"], capture_output=True, text=True, timeout=20)
        lines = [l for l in r.stdout.strip().splitlines() if l]
        head, row = lines[0].split(","), lines[1].split(",")
        return {h: v for h, v in zip(head, row) if "sclk" in h.lower() or "mclk" in h.lower()}
    except Exception as e:                                       # the figure is context, not a result
        return {"unavailable": repr(e)}


def _alternate(forms, rounds, inner, warm_s=1.0):
    """forms: {name: fn} -> ({name: [ms per call, one per round]}, clocks read while the forms were in flight)"""
    for fn in forms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
    for _ in range(3):
        for fn in forms.values():
            fn()
    clocks = _sclk()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            out[k].append(_timed(fn, inner))
    return out, clocks


def _stat(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))


def _features(q_n, n):
    g = torch.Generator(device="cuda").manual_seed(q_n + n)
    pred = torch.nn.functional.normalize(torch.randn((q_n, 256), generator=g, device="cuda"), dim=-1)
    index = torch.nn.functional.normalize(torch.randn((n, 256), generator=g, device="cuda"), dim=-1)
    target = torch.randint(0, n, (q_n, 1), generator=g, device="cuda")
    return pred, index, target


def small(a):
    rows = []
    for q_n in (64, 4181):
        for n in (2297, 6346, 8192):
            pred, index, target = _features(q_n, n)
            full = V.rank_index(pred, index)
            topk, ranks = V.rank_index_topk(pred, index, a.k, cols=target)
            assert torch.equal(topk, full[:, :a.k]) and torch.equal(torch.gather(full, 1, ranks), target), "the two forms disagree"
            del full, topk, ranks
            ms, clocks = _alternate({"rank_index": lambda: V.rank_index(pred, index),
                                     "rank_index_topk": lambda: V.rank_index_topk(pred, index, a.k, cols=target)}, a.rounds, 3 if q_n > 1000 else 20)
            s, t = _stat(ms["rank_index"]), _stat(ms["rank_index_topk"])
            print(f"Q {q_n} n {n} k {a.k}: rank_index {s['median_ms']:.3f} ms [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]   rank_index_topk "
                  f"{t['median_ms']:.3f} ms [{t['min_ms']:.3f} .. {t['max_ms']:.3f}]   topk / full {t['median_ms'] / s['median_ms']:.3f}   {clocks}", flush=True)
            rows.append(dict(Q=q_n, n=n, k=a.k, rank_index=s, rank_index_topk=t, ratio=round(t["median_ms"] / s["median_ms"], 4), clocks=clocks))
    return rows


def large(a):
    rows = []
    n = 123403
    for q_n in (800, 4181):
        pred, index, target = _features(q_n, n)
        cols = torch.cat([target, torch.randint(0, n, (q_n, 5), device="cuda")], 1)
        exclude = torch.randint(0, n, (q_n,), device="cuda")
        mat = ops.linear_f32(pred, index, None, mode=2)
        forms = {"matrix": lambda: ops.linear_f32(pred, index, None, mode=2),
                 "select": lambda: ops.topk_desc(mat, a.k, exclude),
                 "rank_of_6": lambda: ops.rank_of(mat, cols, exclude),
                 "rank_index_topk": lambda: V.rank_index_topk(pred, index, a.k, exclude=exclude, cols=cols)}
        ms, clocks = _alternate(forms, a.rounds, 2)
        st = {k: _stat(v) for k, v in ms.items()}
        gb = q_n * n * 4 / 1e9
        print(f"Q {q_n} n {n} k {a.k} ({gb:.2f} GB matrix): " + "   ".join(f"{k} {s['median_ms']:.2f} ms [{s['min_ms']:.2f} .. {s['max_ms']:.2f}]"
                                                                           for k, s in st.items()) +
              f"   rank_of reads {gb / st['rank_of_6']['median_ms']:.2f} TB/s   {clocks}", flush=True)
        rows.append(dict(Q=q_n, n=n, k=a.k, matrix_gb=round(gb, 3), **st, rank_of_tb_per_s=round(gb / st["rank_of_6"]["median_ms"], 3), clocks=clocks))
        del mat
    return rows


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["small", "large", "both"], default="both")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--json", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_bench.py measures on an MI355X: no GPU found")
    res = dict(rounds=args.rounds, k=args.k)
    if args.part in ("small", "both"):
        res["small"] = small(args)
    if args.part in ("large", "both"):
        res["large"] = large(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
