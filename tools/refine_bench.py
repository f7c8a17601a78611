"""Rank refinement against the fast modes and the exact mode alone, in one run on one box (validate_stage2.refine_predictions).  Prints only.

  python tools/refine_bench.py                          text32 and f16 as the fast mode
  options: --modes text32,f16  --queries 64  --k 100  --sample 8  --safety 2.0  --query-batch 16  --rounds 3  --limit 600  --json out.json
           --first N --cuts 1,5,10,50     one more selection beside the four below

Workload: the separated-logit synthetic profile of the rank fixtures (tests/golden/rank224.npz: full-size models, weight profile "test",
seed 21, structured `scene_images`, a 256-image bank) as a CIRR-shaped split at K = 100 + 5 candidates per query, 224 px, scored from a
precomputed bank like `generate_val_predictions`.  Per fast mode: the margin calibrated on the first `--sample` queries (`calibrate_margin`),
the share of entries phase 2 re-scores, and triplets/s of phase 1 (the fast run), of phase 2 (refine_predictions, counted on ALL
Q * (K + 5) triplets: what the refinement adds to the run) and of both together, beside the fast mode alone (= phase 1) and the exact mode
alone.  Whether the refined order equals the exact mode's on every position is checked and printed (it must, when `violations` is 0).

Four selections side by side in the same run (refine_predictions' first= / cuts=): every position; first=50 (the CIRR submission's names);
first=10 with cuts=(50,); first=0 with cuts=(1, 5, 10, 50) (the recall tuples alone).  Per selection: the share re-scored, the queries
touched, phase 2 and combined triplets/s, the time of the selection step alone (rank_undecided on both matrices and the two count reads),
and whether what the selection certifies - the first places in order, the set before every cut, the subset rows at every position -
equals the exact run's.

Method: every form is run once before it is timed; the forms alternate inside a round, host wall clock around a synchronised call, median
over the rounds with min .. max beside it.  Each fast mode is measured by a child process of its own under `timeout -k 10 <--limit>`; the
parent never opens the GPU and stops at the first child that fails or runs out of time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _split(n_index, n_query, k, seed=5):
    import numpy as np
    from candidate_reranking_cir_amd import synthetic, validate_stage2 as V
    rng = np.random.default_rng(seed)
    refs = rng.integers(n_index, size=n_query)
    cand = np.stack([rng.permutation(np.delete(np.arange(n_index), r))[:k] for r in refs]).astype(np.int64)
    labels = np.zeros((n_query, k), dtype=bool)
    labels[np.arange(n_query), rng.integers(k, size=n_query)] = True
    targets = cand[labels]
    groups = np.stack([np.concatenate([[targets[q]], rng.permutation(np.setdiff1d(np.arange(n_index), [refs[q], targets[q]]))[:4]])
                       for q in range(n_query)]).astype(np.int64)
    caps = [synthetic.caption_text(q, 30) for q in range(n_query)]
    return V.RelativeValSet(ref_index=refs.astype(np.int64), cand_index=cand, labels=labels, captions=caps, group_index=groups, target_index=targets)


def _clock(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


SELECTIONS = (("every position", None, ()), ("first=50", 50, ()), ("first=10 cuts=(50,)", 10, (50,)), ("first=0 cuts=(1,5,10,50)", 0, (1, 5, 10, 50)))


def _selections(a):
    extra = ()
    if a.first is not None or a.cuts:
        cuts = tuple(int(c) for c in a.cuts.split(",")) if a.cuts else ()
        extra = ((f"first={a.first or 0} cuts={cuts}", a.first or 0, cuts),)
    return SELECTIONS + extra


def _certified_equal(first, cuts, lr, gr, le, ge, active):
    """What the selection certifies, compared with the exact run: every position (first None), or the first places and the cut sets."""
    import torch
    order = lambda x: torch.argsort(x, dim=1, descending=True, stable=True)
    if not torch.equal(order(gr), order(ge)):
        return False
    o_r, o_e = order(lr)[active], order(le)[active]
    if first is None:
        return bool(torch.equal(o_r, o_e))
    k = lr.shape[1]
    if not torch.equal(o_r[:, :min(first, k)], o_e[:, :min(first, k)]):
        return False
    return all(torch.equal(o_r[:, :c].sort(dim=1).values, o_e[:, :c].sort(dim=1).values) for c in cuts if c < k)


def child(a):
    import torch
    from candidate_reranking_cir_amd import config, ops, synthetic, weights, validate_stage2 as V
    from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    if not torch.cuda.is_available():
        sys.exit("refine_bench.py measures on an MI355X: no GPU found")
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    g = config.BertGeometry.from_dict(dict(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, layer_norm_eps=1e-12,
                                           vocab_size=30524, max_position_embeddings=512, encoder_width=768))
    v = config.VitGeometry(image_size=a.image_size)
    m2 = BLIP_NLVR(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m2.load_state_dict(weights.synth_state_dict(weights.nlvr_param_spec(g, v), 21, "test"))
    m1.load_state_dict(weights.synth_state_dict(weights.retrieval_param_spec(g, v), 22, "test"))
    m2, m1 = m2.cuda().float().eval(), m1.cuda().float().eval()
    for m in (m2, m1):
        m.set_precision(a.child)
    r2, r1 = m2.referee(), m1.referee()
    ds = _split(a.index, a.queries, a.k)
    images = synthetic.scene_images(range(a.index), a.image_size)
    bank, bank32 = V.extract_index_features(images, m2, batch_size=64), V.extract_index_features(images, r2, batch_size=64, dtype=torch.float32)
    margin, raw = V.calibrate_margin(m2, m1, ds, bank, bank32, rows=range(a.sample), referee=(r2, r1), query_batch=a.query_batch, safety=a.safety)
    fast = lambda: V.generate_val_predictions(m2, m1, ds, bank, query_batch=a.query_batch)
    exact = lambda: V.generate_val_predictions(r2, r1, ds, bank32, query_batch=a.query_batch)
    refine = lambda lg, first, cuts: V.refine_predictions(m2, m1, ds, lg[0], lg[1], bank32, margin, referee=(r2, r1), query_batch=a.query_batch,
                                                          first=first, cuts=cuts)
    active = torch.as_tensor(ds.labels.any(axis=1), device="cuda")

    def select(lg, first, cuts):                                                # the selection step of phase 2 alone, with its two host reads
        return int(ops.rank_undecided(lg[0], margin, active, first=first, cuts=cuts)[1]) + int(ops.rank_undecided(lg[1], margin)[1])
    sels = _selections(a)
    le, ge = exact()
    first_run = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                        # (a violation is reported in the table, not as a warning)
        for name, first, cuts in sels:                                          # (also the warm-up of every form)
            lr, gr, stats = refine(fast(), first, cuts)
            first_run[name] = (stats, _certified_equal(first, cuts, lr, gr, le, ge, active))
    t = dict(phase1=[], exact=[], phase2={name: [] for name, _, _ in sels}, select={name: [] for name, _, _ in sels})
    for _ in range(a.rounds):
        dt, lg = _clock(fast)
        t["phase1"].append(dt)
        for name, first, cuts in sels:
            mine = (lg[0].clone(), lg[1].clone())                               # refinement writes in place: every selection starts from the fast run
            t["select"][name].append(_clock(lambda: select(mine, first, cuts))[0])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t["phase2"][name].append(_clock(lambda: refine(mine, first, cuts))[0])
        t["exact"].append(_clock(exact)[0])
    n = a.queries * (a.k + 5)
    rate = lambda s: dict(median=round(n / statistics.median(s)), lo=round(n / max(s)), hi=round(n / min(s)))
    ms = lambda s: dict(median=round(1e3 * statistics.median(s), 2), lo=round(1e3 * min(s), 2), hi=round(1e3 * max(s), 2))
    rows = []
    for name, first, cuts in sels:
        stats, same = first_run[name]
        both = [x + y for x, y in zip(t["phase1"], t["phase2"][name])]
        rows.append(dict(selection=name, first=first, cuts=list(cuts), rescored=stats["rescored"], entries=stats["entries"],
                         share=round(stats["rescored"] / stats["entries"], 4), queries_rescored=stats["queries_rescored"],
                         max_deviation=stats["max_deviation"], violations=stats["violations"], certified=stats["certified"],
                         certified_equals_exact=bool(same), phase2_ms=ms(t["phase2"][name]), select_ms=ms(t["select"][name]),
                         triplets_per_s=dict(phase2=rate(t["phase2"][name]), combined=rate(both))))
    full = rows[0]
    res = dict(mode=a.child, queries=a.queries, k=a.k, triplets=n, sample=a.sample, safety=a.safety, margin=margin, raw_max_on_sample=raw,
               rescored=full["rescored"], entries=full["entries"], share=full["share"], queries_rescored=full["queries_rescored"],
               max_deviation=full["max_deviation"], violations=full["violations"], order_equals_exact=full["certified_equals_exact"],
               triplets_per_s=dict(fast_alone=rate(t["phase1"]), phase2=full["triplets_per_s"]["phase2"], combined=full["triplets_per_s"]["combined"],
                                   exact_alone=rate(t["exact"])),
               phase1_ms=ms(t["phase1"]), exact_ms=ms(t["exact"]), selections=rows)
    with open(a.child_out, "w") as f:
        json.dump(res, f)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--modes", default="text32,f16")
    p.add_argument("--queries", type=int, default=64)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--index", type=int, default=256)
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--sample", type=int, default=8)
    p.add_argument("--safety", type=float, default=2.0)
    p.add_argument("--query-batch", type=int, default=16)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--limit", type=int, default=600, help="seconds per fast mode (the child's time limit)")
    p.add_argument("--json", default=None)
    p.add_argument("--first", type=int, default=None, help="one more selection: refine_predictions' first=")
    p.add_argument("--cuts", default="", help="... and its cuts=, comma-separated")
    p.add_argument("--child", default=None, help=argparse.SUPPRESS)
    p.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        return child(a)
    rows = []
    for mode in a.modes.split(","):
        out = os.path.join(tempfile.mkdtemp(prefix="refine_bench_"), mode + ".json")
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--child-out", out] + \
              [x for k in ("queries", "k", "index", "image_size", "sample", "safety", "query_batch", "rounds")
               for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))] + \
              (["--first", str(a.first)] if a.first is not None else []) + (["--cuts", a.cuts] if a.cuts else [])
        r = subprocess.run(cmd)                                                  # (the child's own output goes straight through)
        if r.returncode != 0 or not os.path.exists(out):
            sys.exit(f"refine_bench.py: the {mode} step ended with status {r.returncode}; nothing further is started")
        with open(out) as fres:
            rows.append(json.load(fres))
        d, s = rows[-1], rows[-1]["triplets_per_s"]
        f = lambda x: f"{x['median']:>6} [{x['lo']} .. {x['hi']}]"
        print(f"{mode}: margin {d['margin']:.3e} (sample max {d['raw_max_on_sample']:.3e} x {d['safety']})  re-scored {d['rescored']} of {d['entries']} "
              f"({d['share']:.3f}) in {d['queries_rescored']} of {d['queries']} queries  max deviation {d['max_deviation']:.3e}  violations "
              f"{d['violations']}  order equals exact: {d['order_equals_exact']}\n"
              f"   triplets/s   fast alone (= phase 1) {f(s['fast_alone'])}   phase 2 {f(s['phase2'])}   combined {f(s['combined'])}   "
              f"exact alone {f(s['exact_alone'])}", flush=True)
        g = lambda x: f"{x['median']:.1f} [{x['lo']:.1f} .. {x['hi']:.1f}]"
        for r in d["selections"]:
            rs = r["triplets_per_s"]
            print(f"   {r['selection']:<26} re-scored {r['rescored']:>5} of {r['entries']} ({r['share']:.3f}) in {r['queries_rescored']:>3} queries  "
                  f"violations {r['violations']}  certified part equals exact: {r['certified_equals_exact']}\n"
                  f"   {'':<26} phase 2 {f(rs['phase2'])} triplets/s = {g(r['phase2_ms'])} ms (selection step {g(r['select_ms'])} ms)   "
                  f"combined {f(rs['combined'])}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fjson:
            json.dump(rows, fjson, indent=1)


if __name__ == "__main__":
    main()
