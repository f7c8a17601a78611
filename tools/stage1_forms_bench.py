"""Stage-I CIRR validation over a whole split, wall time: validate.compute_cirr_val_metrics in the reference's call form (a dataset object
with names, fp32 index tokens as utils.py:57-72 hands them over) beside the native call sequences on the same model, tokens and queries.
GPU box only.

  python tools/stage1_forms_bench.py                     the reference's geometry: 2297 index images, 4181 queries, 384 px (577 tokens)
  options: --index N  --queries Q  --px P  --topk K  --rounds R  --json out.json

Forms (each a complete call: names -> rows, query features, ranking, metrics, top-K dict):
  reference_fp32    compute_cirr_val_metrics(dataset, model, fp32 tokens, pooled, names, topk=K): parses the items, converts the tokens
  reference_bank16  the same given the 16-bit bank (no conversion launch)
  native_topk       generate_val_predictions + rank_index_topk + cirr_topk_from_ranks on integer rows (INTEGRATION, stage-I section)
  native_fullsort   generate_val_predictions + rank_index + cirr_topk: every row sorted, the name matrix built on the host (n <= 8192)

Method: the index tokens and pooled features are random (the ViT is not part of any form); the model is the full-size BLIP_Retrieval with
synthesised weights, fp16 operands.  Every form runs once on 64 queries before anything is timed; the forms then ALTERNATE inside a round and
the figure is the MEDIAN wall time (perf_counter around the call, device synchronised) over the rounds with min .. max beside it.  The four
forms' metrics and top-K names are compared before timing (they must be equal)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from candidate_reranking_cir_amd import config, ops, synthetic, validate as V1, weights
from candidate_reranking_cir_amd.blip_stage1 import BLIP_Retrieval


class CirrVal:
    """CIRR 'relative' val items of stage I (data_utils.py:340) over integer arrays."""
    split = "val"

    def __init__(self, names, refs, targets, captions, groups):
        self.names, self.refs, self.targets, self.captions, self.groups = names, refs, targets, captions, groups

    def __len__(self):
        return len(self.refs)

    def __getitem__(self, i):
        return self.names[self.refs[i]], self.names[self.targets[i]], self.captions[i], [self.names[j] for j in self.groups[i]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", type=int, default=2297)
    ap.add_argument("--queries", type=int, default=4181)
    ap.add_argument("--px", type=int, default=384)
    ap.add_argument("--topk", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = config.BertGeometry(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072, encoder_width=768)
    v = config.VitGeometry(image_size=a.px)
    m1 = BLIP_Retrieval(med_config=g, vit_geometry=v, tokenizer=synthetic.HashTokenizer())
    m1.load_state_dict(weights.synth_state_dict(weights.retrieval_param_spec(g, v), 12, "test"))
    m1 = m1.to(dev).float().eval()
    gen = torch.Generator(device="cpu").manual_seed(5)
    tokens32 = torch.empty((a.index, v.num_tokens, v.width), dtype=torch.float32, device=dev).normal_(0.0, 0.5)
    pooled = torch.nn.functional.normalize(torch.randn((a.index, 256), generator=gen), dim=-1).to(dev)
    bank16 = ops.gather_rows(tokens32, None, m1.token_dtype)
    names = ["img%06d" % (7 * i) for i in range(a.index)]
    groups = np.stack([torch.randperm(a.index, generator=gen)[:6].numpy() for _ in range(a.queries)])       # 6 members, the reference first
    refs, targets = groups[:, 0].copy(), groups[np.arange(a.queries), 1 + np.arange(a.queries) % 5].copy()
    captions = [synthetic.caption_text(q, 4 + q % 27) for q in range(a.queries)]                             # 6-32 tokens
    k = a.topk

    def reference(feats):
        def run(n=a.queries):
            return V1.compute_cirr_val_metrics(CirrVal(names, refs[:n], targets[:n], captions[:n], groups[:n]), m1, feats, pooled, names, topk=k)
        return run

    def native_topk(n=a.queries):
        pred = V1.generate_val_predictions(m1, refs[:n], captions[:n], bank16)
        top, ranks = V1.rank_index_topk(pred, pooled, k, exclude=refs[:n], cols=V1.cirr_rank_cols(refs[:n], targets[:n], groups[:n]))
        return V1.cirr_topk_from_ranks(top.cpu().numpy(), ranks.cpu().numpy(), refs[:n], targets[:n], groups[:n], names, k, "val")

    def native_fullsort(n=a.queries):
        pred = V1.generate_val_predictions(m1, refs[:n], captions[:n], bank16)
        return V1.cirr_topk(V1.rank_index(pred, pooled).cpu().numpy(), refs[:n], targets[:n], groups[:n], names, k, "val")

    forms = {"reference_fp32": reference(tokens32), "reference_bank16": reference(bank16), "native_topk": native_topk}
    if a.index <= 8192:
        forms["native_fullsort"] = native_fullsort
    for fn in forms.values():
        fn(64)
    torch.cuda.synchronize()
    results = {name: fn() for name, fn in forms.items()}
    base = results["native_topk"]
    for name, (metrics, top) in results.items():
        assert metrics == base[0] and (top["sorted_index_names"] == base[1]["sorted_index_names"]).all(), name
        assert torch.equal(top["labels"], base[1]["labels"]) and torch.equal(top["group_labels"], base[1]["group_labels"]), name
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    out = dict(index=a.index, queries=a.queries, px=a.px, tokens=v.num_tokens, topk=k, rounds=a.rounds, metrics=list(base[0]),
               seconds={n: dict(median=statistics.median(t), min=min(t), max=max(t)) for n, t in times.items()})
    for n, t in out["seconds"].items():
        print(f"{n:18s} {t['median']:7.3f} s [{t['min']:.3f} .. {t['max']:.3f}]")
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh)


if __name__ == "__main__":
    main()
