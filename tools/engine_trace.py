"""Launch traces of `NlvrEngine.forward` on a CPU, for comparing two trees of this repository (LABNOTES.md section 17).

  PYTHONPATH=<tree A> python tools/engine_trace.py dump a.json
  PYTHONPATH=<tree B> python tools/engine_trace.py dump b.json
  python tools/engine_trace.py compare a.json b.json

`dump` packs a set of small engines from seeded synthetic weights, runs each through a set of calls with `ops` replaced by the recording
stubs of tests/engine_stub.py (always this tree's), and stores per (engine, call) the SHA-256 of the trace, its length, the logits' shape, how
far `fold_fallbacks` moved, how many "projected" warnings were raised, or the exception.  `compare` asserts that two such files are equal."""
import hashlib
import importlib.util
import json
import os
import sys

import pytest
import torch


def _stub():
    spec = importlib.util.spec_from_file_location("engine_stub", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "engine_stub.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def engines():
    from candidate_reranking_cir_amd import engine as E
    from candidate_reranking_cir_amd import weights
    from candidate_reranking_cir_amd.config import BertGeometry, VitGeometry
    f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32

    def make(layers=4, width=768, merge_from=2, **kw):
        heads = width // 64
        geo = BertGeometry(hidden_size=width, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=4 * width if width == 768 else 256,
                           encoder_width=width, merge_mlp_from_layer=merge_from)
        vit = VitGeometry(image_size=64, patch_size=16, width=width, depth=1, num_heads=heads)
        sd = weights.synth_state_dict(weights.nlvr_param_spec(geo, vit), 1)
        kw.setdefault("dtype", f16)
        return E.NlvrEngine(sd, geo, kw.pop("dtype"), torch.device("cpu"), **kw)

    yield "f16", make()
    yield "bf16", make(dtype=bf16)
    yield "mixed", make(cross_dtype=bf16)
    yield "stream32", make(stream_dtype=f32)
    e = make()
    e.stream32_from = 2
    yield "stream32_from2", e
    yield "text32x3", make(dtype=f32, stream_dtype=f32, cross_dtype=f16, split3=3)
    yield "text32", make(dtype=f32, stream_dtype=f32, cross_dtype=f16, split3=8)
    yield "exact", make(dtype=f32, stream_dtype=f32, fold_merge=False)
    yield "unfolded_merge", make(fold_merge=False)
    yield "1layer", make(layers=1, merge_from=0)
    yield "2layer", make(layers=2, merge_from=1)
    yield "w128", make(width=128)
    yield "w128_text32", make(width=128, dtype=f32, stream_dtype=f32, cross_dtype=f16, split3=8)


SWITCHES = [("trim_last", False), ("fold_cls_kv", False), ("fold_cross_kv", False), ("fold_long", True), ("kv_chunk", 2), ("cls_fold", None)]


# K/V bank cases: (fold_cls_kv while the bank is built, fold_cls_kv during the call); "foreign": a bank that is not this engine's
BANKS = {"bank": (True, True), "bank_full": (False, False), "bank_full_foldon": (False, True), "bank_mismatch": (True, False), "bank_foreign": (True, True)}


def calls():
    """(name, call arguments of run_forward, attributes set for the call)"""
    for l in (8, 32, 33, 40, 64, 65):
        for n in (5, 197, 224, 225, 577, 608, 609):
            for masked in (False, True):
                yield f"L{l}_N{n}_m{int(masked)}", dict(l=l, n=n, cand_mask=masked), {}
    for l, n in ((32, 197), (40, 197), (40, 225), (65, 577)):
        for masked in (False, True):
            for name, value in SWITCHES:
                yield f"L{l}_N{n}_m{int(masked)}_{name}", dict(l=l, n=n, cand_mask=masked), {name: value}
            yield f"L{l}_N{n}_m{int(masked)}_long_chunk", dict(l=l, n=n, cand_mask=masked), {"fold_long": True, "kv_chunk": 2}
            yield f"L{l}_N{n}_m{int(masked)}_taps", dict(l=l, n=n, cand_mask=masked, taps=True), {}
            for bank in BANKS:
                yield f"L{l}_N{n}_m{int(masked)}_{bank}", dict(l=l, n=n, cand_mask=masked, bank=bank), {}
    yield "dv_other", dict(l=32, n=197, dv=512), {}


def run(stub_mod, name, eng, args, attrs):
    from candidate_reranking_cir_amd import engine as E
    args = dict(args)
    saved = {k: getattr(eng, k) for k in attrs}
    saved["fold_cls_kv"] = eng.fold_cls_kv
    q_n, k, n = 2, 3, args["n"]
    before = eng.fold_fallbacks
    rec = {}
    try:
        for key, v in attrs.items():
            setattr(eng, key, v)
        bank = args.pop("bank", None)
        if bank:
            # the bank itself is built with the real (torch-only on a CPU) packing replaced by the stubs too: its K|V GEMMs are not traced
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(E, "ops", stub_mod.StubOps())
                eng.fold_cls_kv = BANKS[bank][0] and saved["fold_cls_kv"]
                kv = eng.build_kv_bank(torch.zeros((4, n, eng.geo.encoder_width), dtype=eng.xdtype))
                eng.fold_cls_kv = BANKS[bank][1] and saved["fold_cls_kv"]
                if bank == "bank_foreign":
                    kv.engine = None
            args.update(kv_bank=kv, cand_rows=torch.tensor([0, 3, 1, 1, 2, 0]))
        if args.pop("taps", False):
            args["taps"] = []
        with pytest.MonkeyPatch.context() as mp:
            try:
                stub, out, warned = stub_mod.run_forward(eng, mp, q_n=q_n, k=k, **args)
                rec = dict(sha=hashlib.sha256(repr(stub.trace).encode()).hexdigest(), launches=len(stub.trace), out=list(out.shape),
                           warned=sum("projected" in str(x.message) for x in warned), taps=len(args.get("taps") or []))
            except Exception as e:                     # the refusals are part of the behaviour compared
                rec = dict(error=f"{type(e).__name__}: {e}")
    finally:
        for key, v in saved.items():
            setattr(eng, key, v)
    rec["fallbacks"] = eng.fold_fallbacks - before
    return rec


def dump(path):
    stub_mod = _stub()
    import candidate_reranking_cir_amd
    result = {"tree": os.path.dirname(os.path.abspath(candidate_reranking_cir_amd.__file__))}
    for ename, eng in engines():
        eng.fold_fallbacks = 0
        for cname, args, attrs in calls():
            result[f"{ename}/{cname}"] = run(stub_mod, cname, eng, args, attrs)
        result[f"{ename}/fold_fallbacks"] = eng.fold_fallbacks
        print(ename, "done", flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=0, sort_keys=True)


def compare(a, b):
    ra, rb = json.load(open(a)), json.load(open(b))
    print("trees:", ra.pop("tree"), "|", rb.pop("tree"))
    diff = [k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    pairs = [k for k in ra if isinstance(ra[k], dict)]
    print(f"{len(pairs)} (engine, call) pairs: {sum('sha' in ra[k] for k in pairs)} traces, {sum('error' in ra[k] for k in pairs)} refusals, "
          f"{sum(ra[k]['launches'] for k in pairs if 'sha' in ra[k])} launches, fold_fallbacks moved {sum(ra[k]['fallbacks'] for k in pairs)} times, "
          f"{sum(ra[k].get('warned', 0) for k in pairs)} warnings; {len(diff)} differ")
    for k in diff[:20]:
        print("  ", k, ra.get(k), rb.get(k))
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3])
