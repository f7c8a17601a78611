"""The grouped / clipped optimizer kernels beside the ones they stand next to, on slab sizes of the stage-II trainer and of the ViT trainer.
Prints only (and --json).

  python tools/optim_bench.py                      both slabs
  options: --slabs text,vit  --rounds 20  --limit 300  --json out.json

Per slab (full-size geometry; the sizes and the parameter order come from weights.nlvr_param_spec, every parameter padded to 8 elements as
train_core._Slab pads it - no model is built):
    cir_grads_check (scale 1: read only)       beside   cir_grads_sumsq                      bytes = 4 n  (one read of g)
    cir_adamw_step_dev                         beside   cir_adamw_step_groups in three configurations:
        1 segment (no table);  the segments train.param_groups gives for that parameter order (no decay on ndim <= 1, pos_embed and
        cls_token; the ViT at lr_scale 0.1);  the same with the clip flag on             bytes = 30 n  (p, m, v read and written, g read,
                                                                                          the 16-bit copy written)
The slab order of the trainers lays the weights of a group of Linears side by side and their biases behind them, so a real slab has FEWER
segments than the spec order used here, which alternates weight and bias: the table timed is the longer one.

Method: every form is launched once before it is timed; the forms alternate inside a round, device events around ONE launch, median over
the rounds with min .. max beside it; every fp32 buffer (772 MiB and 327 MiB) is larger than the 256 MiB Infinity Cache, so a launch
streams from HBM.  Each slab is measured by a child process of its own under `timeout -k 10 <--limit>`; the parent
never opens the GPU and stops at the first child that fails or runs out of time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NO_DECAY = ("visual_encoder.pos_embed", "visual_encoder.cls_token")


def slab_layout(which):
    """(n, segment ends, group ids, number of groups) of the `text` (text_encoder.* + cls_head.*) or the `vit` slab in spec order."""
    from candidate_reranking_cir_amd import config, weights
    spec = weights.nlvr_param_spec(config.BertGeometry(), config.VitGeometry())
    vis = which == "vit"
    ends, ids, o = [], [], 0
    for name, (shape, _) in spec.items():
        if name.startswith("visual_encoder.") != vis or (not vis and not name.startswith(("text_encoder.", "cls_head."))):
            continue
        numel = 1
        for s in shape:
            numel *= s
        o += (numel + 7) // 8 * 8
        gid = int(len(shape) <= 1 or name in NO_DECAY)                 # 0: decayed, 1: not - each slab holds ONE lr_scale
        if ids and ids[-1] == gid:
            ends[-1] = o
        else:
            ends.append(o); ids.append(gid)
    return o, ends, ids, 2


def child(which, rounds, out_path):
    import torch
    from candidate_reranking_cir_amd import train_ops as T
    n, ends, ids, _ = slab_layout(which)
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1)
    p, m = (torch.randn((n,), device=dev, generator=gen) for _ in range(2))
    g = torch.randn((n,), device=dev, generator=gen) * 1e-2
    v = torch.rand((n,), device=dev, generator=gen) * 1e-4
    p16 = torch.empty((n,), dtype=torch.float16, device=dev)
    st = torch.zeros((8,), dtype=torch.int32, device=dev)
    part = torch.empty((T.grads_sumsq_workspace(n),), dtype=torch.float64, device=dev)
    table = T.SegmentTable(ends, ids, dev)
    betas, hp = (0.9, 0.999), (2e-5, 0.05, 1e-8)
    groups = [(2e-5, 0.05, 1e-8), (2e-5, 0.0, 1e-8)]
    if which == "vit":
        groups = [(2e-6, wd, eps) for _, wd, eps in groups]
    T.grads_sumsq(g, st, part)
    T.adamw_begin_clip(st, betas, part, 1.0)                           # t = 1, a coefficient below 1 in state[5]
    forms = {
        "cir_grads_check": (lambda: T.grads_check(g, st), 4),
        "cir_grads_sumsq": (lambda: T.grads_sumsq(g, st, part), 4),
        "cir_adamw_step_dev": (lambda: T.adamw_step_dev(p, g, m, v, st, hp[0], betas, hp[2], hp[1], p16=p16), 30),
        "cir_adamw_step_groups, 1 segment": (lambda: T.adamw_step_groups(p, g, m, v, st, groups, betas, group=0, p16=p16), 30),
        f"cir_adamw_step_groups, {len(ends)} segments": (lambda: T.adamw_step_groups(p, g, m, v, st, groups, betas, table=table, p16=p16), 30),
        f"cir_adamw_step_groups, {len(ends)} segments, clip": (lambda: T.adamw_step_groups(p, g, m, v, st, groups, betas, table=table, clip=True, p16=p16), 30),
    }
    for fn, _ in forms.values():
        fn()
    torch.cuda.synchronize()
    assert int(st[0]) == 0, "the buffers went non-finite: the update kernels would return at once"
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for name, (fn, _) in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    assert int(st[0]) == 0
    rows = []
    for name, (_, bytes_per) in forms.items():
        med = statistics.median(times[name])
        rows.append(dict(slab=which, n=n, segments=len(ends), form=name, us=med, us_min=min(times[name]), us_max=max(times[name]),
                         gbps=bytes_per * n / med / 1e3))
    with open(out_path, "w") as f:
        json.dump(rows, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slabs", default="text,vit")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--json")
    ap.add_argument("--child")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.out)
    rows = []
    for which in a.slabs.split(","):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "rows.json")
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", which, "--rounds", str(a.rounds), "--out", out]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"optim_bench: the {which} child ended with status {rc}; stopping")
                return rc
            rows += json.load(open(out))
    for r in rows:
        print(f"{r['slab']:5s} n={r['n']:>11d} {r['form']:50s} {r['us']:9.1f} us ({r['us_min']:.1f} .. {r['us_max']:.1f})  {r['gbps']:7.0f} GB/s")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
