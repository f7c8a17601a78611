"""Parameter groups and the global-norm clip on a real MI355X against tests/optim_group_cases.py: cir_grads_sumsq (norm, flag, repeatable
partials, workspace), cir_adamw_begin_clip (coefficient bit for bit from the kernel's own norm, counts as cir_adamw_begin's), and
cir_adamw_step_groups (every element inside optim_cases' bound for its own group's scalars; nseg = 1 bit-identical to cir_adamw_step_dev);
train_optim.AdamW with groups and max_grad_norm over flat storages and a transposed parameter, its default form beside the parent's path,
resume in deterministic mode, and one end-to-end step of the tiny stage-II model.  Everything goes through the train_ops wrappers.

As in tests/test_optim_gpu.py every buffer a kernel writes is a flat view between two canary bands, g must come back bit-identical and the
device state sits between canary words."""
import copy
import dataclasses

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import optim_cases as O
from tests import optim_group_cases as G
from tests.test_guard_gpu import CANARY
from tests.test_optim_gpu import BAND, SENTINEL, Flat, State, _i32, _slab

pytestmark = pytest.mark.gpu

F32, F16, BF16 = O.F32, O.F16, O.BF16
_dt = lambda d: "none" if d is None else O.DT_NAME[d]      # noqa: E731
WORD = 0x5A5A5A5A
D_CANARY = 0x7FF8DEADBEEF0BAD                              # a float64 NaN pattern


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    return train_ops


class Partials:
    """k doubles between two BAND-element canary bands."""

    def __init__(self, k):
        self.k = k
        self.big = torch.full((k + 2 * BAND,), D_CANARY, dtype=torch.int64, device="cuda")
        self.view = self.big[BAND:BAND + k].view(torch.float64)

    def written(self):
        """(every one of the k doubles was written, both bands intact)."""
        b = self.big.cpu()
        return bool((b[BAND:BAND + self.k] != D_CANARY).all()), bool((b[:BAND] == D_CANARY).all()) and bool((b[BAND + self.k:] == D_CANARY).all())


def read_state(st):
    """(the 8 words, canary words and state[7] intact) of a test_optim_gpu.State whose [5] and [6] the clip kernels may write."""
    b = st.big.cpu()
    return b[8:16].tolist(), bool((b[:8] == WORD).all()) and bool((b[16:] == WORD).all()) and int(b[15]) == SENTINEL[2]


def f32_of(word):
    return np.array(word, dtype=np.int32).view(np.float32)[()]


# ------------------------------------------------------------------------------------------------ cir_grads_sumsq
SUMSQ_CAP = 1024
# every workgroup of the full grid takes a second trip (5 strides of float4 and 257 more), the finishing sum reads 4 partials per thread
# and folds 256 of them; a 3-element tail
LONG_N = 4 * (5 * SUMSQ_CAP * 256 + 257) + 3
SUMSQ_LENGTHS = O.DEV_LENGTHS + (LONG_N,)


def _grid(n):
    return min(max(-(-(n // 4) // 1024), 1), SUMSQ_CAP)


def _magnitudes(n, shift=0):
    """|g| in 0, 1e-30 ... 1e15 (optim_cases.G_ABS), both signs, laid through n elements."""
    i = torch.arange(n) + shift
    mag = torch.tensor(np.array(O.G_ABS, dtype=np.float64).astype(np.float32))[i % len(O.G_ABS)]
    return torch.where((i // len(O.G_ABS)) % 2 == 0, mag, -mag)


def test_sumsq_lengths_cover_the_grid(T):
    assert _grid(LONG_N) == SUMSQ_CAP and LONG_N // 4 > 5 * SUMSQ_CAP * 256 and LONG_N % 4 == 3
    for n in SUMSQ_LENGTHS + (4096, 4100, 4 * 1024 * 1024 + 4):
        assert T.grads_sumsq_workspace(n) == _grid(n), n


@pytest.mark.parametrize("n", SUMSQ_LENGTHS)
def test_grads_sumsq(T, n):
    g_cpu = _magnitudes(n, shift=n % 5)
    want = G.norm32([g_cpu.numpy()])
    k = T.grads_sumsq_workspace(n)
    g = Flat(n, F32, g_cpu)
    runs = []
    for preset in (0, 1):                                                                      # a clean buffer leaves a preset flag alone
        part, st = Partials(k), State(flag=preset, t=7, skipped=3, bc=(41, 42))
        T.grads_sumsq(g.view, st.st, part.view)
        words, ok = st.read()                                                                  # (state[1..7] untouched: sentinels included)
        assert ok and words[:5] == [preset, 7, 3, 41, 42], (n, words)
        written, intact = part.written()
        assert written and intact, (n, "the workspace query is not the number of doubles written")
        runs.append(part.view.cpu())
    assert torch.equal(runs[0], runs[1])                                                       # bit-repeatable partials
    got = np.float32(np.sqrt(float(runs[0].sum())))
    print(f"cir_grads_sumsq n={n}: {k} partials, norm {got!r} (float64 reference {want!r}, {G.ulps32(got, want)} ulp)")
    assert G.ulps32(got, want) <= G.NORM_ULPS
    assert torch.equal(g.bits().cpu(), g_cpu.view(torch.int32)) and g.intact()                 # g is only read
    # an inf or a NaN at the first element, the last element of the float4 body and each tail position sets the flag
    n4 = n // 4
    spots = {0, n - 1} | ({4 * n4 - 1} if n4 else set()) | set(range(4 * n4, n))
    for j, pos in enumerate(sorted(spots)):
        bits = g_cpu.view(torch.int32).clone()
        bits[pos] = _i32((0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001)[j % 4])
        bad, part, st = Flat(n, F32, bits.view(torch.float32)), Partials(k), State()
        T.grads_sumsq(bad.view, st.st, part.view)
        words, ok = st.read()
        assert ok and words[0] == 1 and words[1:5] == [0, 0, 0, 0], (n, pos, words)
        assert torch.equal(bad.bits().cpu(), bits) and bad.intact() and part.written()[1]


# ------------------------------------------------------------------------------------------------ cir_adamw_begin_clip
def _partials(sizes, total):
    """Positive doubles for work items of `sizes` partials each, side by side, scaled so that their float64 sum is close to `total`."""
    gen = torch.Generator().manual_seed(sum(sizes))
    x = torch.rand((sum(sizes),), generator=gen, dtype=torch.float64) + 0.5
    return x * (total / float(x.sum()))


@pytest.mark.parametrize("sizes", [(1, 3), (1024, 2, 300)], ids=["two_items", "three_items"])
def test_adamw_begin_clip(T, sizes):
    betas = (0.9, 0.999)
    for sumsq in (9.0, 1e-12, 2.5e31):
        part_cpu = _partials(sizes, sumsq)
        ref_norm = np.float32(np.sqrt(float(part_cpu.sum())))
        # norm above, at and below max_norm
        for which, max_norm in (("above", float(ref_norm) * 0.5), ("at", float(ref_norm)), ("below", float(ref_norm) * 3.0)):
            part = Partials(sum(sizes))
            part.view.copy_(part_cpu)
            st, twin = State(t=4, skipped=2, bc=(41, 42)), State(t=4, skipped=2, bc=(41, 42))
            T.adamw_begin_clip(st.st, betas, part.view, max_norm)
            T.adamw_begin(twin.st, betas)
            words, ok = read_state(st)
            assert ok and words[:5] == twin.read()[0][:5] and words[:3] == [0, 5, 2], (which, words)      # t / skipped / bc1 / bc2 as cir_adamw_begin
            norm, coef = f32_of(words[6]), f32_of(words[5])
            assert G.ulps32(norm, ref_norm) <= G.NORM_ULPS, (which, norm, ref_norm)
            assert coef.tobytes() == G.coef32(norm, max_norm).tobytes(), (which, coef, G.coef32(norm, max_norm))   # from the kernel's OWN norm
            # (at: 1 or under it - half of it where the norm is of the order of the 1e-6 itself)
            assert (coef < 1.0) if which == "above" else (coef == 1.0 if which == "below" else 0.49 < coef <= 1.0)
            assert torch.equal(part.view.cpu(), part_cpu) and part.written()[1]
    # a set flag: skipped += 1, t and both corrections stay, state[6] = the norm as summed (inf / NaN possible), state[5] = 0
    for poison, test in ((None, lambda x: x == np.float32(3.0)), (float("inf"), np.isinf), (float("nan"), np.isnan)):
        part_cpu = _partials(sizes, 9.0)
        if poison is not None:
            part_cpu[sizes[0]] = poison
        part = Partials(sum(sizes))
        part.view.copy_(part_cpu)
        st = State(flag=1, t=4, skipped=2, bc=(41, 42))
        T.adamw_begin_clip(st.st, betas, part.view, 1.0)
        words, ok = read_state(st)
        assert ok and words[:5] == [1, 4, 3, 41, 42] and f32_of(words[5]) == 0.0, words
        norm = f32_of(words[6])
        assert test(norm) if poison is not None else G.ulps32(norm, np.float32(3.0)) <= G.NORM_ULPS, (poison, norm)


# ------------------------------------------------------------------------------------------------ cir_adamw_step_groups
def _run_scenario(T, scn, p16, clip_flag=True):
    """A scenario through the three kernels: (norms, coefs, outputs per item, failures of everything that is not the bounded comparison)."""
    items = scn.inputs()
    st = State(t=scn.t - 1)
    clip = scn.max_norm is not None and clip_flag
    sizes = [T.grads_sumsq_workspace(i["g"].numel()) for i in items]
    part = Partials(sum(sizes))
    bufs = [{k: Flat(i[k].numel(), F32, i[k]) for k in "pgmv"} for i in items]
    fails = []
    if clip:
        o = 0
        for b, k in zip(bufs, sizes):
            T.grads_sumsq(b["g"].view, st.st, part.view[o:o + k])
            o += k
        T.adamw_begin_clip(st.st, (G.B1, G.B2), part.view, scn.max_norm)
    else:
        T.adamw_begin(st.st, (G.B1, G.B2))
    words, ok = read_state(st)
    if not ok or words[:3] != [0, scn.t, 0]:
        fails.append(f"{scn}: state {words} after the begin")
    sc = G.applied(scn.groups)
    outs = []
    for j, (i, b) in enumerate(zip(items, bufs)):
        n = i["p"].numel()
        h = Flat(n, p16) if p16 is not None else None
        # (a buffer of one segment whose length a table cannot describe goes without one, as a per-tensor work item does)
        table = None if len(i["ends"]) == 1 and n % 8 else T.SegmentTable(i["ends"], i["ids"], "cuda")
        T.adamw_step_groups(b["p"].view, b["g"].view, b["m"].view, b["v"].view, st.st, sc, (G.B1, G.B2), table=table, group=i["ids"][0],
                            clip=clip, p16=None if h is None else h.view)
        out = {k: b[k].view.cpu() for k in "pmv"}
        outs.append(out)
        if not torch.equal(b["g"].bits().cpu(), i["g"].view(torch.int32)):
            fails.append(f"{scn} item {j}: the gradient was written to")
        fails += [f"{scn} item {j}: canary of {k} overwritten" for k, x in b.items() if not x.intact()]
        if h is not None:
            want = out["p"].to(p16).view(torch.int16)                                          # RNE of the kernel's OWN p'
            if not h.intact() or not torch.equal(h.bits().cpu(), want):
                fails.append(f"{scn} item {j}: p16 is not the {_dt(p16)} rounding of p' (or its canary is gone)")
    words2, ok2 = read_state(st)
    if not ok2 or words2 != words:
        fails.append(f"{scn}: the update kernel wrote to the state: {words} -> {words2}")
    if clip:
        norm, coef = f32_of(words[6]), f32_of(words[5])
    else:                                                                                      # (no norm was taken: the reference's stands in)
        norm, coef = G.reference(scn)[0], None
    return [norm] * len(items), [coef] * len(items), outs, fails


STEP_CASES = [(name, p16) for name in sorted(G.SCENARIOS) for p16 in (F16, BF16, None)]


@pytest.mark.parametrize("name,p16", STEP_CASES, ids=[f"{n}-{_dt(p)}" for n, p in STEP_CASES])
def test_adamw_step_groups(T, name, p16):
    scn = G.SCENARIOS[name]
    norms, coefs, outs, fails = _run_scenario(T, scn, p16)
    fails += G.check(scn, norms, coefs, outs)
    _, _, terms = G.reference(scn)
    worst = {k: max(O.worst_ratio(scn, {k: out[k]}, ref, bnd) for out, (ref, bnd) in zip(outs, terms)) for k in "pmv"}
    print(f"cir_adamw_step_groups {name} {_dt(p16)}: worst |error| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(worst.items())))
    assert not fails, fails[:10]


def test_adamw_step_groups_clip_flag_off_ignores_the_coefficient(T):
    """The same tables without the clip flag: the gradient is applied as it is, whatever state[5] holds."""
    scn = copy.copy(G.SCENARIOS["clip_active"])
    scn._max_norm = None
    items = scn.inputs()
    st = State(t=scn.t - 1)
    T.adamw_begin(st.st, (G.B1, G.B2))
    st.st[5] = _i32(0x3E000000)                                                                # 0.125 where a coefficient would be
    outs = []
    for i in items:
        b = {k: Flat(i[k].numel(), F32, i[k]) for k in "pgmv"}
        T.adamw_step_groups(b["p"].view, b["g"].view, b["m"].view, b["v"].view, st.st, G.applied(scn.groups), (G.B1, G.B2),
                            table=T.SegmentTable(i["ends"], i["ids"], "cuda"), clip=False)
        outs.append({k: b[k].view.cpu() for k in "pmv"})
    norm = G.reference(scn)[0]
    fails = G.check(scn, [norm] * len(items), [None] * len(items), outs)
    assert not fails, fails[:10]


@pytest.mark.parametrize("n", [1, 7, 1027, 2051])
@pytest.mark.parametrize("p16", [F16, BF16, None], ids=_dt)
def test_one_segment_without_clip_has_the_bits_of_adamw_step_dev(T, n, p16):
    c = next(c for c in O.CASES["adamw_dev"] if c.n == n and c.t == 2 and c.hp == 1 and c.wd == 1 and c.p16 == F16)
    i, (lr, b1, b2, eps, wd) = O.inputs(c), O.hyper(c)
    got = []
    for form in ("dev", "groups"):
        buf = {k: Flat(n, F32, i[k]) for k in "pgmv"}
        h = Flat(n, p16) if p16 is not None else None
        st = State(t=c.t - 1)
        T.adamw_begin(st.st, (b1, b2))
        if form == "dev":
            T.adamw_step_dev(buf["p"].view, buf["g"].view, buf["m"].view, buf["v"].view, st.st, lr, (b1, b2), eps, wd, p16=None if h is None else h.view)
        else:                                                                                  # the group in use is the LAST of three
            T.adamw_step_groups(buf["p"].view, buf["g"].view, buf["m"].view, buf["v"].view, st.st, [(0.5, 0.5, 0.5), (0.25, 0.0, 1.0), (lr, wd, eps)],
                                (b1, b2), group=2, p16=None if h is None else h.view)
        assert all(b.intact() for b in buf.values()) and (h is None or h.intact()) and st.read()[1]
        assert torch.equal(buf["g"].bits().cpu(), i["g"].view(torch.int32))
        got.append({k: buf[k].bits().cpu() for k in "pmv"} | ({} if h is None else {"p16": h.bits().cpu()}))
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), (n, k, int((got[0][k] != got[1][k]).sum()))
    assert not torch.equal(got[0]["p"], i["p"].view(torch.int32))


@pytest.mark.parametrize("form", ["table", "one_segment"])
def test_step_groups_under_a_set_flag_changes_nothing(T, form):
    scn = G.SCENARIOS["clip_active"]
    i = scn.inputs()[0]
    n = i["p"].numel() if form == "table" else 2051
    src = {k: i[k][:n].clone() for k in "pgmv"}
    buf = {k: Flat(n, F32, src[k]) for k in "pgmv"}
    h = Flat(n, F16)
    st = State(flag=1, t=3, skipped=1, bc=(41, 42))
    before = read_state(st)[0]
    table = T.SegmentTable(i["ends"], i["ids"], "cuda") if form == "table" else None
    T.adamw_step_groups(buf["p"].view, buf["g"].view, buf["m"].view, buf["v"].view, st.st, G.applied(scn.groups), (G.B1, G.B2), table=table,
                        group=1, clip=True, p16=h.view)
    words, ok = st.read()
    assert ok and words == before
    for k in "pgmv":
        assert torch.equal(buf[k].bits().cpu(), src[k].view(torch.int32)) and buf[k].intact(), k
    assert bool((h.big.view(torch.int16) == CANARY[F16]).all())                                # not one element of the 16-bit copy written


# ------------------------------------------------------------------------------------------------ train_optim.AdamW
def _moderate_grads(params, k):
    """Gradients like the scenarios' (+-[2^-12, 2^4)), written INTO the installed buffers."""
    gen = torch.Generator().manual_seed(900 + k)
    for p in params:
        if p.grad is not None:
            g = torch.randn(p.shape, generator=gen) * torch.exp2(torch.randint(-12, 4, p.shape, generator=gen).float())
            p.grad.copy_(g.cuda())


def _count(T, monkeypatch, names):
    calls = {n: 0 for n in names}
    for name in names:
        real = getattr(T, name)
        monkeypatch.setattr(T, name, (lambda real, name: lambda *a, **k: (calls.__setitem__(name, calls[name] + 1), real(*a, **k))[1])(real, name))
    return calls


ENTRY_POINTS = ("adamw_begin", "adamw_step_dev", "grads_check", "grads_sumsq", "adamw_begin_clip", "adamw_step_groups")


def _three_groups(slab_a, slab_b, tr):
    """decay / no-decay / lr_scale 0.1, mixed through both storages; the transposed parameter in the scaled group."""
    return [{"params": [slab_a[0], slab_b[1]]}, {"params": [slab_a[1], slab_b[0]], "weight_decay": 0.0},
            {"params": [slab_a[2], tr], "lr_scale": 0.1, "eps": 1e-6}]


def _build(seed=0):
    slab_a, _ = _slab([(5, 7), (16,), (3, 3)], seed)
    slab_b, _ = _slab([(9,), (2, 260)], seed + 5)
    tr = torch.nn.Parameter((O.REGIMES[0][torch.arange(6 * 10) % O.N_REGIMES].view(6, 10).cuda()).t())           # (10, 6), transposed
    tr.grad = torch.zeros_like(tr)
    assert not tr.is_contiguous()
    return slab_a, slab_b, tr


def test_adamw_class_with_groups_and_clipping(T, monkeypatch):
    from candidate_reranking_cir_amd.train_optim import AdamW
    slab_a, slab_b, tr = _build()
    params = slab_a + slab_b + [tr]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    _moderate_grads(params, 0)
    first_norm = float(G.norm32([p.grad.cpu().numpy() for p in params]))
    opt = AdamW(_three_groups(slab_a, slab_b, tr), max_grad_norm=0.5 * first_norm, **kw)
    group_of = {id(p): k for k, g in enumerate(opt.param_groups) for p in g["params"]}
    calls = _count(T, monkeypatch, ENTRY_POINTS)

    def snapshot():
        torch.cuda.synchronize()
        return [(p.detach().cpu().clone(), opt.m[id(p)].cpu().clone() if id(p) in opt.m else torch.zeros(p.shape),
                 opt.v[id(p)].cpu().clone() if id(p) in opt.v else torch.zeros(p.shape)) for p in params]

    worst, t = {}, 0
    for k, lr in enumerate((1e-2, 1e-2, 1e-3, 1e-3)):
        for g in opt.param_groups:                                                             # (as a schedule writes it: every group's lr)
            g["lr"] = lr
        _moderate_grads(params, k)
        before = snapshot()
        if k == 1:                                                                             # the ONE skipped step: an inf in the LAST work item
            tr.grad[3, 2] = float("inf")
        for name in calls:
            calls[name] = 0
        opt.step()
        # two flat storages + one tensor: one norm pass and one step per work item, ONE begin, nothing of the one-group path
        assert calls == dict(adamw_begin=0, adamw_step_dev=0, grads_check=0, grads_sumsq=3, adamw_begin_clip=1, adamw_step_groups=3), calls
        after = snapshot()
        if k == 1:
            assert opt.t == t and opt.skipped_steps == 1 and opt.clip_coef == 0.0 and not np.isfinite(opt.grad_norm)
            for (p0, m0, v0), (p1, m1, v1) in zip(before, after):
                assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(m0, m1) and torch.equal(v0, v1)
            continue
        t += 1
        assert opt.t == t and opt.skipped_steps == (1 if k > 1 else 0)
        grads = [p.grad.cpu() for p in params]
        want = G.norm32([g.numpy() for g in grads])
        norm, coef = np.float32(opt.grad_norm), np.float32(opt.clip_coef)
        assert G.ulps32(norm, want) <= G.NORM_ULPS, (k, norm, want)                            # ONE global norm over all three work items
        assert coef.tobytes() == G.coef32(norm, opt.max_grad_norm).tobytes() and coef < 1.0
        if k == 0:
            assert 0.49 < coef < 0.51
        sc = G.applied(opt.param_groups)
        assert sc[2][0] == O.f32(lr * 0.1) and sc[1][1] == 0.0 and sc[2][2] == O.f32(1e-6)
        for j, (p, g, (p0, m0, v0), (p1, m1, v1)) in enumerate(zip(params, grads, before, after)):
            eg = torch.full((p.numel(),), group_of[id(p)], dtype=torch.int64)
            ref, bnd = G.group_step_terms(p0.flatten(), g.flatten(), m0.flatten(), v0.flatten(), eg, sc, t, coef)
            out = dict(p=p1.flatten(), m=m1.flatten(), v=v1.flatten())
            fails = G.check_step(f"AdamW.step {k + 1} parameter {j} {tuple(p.shape)}", out, ref, bnd)
            assert not fails, fails
            for name in "pmv":
                worst[name] = max(worst.get(name, 0.0), O.worst_ratio("AdamW", {name: out[name]}, ref, bnd))
    assert len(opt._flats) == 2 and sorted(tb[1].nseg for tb in opt._tables.values()) == [2, 3]
    print("train_optim.AdamW with groups and clipping, 3 applied steps: worst |error| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(worst.items())))


def test_adamw_class_one_group_with_clipping_only(T, monkeypatch):
    """AdamW(params, max_grad_norm=x): ONE group, so every work item - two flat storages, one tensor - steps without a table, with the
    clip on: one norm pass and one update per work item, one begin, no cir_grads_check; each step inside the bound from the kernel's own
    previous state."""
    from candidate_reranking_cir_amd.train_optim import AdamW
    slab_a, slab_b, tr = _build(21)
    params = slab_a + slab_b + [tr]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    _moderate_grads(params, 0)
    opt = AdamW(params, max_grad_norm=0.5 * float(G.norm32([p.grad.cpu().numpy() for p in params])), **kw)
    assert len(opt.param_groups) == 1 and opt._grouped()
    calls = _count(T, monkeypatch, ENTRY_POINTS)
    sc = G.applied(opt.param_groups)
    assert sc == [tuple(O.f32(x) for x in (1e-2, 0.05, 1e-8))]
    worst = {}
    for k in range(2):
        _moderate_grads(params, k)
        torch.cuda.synchronize()
        before = [(p.detach().cpu().clone(), opt.m[id(p)].cpu().clone() if id(p) in opt.m else torch.zeros(p.shape),
                   opt.v[id(p)].cpu().clone() if id(p) in opt.v else torch.zeros(p.shape)) for p in params]
        for name in calls:
            calls[name] = 0
        opt.step()
        assert calls == dict(adamw_begin=0, adamw_step_dev=0, grads_check=0, grads_sumsq=3, adamw_begin_clip=1, adamw_step_groups=3), calls
        grads = [p.grad.cpu() for p in params]
        norm, coef = np.float32(opt.grad_norm), np.float32(opt.clip_coef)
        assert opt.t == k + 1 and opt.skipped_steps == 0
        assert G.ulps32(norm, G.norm32([g.numpy() for g in grads])) <= G.NORM_ULPS
        assert coef.tobytes() == G.coef32(norm, opt.max_grad_norm).tobytes() and coef < 1.0
        for j, (p, g, (p0, m0, v0)) in enumerate(zip(params, grads, before)):
            eg = torch.zeros((p.numel(),), dtype=torch.int64)
            ref, bnd = G.group_step_terms(p0.flatten(), g.flatten(), m0.flatten(), v0.flatten(), eg, sc, k + 1, coef)
            out = dict(p=p.detach().cpu().flatten(), m=opt.m[id(p)].cpu().flatten(), v=opt.v[id(p)].cpu().flatten())
            fails = G.check_step(f"one-group AdamW.step {k + 1} parameter {j} {tuple(p.shape)}", out, ref, bnd)
            assert not fails, fails
            for name in "pmv":
                worst[name] = max(worst.get(name, 0.0), O.worst_ratio("AdamW", {name: out[name]}, ref, bnd))
    assert len(opt._flats) == 2 and all(tb[1] is None for tb in opt._tables.values())         # one group: no table anywhere
    print("train_optim.AdamW, one group with clipping, 2 steps: worst |error| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(worst.items())))


def test_default_optimizer_takes_the_parents_path(T, monkeypatch):
    """One group, no clipping: cir_adamw_begin / cir_grads_check / cir_adamw_step_dev and none of the new entry points; after two steps the
    parameters equal a twin stepped by those three calls written out by hand."""
    from candidate_reranking_cir_amd.train_optim import AdamW
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    ps, _ = _slab([(5, 7), (16,), (2, 260)], 3)
    qs, qg = _slab([(5, 7), (16,), (2, 260)], 3)
    opt = AdamW(ps, **kw)
    calls = _count(T, monkeypatch, ENTRY_POINTS)
    n = qg.numel()
    qflat = torch.empty(0, device="cuda").set_(qs[0].data.untyped_storage(), 0, (n,))
    m, v, st = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    for k in range(2):
        _moderate_grads(ps, k)
        _moderate_grads(qs, k)
        for name in calls:
            calls[name] = 0
        opt.step()
        assert calls == dict(adamw_begin=1, adamw_step_dev=1, grads_check=1, grads_sumsq=0, adamw_begin_clip=0, adamw_step_groups=0), calls
        st[0:1].zero_()
        T.grads_check(qg, st)
        T.adamw_begin(st, kw["betas"])
        T.adamw_step_dev(qflat, qg, m, v, st, kw["lr"], kw["betas"], kw["eps"], kw["weight_decay"])
    assert opt.t == 2 and all(torch.equal(p, q) for p, q in zip(ps, qs)) and not torch.equal(ps[0].cpu(), _slab([(5, 7)], 3)[0][0].cpu())
    assert torch.equal(opt._state[5:8].cpu(), torch.zeros(3, dtype=torch.int32))              # the one-group path leaves state[5..7] alone


def test_resume_with_groups_and_clipping_in_deterministic_mode(T):
    from candidate_reranking_cir_amd.train_optim import AdamW
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_grad_norm=3.0)
    was = T.deterministic()
    T.set_deterministic(True)
    try:
        runs = []
        for resume in (False, True):
            slab_a, slab_b, tr = _build(11)
            params = slab_a + slab_b + [tr]
            opt = AdamW(_three_groups(slab_a, slab_b, tr), **kw)
            for k in range(4):
                if resume and k == 2:
                    sd = copy.deepcopy(opt.state_dict())
                    assert sd["cir"]["max_grad_norm"] == 3.0 and len(sd["param_groups"]) == 3
                    opt = AdamW(_three_groups(slab_a, slab_b, tr), lr=1.0, betas=(0.9, 0.999), eps=1.0, weight_decay=0.3)
                    opt.load_state_dict(sd)
                    assert opt.max_grad_norm == 3.0 and opt.t == 2
                _moderate_grads(params, k)
                opt.step()
                assert 0.0 < opt.clip_coef < 1.0
            assert opt.t == 4
            runs.append([(p.detach().clone(), opt.m[id(p)].clone(), opt.v[id(p)].clone()) for p in params])
        for a, b in zip(*runs):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    finally:
        T.set_deterministic(was)


def test_tiny_stage2_model_end_to_end(T):
    """train.param_groups with image tuning on, max_grad_norm 1, two steps of the tiny stage-II model: both slabs step through the segmented
    kernel, the 16-bit slab copies are the rounding of the stepped parameters, and the packed inference engines see the updated weights
    (the eval-mode logits change and equal those of a fresh model loaded with the stepped state dict)."""
    from candidate_reranking_cir_amd import train
    from tests.test_weight_coherence_gpu import _check_eval, _check_slab, _inputs, _nlvr, _score, _train_step
    z, g, v, sd2, _ = H.tiny_setup()
    geo = dict(g=g, v=dataclasses.replace(v, drop_path_rate=0.0), sd2=sd2)
    m = _nlvr(geo, sd2, "f16")
    x = _inputs(geo)
    before = _score(m, x).clone()
    groups = train.param_groups(m, 0.05, {"visual_encoder.": 0.1})
    assert len(groups) == 4
    opt = train.AdamW(groups, lr=1e-3, model=m, max_grad_norm=1.0)
    for _ in range(2):
        opt.zero_grad()
        _train_step(m, x, img_tune=True)
        opt.step()
    assert opt.t + opt.skipped_steps == 2 and opt.t >= 1 and np.isfinite(opt.grad_norm) and 0.0 < opt.clip_coef <= 1.0
    assert len(opt._flats) == 2 and all(tb[1] is not None and tb[1].nseg > 1 for tb in opt._tables.values())
    for tr in (m._trainer, m._vit_trainer):                                                    # the step wrote the 16-bit copy along
        assert torch.equal(tr.slab.flat16, tr.slab.flat32.to(tr.slab.dtype))
    f = _check_eval(m, geo, "f16", x)
    assert not torch.equal(before, _score(f, x))
    _train_step(m, x, img_tune=True)                                                           # (the next step refreshes the transposed twin)
    _check_slab(m._trainer), _check_slab(m._vit_trainer)
