"""The optimizer step on a real MI355X against the float64 reference and the a-priori bounds of tests/optim_cases.py: cir_adamw_step_dev and
cir_adamw_step on every regime, hyperparameter set, step count and length of the table; cir_adamw_begin's counts and bias corrections; a
chained run whose reference restarts from the kernel's own state at every step; cir_grads_check on bit patterns, scales and positions,
with ONE buffer long enough for a second trip of its loop; and train_optim.AdamW over flat storages, a transposed parameter, a misaligned
one and one without a gradient.  Everything goes through the train_ops wrappers.

Every buffer a kernel writes (p, m, v, p16; g for cir_grads_check) is a flat view between two 64-element canary bands (256 bytes: the
views keep the 16-byte alignment the entry points demand at every length), g of the update kernels must come back bit-identical, and the
device state sits between canary words.  Each group prints its worst |error| / bound per output."""
import time

import numpy as np
import pytest
import torch

from tests import optim_cases as O
from tests.test_guard_gpu import _INT, CANARY

pytestmark = pytest.mark.gpu

F32, F16, BF16 = O.F32, O.F16, O.BF16
BAND = 64
_dt = lambda d: "none" if d is None else O.DT_NAME[d]      # noqa: E731
SENTINEL = (0x11111111, 0x22222222, 0x33333333)           # state[5..7]: no kernel touches them


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import train_ops
    return train_ops


class Flat:
    """n elements between two BAND-element canary bands of one flat allocation."""

    def __init__(self, n, dtype, src=None):
        self.n, self.dtype = n, dtype
        self.big = torch.empty((n + 2 * BAND,), dtype=dtype, device="cuda")
        self.big.view(_INT[dtype]).fill_(CANARY[dtype])
        self.view = self.big[BAND:BAND + n]
        assert self.view.data_ptr() % 16 == 0
        if src is not None:
            self.bits().copy_(src.view(_INT[dtype]))

    def bits(self):
        return self.view.view(_INT[self.dtype])

    def intact(self):
        b = self.big.view(_INT[self.dtype])
        return bool((b[:BAND] == CANARY[self.dtype]).all()) and bool((b[BAND + self.n:] == CANARY[self.dtype]).all())


class State:
    """The 8-word device state between canary words; [5..7] hold sentinels."""

    def __init__(self, flag=0, t=0, skipped=0, bc=(0, 0)):
        self.big = torch.full((24,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.st = self.big[8:16]
        self.st.copy_(torch.tensor([flag, t, skipped, bc[0], bc[1], *SENTINEL], dtype=torch.int32))

    def read(self):
        """(the 8 words as a list, canaries and sentinels intact)."""
        b = self.big.cpu()
        return b[8:16].tolist(), bool((b[:8] == 0x5A5A5A5A).all()) and bool((b[16:] == 0x5A5A5A5A).all()) and tuple(b[13:16].tolist()) == SENTINEL

    def corrections(self):
        return self.st[3:5].cpu().view(torch.float32)


def _i32(x):
    return int(np.array(x, dtype=np.uint32).view(np.int32))


# ------------------------------------------------------------------------------------------------ the update kernels on the table
def _launch(T, c):
    """One case through its kernel: ({output: CPU tensor}, failures of everything that is not the bounded comparison)."""
    i, (lr, b1, b2, eps, wd) = O.inputs(c), O.hyper(c)
    buf = {k: Flat(c.n, F32, i[k]) for k in "pgmv"}
    p16 = Flat(c.n, c.p16) if c.p16 is not None else None
    fails = []
    if c.form == "dev":
        st = State(t=c.t - 1)
        T.adamw_begin(st.st, (b1, b2))
        T.adamw_step_dev(buf["p"].view, buf["g"].view, buf["m"].view, buf["v"].view, st.st, lr, (b1, b2), eps, wd, p16=None if p16 is None else p16.view)
        words, ok = st.read()
        if not ok or words[:3] != [0, c.t, 0]:
            fails.append(f"{c}: state {words} after the step")
        bc = st.corrections()
    else:
        T.adamw_step(buf["p"].view, buf["g"].view, buf["m"].view, buf["v"].view, lr, (b1, b2), eps, wd, step=c.t)
    out = {k: buf[k].view.cpu() for k in "pmv"}
    if c.form == "dev":
        out.update(bc1=bc[0:1].clone(), bc2=bc[1:2].clone())
    if not torch.equal(buf["g"].bits().cpu(), i["g"].view(torch.int32)):
        fails.append(f"{c}: the gradient was written to")
    fails += [f"{c}: canary of {k} overwritten" for k, b in buf.items() if not b.intact()]
    if p16 is not None:
        if not p16.intact():
            fails.append(f"{c}: canary of p16 overwritten")
        want = out["p"].to(c.p16).view(torch.int16)                # RNE of the kernel's OWN p'
        if not torch.equal(p16.bits().cpu(), want):
            fails.append(f"{c}: p16 is not the {_dt(c.p16)} rounding of p' at {int((p16.bits().cpu() != want).sum())} elements")
    return out, fails


def _run_group(T, cases, label):
    assert cases, label
    t0 = time.time()
    fails, worst = [], {}
    for c in cases:
        out, f = _launch(T, c)
        fails += f + O.check(c, out)
        for name, w in O.worst(c, out).items():
            if w > worst.get(name, (-1.0, None))[0]:
                worst[name] = (w, c.id)
    for name, (w, cid) in sorted(worst.items()):
        print(f"{label:30s} {name:4s} worst |error| / bound {w:.3f}  ({cid})")
    print(f"{label:30s} {len(cases)} cases in {time.time() - t0:.1f} s")
    assert not fails, fails[:20]


DEV_GROUPS = [(p16, hp) for p16 in (F16, BF16) for hp in range(len(O.HYPER))] + [(None, 0)]


@pytest.mark.parametrize("p16,hp", DEV_GROUPS, ids=[f"{_dt(p)}-hp{h}" for p, h in DEV_GROUPS])
def test_adamw_step_dev(T, p16, hp):
    _run_group(T, [c for c in O.CASES["adamw_dev"] if c.p16 == p16 and c.hp == hp], f"cir_adamw_step_dev {_dt(p16)} hp{hp}")


@pytest.mark.parametrize("hp", range(len(O.HYPER)))
def test_adamw_step(T, hp):
    _run_group(T, [c for c in O.CASES["adamw"] if c.hp == hp], f"cir_adamw_step hp{hp}")


def test_every_case_runs():
    n = sum(len([c for c in O.CASES["adamw_dev"] if c.p16 == p and c.hp == h]) for p, h in DEV_GROUPS)
    assert n == len(O.CASES["adamw_dev"]) and all(c.hp in range(3) for c in O.CASES["adamw"])


# ------------------------------------------------------------------------------------------------ cir_adamw_begin
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.9, 0.98)], ids=["b2_0.999", "b2_0.98"])
def test_adamw_begin(T, betas):
    b32 = tuple(O.f32(b) for b in betas)
    for t in O.STEPS:
        st = State(t=t - 1, skipped=5, bc=(_i32(0x7FC0DEAD), _i32(0x7FC0BEEF)))
        T.adamw_begin(st.st, betas)
        words, ok = st.read()
        assert ok and words[:3] == [0, t, 5], (t, words)                                      # t counts applied steps, skipped stays
        want = np.array([1.0 - b ** t for b in b32]).astype(np.float32).view(np.int32)          # float32(1 - double(beta_f32)^t)
        got = np.array(words[3:5], dtype=np.int32)
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1, (t, got.view(np.float32), want.view(np.float32))
        # a set flag: the skip count moves, t and both corrections stay, and the update kernel changes nothing
        c = next(c for c in O.CASES["adamw_dev"] if c.n == 2051 and c.t == t and c.p16 == F16)
        i = O.inputs(c)
        buf = {k: Flat(c.n, F32, i[k]) for k in "pgmv"}
        p16 = Flat(c.n, BF16 if t % 2 else F16)
        st.st[0] = 1
        before = st.read()[0]
        T.adamw_begin(st.st, betas)
        T.adamw_step_dev(buf["p"].view, buf["g"].view, buf["m"].view, buf["v"].view, st.st, 0.1, betas, 1e-8, 0.5, p16=p16.view)
        words, ok = st.read()
        assert ok and words == [1, before[1], before[2] + 1] + before[3:], (t, before, words)
        for k in "pgmv":
            assert torch.equal(buf[k].bits().cpu(), i[k].view(torch.int32)) and buf[k].intact(), (t, k)
        assert bool((p16.big.view(torch.int16) == CANARY[p16.dtype]).all()), t                  # not one element of the 16-bit copy written


# ------------------------------------------------------------------------------------------------ a chained run
def test_chained_steps_from_the_kernels_own_state(T):
    """8 steps from zero moments on the reference's hyperparameters; at every step the float64 reference starts from the fp32 state the
    kernel left, so the carry of m, v and t is tested without a trajectory tolerance."""
    hp = tuple(O.f32(x) for x in O.HYPER[0])
    lr, b1, b2, eps, wd = hp
    n = 2051
    idx = torch.arange(n)
    p, m, v = Flat(n, F32, O.REGIMES[0][idx % O.N_REGIMES].clone()), Flat(n, F32, torch.zeros(n)), Flat(n, F32, torch.zeros(n))
    p16 = Flat(n, F16)
    st = State()
    worst = {}
    for k in range(8):
        g_cpu = O.REGIMES[1][(idx * 7 + 97 * k) % O.N_REGIMES].clone()
        if k % 3 == 2:
            g_cpu = -g_cpu
        g = Flat(n, F32, g_cpu)
        prev = {name: b.view.cpu() for name, b in (("p", p), ("m", m), ("v", v))}
        assert bool(O.in_range(g_cpu, prev["v"], hp, k + 1).all())
        T.adamw_begin(st.st, (b1, b2))
        T.adamw_step_dev(p.view, g.view, m.view, v.view, st.st, lr, (b1, b2), eps, wd, p16=p16.view)
        words, ok = st.read()
        assert ok and words[:3] == [0, k + 1, 0], words
        out = dict(p=p.view.cpu(), m=m.view.cpu(), v=v.view.cpu())
        fails, w = O.check_state(f"chained step {k + 1}", out, prev["p"], g_cpu, prev["m"], prev["v"], hp, k + 1)
        assert not fails, fails
        assert torch.equal(g.bits().cpu(), g_cpu.view(torch.int32)) and all(b.intact() for b in (p, m, v, g, p16))
        assert torch.equal(p16.bits().cpu(), out["p"].to(F16).view(torch.int16))
        worst = {name: max(worst.get(name, 0.0), x) for name, x in w.items()}
    print("chained run, 8 steps: worst |error| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------ cir_grads_check
@pytest.mark.parametrize("n", O.GC_LENGTHS)
def test_grads_check_table(T, n):
    fails, runs = [], 0
    for pname, pos in O.gc_positions(n).items():
        for (vname, vbits, _), (sname, scale) in ((v, s) for v in O.GC_VALUES for s in O.GC_SCALES):
            what = f"n{n}-{pname}-{vname}-x{sname}"
            bits = O.gc_buffer(n, pos, vbits)
            g, st = Flat(n, F32, bits.view(torch.float32)), State(t=7, skipped=3, bc=(41, 42))
            T.grads_check(g.view, st.st, scale)
            words, ok = st.read()
            fails += O.gc_check(what, bits, scale, g.bits().cpu(), words[0])
            if not (ok and words[1:5] == [7, 3, 41, 42] and g.intact()):
                fails.append(f"{what}: state {words} or a canary touched")
            runs += 1
    assert runs == len(O.gc_positions(n)) * len(O.GC_VALUES) * len(O.GC_SCALES)
    # the flag only ORs: a preset 1 survives a clean buffer, under every scale
    clean = O.gc_base(n).view(torch.int32)
    for sname, scale in O.GC_SCALES:
        for preset in (0, 1):
            g, st = Flat(n, F32, clean.view(torch.float32)), State(flag=preset)
            T.grads_check(g.view, st.st, scale)
            words, ok = st.read()
            fails += O.gc_check(f"n{n}-clean-x{sname}-preset{preset}", clean, scale, g.bits().cpu(), words[0], preset=preset)
            assert ok and g.intact()
    assert not fails, fails[:20]


def test_grads_check_second_trip(T):
    """The ONE long buffer (optim_cases.GC_LONG_N: a whole first trip, of the second the u = 0 quarter and 257 float4 of u = 1, a 3-element
    tail).  Generated on the device from an integer pattern, compared on the device with torch's own fp32 product over the WHOLE buffer,
    so every element is seen to be scaled exactly once; a value planted in the first trip, in both quarters of the second and in the
    tail is flagged."""
    n, dev = O.GC_LONG_N, torch.device("cuda")
    n4, blocks, stride = O.gc_grid(n)
    assert blocks == O.GC_CAP and 4 * stride < n4 < 6 * stride
    h = torch.arange(n, dtype=torch.int32, device=dev) * -1640531535                           # (2654435761 as int32: wraps)
    base = (((h >> 9) & 0xFFFFF) - 0x80000).float() * 2.0 ** -7                                # 20 significant bits, |x| <= 4096
    del h
    scale = 0.3
    s32 = torch.tensor(scale, dtype=torch.float32, device=dev)
    want = base * s32
    assert not torch.equal(want, (base.double() * scale).float())                              # the product is inexact somewhere
    g = Flat(n, F32)
    plants = {"clean": None, "trip0_u3": 4 * (3 * stride + 12345) + 2, "trip1_u0": 4 * (4 * stride + 777) + 1,
              "trip1_u1_last_float4": 4 * (n4 - 1) + 3, "tail0": 4 * n4, "tail2": n - 1}
    for name, pos in plants.items():
        g.view.copy_(base)
        st = State()
        if pos is not None:
            g.view[pos] = float("inf")
            want[pos] = float("inf")
        T.grads_check(g.view, st.st, scale)
        words, ok = st.read()
        assert ok and words[0] == int(pos is not None), (name, words)
        assert torch.equal(g.view, want), (name, int((g.view != want).sum()))
        assert g.intact(), name
        if pos is not None:
            want[pos] = base[pos] * s32
    # scale 1 writes nothing: the bits stay, a NaN payload in the second trip included, and it is flagged
    g.view.copy_(base)
    g.bits()[plants["trip1_u1_last_float4"]] = _i32(0x7F800001)
    keep = g.bits().clone()
    st = State()
    T.grads_check(g.view, st.st, 1.0)
    assert st.read()[0][0] == 1 and torch.equal(g.bits(), keep) and g.intact()


# ------------------------------------------------------------------------------------------------ train_optim.AdamW
def _slab(shapes, seed):
    """Parameters that tile ONE flat fp32 storage in slices padded to 8 elements, gradients laid out the same in another."""
    sizes = [(int(np.prod(s)) + 7) // 8 * 8 for s in shapes]
    flat, gflat = torch.zeros((sum(sizes),), device="cuda"), torch.zeros((sum(sizes),), device="cuda")
    params, o = [], 0
    for s, size in zip(shapes, sizes):
        k = int(np.prod(s))
        flat[o:o + k] = O.REGIMES[0][(torch.arange(k) * 11 + seed + o) % O.N_REGIMES].cuda()
        p = torch.nn.Parameter(flat[o:o + k].view(s))
        p.grad = gflat[o:o + k].view(s)
        params.append(p)
        o += size
    return params, gflat


def _fill_grads(params, k):
    for j, p in enumerate(params):
        if p.grad is not None:
            idx = (torch.arange(p.numel()) * 13 + 101 * k + 7 * j) % O.N_REGIMES
            p.grad.copy_(O.REGIMES[1][idx].view(p.shape).cuda())


def test_adamw_class_one_step_covers_every_kind_of_parameter(T, monkeypatch):
    from candidate_reranking_cir_amd.train_optim import AdamW
    slab_a, _ = _slab([(5, 7), (16,), (3, 3)], 0)
    slab_b, _ = _slab([(9,), (2, 260)], 5)
    tr = torch.nn.Parameter((O.REGIMES[0][torch.arange(6 * 10) % O.N_REGIMES].view(6, 10).cuda()).t())           # (10, 6), transposed
    store = torch.zeros((34,), device="cuda")
    store[1:] = O.REGIMES[0][(torch.arange(33) * 5) % O.N_REGIMES].cuda()
    off = torch.nn.Parameter(store[1:])                                                                            # one element into its storage
    nograd = torch.nn.Parameter(torch.full((12,), 0.75, device="cuda"))
    assert not tr.is_contiguous() and off.data_ptr() % 16 == 4
    for p in (tr, off):
        p.grad = torch.zeros_like(p)
    params = slab_a + [tr] + slab_b + [off, nograd]
    kw = dict(lr=2e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    opt = AdamW(params, **kw)
    calls = dict(begin=0, step=0, check=0)
    for name, key in (("adamw_begin", "begin"), ("adamw_step_dev", "step"), ("grads_check", "check")):
        real = getattr(T, name)
        monkeypatch.setattr(T, name, (lambda real, key: lambda *a, **k: (calls.__setitem__(key, calls[key] + 1), real(*a, **k))[1])(real, key))
    stepped = [p for p in params if p is not nograd]

    def snapshot():
        torch.cuda.synchronize()
        return [(p.detach().cpu().clone(), opt.m[id(p)].cpu().clone() if id(p) in opt.m else torch.zeros(p.shape),
                 opt.v[id(p)].cpu().clone() if id(p) in opt.v else torch.zeros(p.shape)) for p in stepped]

    worst, t = {}, 0
    for k, lr in enumerate((2e-5, 2e-5, 1e-3, 1e-3)):
        opt.param_groups[0]["lr"] = lr                                                         # (steps 3 and 4: the changed lr must be applied)
        _fill_grads(params, k)
        before = snapshot()
        if k == 1:                                                                             # the ONE skipped step: an inf in the LAST work item
            off.grad[17] = float("inf")
        calls.update(begin=0, step=0, check=0)
        opt.step()
        assert calls == dict(begin=1, step=4, check=4), calls                                  # two flat storages + two tensors share ONE begin
        after = snapshot()
        if k == 1:
            assert opt.t == t and opt.skipped_steps == 1
            for (p0, m0, v0), (p1, m1, v1) in zip(before, after):
                assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(m0, m1) and torch.equal(v0, v1)
            continue
        t += 1
        assert opt.t == t and opt.skipped_steps == (1 if k > 1 else 0)                          # t grows by exactly 1 per applied step
        hp = tuple(O.f32(x) for x in (lr, 0.9, 0.999, 1e-8, 0.05))
        for j, (p, (p0, m0, v0), (p1, m1, v1)) in enumerate(zip(stepped, before, after)):
            g = p.grad.cpu()
            assert bool(O.in_range(g.flatten(), v0.flatten(), hp, t).all())
            fails, w = O.check_state(f"AdamW.step {k + 1} parameter {j} {tuple(p.shape)}", dict(p=p1, m=m1, v=v1), p0, g, m0, v0, hp, t)
            assert not fails, fails
            worst = {name: max(worst.get(name, 0.0), x) for name, x in w.items()}
        assert bool((nograd == 0.75).all()) and id(nograd) not in opt.m
    assert len(opt._flats) == 2 and bool((store[0] == 0).all())
    print("train_optim.AdamW, 3 applied steps: worst |error| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(worst.items())))


def test_unscale_and_check_divides_by_the_loss_scale(T):
    """train_core._unscale_and_check: gflat /= S for the power of two `loss_scale` returns (exact: bit for bit the quotient), "all finite"
    as a device flag; a non-finite element anywhere turns it False."""
    from candidate_reranking_cir_amd.train_core import _unscale_and_check, loss_scale
    base = O.gc_base(2051)
    s = loss_scale(float(base.abs().max()) / 3.7)
    assert s != 1.0
    for pos, ok in ((None, True), (2050, False), (1024, False)):
        g = Flat(2051, F32, base * s)
        if pos is not None:
            g.view[pos] = float("nan") if pos % 2 else float("-inf")
        fin = _unscale_and_check(g.view, s)
        assert fin.dtype == torch.bool and bool(fin) == ok and g.intact()
        got = g.view.cpu()
        keep = torch.ones(2051, dtype=torch.bool)
        if pos is not None:
            keep[pos] = False
        assert torch.equal(got[keep].view(torch.int32), base[keep].view(torch.int32))
