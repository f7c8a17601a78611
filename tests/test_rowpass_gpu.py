"""The LayerNorm family and the row passes of the training step on a real MI355X against the float64 references and the a-priori bounds of
tests/rowpass_cases.py: cir_layernorm (fp32 and fp16 stream rows, every output pairing, residual, the twin form), cir_residual_layernorm_train,
cir_layernorm_bwd and cir_layernorm_bwd_fused (plain and ordered), cir_rows16_colsum (both modes, strided views, the halves of one buffer,
ordered) and cir_rows_scale_add - each through its wrapper in ops.py / train_ops.py, on the eight row kinds (ViT outlier channels, offsets,
constant, zero, one-hot, tiny) at shapes with a one-lane chunk (5 x 260), ragged last blocks and 66-block column sums (2100 x 768).

Every output of every case is written inside canary bands (tests.test_guard_gpu.Guarded) and every accumulated output starts from 0.25.
Every ordered case runs twice and must give the same bits, and its dx / dt16 / out must equal the plain form's.  One test function covers
one kernel and type and prints the worst |error| / bound per output."""
import math
import time

import pytest
import torch

from tests import rowpass_cases as R
from tests.test_guard_gpu import Guarded

pytestmark = pytest.mark.gpu

BF16, F16, F32 = R.BF16, R.F16, R.F32
_dt = lambda d: "none" if d is None else R.DT_NAME[d]      # noqa: E731


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import ops, train_ops

    class RT:
        pass
    r = RT()
    r.ops, r.T = ops, train_ops
    return r


class Bands:
    """The outputs of one launch, each a contiguous (or column-padded) view between canary rows (and columns)."""

    def __init__(self):
        self.guards = []

    def out(self, shape, dtype, pc=0):
        g = Guarded(math.prod(shape[:-1]), shape[-1], dtype, pr=8, pc=pc)
        self.guards.append(g)
        return g.view.view(shape) if pc == 0 else g.view

    def acc(self, cols):
        v = self.out((1, cols), F32)
        v.fill_(R.START)
        return v[0]

    def intact(self, what):
        for g in self.guards:
            g.assert_intact(str(what))


def _dev(t):
    return None if t is None else t.cuda()


def _cpu(outs):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in outs.items()}


# ------------------------------------------------------------------------------------------------ one launch per kernel
def _layernorm(rt, c, b, work=None):
    i = R.inputs(c)
    lead = ((2,) if c.twin else ()) + tuple(c.shape)
    o32 = b.out(lead, c.sdt) if c.sdt is not None else None
    o16 = b.out(lead, c.dt16) if c.dt16 is not None else None
    ys, y16 = rt.ops.layernorm(i["x"].cuda(), i["gamma"].cuda(), i["beta"].cuda(), c.eps, residual=_dev(i["residual"]), out32=o32, out16=o16,
                               want32=c.sdt is not None, dtype16=c.dt16, stream_dtype=c.sdt)
    assert (ys is None) == (c.sdt is None) and (y16 is None) == (c.dt16 is None)
    return {k: v for k, v in (("stream", ys), ("y16", y16)) if v is not None}


def _res_ln_train(rt, c, b, work=None):
    i = R.inputs(c)
    pre, y32, y16 = rt.T.residual_layernorm_train(i["t0"].cuda(), _dev(i["t1"]), i["residual"].cuda(), i["gamma"].cuda(), i["beta"].cuda(), c.eps, c.dt16,
                                                  alpha=c.alpha, p_drop=c.p, seed=R.drop_seed(c), pre=b.out(c.shape, F32),
                                                  y32=b.out(c.shape, F32) if c.want32 else None, y16=b.out(c.shape, c.dt16), want32=bool(c.want32))
    assert (y32 is None) == (not c.want32)
    return {k: v for k, v in (("pre", pre), ("y32", y32), ("y16", y16)) if v is not None}


def _ln_bwd(rt, c, b, work=None):
    i = R.inputs(c)
    dgamma, dbeta = b.acc(c.shape[1]), b.acc(c.shape[1])
    dx = rt.T.layernorm_bwd(i["x"].cuda(), i["gamma"].cuda(), i["dy"].cuda(), dgamma, dbeta, c.eps, work=work, dx=b.out(c.shape, F32))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def _ln_bwd_fused(rt, c, b, work=None):
    i = R.inputs(c)
    cols = c.shape[1]
    dgamma, dbeta = b.acc(cols), b.acc(cols)
    bias = [b.acc(cols) for _ in range(c.nbias)] + [None, None]
    want_dx, want_dt = c.outs != "dt_only", c.outs != "dx_only"
    dx, dt16 = rt.T.layernorm_bwd_fused(i["x"].cuda(), i["gamma"].cuda(), i["dy"].cuda(), dgamma, dbeta, c.eps, c.dt16, t_add=_dev(i["t_add"]),
                                        dbias=bias[0], dbias2=bias[1], alpha=c.alpha, p_drop=c.p, seed=R.drop_seed(c), want_dx=want_dx, want_dt=want_dt,
                                        dx=b.out(c.shape, F32) if want_dx else None, dt16=b.out(c.shape, c.dt16) if want_dt else None, work=work)
    assert (dx is None) == (not want_dx) and (dt16 is None) == (not want_dt)
    outs = dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dt16=dt16, dbias=bias[0], dbias2=bias[1])
    return {k: v for k, v in outs.items() if v is not None}


def _rows16(rt, c, b, work=None):
    i = R.inputs(c)
    rows, cols = c.shape
    lo = cols * (c.half or 0)
    a, z = i["abuf"].cuda()[:, lo:lo + cols], i["zbuf"].cuda()[:, lo:lo + cols]
    assert a.stride(0) == cols + c.pad and a.data_ptr() % 16 == 0
    sums = b.acc(cols) if c.sums else None
    if c.mode == 0:
        return dict(sums=rt.T.colsum16(a, sums, work=work))
    out = rt.T.gelu_bwd16(a, z, sums, work=work, out=b.out(c.shape, c.dt, pc=392 if c.half is not None else (8 if c.pad else 0)))
    return dict(out=out, sums=sums) if c.sums else dict(out=out)


def _rows_scale_add(rt, c, b, work=None):
    i = R.inputs(c)
    return dict(out=rt.T.rows_scale_add(_dev(i["a"]), i["b"].cuda(), i["scale"].cuda(), i["rows_per_group"], c.out, out=b.out(c.shape, c.out)))


LAUNCH = {"layernorm": _layernorm, "res_ln_train": _res_ln_train, "ln_bwd": _ln_bwd, "ln_bwd_fused": _ln_bwd_fused, "rows16_colsum": _rows16,
          "rows_scale_add": _rows_scale_add}
SAME_AS_PLAIN = ("dx", "dt16", "out")       # of an ordered form: bit for bit the plain form's


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _run_group(rt, cases, label):
    assert cases, label
    t0 = time.time()
    fails, worst = [], {}
    for c in cases:
        launch, bands = LAUNCH[c.kernel], Bands()
        ordered = bool(getattr(c, "ordered", 0))
        got = _cpu(launch(rt, c, bands, rt.T.Workspace() if ordered else None))
        bands.intact(c)
        fails += R.check(c, got)
        for name, w in R.worst(c, got).items():
            if w > worst.get(name, (-1.0, None))[0]:
                worst[name] = (w, c.id)
        if ordered:
            work, again_bands, plain_bands = rt.T.Workspace(), Bands(), Bands()
            work.f32(1 << 18, torch.device("cuda", torch.cuda.current_device())).fill_(float("nan"))     # the workspace's old contents do not matter
            again, plain = _cpu(launch(rt, c, again_bands, work)), _cpu(launch(rt, c, plain_bands, None))
            again_bands.intact(c)
            plain_bands.intact(c)
            fails += [f"{c} {n}: two runs of the ordered form differ" for n in got if not torch.equal(_bits(got[n]), _bits(again[n]))]
            fails += [f"{c} {n}: the ordered form differs from the plain form" for n in got
                      if n in SAME_AS_PLAIN and not torch.equal(_bits(got[n]), _bits(plain[n]))]
            fails += R.check(c, plain)
    for name, (w, cid) in sorted(worst.items()):
        print(f"{label:34s} {name:7s} worst |error| / bound {w:.3f}  ({cid})")
    print(f"{label:34s} {len(cases)} cases in {time.time() - t0:.1f} s")
    assert not fails, fails[:20]


def _pick(kernel, **kw):
    return [c for c in R.CASES[kernel] if all(getattr(c, k) == v for k, v in kw.items())]


@pytest.mark.parametrize("xdt", [F32, F16], ids=_dt)
def test_layernorm(rt, xdt):
    _run_group(rt, _pick("layernorm", xdt=xdt), f"cir_layernorm x {_dt(xdt)}")


@pytest.mark.parametrize("dt16", [BF16, F16], ids=_dt)
def test_residual_layernorm_train(rt, dt16):
    _run_group(rt, _pick("res_ln_train", dt16=dt16), f"cir_residual_layernorm_train {_dt(dt16)}")


@pytest.mark.parametrize("ordered", [0, 1], ids=["plain", "ordered"])
def test_layernorm_bwd(rt, ordered):
    _run_group(rt, _pick("ln_bwd", ordered=ordered), "cir_layernorm_bwd" + "_ordered" * ordered)


@pytest.mark.parametrize("ordered", [0, 1], ids=["plain", "ordered"])
@pytest.mark.parametrize("dt16", [BF16, F16], ids=_dt)
def test_layernorm_bwd_fused(rt, dt16, ordered):
    _run_group(rt, _pick("ln_bwd_fused", dt16=dt16, ordered=ordered), "cir_layernorm_bwd_fused" + "_ordered" * ordered + " " + _dt(dt16))


@pytest.mark.parametrize("mode", [0, 1], ids=["colsum", "gelu_bwd"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_dt)
def test_rows16_colsum(rt, dt, mode):
    _run_group(rt, _pick("rows16_colsum", dt=dt, mode=mode), f"cir_rows16_colsum mode {mode} {_dt(dt)}")


@pytest.mark.parametrize("out", [F32, BF16, F16], ids=_dt)
def test_rows_scale_add(rt, out):
    _run_group(rt, _pick("rows_scale_add", out=out), f"cir_rows_scale_add out {_dt(out)}")


def test_every_case_runs():
    """The groups above partition the table."""
    n = sum(len(_pick("layernorm", xdt=d)) for d in (F32, F16)) + sum(len(_pick("res_ln_train", dt16=d)) for d in (BF16, F16))
    n += sum(len(_pick("ln_bwd", ordered=o)) for o in (0, 1)) + sum(len(_pick("ln_bwd_fused", dt16=d, ordered=o)) for d in (BF16, F16) for o in (0, 1))
    n += sum(len(_pick("rows16_colsum", dt=d, mode=m)) for d in (BF16, F16) for m in (0, 1)) + sum(len(_pick("rows_scale_add", out=o)) for o in (F32, BF16, F16))
    assert n == sum(len(v) for v in R.CASES.values())
    for shape in R.GUARDED_SHAPES:
        assert any(tuple(c.shape) == shape for v in R.CASES.values() for c in v), shape
