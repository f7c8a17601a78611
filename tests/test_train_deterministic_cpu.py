"""Host side of the deterministic training mode (train.set_deterministic), no GPU: the switch, and which operators the layer views of
train_core call with it off and on.  The kernels are replaced by recording stubs that return tensors of the right shape; the slab is a
real `_Slab` over CPU parameters."""
import pytest
import torch

from candidate_reranking_cir_amd import train, train_core, train_ops

BF = torch.bfloat16


@pytest.fixture
def mode():
    assert train.deterministic() is False                       # the default, and what every other test runs under
    yield train.set_deterministic
    train.set_deterministic(False)


def test_switch_defaults_off_and_round_trips(mode):
    assert train.deterministic() is False and train_ops.deterministic() is False
    assert train.set_deterministic is train_ops.set_deterministic and train.deterministic is train_ops.deterministic
    mode(True)
    assert train.deterministic() is True
    mode(0)
    assert train.deterministic() is False
    mode(1)
    assert train.deterministic() is True


class Recorder:
    """Stand-ins for the train_ops / ops entry points the layer views call: (name, number of positional arguments, keyword arguments
    that are not tensors) per call; `work` is recorded as True."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("colsum", "colsum16", "wgrad", "wgrad_grouped", "bmm", "layernorm_bwd", "layernorm_bwd_fused", "eltwise"):
            monkeypatch.setattr(train_ops, name, self._stub(name))
        monkeypatch.setattr(train_core.ops, "gemm", self._stub("gemm"))

    def _stub(self, name):
        def fn(*a, **kw):
            self.calls.append((name, len(a), {k: (True if k == "work" else v) for k, v in kw.items() if not torch.is_tensor(v)}))
            if name == "eltwise":                               # _cast
                return a[0].to(kw.get("out_dtype") or a[0].dtype)
            if name == "bmm" and kw.get("out") is None:         # the row-chunk partial products of _Lin.bwd
                return torch.zeros((a[0].shape[0], a[0].shape[2], a[1].shape[2]))
            if name == "gemm":
                return torch.zeros((a[0].shape[0], a[1].shape[0]), dtype=kw.get("out_dtype", torch.float32))
            if name in ("layernorm_bwd", "layernorm_bwd_fused"):
                return torch.zeros_like(a[0])
            return None
        return fn


def _slab():
    shapes = {"a.weight": (128, 128), "a.bias": (128,), "small.weight": (2, 128), "small.bias": (2,), "ln.weight": (128,), "ln.bias": (128,)}
    params = {n: torch.nn.Parameter(torch.randn(s)) for n, s in shapes.items()}
    slab = train_core._Slab(params, list(shapes), BF, key=lambda: ())
    slab.flat16 = torch.zeros((slab.total,), dtype=BF)
    slab.flat16t = torch.zeros((slab.total,), dtype=BF)
    slab.gflat = torch.zeros((slab.total,))
    return slab


def _drive(slab, tr):
    """One of each backward the three passes are made of: an fp32-gradient Linear with a row split, the 16-bit-gradient Linear on and off
    the 128 grid (stand-alone and queued), both LayerNorm adjoints, the layer's grouped weight-gradient launch."""
    a, small, ln = train_core._Lin(slab, "a"), train_core._Lin(slab, "small"), train_core._LN(slab, "ln", 1e-12)
    x16, dy, dy16 = torch.zeros((256, 128), dtype=BF), torch.zeros((256, 128)), torch.zeros((256, 128), dtype=BF)
    a.bwd(x16, dy)
    a.bwd16(x16, dy16, bias=True)
    queue = []
    a.bwd16(x16, dy16, need_dx=False, queue=queue)
    small.bwd16(x16, torch.zeros((256, 2), dtype=BF), need_dx=False, bias=True)
    ln.bwd(dy, dy)
    ln.bwd_res(dy, dy, BF, dbias=a.db, p_drop=0.1, seed=7)
    tr._wgrad_grouped(queue)
    assert len(queue) == 1


def _trainer(slab):
    tr = train_core.Trainer.__new__(train_core.Trainer)
    tr.slab = slab
    return tr


# what the layer views called before the mode existed: the same names, positional counts and keywords - nothing added, nothing dropped
DEFAULT_CALLS = [
    ("eltwise", 2, {"out_dtype": BF, "p_drop": 1.0}),                               # _Lin.bwd: cast dy
    ("colsum", 2, {}),                                                              # ... bias gradient
    ("bmm", 4, {"out_dtype": torch.float32}),                                       # ... two row chunks of 128 -> partial products
    ("colsum", 2, {}),                                                              # ... summed into dW
    ("gemm", 3, {"out_dtype": torch.float32}),
    ("colsum16", 2, {}),                                                            # _Lin.bwd16 (stand-alone)
    ("wgrad", 3, {}),
    ("gemm", 3, {"out_dtype": torch.float32}),
    ("colsum16", 2, {}),                                                            # the 128 -> 2 Linear: cir_bmm, atomically shared dW
    ("bmm", 4, {"accumulate": "atomic"}),
    ("layernorm_bwd", 6, {}),
    ("layernorm_bwd_fused", 7, {"p_drop": 0.1, "seed": 7}),
    ("wgrad_grouped", 1, {}),
]


def test_mode_off_calls_what_the_layers_called_before(mode, monkeypatch):
    rec = Recorder(monkeypatch)
    slab = _slab()
    assert slab.read_mode() == {} and slab.work is None
    _drive(slab, _trainer(slab))
    got = [(n, k, {q: v for q, v in kw.items() if q not in ("residual", "out")}) for n, k, kw in rec.calls]
    assert got == DEFAULT_CALLS


def test_mode_on_calls_no_atomic_form(mode, monkeypatch):
    rec = Recorder(monkeypatch)
    slab = _slab()
    mode(True)
    kw = slab.read_mode()
    assert set(kw) == {"work"} and isinstance(kw["work"], train_ops.Workspace) and slab.work is kw["work"]
    _drive(slab, _trainer(slab))
    names = [c[0] for c in rec.calls]
    assert names == [c[0] for c in DEFAULT_CALLS]                                  # the same operators in the same places ...
    for name, _, kws in rec.calls:
        assert kws.get("accumulate") != "atomic", name                              # ... none shares a destination through atomics,
        if name in ("wgrad", "wgrad_grouped"):
            assert kws.get("splits") == 1, name                                     # every weight-gradient tile has one workgroup,
        if name in ("colsum", "colsum16", "layernorm_bwd", "layernorm_bwd_fused"):
            assert kws.get("work") is True, name                                    # and every cross-workgroup sum takes its fixed-order form
    small_bmm = [kws for name, _, kws in rec.calls if name == "bmm"][1]
    assert small_bmm.get("accumulate") is True
    # the switch is read when a backward starts: one trainer, the mode changed between two passes; the workspace is kept
    work = slab.work
    mode(False)
    assert slab.read_mode() == {} and slab.work is None
    mode(True)
    assert slab.read_mode()["work"] is work


def test_workspace_grows_and_is_reused():
    w = train_ops.Workspace()
    dev = torch.device("cpu")
    a = w.f32(10, dev)
    assert a.numel() >= 10 and w.f32(4, dev) is a and w.f32(0, dev) is a
    b = w.f32(11, dev)
    assert b.numel() >= 11 and b is not a
    i = w.i32(5, dev)
    assert i.dtype == torch.int32 and w.i32(5, dev) is i
