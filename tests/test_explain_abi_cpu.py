"""The attention-map entry points at the C-ABI boundary, without a GPU: cir_attention_maps / cir_attention_gradcam are declared in
include/cirrank.h, bound in lib.py with matching argument lists and exported by the library; their argument errors are raised on the host
before any launch (fake, never dereferenced device addresses, as tests/test_abi.py does for the other entry points); and
explain.patch_grid lays out / refuses key counts."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cirrank.h")
NAMES = ("cir_attention_maps", "cir_attention_gradcam")
EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
BF16, F16, F32 = 0, 1, 2
P = 0x10000                                         # a 16-byte aligned fake device address


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/cirrank.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(param):
    import ctypes
    if "*" in param:
        return ctypes.c_void_p
    return {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}[param.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_declared_bound_and_exported_with_matching_signatures(name):
    import ctypes
    from candidate_reranking_cir_amd import lib
    params = _declaration(name)
    restype, argtypes = lib.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert [_ctype(p) for p in params] == list(argtypes), name
    # head views: three element strides behind each of q, k, v, d_o, as in cir_attention_train_bwd
    for t in ("q", "k", "v", "d_o"):
        j = next(i for i, p in enumerate(params) if p.endswith("* " + t))
        assert [p.split()[0] for p in params[j + 1:j + 4]] == ["int64_t"] * 3, (name, t)
    assert hasattr(lib.load(), name)
    assert lib.load().cir_version() == 15                           # additive: the ABI version stays


def _maps(c, **over):
    a = dict(q=P, k=P, v=P, mask=None, d_o=P, lse=P, probs=P, dprobs=P, ldk=12, G=2, H=2, Lq=5, Lk=9, hd=64, scale=0.125, dmul=1.0, dt=BF16, s=64)
    a.update(over)
    s = a["s"]
    return c.cir_attention_maps(a["q"], s, s, s, a["k"], s, s, s, a["v"], s, s, s, a["mask"], a["d_o"], s, s, s, a["lse"], a["probs"], a["dprobs"],
                                a["ldk"], a["G"], a["H"], a["Lq"], a["Lk"], a["hd"], a["scale"], a["dmul"], a["dt"], None)


def _cam(c, **over):
    a = dict(q=P, k=P, v=P, mask=None, d_o=P, lse=P, cam=P, ldk=12, G=2, H=2, Lq=5, Lk=9, hd=64, scale=0.125, dmul=1.0, dt=F16, s=64)
    a.update(over)
    s = a["s"]
    return c.cir_attention_gradcam(a["q"], s, s, s, a["k"], s, s, s, a["v"], s, s, s, a["mask"], a["d_o"], s, s, s, a["lse"], a["cam"],
                                   a["ldk"], a["G"], a["H"], a["Lq"], a["Lk"], a["hd"], a["scale"], a["dmul"], a["dt"], None)


def test_argument_errors_before_any_launch():
    """(the valid argument list itself is never passed: it would launch)"""
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    for call in (_maps, _cam):
        assert call(c, ldk=10) == ESHAPE                            # not a multiple of 4
        assert call(c, ldk=8) == ESHAPE                             # below Lk
        assert call(c, hd=32) == ESHAPE and call(c, hd=128) == ESHAPE
        assert call(c, q=None) == EINVAL and call(c, k=None) == EINVAL and call(c, lse=None) == EINVAL and call(c, Lq=0) == EINVAL
        assert call(c, dt=F32) == EDTYPE and call(c, dt=7) == EDTYPE
        assert call(c, s=60) == EALIGN and call(c, q=P + 2) == EALIGN
    assert _maps(c, probs=None) == EINVAL and _maps(c, probs=P + 4) == EALIGN and _maps(c, dprobs=P + 8) == EALIGN
    # v, d_o and dprobs: all or none
    assert _maps(c, v=None) == ESHAPE and _maps(c, d_o=None) == ESHAPE and _maps(c, dprobs=None) == ESHAPE
    assert _maps(c, v=None, d_o=None) == ESHAPE and _maps(c, v=None, dprobs=None) == ESHAPE and _maps(c, d_o=None, dprobs=None) == ESHAPE
    assert _maps(c, v=None, d_o=None, dprobs=None, ldk=10) == ESHAPE        # (the consistent probabilities-only pattern gets past that check)
    assert _cam(c, v=None) == EINVAL and _cam(c, d_o=None) == EINVAL and _cam(c, cam=None) == EINVAL and _cam(c, cam=P + 4) == EALIGN


def test_operators_refuse_cpu_tensors():
    from candidate_reranking_cir_amd import train_ops as T
    from candidate_reranking_cir_amd.lib import CirrankError
    q = torch.zeros((1, 1, 4, 64), dtype=torch.bfloat16)
    lse = torch.zeros((1, 1, 4))
    with pytest.raises(CirrankError):
        T.attention_maps(q, q, q, None, q, lse)
    with pytest.raises(CirrankError):
        T.attention_gradcam(q, q, q, None, q, lse)


def test_patch_grid():
    from candidate_reranking_cir_amd import explain
    from candidate_reranking_cir_amd.blip_stage2 import BLIP_NLVR
    x = torch.arange(2 * 3 * 17, dtype=torch.float32).view(2, 3, 17)
    g = explain.patch_grid(x)
    assert g.shape == (2, 3, 4, 4) and torch.equal(g.reshape(2, 3, 16), x[..., 1:])
    assert explain.patch_grid(torch.zeros(577)).shape == (24, 24)
    assert BLIP_NLVR.patch_grid(x).shape == (2, 3, 4, 4)
    for n in (1, 3, 16, 18, 576):
        with pytest.raises(ValueError, match="patch grid"):
            explain.patch_grid(torch.zeros((2, n)))
    assert all(hasattr(BLIP_NLVR, m) for m in ("cross_attention_maps", "gradcam", "patch_grid"))
