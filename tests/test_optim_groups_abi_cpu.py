"""Argument validation of cir_grads_sumsq, cir_grads_sumsq_workspace, cir_adamw_begin_clip and cir_adamw_step_groups on the host: negative
CIR_E* codes before any launch (fake, never dereferenced device addresses, as tests/test_abi.py does), and the host checks of the
train_ops wrappers around them (the segment table lives on the device, so train_ops.SegmentTable checks it where it is built)."""
import ctypes
import math

import pytest

from candidate_reranking_cir_amd import lib

EINVAL, ESHAPE, EALIGN, EDTYPE = -1, -2, -3, -4
P = 0x10000          # 16-byte aligned fake device address
BF16, F16, F32 = 0, 1, 2


@pytest.fixture(scope="module")
def c():
    return lib.load()


def test_grads_sumsq_validation(c):
    assert c.cir_grads_sumsq(None, 8, P, P, None) == EINVAL and c.cir_grads_sumsq(P, 8, None, P, None) == EINVAL
    assert c.cir_grads_sumsq(P, 8, P, None, None) == EINVAL and c.cir_grads_sumsq(P, 0, P, P, None) == EINVAL
    assert c.cir_grads_sumsq(P + 4, 8, P, P, None) == EALIGN and c.cir_grads_sumsq(P, 8, P, P + 4, None) == EALIGN


def test_grads_sumsq_workspace_is_a_pure_function_of_n(c):
    w = c.cir_grads_sumsq_workspace
    assert w(0) == EINVAL and w(-5) == EINVAL
    # one workgroup per 1024 float4, at least one, at most 1024
    assert [w(n) for n in (1, 3, 4, 4096, 4097, 4100, 8192, 8196)] == [1, 1, 1, 1, 1, 2, 2, 3]
    assert w(4 * 1024 * 1024) == 1024 and w(4 * 1024 * 1024 + 4) == 1024 and w(4 * 10 ** 7) == 1024 and w(2 ** 33) == 1024
    assert w(12345) == w(12345)


def test_adamw_begin_clip_validation(c):
    f = c.cir_adamw_begin_clip
    assert f(None, 0.9, 0.999, P, 4, 1.0, None) == EINVAL and f(P, 0.9, 0.999, None, 4, 1.0, None) == EINVAL
    assert f(P, 0.9, 0.999, P, 0, 1.0, None) == EINVAL
    for bad in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert f(P, 0.9, 0.999, P, 4, bad, None) == EINVAL, bad
    assert f(P, 0.9, 0.999, P + 4, 4, 1.0, None) == EALIGN


def test_adamw_step_groups_validation(c):
    groups = lib.AdamwGroups()
    names = ["p", "g", "m", "v", "n", "b1", "b2", "state", "seg_end", "seg_group", "nseg", "group", "groups", "ngroups", "clip", "p16", "dtype16", "stream"]
    ok = dict(p=P, g=P, m=P, v=P, n=64, b1=0.9, b2=0.999, state=P, seg_end=P, seg_group=P, nseg=2, group=0, groups=ctypes.byref(groups), ngroups=2,
              clip=0, p16=None, dtype16=0, stream=None)

    def call(**over):                       # (the valid argument list itself is never passed: it would launch)
        a = dict(ok, **over)
        return c.cir_adamw_step_groups(*[a[k] for k in names])

    for k in ("p", "g", "m", "v", "state", "groups"):
        assert call(**{k: None}) == EINVAL, k
    assert call(n=0) == EINVAL and call(nseg=0) == EINVAL and call(nseg=-1) == EINVAL
    assert call(ngroups=0) == EINVAL and call(ngroups=9) == EINVAL                              # more than 8 groups
    assert call(seg_end=None) == EINVAL and call(seg_group=None) == EINVAL                    # the table comes whole or not at all
    assert call(n=66) == EINVAL                                                               # a table's n is a multiple of 4
    # the form without a table: one segment, its group id in range; the only one whose n may be no multiple of 4
    none = dict(seg_end=None, seg_group=None, nseg=1)
    assert call(seg_end=None, seg_group=None, nseg=2) == EINVAL
    assert call(**none, group=2) == EINVAL and call(**none, group=-1) == EINVAL and call(**none, group=8, ngroups=8) == EINVAL
    assert call(**none, n=7, p=P + 4) == EALIGN                                               # (n = 7 itself is accepted: the next check answers)
    for k in ("p", "g", "m", "v"):
        assert call(**{k: P + 8}) == EALIGN, k
    assert call(p16=P + 4, dtype16=F16) == EALIGN and call(seg_end=P + 4) == EALIGN and call(seg_group=P + 2) == EALIGN
    assert call(p16=P, dtype16=F32) == EDTYPE and call(p16=P, dtype16=7) == EDTYPE


def test_wrappers_check_on_the_host():
    import torch
    from candidate_reranking_cir_amd import train_ops as T
    with pytest.raises(ValueError, match="1 to 8 groups"):
        T.adamw_groups([])
    with pytest.raises(ValueError, match="1 to 8 groups"):
        T.adamw_groups([(1e-3, 0.0, 1e-8)] * 9)
    a = T.adamw_groups([(1e-3, 0.05, 1e-8), (2e-3, 0.0, 1e-6)])
    assert (a.lr[1], a.weight_decay[0], a.eps[1]) == (ctypes.c_float(2e-3).value, ctypes.c_float(0.05).value, ctypes.c_float(1e-6).value)
    for ends, ids in (([], []), ([8, 16], [0]), ([8, 8], [0, 1]), ([16, 8], [0, 1]), ([4, 16], [0, 1]), ([8, 18], [0, 1]), ([0, 8], [0, 1])):
        with pytest.raises(ValueError, match="segment table"):
            T.SegmentTable(ends, ids, "cpu")
    for ids in ([0, 8], [-1, 0]):
        with pytest.raises(ValueError, match="group ids"):
            T.SegmentTable([8, 16], ids, "cpu")
    t = T.SegmentTable([8, 24, 28], [0, 3, 0], "cpu")
    assert (t.n, t.nseg, t.max_id) == (28, 3, 3) and t.ends.dtype == torch.int64 and t.ids.dtype == torch.int32
    with pytest.raises(lib.CirrankError):                                                     # CPU tensors are refused, as everywhere
        T.grads_sumsq(torch.zeros(8), torch.zeros(8, dtype=torch.int32), torch.zeros(1, dtype=torch.float64))
