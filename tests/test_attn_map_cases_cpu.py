"""tests/attn_map_cases.py on the CPU: what its comparison lets through and what it catches.  The torch fp32 stand-in "kernel" passes
every case within the a-priori bounds; every wrong form fails on a named case; the table has the cases the kernels' branches need."""
import pytest
import torch

from tests import attn_bwd_cases as B
from tests import attn_map_cases as M
from tests.attn_cases import BF16, F16


def test_table_covers_the_branches():
    shapes = {c.shape for c in M.CASES}
    assert shapes == set(B.SHAPES)
    for dt in (BF16, F16):
        masks = {c.mask for c in M.CASES if c.dt == dt}
        assert {"none", "tail", "front", "min_tail", "tail40", "all10k", "min_all"} <= masks
        assert any(getattr(c, "items", None) == "sub7" for c in M.CASES if c.dt == dt)
    assert all(c.p == 0.0 for c in M.CASES)
    loss = [c for c in M.CASES if getattr(c, "do", None) == "loss"]
    assert loss and all(M.dmul(c) < 1.0 and 256.0 <= float(B.inputs(c)["do"].float().abs().max()) < 512.0 for c in loss)
    assert len({c.id for c in M.CASES}) == len(M.CASES)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_stand_in_passes(case):
    if case not in B.CASES:                                         # (the others: tests/test_attn_bwd_cases_cpu.py asserts it)
        assert float(B.second_order_ok(case).max()) <= 0.05
    out = M.emulate(case, "kernel")
    fails = M.check(case, out)
    assert not fails, fails
    ref = M.ref64(case)
    assert all(bool(torch.isfinite(ref[n]).all()) for n in M.OUTPUTS)
    # pad-free reference: every row of P^ sums to 1, a masked key (-10000 or saturated, beside an open one) has weight ~0
    assert float((ref["probs"].sum(-1) - 1).abs().max()) < 1e-12


NAMED = {
    "no_unscale": ((33, 100), F16, "none", None, "loss"),
    "natural_lse": ((9, 9), BF16, "none", None, None),
    "mask_dropped": ((33, 100), BF16, "tail", None, None),
    "g_from_k": ((32, 32), F16, "none", None, None),
    "relu_after_mean": ((64, 65), BF16, "none", None, None),
    "no_head_mean": ((70, 197), F16, "none", None, None),
    "sat_row_unhandled": ((33, 100), BF16, "min_all", None, None),
}


@pytest.mark.parametrize("variant", M.WRONG)
def test_wrong_forms_fail(variant):
    case = M.named(*NAMED[variant])
    fails = M.check(case, M.emulate(case, variant))
    assert fails, f"{variant} passes {case}"
    assert not M.check(case, M.emulate(case, "kernel"))
    which = {f.split()[1].rstrip(":") for f in fails}
    if variant in ("relu_after_mean", "no_head_mean"):
        assert which == {"cam"}, which                              # the maps themselves are right
    if variant in ("no_unscale", "g_from_k"):
        assert "probs" not in which and "rowsum" not in which


def test_no_head_mean_is_invisible_with_one_head():
    """H = 1 (items = sub7): the mean is the identity - why the named case of `no_head_mean` has two heads."""
    case = M.named((9, 9), BF16, "none", "sub7", None)
    assert not M.check(case, M.emulate(case, "no_head_mean"))
