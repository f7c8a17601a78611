"""cir_rank_undecided_cuts at the C-ABI boundary, without a GPU: the binding names it, the library exports it, and every refusal happens on
the host before any launch (fake, never dereferenced device addresses, as tests/test_abi.py does for the other entry points)."""
import ctypes
import inspect

import pytest


def test_the_binding_and_the_library_hold_the_new_entry_point():
    from candidate_reranking_cir_amd import lib
    assert "cir_rank_undecided_cuts" in lib.SIGNATURES
    restype, argtypes = lib.SIGNATURES["cir_rank_undecided_cuts"]
    assert restype is ctypes.c_int and len(argtypes) == 14
    c = lib.load()
    assert hasattr(c, "cir_rank_undecided_cuts")
    assert c.cir_version() == 15                                            # additive within ABI v15


def test_arguments_are_checked_before_any_launch():
    from candidate_reranking_cir_amd import lib
    c = lib.load()
    EINVAL, ESHAPE = -1, -2
    P = 0x10000
    ws = c.cir_rank_undecided_workspace

    def und(cuts=(1, 5, 10, 50), n_cuts=None, **over):
        host = None if cuts is None else (ctypes.c_int * max(len(cuts), 1))(*cuts)
        a = dict(values=P, ld=100, active=None, margin=0.5, first=10, cuts=host, n_cuts=len(cuts) if n_cuts is None else n_cuts, pos=P, count=P,
                 Q=4, K=100, work=P, bytes=ws(4, 100), stream=None)
        a.update(over)
        return c.cir_rank_undecided_cuts(*[a[x] for x in ("values", "ld", "active", "margin", "first", "cuts", "n_cuts", "pos", "count", "Q", "K",
                                                          "work", "bytes", "stream")])

    # the four refusals of the new arguments
    assert und(first=-1) == EINVAL
    assert und(cuts=tuple(range(1, 10))) == EINVAL and und(n_cuts=-1) == EINVAL
    assert und(cuts=(0, 5)) == EINVAL and und(cuts=(-3,)) == EINVAL
    assert und(cuts=(5, 5)) == EINVAL and und(cuts=(1, 10, 5)) == EINVAL
    assert und(cuts=None, n_cuts=2) == EINVAL                              # cuts announced, none given
    # and cir_rank_undecided's own
    assert und(K=8193, ld=8193) == ESHAPE
    assert und(values=None) == EINVAL and und(pos=None) == EINVAL and und(count=None) == EINVAL and und(ld=99) == EINVAL and und(Q=0) == EINVAL
    assert und(margin=-1e-6) == EINVAL and und(margin=float("nan")) == EINVAL and und(margin=float("inf")) == EINVAL
    assert und(work=None) == EINVAL and und(work=P + 4) == EINVAL and und(bytes=ws(4, 100) - 1) == EINVAL


def test_python_surface_keeps_every_existing_call():
    import torch
    from candidate_reranking_cir_amd import cirr_test_submission_stage2 as T, ops, validate_stage2 as V
    from candidate_reranking_cir_amd.lib import CirrankError
    assert V.RECALL_CUTS == {"cirr": (1, 5, 10, 50), "fiq": (10, 50)}
    for fn, names in ((ops.rank_undecided, ("first", "cuts")), (V.refine_predictions, ("first", "cuts")),
                      (V.generate_val_predictions, ("refine_first", "refine_cuts")), (T._cirr_test_dicts, ("refine_margin",))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default in (None, ())
    with pytest.raises(CirrankError):
        ops.rank_undecided(torch.zeros(3, 5), 0.1, first=2, cuts=(1,))      # host tensors are refused, as before
    for bad in (dict(first=-1), dict(cuts=(0,)), dict(cuts=(3, 3)), dict(cuts=tuple(range(1, 10)))):
        with pytest.raises(ValueError):
            V.refine_predictions(None, None, V.RelativeValSet(None, None, None), torch.zeros(1, 1), None, torch.zeros(1), 0.1, **bad)
