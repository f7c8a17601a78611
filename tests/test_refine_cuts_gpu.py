"""Selective rank refinement end to end on a real MI355X (validate_stage2.refine_predictions with first= / cuts=): the exact mode re-scores
only the clusters that reach into the first places or straddle a recall cut-off, and the refined matrices must give the exact mode's first
places, its sets before every cut, its subset order and its metrics.

The world is tests/test_refine_gpu.py's (12 queries x 24 candidates + 5 on the tiny geometry, three skipped queries, three caption
lengths), imported from there; the margin is the bound that holds by construction, the selection is the numpy restatement's
(tests/refine_cut_cases.py), which tests/test_refine_cuts_ops_gpu.py holds the kernel to, and every comparison is equality."""
import numpy as np
import pytest
import torch

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests import refine_cases as R
from tests import refine_cut_cases as C
from tests.test_refine_gpu import K, N_QUERY, World, _bits

pytestmark = pytest.mark.gpu

MODES = ("f16", "bf16", "text32")
SELECTIONS = ((5, (10,)), (0, (1, 5, 10)))


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def world(cuda):
    return World(cuda)


def _selection(world, mode, margin, first, cuts):
    """The K-matrix entries the restatement selects (skipped rows: none)."""
    lf = world.fast(mode)[1].cpu().numpy()
    return np.stack([C.selected_links(lf[q], margin, first, cuts) if world.active[q] else np.zeros(K, dtype=bool) for q in range(N_QUERY)])


@pytest.mark.parametrize("first,cuts", SELECTIONS)
@pytest.mark.parametrize("mode", MODES)
def test_first_places_and_cut_sets_are_the_exact_modes(world, mode, first, cuts):
    V = world.V
    _, lf, gf = world.fast(mode)
    margin = world.bound(mode)
    lr, gr, stats = world.refine(mode, margin, first=first, cuts=cuts)
    sel = _selection(world, mode, margin, first, cuts)
    und, gund = world.selection(mode, margin)                               # the full rule: the subset matrix keeps it
    le, ge = world.exact_np
    print(f"\n[refine cuts tiny {mode} first={first} cuts={cuts}] margin {margin:.3e}  re-scored {stats['rescored']} (K matrix {int(sel.sum())}, "
          f"subset {int(gund.sum())}) of {stats['entries']}; the full rule: {int(und.sum() + gund.sum())}  certified: {stats['certified']}")
    assert stats["rescored"] == int(sel.sum() + gund.sum()) and stats["entries"] == int(world.active.sum()) * K + N_QUERY * 5
    assert stats["queries_rescored"] == int((sel.any(1) | gund.any(1)).sum())
    assert stats["violations"] == 0 and stats["max_deviation"] <= margin
    assert stats["first"] == first and stats["cuts"] == cuts and stats["margin"] == margin and f"first {first} places" in stats["certified"]
    assert not (sel & ~und).any()
    # selected entries are the exact mode's full-run logits, all others the fast run's, bit for bit; skipped rows are untouched
    assert torch.equal(_bits(lr), _bits(np.where(sel, le, lf.cpu().numpy()))) and torch.equal(_bits(gr), _bits(np.where(gund, ge, gf.cpu().numpy())))
    assert bool((lr[~torch.from_numpy(world.active)] == np.float32(V.SKIP_FILL)).all())
    for q in np.where(world.active)[0]:
        got, want = R.order_desc(lr[q].cpu().numpy()), R.order_desc(le[q])
        assert np.array_equal(got[:first], want[:first]), q                 # the first `first` places, in order (first=5: the first 5 places)
        for c in cuts:                                                      # the set before every cut (cuts 1, 5, 10: the first 5 as a set)
            assert set(got[:c].tolist()) == set(want[:c].tolist()), (q, c)
    for q in range(N_QUERY):
        assert np.array_equal(R.order_desc(gr[q].cpu().numpy()), R.order_desc(ge[q])), q
    ours, exact = V.compute_cirr_val_metrics(lr, gr, world.cirr), V.compute_cirr_val_metrics(*world.exact, world.cirr)
    assert ours[:6] == exact[:6]                                            # Recall_subset@1/2/3, Recall@1/5/10
    assert ours[6] == exact[6]                                              # (Recall@50 of 24 columns: every place, as a set)


def test_the_selection_is_a_real_part_of_the_full_rule(world):
    """For at least one mode and one of the selections, 0 < re-scored < the full rule's count on the K matrix (restatements only; the
    refinement tests above hold the run to them)."""
    seen = {}
    for mode in MODES:
        margin = world.bound(mode)
        full = int(world.selection(mode, margin)[0].sum())
        for first, cuts in SELECTIONS:
            seen[(mode, first, cuts)] = (int(_selection(world, mode, margin, first, cuts).sum()), full)
    print(f"\n[refine cuts tiny] K-matrix entries selected / by the full rule: {seen}")
    assert any(0 < n < full for n, full in seen.values()), seen


def test_keyword_forms_pass_the_selection_through(world):
    V = world.V
    bank, lf, gf = world.fast("f16")
    margin = world.bound("f16")
    lr, gr, stats = world.refine("f16", margin, first=5, cuts=(10,))
    kw = dict(query_batch=3, refine_margin=margin, referee_index_features=world.bank32, referee=(world.r2, world.r1), refine_first=5, refine_cuts=(10,))
    got = {}
    l1, g1 = V.generate_val_predictions(world.m2, world.m1, world.cirr, bank, refine_stats=got, **kw)
    assert torch.equal(_bits(l1), _bits(lr)) and torch.equal(_bits(g1), _bits(gr)) and got == stats
    l2, g2 = V.generate_cirr_val_predictions(world.m2, world.m1, world.cirr, bank, **kw)
    assert torch.equal(_bits(l2), _bits(lr)) and torch.equal(_bits(g2), _bits(gr))
    l3 = V.generate_fiq_val_predictions(world.m2, world.m1, world.fiq, bank, **kw)
    assert torch.equal(_bits(l3), _bits(lr))                                # the same K matrix without the subset
    # first >= K is the full rule, bit for bit, and the defaults are the present code path
    full = world.refine("f16", margin)
    same = world.refine("f16", margin, first=K)
    assert torch.equal(_bits(same[0]), _bits(full[0])) and torch.equal(_bits(same[1]), _bits(full[1])) and same[2]["rescored"] == full[2]["rescored"]
    assert full[2]["first"] is None and full[2]["cuts"] == () and "every position" in full[2]["certified"]
    # the CIRR test submission: first=50 covers all 24 columns here, so its names are the exact mode's
    from candidate_reranking_cir_amd import cirr_test_submission_stage2 as T
    names = [f"img{i}" for i in range(world.images.shape[0])]
    sub_stats = {}
    rec, sub = T.generate_cirr_test_dicts(world.m2, world.m1, world.cirr, bank, names, list(range(N_QUERY)), query_batch=3, refine_margin=10.0,
                                          referee_index_features=world.bank32, referee=(world.r2, world.r1), refine_stats=sub_stats)
    want_rec, want_sub = T.generate_cirr_test_dicts(world.r2, world.r1, world.cirr, world.bank32, names, list(range(N_QUERY)), query_batch=3)
    assert rec == want_rec and sub == want_sub and sub_stats["first"] == 50 and sub_stats["violations"] == 0


def test_refine_text32_first10_cut50_on_rank224_c100(cuda):
    """tests/golden/rank224.npz, tag c100 (4 scored queries x 105 at 224 px, full-size models), beside test_refine_gpu's case: text32 as the
    fast mode, the margin calibrated on all rows, first=10 and cuts=(50,).  The first 10 places and the set of the first 50 are the exact
    mode's full run's.  The count is printed beside the full rule's (186 of 425 when that test was written), not asserted."""
    from candidate_reranking_cir_amd import validate_stage2 as V
    from tests.test_model_gpu import DEF, build_models
    z = H.load("rank224.npz")
    g, v = H.geometry(H.FULL_BERT, dict(image_size=224))
    m2, m1 = build_models(g, v, int(z["seed"]), str(z["profile"]), DEF, cuda)
    for m in (m2, m1):
        m.set_precision("text32")
    r2, r1 = m2.referee(), m1.referee()
    images = synthetic.scene_images(range(int(z["n_index"])), 224)
    bank, bank32 = V.extract_index_features(images, m2, batch_size=64), V.extract_index_features(images, r2, batch_size=64, dtype=torch.float32)
    ds = V.RelativeValSet(ref_index=z["c100_refs"], cand_index=z["c100_cand"], labels=z["c100_labels"], captions=[str(c) for c in z["c100_caps"]],
                          group_index=z["c100_groups"], target_index=z["c100_targets"])
    active = z["c100_labels"].any(1)
    margin, raw = V.calibrate_margin(m2, m1, ds, bank, bank32, referee=(r2, r1), query_batch=4, safety=2.0)
    le, ge = V.generate_val_predictions(r2, r1, ds, bank32, query_batch=4)
    lf, gf = V.generate_val_predictions(m2, m1, ds, bank, query_batch=4)
    full = sum(int(R.undecided_links(m[q], margin)[0].sum()) for m, rows in ((lf.cpu().numpy(), np.where(active)[0]), (gf.cpu().numpy(), range(len(ds))))
               for q in rows)
    lr, gr, stats = V.refine_predictions(m2, m1, ds, lf.clone(), gf.clone(), bank32, margin, referee=(r2, r1), query_batch=4, first=10, cuts=(50,))
    print(f"\n[refine cuts rank224 c100 text32 first=10 cuts=(50,)] calibrated margin {margin:.3e} (raw max {raw:.3e})  re-scored "
          f"{stats['rescored']} of {stats['entries']} ({stats['rescored'] / stats['entries']:.3f}); the full rule: {full}")
    assert stats["entries"] == int(active.sum()) * 100 + len(ds) * 5 and stats["rescored"] <= full
    assert stats["violations"] == 0 and stats["max_deviation"] <= margin
    for q in np.where(active)[0]:
        got, want = R.order_desc(lr[q].cpu().numpy()), R.order_desc(le[q].cpu().numpy())
        assert np.array_equal(got[:10], want[:10]), q
        assert set(got[:50].tolist()) == set(want[:50].tolist()), q
    for q in range(len(ds)):
        assert np.array_equal(R.order_desc(gr[q].cpu().numpy()), R.order_desc(ge[q].cpu().numpy())), q
    assert V.compute_cirr_val_metrics(lr, gr, ds) == V.compute_cirr_val_metrics(le, ge, ds)
