"""Rank refinement end to end on a real MI355X (validate_stage2.refine_predictions, calibrate_margin, the referee twins): a fast precision
mode scores everything, the exact mode re-scores only the entries whose order the fast logits cannot decide, and the refined matrices must
sort exactly as the exact mode's own full run.

The loop tests run on the tiny geometry of tests/golden/tiny_loop.npz (its weights, seed and profile) with a CIRR-shaped split built
here - 12 queries x 24 candidates over a 40-image bank, the 5-member subsets, three skipped queries, captions of three lengths - because
the fixture's own 6 candidates per row leave almost no close pairs.  The expected matrices come from the two full runs of the same test,
so the margin holds by construction and every comparison is bit equality; the selection is the numpy restatement's (tests/refine_cases.py),
which tests/test_refine_ops_gpu.py holds the kernel to."""
import json
import warnings

import numpy as np
import pytest
import torch

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H
from tests import refine_cases as R

pytestmark = pytest.mark.gpu

N_INDEX, N_QUERY, K = 40, 12, 24
SKIPPED = (2, 7, 10)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _tiny_models(cuda):
    from tests.test_model_gpu import DEF, build_models
    z = H.load("tiny_loop.npz")
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    m2, m1 = build_models(g, v, int(z["seed"]), str(z["profile"]), DEF, cuda)
    return z, v, m2, m1


def _split():
    from candidate_reranking_cir_amd import validate_stage2 as V
    rng = np.random.default_rng(7)
    refs = np.arange(N_QUERY, dtype=np.int64) * 3 % N_INDEX
    cand = np.stack([rng.permutation(np.delete(np.arange(N_INDEX), r))[:K] for r in refs]).astype(np.int64)
    labels = np.zeros((N_QUERY, K), dtype=bool)
    for q in range(N_QUERY):
        if q not in SKIPPED:
            labels[q, rng.integers(K)] = True
    targets = np.array([cand[q, int(np.argmax(labels[q]))] for q in range(N_QUERY)], dtype=np.int64)
    groups = np.stack([np.concatenate([[targets[q]], rng.permutation(np.setdiff1d(np.arange(N_INDEX), [refs[q], targets[q]]))[:4]])
                       for q in range(N_QUERY)]).astype(np.int64)
    caps = [synthetic.caption_text(q, (4, 9, 17)[q % 3]) for q in range(N_QUERY)]
    cirr = V.RelativeValSet(ref_index=refs, cand_index=cand, labels=labels, captions=caps, group_index=groups, target_index=targets)
    fiq = V.RelativeValSet(ref_index=refs, cand_index=cand, labels=labels, captions=caps)
    return cirr, fiq


class World:
    """The models (precision switched per test), their referee twins, the exact-mode bank and the exact mode's full run."""

    def __init__(self, cuda):
        from candidate_reranking_cir_amd import validate_stage2 as V
        self.V = V
        z, v, self.m2, self.m1 = _tiny_models(cuda)
        self.r2, self.r1 = self.m2.referee(), self.m1.referee()
        self.images = H.fixture_images(z, range(N_INDEX), v.image_size)
        self.cirr, self.fiq = _split()
        self.active = self.cirr.labels.any(axis=1)
        self.bank32 = V.extract_index_features(self.images, self.r2, dtype=torch.float32)
        self.exact = V.generate_val_predictions(self.r2, self.r1, self.cirr, self.bank32, query_batch=5)
        self.exact_np = [t.cpu().numpy() for t in self.exact]
        self._fast = {}

    def fast(self, mode):
        """(bank, logits, subset logits) of the fast mode's full run; the primaries are left in that mode."""
        for m in (self.m2, self.m1):
            m.set_precision(mode)
        if mode not in self._fast:
            bank = self.V.extract_index_features(self.images, self.m2)
            lf, gf = self.V.generate_val_predictions(self.m2, self.m1, self.cirr, bank, query_batch=3)
            self._fast[mode] = (bank, lf, gf)
        return self._fast[mode]

    def bound(self, mode):
        """max |fast - exact| over every scored entry, taken in float64 and rounded UP to fp32: the margin that holds by construction."""
        _, lf, gf = self.fast(mode)
        d = max(np.abs(lf.cpu().numpy().astype(np.float64) - self.exact_np[0])[self.active].max(),
                np.abs(gf.cpu().numpy().astype(np.float64) - self.exact_np[1]).max())
        m = np.float32(d)
        return float(m if float(m) >= d else np.nextafter(m, np.float32(np.inf)))

    def selection(self, mode, margin):
        """The undecided entries of the fast matrices by the restatement: (K-matrix mask, subset mask)."""
        _, lf, gf = self.fast(mode)
        lf, gf = lf.cpu().numpy(), gf.cpu().numpy()
        und = np.stack([R.undecided_links(lf[q], margin)[0] if self.active[q] else np.zeros(K, dtype=bool) for q in range(N_QUERY)])
        gund = np.stack([R.undecided_links(gf[q], margin)[0] for q in range(N_QUERY)])
        return und, gund

    def refine(self, mode, margin, **kw):
        bank, lf, gf = self.fast(mode)
        kw.setdefault("referee", (self.r2, self.r1))
        return self.V.refine_predictions(self.m2, self.m1, self.cirr, lf.clone(), gf.clone(), self.bank32, margin, query_batch=3, **kw)


@pytest.fixture(scope="module")
def world(cuda):
    return World(cuda)


def _bits(t):
    return (t.cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).view(torch.int32)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("mode", ["f16", "bf16", "text32"])
def test_refined_matrices_sort_as_the_referees(world, mode):
    V = world.V
    _, lf, gf = world.fast(mode)
    margin = world.bound(mode)
    lr, gr, stats = world.refine(mode, margin)
    und, gund = world.selection(mode, margin)
    le, ge = world.exact_np
    share = stats["rescored"] / stats["entries"]
    print(f"\n[refine tiny {mode}] margin {margin:.3e}  re-scored {stats['rescored']} of {stats['entries']} entries ({share:.3f}) in "
          f"{stats['queries_rescored']} queries  max deviation {stats['max_deviation']:.3e}")
    assert stats["entries"] == int(world.active.sum()) * K + N_QUERY * 5 and stats["rescored"] == int(und.sum() + gund.sum())
    assert stats["queries_rescored"] == int((und.any(1) | gund.any(1)).sum()) and stats["margin"] == margin
    assert stats["violations"] == 0 and stats["max_deviation"] <= margin
    if mode == "f16":
        assert 0 < stats["rescored"] < stats["entries"]                    # the mixed path: some entries re-scored, some kept
    # re-scored entries are the referee's full-run logits, the others the fast run's, bit for bit; skipped rows are untouched
    assert torch.equal(_bits(lr), _bits(np.where(und, le, lf.cpu().numpy()))) and torch.equal(_bits(gr), _bits(np.where(gund, ge, gf.cpu().numpy())))
    assert bool((lr[~torch.from_numpy(world.active)] == np.float32(V.SKIP_FILL)).all())
    for q in np.where(world.active)[0]:
        assert np.array_equal(R.order_desc(lr[q].cpu().numpy()), R.order_desc(le[q])), q
    for q in range(N_QUERY):
        assert np.array_equal(R.order_desc(gr[q].cpu().numpy()), R.order_desc(ge[q])), q
    assert V.compute_cirr_val_metrics(lr, gr, world.cirr) == V.compute_cirr_val_metrics(*world.exact, world.cirr)


# ------------------------------------------------------------------------------------------------ (b)
def test_margin_zero_touches_nothing_and_packs_no_referee(world):
    _, lf, gf = world.fast("f16")
    r2, r1 = world.m2.referee(), world.m1.referee()
    lr, gr, stats = world.refine("f16", 0.0, referee=(r2, r1))
    assert stats["rescored"] == 0 and stats["violations"] == 0 and stats["queries_rescored"] == 0
    assert torch.equal(_bits(lr), _bits(lf)) and torch.equal(_bits(gr), _bits(gf))
    assert r2._engines is None and r1._engines is None


# ------------------------------------------------------------------------------------------------ (c)
def test_a_margin_above_the_logit_range_gives_the_referees_matrices(world):
    lr, gr, stats = world.refine("f16", 10.0)
    assert stats["rescored"] == stats["entries"] and stats["violations"] == 0 and stats["queries_rescored"] == N_QUERY
    assert torch.equal(_bits(lr), _bits(world.exact[0])) and torch.equal(_bits(gr), _bits(world.exact[1]))


# ------------------------------------------------------------------------------------------------ (d)
def test_a_margin_that_is_too_small_is_reported(world):
    V = world.V
    _, lf, gf = world.fast("f16")
    margin = float(np.float32(world.bound("f16") / 2))
    und, gund = world.selection("f16", margin)
    dev = np.concatenate([np.abs(lf.cpu().numpy() - world.exact_np[0])[und], np.abs(gf.cpu().numpy() - world.exact_np[1])[gund]])      # fp32
    want_bad = int((dev > np.float32(margin)).sum())
    assert want_bad > 0, "premise of this test: an undecided entry deviates by more than half the bound"
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _, _, stats = world.refine("f16", margin)
    assert len([w for w in seen if issubclass(w.category, RuntimeWarning) and "not certified" in str(w.message)]) == 1
    assert stats["violations"] == want_bad and np.float32(stats["max_deviation"]) == dev.max()
    with pytest.raises(V.RefineBoundError, match="not certified"):
        world.refine("f16", margin, on_violation="raise")


# ------------------------------------------------------------------------------------------------ (e)
def test_referee_twins_share_parameters_and_follow_their_writes(cuda):
    from candidate_reranking_cir_amd import train
    _, v, m2, m1 = _tiny_models(cuda)
    m2.set_precision("bf16")
    for m in (m2, m1):
        before = (m.precision, m._engines, m.graph_candidates)
        t = m.referee()
        assert type(t) is type(m) and t.precision == "exact" and t.vit_geometry == m.vit_geometry and t.bert_geometry is m.bert_geometry
        assert (m.precision, m._engines, m.graph_candidates) == before                      # the primary is untouched
        mine, theirs = dict(m.named_parameters()), dict(t.named_parameters())
        assert list(mine) == list(theirs) and all(mine[n] is theirs[n] for n in mine)        # shared by identity: no second fp32 copy
        assert t.text_encoder is not m.text_encoder and t.weights_key() == m.weights_key()
    t2 = m2.referee()
    img = synthetic.images(range(2), v.image_size).to(cuda)
    assert m2.img_embed16(img).dtype == torch.bfloat16 and t2.img_embed(img).dtype == torch.float32
    own, twin = m2.engines(), t2.engines()
    assert own[1] is not twin[1] and twin[1].dtype == torch.float32 and own[1].dtype == torch.bfloat16
    assert t2.engines()[1] is twin[1]                                                      # nothing written: no repack
    # train.AdamW.step on the primary's parameters: both sides repack their text engines
    p = next(p for n, p in m2.named_parameters() if n.startswith("cls_head."))
    p.grad = torch.full_like(p, 1e-3)
    train.AdamW([p], lr=1e-3).step()
    after_own, after_twin = m2.engines(), t2.engines()
    assert after_own[1] is not own[1] and after_twin[1] is not twin[1]
    # a copying load_state_dict on the primary: both again
    m2.load_state_dict({k: val.clone() for k, val in m2.state_dict().items()})
    assert t2.engines()[1] is not after_twin[1] and m2.engines()[1] is not after_own[1]
    # writes no counter sees: invalidate_packed_weights on the primary reaches the live twin
    held = t2.engines()
    m2.invalidate_packed_weights()
    now = t2.engines()
    assert now[0] is not held[0] and now[1] is not held[1]
    # load_state_dict(assign=True) replaces the primary's Parameter objects: the sharing is broken (documented)
    m2.load_state_dict({k: val.clone() for k, val in m2.state_dict().items()}, assign=True)
    assert next(m2.parameters()) is not next(t2.parameters())


# ------------------------------------------------------------------------------------------------ (f)
def test_keyword_forms_equal_refine_predictions(world):
    V = world.V
    bank, lf, gf = world.fast("f16")
    margin = world.bound("f16")
    lr, gr, stats = world.refine("f16", margin)
    kw = dict(query_batch=3, refine_margin=margin, referee_index_features=world.bank32, referee=(world.r2, world.r1))
    got = {}
    l1, g1 = V.generate_val_predictions(world.m2, world.m1, world.cirr, bank, refine_stats=got, **kw)
    assert torch.equal(_bits(l1), _bits(lr)) and torch.equal(_bits(g1), _bits(gr)) and got == stats
    l2, g2 = V.generate_cirr_val_predictions(world.m2, world.m1, world.cirr, bank, **kw)
    assert torch.equal(_bits(l2), _bits(lr)) and torch.equal(_bits(g2), _bits(gr))
    plain = V.generate_fiq_val_predictions(world.m2, world.m1, world.fiq, bank, query_batch=3)
    want, _, fstats = V.refine_predictions(world.m2, world.m1, world.fiq, plain.clone(), None, world.bank32, margin, referee=(world.r2, world.r1),
                                           query_batch=3)
    l3 = V.generate_fiq_val_predictions(world.m2, world.m1, world.fiq, bank, **kw)
    assert torch.equal(_bits(l3), _bits(want)) and fstats["entries"] == int(world.active.sum()) * K and not torch.equal(_bits(l3), _bits(plain))
    with pytest.raises(ValueError, match="referee_index_features"):
        V.generate_val_predictions(world.m2, world.m1, world.cirr, bank, refine_margin=margin)
    # the default is the present code path: no keyword, the fast run as it always was
    assert torch.equal(_bits(V.generate_val_predictions(world.m2, world.m1, world.cirr, bank, query_batch=3)[0]), _bits(lf))


def test_calibrate_margin_on_a_sample(world):
    V = world.V
    bank, lf, gf = world.fast("f16")
    sample = [0, 1, 4, 7, 9]
    margin, raw = V.calibrate_margin(world.m2, world.m1, world.cirr, bank, world.bank32, rows=sample, referee=(world.r2, world.r1), query_batch=3,
                                     safety=2.0)
    fast = V.generate_val_predictions(world.m2, world.m1, world.cirr, bank, query_batch=3, rows=sample)
    exact = V.generate_val_predictions(world.r2, world.r1, world.cirr, world.bank32, query_batch=3, rows=sample)
    want = max(float(np.abs(f.cpu().numpy().astype(np.float64) - e.cpu().numpy()).max()) for f, e in zip(fast, exact))
    assert raw == want and 0.0 < 2.0 * raw <= margin <= 2.0 * raw * (1 + 1e-6)
    assert torch.equal(_bits(exact[0]), _bits(world.exact[0][sample]))                     # the exact mode does not depend on the batch


# ------------------------------------------------------------------------------------------------ the real geometry
def test_refine_text32_on_rank224_c100(cuda):
    """tests/golden/rank224.npz, tag c100 (4 scored queries x 105 at 224 px, full-size models): text32 as the fast mode, the margin
    calibrated here on all rows.  The refined order equals the exact mode's at every position, so its agreement with the reference's own
    order is the exact mode's."""
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
    lr, gr = V.generate_val_predictions(m2, m1, ds, bank, query_batch=4)
    lf = lr.clone()
    lr, gr, stats = V.refine_predictions(m2, m1, ds, lr, gr, bank32, margin, referee=(r2, r1), query_batch=4)
    share = stats["rescored"] / stats["entries"]
    agree = lambda a: float(np.mean([np.mean(R.order_desc(a[q]) == R.order_desc(z["c100_logits"][q])) for q in np.where(active)[0]]))
    print(f"\n[refine rank224 c100 text32] calibrated margin {margin:.3e} (raw max {raw:.3e})  re-scored {stats['rescored']} of {stats['entries']} "
          f"({share:.3f})  positions equal to the reference's: fast {agree(lf.cpu().numpy()):.4f}  refined {agree(lr.cpu().numpy()):.4f}  "
          f"exact {agree(le.cpu().numpy()):.4f}")
    assert stats["entries"] == int(active.sum()) * 100 + len(ds) * 5 and 0 < stats["rescored"] < stats["entries"]
    assert stats["violations"] == 0 and stats["max_deviation"] <= margin
    for q in np.where(active)[0]:
        assert np.array_equal(R.order_desc(lr[q].cpu().numpy()), R.order_desc(le[q].cpu().numpy())), q
    for q in range(len(ds)):
        assert np.array_equal(R.order_desc(gr[q].cpu().numpy()), R.order_desc(ge[q].cpu().numpy())), q
    assert agree(lr.cpu().numpy()) == agree(le.cpu().numpy())
    assert V.compute_cirr_val_metrics(lr, gr, ds) == V.compute_cirr_val_metrics(le, ge, ds)
