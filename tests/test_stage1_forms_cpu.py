"""Stage I in the reference's call forms, host logic only (no device): item parsing of the four 'relative' layouts, the test1-schema
top-K file through `load_topk`, and the dict assembly of the metrics / test-submission functions fed with rankings made on the CPU."""
import json

import numpy as np
import pytest
import torch

from candidate_reranking_cir_amd import cirr_test_submission as T1, cirr_test_submission_stage2 as T2, validate as V1, validate_stage2 as V2
from tests import stage1_forms_cases as C


# ------------------------------------------------------------------------------------------------ item parsing
def test_parse_fiq_val_items():
    z, names = C.golden()
    q = V1.relative_queries_from_dataset(C.DuckFIQ1(names, z["refs"], z["targets"], z["fiq_caps"]), names, "fiq_val")
    np.testing.assert_array_equal(q.ref_index, z["refs"])
    np.testing.assert_array_equal(q.target_index, z["targets"])
    assert q.target_names == [names[i] for i in z["targets"]] and q.reference_names == [names[i] for i in z["refs"]]
    assert q.captions == [V2.fiq_caption(str(a), str(b)) for a, b in z["fiq_caps"]]
    assert q.group_index is None and q.pair_ids is None and len(q) == 8


@pytest.mark.parametrize("ref_slot", [0, 3, 5])
def test_parse_cirr_val_items(ref_slot):
    z, names = C.golden()
    ds = C.DuckCIRR1(names, z["refs"], z["targets"], z["cirr_caps"], z["groups"], ref_slot)
    q = V1.relative_queries_from_dataset(ds, names, "cirr_val")
    np.testing.assert_array_equal(q.ref_index, z["refs"])
    np.testing.assert_array_equal(q.target_index, z["targets"])
    assert q.group_index.shape == (8, 5)
    np.testing.assert_array_equal(q.group_index, z["groups"])                       # 6 arrive, the reference leaves wherever it sits
    assert all(len(m) == 6 and m[ref_slot] == names[r] for m, r in zip(q.group_members, z["refs"]))
    assert q.captions == [str(c) for c in z["cirr_caps"]]


def test_parse_cirr_test_items_both_stages():
    z, names = C.golden()
    shuffled = names[::-1]                                                          # names are NOT their row numbers
    row = {n: i for i, n in enumerate(shuffled)}
    q = V1.relative_queries_from_dataset(C.DuckCIRRTest1(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"], 2), shuffled, "cirr_test")
    np.testing.assert_array_equal(q.ref_index, [row[names[i]] for i in z["refs"]])
    np.testing.assert_array_equal(q.group_index, np.vectorize(lambda j: row[names[j]])(z["groups"]))
    assert q.pair_ids == [int(p) for p in z["pair_ids"]] and q.target_index is None and q.target_names is None
    ds2 = C.DuckCIRRTest2(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"], z["cirr_file_names"], 4)
    rv, refs, members, pair_ids = V2.relative_test_set_from_dataset(ds2, shuffled)
    np.testing.assert_array_equal(rv.ref_index, q.ref_index)
    np.testing.assert_array_equal(rv.group_index, q.group_index)
    np.testing.assert_array_equal(rv.cand_index, np.vectorize(row.__getitem__)(z["cirr_file_names"]))
    assert rv.labels.all() and rv.labels.shape == (8, 6) and rv.target_index is None and rv.captions == q.captions
    assert refs == q.reference_names and pair_ids == q.pair_ids
    assert members == [[names[j] for j in g] for g in z["groups"]]


def test_parse_errors():
    z, names = C.golden()
    fiq = C.DuckFIQ1(names, z["refs"], z["targets"], z["fiq_caps"])
    cirr = C.DuckCIRR1(names, z["refs"], z["targets"], z["cirr_caps"], z["groups"])
    test1 = C.DuckCIRRTest1(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"])
    test2 = C.DuckCIRRTest2(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"], z["cirr_file_names"])
    for ds, layout in ((fiq, "fiq_val"), (cirr, "cirr_val"), (test1, "cirr_test")):
        with pytest.raises(ValueError, match="duplicates"):
            V1.relative_queries_from_dataset(ds, names[:-1] + [names[0]], layout)
        with pytest.raises(KeyError):
            V1.relative_queries_from_dataset(ds, ["other"] + names[1:], layout)      # img0000 is a reference / member / target
    with pytest.raises(ValueError, match="duplicates"):
        V2.relative_test_set_from_dataset(test2, names[:-1] + [names[0]])
    with pytest.raises(KeyError):
        V2.relative_test_set_from_dataset(test2, ["other"] + names[1:])
    with pytest.raises(TypeError, match="FashionIQ val"):
        V1.relative_queries_from_dataset(cirr, names, "fiq_val")                     # 4 fields into the 3-field layout
    with pytest.raises(TypeError, match="CIRR val"):
        V1.relative_queries_from_dataset(fiq, names, "cirr_val")
    with pytest.raises(TypeError, match="CIRR test1"):
        V1.relative_queries_from_dataset(test2, names, "cirr_test")                  # a stage-II dataset (5 fields) into stage I
    with pytest.raises(TypeError, match="5 fields"):
        V2.relative_test_set_from_dataset(test1, names)                              # and the other way round
    cirr.K = 6
    with pytest.raises(TypeError, match="5 .FashionIQ. or 7 .CIRR."):                # the 5 / 7-field check of the val parser is as it was
        V2.relative_val_set_from_dataset(cirr, names)


# ------------------------------------------------------------------------------------------------ load_topk
def test_load_topk_test1_schema_round_trip(tmp_path):
    z, names = C.golden()
    path = str(tmp_path / "cirr_top_6_test1.pt")
    V1.save_topk(path, dict(sorted_index_names=z["cirr_file_names"], index_names=names, split="test1"))
    caps = [str(c) for c in z["cirr_caps"]]
    ds = V1.load_topk(path, 4, z["refs"], captions=caps, group_index=z["groups"], split="test1")
    row = {n: i for i, n in enumerate(names)}
    np.testing.assert_array_equal(ds.cand_index, np.vectorize(row.__getitem__)(z["cirr_file_names"][:, :4]))
    assert ds.labels.dtype == bool and ds.labels.shape == (8, 4) and ds.labels.all()
    assert ds.target_index is None and ds.captions == caps and ds.K == 4
    np.testing.assert_array_equal(ds.group_index, z["groups"])
    assert V1.load_topk(path, 6, z["refs"]).K == 6                                   # no split asked: no check
    with pytest.raises(ValueError, match="test1"):
        V1.load_topk(path, 4, z["refs"], split="val")


def test_load_topk_val_schema_unchanged(tmp_path):
    z, names = C.golden()
    path = str(tmp_path / "cirr_top_6_val.pt")
    V1.save_topk(path, dict(sorted_index_names=z["cirr_file_names"], target_names=[names[i] for i in z["targets"]], index_names=names,
                            labels=torch.tensor(z["cirr_file_labels"]), group_labels=torch.tensor(z["cirr_file_group_labels"]), split="val"))
    ds = V1.load_topk(path, 5, z["refs"], split="val")
    row = {n: i for i, n in enumerate(names)}
    np.testing.assert_array_equal(ds.cand_index, np.vectorize(row.__getitem__)(z["cirr_file_names"][:, :5]))   # what the loader gave before
    np.testing.assert_array_equal(ds.labels, z["cirr_file_labels"][:, :5])
    np.testing.assert_array_equal(ds.target_index, z["targets"])
    assert ds.labels.dtype == bool and not ds.labels.all()
    with pytest.raises(ValueError):
        V1.load_topk(path, 5, z["refs"], split="test1")


# ------------------------------------------------------------------------------------------------ dict assembly
def _cirr_distances(z):
    return 1 - z["cirr_pred"] @ z["pooled"].T


def test_test_dicts_assembly_against_restatement(tmp_path):
    z, names = C.golden()
    dist = _cirr_distances(z)
    ds = C.DuckCIRRTest1(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"], ref_slot=1)
    want_rec, want_sub, want_sorted = C.restate_test_dicts(dist, names, [names[i] for i in z["refs"]], [ds.members(i) for i in range(8)], z["pair_ids"])
    ranked = C.ranked_on_cpu(dist, 13, z["groups"], exclude=z["refs"])               # k = max(50, 6) capped at n_index - 1 = 13
    rec, sub, top = T1.cirr_test_dicts_from_predictions(None, None, z["refs"], z["groups"], names, z["pair_ids"], topk=6, ranked=ranked)
    assert rec == want_rec and sub == want_sub
    assert all(len(v) == 13 for v in rec.values()) and all(len(v) == 3 for v in sub.values())
    assert list(rec) == [str(int(p)) for p in z["pair_ids"]]
    assert (top["sorted_index_names"] == want_sorted[:, :6]).all() and top["index_names"] == names and top["split"] == "test1"
    assert set(top) == {"sorted_index_names", "index_names", "split"}                # cirr_test_submission.py:123-127
    # (Q, 6) groups incl. the reference are read alike; without topk only the two dicts come back
    rec6, sub6 = T1.cirr_test_dicts_from_predictions(None, None, z["refs"], C.group6(z["refs"], z["groups"]), names, z["pair_ids"], ranked=ranked)
    assert rec6 == rec and sub6 == sub
    with pytest.raises(ValueError, match="13"):
        T1.cirr_test_dicts_from_predictions(None, None, z["refs"], z["groups"], names, z["pair_ids"], topk=14, ranked=ranked)
    # the two server files, through the stage-II writer: keys in sort_keys order
    p1, p2 = T2.write_submissions(str(tmp_path), "t", rec, sub)
    for path, want, metric in ((p1, want_rec, "recall"), (p2, want_sub, "recall_subset")):
        pairs = json.load(open(path), object_pairs_hook=list)
        assert [k for k, _ in pairs] == sorted(list(want) + ["version", "metric"])
        assert dict(pairs) == dict(want, version="rc2", metric=metric)


def test_cirr_metrics_assembly_against_golden_and_restatement():
    z, names = C.golden()
    dist, k = _cirr_distances(z), int(z["k"])
    g6 = C.group6(z["refs"], z["groups"])
    cols = V1.cirr_rank_cols(z["refs"], z["targets"], g6)
    want_metrics, want_sorted, want_labels, want_glabels = C.restate_cirr_val(
        dist, names, [names[i] for i in z["refs"]], [names[i] for i in z["targets"]], [[names[j] for j in row] for row in g6])
    metrics, top = V1.cirr_metrics_from_predictions(None, None, z["refs"], z["targets"], z["groups"], names, "val", topk=k,
                                                    ranked=C.ranked_on_cpu(dist, k, cols, exclude=z["refs"]))
    assert metrics == want_metrics
    np.testing.assert_allclose(metrics, z["cirr_metrics"], atol=1e-4)
    assert (top["sorted_index_names"] == want_sorted[:, :k]).all() and (top["sorted_index_names"] == z["cirr_file_names"]).all()
    assert torch.equal(top["labels"], want_labels[:, :k]) and (top["labels"].numpy() == z["cirr_file_labels"]).all()
    assert torch.equal(top["group_labels"], want_glabels) and (top["group_labels"].numpy() == z["cirr_file_group_labels"]).all()
    assert top["target_names"] == [names[i] for i in z["targets"]] and top["split"] == "val" and top["index_names"] == names
    only = V1.cirr_metrics_from_predictions(None, None, z["refs"], z["targets"], g6, names, "val",
                                            ranked=C.ranked_on_cpu(dist, 1, cols, exclude=z["refs"]))            # metrics alone: k = 1
    assert only == metrics and len(only) == 7
    with pytest.raises(ValueError, match="13"):
        V1.cirr_metrics_from_predictions(None, None, z["refs"], z["targets"], g6, names, "val", topk=14)


def test_fiq_metrics_assembly_against_golden():
    z, names = C.golden()
    dist, k = 1 - z["fiq_pred"] @ z["pooled"].T, int(z["k"])
    ranked = C.ranked_on_cpu(dist, k, z["targets"][:, None])
    metrics, top = V1.fiq_metrics_from_predictions(None, None, z["targets"], names, "val", ["dress"], topk=k, ranked=ranked)
    np.testing.assert_allclose(metrics, z["fiq_metrics"], atol=1e-4)
    assert (top["sorted_index_names"] == z["fiq_file_names"]).all() and (top["labels"].numpy() == z["fiq_file_labels"]).all()
    assert top["target_names"] == [str(t) for t in z["fiq_file_targets"]]
    assert top["dress_types"] == str(z["fiq_file_dress"]) and top["split"] == str(z["fiq_file_split"])
    want_sorted = C.sorted_names_of(dist, names)
    assert (top["sorted_index_names"] == want_sorted[:, :k]).all()
    assert V1.fiq_metrics_from_predictions(None, None, z["targets"], names, "val", "dress", ranked=C.ranked_on_cpu(dist, 1, z["targets"][:, None])) == metrics
    assert V1.fiq_metrics_from_predictions(None, None, z["targets"], names, "val", ["dress", "shirt"], topk=2, ranked=ranked)[1]["dress_types"] == "dress,shirt"
    with pytest.raises(ValueError, match="13"):
        V1.fiq_metrics_from_predictions(None, None, z["targets"], names, "val", "dress", topk=0)


def test_save_path_needs_topk():
    with pytest.raises(ValueError, match="topk"):
        V1._finish(((0.0, 0.0),), None, "x.pt")
