"""Stage I in the reference's call forms on the HIP path: validation metrics and top-K files (validate.py), the CIRR test submission
(cirr_test_submission.py), the test-split top-K file into stage II (cirr_test_submission_stage2.py) - against the reference's goldens
(tests/golden/stage1_tiny.npz) and restatements of the reference's ranking code (tests/stage1_forms_cases.py)."""
import json

import numpy as np
import pytest
import torch

from candidate_reranking_cir_amd import synthetic
from tests import helpers as H, stage1_forms_cases as C
from tests.test_model_gpu import build_models, margin_order_ok

pytestmark = pytest.mark.gpu

BIG_SEED = 28           # see test_index_above_8192: seeds 0-27 leave neighbouring distances within a few ulp of each other (0, 1, 8: equal)


@pytest.fixture(scope="module")
def s1():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import validate_stage2 as V2
    z, names = C.golden()
    g, v = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))
    m2, m1 = build_models(g, v, int(z["seed"]), str(z["profile"]), torch.float16, torch.device("cuda"))
    images = synthetic.images(range(14), v.image_size)
    tokens32, pooled = m1.img_embed(images, return_pool_and_normalized=True)       # what utils.py:57-72 hands the reference's callers
    feats32 = m2.img_embed(images.cuda())                                           # utils.py:43-55, stage II
    bank2 = V2.extract_index_features(images, m2)
    return dict(z=z, names=names, v=v, m2=m2, m1=m1, tokens32=tokens32, pooled=pooled, feats32=feats32, bank2=bank2)


def _datasets(z, names):
    fiq = C.DuckFIQ1(names, z["refs"], z["targets"], z["fiq_caps"])
    cirr = C.DuckCIRR1(names, z["refs"], z["targets"], z["cirr_caps"], z["groups"], ref_slot=2)
    test1 = C.DuckCIRRTest1(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"], ref_slot=4)
    return fiq, cirr, test1


def test_reference_form_predictions(s1):
    """generate_*_val_predictions (validate.py:102-149, 271-316): the native call's features bit for bit, the reference's within the
    bound tests/test_stage1_gpu.py holds the same quantities to (2e-3: fp16 operands, unit-norm features), names in dataset order."""
    from candidate_reranking_cir_amd import validate as V1, validate_stage2 as V2
    z, names, m1 = s1["z"], s1["names"], s1["m1"]
    fiq, cirr, _ = _datasets(z, names)
    bank = V1.extract_index_features(synthetic.images(range(14), s1["v"].image_size), m1)[0]
    fpred, ftargets = V1.generate_fiq_val_predictions(m1, fiq, names, s1["tokens32"])
    cpred, crefs, ctargets, cmembers = V1.generate_cirr_val_predictions(m1, cirr, names, s1["tokens32"])
    assert fpred.shape == (8, 256) and fpred.dtype == torch.float32 and fpred.is_cuda and cpred.shape == (8, 256)
    assert torch.equal(fpred, V1.generate_val_predictions(m1, z["refs"], [V2.fiq_caption(str(a), str(b)) for a, b in z["fiq_caps"]], bank))
    assert torch.equal(cpred, V1.generate_val_predictions(m1, z["refs"], [str(c) for c in z["cirr_caps"]], bank))
    assert torch.equal(cpred, V1.generate_cirr_val_predictions(m1, cirr, names, bank)[0])          # the 16-bit bank is taken as it is
    e_f, e_c = np.abs(fpred.cpu().numpy() - z["fiq_pred"]).max(), np.abs(cpred.cpu().numpy() - z["cirr_pred"]).max()
    print(f"\n[stage-I reference forms] fiq query feature {e_f:.2e}  cirr query feature {e_c:.2e}")
    assert e_f < 2e-3 and e_c < 2e-3
    assert ftargets == [names[i] for i in z["targets"]] and ctargets == ftargets and crefs == [names[i] for i in z["refs"]]
    assert cmembers == [cirr.members(i) for i in range(8)] and all(len(m) == 6 for m in cmembers)


def test_metrics_and_files_from_golden_features(s1):
    """*_metrics_from_predictions on the reference's own features: its metrics and its top-K files, through rank_index_topk."""
    from candidate_reranking_cir_amd import validate as V1
    z, names = s1["z"], s1["names"]
    k = int(z["k"])
    pooled = torch.tensor(z["pooled"]).cuda()
    metrics, top = V1.cirr_metrics_from_predictions(torch.tensor(z["cirr_pred"]).cuda(), pooled, z["refs"], z["targets"],
                                                    C.group6(z["refs"], z["groups"]), names, "val", topk=k)
    np.testing.assert_allclose(metrics, z["cirr_metrics"], atol=1e-4)
    assert (top["sorted_index_names"] == z["cirr_file_names"]).all() and (top["labels"].numpy() == z["cirr_file_labels"]).all()
    assert (top["group_labels"].numpy() == z["cirr_file_group_labels"]).all() and top["split"] == str(z["cirr_file_split"])
    only = V1.cirr_metrics_from_predictions(torch.tensor(z["cirr_pred"]).cuda(), pooled, z["refs"], z["targets"], z["groups"], names, "val")
    assert only == metrics and len(only) == 7
    fmetrics, ftop = V1.fiq_metrics_from_predictions(torch.tensor(z["fiq_pred"]).cuda(), pooled, z["targets"], names, "val", ["dress"], topk=k)
    np.testing.assert_allclose(fmetrics, z["fiq_metrics"], atol=1e-4)
    assert (ftop["sorted_index_names"] == z["fiq_file_names"]).all() and (ftop["labels"].numpy() == z["fiq_file_labels"]).all()
    assert ftop["target_names"] == [str(t) for t in z["fiq_file_targets"]] and ftop["dress_types"] == str(z["fiq_file_dress"])
    assert V1.fiq_metrics_from_predictions(torch.tensor(z["fiq_pred"]).cuda(), pooled.cpu(), z["targets"], names, "val", "dress") == fmetrics
    with pytest.raises(ValueError, match="13"):
        V1.fiq_metrics_from_predictions(torch.tensor(z["fiq_pred"]).cuda(), pooled, z["targets"], names, "val", "dress", topk=14)


def test_reference_form_metrics_and_saved_file(s1, tmp_path):
    """compute_*_val_metrics (validate.py:33-36, 176-179; stage1_train.py:244, 459) == *_from_predictions(generate_*(...)); topk= and
    save_path= write a file load_topk reads back to the same rows; our distances keep the reference's order wherever its gap is real."""
    from candidate_reranking_cir_amd import validate as V1
    z, names, m1, tokens32, pooled = s1["z"], s1["names"], s1["m1"], s1["tokens32"], s1["pooled"]
    fiq, cirr, _ = _datasets(z, names)
    k = int(z["k"])
    cpred = V1.generate_cirr_val_predictions(m1, cirr, names, tokens32)[0]
    fpred = V1.generate_fiq_val_predictions(m1, fiq, names, tokens32)[0]
    want_c, want_ctop = V1.cirr_metrics_from_predictions(cpred, pooled, z["refs"], z["targets"], z["groups"], names, "val", topk=k)
    want_f, want_ftop = V1.fiq_metrics_from_predictions(fpred, pooled, z["targets"], names, "val", ["dress"], topk=k)
    assert V1.compute_cirr_val_metrics(cirr, m1, tokens32, pooled, names) == want_c
    assert V1.compute_fiq_val_metrics(fiq, m1, tokens32, pooled, names) == want_f
    cpath, fpath = str(tmp_path / "cirr_top_6_val.pt"), str(tmp_path / "fiq_top_6_val_dress.pt")
    got_c, ctop = V1.compute_cirr_val_metrics(cirr, m1, tokens32, pooled, names, topk=k, save_path=cpath)
    got_f, ftop = V1.compute_fiq_val_metrics(fiq, m1, tokens32, pooled, names, topk=k, save_path=fpath)
    assert got_c == want_c and got_f == want_f
    row = {n: i for i, n in enumerate(names)}
    for path, top, want in ((cpath, ctop, want_ctop), (fpath, ftop, want_ftop)):
        assert (top["sorted_index_names"] == want["sorted_index_names"]).all() and torch.equal(top["labels"], want["labels"])
        ds = V1.load_topk(path, k, z["refs"], split="val")
        np.testing.assert_array_equal(ds.cand_index, np.vectorize(row.__getitem__)(top["sorted_index_names"]))
        np.testing.assert_array_equal(ds.labels, top["labels"].numpy())
        np.testing.assert_array_equal(ds.target_index, z["targets"])
    assert ftop["dress_types"] == "dress" and ctop["split"] == "val"
    with pytest.raises(ValueError, match="topk"):
        V1.compute_cirr_val_metrics(cirr, m1, tokens32, pooled, names, save_path=cpath)
    print(f"\n[stage-I reference forms] cirr {np.round(got_c, 2)} (reference {np.round(z['cirr_metrics'], 2)})  fiq {np.round(got_f, 2)} "
          f"(reference {np.round(z['fiq_metrics'], 2)})")
    ref_dist = 1 - z["cirr_pred"] @ z["pooled"].T
    ours = 1 - cpred.cpu().numpy() @ pooled.cpu().numpy().T
    for q in range(len(ours)):                                          # order kept wherever the reference gap is real
        assert margin_order_ok(-ours[q], -ref_dist[q], 2e-3)


def test_stage1_test_dicts_from_golden_features(s1):
    """cirr_test_dicts_from_predictions == cirr_test_submission.py:96-115 restated, on the reference's own features."""
    from candidate_reranking_cir_amd import cirr_test_submission as T1
    z, names = s1["z"], s1["names"]
    test1 = _datasets(z, names)[2]
    want_rec, want_sub, want_sorted = C.restate_test_dicts(1 - z["cirr_pred"] @ z["pooled"].T, names, [names[i] for i in z["refs"]],
                                                           [test1.members(i) for i in range(8)], z["pair_ids"])
    pred, pooled = torch.tensor(z["cirr_pred"]).cuda(), torch.tensor(z["pooled"]).cuda()
    rec, sub = T1.cirr_test_dicts_from_predictions(pred, pooled, z["refs"], z["groups"], names, z["pair_ids"])
    assert rec == want_rec and sub == want_sub
    assert all(len(r) == 13 for r in rec.values()) and all(len(r) == 3 for r in sub.values())
    rec6, sub6, top = T1.cirr_test_dicts_from_predictions(pred, pooled, z["refs"], z["groups"], names, z["pair_ids"], topk=6)
    assert rec6 == rec and sub6 == sub
    assert (top["sorted_index_names"] == want_sorted[:, :6]).all() and top["index_names"] == names and top["split"] == "test1"


def _reference_margins_agree(s1, rec, cand_idx):
    """The margin rule of tests/test_stage1_gpu.py::test_cirr_test_dicts_hip_vs_reference: wherever the reference's logits (the oracle's,
    equal to 2e-5) leave a gap above the fp16 bound on both sides of a position, `rec` holds the reference's name there."""
    from oracle import cir_oracle as O
    z, v = s1["z"], s1["v"]
    g = H.geometry(json.loads(str(z["bert_cfg"])), json.loads(str(z["vit_cfg"])))[0]
    ref_rec = json.loads(str(z["test_recall_json"]))
    sd2, sd1 = H.state_dicts(g, v, int(z["seed"]), str(z["profile"]))
    agree = total = 0
    with torch.no_grad():
        feats = O.img_embed(sd2, synthetic.images(range(14), v.image_size))
        for q, cap in enumerate(z["cirr_caps"]):
            ids, mask = H.tokenize([str(cap)])
            lg, glg = O.score_queries(sd2, sd1, feats, [int(z["refs"][q])], cand_idx[q:q + 1], np.ones((1, cand_idx.shape[1]), dtype=bool),
                                      ids, mask, group_index=z["groups"][q:q + 1])
            pid = str(int(z["pair_ids"][q]))
            order = np.argsort(-lg[0].numpy(), kind="stable")
            gaps = np.abs(np.diff(lg[0].numpy()[order]))
            for pos in range(len(order)):
                clear = (pos == 0 or gaps[pos - 1] > 4e-4) and (pos == len(order) - 1 or gaps[pos] > 4e-4)
                if clear:
                    total += 1
                    agree += rec[pid][pos] == ref_rec[pid][pos]
    return agree, total


def test_stage1_to_stage2_test_chain(s1, tmp_path):
    """Stage-I test predictions -> the test-split top-K file -> load_topk(split="test1") -> stage II's dicts: the reference form over
    5-field items (data_utils.py:346) gives the native form's dicts, and those agree with the reference's submission files."""
    from candidate_reranking_cir_amd import cirr_test_submission as T1, cirr_test_submission_stage2 as T2, validate as V1
    z, names, m1, m2 = s1["z"], s1["names"], s1["m1"], s1["m2"]
    test1 = _datasets(z, names)[2]
    k, path = int(z["k"]), str(tmp_path / "cirr_top_6_test1.pt")
    pred, refs, members, pair_ids = T1.generate_cirr_test_predictions(m1, test1, names, s1["tokens32"])
    assert refs == [names[i] for i in z["refs"]] and pair_ids == [int(p) for p in z["pair_ids"]] and members == [test1.members(i) for i in range(8)]
    assert torch.equal(pred, V1.generate_cirr_val_predictions(m1, _datasets(z, names)[1], names, s1["tokens32"])[0])     # same rows, same captions
    rec1, sub1, top = T1.generate_cirr_test_dicts(test1, m1, s1["tokens32"], s1["pooled"], names, topk=k, save_path=path)
    want = T1.cirr_test_dicts_from_predictions(pred, s1["pooled"], z["refs"], z["groups"], names, z["pair_ids"], topk=k)
    assert (rec1, sub1) == want[:2] and (top["sorted_index_names"] == want[2]["sorted_index_names"]).all()
    assert all(r[:k] == row.tolist() for r, row in zip(rec1.values(), top["sorted_index_names"]))
    caps = [str(c) for c in z["cirr_caps"]]
    ds = V1.load_topk(path, k, z["refs"], captions=caps, group_index=z["groups"], split="test1")
    assert ds.labels.all() and ds.target_index is None
    native = T2.generate_cirr_test_dicts(m2, m1, ds, s1["bank2"], names, z["pair_ids"], query_batch=3)
    test2 = C.DuckCIRRTest2(names, z["refs"], z["cirr_caps"], z["groups"], z["pair_ids"], top["sorted_index_names"], ref_slot=1)
    assert T2.generate_cirr_test_dicts(test2, m2, m1, s1["feats32"], names, query_batch=3) == native
    lg, glg, refs2, members2, pair_ids2 = T2.generate_cirr_test_predictions(m2, m1, test2, names, s1["feats32"], query_batch=3)
    assert lg.shape == (8, k) and glg.shape == (8, 5) and refs2 == refs and pair_ids2 == pair_ids
    assert members2 == [[names[j] for j in row] for row in z["groups"]]
    rec, sub = native
    ref_rec, ref_sub = json.loads(str(z["test_recall_json"])), json.loads(str(z["test_subset_json"]))
    assert set(rec) == set(ref_rec) and all(sorted(rec[p]) == sorted(ref_rec[p]) for p in rec)     # same candidate sets
    agree, total = _reference_margins_agree(s1, rec, ds.cand_index)
    print(f"\n[stage I -> stage II test dicts] positions with a clear reference margin: {agree}/{total} identical")
    assert total > 0 and agree == total
    assert all(len(r) == 3 for r in sub.values()) and set(sub) == set(ref_sub)


def big_case(seed: int, n_index: int = 9000, n_q: int = 4, k: int = 100):
    """4 unit queries against 9000 unit index rows (above the 8192 columns `rank_index` sorts), each with a reference, 5 further group
    members and the target among them.  `margin`: the smallest gap between neighbouring distances of a row within its first k + 2
    columns and on both sides of every `cols` rank - what a ranking made from another matmul's bits has to spare."""
    gen = torch.Generator().manual_seed(seed)
    pooled = torch.nn.functional.normalize(torch.randn((n_index, 256), generator=gen), dim=-1)
    pred = torch.nn.functional.normalize(torch.randn((n_q, 256), generator=gen), dim=-1)
    picks = torch.stack([torch.randperm(n_index, generator=gen)[:6] for _ in range(n_q)]).numpy()
    refs, groups, targets = picks[:, 0], picks[:, 1:], picks[np.arange(n_q), 1 + np.arange(n_q) % 5]
    dist = 1 - pred @ pooled.T
    order = torch.argsort(dist, dim=-1, stable=True).numpy()
    margin = np.inf
    for q in range(n_q):
        row = order[q][order[q] != refs[q]]
        d = dist[q].numpy()[row]
        at = set(range(k + 2))
        for c in groups[q]:
            r = int(np.where(row == c)[0][0])
            at |= {r - 1, r, r + 1}
        gaps = np.diff(d)
        margin = min(margin, min(gaps[i] for i in at if 0 <= i < len(gaps)), min(gaps[i - 1] for i in at if 1 <= i <= len(gaps)))
    return dict(pooled=pooled, pred=pred, refs=refs, groups=groups, targets=targets, dist=dist, margin=float(margin),
                names=["im%05d" % i for i in range(n_index)])


def test_index_above_8192():
    """cirr_metrics_from_predictions over 9000 index rows, topk=100: metrics and top-K names of a stable-argsort restatement of
    validate.py:202-247.  torch.argsort(stable=True) and the kernels break ties alike, but the two matmuls may differ in the last bit:
    the 256-term dot products agree to ~1e-8 and `1 - x` rounds to an ulp of 1.2e-7 (6e-8 below 1) either way.  Seed 28 leaves no two
    neighbouring distances closer than 1.4e-6 (12 ulp) where the result reads them - the first k + 2 columns and both sides of every
    `cols` rank; seeds 0-27 were tried on the CPU first and leave 0 to 1.2e-6.  The margin is asserted again before the device runs."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from candidate_reranking_cir_amd import validate as V1
    c = big_case(BIG_SEED)
    assert c["margin"] > 1e-6, c["margin"]
    names = c["names"]
    g6 = C.group6(c["refs"], c["groups"])
    want_metrics, want_sorted, want_labels, want_glabels = C.restate_cirr_val(
        c["dist"], names, [names[i] for i in c["refs"]], [names[i] for i in c["targets"]], [[names[j] for j in row] for row in g6])
    metrics, top = V1.cirr_metrics_from_predictions(c["pred"].cuda(), c["pooled"].cuda(), c["refs"], c["targets"], g6, names, "train", topk=100)
    assert metrics == want_metrics
    assert (top["sorted_index_names"] == want_sorted[:, :100]).all() and torch.equal(top["labels"], want_labels[:, :100])
    assert torch.equal(top["group_labels"], want_glabels) and len(top["index_names"]) == 9000 and top["split"] == "train"
    with pytest.raises(ValueError, match="2048"):
        V1.cirr_metrics_from_predictions(c["pred"].cuda(), c["pooled"].cuda(), c["refs"], c["targets"], g6, names, "train", topk=2049)
