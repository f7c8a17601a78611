"""CIRR test-split submission through stage I - counterpart of the reference's src/cirr_test_submission.py
(SURVEY.md section 8(f) row 3): rank the test1 index by the fused query feature, delete the reference image, keep the
top-50 and the subset top-3 per pair id - and write the test-split top-K file that stage II's submission reads.

Reference arithmetic (cirr_test_submission.py:96-115): `distances = 1 - predicted @ index.T` -> `argsort` ascending -> names,
the reference image masked out of each row, the subset = the row's entries that are group members.  Here the ranking is one
`validate.rank_index_topk` call: the first max(50, K) columns of every row and the positions of the 5 subset members; no row is
sorted and no (Q, n_index) array of names exists.  File schema (:121-127; read at data_utils.py:290-305 and by
`validate.load_topk`): `sorted_index_names (Q, K) str`, `index_names`, `split` - no labels on the test split.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import validate as V1
from .cirr_test_submission_stage2 import write_submissions  # noqa: F401  (the two server files: the same writer for both stages)


def generate_cirr_test_predictions(blip_model, relative_test_dataset, index_names: Sequence[str], index_features: torch.Tensor):
    """cirr_test_submission.py:135-181 in the reference's call form, over items (pair_id, reference, caption, 6 members)
    (data_utils.py:350): (predicted (Q, 256) fp32 on the device, reference_names, group_members, pairs_id)."""
    q = V1.relative_queries_from_dataset(relative_test_dataset, index_names, "cirr_test")
    return V1._query_features(blip_model, q, index_features), q.reference_names, q.group_members, q.pair_ids


@torch.no_grad()
def cirr_test_dicts_from_predictions(predicted, index_pooled, ref_index, group_index, index_names: Sequence[str], pair_ids,
                                     topk: Optional[int] = None, split: str = "test1", ranked=None):
    """cirr_test_submission.py:93-127 from the query features on: (pairid_to_predictions, pairid_to_group_predictions) - the first
    min(50, n_index - 1) names of every ranking without its reference image, and the first 3 subset members by rank; with `topk=K`
    also the test-split top-K dict {sorted_index_names (Q, K), index_names, split}.  One `rank_index_topk` call: `exclude` = the
    reference, `cols` = the 5 members besides it, k = max(50, K) capped at n_index - 1.  `group_index`: (Q, 6) incl. the reference or
    (Q, 5) without it; `ranked`: the (topk, ranks) pair of that call where the caller already holds it."""
    index_names = list(index_names)
    ref_index = np.asarray(ref_index, dtype=np.int64)
    members = V1.group_index6(ref_index, group_index)
    members = members[members != ref_index[:, None]].reshape(len(ref_index), 5)
    limit = min(2048, len(index_names) - 1)
    if topk is not None and not 1 <= int(topk) <= limit:
        raise ValueError(f"topk = {topk}: the top-K path holds 1 <= K <= min(2048, n_index - 1) = {limit}")
    k = min(max(50, topk or 0), len(index_names) - 1)
    if ranked is None:
        ranked = V1.rank_index_topk(predicted, index_pooled.to(predicted.device).float(), k, exclude=ref_index, cols=members)
    top_rows, ranks = V1._host(ranked)
    assert top_rows.shape == (len(ref_index), k) and ranks.shape == members.shape and (ranks >= 0).all()
    names = np.array(index_names)
    sorted_names = names[top_rows]                                                              # (Q, k): the only name matrix
    by_rank = np.take_along_axis(members, np.argsort(ranks, axis=1, kind="stable"), axis=1)     # :107-109
    rec = {str(int(p)): row[:50].tolist() for p, row in zip(pair_ids, sorted_names)}            # :112-113
    sub = {str(int(p)): row[:3].tolist() for p, row in zip(pair_ids, names[by_rank])}           # :114-115
    if topk is None:
        return rec, sub
    return rec, sub, dict(sorted_index_names=sorted_names[:, :int(topk)], index_names=index_names, split=split)


def generate_cirr_test_dicts(relative_test_dataset, blip_model, index_features, index_features_normed_pooled, index_names: Sequence[str],
                             topk: Optional[int] = None, save_path: Optional[str] = None):
    """cirr_test_submission.py:73-132 in the reference's call form: (pairid_to_predictions, pairid_to_group_predictions).  `topk=K`
    also returns the test-split top-K dict and `save_path=` writes it - the reference's SAVE_TOPK / K_VALUE / STAGE1_PATH globals and
    breakpoint() (:117-128); `split` is the dataset's attribute (:126)."""
    V1._check_save(topk, save_path)
    q = V1.relative_queries_from_dataset(relative_test_dataset, index_names, "cirr_test")
    predicted = V1._query_features(blip_model, q, index_features)
    out = cirr_test_dicts_from_predictions(predicted, index_features_normed_pooled, q.ref_index, q.group_index, index_names, q.pair_ids,
                                           topk=topk, split=relative_test_dataset.split)
    return V1._finish(out, topk, save_path)
