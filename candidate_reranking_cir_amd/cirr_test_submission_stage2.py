"""CIRR test-split submission through stage II - counterpart of the reference's
src/cirr_test_submission_stage2.py.

No labels on the test split: every query is scored (no skip rule, :111-178); the server files are
`{"version": "rc2", "metric": "recall", pair_id: [50 names]}` and
`{"version": "rc2", "metric": "recall_subset", pair_id: [3 names]}` (:50-71, :92-108), written with sort_keys.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .validate_stage2 import RelativeValSet, _bank16, generate_val_predictions, relative_test_set_from_dataset


def generate_cirr_test_dicts(*args, **kw) -> Tuple[Dict[str, List[str]], Dict[str, List[str]]]:
    """Top-50 global and top-3 subset predictions per pair id (cirr_test_submission_stage2.py:74-108).  Two call forms.  Native:
    (blip_model, model_stage1, RelativeValSet, index_features, index_names, pair_ids, query_batch=8, kv_bank=None) - `ds.labels` is
    ignored: all queries are scored; `ds.group_index` holds the 5 non-reference members.  The reference's own (:74-78):
    (relative_test_dataset, blip_model, model_stage1, index_features, index_names, query_batch=..., kv_bank=...) over 5-field test items
    (data_utils.py:346) and the fp32 `index_features` of utils.py:43-55; it runs the native form underneath."""
    third = args[2] if len(args) > 2 else kw.get("ds")
    if isinstance(third, RelativeValSet):
        return _cirr_test_dicts(*args, **kw)
    names = ("relative_test_dataset", "blip_model", "model_stage1", "index_features", "index_names")
    if len(args) > len(names):
        raise TypeError("reference form: (relative_test_dataset, blip_model, model_stage1, index_features, index_names)")
    relative_test_dataset, blip_model, model_stage1, index_features, index_names = list(args) + [kw.pop(n) for n in names[len(args):]]
    ds, _, _, pair_ids = relative_test_set_from_dataset(relative_test_dataset, index_names)
    return _cirr_test_dicts(blip_model, model_stage1, ds, _bank16(blip_model, index_features), list(index_names), pair_ids, **kw)


def generate_cirr_test_predictions(blip_model, model_stage1, relative_test_dataset, index_names: Sequence[str], index_features: torch.Tensor, **kw):
    """cirr_test_submission_stage2.py:111-178 in the reference's call form, over 5-field test items (data_utils.py:346):
    (predicted_logits (Q, K), group_predicted_logits (Q, 5), reference_names, group_members_noRef, pairs_id) - the batched loop
    underneath (`query_batch=`, `kv_bank=`), every query scored."""
    if isinstance(index_names, torch.Tensor) or not isinstance(index_features, torch.Tensor):
        raise TypeError("reference form takes index_names (list of str) BEFORE index_features (tensor), cirr_test_submission_stage2.py:111-113")
    ds, refs, members, pair_ids = relative_test_set_from_dataset(relative_test_dataset, index_names)
    logits, glogits = generate_val_predictions(blip_model, model_stage1, ds, _bank16(blip_model, index_features), **kw)
    return logits, glogits, refs, members, pair_ids


@torch.no_grad()
def _cirr_test_dicts(blip_model, model_stage1, ds: RelativeValSet, index_features: torch.Tensor, index_names: Sequence[str],
                     pair_ids: Sequence[int], query_batch: int = 8, kv_bank=None, *, refine_margin=None, referee_index_features=None,
                     referee=None, on_violation: str = "warn", refine_stats=None) -> Tuple[Dict[str, List[str]], Dict[str, List[str]]]:
    """The native form of `generate_cirr_test_dicts`.  `refine_margin` (opt-in, with `referee_index_features` etc. as in
    `generate_val_predictions`): rank refinement with first=50 - the 50 names written per pair are the first 50 places, so only clusters that
    reach into them are scored again; the 3 subset names come from the subset matrix, refined by the full rule."""
    all_true = RelativeValSet(ref_index=ds.ref_index, cand_index=ds.cand_index, labels=np.ones_like(ds.cand_index, dtype=bool),
                              captions=ds.captions, input_ids=ds.input_ids, attention_mask=ds.attention_mask,
                              group_index=ds.group_index, target_index=ds.target_index)
    refine = {} if refine_margin is None else dict(refine_margin=refine_margin, referee_index_features=referee_index_features, referee=referee,
                                                   on_violation=on_violation, refine_stats=refine_stats, refine_first=50)
    logits, glogits = generate_val_predictions(blip_model, model_stage1, all_true, index_features, query_batch=query_batch, kv_bank=kv_bank, **refine)
    names = np.asarray(index_names)
    order = ops.argsort_desc(logits).cpu().numpy()
    sorted_names = np.take_along_axis(names[ds.cand_index], order, axis=1)
    gorder = ops.argsort_desc(glogits).cpu().numpy()
    sorted_group = np.take_along_axis(names[ds.group_index], gorder, axis=1)
    rec = {str(int(p)): row[:50].tolist() for p, row in zip(pair_ids, sorted_names)}
    sub = {str(int(p)): row[:3].tolist() for p, row in zip(pair_ids, sorted_group)}
    return rec, sub


def write_submissions(folder: str, file_name: str, pairid_to_predictions: dict, pairid_to_group_predictions: dict) -> Tuple[str, str]:
    """cirr_test_submission_stage2.py:50-71."""
    submission = {"version": "rc2", "metric": "recall"}
    group_submission = {"version": "rc2", "metric": "recall_subset"}
    submission.update(pairid_to_predictions)
    group_submission.update(pairid_to_group_predictions)
    os.makedirs(folder, exist_ok=True)
    p1 = os.path.join(folder, f"recall_submission_{file_name}.json")
    p2 = os.path.join(folder, f"recall_subset_submission_{file_name}.json")
    with open(p1, "w+") as fh:
        json.dump(submission, fh, sort_keys=True)
    with open(p2, "w+") as fh:
        json.dump(group_submission, fh, sort_keys=True)
    return p1, p2
