"""Stage-I retrieval and the top-K file - the build's counterpart of the reference's src/validate.py
(SURVEY.md section 8(f) row 2): rank the whole index by cosine distance to the fused query feature, compute
Recall@k, and write / read the top-K file that stage II consumes.

Reference arithmetic (validate.py:57-64, 202-226): `distances = 1 - predicted @ index.T` ->
`argsort` ascending -> names; CIRR removes the reference image from each row, derives subset labels from
the 6-member groups, asserts exactly one positive per row.  File schema (validate.py:86-93, 255-262;
read back at data_utils.py:166-179, 290-305): `sorted_index_names (Q,K) str`, `target_names`, `index_names`,
`labels (Q,K) bool`, `split`, plus `dress_types` (FashionIQ) or `group_labels (Q,5)` (CIRR).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .blip_stage2 import encode_text
from .validate_stage2 import RelativeValSet, _bank16, fiq_caption


@torch.no_grad()
def extract_index_features(images: torch.Tensor, model_stage1, batch_size: int = 64):
    """utils.py:57-72 (blip_stage1 branch): ViT tokens of every index image and their normalised 256-d pooled
    features.  Returns (tokens (n, N, D) in the compute dtype, pooled (n, 256) fp32)."""
    toks, pooled = [], []
    for i in range(0, images.shape[0], batch_size):
        t32, p = model_stage1.img_embed(images[i:i + batch_size].to(model_stage1.device), return_pool_and_normalized=True)
        toks.append(ops.gather_rows(t32, None, model_stage1.token_dtype))
        pooled.append(p)
    return torch.cat(toks), torch.cat(pooled)


@torch.no_grad()
def extract_index_features_raw(images: Sequence, model_stage1, transform, batch_size: int = 64):
    """`extract_index_features` from decoded uint8 RGB images of any sizes and a `preprocess.DeviceTransform` (data_utils.py:71-101 on the
    device, patch operand rows out: no fp32 image tensor exists).  Same results, bit for bit, as on `transform.batch(images)`."""
    toks, pooled = [], []
    for i in range(0, len(images), batch_size):
        t32, p = model_stage1.img_embed_raw(images[i:i + batch_size], transform, return_pool_and_normalized=True)
        toks.append(ops.gather_rows(t32, None, model_stage1.token_dtype))
        pooled.append(p)
    return torch.cat(toks), torch.cat(pooled)


@torch.no_grad()
def generate_val_predictions(model_stage1, ref_index: np.ndarray, captions: Sequence[str], index_tokens: torch.Tensor,
                             batch_size: int = 32) -> torch.Tensor:
    """validate.py:100-147 / 281-330: fused, normalised query features (Q, 256); captions are padded per batch of 32
    (`padding='longest'`), like the reference's DataLoader batches."""
    dev = model_stage1.device
    out = []
    for s in range(0, len(captions), batch_size):
        rows = list(range(s, min(s + batch_size, len(captions))))
        ids, mask = encode_text(model_stage1.tokenizer, [captions[i] for i in rows], dev)
        ref = ops.gather_rows(index_tokens, torch.as_tensor(ref_index[rows], device=dev))
        heads = model_stage1.engines()[2]
        z = model_stage1.z_t(ref, ids, mask)
        out.append(ops.l2_normalize(ops.linear_f32(z.last_hidden_state[:, 0, :], heads["tw"], heads["tb"])))
    return torch.cat(out)


@torch.no_grad()
def rank_index(predicted: torch.Tensor, index_pooled: torch.Tensor) -> torch.Tensor:
    """(Q, n_index) int64: index rows by ascending `1 - predicted @ index.T` (validate.py:57-58, 202-203)."""
    neg_dist = ops.linear_f32(predicted, index_pooled.contiguous(), None, mode=2)   # -(1 - q.i), exact negation
    return ops.argsort_desc(neg_dist)                                    # ascending distance; ties -> lower index


@torch.no_grad()
def rank_index_topk(predicted: torch.Tensor, index_pooled: torch.Tensor, k: int, exclude=None, cols=None, row_block: Optional[int] = None):
    """What stage II reads of `rank_index`'s ranking, for an index of any size: (topk (Q, k) int64, ranks (Q, m) int64 or None).
    `topk` holds the first k columns of each row of `rank_index(predicted, index_pooled)` - with column `exclude[q]` removed from row q
    first, where given (CIRR drops the reference image, validate.py:207-210) -, `ranks[q, t]` the position of index row `cols[q, t]` in that
    ranking (m <= 8; -1 for the excluded row).  The distance matrix comes from the same `ops.linear_f32` call as `rank_index`'s, `row_block`
    query rows at a time (default: tiles of at most 1 GiB), so its bits and therefore the order are `rank_index`'s wherever both run; no row is
    sorted (ops.topk_desc, ops.rank_of), and `n_index` has no ceiling."""
    index = index_pooled.contiguous()
    q_n, n_idx = predicted.shape[0], index.shape[0]
    dev = predicted.device
    if row_block is None:
        row_block = max(1, min((1 << 30) // (4 * n_idx), 65535 * 64))
    exclude = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64, device=dev)
    cols = None if cols is None else torch.as_tensor(cols, dtype=torch.int64, device=dev).reshape(q_n, -1)
    topk = torch.empty((q_n, k), dtype=torch.int64, device=dev)
    ranks = None if cols is None else torch.empty_like(cols)
    for s in range(0, q_n, row_block):
        rows = slice(s, min(s + row_block, q_n))
        neg_dist = ops.linear_f32(predicted[rows], index, None, mode=2)     # rank_index's matrix, a tile of it
        ex = None if exclude is None else exclude[rows]
        topk[rows] = ops.topk_desc(neg_dist, k, ex)
        if cols is not None:
            ranks[rows] = ops.rank_of(neg_dist, cols[rows], ex)
    return topk, ranks


def recall_at(labels: np.ndarray, k: int) -> float:
    lab = torch.tensor(labels)
    return (torch.sum(lab[:, :k]) / len(lab)).item() * 100


def fiq_topk(sorted_rows: np.ndarray, target_index: np.ndarray, index_names: List[str], k: int, split: str, dress_type: str):
    """FashionIQ: labels, (R@10, R@50) and the top-K dict of validate.py:60-95."""
    labels = sorted_rows == target_index[:, None]
    assert (labels.sum(1) == 1).all()                                      # validate.py:64
    names = np.array(index_names)
    top = dict(sorted_index_names=names[sorted_rows[:, :k]], target_names=[index_names[i] for i in target_index],
               index_names=list(index_names), labels=torch.tensor(labels[:, :k]), split=split, dress_types=dress_type)
    return (recall_at(labels, 10), recall_at(labels, 50)), top


def cirr_topk(sorted_rows: np.ndarray, ref_index: np.ndarray, target_index: np.ndarray, group_index: np.ndarray,
              index_names: List[str], k: int, split: str):
    """CIRR: drop the reference image from each ranking, labels, subset labels, the 7 metrics and the top-K dict
    (validate.py:205-264).  `group_index` (Q, 6) holds the full groups incl. the reference, as in the dataset."""
    q_n, n_idx = sorted_rows.shape
    keep = sorted_rows != ref_index[:, None]                               # validate.py:207-210
    rows = sorted_rows[keep].reshape(q_n, n_idx - 1)
    labels = rows == target_index[:, None]
    group_mask = (rows[..., None] == group_index[:, None, :]).sum(-1).astype(bool)   # validate.py:219
    group_labels = labels[group_mask].reshape(q_n, -1)
    assert (labels.sum(1) == 1).all() and (group_labels.sum(1) == 1).all()           # validate.py:225-226
    names = np.array(index_names)
    top = dict(sorted_index_names=names[rows[:, :k]], target_names=[index_names[i] for i in target_index],
               index_names=list(index_names), labels=torch.tensor(labels[:, :k]), group_labels=torch.tensor(group_labels), split=split)
    metrics = (recall_at(group_labels, 1), recall_at(group_labels, 2), recall_at(group_labels, 3),
               recall_at(labels, 1), recall_at(labels, 5), recall_at(labels, 10), recall_at(labels, 50))
    return metrics, top


def _recall_of_ranks(rank: np.ndarray, k: int) -> float:
    """recall_at(labels, k) of the full label matrix whose one positive of row q sits at column rank[q]."""
    return recall_at((rank < k)[:, None], 1)


def fiq_topk_from_ranks(topk: np.ndarray, target_rank: np.ndarray, target_index: np.ndarray, index_names: List[str], k: int, split: str,
                        dress_type: str):
    """`fiq_topk` from `rank_index_topk(pred, pooled, k, cols=target_index[:, None])` instead of a full ranking: the same metrics tuple and
    the same top-K dict.  The reference's "one positive per row" (validate.py:64) is the target's rank lying inside the row."""
    topk, target_index = np.asarray(topk), np.asarray(target_index)
    rank = np.asarray(target_rank).reshape(len(topk))
    assert topk.shape[1] >= k and ((rank >= 0) & (rank < len(index_names))).all()       # validate.py:64
    labels = np.arange(k)[None, :] == rank[:, None]
    assert (topk[:, :k][labels] == target_index[labels.any(1)]).all()                   # the column at the target's rank is the target
    names = np.array(index_names)
    top = dict(sorted_index_names=names[topk[:, :k]], target_names=[index_names[i] for i in target_index],
               index_names=list(index_names), labels=torch.tensor(labels), split=split, dress_types=dress_type)
    return (_recall_of_ranks(rank, 10), _recall_of_ranks(rank, 50)), top


def cirr_rank_cols(ref_index: np.ndarray, target_index: np.ndarray, group_index: np.ndarray) -> np.ndarray:
    """(Q, 6) index rows whose ranks `cirr_topk_from_ranks` reads: [target | the 5 group members besides the reference]; pass it as `cols`
    and `ref_index` as `exclude` to `rank_index_topk`.  `group_index` (Q, 6) holds the full groups incl. the reference, as in the dataset."""
    ref_index, group_index = np.asarray(ref_index), np.asarray(group_index)
    keep = group_index != ref_index[:, None]
    assert (keep.sum(1) == group_index.shape[1] - 1).all()                              # the reference is one member of its group
    return np.concatenate([np.asarray(target_index)[:, None], group_index[keep].reshape(len(group_index), -1)], axis=1).astype(np.int64)


def cirr_topk_from_ranks(topk: np.ndarray, ranks: np.ndarray, ref_index: np.ndarray, target_index: np.ndarray, group_index: np.ndarray,
                         index_names: List[str], k: int, split: str):
    """`cirr_topk` from `rank_index_topk(pred, pooled, k, exclude=ref_index, cols=cirr_rank_cols(...))` instead of a full ranking: the same 7
    metrics and the same top-K dict, `group_labels (Q, 5)` included (group_labels[q, j]: the j-th group member by rank is the target).  The
    reference's asserts (validate.py:225-226) become: the target's rank lies inside the row, and the target is one of its group's members."""
    topk, ranks, target_index = np.asarray(topk), np.asarray(ranks), np.asarray(target_index)
    members = cirr_rank_cols(ref_index, target_index, group_index)[:, 1:]
    rank, group_rank = ranks[:, 0], ranks[:, 1:]
    assert topk.shape[1] >= k and ranks.shape == (len(topk), 1 + members.shape[1])
    assert ((rank >= 0) & (rank < len(index_names) - 1)).all() and (group_rank >= 0).all()
    labels = np.arange(k)[None, :] == rank[:, None]
    assert (topk[:, :k][labels] == target_index[labels.any(1)]).all()
    by_rank = np.take_along_axis(members, np.argsort(group_rank, axis=1, kind="stable"), axis=1)
    group_labels = by_rank == target_index[:, None]
    assert (group_labels.sum(1) == 1).all()                                             # validate.py:225-226
    names = np.array(index_names)
    top = dict(sorted_index_names=names[topk[:, :k]], target_names=[index_names[i] for i in target_index],
               index_names=list(index_names), labels=torch.tensor(labels), group_labels=torch.tensor(group_labels), split=split)
    metrics = (recall_at(group_labels, 1), recall_at(group_labels, 2), recall_at(group_labels, 3),
               _recall_of_ranks(rank, 1), _recall_of_ranks(rank, 5), _recall_of_ranks(rank, 10), _recall_of_ranks(rank, 50))
    return metrics, top


def save_topk(path: str, top: dict) -> None:
    torch.save(top, path)


def load_topk(path: str, k: int, ref_index: np.ndarray, captions: Optional[List[str]] = None,
              group_index: Optional[np.ndarray] = None, target_index: Optional[np.ndarray] = None, split: Optional[str] = None) -> RelativeValSet:
    """Read a top-K file (ours or the authors') into the tensor form stage II consumes: names -> rows of `index_names`
    (data_utils.py:166-179, 290-305 keep the first K columns the same way).  A file without `labels` / `target_names` - the test1 schema,
    cirr_test_submission.py:121-127, which data_utils.py:299 reads without them - gives all-true labels (every query is scored) and no
    `target_index` unless the caller passes one.  `split`, where given, must be the file's (data_utils.py:171, 294)."""
    f = torch.load(path, weights_only=False)
    assert k <= f["sorted_index_names"].shape[-1]                           # data_utils.py:169, 293
    if split is not None and f["split"] != split:
        raise ValueError(f"{path} holds the top-K of split {f['split']!r}, not {split!r}")
    row_of = {n: i for i, n in enumerate(f["index_names"])}
    names = np.asarray(f["sorted_index_names"])[:, :k]
    cand = np.vectorize(row_of.__getitem__, otypes=[np.int64])(names)
    if "labels" in f:
        labels = np.asarray(f["labels"])[:, :k].astype(bool)
    else:
        labels = np.ones(cand.shape, dtype=bool)
    if target_index is None and "target_names" in f:
        target_index = np.array([row_of[n] for n in f["target_names"]], dtype=np.int64)
    return RelativeValSet(ref_index=np.asarray(ref_index), cand_index=cand, labels=labels, captions=captions,
                          group_index=group_index, target_index=target_index)


# ------------------------------------------------------------------------------------------------ reference signatures
@dataclass
class RelativeQueries:
    """A stage-I 'relative' split (no top-K file) in tensor form: every name an integer row of `index_names`, next to the lists of
    names the reference's generate_* functions return."""
    ref_index: np.ndarray                      # (Q,)
    captions: List[str]                        # one per query (FashionIQ: already joined)
    reference_names: List[str]
    target_index: Optional[np.ndarray] = None  # (Q,)   val items
    target_names: Optional[List[str]] = None
    group_index: Optional[np.ndarray] = None   # (Q, 5) CIRR subset members without the reference
    group_members: Optional[List[List[str]]] = None   # the 6 members as the dataset holds them, reference included
    pair_ids: Optional[list] = None            # CIRR test items

    def __len__(self) -> int:
        return len(self.ref_index)


_LAYOUTS = {
    "fiq_val": (3, "(reference, target, [cap1, cap2]) (FashionIQ val, data_utils.py:212)"),
    "cirr_val": (4, "(reference, target_hard, caption, 6 group members incl. the reference) (CIRR val, data_utils.py:340)"),
    "cirr_test": (4, "(pair_id, reference, caption, 6 group members incl. the reference) (CIRR test1, data_utils.py:350)"),
}


def name_rows(index_names: Sequence[str]) -> dict:
    """name -> row of `index_names`; duplicates raise ValueError (the reference's dict(zip(index_names, index_features)),
    validate.py:121, would silently keep the last)."""
    row = {str(n): i for i, n in enumerate(index_names)}
    if len(row) != len(index_names):
        raise ValueError("index_names holds duplicates")
    return row


def group_rows(row: dict, reference: str, members) -> List[int]:
    """Rows of the 5 subset members besides the reference, in the dataset's order (validate.py:219-220 masks them out of rankings
    that no longer hold the reference; cirr_test_submission_stage2.py:166, 173 drop it the same way)."""
    rest = [row[str(m)] for m in members if str(m) != str(reference)]
    if len(members) != 6 or len(rest) != 5:
        raise ValueError(f"a CIRR subset has 6 members, the reference among them: got {len(members)} members, {len(rest)} besides {reference!r}")
    return rest


def relative_queries_from_dataset(relative_dataset, index_names: Sequence[str], layout: str) -> RelativeQueries:
    """The reference's stage-I 'relative' dataset (anything with `__len__` and items in one of `_LAYOUTS`) -> RelativeQueries.  Names
    become rows of `index_names` ONCE here (the reference looks each up in a dict per batch, validate.py:142, 307): a name that is
    not in the index raises KeyError as there, any other field count TypeError."""
    fields, text = _LAYOUTS[layout]
    row = name_rows(index_names)
    n_q = len(relative_dataset)
    q = RelativeQueries(ref_index=np.empty(n_q, dtype=np.int64), captions=[], reference_names=[])
    if layout != "cirr_test":
        q.target_index, q.target_names = np.empty(n_q, dtype=np.int64), []
    else:
        q.pair_ids = []
    if layout != "fiq_val":
        q.group_index, q.group_members = np.empty((n_q, 5), dtype=np.int64), []
    for i in range(n_q):
        item = relative_dataset[i]
        if not isinstance(item, (tuple, list)) or len(item) != fields:
            raise TypeError(f"a stage-I item is {text}; got {len(item) if isinstance(item, (tuple, list)) else type(item).__name__} fields "
                            "(a dataset built with load_topk= / K= belongs to stage II)")
        if layout == "fiq_val":
            ref, tgt, cap = item
            q.captions.append(fiq_caption(str(cap[0]), str(cap[1])))                        # validate.py:130-133
        elif layout == "cirr_val":
            ref, tgt, cap, members = item
        else:
            pair_id, ref, cap, members = item
            q.pair_ids.append(pair_id)
        ref = str(ref)
        q.ref_index[i] = row[ref]
        q.reference_names.append(ref)
        if layout != "cirr_test":
            q.target_index[i] = row[str(tgt)]
            q.target_names.append(str(tgt))
        if layout != "fiq_val":
            q.captions.append(str(cap))
            q.group_index[i] = group_rows(row, ref, members)
            q.group_members.append([str(m) for m in members])
    return q


def _query_features(blip_model, q: RelativeQueries, index_features: torch.Tensor) -> torch.Tensor:
    return generate_val_predictions(blip_model, q.ref_index, q.captions, _bank16(blip_model, index_features))


def generate_fiq_val_predictions(blip_model, relative_val_dataset, index_names: Sequence[str], index_features: torch.Tensor):
    """validate.py:102-149 in the reference's call form: (predicted (Q, 256) fp32 on the device, target_names).  `index_features` is
    what utils.py:57-72 hands over - fp32 (n, N, D) tokens - or the 16-bit bank (one conversion launch otherwise); the features are the
    native `generate_val_predictions` on the same rows and captions, in batches of 32 padded to the longest caption (:116)."""
    q = relative_queries_from_dataset(relative_val_dataset, index_names, "fiq_val")
    return _query_features(blip_model, q, index_features), q.target_names


def generate_cirr_val_predictions(blip_model, relative_val_dataset, index_names: Sequence[str], index_features: torch.Tensor):
    """validate.py:271-316 in the reference's call form: (predicted, reference_names, target_names, group_members) - the 6 members
    of every subset as the dataset holds them, the reference among them (:298, :313)."""
    q = relative_queries_from_dataset(relative_val_dataset, index_names, "cirr_val")
    return _query_features(blip_model, q, index_features), q.reference_names, q.target_names, q.group_members


def _check_topk(topk: Optional[int], n_index: int) -> int:
    """The k to ask `rank_index_topk` for: its smallest (1) when only metrics are wanted."""
    limit = min(2048, n_index - 1)
    if topk is None:
        return 1
    if not 1 <= int(topk) <= limit:
        raise ValueError(f"topk = {topk}: the top-K path holds 1 <= K <= min(2048, n_index - 1) = {limit}")
    return int(topk)


def _host(ranked):
    return tuple(None if a is None else (a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)) for a in ranked)


def group_index6(ref_index: np.ndarray, group_index: np.ndarray) -> np.ndarray:
    """(Q, 6) groups incl. the reference, the layout `cirr_rank_cols` / `cirr_topk_from_ranks` read, from either that layout (the
    dataset's) or the (Q, 5) members without the reference (RelativeValSet.group_index, RelativeQueries.group_index)."""
    ref_index, group_index = np.asarray(ref_index), np.asarray(group_index)
    if group_index.shape[1] == 6:
        return group_index
    if group_index.shape[1] != 5 or (group_index == ref_index[:, None]).any():
        raise ValueError("group_index is (Q, 6) with the reference or (Q, 5) without it")
    return np.concatenate([ref_index[:, None], group_index], axis=1)


@torch.no_grad()
def fiq_metrics_from_predictions(predicted, index_pooled, target_index, index_names: Sequence[str], split: str, dress_types,
                                 topk: Optional[int] = None, ranked=None):
    """validate.py:53-99 from the query features on: (R@10, R@50); with `topk=K` ((R@10, R@50), the top-K dict of :87-94).  One
    `rank_index_topk` call with `cols` = the target (no row is sorted, `n_index` has no ceiling); recalls are formed from the target's
    rank in the reference's float32 arithmetic.  `dress_types`: the dataset's list (joined with ',' as :85 does) or that string.
    `ranked`: the (topk, ranks) pair of that call where the caller already holds it - `predicted` / `index_pooled` are not read then."""
    index_names = list(index_names)
    target_index = np.asarray(target_index, dtype=np.int64)
    k = _check_topk(topk, len(index_names))
    if ranked is None:
        ranked = rank_index_topk(predicted, index_pooled.to(predicted.device).float(), k, cols=target_index[:, None])
    top_rows, rank = _host(ranked)
    dress = dress_types if isinstance(dress_types, str) else ",".join(dress_types)
    metrics, top = fiq_topk_from_ranks(top_rows, rank, target_index, index_names, k, split, dress)
    return metrics if topk is None else (metrics, top)


@torch.no_grad()
def cirr_metrics_from_predictions(predicted, index_pooled, ref_index, target_index, group_index, index_names: Sequence[str], split: str,
                                  topk: Optional[int] = None, ranked=None):
    """validate.py:196-268 from the query features on: (Rs@1, Rs@2, Rs@3, R@1, R@5, R@10, R@50), the reference's order (:268); with
    `topk=K` (that tuple, the top-K dict of :256-263).  One `rank_index_topk` call with `exclude` = the reference image (:207-210) and
    `cols` = `cirr_rank_cols(...)`.  `group_index`: (Q, 6) incl. the reference or (Q, 5) without it; `ranked` as above."""
    index_names = list(index_names)
    ref_index, target_index = np.asarray(ref_index, dtype=np.int64), np.asarray(target_index, dtype=np.int64)
    group6 = group_index6(ref_index, group_index)
    k = _check_topk(topk, len(index_names))
    if ranked is None:
        ranked = rank_index_topk(predicted, index_pooled.to(predicted.device).float(), k, exclude=ref_index,
                                 cols=cirr_rank_cols(ref_index, target_index, group6))
    top_rows, ranks = _host(ranked)
    metrics, top = cirr_topk_from_ranks(top_rows, ranks, ref_index, target_index, group6, index_names, k, split)
    return metrics if topk is None else (metrics, top)


def _check_save(topk, save_path) -> None:
    if save_path is not None and topk is None:
        raise ValueError("save_path needs topk=K: the number of columns the file keeps")


def _finish(result, topk, save_path):
    """`result` as the caller returns it; its last entry, the top-K dict, written to `save_path` where given."""
    _check_save(topk, save_path)
    if save_path is not None:
        save_topk(save_path, result[-1])
    return result


def compute_fiq_val_metrics(relative_val_dataset, blip_model, index_features, index_features_normed_pooled, index_names: Sequence[str],
                            topk: Optional[int] = None, save_path: Optional[str] = None):
    """validate.py:33-99 in the reference's call form (stage1_train.py:244): (R@10, R@50).  `topk=K` also returns the top-K dict and
    `save_path=` writes it - what the reference does through the SAVE_TOPK / K_VALUE / STAGE1_PATH globals and a breakpoint() (:80-95);
    `split` and `dress_types` are the dataset's attributes, as there (:85-92)."""
    _check_save(topk, save_path)
    q = relative_queries_from_dataset(relative_val_dataset, index_names, "fiq_val")
    predicted = _query_features(blip_model, q, index_features)
    out = fiq_metrics_from_predictions(predicted, index_features_normed_pooled, q.target_index, index_names, relative_val_dataset.split,
                                       relative_val_dataset.dress_types, topk=topk)
    return _finish(out, topk, save_path)


def compute_cirr_val_metrics(relative_val_dataset, blip_model, index_features, index_features_normed_pooled, index_names: Sequence[str],
                             topk: Optional[int] = None, save_path: Optional[str] = None):
    """validate.py:176-268 in the reference's call form (stage1_train.py:459; `cirr_val_retrieval(train=True)`, :329-332, over the
    ~17 k images of the train split likewise): the 7 metrics; `topk=K` / `save_path=` as `compute_fiq_val_metrics` (:249-264)."""
    _check_save(topk, save_path)
    q = relative_queries_from_dataset(relative_val_dataset, index_names, "cirr_val")
    predicted = _query_features(blip_model, q, index_features)
    out = cirr_metrics_from_predictions(predicted, index_features_normed_pooled, q.ref_index, q.target_index, q.group_index, index_names,
                                        relative_val_dataset.split, topk=topk)
    return _finish(out, topk, save_path)
