"""Shared by tests/test_stage1_forms_cpu.py and tests/test_stage1_forms_gpu.py: the reference's stage-I dataset duck types built from
tests/golden/stage1_tiny.npz, and restatements of the reference's ranking code (validate.py:57-64, 202-247; cirr_test_submission.py:96-115)
written with masks over name arrays, as the reference writes them."""
import numpy as np
import torch

from tests import helpers as H


def golden():
    z = H.load("stage1_tiny.npz")
    names = [str(n) for n in z["index_names"]]
    return z, names


class DuckFIQ1:
    """FashionIQ 'relative' val, stage I (data_utils.py:212): (reference, target, [cap1, cap2]); `split`, `dress_types`."""

    def __init__(self, names, refs, targets, captions):
        self.names, self.refs, self.targets, self.captions = list(names), refs, targets, captions
        self.split, self.dress_types = "val", ["dress"]

    def __len__(self):
        return len(self.refs)

    def __getitem__(self, i):
        return self.names[self.refs[i]], self.names[self.targets[i]], [str(c) for c in self.captions[i]]


class DuckCIRR1(DuckFIQ1):
    """CIRR 'relative' val, stage I (data_utils.py:340): (reference, target_hard, caption, 6 members INCLUDING the reference)."""

    def __init__(self, names, refs, targets, captions, groups, ref_slot=0):
        super().__init__(names, refs, targets, captions)
        self.groups, self.ref_slot = groups, ref_slot

    def members(self, i):
        m = [self.names[j] for j in self.groups[i]]
        m.insert(self.ref_slot % 6, self.names[self.refs[i]])
        return m

    def __getitem__(self, i):
        return self.names[self.refs[i]], self.names[self.targets[i]], str(self.captions[i]), self.members(i)


class DuckCIRRTest1(DuckCIRR1):
    """CIRR 'relative' test1, stage I (data_utils.py:350): (pair_id, reference, caption, 6 members)."""

    def __init__(self, names, refs, captions, groups, pair_ids, ref_slot=0):
        super().__init__(names, refs, None, captions, groups, ref_slot)
        self.pair_ids, self.split = pair_ids, "test1"

    def __getitem__(self, i):
        return int(self.pair_ids[i]), self.names[self.refs[i]], str(self.captions[i]), self.members(i)


class DuckCIRRTest2(DuckCIRRTest1):
    """CIRR 'relative' test1 with its top-K file, stage II (data_utils.py:346): the same + the K names of the query's row."""

    def __init__(self, names, refs, captions, groups, pair_ids, k_sorted_index_names, ref_slot=0):
        super().__init__(names, refs, captions, groups, pair_ids, ref_slot)
        self.K_sorted_index_names, self.K = np.asarray(k_sorted_index_names), np.asarray(k_sorted_index_names).shape[1]

    def __getitem__(self, i):
        return super().__getitem__(i) + (self.K_sorted_index_names[i].tolist(),)


def group6(refs, groups):
    return np.concatenate([np.asarray(refs)[:, None], np.asarray(groups)], axis=1)


def sorted_names_of(distances, index_names, reference_names=None):
    """validate.py:57-59 / 202-210, cirr_test_submission.py:97-105: names by ascending distance (stable: ties -> the lower index row, the
    order the kernels keep), the reference image masked out of its row where given."""
    sorted_indices = torch.argsort(torch.as_tensor(distances), dim=-1, stable=True)
    sorted_index_names = np.array(index_names)[sorted_indices.numpy()]
    if reference_names is not None:
        reference_mask = sorted_index_names != np.repeat(np.array(reference_names), len(index_names)).reshape(len(sorted_index_names), -1)
        sorted_index_names = sorted_index_names[reference_mask].reshape(sorted_index_names.shape[0], sorted_index_names.shape[1] - 1)
    return sorted_index_names


def restate_test_dicts(distances, index_names, reference_names, group_members, pair_ids):
    """cirr_test_submission.py:96-115 -> (pairid_to_predictions, pairid_to_group_predictions, sorted_index_names without the reference)."""
    sorted_index_names = sorted_names_of(distances, index_names, reference_names)
    group_members = np.array(group_members)
    group_mask = (sorted_index_names[..., None] == group_members[:, None, :]).sum(-1).astype(bool)
    sorted_group_names = sorted_index_names[group_mask].reshape(sorted_index_names.shape[0], -1)
    rec = {str(int(pair_id)): prediction[:50].tolist() for (pair_id, prediction) in zip(pair_ids, sorted_index_names)}
    sub = {str(int(pair_id)): prediction[:3].tolist() for (pair_id, prediction) in zip(pair_ids, sorted_group_names)}
    return rec, sub, sorted_index_names


def restate_cirr_val(distances, index_names, reference_names, target_names, group_members):
    """validate.py:202-247 -> (the 7 metrics in the order of :268, sorted_index_names, labels, group_labels)."""
    sorted_index_names = sorted_names_of(distances, index_names, reference_names)
    labels = torch.tensor(sorted_index_names == np.repeat(np.array(target_names), len(index_names) - 1).reshape(len(target_names), -1))
    group_members = np.array(group_members)
    group_mask = (sorted_index_names[..., None] == group_members[:, None, :]).sum(-1).astype(bool)
    group_labels = labels[group_mask].reshape(labels.shape[0], -1)
    assert torch.equal(torch.sum(labels, dim=-1).int(), torch.ones(len(target_names)).int())
    assert torch.equal(torch.sum(group_labels, dim=-1).int(), torch.ones(len(target_names)).int())

    def recall(lab, k):
        return (torch.sum(lab[:, :k]) / len(lab)).item() * 100
    metrics = (recall(group_labels, 1), recall(group_labels, 2), recall(group_labels, 3),
               recall(labels, 1), recall(labels, 5), recall(labels, 10), recall(labels, 50))
    return metrics, sorted_index_names, labels, group_labels


def ranked_on_cpu(distances, k, cols, exclude=None):
    """What `validate.rank_index_topk` returns, from a full stable argsort on the host: (topk (Q, k), ranks (Q, m))."""
    order = torch.argsort(torch.as_tensor(distances), dim=-1, stable=True).numpy()
    if exclude is not None:
        order = order[order != np.asarray(exclude)[:, None]].reshape(len(order), -1)
    cols = np.asarray(cols).reshape(len(order), -1)
    ranks = np.array([[int(np.where(order[q] == c)[0][0]) if (order[q] == c).any() else -1 for c in cols[q]] for q in range(len(order))])
    return order[:, :k].copy(), ranks
