"""The selective rank-refinement rule (include/cirrank.h, cir_rank_undecided_cuts) restated in numpy fp32, two ways, on top of
tests/refine_cases.py.

Links and clusters are refine_cases': neighbours of the sorted row are linked iff their fp32 difference is <= width = 2 * margin, a cluster is
a maximal run [a, b] of linked places.  New: an integer first >= 0 and up to 8 strictly ascending cuts >= 1.  A cluster is SELECTED iff
b > a and (a < first, or a < c <= b for some cut c); an entry is undecided iff its cluster is selected.

`selected_links` follows that text on the sorted row.  `selected_pairs` never sorts: clusters are the connected components of the tie graph
over all pairs, a component's first place is the number of entries OUTSIDE it that rank ahead of it (a component is contiguous in the
order, so that is the place of its first member), and it is selected iff its size is > 1 and (start < first, or start < c < start + size
for some cut c).
"""
import numpy as np

from tests import refine_cases as R

F32 = np.float32


def selected_links(row: np.ndarray, margin, first: int, cuts=()) -> np.ndarray:
    """-> undecided (K,) bool, by column."""
    k = len(row)
    order, key = R.order_desc(row), R.keys(row)
    s = key[order]
    with np.errstate(invalid="ignore", over="ignore"):
        link = (s[:-1] - s[1:]) <= R.width_of(margin)                     # link[j]: places j and j + 1
    a = np.flatnonzero(np.concatenate([[True], ~link]))                  # every cluster's first place: place 0 and every place after a missing link
    b = np.concatenate([a[1:] - 1, [k - 1]])                              # ... and its last
    chosen = a < first
    for c in cuts:
        chosen |= (a < c) & (c <= b)
    chosen &= b > a
    sel_sorted = np.repeat(chosen, b - a + 1)
    und = np.zeros(k, dtype=bool)
    und[order] = sel_sorted
    return und


def selected_pairs(row: np.ndarray, margin, first: int, cuts=()) -> np.ndarray:
    """The same without a sort."""
    k = len(row)
    key = R.keys(row)
    _, label = R.undecided_pairs(row, margin)
    col = np.arange(k)
    with np.errstate(invalid="ignore"):
        ahead = (key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) & (col[None, :] < col[:, None]))   # ahead[i, j]: j ranks before i
    und = np.zeros(k, dtype=bool)
    for lab in set(label[label >= 0].tolist()):
        inside = label == lab
        size = int(inside.sum())
        member = int(np.where(inside)[0][0])
        start = int((ahead[member] & ~inside).sum())
        if size > 1 and (start < first or any(start < c < start + size for c in cuts)):
            und |= inside
    return und


def selected_positions(values: np.ndarray, margin, first: int, cuts=(), active=None) -> np.ndarray:
    """What cir_rank_undecided_cuts writes for a (Q, K) matrix: the flat positions q * K + k of the selected entries, ascending."""
    q, k = values.shape
    out = []
    for r in range(q):
        if active is not None and not active[r]:
            continue
        out.append(r * k + np.where(selected_links(values[r], margin, first, cuts))[0])
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, dtype=np.int64)


def hybrid(fast: np.ndarray, ref: np.ndarray, margin, first: int, cuts=()) -> np.ndarray:
    """The refined row: the referee's value on every selected entry, the fast value elsewhere."""
    return np.where(selected_links(fast, margin, first, cuts), np.asarray(ref, dtype=F32), np.asarray(fast, dtype=F32))


def guarantee_holds(fast: np.ndarray, ref: np.ndarray, margin, first: int, cuts=()) -> bool:
    """(i) places 0 .. min(first, K) - 1 of the refined row's order hold the referee row's columns; (ii) for every cut c < K the set of
    columns in places 0 .. c - 1 is the referee row's."""
    k = len(fast)
    got, want = R.order_desc(hybrid(fast, ref, margin, first, cuts)), R.order_desc(ref)
    n = min(first, k)
    if not np.array_equal(got[:n], want[:n]):
        return False
    return all(set(got[:c].tolist()) == set(want[:c].tolist()) for c in cuts if c < k)


def selection_grid(k: int):
    """(first, cuts) pairs every test walks for a row of K entries: first at 0, 1, K - 1, K, K + 7; cuts at 1, at K - 1, at and beyond K, and
    8 of them."""
    grid = [(0, ()), (1, ()), (max(k - 1, 0), ()), (k, ()), (k + 7, ()),
            (0, (1,)), (0, (max(k - 1, 1),)), (0, (k,)), (0, (k + 3,)), (1, (max(k - 1, 2), k + 2)),
            (0, tuple(range(1, 9))), (2, tuple(1 + (i * max(k, 8)) // 8 + i for i in range(8)))]
    return grid


def theorem_rows(seed: int, n: int):
    """refine_cases.theorem_row over the shapes, margins and magnitudes of its own test, with a (first, cuts) drawn from the grid and at random."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        k = int(rng.choice([1, 2, 3, 5, 8, 33, 100, 105]))
        margin = float(rng.choice([0.0, 1e-4, 3e-3, 0.05, 0.5]))
        scale = float(rng.choice([0.02, 0.3, 3.0]))
        offset = float(rng.choice([0.0, 0.0, 1e5, -1e5]))
        if rng.integers(2):
            grid = selection_grid(k)
            first, cuts = grid[int(rng.integers(len(grid)))]
        else:
            first = int(rng.integers(0, k + 2))
            cuts = tuple(sorted(set(int(c) for c in rng.integers(1, k + 3, size=int(rng.integers(0, 5))))))
        yield rng, k, margin, scale, offset, first, cuts


def profile_rows(n: int = 2000, k: int = 100, sigma: float = 0.14, seed: int = 0) -> np.ndarray:
    """The "separated-logit" profile of tools/refine_bench.py: n rows of k fp32 N(0, sigma^2) values."""
    return (sigma * np.random.default_rng(seed).standard_normal((n, k))).astype(F32)
