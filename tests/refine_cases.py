"""The rank-refinement rule (include/cirrank.h, cir_rank_undecided) restated in numpy fp32, two ways, and the rows its theorem is tried on.

The rule: sort a row of fast logits in cir_topk_desc's order (value descending, ties to the lower column, a NaN as -inf); with width =
2 * margin in fp32, neighbours a, b of the sorted row are LINKED iff the fp32 difference a - b <= width (a difference that is not a number
links nothing); an entry is UNDECIDED iff it is linked to a neighbour; a CLUSTER is a maximal run of linked entries.

`undecided_links` follows that text.  `undecided_pairs` does not sort: two entries are tied iff the fp32 difference of the larger and the
smaller key is at most width, an entry is undecided iff it is tied to any other, and a cluster is a connected component of the tie graph.
The two agree because rounding is monotone: a third value between two tied ones is tied to both.
"""
import numpy as np

F32 = np.float32


def keys(row: np.ndarray) -> np.ndarray:
    row = np.asarray(row, dtype=F32)
    return np.where(np.isnan(row), F32(-np.inf), row)


def order_desc(row: np.ndarray) -> np.ndarray:
    """cir_topk_desc's order: value descending, ties to the lower column, NaN as -inf."""
    return np.argsort(-keys(row), kind="stable")


def width_of(margin) -> np.float32:
    return F32(2.0) * F32(margin)


def undecided_links(row: np.ndarray, margin):
    """-> (undecided (K,) bool, cluster (K,) int: the same number within a cluster, -1 for a decided entry)."""
    k = len(row)
    order, key = order_desc(row), keys(row)
    s = key[order]
    with np.errstate(invalid="ignore", over="ignore"):
        link = (s[:-1] - s[1:]) <= width_of(margin)                       # (K - 1,): NaN compares false
    und_sorted = np.zeros(k, dtype=bool)
    und_sorted[:-1] |= link
    und_sorted[1:] |= link
    run = np.concatenate([[0], np.cumsum(~link)]) if k > 1 else np.zeros(1, dtype=np.int64)      # a new run starts after every missing link
    und, cluster = np.zeros(k, dtype=bool), np.full(k, -1, dtype=np.int64)
    und[order] = und_sorted
    cluster[order] = np.where(und_sorted, run, -1)
    return und, cluster


def undecided_pairs(row: np.ndarray, margin):
    """The same by brute force over all pairs, without a sort: -> (undecided, cluster) as above (cluster numbers differ)."""
    k = len(row)
    key = keys(row)
    with np.errstate(invalid="ignore", over="ignore"):
        hi, lo = np.maximum(key[:, None], key[None, :]), np.minimum(key[:, None], key[None, :])
        tied = (hi - lo) <= width_of(margin)
    tied &= ~np.eye(k, dtype=bool)
    und = tied.any(axis=1)
    label = np.arange(k)
    while True:                                                           # connected components: every entry takes the lowest label it is tied to
        new = np.where(tied, label[None, :], k).min(axis=1, initial=k)
        new = np.minimum(label, new)
        if np.array_equal(new, label):
            break
        label = new
    return und, np.where(und, label, -1)


def same_partition(a: np.ndarray, b: np.ndarray) -> bool:
    """Two cluster labelings name the same clusters."""
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = {(int(x), int(y)) for x, y in zip(a, b) if x >= 0}
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


def undecided_positions(values: np.ndarray, margin, active=None):
    """What cir_rank_undecided writes for a (Q, K) matrix: the flat positions q * K + k of all undecided entries, ascending."""
    q, k = values.shape
    out = []
    for r in range(q):
        if active is not None and not active[r]:
            continue
        out.append(r * k + np.where(undecided_links(values[r], margin)[0])[0])
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, dtype=np.int64)


def hybrid(fast: np.ndarray, ref: np.ndarray, margin) -> np.ndarray:
    """The refined row: the referee's value on every undecided entry, the fast value elsewhere."""
    return np.where(undecided_links(fast, margin)[0], np.asarray(ref, dtype=F32), np.asarray(fast, dtype=F32))


def theorem_row(rng: np.random.Generator, k: int, margin: float, scale: float, offset: float = 0.0, ties: int = 0, specials: int = 0):
    """(fast, ref) with |fast - ref| <= margin on every entry, the premise of the theorem: ref random fp32 (with `ties` exact repeats and
    `specials` NaN / +-inf entries), fast = fp32(ref + U(-margin, margin)).  Where that rounding carried an entry past the margin - at
    magnitude 1e5 an ulp is 0.0078 - the entry takes the nearest fp32 value inside the bound, or ref itself."""
    ref = (offset + scale * rng.standard_normal(k)).astype(F32)
    for _ in range(ties):
        ref[rng.integers(k)] = ref[rng.integers(k)]
    m = float(F32(margin))
    fast = (ref.astype(np.float64) + rng.uniform(-m, m, k)).astype(F32)
    over = np.abs(fast.astype(np.float64) - ref.astype(np.float64)) > m
    toward = np.nextafter(fast, ref)
    fast = np.where(over, toward, fast)
    over = np.abs(fast.astype(np.float64) - ref.astype(np.float64)) > m
    fast = np.where(over, ref, fast)
    for _ in range(specials):
        i = rng.integers(k)
        ref[i] = fast[i] = F32(rng.choice([np.nan, np.inf, -np.inf]))
    return fast, ref
