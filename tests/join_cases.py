"""The float64 reference, the corpora and the checkers of the self-join tests
(test_join_cases.py and test_join_host.py on the CPU, test_gpu_join.py on the GPU).  A plain
module; the exact class, the masks and the fp32 bound are grouped_cases's.

The definition (include/mq.h, "Self-join"): j is a partner of left row i when the mask admits
both, j != i and score(i, j) = the dot of the two stored rows, + 0.0, is >= min_score.  Per left
row: the number of partners, the smallest partner row (-1: none), the partner that ranks first by
(score desc, row asc) and its score (-1, -inf: none).  A left row outside the mask has no partner.
`join_reference` states exactly that in float64; `reference_by_loop` is the plain loop.

Two classes of data.  On the exact class (grouped_cases.exact_corpus: coordinates +-1/4, rows
repeating from a third as many vectors) every dot is a multiple of 1/16, exact in fp32 and in
bf16 in any order, and the device must equal the reference bit for bit.  The random class is
`neardup_corpus`: families of about 8 members around a unit Gaussian base, member =
normalise(base + sigma z) with sigma uniform in [0.1, 0.6] and z ~ N(0, I / dim), so the cosine
of two members is about 1 / sqrt((1 + sigma1^2)(1 + sigma2^2)) and the pair cosines straddle
0.8 to 0.95.  An fp32 dot is within b = bound(dim) of float64, so `check_random` leaves a left
row undecided when one of its pairs lies within b of min_score or its two best partners lie
within 2b of each other, and asks every other row to match the reference exactly in count,
first and nearest, with the nearest score within b.  Undecided rows may be at most NEAR_TIE_CAP
of the left rows (test_join_cases.py holds every case to it from the reference alone).
"""
import functools

import numpy as np

from grouped_cases import (MASKS, NEAR_TIE_CAP, bound, exact_corpus, mask_words, row_mask)  # noqa: F401

# exact class (test_gpu_join.py rotates the combinations)
NS = (1, 2, 31, 32, 33, 65, 257, 1000, 4097)
DIMS = (64, 256, 768, 1024)
SCREEN_DIMS = (256, 512, 768)
# 1.0 is the score of a repeated row, 1.0625 is above every score; -0.0 must behave as 0.0
MIN_SCORES = (-np.inf, -0.0, 1 / 4, 3 / 4, 1.0, 1.0625)
LEFTS = ("all", "third", "single", "reversed")
# random class: (dim, n rows), each at every min_score of RANDOM_MIN_SCORES
RANDOM_SHAPES = ((256, 1000), (512, 900), (768, 700), (256, 4500), (64, 3000), (1024, 600))
RANDOM_MIN_SCORES = (0.8, 0.9, 0.95)
FAMILY = 8


def left_rows(kind, n):
    """-> int64 left rows, or None for every row.  third: every third row; single: one row;
    reversed: every row, descending (the outputs follow the list's order)."""
    if kind == "all":
        return None
    if kind == "third":
        return np.arange(0, n, 3, dtype=np.int64)
    if kind == "single":
        return np.array([n // 2], np.int64)
    return np.arange(n - 1, -1, -1, dtype=np.int64)


# ---------------------------------------------------------------- the definition ----
def scores64(rows, left=None):
    """-> float64 [n_left, n]: the dots of the left rows with every row, + 0.0."""
    r = np.asarray(rows, np.float64)
    return (r if left is None else r[left]) @ r.T + 0.0


def join_reference(s, left, mask, min_score):
    """s: scores64(rows, left); left: int64 [n_left] or None; mask: bool [n] or None ->
    (counts int64, first int64, nearest int64, nearest scores float64), all [n_left]."""
    n_left, n = s.shape
    left = np.arange(n) if left is None else np.asarray(left)
    ok = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    part = (s >= min_score) & ok[None, :] & ok[left][:, None]
    part[np.arange(n_left), left] = False
    counts = part.sum(1).astype(np.int64)
    first = np.where(counts > 0, part.argmax(1), -1).astype(np.int64)
    sp = np.where(part, s, -np.inf)
    nearest = np.where(counts > 0, sp.argmax(1), -1).astype(np.int64)  # argmax: the lowest row of the best score
    return counts, first, nearest, sp.max(1, initial=-np.inf)


def reference_by_loop(s_row, i, mask, min_score):
    """One left row i, by a loop over the rows -> (count, first, nearest, nearest score)."""
    count, first, nearest, best = 0, -1, -1, -np.inf
    for j in range(len(s_row)):
        if j == i or (mask is not None and not (mask[i] and mask[j])):
            continue
        x = float(s_row[j]) + 0.0
        if x >= min_score:
            count += 1
            if first < 0:
                first = j
            if x > best:  # rows ascend: an equal score keeps the lower row
                nearest, best = j, x
    return count, first, nearest, best


# ------------------------------------------------------------------- random class ----
@functools.lru_cache(maxsize=None)
def neardup_corpus(dim, n, seed=0):
    """rows [n, dim] float32 (read-only): each row a noisy copy of one of ceil(n / FAMILY) unit
    Gaussian bases, the base drawn at random (families of about FAMILY members)."""
    rng = np.random.default_rng([seed, dim, n, 18])
    n_fam = (n + FAMILY - 1) // FAMILY
    base = rng.standard_normal((n_fam, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    fam = rng.integers(0, n_fam, n)
    sigma = rng.uniform(0.1, 0.6, n)
    rows = base[fam] + sigma[:, None] * rng.standard_normal((n, dim)) / np.sqrt(dim)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows = rows.astype(np.float32)
    rows.setflags(write=False)
    return rows


def undecided_rows(s, left, mask, min_score, dim):
    """bool [n_left]: the left rows `check_random` leaves open - a pair within bound(dim) of
    min_score, or the two best partners within twice that of each other.  From the reference."""
    b = bound(dim)
    n_left, n = s.shape
    left = np.arange(n) if left is None else np.asarray(left)
    ok = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    pair = ok[None, :] & ok[left][:, None]
    pair[np.arange(n_left), left] = False
    near_tau = (pair & (np.abs(s - min_score) <= b)).any(1)
    sp = np.where(pair & (s >= min_score), s, -np.inf)
    if n >= 2:
        top2 = -np.partition(-sp, 1, axis=1)[:, :2]
        two = np.isfinite(top2[:, 1])
        near_best = two & (np.where(two, top2[:, 0], 0.0) - np.where(two, top2[:, 1], 0.0) <= 2 * b)
    else:
        near_best = np.zeros(n_left, bool)
    return near_tau | near_best


def check_random(got, s, left, mask, min_score, dim):
    """got = (counts, first, nearest, nearest scores) of the device -> (failures, undecided
    bool [n_left]).  A decided row equals the reference in count, first and nearest and its
    score is within bound(dim) of the float64 score; an undecided row's count lies between the
    pairs at or above min_score + b and those at or above min_score - b."""
    b = bound(dim)
    counts, first, nearest, scores = (np.asarray(a) for a in got)
    rc, rf, rn, rs = join_reference(s, left, mask, min_score)
    und = undecided_rows(s, left, mask, min_score, dim)
    lo = join_reference(s, left, mask, min_score + b)[0]
    hi = join_reference(s, left, mask, min_score - b)[0]
    fails = []
    for p in range(len(counts)):
        if und[p]:
            if not lo[p] <= counts[p] <= hi[p]:
                fails.append("position %d (undecided): count %d outside [%d, %d]" % (p, counts[p], lo[p], hi[p]))
            continue
        if (counts[p], first[p], nearest[p]) != (rc[p], rf[p], rn[p]):
            fails.append("position %d: (count, first, nearest) = (%d, %d, %d), reference (%d, %d, %d)"
                         % (p, counts[p], first[p], nearest[p], rc[p], rf[p], rn[p]))
        elif rc[p] == 0:
            if scores[p] != -np.inf:
                fails.append("position %d: score %r with no partner" % (p, scores[p]))
        elif abs(float(scores[p]) - rs[p]) > b:
            fails.append("position %d: score %.9g, float64 %.9g" % (p, scores[p], rs[p]))
    return fails, und


# ------------------------------------------------------------ the bf16 screen, restated ----
def to_bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)).view(np.float32)


def screen_bound(rows, dim):
    """The bound E of csrc/join.hip on |score - bf16 score|, from the rows' rounding maxima."""
    r = np.asarray(rows, np.float64)
    d = np.linalg.norm(r - to_bf16(rows).astype(np.float64), axis=1).max() * 1.001
    c = np.linalg.norm(r, axis=1).max() * 1.001
    g = 2 * dim * 2.0 ** -24
    return (2 * d * c + d * d + g * (c + d) ** 2 + g * c * c) * 1.001 + 1e-7


def screen_only_pairs(rows, s, min_score, dim):
    """Ordered pairs (i != j) whose bf16 dot clears min_score - E while the float64 score stays
    below min_score: what the screen lists and the verification must drop."""
    r16 = to_bf16(rows).astype(np.float64)
    s16 = r16 @ r16.T
    hit = (s16 >= min_score - screen_bound(rows, dim)) & (s < min_score)
    np.fill_diagonal(hit, False)
    return int(hit.sum())


# ---------------------------------------------------------- the greedy rule, restated ----
def greedy_keep(s, min_score, left=None, mask=None):
    """The sequential greedy rule by a plain loop -> bool [n] kept: a row of `left` (None: every
    row) that the mask admits is kept iff no KEPT earlier admitted row is its partner; every
    other row is kept."""
    n = s.shape[0]
    ok = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    may_drop = np.zeros(n, bool)
    may_drop[np.arange(n) if left is None else left] = True
    kept = np.ones(n, bool)
    for r in range(n):
        if may_drop[r] and ok[r]:
            earlier = np.flatnonzero(kept[:r] & ok[:r])
            kept[r] = not (s[r, earlier] + 0.0 >= min_score).any()
    return kept


def numpy_scan_first(s, min_score):
    """A stand-in for the device scan of `greedy_dedup_rounds`: (rows, mask) -> each row's
    smallest partner among the rows of the mask, or -1."""
    def scan(rows, mask):
        part = (s[rows] >= min_score) & mask[None, :] & mask[rows][:, None]
        part[np.arange(len(rows)), rows] = False
        return np.where(part.any(1), part.argmax(1), -1)
    return scan
