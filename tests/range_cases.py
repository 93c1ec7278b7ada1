"""The float64 reference, the cases and the checkers of the range search tests
(test_range_cases.py on the CPU, test_gpu_range.py on the GPU).  A plain module; corpora,
queries, masks and the fp32 bound are grouped_cases's.

The definition (include/mq.h, "Range search"): row r is a candidate of a query when the mask
admits it; a hit is a candidate whose score (the dot of the query with the row, + 0.0) is >=
min_score; hits rank by (score desc, row asc); the count of hits is exact and may exceed
max_hits; the list is the first min(count, max_hits) hits, padded with (-inf, -1).
`range_reference` states exactly that in float64, as a plain sort.

Two classes of data, as in grouped_cases: on the exact class every dot is a multiple of 1/16,
exact in fp32 in any order, and the device must equal the reference bit for bit - counts, ids
and scores.  On the random class an fp32 dot is within b = bound(dim) of float64, so with
tau = min_score and v = the max_hits-th largest float64 score of the candidates (-inf when they
are fewer) `check_random` asks:
  * every returned score is within b of the float64 score of its id;
  * the list is sorted by its own (score desc, id asc), ids distinct, candidates only, scores
    >= min_score, as many entries as min(count, max_hits), padding after them;
  * #(s64 >= tau + b) <= count <= #(s64 >= tau - b);
  * every row with s64 >= tau + b and s64 > v + 2b is returned;
  * no returned row has s64 < max(tau - b, v - 2b).
That decides every row but those within b of tau or within 2b of v (the row of rank max_hits
itself among them, when it can be returned at all): `undecided_rows`, computed from the
reference alone.  Their share of the positions a case returns may be at most NEAR_TIE_CAP.
"""
import numpy as np

from grouped_cases import (MASKS, NEAR_TIE_CAP, bound, dots64, exact_corpus, exact_queries,  # noqa: F401
                           mask_words, random_corpus, random_queries, row_mask)

MAX_HITS_LIMIT = 4096
# exact class (test_gpu_range.py rotates the combinations)
NS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 4097)
DIMS = (64, 256, 768, 1024)
NQS = (1, 2, 16, 17, 40)          # 17 and 40 cross the 16-query pass boundary
MAX_HITS = (1, 5, 64, 65, 1000, 4096)
# 3/4 is the largest score of the 4097-row corpora at dims 256, 768 and 1024 (a handful of hits;
# at dim 64 the largest is 11/16), 0.8 is above every score (no hits); -0.0 must behave as 0.0
MIN_SCORES = (-np.inf, -1 / 16, -0.0, 0.0, 1 / 32, 1 / 4, 3 / 4, 0.8)
# random class: (dim, n rows), 17 queries each, every max_hits of random_max_hits(n) at every
# min_score of random_min_scores(dim); a case is one (dim, n, min_score).  The wide dims leave
# min_score 0.1 out: about 20 rows reach it there, too few positions for the cap to mean much.
RANDOM_SHAPES = ((64, 3000), (256, 1000), (768, 700), (1024, 600), (64, 4500))
RANDOM_NQ = 17


def random_max_hits(n):
    return (64, 65, 300, min(n, MAX_HITS_LIMIT))


def random_min_scores(dim):
    return (-np.inf, 0.0, 0.05) + ((0.1,) if dim <= 256 else ())


# ---------------------------------------------------------------- the definition ----
def range_reference(scores64, mask, min_score, max_hits):
    """scores64 [nq, n] float64 (dots64), mask bool [n] or None -> (counts int64 [nq], scores
    float64 [nq, max_hits], ids int64 [nq, max_hits]) of the definition."""
    s = np.atleast_2d(np.asarray(scores64, np.float64)) + 0.0
    nq, n = s.shape
    rows = np.arange(n) if mask is None else np.flatnonzero(np.asarray(mask, bool))
    counts = np.zeros(nq, np.int64)
    out_s = np.full((nq, max_hits), -np.inf)
    out_i = np.full((nq, max_hits), -1, np.int64)
    for j in range(nq):
        hits = rows[s[j, rows] >= min_score]
        counts[j] = len(hits)
        order = hits[np.lexsort((hits, -s[j, hits]))][:max_hits]
        out_i[j, :len(order)] = order
        out_s[j, :len(order)] = s[j, order]
    return counts, out_s, out_i


def reference_by_loop(s, mask, min_score, max_hits):
    """One query, by a loop over the rows and Python's sort -> (count, [(score, row)])."""
    hits = []
    for r in range(len(s)):
        if (mask is None or mask[r]) and float(s[r]) + 0.0 >= min_score:
            hits.append((float(s[r]) + 0.0, r))
    hits.sort(key=lambda e: (-e[0], e[1]))
    return len(hits), hits[:max_hits]


# ------------------------------------------------------------------- random class ----
def _rank_score(s_ok, max_hits):
    """v: the max_hits-th largest of the candidates' float64 scores, -inf when they are fewer."""
    return -np.inf if len(s_ok) < max_hits else float(np.partition(s_ok, len(s_ok) - max_hits)[len(s_ok) - max_hits])


def undecided_rows(s, ok, min_score, max_hits, dim):
    """One query: the number of candidate rows the checks of `check_random` leave open - within
    bound(dim) of min_score or within twice that of v - among those that can be returned at
    all (s64 >= min_score - bound(dim)).  From the reference alone."""
    b = bound(dim)
    so = s[ok]
    v = _rank_score(so, max_hits)
    near = (np.abs(so - min_score) <= b) | (np.abs(so - v) <= 2 * b)
    return int((near & (so >= min_score - b)).sum())


def returned_positions(s, ok, min_score, max_hits):
    """One query: the entries the reference's list holds."""
    return int(min(max_hits, (s[ok] + 0.0 >= min_score).sum()))


def check_random(count, got_s, got_i, s, ok, min_score, max_hits, dim):
    """One query's device result (count, scores [max_hits], ids [max_hits]) against the float64
    scores s [n] of the candidates `ok` -> failures (the module docstring's list)."""
    b = bound(dim)
    tau32 = np.float32(min_score)
    so = s[ok]
    v = _rank_score(so, max_hits)
    fails = []
    lo, hi = int((so >= min_score + b).sum()), int((so >= min_score - b).sum())
    if not lo <= count <= hi:
        fails.append("count %d outside [%d, %d]" % (count, lo, hi))
    m = int(min(count, max_hits))
    ids, sc = got_i[:m], got_s[:m]
    if (got_i[m:] != -1).any() or not np.isneginf(got_s[m:]).all():
        fails.append("padding does not start at position %d" % m)
    if (ids < 0).any() or (ids >= len(s)).any():
        return fails + ["an id outside [0, n) among the first %d" % m]
    if len(set(ids.tolist())) != m:
        fails.append("ids repeat")
    if not ok[ids].all():
        fails.append("a row that is no candidate")
    if not (sc >= tau32).all():
        fails.append("a score below min_score")
    if m > 1 and not ((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (ids[:-1] < ids[1:]))).all():
        fails.append("not sorted by (score desc, id asc)")
    err = np.abs(sc.astype(np.float64) - s[ids])
    if m and err.max() > b:
        fails.append("score off by %.3g (bound %.3g)" % (err.max(), b))
    must = np.flatnonzero(ok & (s >= min_score + b) & (s > v + 2 * b))
    missing = np.setdiff1d(must, ids)
    if len(missing):
        fails.append("rows %s must be returned" % missing[:5].tolist())
    floor = max(min_score - b, v - 2 * b)
    if m and (s[ids] < floor).any():
        fails.append("rows %s lie below %.9g" % (ids[s[ids] < floor][:5].tolist(), floor))
    return fails
