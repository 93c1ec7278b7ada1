"""Corpora, group layouts, masks, the float64 reference and the checkers of the grouped search
tests (test_grouped_cases.py on the CPU, test_gpu_grouped.py on the GPU).  A plain module.

The definition (include/mq.h, "Grouped search"): row r is a candidate of a query when the mask
admits it and 0 <= codes[r] < n_groups; a group's score is the maximum dot over its candidate
rows, its representative the row reaching it (equal scores: the lowest row); groups rank by
(score desc, representative row asc); the top k, padded with (-inf, -1).
`grouped_reference` states exactly that in float64.  `collapse_full_ranking` is what LangChain's
ParentDocumentRetriever does with a top-k that covers every row - the distinct codes of the
full ranking, in order - and the two agree (test_grouped_cases.py).

Two classes of data (all seeded):
  exact   every row and query has 16 non-zero coordinates of +-1/4, drawn from a pool of 24
          coordinates spread over the row: the norm is exactly 1 and every dot is a multiple of
          1/16 of magnitude <= 1, so any summation order in fp32 gives the float64 value and the
          device must equal the reference bit for bit, ids and scores.  Rows are drawn from a
          third as many distinct vectors, so duplicates inside a group and across groups give
          exact ties on purpose.
  random  Gaussian rows, unit-norm up to fp32 rounding; the reference is computed from the rows
          the index stores.  An fp32 dot of unit vectors is within BOUND(dim) = (dim + 8) 2^-24
          of float64 (sum |a_i b_i| <= 1), so a position may hold another id only inside a
          near-tie: reference scores within twice that bound (`near_tie_positions`, computed
          from the reference alone).  Near-tie positions may be at most NEAR_TIE_CAP of a
          test's positions.
"""
import functools

import numpy as np

EXACT_NNZ, EXACT_VAL, EXACT_POOL = 16, 0.25, 24
LAYOUTS = ("singletons", "one", "families", "interleaved", "sprinkled")
MASKS = ("none", "ones", "zeros", "third", "single")
NEAR_TIE_CAP = 0.05
# The random-class cases of the GPU test: (dim, n rows, layout, mask, nq, seed), each run at
# every k of RANDOM_KS; a case's positions are those of all its k.  Gaussian dots crowd as the
# dim grows (their spread is dim^-1/2 while BOUND grows with dim), so the wide cases hold fewer
# rows: the shapes were picked with the reference alone (test_grouped_cases.py keeps each
# inside the cap), before any device result existed.
RANDOM_CASES = ((64, 3000, "families", "none", 17, 0), (64, 3000, "sprinkled", "third", 16, 1),
                (64, 3000, "singletons", "none", 17, 0), (256, 1000, "families", "ones", 17, 5),
                (768, 700, "families", "none", 17, 2), (768, 700, "interleaved", "third", 17, 3),
                (1024, 600, "sprinkled", "none", 17, 4))
RANDOM_KS = (5, 64)


def bound(dim):
    """|fp32 dot - float64 dot| of unit vectors of `dim` coordinates, whatever the order."""
    return (dim + 8) * 2.0 ** -24


# ---------------------------------------------------------------- the definition ----
def dots64(rows, queries):
    """queries [nq, d] . rows [n, d] -> [nq, n] float64, every entry summed in the same order
    (einsum's own loop): bitwise-equal rows give bitwise-equal dots."""
    return np.einsum("qd,nd->qn", np.asarray(queries, np.float64), np.asarray(rows, np.float64))


def candidates(codes, mask, n_groups=None):
    codes = np.asarray(codes)
    ok = codes >= 0
    if n_groups is not None:
        ok &= codes < n_groups
    if mask is not None:
        ok &= np.asarray(mask, bool)
    return ok


def group_best(s, codes, ok):
    """One query's scores s [n] -> {code: (best score, lowest row reaching it)} over the
    candidate rows `ok`, by a plain loop over the rows: the definition, nothing else."""
    best = {}
    for r in np.flatnonzero(ok).tolist():
        c, x = int(codes[r]), float(s[r])
        if c not in best or x > best[c][0]:  # rows ascend: an equal score keeps the lower row
            best[c] = (x, r)
    return best


def grouped_reference(rows64, q64, codes, mask, k, n_groups=None, scores=None):
    """-> (scores float64 [nq, k], ids int64 [nq, k]) of the definition, padded with (-inf, -1).
    n_groups None: every non-negative code is in range.  Computed as the sort of `group_best`'s
    values by (score desc, row asc), vectorised: the candidates ranked by (score desc, row asc),
    the first row of each code (np.unique's first index), those in rank order
    (test_grouped_cases.py holds it against the loop).  scores: dots64(rows64, q64) when the
    caller has it already (computed once, shared among the cases of one corpus)."""
    s = dots64(rows64, np.atleast_2d(q64)) if scores is None else scores
    codes = np.asarray(codes)
    rows = np.flatnonzero(candidates(codes, mask, n_groups))
    out_s = np.full((s.shape[0], k), -np.inf)
    out_i = np.full((s.shape[0], k), -1, np.int64)
    for j in range(s.shape[0]):
        order = rows[np.lexsort((rows, -s[j, rows]))]
        first = np.sort(np.unique(codes[order], return_index=True)[1])[:k]
        out_i[j, :len(first)] = order[first]
        out_s[j, :len(first)] = s[j, order[first]]
    return out_s, out_i


def reference_by_loop(s, codes, ok, k):
    """One query's top-k [(score, row)] straight from `group_best`."""
    return sorted(group_best(s, codes, ok).values(), key=lambda e: (-e[0], e[1]))[:k]


def collapse_full_ranking(s, codes, ok):
    """LangChain's collapse over a ranking of EVERY candidate row (score desc, row asc): the
    first row of each distinct code, in order -> [(score, row)]."""
    rows = np.flatnonzero(ok)
    order = rows[np.lexsort((rows, -np.asarray(s)[rows]))]
    seen, out = set(), []
    for r in order.tolist():
        c = int(codes[r])
        if c not in seen:
            seen.add(c)
            out.append((float(s[r]), r))
    return out


# -------------------------------------------------------------------- exact class ----
def _pool(dim, seed):
    return np.sort(np.random.default_rng([seed, dim, 1]).choice(dim, EXACT_POOL, replace=False))


def _exact_vectors(dim, count, seed, stream):
    rng = np.random.default_rng([seed, dim, count, stream])
    pool = _pool(dim, seed)
    out = np.zeros((count, dim), np.float32)
    for i in range(count):
        sup = rng.choice(pool, EXACT_NNZ, replace=False)
        out[i, sup] = rng.choice(np.array([-EXACT_VAL, EXACT_VAL], np.float32), EXACT_NNZ)
    return out


@functools.lru_cache(maxsize=None)
def exact_corpus(dim, n, seed=0):
    """rows [n, dim] float32 (read-only), drawn with repeats from ceil(n / 3) distinct vectors."""
    base = _exact_vectors(dim, (n + 2) // 3, seed, 2)
    rows = base[np.random.default_rng([seed, dim, n, 3]).integers(0, len(base), n)]
    assert np.all((rows.astype(np.float64) ** 2).sum(1) == 1.0)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def exact_queries(dim, nq, seed=0):
    """Exact-class vectors over the corpus's coordinate pool: half of them corpus-like draws,
    so some equal a stored row (score exactly 1)."""
    q = _exact_vectors(dim, nq, seed, 4)
    q.setflags(write=False)
    return q


# ------------------------------------------------------------- layouts and masks ----
def group_codes(layout, n, seed=0):
    """-> (codes int32 [n], n_groups).  singletons: one group per row; one: a single group;
    families: contiguous families of 1..100 children; interleaved: r % G; sprinkled: the
    families with absent (-1) and out-of-range codes (negative, n_groups + 3, INT32_MAX) put in."""
    rng = np.random.default_rng([seed, n, LAYOUTS.index(layout)])
    if layout == "singletons":
        return np.arange(n, dtype=np.int32), n
    if layout == "one":
        return np.zeros(n, np.int32), 1
    if layout == "interleaved":
        g = max(1, min(n, 7 + n // 50))
        return (np.arange(n) % g).astype(np.int32), g
    codes = np.empty(n, np.int32)
    r = g = 0
    while r < n:
        size = int(rng.integers(1, 101))
        codes[r:r + size] = g
        r += size
        g += 1
    if layout == "sprinkled":
        codes[1::5] = -1
        codes[2::7] = g + 3
        codes[3::11] = -7
        codes[4::13] = np.iinfo(np.int32).max
    return codes, g


def row_mask(kind, n):
    """-> bool [n], or None for no mask."""
    if kind == "none":
        return None
    m = np.zeros(n, bool)
    if kind == "ones":
        m[:] = True
    elif kind == "third":
        m[::3] = True
    elif kind == "single":
        m[n // 2] = True
    return m


def mask_words(mask):
    """bool [n] -> int32 words, bit r % 32 of word r / 32 (the masked search's layout)."""
    n = len(mask)
    padded = np.zeros((n + 31) // 32 * 32 or 32, np.uint8)
    padded[:n] = mask
    return np.packbits(padded, bitorder="little").view(np.int32)


# ------------------------------------------------------------------- random class ----
@functools.lru_cache(maxsize=None)
def random_corpus(dim, n, seed=0):
    rng = np.random.default_rng([seed, dim, n, 5])
    rows = rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows = rows.astype(np.float32)
    rows.setflags(write=False)
    return rows


def random_queries(dim, nq, seed=0):
    rng = np.random.default_rng([seed, dim, nq, 6])
    q = rng.standard_normal((nq, dim))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def near_tie_positions(s, codes, ok, ref_s, ref_i, tol):
    """One query: bool [k], position p of the reference is inside a near-tie - another group's
    best score, or another candidate row of its own group, lies within tol of ref_s[p].  Only
    there may fp32 arithmetic put another id.  Padding positions are never near-ties."""
    best = group_best(s, codes, ok)
    gs = np.array(sorted(x for x, _ in best.values()))
    out = np.zeros(len(ref_i), bool)
    for p, (x, r) in enumerate(zip(ref_s, ref_i)):
        if r < 0:
            continue
        others = np.searchsorted(gs, x + tol, "right") - np.searchsorted(gs, x - tol, "left") - 1
        own = ok & (np.asarray(codes) == codes[r])
        out[p] = others > 0 or int((s[own] >= x - tol).sum()) > 1
    return out


def check_random(got_s, got_i, s, codes, ok, ref_s, ref_i, dim):
    """One query's device result against the reference -> (failures, near-tie positions).
    Every valid entry: a candidate row whose float64 dot is within bound(dim) of the returned
    score; equal to the reference's id except inside a near-tie (2 bound(dim)), where it must
    still be a candidate row whose group's float64 best is within that of the reference's
    score and whose group is not repeated; padding exactly where the reference pads."""
    b = bound(dim)
    near = near_tie_positions(s, codes, ok, ref_s, ref_i, 2 * b)
    best = group_best(s, codes, ok)
    fails, seen = [], set()
    for p, (x, r) in enumerate(zip(got_s.tolist(), got_i.tolist())):
        if ref_i[p] < 0 or r < 0:
            if r != ref_i[p] or (r < 0 and x != -np.inf):
                fails.append("position %d: (%r, %d), reference id %d" % (p, x, r, ref_i[p]))
            continue
        if not ok[r]:
            fails.append("position %d: row %d is no candidate" % (p, r))
            continue
        if codes[r] in seen:
            fails.append("position %d: group %d repeats" % (p, codes[r]))
        seen.add(int(codes[r]))
        if abs(x - s[r]) > b:
            fails.append("position %d: score %.9g, float64 %.9g" % (p, x, s[r]))
        if r != ref_i[p]:
            if not near[p]:
                fails.append("position %d: row %d, reference row %d outside a near-tie" % (p, r, ref_i[p]))
            elif abs(best[int(codes[r])][0] - ref_s[p]) > 2 * b or s[r] < best[int(codes[r])][0] - 2 * b:
                fails.append("position %d: row %d is not within the near-tie of %d" % (p, r, ref_i[p]))
    return fails, near
