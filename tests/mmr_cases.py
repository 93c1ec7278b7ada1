"""Corpora, candidate lists, the float64 reference and the path checker of the maximal
marginal relevance tests (test_mmr_cases.py on the CPU, test_gpu_mmr.py on the GPU).  A plain
module.

The algorithm (LangChain's maximal_marginal_relevance; include/mq.h, mq_index_mmr_select):
candidates c_0 .. c_{m-1} in list order, s_i their similarity to the query, G[i][j] the
cosine of candidates i and j.  Pick 0 = argmax s_i; pick t = argmax over the unpicked i of
lam * s_i - (1 - lam) * max_{p picked} G[i][p]; every tie goes to the lowest i (a strict >
scan); min(k, m) picks, in selection order.

Two classes of data (all seeded):
  exact   rows with 4^j non-zero entries of +-2^-j (dim 32: 16 x 1/4, 96: 64 x 1/8,
          768: 256 x 1/16, 1024: 1024 x 1/32) on a random support, so the non-zeros fall in
          every K-slice.  Every norm is exactly 1, every dot a multiple of 4^-j of magnitude
          <= 1: exact in fp32 in any summation order; with lam in {0, 1/4, 1/2, 3/4, 1} every
          product and difference of the score is exact too, so fp32 must equal float64 pick
          for pick.  Rows come in families that share a support: the base row, an exact
          copy, two rows one sign flip away (equal scores against the base), a copy of a
          near-copy, then rows 1-3 flips away - ties are common on purpose.
  random  clustered unit rows (64 centroids + 0.35 noise: cluster-mates at cosine ~0.89, as
          the bench's corpus) with the reference corpus's exact-duplicate pattern planted;
          queries are a corpus row plus noise.  fp32 cannot reproduce float64's sequence
          where two scores are closer than the arithmetic's error, so a result is checked
          along its own prefix (check_path) at TOL = 1e-5, the project's tie-group cap for
          the same fp32 dots (oracle/flat.py check_topk tol_cap).
"""
import functools

import numpy as np

LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)  # the exact class's
EXACT_DIMS = {32: (16, 0.25), 96: (64, 0.125), 768: (256, 0.0625), 1024: (1024, 0.03125)}
TOL = 1e-5
MUTANTS = ("red_stale", "last_only", "tie_high", "swap")
DUPLICATE_PAIRS = ((72, 74), (104, 105), (110, 111), (120, 121))  # synth.REF_DUPLICATE_PAIRS


# ---------------------------------------------------------------- the algorithm ----
def mmr_reference(s, G, lam, k):
    """The picks (list positions, selection order) in float64."""
    s = np.asarray(s, np.float64)
    G = np.asarray(G, np.float64)
    m = s.shape[0]
    if m == 0 or k <= 0:
        return []
    picks = [int(np.argmax(s))]  # np.argmax returns the first maximum: ties to the lowest i
    free = np.ones(m, bool)
    free[picks[0]] = False
    red = G[:, picks[0]].copy()
    while len(picks) < min(k, m):
        score = np.where(free, lam * s - (1.0 - lam) * red, -np.inf)
        b = int(np.argmax(score))
        picks.append(b)
        free[b] = False
        red = np.maximum(red, G[:, b])
    return picks


def mmr_fp32(s, G, lam, k, mutant=None):
    """The same in fp32 with the arithmetic of include/mq.h (MQ_MMR_SCORE: every product and
    difference rounded to fp32 on its own - numpy's float32 ufuncs do not contract), or one
    of the MUTANTS: `red_stale` stops updating red after the second pick, `last_only` takes
    the last pick's similarity instead of the maximum, `tie_high` breaks ties to the highest
    index, `swap` exchanges lam and 1 - lam."""
    assert mutant is None or mutant in MUTANTS
    f = np.float32
    s = np.asarray(s, f)
    G = np.asarray(G, f)
    a, b = f(lam), f(1.0) - f(lam)
    if mutant == "swap":
        a, b = b, a
    m = s.shape[0]
    if m == 0 or k <= 0:
        return []

    def argmax(x):
        return m - 1 - int(np.argmax(x[::-1])) if mutant == "tie_high" else int(np.argmax(x))

    picks = [argmax(s)]
    free = np.ones(m, bool)
    free[picks[0]] = False
    red = G[:, picks[0]].copy()
    while len(picks) < min(k, m):
        score = np.where(free, a * s - b * red, f(-np.inf))
        p = argmax(score)
        picks.append(p)
        free[p] = False
        if mutant == "last_only":
            red = G[:, p].copy()
        elif not (mutant == "red_stale" and len(picks) > 2):
            red = np.maximum(red, G[:, p])
    return picks


def path_deficits(picks, s64, G64, lam):
    """Per step t: (best float64 score among the unpicked given picks[:t]) - (float64 score
    of picks[t]); 0 where the pick is the float64 argmax.  Step 0 scores by s alone."""
    s = np.asarray(s64, np.float64)
    G = np.asarray(G64, np.float64)
    free = np.ones(len(s), bool)
    red = np.full(len(s), -np.inf)
    out = []
    for t, p in enumerate(picks):
        score = s if t == 0 else lam * s - (1.0 - lam) * red
        out.append(float(np.max(score[free]) - score[p]))
        free[p] = False
        red = np.maximum(red, G[:, p])
    return out


def check_path(picks, s64, G64, lam, tol, k):
    """Failures (empty = pass) of a device result followed along its own prefix: `picks` are
    list positions into s64 / G64 (the valid candidates in list order; a pick that is not one
    of them - padding - is passed as -1).  Every step of the sequence is checked:
      * len(picks) == min(k, m); no pick is padding or a repeat;
      * at step t the float64 score of picks[t] given picks[:t] is at least the best
        float64 score among the unpicked minus tol;
      * where picks[t]'s float64 score EQUALS that best score (bitwise-equal rows: exact
        copies), it is the lowest list position among those that do - the tie rule."""
    s = np.asarray(s64, np.float64)
    G = np.asarray(G64, np.float64)
    m = len(s)
    fails = []
    picks = [int(p) for p in picks]
    if len(picks) != min(k, m):
        return ["%d picks, expected min(k, m) = %d" % (len(picks), min(k, m))]
    free = np.ones(m, bool)
    red = np.full(m, -np.inf)
    for t, p in enumerate(picks):
        if p < 0 or p >= m:
            return fails + ["step %d: pick %d is padding" % (t, p)]
        if not free[p]:
            return fails + ["step %d: pick %d repeats" % (t, p)]
        score = s if t == 0 else lam * s - (1.0 - lam) * red
        best = float(np.max(score[free]))
        if score[p] < best - tol:
            fails.append("step %d: pick %d scores %.9g, best unpicked %.9g (deficit %.3g)"
                         % (t, p, score[p], best, best - score[p]))
        elif score[p] == best:
            lowest = int(np.flatnonzero(free & (score == best))[0])
            if p != lowest:
                fails.append("step %d: pick %d ties with %d, the lower position" % (t, p, lowest))
        free[p] = False
        red = np.maximum(red, G[:, p])
    return fails


def positions(ids, cand_ids):
    """Device row ids -> list positions in cand_ids (the valid candidates, distinct), -1 for
    an id that is not among them; the (-1) padding tail of `ids` is cut."""
    pos = {int(c): j for j, c in enumerate(cand_ids)}
    ids = [int(i) for i in ids]
    while ids and ids[-1] < 0:
        ids.pop()
    return [pos.get(i, -1) for i in ids]


# ------------------------------------------------------------------ exact class ----
@functools.lru_cache(maxsize=None)
def exact_corpus(dim, n_fam, fam, seed=0):
    """-> rows [n_fam * fam, dim] float32 (read-only): member v of family f is row
    v * n_fam + f; v = 0 the base, 1 its exact copy, 2 and 3 one flip away, 4 a copy of 2,
    then 1 + v % 3 flips."""
    nnz, val = EXACT_DIMS[dim]
    rng = np.random.default_rng([seed, dim, n_fam, fam])
    rows = np.zeros((n_fam * fam, dim), np.float32)
    for f in range(n_fam):
        sup = np.sort(rng.choice(dim, nnz, replace=False))
        sign = rng.choice(np.array([-val, val], np.float32), nnz)
        members = []
        for v in range(fam):
            x = sign.copy()
            if v == 1:
                pass
            elif v == 4:
                x = members[2].copy()
            elif v >= 2:
                flips = rng.choice(nnz, 1 if v < 4 else 1 + v % 3, replace=False)
                x[flips] = -x[flips]
            members.append(x)
            rows[v * n_fam + f, sup] = x
    assert np.all((rows.astype(np.float64) ** 2).sum(1) == 1.0)
    rows.setflags(write=False)
    return rows


def exact_queries(rows, n_fam, nq):
    """The base rows of the first nq families (exact-class vectors themselves)."""
    return rows[:n_fam][np.arange(nq) % n_fam].copy()


def exact_candidates(rows, n_fam, fam, q_fam, fetch_k, seed=0):
    """fetch_k distinct row ids for a query on family q_fam: its family's members first (as
    many as fit), the rest drawn from the other rows; sorted as a search returns them
    (score desc, id asc).  -> (ids int64 [fetch_k], s float64 [fetch_k])."""
    rng = np.random.default_rng([seed, q_fam, fetch_k])
    own = np.arange(fam) * n_fam + q_fam
    take = own[:min(fam, max(1, (2 * fetch_k) // 3))]
    others = np.setdiff1d(np.arange(len(rows)), own)
    ids = np.concatenate([take, rng.choice(others, fetch_k - len(take), replace=False)])[:fetch_k]
    s = rows[ids].astype(np.float64) @ rows[q_fam].astype(np.float64)
    order = np.lexsort((ids, -s))
    return ids[order].astype(np.int64), s[order]


def _dots64(a, b):
    """a [m, d] . b [n, d] -> [m, n] in float64, every entry summed over d in the same order
    (einsum's own loop, no blocked BLAS kernel): bitwise-equal rows give bitwise-equal dots,
    so float64 itself ties where the data tie."""
    return np.einsum("id,jd->ij", np.asarray(a, np.float64), np.asarray(b, np.float64))


def gram64(rows, ids):
    r = np.asarray(rows)[np.asarray(ids, np.int64)]
    return _dots64(r, r)


# ----------------------------------------------------------------- random class ----
@functools.lru_cache(maxsize=None)
def random_corpus(dim, n=2048, seed=0):
    """Clustered float32 rows, unit-norm up to fp32 rounding, with DUPLICATE_PAIRS planted
    in every block of 154 rows (read-only)."""
    rng = np.random.default_rng([seed, dim, n])
    cents = rng.standard_normal((64, dim))
    rows = cents[rng.integers(0, 64, n)] + 0.35 * rng.standard_normal((n, dim))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows = rows.astype(np.float32)
    for base in range(0, n - 153, 154):
        for a, b in DUPLICATE_PAIRS:
            rows[base + b] = rows[base + a]
    rows.setflags(write=False)
    return rows


def random_queries(rows, nq, seed=0, noise=0.05):
    """A corpus row plus noise, unit-norm float32; every other query sits on a duplicated row."""
    rng = np.random.default_rng([seed, nq, rows.shape[1]])
    n, dim = rows.shape
    base = rng.integers(0, n, nq)
    dup = [blk + a for blk in range(0, n - 153, 154) for a, _ in DUPLICATE_PAIRS]
    base[::2] = np.asarray(dup)[np.arange(len(base[::2])) % len(dup)]
    q = rows[base].astype(np.float64) + noise * rng.standard_normal((nq, dim)) / np.sqrt(dim)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)


def top_candidates(stored, query, fetch_k, allowed=None):
    """The float64 top-fetch_k of `query` over the stored rows (score desc, id asc; `allowed`:
    a bool row mask).  -> (ids int64, s float64), min(fetch_k, rows allowed) long."""
    s = _dots64(stored, np.asarray(query)[None])[:, 0]
    ids = np.arange(len(s)) if allowed is None else np.flatnonzero(allowed)
    order = np.lexsort((ids, -s[ids]))[:fetch_k]
    return ids[order].astype(np.int64), s[ids[order]]


@functools.lru_cache(maxsize=None)
def random_cases(dim, fetch_k, nq=6, seed=0):
    """The committed random cases of the CPU tests: (s64, G64) per query."""
    rows = random_corpus(dim)
    out = []
    for q in random_queries(rows, nq, seed):
        ids, s = top_candidates(rows, q, fetch_k)
        out.append((s, gram64(rows, ids)))
    return out
