"""Corpora, the float64 BM25 and reciprocal-rank references and the result checker of the
lexical retrieval tests (test_lexical_cases.py / test_lexical_host.py on the CPU,
test_gpu_lexical.py on the GPU).  A plain module.

The definition (include/mq.h, "Lexical retrieval") restated: a row's terms are its body token
ids (ngram 1) or the pairs (id[i] << 16) | id[i + 1] of adjacent tokens of the row (ngram 2);
N, dl, avgdl and df are taken over ALL rows; idf = ln(1 + (N - df + 0.5) / (df + 0.5));
w = qf (k1 + 1) idf, c0 = k1 (1 - b), c1 = k1 b / avgdl in float64, each rounded to fp32 once
(the device gets exactly these numbers); score = sum_t w tf / (tf + c0 + c1 dl), here in float64;
candidates are the rows with a query term that the mask admits, by (score desc, id asc).  More
than MAX_TERMS distinct query terms: the MAX_TERMS with the largest idf stay, ties to the
smaller key.

A corpus is (flat uint16 tokens, int64 offsets [n + 1]), the layout the device takes.

Tolerances (derived, not measured): a device score is within (n_terms + 8) * 2^-24 relative of
the reference (per term about six fp32 roundings, plus the running sum's); a position of the
result must hold the reference's id wherever both neighbours in the reference ranking differ
from it by more than that bound or by exactly 0 (exact ties are ordered by row id: strict),
inside a near-tie group any member passes; at most AMBIGUOUS_CAP of a test's checked
positions may be in near-tie groups.  A near-tie group is a run of reference positions joined
by differences of at most the bound that holds at least one non-zero difference: rows that tie
exactly and sit next to a near tie belong to it (with 1 term, tf = 2, dl = 110 and tf = 1,
dl = 29 differ by 2e-9 relative in float64 and are one fp32 number, so the definition itself
orders those three rows by id), an exact tie with no near tie beside it is checked strictly.
Whatever the group, the result itself must be in (score desc, id asc) order of its own fp32
scores."""
import numpy as np

K1, B = 1.2, 0.75
MAX_TERMS = 128
AMBIGUOUS_CAP = 0.05
MUTANTS = ("rank_bm25_idf", "dl_tokens", "cross_row", "stats_masked", "tie_high", "rrf_rank0")


def score_tol(n_terms):
    return (n_terms + 8) * 2.0 ** -24


# ------------------------------------------------------------------------ corpora ----
def pack(rows):
    """Rows (sequences of token ids) -> (flat uint16, offsets int64 [n + 1])."""
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    flat = np.concatenate([np.asarray(r, np.uint16) for r in rows]) if len(rows) and offs[-1] else np.zeros(0, np.uint16)
    return flat.astype(np.uint16), offs


def unpack(corpus):
    flat, offs = corpus
    return [flat[offs[r]:offs[r + 1]] for r in range(len(offs) - 1)]


def zipf_rows(n, vocab, seed, max_len=300, first_id=1000, copy_every=7):
    """n rows of 0..max_len tokens, Zipf-distributed over `vocab` ids from first_id; every
    copy_every-th row is copied into its neighbour (exact score ties)."""
    rng = np.random.default_rng([seed, n, vocab])
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    rows = [(first_id + rng.choice(vocab, int(rng.integers(0, max_len + 1)), p=p)).astype(np.uint16) for _ in range(n)]
    for r in range(0, n - 1, copy_every):
        rows[r + 1] = rows[r].copy()
    return rows


def query_tokens(rows, n_distinct, seed, ngram=1, repeat=0, absent=0):
    """A query (token id list) with exactly n_distinct distinct terms where the corpus allows:
    terms of the corpus (frequent and rare alike), `repeat` of them said twice (qf = 2) and
    `absent` terms that occur in no row (ids below the corpus's).  ngram 1: a shuffle of the
    chosen ids.  ngram 2: a walk along the blob from a random position (so most pairs are pairs
    of the corpus, a few span a row boundary there) that stops at n_distinct distinct pairs,
    starts with an absent id when `absent`, and is extended by tokens that say a pair again."""
    rng = np.random.default_rng([seed, n_distinct, ngram])
    flat = np.concatenate([np.asarray(r, np.uint32) for r in rows if len(r)] or [np.zeros(0, np.uint32)])
    if ngram == 1:
        pool = np.unique(flat)
        take = rng.permutation(pool)[:max(0, n_distinct - absent)].tolist()
        take += list(range(7, 7 + n_distinct - len(take)))  # ids the corpus lacks
        q = take + take[:repeat]
        return [int(x) for x in rng.permutation(q)]
    q = [3] if absent else []
    seen = set()
    p = int(rng.integers(0, max(1, flat.size)))
    for step in range(flat.size + 1):
        if len(seen) >= n_distinct or not flat.size:
            break
        t = int(flat[(p + step) % flat.size])
        if q:
            seen.add((q[-1], t))
        q.append(t)
    for _ in range(repeat):
        again = sorted(x for x in seen if x[0] == q[-1])
        if not again:
            break
        q.append(again[int(rng.integers(0, len(again)))][1])
    return q


# ---------------------------------------------------------------------- reference ----
def row_of_positions(offs, n_pos):
    """Row of every token position 0 .. n_pos - 1."""
    return np.searchsorted(offs, np.arange(n_pos), side="right") - 1


def corpus_terms(corpus, ngram, cross_row=False):
    """-> (keys uint32 [m], rows int64 [m]): every term of the corpus with its row.  A bigram
    belongs to the row of its second token and needs its first token in the same row
    (cross_row: the mutant that does not ask)."""
    flat, offs = corpus
    flat = flat.astype(np.uint32)
    rows = row_of_positions(offs, flat.size)
    if ngram == 1:
        return flat, rows
    if flat.size < 2:
        return np.zeros(0, np.uint32), np.zeros(0, np.int64)
    keys = (flat[:-1] << np.uint32(16)) | flat[1:]
    ok = rows[:-1] == rows[1:]
    if cross_row:
        ok = np.ones_like(ok)
    return keys[ok], rows[1:][ok]


def query_terms(tokens, ngram):
    t = np.asarray(tokens, np.uint32)
    if ngram == 1:
        return t
    return (t[:-1] << np.uint32(16)) | t[1:] if t.size > 1 else np.zeros(0, np.uint32)


def bm25_setup(corpus, query, ngram, k1=K1, b=B, mask=None, mutant=None, max_terms=MAX_TERMS):
    """Everything a scorer needs, or None for a query without terms: dict with keys (uint32,
    slot order = ascending key), w / c0 / c1 (float32, what the device is given), df (int64),
    tf (int64 [n, T]), dl (int64 [n])."""
    assert mutant is None or mutant in MUTANTS
    flat, offs = corpus
    n = len(offs) - 1
    lens = np.diff(offs)
    dl = lens if ngram == 1 or mutant == "dl_tokens" else np.maximum(lens - 1, 0)
    qt = query_terms(query, ngram)
    if qt.size == 0 or n == 0:
        return None
    keys, qf = np.unique(qt, return_counts=True)
    ck, cr = corpus_terms(corpus, ngram, cross_row=mutant == "cross_row")
    slot = np.searchsorted(keys, ck)
    slot[slot == len(keys)] = 0
    hit = keys[slot] == ck
    tf = np.zeros((n, len(keys)), np.int64)
    np.add.at(tf, (cr[hit], slot[hit]), 1)
    stat = np.ones(n, bool) if mutant != "stats_masked" or mask is None else np.asarray(mask, bool)
    N = int(stat.sum())
    df = (tf[stat] > 0).sum(axis=0).astype(np.int64)
    total = float(dl[stat].sum())
    if total == 0.0:
        return None
    avgdl = total / N
    if mutant == "rank_bm25_idf":
        idf = np.log((N - df + 0.5) / (df + 0.5))
    else:
        idf = np.log(1.0 + (N - df + 0.5) / (df + 0.5))
    if len(keys) > max_terms:
        keep = np.sort(np.lexsort((keys, -idf))[:max_terms])
        keys, qf, idf, df, tf = keys[keep], qf[keep], idf[keep], df[keep], tf[:, keep]
    w = (qf * (k1 + 1.0) * idf).astype(np.float32)
    return {"keys": keys.astype(np.uint32), "w": w, "c0": np.float32(k1 * (1.0 - b)),
            "c1": np.float32(k1 * b / avgdl), "df": df, "tf": tf, "dl": dl.astype(np.int64), "n": n}


def bm25_rank(setup, mask=None, tie_high=False):
    """-> (ids int64, scores float64): every candidate, best first, in float64 from the fp32
    inputs of `setup`."""
    if setup is None:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    tf = setup["tf"].astype(np.float64)
    norm = np.float64(setup["c0"]) + np.float64(setup["c1"]) * setup["dl"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        part = setup["w"].astype(np.float64)[None, :] * tf / (tf + norm[:, None])
    score = np.where(tf > 0, part, 0.0).sum(axis=1)
    cand = setup["tf"].sum(axis=1) > 0
    if mask is not None:
        cand &= np.asarray(mask, bool)
    ids = np.flatnonzero(cand)
    order = np.lexsort((-ids if tie_high else ids, -score[ids]))
    return ids[order].astype(np.int64), score[ids][order]


def bm25_reference(rows_tokens, query_tokens, ngram, k1=K1, b=B, mask=None, mutant=None):
    """The full float64 ranking (ids, scores) of a query over rows (a list of id sequences or a
    packed corpus), or what one of the MUTANTS makes of it: rank_bm25's idf ln((N - df + 0.5) /
    (df + 0.5)) instead of Lucene's; dl counted in tokens for ngram 2; a bigram matched across a
    row boundary; N, avgdl and df over the masked rows only; ties to the higher id."""
    corpus = rows_tokens if isinstance(rows_tokens, tuple) else pack(rows_tokens)
    setup = bm25_setup(corpus, query_tokens, ngram, k1, b, mask, mutant)
    return bm25_rank(setup, mask, tie_high=mutant == "tie_high")


def rrf_reference(dense_ids, lexical_ids, weights=(0.5, 0.5), c=60, k=None, mutant=None):
    """LangChain's weighted_reciprocal_rank over two lists of row ids in float64 -> [(id, rrf)]:
    rank from 1 (the mutant rrf_rank0: from 0), a stable sort by rrf descending over the order
    "dense list, then the lexical rows not yet seen"."""
    first = 0 if mutant == "rrf_rank0" else 1
    score = {}
    for ids, wt in ((dense_ids, weights[0]), (lexical_ids, weights[1])):
        for rank, r in enumerate(ids, start=first):
            score[int(r)] = score.get(int(r), 0.0) + float(wt) / (rank + float(c))
    seen, order = set(), []
    for r in list(dense_ids) + list(lexical_ids):
        if int(r) not in seen:
            seen.add(int(r))
            order.append(int(r))
    order = sorted(order, key=lambda r: -score[r])  # sorted() is stable
    out = [(r, score[r]) for r in order]
    return out if k is None else out[:k]


# ------------------------------------------------------------------------ checker ----
class Tally:
    """Checked and ambiguous (near-tie) positions of one test."""

    def __init__(self):
        self.checked = 0
        self.ambiguous = 0

    def ok(self):
        return self.ambiguous <= AMBIGUOUS_CAP * max(1, self.checked)


def check_topk(got_ids, got_scores, ref_ids, ref_scores, k, n_terms, tally=None):
    """Failures (empty = pass) of a device result [k] against the full reference ranking:
    min(k, candidates) results then (-inf, -1) padding; no id twice; every score within
    score_tol(n_terms) relative of the reference's score of that id; every position holds
    the reference's id, except inside a near-tie group (module doc), where any member of the
    group passes."""
    got_ids = [int(i) for i in got_ids]
    got_scores = [float(s) for s in got_scores]
    ref_ids = np.asarray(ref_ids, np.int64)
    ref_scores = np.asarray(ref_scores, np.float64)
    fails = []
    if len(got_ids) != k or len(got_scores) != k:
        return ["result holds %d ids / %d scores, k = %d" % (len(got_ids), len(got_scores), k)]
    m = min(k, len(ref_ids))
    for p in range(m, k):
        if got_ids[p] != -1 or got_scores[p] != -np.inf:
            fails.append("position %d: (%r, %r) is not padding" % (p, got_scores[p], got_ids[p]))
    if len(set(got_ids[:m])) != m:
        fails.append("an id repeats: %r" % (got_ids[:m],))
    tol = score_tol(n_terms)
    where = {int(r): j for j, r in enumerate(ref_ids)}
    # links between reference positions p and p + 1: `near` = they differ by at most the bound but
    # not by exactly 0, `close` = near or exactly equal.  A near-tie group is a maximal run of
    # positions joined by close links that holds at least one near link: an exact tie next to a
    # near tie is part of the group (fp32 may round all of them to one score, and then the row
    # ids order them), an exact tie on its own is not and stays strict.
    top = ref_scores[:m + 1]
    d = np.abs(np.diff(top))
    scale = np.maximum(np.abs(top[:-1]), np.abs(top[1:]))
    near = (d > 0) & (d <= tol * scale)
    close = d <= tol * scale
    group = [None] * m  # (lo, hi) of the near-tie group of position p
    p = 0
    while p < m:
        hi = p
        while hi < len(close) and close[hi]:
            hi += 1
        if near[p:hi].any():
            for j in range(p, min(hi, m - 1) + 1):
                group[j] = (p, hi)
        p = hi + 1
    for p in range(m):
        g = got_ids[p]
        if g not in where:
            fails.append("position %d: id %d is no candidate" % (p, g))
            continue
        want = ref_scores[where[g]]
        if abs(got_scores[p] - want) > tol * abs(want):
            fails.append("position %d (id %d): score %.9g, reference %.9g (rel %.3g > %.3g)"
                         % (p, g, got_scores[p], want, abs(got_scores[p] - want) / abs(want), tol))
        if p and not (got_scores[p - 1] > got_scores[p] or (got_scores[p - 1] == got_scores[p] and got_ids[p - 1] < g)):
            fails.append("positions %d, %d: (%.9g, %d) before (%.9g, %d) is not (score desc, id asc)"
                         % (p - 1, p, got_scores[p - 1], got_ids[p - 1], got_scores[p], g))
        if tally is not None:
            tally.checked += 1
            tally.ambiguous += group[p] is not None
        if group[p] is None:
            if g != int(ref_ids[p]):
                fails.append("position %d: id %d, reference %d" % (p, g, int(ref_ids[p])))
        elif not group[p][0] <= where[g] <= group[p][1]:
            fails.append("position %d: id %d (reference place %d) is outside the near-tie group %d..%d"
                         % (p, g, where[g], group[p][0], group[p][1]))
    return fails


def bm25_fp32(setup, mask=None):
    """The device's arithmetic in numpy float32 (MQ_LEX_NORM / MQ_LEX_TERM: every operation
    rounded on its own, the terms with tf > 0 added in slot order) -> (ids, scores float32),
    best first."""
    if setup is None:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    f = np.float32
    tf = setup["tf"].astype(f)
    norm = setup["c0"] + setup["c1"] * setup["dl"].astype(f)
    score = np.zeros(tf.shape[0], f)
    for t in range(tf.shape[1]):
        with np.errstate(invalid="ignore", divide="ignore"):
            term = (setup["w"][t] * tf[:, t]) / (tf[:, t] + norm)
        score = np.where(tf[:, t] > 0, score + term.astype(f), score).astype(f)
    cand = setup["tf"].sum(axis=1) > 0
    if mask is not None:
        cand &= np.asarray(mask, bool)
    ids = np.flatnonzero(cand)
    order = np.lexsort((ids, -score[ids]))
    return ids[order].astype(np.int64), score[ids][order]
