"""Batched BM25 on the device: mq_lex_topk_batch / mq_lex_df_batch (lex_batch_kernel, K15)
through native.lex_topk_batch / lex_df_batch.  The oracle needs no tolerance: row j of a batch
must equal, bit for bit in scores and ids, what lex_topk (K14) returns for query j alone, and a
batched df must equal the reference's exactly.  Every row is held to the float64 reference of
tests/lexical_cases.py as well.  Shapes: row counts around the 16-, 32- and 64-row blocks of the
three builds (picked by the size of a group's key union: up to 128 / 256 / 512 keys), batches
around the 16-query group, unions past 512 keys, and a corpus on which every workgroup of the
768-workgroup grid walks at least two blocks; then `HipChroma`'s batch methods against its
single-query methods."""
import ctypes
import functools

import numpy as np
import pytest

import lexical_cases as lc
from mediquery_hip import _lib
from mediquery_hip.native import lex_batch_scratch_bytes, lex_df_batch, lex_topk, lex_topk_batch
from mediquery_hip import vectorstore
from mediquery_hip.vectorstore import HipChroma

pytestmark = pytest.mark.gpu

G, U = _lib.MQ_LEX_BATCH_GROUP, _lib.MQ_LEX_BATCH_UNION
GRID = 768  # workgroups of one batched scan


class _Dev:
    """A packed corpus on the device: the token tensor holds exactly n_tokens tokens."""

    def __init__(self, corpus):
        import torch
        self.dev = torch.device("cuda", 0)
        flat, offs = corpus
        self.corpus = corpus
        self.n = len(offs) - 1
        self.tokens = (torch.from_numpy(flat.view(np.int16).copy()).to(self.dev).view(torch.uint16) if flat.size
                       else torch.empty(0, dtype=torch.uint16, device=self.dev))
        self.offs = torch.from_numpy(offs).to(self.dev)

    def bits(self, mask):
        import torch
        if mask is None:
            return None
        m = np.concatenate([np.asarray(mask, bool), np.zeros(-self.n % 32, bool)])
        words = np.packbits(m, bitorder="little").view(np.int32) if m.size else np.zeros(1, np.int32)
        return torch.from_numpy(words.copy()).to(self.dev)


class _Query:
    """One query of a batch: its plan (keys, w: what both calls are given) and reference setup."""

    def __init__(self, setup, order=None):
        self.setup = setup
        if setup is None:
            self.keys, self.w = np.zeros(0, np.uint32), np.zeros(0, np.float32)
        else:
            order = np.arange(len(setup["keys"])) if order is None else order
            self.keys, self.w = setup["keys"][order].copy(), setup["w"][order].copy()


class _Bench:
    """A corpus with its queries; the single-call result of each (query, mask, k) is computed
    once, checked against float64 once, and then shared by every batch that holds the query."""

    def __init__(self, dev, ngram, tally):
        self.dev, self.ngram, self.tally = dev, ngram, tally
        self.c = None
        self.single = {}

    def query(self, tokens, order=None, max_terms=lc.MAX_TERMS):
        setup = lc.bm25_setup(self.dev.corpus, tokens, self.ngram, max_terms=max_terms)
        if setup is not None:
            c = (setup["c0"], setup["c1"])
            assert self.c is None or self.c == c  # c0, c1 belong to the corpus
            self.c = c
        return _Query(setup, order)

    def expect(self, q, mask_id, mask, k):
        """lex_topk of q alone -> (scores, ids) device tensors; no terms: padding."""
        import torch
        key = (id(q), mask_id, k)
        if key not in self.single:
            d = self.dev
            if q.keys.size == 0:
                s = torch.full((k,), -np.inf, dtype=torch.float32, device=d.dev)
                i = torch.full((k,), -1, dtype=torch.int64, device=d.dev)
            else:
                s, i = lex_topk(d.tokens, d.offs, self.ngram, q.keys, q.w, self.c[0], self.c[1], k, bits=d.bits(mask))
                ids, scores = lc.bm25_rank(q.setup, mask)
                fails = lc.check_topk(i.cpu().numpy(), s.cpu().numpy(), ids, scores, k, len(q.keys), self.tally)
                assert not fails, (self.ngram, k, fails[:4])
            self.single[key] = (s, i)
        return self.single[key]

    def check(self, batch, mask_id, mask, k, note=""):
        import torch
        d = self.dev
        s, i = lex_topk_batch(d.tokens, d.offs, self.ngram, [(q.keys, q.w) for q in batch], self.c[0], self.c[1], k,
                              bits=d.bits(mask))
        assert s.shape == (len(batch), k) and i.shape == (len(batch), k)
        want = [self.expect(q, mask_id, mask, k) for q in batch]
        ws, wi = torch.stack([x for x, _ in want]), torch.stack([x for _, x in want])
        if not (torch.equal(i, wi) and torch.equal(s, ws)):
            bad = [j for j in range(len(batch)) if not (torch.equal(i[j], wi[j]) and torch.equal(s[j], ws[j]))]
            j = bad[0]
            raise AssertionError((note, self.ngram, k, mask_id, "rows", bad[:8], "of", len(batch), len(batch[j].keys),
                                  i[j].tolist()[:6], wi[j].tolist()[:6], s[j].tolist()[:4], ws[j].tolist()[:4]))
        return s, i


def _masks(n, seed):
    rng = np.random.default_rng([seed, n])
    one = np.zeros(n, bool)
    one[int(rng.integers(0, n))] = True
    return rng.random(n) < 0.5, np.zeros(n, bool), one


@functools.lru_cache(maxsize=None)
def _zipf(n, vocab, seed):
    rows = lc.zipf_rows(n, vocab, seed)
    if not any(len(r) > 1 for r in rows):
        rows = [np.array([1000, 1001, 1000], np.uint16)] + list(rows[1:])
    return rows


def _pool(bench, rows, n, ngram):
    """Queries of 1, 2, 64 and 128 terms (repeated and absent terms), none, one no row holds,
    the 2-term one again, the 64-term one with its slots reversed, and two that share half
    their keys at different slots."""
    qs = {}
    for n_terms in (1, 2, 64, 128):
        qs[n_terms] = bench.query(lc.query_tokens(rows, n_terms, n_terms + n, ngram, repeat=2 if n_terms > 1 else 0,
                                                  absent=1 if n_terms > 2 else 0))
    empty = bench.query([])
    assert empty.setup is None
    nowhere = bench.query([9] if ngram == 1 else [9, 8])
    assert nowhere.setup["df"].tolist() == [0]
    twice = qs[2]
    rev = bench.query(lc.query_tokens(rows, 64, 64 + n, ngram, repeat=2, absent=1),
                      order=np.arange(len(qs[64].keys))[::-1])
    if ngram == 1:
        ids = np.unique(np.concatenate([np.asarray(r, np.int64) for r in rows]))[:12].tolist()
        ids = sorted(ids + list(range(20, 20 + 12 - len(ids))))
        a, b = bench.query(ids[:8]), bench.query(ids[4:12])
        assert a.keys[4:].tolist() == b.keys[:4].tolist()  # the shared half: slots 4..7 and 0..3
    else:
        long_ = max(rows, key=len)
        a, b = bench.query(list(long_[:10]) + [5]), bench.query([4] + list(long_[5:15]))
    return [qs[1], qs[2], qs[64], empty, qs[128], nowhere, twice, rev, a, b]


# the three builds' rows per block - 1 / + 0 / + 1 / x 2 + 1, and the single-query suite's sizes
SIZES = sorted({1, 63, 64, 65, 129, 1000} | {r + d for r in (16, 32, 64) for d in (-1, 0, 1)}
               | {2 * r + 1 for r in (16, 32, 64)})


@pytest.mark.parametrize("ngram", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_batch_rows_equal_single_calls_zipf(require_gpu, n, ngram):
    """Batches of 1, 2, G - 1, G, G + 1 and 70 queries drawn from the pool (so that groups are
    cut by the query count and by the union size, and small unions take the 64- and 32-row
    builds), no mask, a random one, all zero, one bit, k 1, 5 and 64."""
    tally = lc.Tally()
    for vocab in (12, 60, 2000):
        rows = _zipf(n, vocab, 11)
        bench = _Bench(_Dev(lc.pack(rows)), ngram, tally)
        pool = _pool(bench, rows, n, ngram)
        rand, zero, one = _masks(n, vocab)
        cases = [("none", None, 5), ("rand", rand, 64), ("zero", zero, 1), ("one", one, 5), ("none", None, 64),
                 ("rand", rand, 1)]
        small = [pool[0], pool[1], pool[3], pool[5], pool[6], pool[8], pool[9]]  # a union of a few keys
        batches = [[pool[0]], [pool[4]], [pool[2], pool[4]], small]
        batches += [[pool[(3 * j + size) % len(pool)] for j in range(size)] for size in (2, G - 1, G, G + 1, 70)]
        batches += [[small[j % len(small)] for j in range(G + 1)]]
        for mask_id, mask, k in cases:
            for batch in batches:
                bench.check(batch, mask_id, mask, k, (n, vocab, len(batch)))
    assert tally.ok(), (tally.ambiguous, tally.checked)


@pytest.mark.parametrize("ngram", [1, 2])
def test_group_cuts_by_union_and_by_count(require_gpu, ngram):
    """Five queries of 128 pairwise disjoint terms (a union of 640 > U) and 40 one-term queries
    (> G) give the single calls' rows; so does a batch that fills a group's term slots (16
    queries of 128 terms over one union of 256 keys)."""
    n = 1000
    rows = _zipf(n, 2000, 11)
    tally = lc.Tally()
    bench = _Bench(_Dev(lc.pack(rows)), ngram, tally)
    walk = lc.query_tokens(rows, 5 * 128 + 40, 3, ngram)
    terms = lc.query_terms(walk, ngram)
    _, first = np.unique(terms, return_index=True)
    distinct = terms[np.sort(first)]
    assert distinct.size >= 5 * 128 + 40

    full = lc.bm25_setup(bench.dev.corpus, walk, ngram, max_terms=10 ** 6)
    bench.c = (full["c0"], full["c1"])

    def by_keys(keys):
        """A query holding exactly these term keys (the walk's weights for them)."""
        pick = np.searchsorted(full["keys"], np.sort(keys))
        assert np.array_equal(full["keys"][pick], np.sort(keys))
        return _Query(dict(full, keys=full["keys"][pick], w=full["w"][pick], df=full["df"][pick],
                           tf=full["tf"][:, pick]))

    big = [by_keys(distinct[j * 128:(j + 1) * 128]) for j in range(5)]
    assert len(np.unique(np.concatenate([q.keys for q in big]))) == 640 > U
    ones = [by_keys(distinct[640 + j:641 + j]) for j in range(40)]
    assert len(ones) > G
    halves = [by_keys(distinct[:256][(j % 2) * 128:(j % 2) * 128 + 128]) for j in range(2)]
    rand = _masks(n, 1)[0]
    for mask_id, mask, k in (("none", None, 64), ("rand", rand, 5), ("none", None, 1)):
        bench.check(big, mask_id, mask, k, "union")
        bench.check(ones, mask_id, mask, k, "count")
        bench.check(ones[:7] + big[:2] + ones[7:] + big[2:], mask_id, mask, k, "mixed")
        bench.check([halves[j % 2] for j in range(G)], mask_id, mask, k, "term slots")
    assert tally.ok(), (tally.ambiguous, tally.checked)


@pytest.mark.parametrize("ngram", [1, 2])
def test_a_row_does_not_depend_on_the_rest_of_the_batch(require_gpu, ngram):
    """The batch reversed, and the batch with a 128-term query inserted in the middle, give every
    original query bitwise the same row (checked against the shared single-call rows, and the
    two batch results against each other)."""
    import torch
    n = 129
    rows = _zipf(n, 60, 11)
    tally = lc.Tally()
    bench = _Bench(_Dev(lc.pack(rows)), ngram, tally)
    pool = _pool(bench, rows, n, ngram)
    batch = [pool[(5 * j) % len(pool)] for j in range(G + 3)]
    extra = bench.query(lc.query_tokens(rows, 128, 999, ngram, repeat=1, absent=1))
    mid = len(batch) // 2
    for mask_id, mask, k in (("none", None, 64), ("rand", _masks(n, 2)[0], 5)):
        s0, i0 = bench.check(batch, mask_id, mask, k, "as is")
        s1, i1 = bench.check(batch[::-1], mask_id, mask, k, "reversed")
        s2, i2 = bench.check(batch[:mid] + [extra] + batch[mid:], mask_id, mask, k, "inserted")
        assert torch.equal(s1.flip(0), s0) and torch.equal(i1.flip(0), i0)
        keep = [j for j in range(len(batch) + 1) if j != mid]
        assert torch.equal(s2[keep], s0) and torch.equal(i2[keep], i0)
    assert tally.ok(), (tally.ambiguous, tally.checked)


# ------------------------------------------------- more blocks than workgroups ----
# A batched scan runs at most 768 workgroups over blocks of 64, 32 or 16 rows: past 2 * 768 * 64
# rows every workgroup of every build walks at least two blocks (the 16-row build eight).
BIG_N = 2 * GRID * 64 + 77


@functools.lru_cache(maxsize=None)
def _big_corpus():
    """BIG_N rows of 0..8 tokens over 30 ids; every seventh row copied into its neighbour, and
    every fifth row of the first 768 * 64 copied one grid of 64-row blocks and one grid of 16-row
    blocks up, where the same workgroup meets it in a later block (exact ties across blocks)."""
    rng = np.random.default_rng(78)
    p = 1.0 / np.arange(1, 31)
    p /= p.sum()
    lens = rng.integers(0, 9, BIG_N)
    flat = (1000 + rng.choice(30, int(lens.sum()), p=p)).astype(np.uint16)
    offs = np.zeros(BIG_N + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    rows = [flat[offs[r]:offs[r + 1]] for r in range(BIG_N)]
    for r in range(0, BIG_N - 1, 7):
        rows[r + 1] = rows[r]
    for r in range(0, GRID * 64, 5):
        rows[r + GRID * 64] = rows[r]
        rows[r + GRID * 16] = rows[r]
    return lc.pack(rows)


@functools.lru_cache(maxsize=None)
def _big_dev():
    return _Dev(_big_corpus())


def _big_queries(corpus, ngram):
    """The token lists of the G + 1 queries of the several-blocks test, and its sparse mask."""
    flat, offs = corpus
    head = [flat[offs[r]:offs[r + 1]] for r in range(0, 4000)]
    queries = [lc.query_tokens(head, 4 + 2 * j, 50 + j, ngram, repeat=1, absent=1) for j in range(G + 1)]
    return queries, np.arange(BIG_N) % 4099 == 0


@pytest.mark.parametrize("ngram", [1, 2])
def test_workgroups_walk_several_blocks(require_gpu, ngram):
    """G + 1 queries at BIG_N rows: unigram unions stay below 128 keys (the 64-row build), the
    bigram group's union is larger (the 32- or 16-row build), the last query runs alone; without
    a mask, with one that admits every 4099th row, k 64 and 1."""
    dev = _big_dev()
    queries, sparse = _big_queries(dev.corpus, ngram)
    tally = lc.Tally()
    bench = _Bench(dev, ngram, tally)
    batch = [bench.query(q) for q in queries]
    if ngram == 2:
        assert len(np.unique(np.concatenate([q.keys for q in batch[:G]]))) > 128
    for mask_id, mask, k in (("none", None, 64), ("sparse", sparse, 64), ("none", None, 1)):
        bench.check(batch, mask_id, mask, k, "big")
    assert tally.ok(), (tally.ambiguous, tally.checked)


@pytest.mark.parametrize("ngram", [1, 2])
def test_df_batch_equals_reference(require_gpu, ngram):
    """1, 128, U, U + 1 and 3 U distinct keys, absent ones included, in shuffled order, equal the
    reference's df exactly; n = 0 gives zeros."""
    n = 1000
    rows = _zipf(n, 2000, 11)
    dev = _Dev(lc.pack(rows))
    walk = lc.query_tokens(rows, 3 * U, 5, ngram, absent=1)
    setup = lc.bm25_setup(dev.corpus, walk, ngram, max_terms=10 ** 6)
    assert len(setup["keys"]) >= 3 * U and setup["df"].min() == 0 and setup["df"].max() > 1
    rng = np.random.default_rng(ngram)
    for count in (1, 128, U, U + 1, 3 * U):
        pick = rng.permutation(len(setup["keys"]))[:count]
        absent = int(np.argmin(setup["df"]))
        if count > 1 and absent not in pick:
            pick[0] = absent  # a key no row holds is always among them
        assert len(pick) == count
        got = lex_df_batch(dev.tokens, dev.offs, ngram, setup["keys"][pick])
        assert got.dtype == np.int64 and np.array_equal(got, setup["df"][pick]), (count, np.flatnonzero(got != setup["df"][pick])[:5])
    none = _Dev((np.zeros(0, np.uint16), np.zeros(1, np.int64)))
    assert lex_df_batch(none.tokens, none.offs, ngram, setup["keys"][:U + 3]).tolist() == [0] * (U + 3)
    empty_rows = _Dev(lc.pack([np.zeros(0, np.uint16)] * 70))
    assert lex_df_batch(empty_rows.tokens, empty_rows.offs, ngram, setup["keys"][:5]).tolist() == [0] * 5
    with pytest.raises(ValueError, match="distinct"):
        lex_df_batch(dev.tokens, dev.offs, ngram, np.array([9, 10, 9], np.uint32))
    with pytest.raises(ValueError, match="at least 1"):
        lex_df_batch(dev.tokens, dev.offs, ngram, np.zeros(0, np.uint32))


def test_host_outputs_empty_batch_and_empty_corpus(require_gpu):
    """io_on_device = 0 stages the rows in scratch and copies them to host arrays: the same bits
    as the device-output call (a batch of several groups, padding rows included); nq = 0 and
    n = 0."""
    import torch
    rows = _zipf(1000, 60, 11)
    tally = lc.Tally()
    bench = _Bench(_Dev(lc.pack(rows)), 1, tally)
    pool = _pool(bench, rows, 1000, 1)
    batch = [pool[(3 * j) % len(pool)] for j in range(2 * G + 5)]
    d = bench.dev
    for k in (64, 7):
        s, i = bench.check(batch, "none", None, k, "device outputs")
        term_start = np.zeros(len(batch) + 1, np.int64)
        np.cumsum([len(q.keys) for q in batch], out=term_start[1:])
        keys, w = np.concatenate([q.keys for q in batch]), np.concatenate([q.w for q in batch])
        scratch = torch.empty(lex_batch_scratch_bytes(d.n, len(batch), keys.size, k), dtype=torch.uint8, device=d.dev)
        hs, hi = np.full((len(batch), k), 7.0, np.float32), np.full((len(batch), k), 7, np.int64)
        _lib.call("mq_lex_topk_batch", _lib.ptr(d.tokens), d.tokens.numel(), _lib.ptr(d.offs), d.n, 1, len(batch),
                  _lib.ptr(term_start), _lib.ptr(keys), _lib.ptr(w), ctypes.c_float(float(bench.c[0])),
                  ctypes.c_float(float(bench.c[1])), None, k, _lib.ptr(hs), _lib.ptr(hi), 0, _lib.ptr(scratch),
                  _lib.stream_handle(None))
        assert np.array_equal(hi, i.cpu().numpy()) and hs.tobytes() == s.cpu().numpy().tobytes()
    s, i = lex_topk_batch(d.tokens, d.offs, 1, [], bench.c[0], bench.c[1], 5)
    assert s.shape == (0, 5) and i.shape == (0, 5)
    assert _lib.call("mq_lex_topk_batch", _lib.ptr(d.tokens), d.tokens.numel(), _lib.ptr(d.offs), d.n, 1, 0, None, None,
                     None, ctypes.c_float(0.3), ctypes.c_float(0.01), None, 5, None, None, 1, None,
                     _lib.stream_handle(None)) == _lib.MQ_OK
    none = _Dev((np.zeros(0, np.uint16), np.zeros(1, np.int64)))
    s, i = lex_topk_batch(none.tokens, none.offs, 1, [(q.keys, q.w) for q in batch[:G + 1]], 0.3, 0.01, 4)
    assert (i.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all() and s.shape == (G + 1, 4)
    with pytest.raises(ValueError, match="distinct within a query"):
        lex_topk_batch(d.tokens, d.offs, 1, [(np.array([9], np.uint32), np.ones(1, np.float32)),
                                             (np.array([8, 8], np.uint32), np.ones(2, np.float32))], 0.3, 0.01, 4)
    with pytest.raises(ValueError, match="0..128 terms"):
        lex_topk_batch(d.tokens, d.offs, 1, [(np.arange(129, dtype=np.uint32), np.ones(129, np.float32))], 0.3, 0.01, 4)
    assert tally.ok(), (tally.ambiguous, tally.checked)


# ------------------------------------------------------------------ through the store ----
@functools.lru_cache(maxsize=None)
def _embeddings():
    from mediquery_hip.config import BertConfig
    from mediquery_hip.embeddings import HipBertEmbeddings
    return HipBertEmbeddings(synthetic=True, config=BertConfig(layers=2))


def _texts(n, seed=0):
    """Short rows over 40 characters (frequent terms), some empty or blank, some copied."""
    rng = np.random.default_rng(seed)
    chars = [chr(0x4E00 + 37 * j) for j in range(40)]
    p = 1.0 / np.arange(1, 41)
    p /= p.sum()
    out = ["".join(rng.choice(chars, int(rng.integers(0, 40)), p=p)) for _ in range(n)]
    out[3], out[4] = "", "   "
    for r in range(0, n - 1, 7):
        out[r + 1] = out[r]
    return out


def _store(texts, ngram):
    store = HipChroma(embedding_function=_embeddings(), auto_persist=False, lexical_ngram=ngram)
    store.add_texts(texts, metadatas=[{"part": r % 3, "r": r} for r in range(len(texts))],
                    ids=["id%d" % r for r in range(len(texts))])
    return store


def _flat(results):
    return [[(d.id, d.page_content, x) for d, x in hits] for hits in results]


def _check_store(store, qs, monkeypatch):
    """The batch methods against the single-query methods (lexical: ids, documents and scores
    with ==) and against themselves on the looped path (hybrid: the same dense rows go into
    both, so the fused lists and rrf values are equal exactly)."""
    sub = qs[1][:1]
    for kw in ({}, {"filter": {"part": 1}}, {"where_document": {"$contains": sub}},
               {"filter": {"part": {"$ne": 0}}, "where_document": {"$contains": sub}}):
        for k in (4, 64):
            got = store.lexical_search_batch_with_score(qs, k=k, **kw)
            assert _flat(got) == _flat([store.lexical_search_with_score(q, k=k, **kw) for q in qs]), (kw, k)
            assert [[d.id for d in hits] for hits in store.lexical_search_batch(qs, k=k, **kw)] == \
                [[d.id for d, _ in hits] for hits in got]
        assert any(len(hits) for hits in got)
        hyb = store._hybrid(qs, 5, 20, (0.4, 0.6), 60, kw.get("filter"), kw.get("where_document"))
        with monkeypatch.context() as m:
            m.setattr(vectorstore, "LEX_BATCH_MIN", 10 ** 9)  # the looped path: one plan / topk a query
            looped = store._hybrid(qs, 5, 20, (0.4, 0.6), 60, kw.get("filter"), kw.get("where_document"))
        assert _flat(hyb) == _flat(looped), kw
        assert [[d.id for d in hits] for hits in store.hybrid_search_batch(qs, k=5, fetch_k=20, weights=(0.4, 0.6), **kw)] \
            == [[d.id for d, _ in hits] for hits in hyb]
        # each hybrid row is the fusion of the batch's dense row with the single query's lexical row
        rows = {i: r for r, i in enumerate(store._ids)}
        dense = store.similarity_search_batch(qs, k=20, **kw)
        for q, got_q, dq in zip(qs, hyb, dense):
            lex = [rows[d.id] for d in store.lexical_search(q, k=20, **kw)]
            want = lc.rrf_reference([rows[d.id] for d in dq], lex, (0.4, 0.6), 60, 5)
            assert [(rows[d.id], x) for d, x in got_q] == want, (q, kw)


@pytest.mark.parametrize("ngram", [1, 2])
def test_store_batch_methods_equal_single_queries(require_gpu, monkeypatch, ngram):
    texts = _texts(300, seed=5)
    store = _store(texts[:250], ngram)
    long_ = [t for t in texts if len(t) >= 12]
    qs = [long_[0][:6], long_[1][2:9] + long_[2][:3], "", long_[3], long_[0][:6], "  \n ", long_[4][:30],
          long_[5][:2]] + [t[:12] for t in long_[6:6 + G + 2]]
    _check_store(store, qs, monkeypatch)
    got = store.lexical_search_batch(qs, k=4)
    assert got[2] == [] and got[5] == [] and got[0] and [d.id for d in got[0]] == [d.id for d in got[4]]
    assert store.hybrid_search_batch(["", qs[0]], k=3)[1]
    first = store._lex_mirror
    assert first.batch_scratch is not None and first.df
    store.add_texts(texts[250:], metadatas=[{"part": r % 3, "r": r} for r in range(250, 300)],
                    ids=["id%d" % r for r in range(250, 300)])
    _check_store(store, qs, monkeypatch)
    assert store._lex_mirror is first and first.n == 300  # extended, not rebuilt
    store.delete(["id5", "id20", "id260"])
    _check_store(store, qs, monkeypatch)
    assert store._lex_mirror is not first and store._lex_mirror.n == 297


def test_store_batches_do_not_call_the_single_query_kernels(require_gpu, monkeypatch):
    """Two queries already take the batch path: with the single-query wrappers replaced by ones
    that raise, the batch methods still answer (and one query alone does raise)."""
    texts = _texts(200, seed=9)
    store = _store(texts, 1)
    long_ = [t for t in texts if len(t) >= 12]
    want = [[d.id for d in store.lexical_search(q, k=5)] for q in long_[:2]]

    def boom(*a, **kw):
        raise AssertionError("the single-query call ran")

    monkeypatch.setattr(vectorstore, "lex_topk", boom)
    monkeypatch.setattr(vectorstore, "lex_df", boom)
    store._lex_mirror.df.clear()  # the df values must come from the batch call too
    assert [[d.id for d in hits] for hits in store.lexical_search_batch(long_[:2], k=5)] == want
    assert all(len(hits) == 5 for hits in store.hybrid_search_batch(long_[2:4], k=5))
    with pytest.raises(AssertionError, match="single-query call ran"):
        store.lexical_search_batch(long_[4:5], k=5)
