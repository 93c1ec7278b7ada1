"""BM25 lexical retrieval on the device: mq_lex_df / mq_lex_topk (lex_scan_kernel, K14) through
native.lex_df / lex_topk against the float64 reference of tests/lexical_cases.py at the smallest
shapes that can break the walk - row counts around the 64-row block, rows of 0..300 tokens,
frequent (Zipf over 12-60 ids) and rare (2000 ids) terms, exact score ties, every row start and
length modulo the 8-token lane chunk, bigrams over chunk / wave / workgroup-step and row
boundaries, masks, k up to 64 - and `HipChroma.lexical_search*` / `hybrid_search*` against the
same reference on the store's own texts.  df must equal the reference exactly; scores and order
are held to the derived bounds of lexical_cases.py."""
import functools
import os

import numpy as np
import pytest

import lexical_cases as lc
from mediquery_hip import _lib
from mediquery_hip.native import lex_df, lex_topk
from mediquery_hip.vectorstore import HipChroma, body_tokens

pytestmark = pytest.mark.gpu


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
        assert self.tokens.numel() == flat.size == offs[-1]
        self.offs = torch.from_numpy(offs).to(self.dev)

    def bits(self, mask):
        import torch
        if mask is None:
            return None
        m = np.concatenate([np.asarray(mask, bool), np.zeros(-self.n % 32, bool)])
        words = np.packbits(m, bitorder="little").view(np.int32) if m.size else np.zeros(1, np.int32)
        return torch.from_numpy(words.copy()).to(self.dev)

    def check(self, query, ngram, cases, tally, note=""):
        """One query: df equal to the reference, then each (mask, k) of `cases` through
        lex_topk against the reference ranking.  -> the reference setup."""
        setup = lc.bm25_setup(self.corpus, query, ngram)
        assert setup is not None, note
        keys = setup["keys"]
        df = lex_df(self.tokens, self.offs, ngram, keys)
        assert np.array_equal(df, setup["df"]), (note, np.flatnonzero(df != setup["df"])[:5], df[:5], setup["df"][:5])
        for mask, k in cases:
            ids, scores = lc.bm25_rank(setup, mask)
            s, i = lex_topk(self.tokens, self.offs, ngram, keys, setup["w"], setup["c0"], setup["c1"], k,
                            bits=self.bits(mask))
            fails = lc.check_topk(i.cpu().numpy(), s.cpu().numpy(), ids, scores, k, len(keys), tally)
            assert not fails, (note, ngram, k, None if mask is None else int(np.sum(mask)), fails[:4])
        return setup


def _masks(n, seed):
    rng = np.random.default_rng([seed, n])
    one = np.zeros(n, bool)
    one[int(rng.integers(0, n))] = True
    return rng.random(n) < 0.5, np.zeros(n, bool), one


@functools.lru_cache(maxsize=None)
def _zipf(n, vocab, seed):
    return lc.zipf_rows(n, vocab, seed)


@pytest.mark.parametrize("ngram", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000, 4097])
def test_kernel_matches_reference_zipf(require_gpu, n, ngram):
    """Rows of 0..300 tokens, every seventh copied into its neighbour; frequent terms (Zipf over
    12 / 60 ids) and rare ones (2000 ids); 1, 2, 64 and 128 query terms with repeated (qf = 2)
    and absent (df = 0) terms; no mask, a random one, all zero, one bit; k 1, 5, 64."""
    tally = lc.Tally()
    for vocab in (12, 60, 2000):
        rows = _zipf(n, vocab, 11)
        if not any(len(r) > 1 for r in rows):
            rows = [np.array([1000, 1001, 1000], np.uint16)] + list(rows[1:])
        dev = _Dev(lc.pack(rows))
        rand, zero, one = _masks(n, vocab)
        for n_terms in (1, 2, 64, 128):
            q = lc.query_tokens(rows, n_terms, n_terms + n, ngram, repeat=2 if n_terms > 1 else 0,
                                absent=1 if n_terms > 2 else 0)
            cases = [(None, 5), (rand, 64), (zero, 1), (one, 5), (None, 64), (rand, 1)]
            setup = dev.check(q, ngram, cases, tally, (n, vocab, n_terms))
            if n_terms > 2:
                assert setup["df"].min() == 0 and (setup["w"] > 0).all()
                if vocab == 12 and ngram == 1:
                    assert len(setup["keys"]) == n_terms  # the absent ids fill up to n_terms
    assert tally.ok(), (tally.ambiguous, tally.checked)


def _aligned_rows(rng, vocab):
    """A row of each length 0, 1, 7, 8, 9 starting at every token offset modulo 8, behind
    fillers of 0..15 tokens; ids 500 / 501 are the first / last token of some rows only."""
    rows, at = [], 0
    for start in range(8):
        for L in (0, 1, 7, 8, 9):
            fill = (start - at) % 8 + 8 * int(rng.integers(0, 2))
            rows.append(1000 + rng.integers(0, vocab, fill))
            row = 1000 + rng.integers(0, vocab, L)
            if L >= 7:
                row[0], row[-1] = 500, 501
            elif L == 1:
                row[0] = 500 if start % 2 else 501
            rows.append(row)
            at += fill + L
            assert (at - L) % 8 == start
    if at % 8 == 0:
        rows.append(np.array([1000, 500, 1001]))
    return [np.asarray(r, np.uint16) for r in rows]


@pytest.mark.parametrize("ngram", [1, 2])
def test_rows_at_every_offset_and_first_last_tokens(require_gpu, ngram):
    """Every row start modulo the 8-token lane chunk with row lengths 0, 1, 7, 8, 9; query terms
    that are the first and the last token of rows; a blob whose length is no multiple of 8 in
    a tensor of exactly that size."""
    rng = np.random.default_rng(21)
    tally = lc.Tally()
    for vocab in (3, 6):
        rows = _aligned_rows(rng, vocab)
        corpus = lc.pack(rows)
        assert corpus[1][-1] % 8 != 0
        dev = _Dev(corpus)
        n = dev.n
        rand, zero, one = _masks(n, vocab)
        if ngram == 1:
            queries = [[500, 501], [500], [501, 501, 1000], list(range(1000, 1000 + vocab)) + [500, 501, 9]]
        else:
            firsts = sorted({(500, int(r[1])) for r in rows if len(r) >= 7})
            lasts = sorted({(int(r[-2]), 501) for r in rows if len(r) >= 7})
            queries = [list(firsts[0]), list(lasts[0]), list(firsts[-1]) + [9] + list(lasts[-1]),
                       [x for pr in firsts + lasts for x in pr] + [1000, 1001, 1000]]
        for q in queries:
            dev.check(q, ngram, [(None, 64), (rand, 5), (one, 1), (zero, 5), (None, 1)], tally, (vocab, q[:6]))
    assert tally.ok(), (tally.ambiguous, tally.checked)


def test_bigram_over_chunk_wave_step_and_row_boundaries(require_gpu):
    """The pair (600, 601) planted so that its two tokens fall on either side of a lane's
    8-token chunk, of a 64-lane wave (512 tokens), of the workgroup's step (2048 tokens) and of a
    64-row block: each must match.  The same two ids as the last token of one row and the first
    of the next must not.  The first row is longer than two steps of the walk."""
    rng = np.random.default_rng(4)
    long_row = 1000 + rng.integers(0, 5, 5000)
    for p in (8, 24, 512, 2048, 4096, 4608):
        long_row[p - 1], long_row[p] = 600, 601
    rows = [long_row]
    rows.append(np.r_[1000 + rng.integers(0, 5, 40), 600])   # ends with 600 ...
    rows.append(np.r_[601, 1000 + rng.integers(0, 5, 30)])   # ... and the next starts with 601: no pair
    rows.append(np.array([600]))
    rows.append(np.array([601]))
    rows.append(np.zeros(0, np.int64))
    rows.append(np.array([600, 601]))                         # the whole row is the pair
    while len(rows) < 64:
        rows.append(1000 + rng.integers(0, 5, int(rng.integers(0, 20))))
    rows[63] = np.r_[1000 + rng.integers(0, 5, 9), 600]       # the block's last row ends with 600,
    rows.append(np.r_[601, 600, 601, 1000])                   # the next block's first starts with 601
    rows = [np.asarray(r, np.uint16) for r in rows]
    dev = _Dev(lc.pack(rows))
    tally = lc.Tally()
    setup = dev.check([600, 601], 2, [(None, 64), (None, 1)], tally, "planted")
    assert setup["df"].tolist() == [3]
    assert setup["tf"][:, 0][[0, 1, 2, 3, 4, 6, 63, 64]].tolist() == [6, 0, 0, 0, 0, 1, 0, 1]
    dev.check([600, 601, 600], 2, [(None, 64)], tally, "both orders")
    dev.check([600, 601, 1000, 1001, 1002, 1003], 1, [(None, 64)], tally, "unigrams of the long row")
    assert tally.ok(), (tally.ambiguous, tally.checked)


@pytest.mark.parametrize("ngram", [1, 2])
def test_identical_rows_come_back_in_id_order(require_gpu, ngram):
    """All rows identical: every score is bitwise equal, so the ids are 0 .. k - 1 (more than 64
    equal-score rows spread over several blocks and workgroups); with a mask, the admitted ids
    in order."""
    row = np.array([1000, 1001, 1002, 1001, 1000, 1003, 1001], np.uint16)
    n = 300
    dev = _Dev(lc.pack([row] * n))
    setup = lc.bm25_setup(dev.corpus, [1001, 1000, 1003], ngram)
    assert setup["df"].tolist() == [n] * len(setup["keys"])
    assert np.array_equal(lex_df(dev.tokens, dev.offs, ngram, setup["keys"]), setup["df"])
    mask = np.random.default_rng(0).random(n) < 0.3
    for m, k in ((None, 1), (None, 5), (None, 64), (mask, 64)):
        s, i = lex_topk(dev.tokens, dev.offs, ngram, setup["keys"], setup["w"], setup["c0"], setup["c1"], k,
                        bits=dev.bits(m))
        want = (np.arange(n) if m is None else np.flatnonzero(m))[:k]
        assert i.cpu().numpy().tolist() == want.tolist()
        s = s.cpu().numpy()
        assert np.all(s == s[0]) and s[0] > 0


def test_fewer_matches_than_k_pads_and_empty_corpora(require_gpu):
    import torch
    rows = _zipf(1000, 2000, 11)
    dev = _Dev(lc.pack(rows))
    flat = dev.corpus[0]
    ids, counts = np.unique(flat, return_counts=True)
    rare = int(ids[np.argmin(counts)])
    tally = lc.Tally()
    setup = dev.check([rare], 1, [(None, 64), (None, 5)], tally, "rare")
    assert 1 <= setup["df"][0] < 5
    s, i = lex_topk(dev.tokens, dev.offs, 1, setup["keys"], setup["w"], setup["c0"], setup["c1"], 64)
    i, s = i.cpu().numpy(), s.cpu().numpy()
    m = int(setup["df"][0])
    assert (i[m:] == -1).all() and np.isneginf(s[m:]).all() and (i[:m] >= 0).all()
    # a term no row holds: padding only; zero-length rows only; no rows at all
    s, i = lex_topk(dev.tokens, dev.offs, 1, np.array([9], np.uint32), np.ones(1, np.float32), 0.3, 0.01, 5)
    assert i.cpu().tolist() == [-1] * 5 and np.isneginf(s.cpu().numpy()).all()
    empty_rows = _Dev(lc.pack([np.zeros(0, np.uint16)] * 70))
    assert lex_df(empty_rows.tokens, empty_rows.offs, 2, np.array([9, 10], np.uint32)).tolist() == [0, 0]
    s, i = lex_topk(empty_rows.tokens, empty_rows.offs, 1, np.array([9], np.uint32), np.ones(1, np.float32), 0.3,
                    0.01, 3)
    assert i.cpu().tolist() == [-1] * 3
    none = _Dev((np.zeros(0, np.uint16), np.zeros(1, np.int64)))
    assert lex_df(none.tokens, none.offs, 1, np.array([9], np.uint32)).tolist() == [0]
    s, i = lex_topk(none.tokens, none.offs, 1, np.array([9], np.uint32), np.ones(1, np.float32), 0.3, 0.01, 4)
    assert i.cpu().tolist() == [-1] * 4 and np.isneginf(s.cpu().numpy()).all()
    with pytest.raises(ValueError, match="distinct"):
        lex_df(dev.tokens, dev.offs, 1, np.array([9, 9], np.uint32))
    with pytest.raises(ValueError, match="uint16"):
        lex_df(dev.tokens.view(torch.int16), dev.offs, 1, np.array([9], np.uint32))
    with pytest.raises(ValueError, match="1..128 terms"):
        lex_df(dev.tokens, dev.offs, 1, np.arange(129, dtype=np.uint32))


# ------------------------------------------------------------------ through the store ----
@functools.lru_cache(maxsize=None)
def _embeddings():
    from mediquery_hip.config import BertConfig
    from mediquery_hip.embeddings import HipBertEmbeddings
    return HipBertEmbeddings(synthetic=True, config=BertConfig(layers=2))


def _medical_texts(golden):
    from oracle.parse import parse_custom_format
    return [r["page_content"] for r in parse_custom_format(os.path.join(golden, "medical_data.txt"))]


def _synthetic_texts(n, seed=0):
    """Short Chinese-like rows over 40 characters (frequent terms), some empty or blank."""
    rng = np.random.default_rng(seed)
    chars = [chr(0x4E00 + 37 * j) for j in range(40)]
    p = 1.0 / np.arange(1, 41)
    p /= p.sum()
    out = ["".join(rng.choice(chars, int(rng.integers(0, 40)), p=p)) for _ in range(n)]
    out[3], out[4] = "", "   "
    for r in range(0, n - 1, 7):
        out[r + 1] = out[r]
    return out


def _store(texts, ngram, **kw):
    emb = _embeddings()
    store = HipChroma(embedding_function=emb, auto_persist=False, lexical_ngram=ngram, **kw)
    store.add_texts(texts, metadatas=[{"part": r % 3, "r": r} for r in range(len(texts))],
                    ids=["id%d" % r for r in range(len(texts))])
    return store


def _store_reference(store, query, ngram, mask=None):
    """The reference over the store's own texts, tokenised as the store tokenises them."""
    tok = store._lex_tok()
    flat, lens = body_tokens(tok, store._texts)
    offs = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    q, _ = body_tokens(tok, [query])
    setup = lc.bm25_setup((flat, offs), q.tolist(), ngram)
    ids, scores = lc.bm25_rank(setup, mask)
    return ids, scores, (0 if setup is None else len(setup["keys"]))


def _check_store(store, query, ngram, k, tally, mask=None, **kw):
    ids, scores, n_t = _store_reference(store, query, ngram, mask)
    hits = store.lexical_search_with_score(query, k=k, **kw)
    kk = min(k, len(store))
    assert len(hits) == min(kk, len(ids)), (query, len(hits), len(ids))
    got_i = [int(d.metadata["r_now"]) for d, _ in hits] + [-1] * (kk - len(hits))
    got_s = [x for _, x in hits] + [-np.inf] * (kk - len(hits))
    fails = lc.check_topk(got_i, got_s, ids, scores, kk, n_t, tally)
    assert not fails, (query, fails[:4])
    assert [d.page_content for d in store.lexical_search(query, k=k, **kw)] == [d.page_content for d, _ in hits]
    return hits


def _number_rows(store):
    for r, m in enumerate(store._metas):  # the current row of every document, for the checks
        m["r_now"] = r


@pytest.mark.parametrize("ngram", [1, 2])
def test_store_lexical_search_matches_reference(require_gpu, golden, ngram):
    tally = lc.Tally()
    for texts, queries in ((_medical_texts(golden), ["二甲双胍的剂量", "糖尿病", "慢性病有几种？", "低密度脂蛋白 LDL", "运动"]),
                           (_synthetic_texts(500), None)):
        store = _store(texts, ngram)
        _number_rows(store)
        long_ = [t for t in texts if len(t) >= 12]
        queries = queries or [long_[0][:6], long_[1][2:9] + long_[2][:3], long_[3]]
        for q in queries:
            for k in (1, 4, 64):
                _check_store(store, q, ngram, k, tally)
        assert store._lex_mirror.n == len(texts) and store._lex_mirror.df
        # filter and where_document go through the store's mask path
        n = len(texts)
        part1 = np.array([r % 3 == 1 for r in range(n)])
        _check_store(store, queries[0], ngram, 5, tally, mask=part1, filter={"part": 1})
        sub = queries[1][:2]
        has = np.array([sub in t for t in texts])
        _check_store(store, queries[0], ngram, 64 if has.sum() <= 64 else 5, tally, mask=has,
                     where_document={"$contains": sub})
        _check_store(store, queries[0], ngram, 3, tally, mask=has & part1, filter={"part": 1},
                     where_document={"$contains": sub})
        assert store.lexical_search(queries[0], k=5, filter={"part": 7}) == []
        # batch form = the single queries
        batch = store.lexical_search_batch(queries, k=4)
        assert [[d.id for d in hits] for hits in batch] == [[d.id for d in store.lexical_search(q, k=4)] for q in queries]
        # queries without terms return no rows
        assert store.lexical_search("") == [] and store.lexical_search("  \n ") == []
        if ngram == 2:
            assert store.lexical_search(texts[10][:1]) == []
        with pytest.raises(ValueError, match="MQ_MAX_K"):
            store.lexical_search(queries[0], k=100)
    assert tally.ok(), (tally.ambiguous, tally.checked)


def test_store_mirror_follows_writes(require_gpu):
    """add_texts extends the mirror and drops the df cache; delete rebuilds it."""
    texts = _synthetic_texts(200, seed=3)
    store = _store(texts[:150], 1)
    _number_rows(store)
    tally = lc.Tally()
    q = texts[20][:5]
    _check_store(store, q, 1, 10, tally)
    first = store._lex_mirror
    assert first.n == 150 and first.df
    store.add_texts(texts[150:], metadatas=[{"part": 0, "r": r} for r in range(150, 200)],
                    ids=["id%d" % r for r in range(150, 200)])
    _number_rows(store)
    _check_store(store, q, 1, 10, tally)
    assert store._lex_mirror is first and first.n == 200  # extended, not rebuilt
    store.delete(["id5", "id20", "id150"])
    _number_rows(store)
    _check_store(store, q, 1, 10, tally)
    assert store._lex_mirror is not first and store._lex_mirror.n == 197
    assert tally.ok(), (tally.ambiguous, tally.checked)


def test_store_edge_cases(require_gpu):
    emb = _embeddings()
    empty = HipChroma(embedding_function=emb, auto_persist=False)
    assert empty.lexical_search("糖尿病") == [] and empty.hybrid_search("糖尿病") == []
    assert empty.lexical_search_batch(["a"]) == [[]] and empty.hybrid_search_batch(["a", "b"]) == [[], []]
    small = _store(["甲乙丙", "乙丙丁", "丁戊"], 1)
    _number_rows(small)
    hits = small.lexical_search_with_score("乙丙", k=10)  # k > n
    assert [d.metadata["r"] for d, _ in hits] == [0, 1] and hits[0][1] == hits[1][1]
    assert len(small.hybrid_search("乙丙", k=10, fetch_k=50)) == 3
    assert small.lexical_search("乙丙", k=0) == [] and small.hybrid_search("乙丙", k=0) == []


@pytest.mark.parametrize("ngram", [1, 2])
def test_store_hybrid_search_is_rrf_of_its_own_lists(require_gpu, golden, ngram):
    texts = _medical_texts(golden)
    store = _store(texts, ngram)
    queries = ["二甲双胍的剂量", "糖尿病", "运动对长寿的作用"]
    for q in queries:
        for fetch_k, wts, c, kw in ((20, (0.5, 0.5), 60, {}), (64, (0.3, 0.7), 10, {}), (200, (1.0, 0.0), 60, {}),
                                    (8, (0.0, 1.0), 1, {}), (20, (0.5, 0.5), 60, {"filter": {"part": 2}}),
                                    (20, (0.5, 0.5), 60, {"where_document": {"$contains": "的"}})):
            fk = min(fetch_k, _lib.MQ_MAX_K)
            dense = [d.id for d in store.similarity_search(q, k=fk, **kw)]
            lex = [d.id for d in store.lexical_search(q, k=fk, **kw)]
            rows = {i: r for r, i in enumerate(store._ids)}
            want = lc.rrf_reference([rows[i] for i in dense], [rows[i] for i in lex], wts, c, 6)
            got = store.hybrid_search_with_score(q, k=6, fetch_k=fetch_k, weights=wts, c=c, **kw)
            assert [(rows[d.id], x) for d, x in got] == want, (q, fetch_k, wts)
            assert [d.id for d in store.hybrid_search(q, k=6, fetch_k=fetch_k, weights=wts, c=c, **kw)] == \
                [d.id for d, _ in got]
    # the batch form: one encoder batch and one dense search (similarity_search_batch's), looped lexical
    batch = store.hybrid_search_batch(queries, k=5, fetch_k=20)
    dense_b = store.similarity_search_batch(queries, k=20)
    rows = {i: r for r, i in enumerate(store._ids)}
    for q, got, dense in zip(queries, batch, dense_b):
        lex = [rows[d.id] for d in store.lexical_search(q, k=20)]
        want = lc.rrf_reference([rows[d.id] for d in dense], lex, (0.5, 0.5), 60, 5)
        assert [rows[d.id] for d in got] == [r for r, _ in want], q
    # k follows the rule of every search: past MQ_MAX_K it raises while more than that many rows are candidates
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.hybrid_search(queries[0], k=100)
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.hybrid_search(queries[0], k=100, fetch_k=200, filter={"part": {"$ne": 2}})  # 103 rows admitted
    few = store.hybrid_search(queries[0], k=100, fetch_k=200, filter={"r": {"$lt": 9}})
    assert sorted(d.metadata["r"] for d in few) == list(range(9))
    assert store.hybrid_search(queries[0], k=5, fetch_k=0) == [] and store.hybrid_search(queries[0], k=5, fetch_k=-3) == []
    r = store.as_retriever(search_type="hybrid", search_kwargs={"k": 3, "fetch_k": 10})
    assert [d.id for d in r.invoke(queries[0])] == [d.id for d in store.hybrid_search(queries[0], k=3, fetch_k=10)]
    r = store.as_retriever(search_type="lexical", search_kwargs={"k": 3})
    assert [d.id for d in r.get_relevant_documents(queries[1])] == [d.id for d in store.lexical_search(queries[1], k=3)]
    sim = store.as_retriever(search_kwargs={"k": 3}).invoke(queries[0])
    assert [d.id for d in sim] == [d.id for d in store.similarity_search(queries[0], k=3)]


# ------------------------------------------------- more blocks than workgroups ----
# The score pass runs at most 2048 workgroups (queries of <= 16 terms; 1024 above that) and the
# df pass 2048, each walking blocks b, b + grid, ...: past 2048 * 64 = 131072 rows a workgroup
# walks a second block, reuses its LDS tables, loads the next block's row starts ahead, rejects
# rows against a running list that is no longer empty and merges into it.
BIG_N = 2 * 2048 * 64 + 77  # every workgroup of either build walks at least two blocks


@functools.lru_cache(maxsize=None)
def _big_corpus():
    """BIG_N rows of 0..8 tokens over 30 ids; every seventh row copied into its neighbour, and
    every fifth row of the first 131072 copied 131072 rows up: its twin is in the block the
    same workgroup walks next (2048 workgroups) or two blocks on (1024), so exact ties meet in
    one workgroup's running list."""
    rng = np.random.default_rng(77)
    p = 1.0 / np.arange(1, 31)
    p /= p.sum()
    lens = rng.integers(0, 9, BIG_N)
    flat = (1000 + rng.choice(30, int(lens.sum()), p=p)).astype(np.uint16)
    offs = np.zeros(BIG_N + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    rows = [flat[offs[r]:offs[r + 1]] for r in range(BIG_N)]
    for r in range(0, BIG_N - 1, 7):
        rows[r + 1] = rows[r]
    for r in range(0, 2048 * 64, 5):
        rows[r + 2048 * 64] = rows[r]
    return lc.pack(rows)


@functools.lru_cache(maxsize=None)
def _big_dev():
    return _Dev(_big_corpus())


@pytest.mark.parametrize("n_terms", [8, 24])
@pytest.mark.parametrize("ngram", [1, 2])
def test_workgroups_walk_several_blocks(require_gpu, ngram, n_terms):
    """df and the top-k at BIG_N rows, with the 16-term and the 128-term build, without a mask,
    with a random one and with one that admits every 4099th row (its top 64 span all blocks),
    k 1 and 64."""
    dev = _big_dev()
    flat, offs = dev.corpus
    rows = [flat[offs[r]:offs[r + 1]] for r in range(0, 4000)]
    q = lc.query_tokens(rows, n_terms, n_terms, ngram, repeat=2, absent=1)
    sparse = np.arange(BIG_N) % 4099 == 0
    rand = np.random.default_rng(5).random(BIG_N) < 0.5
    tally = lc.Tally()
    setup = dev.check(q, ngram, [(None, 64), (None, 1), (rand, 64), (sparse, 64), (sparse, 1)], tally, (ngram, n_terms))
    assert (len(setup["keys"]) <= 16) == (n_terms == 8)
    assert tally.ok(), (tally.ambiguous, tally.checked)


@pytest.mark.parametrize("n_terms", [3, 20])
def test_identical_rows_over_several_blocks_a_workgroup(require_gpu, n_terms):
    """BIG_N identical rows: every later block of a workgroup ties with its running list and
    must lose to it, so the ids are 0 .. k - 1; with every 4099th row admitted, those rows in
    order (each workgroup merges blocks into a list that is not empty)."""
    row = np.r_[np.arange(1000, 1000 + n_terms), 1000].astype(np.uint16)
    dev = _Dev((np.tile(row, BIG_N), np.arange(BIG_N + 1, dtype=np.int64) * len(row)))
    keys = np.arange(1000, 1000 + n_terms, dtype=np.uint32)
    assert lex_df(dev.tokens, dev.offs, 1, keys).tolist() == [BIG_N] * n_terms
    w = np.linspace(0.5, 1.5, n_terms).astype(np.float32)
    sparse = np.arange(BIG_N) % 4099 == 0
    for m, k in ((None, 64), (None, 1), (sparse, 64)):
        s, i = lex_topk(dev.tokens, dev.offs, 1, keys, w, 0.3, 0.01, k, bits=dev.bits(m))
        want = (np.arange(BIG_N) if m is None else np.flatnonzero(m))[:k]
        assert i.cpu().numpy().tolist() == want.tolist()
        s = s.cpu().numpy()
        assert np.all(s == s[0]) and s[0] > 0


def test_topk_with_host_outputs(require_gpu):
    """mq_lex_topk with io_on_device = 0: the result staged in scratch and copied to host arrays
    equals the device-output call's, bit for bit (rows over several blocks; padding too)."""
    import torch
    from mediquery_hip.native import lex_scratch_bytes
    rows = _zipf(1000, 60, 11)
    dev = _Dev(lc.pack(rows))
    scratch = torch.empty(lex_scratch_bytes(dev.n, 64), dtype=torch.uint8, device=dev.dev)
    for q, k in ((lc.query_tokens(rows, 5, 1, 1), 64), (lc.query_tokens(rows, 40, 2, 1, absent=1), 7), ([9], 3)):
        setup = lc.bm25_setup(dev.corpus, q, 1)
        keys, w = setup["keys"], setup["w"]
        s, i = lex_topk(dev.tokens, dev.offs, 1, keys, w, setup["c0"], setup["c1"], k)
        hs, hi = np.full(k, 7.0, np.float32), np.full(k, 7, np.int64)
        import ctypes
        _lib.call("mq_lex_topk", _lib.ptr(dev.tokens), dev.tokens.numel(), _lib.ptr(dev.offs), dev.n, 1,
                  _lib.ptr(keys), _lib.ptr(w), len(keys), ctypes.c_float(float(setup["c0"])),
                  ctypes.c_float(float(setup["c1"])), None, k, _lib.ptr(hs), _lib.ptr(hi), 0, _lib.ptr(scratch),
                  _lib.stream_handle(None))
        assert hi.tolist() == i.cpu().numpy().tolist() and hs.tobytes() == s.cpu().numpy().tobytes()
        if q == [9]:
            assert hi.tolist() == [-1] * k and np.isneginf(hs).all()
