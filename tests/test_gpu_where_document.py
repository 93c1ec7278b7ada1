"""Document-text filtering (Chroma's `where_document`: $contains / $not_contains / $and / $or)
on the device: mq_mask_contains (contains_scan_kernel, K12) against Python's `in` row by row -
random two-letter text, planted patterns at every lane-chunk and workgroup-span alignment, row
boundaries, zero-length rows, the real corpus - and `HipChroma(where_document=)` against the
same rows selected through metadata, whose masked searches are tested at 1M rows already
(test_gpu_filter.py): identical rows, order and scores."""
import json
import os

import numpy as np
import pytest

from mediquery_hip import _lib, compat
from mediquery_hip.native import mask_contains
from mediquery_hip.vectorstore import HipChroma, _match_document

pytestmark = pytest.mark.gpu

SPAN = _lib.MQ_CONTAINS_SPAN_BYTES  # text bytes per workgroup of the scan
CHUNK = 16                          # start positions per lane and step
SET, AND, OR = _lib.MQ_MASK_SET, _lib.MQ_MASK_AND, _lib.MQ_MASK_OR


class _Blob:
    """Rows (bytes) on the device as mq_mask_contains wants them; the text tensor holds
    exactly text_bytes bytes."""

    def __init__(self, rows):
        import torch
        dev = torch.device("cuda", 0)
        self.rows = rows
        self.n = len(rows)
        text = b"".join(rows)
        offs = np.zeros(self.n + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=offs[1:])
        self.offs_host = offs
        self.text = (torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev) if text
                     else torch.empty(0, dtype=torch.uint8, device=dev))
        assert self.text.numel() == len(text) == offs[-1]
        self.offs = torch.from_numpy(offs).to(dev)
        self.words = (self.n + 31) // 32
        self.scratch = torch.empty(max(1, self.words), dtype=torch.int32, device=dev)

    def run(self, pattern, mode=SET, negate=False, prior=None):
        """-> (bool [n], the mask's words): bits (mode)= contains ^ negate onto `prior` words."""
        import torch
        if prior is None:  # SET must overwrite whatever was there
            bits = torch.full((max(1, self.words),), -1, dtype=torch.int32, device=self.text.device)
        else:
            bits = torch.from_numpy(prior.view(np.int32).copy()).to(self.text.device)
        mask_contains(self.text, self.offs, pattern, bits, mode, negate, scratch=self.scratch)
        words = bits.cpu().numpy().view(np.uint32)[:self.words]
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n].astype(bool), words

    def want(self, pattern):
        return np.array([pattern in r for r in self.rows], dtype=bool)

    def check(self, pattern, note=""):
        got, words = self.run(pattern)
        want = self.want(pattern)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (note, pattern[:20], len(pattern), bad[:5], want[bad[:5]])
        _tail_zero(words, self.n)
        return want


def _tail_zero(words, n):
    if n % 32:
        assert int(words[-1]) >> (n % 32) == 0, "bits past n are set"


def _pack(b):
    return np.packbits(np.concatenate([b, np.zeros(-len(b) % 32, bool)]), bitorder="little").view(np.uint32)


@pytest.mark.parametrize("n", [1, 31, 33, 64, 1000, 4097])
def test_contains_kernel_matches_python_random(require_gpu, n):
    """Rows of 0..300 bytes over b"ab" (partial and overlapping matches everywhere), patterns cut
    from the blob, half of them across a row boundary, plus patterns that occur nowhere: SET,
    AND / OR onto a random prior mask, and negate, each equal to `pattern in row` per row."""
    rng = np.random.default_rng(100 + n)
    ab = np.frombuffer(b"ab", np.uint8)
    rows = [ab[rng.integers(0, 2, int(rng.integers(0, 301)))].tobytes() for _ in range(n)]
    if not any(rows):
        rows[0] = b"abba"
    blob = _Blob(rows)
    text = b"".join(rows)
    offs = blob.offs_host
    patterns = []
    for j in range(40):
        L = int(rng.integers(1, 13))
        if j % 2 and n > 1:  # across a row boundary (when the neighbours are long enough)
            b = int(offs[int(rng.integers(1, n))])
            p0 = max(0, b - int(rng.integers(1, L + 1)))
        else:
            p0 = int(rng.integers(0, max(1, len(text) - L + 1)))
        if text[p0:p0 + L]:
            patterns.append(text[p0:p0 + L])
    patterns += [b"c", b"abc", b"ab" * 6 + b"c", b"\x00", b"a" * 256, b"ab" * 128]
    for pat in patterns:
        want = blob.check(pat, "SET")
        prior_b = rng.integers(0, 2, n).astype(bool)
        prior = _pack(prior_b)
        for mode, neg, ref in ((AND, False, prior_b & want), (OR, False, prior_b | want),
                               (SET, True, ~want), (AND, True, prior_b & ~want), (OR, True, prior_b | ~want)):
            got, words = blob.run(pat, mode, neg, None if mode == SET else prior)
            assert np.array_equal(got, ref), (n, pat, mode, neg, np.flatnonzero(got != ref)[:5])
            _tail_zero(words, n)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 15, 16, 17, 64, 255, 256])
def test_contains_kernel_planted_alignments(require_gpu, m):
    """5,000 rows, row r = r % 97 filler bytes, the pattern, (r * 7) % 89 filler bytes (the filler
    alphabet is disjoint from the pattern's): the pattern's start in the blob takes every residue
    modulo the lane chunk, with every way of straddling two chunks.  Every row matches; with the
    pattern's last byte changed none does.  (The blob has 28-107 workgroup spans, too few to
    meet every split of a pattern over a span boundary: the next test plants those.)"""
    rng = np.random.default_rng(m)
    pat = np.frombuffer(b"PQR", np.uint8)[rng.integers(0, 3, m)].tobytes()
    fill = np.frombuffer(b"01", np.uint8)
    rows, starts, off = [], [], 0
    for r in range(5000):
        row = fill[rng.integers(0, 2, r % 97)].tobytes() + pat + fill[rng.integers(0, 2, (r * 7) % 89)].tobytes()
        starts.append(off + r % 97)
        off += len(row)
        rows.append(row)
    starts = np.array(starts)
    assert set((starts % CHUNK).tolist()) == set(range(CHUNK))
    assert {int(s % CHUNK) for s in starts if s % CHUNK + m > CHUNK} == set(range(max(0, CHUNK - m + 1), CHUNK))
    if m >= 4:  # some occurrences lie across two workgroups' spans
        assert any(s % SPAN + m > SPAN for s in starts)
    blob = _Blob(rows)
    assert blob.check(pat, "planted").all()
    miss = pat[:-1] + b"Z"
    assert not blob.check(miss, "last byte changed").any()
    got, _ = blob.run(miss, SET, True)
    assert got.all()


@pytest.mark.parametrize("m", [2, 3, 5, 17, 64, 256])
def test_contains_kernel_every_split_over_a_span_boundary(require_gpu, m):
    """Row j (as long as a span, starting half a span in) holds the pattern with its first j bytes
    before the span boundary, j = 1 .. m - 1: each matches.  The same bytes cut into rows AT the
    span boundaries put every split over a row boundary too: nothing matches."""
    rng = np.random.default_rng(1000 + m)
    pat = np.frombuffer(b"PQR", np.uint8)[rng.integers(0, 3, m)].tobytes()
    fill = np.frombuffer(b"01", np.uint8)
    half = SPAN // 2
    rows = [fill[rng.integers(0, 2, half)].tobytes()]
    for j in range(1, m):
        body = bytearray(fill[rng.integers(0, 2, SPAN)].tobytes())
        body[half - j:half - j + m] = pat
        rows.append(bytes(body))
    blob = _Blob(rows)
    want = blob.check(pat, "span splits")
    assert want[1:].all() and not want[0]
    text = b"".join(rows) + fill[rng.integers(0, 2, half)].tobytes()
    cut = _Blob([text[i:i + SPAN] for i in range(0, len(text), SPAN)])
    assert not cut.check(pat, "row boundary at the span boundary").any()


def test_contains_kernel_row_boundaries_and_blob_ends(require_gpu):
    fill = b"01" * 40000
    for m in (1, 3, 16, 200):
        pat = (b"PQRRQ" * 52)[:m]
        # one 64 KB row with the pattern at its end, zero-length rows around it (first and last too)
        rows = [b""] * 40 + [fill[:65536 - m] + pat] + [b""] * 40
        want = _Blob(rows).check(pat, "long row")
        assert want.sum() == 1 and want[40]
        # a match at blob byte 0 and a match ending at the blob's last byte
        rows = [pat + fill[:100], fill[:5000], b"", fill[:77] + pat]
        want = _Blob(rows).check(pat, "blob ends")
        assert want.tolist() == [True, False, False, True]
        # the pattern is a whole row / longer than every row
        rows = [fill[:9], pat, fill[:m - 1] if m > 1 else b"", pat[:-1], pat + b"0", b""]
        want = _Blob(rows).check(pat, "whole row")
        assert want.tolist() == [False, True, False, False, True, False]
        assert not _Blob([pat[:-1]] * 70 + [b""]).check(pat, "longer than every row").any()
    # a pattern lying across two rows does not match
    b = _Blob([b"..ab", b"cd..", b"..ab", b"", b"cd..", b"abc", b"d"])
    assert not b.check(b"abcd", "across rows").any()
    assert b.check(b"ab", "").tolist() == [True, False, True, False, False, True, False]
    # self-overlapping patterns, one-byte patterns hitting almost everywhere
    b = _Blob([b"aaab", b"aab", b"aba", b"a" * 1000 + b"b", b"a" * 1000, b"b", b""] * 9)
    for pat in (b"aab", b"a", b"b", b"aaaa", b"a" * 256, b"a" * 255 + b"b", b"ba"):
        b.check(pat, "overlap")
    # a span that holds hundreds of short rows (more rows than the kernel's LDS row table)
    rng = np.random.default_rng(5)
    ab = np.frombuffer(b"ab", np.uint8)
    rows = [ab[rng.integers(0, 2, int(rng.integers(0, 4)))].tobytes() for _ in range(30000)]
    b = _Blob(rows)
    for pat in (b"a", b"ab", b"aba", b"bb", b"abab"):
        b.check(pat, "short rows")
    # only zero-length rows: nothing to scan, negate admits them all
    b = _Blob([b""] * 37)
    assert not b.check(b"a", "empty").any()
    got, words = b.run(b"a", SET, True)
    assert got.all()
    _tail_zero(words, 37)


def test_mask_contains_rejects_bad_tensors(require_gpu):
    import torch
    b = _Blob([b"abc", b"de"])
    bits = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="uint8"):
        mask_contains(b.text.to(torch.int8), b.offs, b"a", bits, SET)
    with pytest.raises(ValueError, match="uint8"):
        mask_contains(b.text.cpu(), b.offs, b"a", bits, SET)
    with pytest.raises(ValueError, match="int64"):
        mask_contains(b.text, b.offs.to(torch.int32), b"a", bits, SET)
    with pytest.raises(ValueError, match="int64"):
        mask_contains(b.text, b.offs.cpu(), b"a", bits, SET)
    with pytest.raises(ValueError, match="ceil"):
        mask_contains(b.text, torch.zeros(100, dtype=torch.int64, device="cuda:0"), b"a", bits, SET)
    with pytest.raises(ValueError, match="bytes"):
        mask_contains(b.text, b.offs, b"", bits, SET)
    with pytest.raises(ValueError, match="bytes"):
        mask_contains(b.text, b.offs, b"a" * 257, bits, SET)
    with pytest.raises(ValueError, match="scratch"):
        mask_contains(b.text, b.offs, b"a", bits, SET, scratch=bits)
    with pytest.raises(ValueError, match="aligned"):
        mask_contains(torch.zeros(64, dtype=torch.uint8, device="cuda:0")[1:6], b.offs, b"a", bits, SET)


def _docs(golden):
    with open(os.path.join(golden, "corpus_docs.json"), encoding="utf-8") as f:
        return [d["page_content"] for d in json.load(f)["docs"]]


def test_contains_kernel_on_the_corpus(require_gpu, golden):
    docs = _docs(golden)
    assert len(docs) == 154
    blob = _Blob([d.encode("utf-8") for d in docs])
    for pat, count in (("糖尿病", 11), ("治疗", 16), ("高血压", 2), ("。", 153), ("头痛", 0), ("a", 21),
                       (docs[0], 1)):  # the full text of document 0: 253 bytes
        want = np.array([pat in d for d in docs])
        if count is not None:
            assert int(want.sum()) == count, pat
        got = blob.check(pat.encode("utf-8"), pat)
        assert np.array_equal(got, want), pat  # bytes in bytes == str in str


# ------------------------------------------------------------------ the store ----
P1, P2 = "糖尿病", "治疗"
FEW = " #1234"  # rows 1234 and 12340..12349


class _Emb:
    """The store embeds through this: query strings are indices into `vecs`."""

    def __init__(self, vecs):
        self.vecs = vecs

    def embed_documents(self, texts):
        return [self.vecs[int(t)] for t in texts]

    def embed_query(self, text):
        return self.vecs[int(text)]


@pytest.fixture(scope="module")
def doc_store(require_gpu, golden):
    docs = _docs(golden)
    n = 20011  # not a multiple of 32
    texts = ["%s #%d" % (docs[i % len(docs)], i) for i in range(n)]
    metas = [{"has": P1 in t, "has2": P2 in t, "few": FEW in t, "par": i % 3} for i, t in enumerate(texts)]
    rng = np.random.default_rng(42)
    emb = rng.standard_normal((n, 64)).astype(np.float32)
    store = HipChroma(dim=64, auto_persist=False)
    store.add_embeddings(emb, texts, metas, ["id%d" % i for i in range(n)])
    qs = emb[rng.integers(0, n, 8)] + 0.3 * rng.standard_normal((8, 64)).astype(np.float32)
    store._embedding_function = _Emb(qs)
    return store, texts, emb, qs


CLAUSES = [
    ({"$contains": P1}, {"has": True}),
    ({"$not_contains": P1}, {"has": False}),
    ({"$and": [{"$contains": P1}, {"$contains": P2}]}, {"$and": [{"has": True}, {"has2": True}]}),
    ({"$or": [{"$contains": P1}, {"$contains": P2}]}, {"$or": [{"has": True}, {"has2": True}]}),
    ({"$or": [{"$and": [{"$contains": P1}, {"$not_contains": P2}]}, {"$contains": FEW}]},
     {"$or": [{"$and": [{"has": True}, {"has2": False}]}, {"few": True}]}),
    ({"$and": [{"$or": [{"$contains": P1}, {"$contains": FEW}]}, {"$not_contains": P2}]},
     {"$and": [{"$or": [{"has": True}, {"few": True}]}, {"has2": False}]}),
]


def _pairs(res):
    return [(d.id, d.page_content, s) for d, s in res]


@pytest.mark.parametrize("wd,meta", CLAUSES)
def test_store_where_document_equals_metadata_filter(doc_store, wd, meta):
    """`where_document` and the metadata filter that marks the same rows give identical results:
    rows, order and scores, on every search path and in get()."""
    store, texts, emb, qs = doc_store
    for q in qs[:3]:
        a = store.similarity_search_by_vector_with_score(q, k=5, where_document=wd)
        b = store.similarity_search_by_vector_with_score(q, k=5, filter=meta)
        assert _pairs(a) == _pairs(b) and len(a) == 5
        a = store.max_marginal_relevance_search_by_vector(q, k=4, fetch_k=20, where_document=wd)
        b = store.max_marginal_relevance_search_by_vector(q, k=4, fetch_k=20, filter=meta)
        assert [d.id for d in a] == [d.id for d in b] and len(a) == 4
    names = [str(j) for j in range(len(qs))]
    a = store.similarity_search_batch(names, k=5, where_document=wd)
    b = store.similarity_search_batch(names, k=5, filter=meta)
    assert [[d.id for d in row] for row in a] == [[d.id for d in row] for row in b]
    a = store.max_marginal_relevance_search_batch(names, k=3, fetch_k=10, where_document=wd)
    b = store.max_marginal_relevance_search_batch(names, k=3, fetch_k=10, filter=meta)
    assert [[d.id for d in row] for row in a] == [[d.id for d in row] for row in b]
    assert store.get(where_document=wd) == store.get(where=meta)
    assert store.get(where_document=wd, limit=7, offset=3) == store.get(where=meta, limit=7, offset=3)
    # with a second metadata filter: the conjunction
    a = store.similarity_search_by_vector_with_score(qs[0], k=5, where_document=wd, filter={"par": 1})
    b = store.similarity_search_by_vector_with_score(qs[0], k=5, filter={"$and": [meta, {"par": 1}]})
    assert _pairs(a) == _pairs(b) and len(a) == 5
    assert store.get(where_document=wd, where={"par": 1}, ids=["id%d" % i for i in range(0, 3000, 7)]) == \
        store.get(where={"$and": [meta, {"par": 1}]}, ids=["id%d" % i for i in range(0, 3000, 7)])
    a = store.similarity_search_with_relevance_scores("1", k=3, where_document=wd)
    b = store.similarity_search_with_relevance_scores("1", k=3, filter=meta)
    assert _pairs(a) == _pairs(b)


def test_store_where_document_clipping_and_raising(doc_store):
    store, texts, emb, qs = doc_store
    q = qs[0]
    few = [i for i, t in enumerate(texts) if FEW in t]
    assert few == [1234] + list(range(12340, 12350))
    assert store.similarity_search_by_vector(q, k=5, where_document={"$contains": "头痛头痛"}) == []
    assert store.similarity_search_batch(["0", "1"], k=5, where_document={"$contains": "头痛头痛"}) == [[], []]
    assert store.max_marginal_relevance_search_by_vector(q, k=5, where_document={"$contains": "头痛头痛"}) == []
    assert store.get(where_document={"$contains": "头痛头痛"})["ids"] == []
    # k larger than the admitted rows returns them all, as the filtered search does
    for k in (50, 64, 100):
        a = store.similarity_search_by_vector_with_score(q, k=k, where_document={"$contains": FEW})
        b = store.similarity_search_by_vector_with_score(q, k=k, filter={"few": True})
        assert _pairs(a) == _pairs(b)
        assert sorted(int(d.id[2:]) for d, _ in a) == few
    a = store.max_marginal_relevance_search_by_vector(q, k=20, fetch_k=100, where_document={"$contains": FEW})
    b = store.max_marginal_relevance_search_by_vector(q, k=20, fetch_k=100, filter={"few": True})
    assert [d.id for d in a] == [d.id for d in b] and len(a) == len(few)
    # k past MQ_MAX_K with more than 64 admitted rows raises; the count is the combined mask's
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.similarity_search_by_vector(q, k=100, where_document={"$contains": P1})
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.similarity_search_batch(["0"], k=65, where_document={"$contains": P1})
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.max_marginal_relevance_search_by_vector(q, k=5, fetch_k=100, where_document={"$contains": P1})
    got = store.similarity_search_by_vector(q, k=100, where_document={"$contains": P1}, filter={"few": True})
    assert sorted(int(d.id[2:]) for d in got) == [i for i in few if P1 in texts[i]]
    with pytest.raises(ValueError, match="regex"):
        store.similarity_search_by_vector(q, k=5, where_document={"$regex": "a"})


def test_store_where_document_against_match_document(doc_store):
    """The admitted set straight from `_match_document` (not through metadata), and the search
    over it against a float64 ranking of those rows."""
    store, texts, emb, qs = doc_store
    wd = {"$and": [{"$contains": P2}, {"$or": [{"$contains": "高血压"}, {"$contains": " #7"}]},
                   {"$not_contains": "#19"}]}
    admitted = np.array([i for i, t in enumerate(texts) if _match_document(t, wd)])
    assert 64 < len(admitted) < len(texts) // 4
    assert store.get(where_document=wd)["ids"] == ["id%d" % i for i in admitted]
    unit = emb[admitted].astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    for q in qs:
        cos = unit @ q.astype(np.float64)  # the index's score: the query as given, unit rows
        order = np.lexsort((admitted, -cos))[:10]
        got = store._search_rows(q, 10, None, wd)
        assert [r for r, _ in got] == admitted[order].tolist()
        np.testing.assert_allclose([c for _, c in got], cos[order], rtol=1e-5, atol=1e-5)


def _admitted_ids(store, wd):
    return [i for i, t in zip(store._ids, store._texts) if _match_document(t, wd)]


def _check_store(store, wd, q):
    want = _admitted_ids(store, wd)
    assert 0 < len(want) <= 64
    for _ in range(2):  # the second pass is served from the one-entry cache
        assert store.get(where_document=wd)["ids"] == want
        got = store.similarity_search_by_vector(q, k=64, where_document=wd)
        assert sorted(d.id for d in got) == sorted(want)
        assert all(_match_document(d.page_content, wd) for d in got)
    return want


def test_mirror_upkeep_across_writes(require_gpu, golden, tmp_path):
    docs = _docs(golden)
    rng = np.random.default_rng(8)
    n = len(docs)
    store = HipChroma(dim=64, persist_directory=str(tmp_path), collection_name="wd")
    store.add_embeddings(rng.standard_normal((n, 64)).astype(np.float32), list(docs), [{"i": i} for i in range(n)],
                         ["d%d" % i for i in range(n)])
    q = rng.standard_normal(64).astype(np.float32)
    wd = {"$contains": P1}
    store.similarity_search_by_vector(q, k=3, filter={"i": {"$lt": 50}})
    assert store._doc_mirror is None  # never allocated without where_document
    first = _check_store(store, wd, q)
    assert len(first) == 11
    mirror = store._doc_mirror
    assert mirror is not None and mirror.n == n
    bits = store._doc_bits(wd)
    assert store._doc_bits(wd) is bits  # repeated clause: no second scan
    assert store._doc_bits({"$contains": P2}) is not bits
    # a plain append extends the mirror in place
    new = ["新增文档：%s的饮食管理 %d" % (P1, j) for j in range(5)] + ["无关的新增文档"]
    store.add_embeddings(rng.standard_normal((6, 64)).astype(np.float32), new, [{"i": -1}] * 6,
                         ["new%d" % j for j in range(6)])
    got = _check_store(store, wd, q)
    assert got == first + ["new%d" % j for j in range(5)]
    assert store._doc_mirror is mirror and mirror.n == n + 6
    assert int(mirror.offs[mirror.n]) == mirror.nbytes == sum(len(t.encode("utf-8")) for t in store._texts)
    # delete renumbers the rows: the mirror is rebuilt
    gone = [first[0], first[3], "new1", next(i for i in store._ids if i not in first)]
    store.delete(gone)
    got = _check_store(store, wd, q)
    assert got == [i for i in first + ["new%d" % j for j in range(5)] if i not in gone]
    assert store._doc_mirror is not mirror
    # an upsert that takes the pattern out of a row, and one that puts it into another
    keep = got[1]
    other = next(i for i in store._ids if i not in got)
    store.add_embeddings(rng.standard_normal((2, 64)).astype(np.float32), ["这一行不再提到它", "这一行现在提到" + P1],
                         [{"i": -2}] * 2, [keep, other])
    got2 = _check_store(store, wd, q)
    assert keep not in got2 and other in got2
    _check_store(store, {"$and": [wd, {"$not_contains": "新增"}]}, q)
    # persisted and reloaded: the same clause, the same answer
    again = HipChroma(dim=64, persist_directory=str(tmp_path), collection_name="wd")
    assert again._doc_mirror is None
    assert again.get(where_document=wd) == store.get(where_document=wd)
    a = again.similarity_search_by_vector_with_score(q, k=5, where_document=wd)
    b = store.similarity_search_by_vector_with_score(q, k=5, where_document=wd)
    assert _pairs(a) == _pairs(b) and len(a) == 5


def test_retriever_passes_where_document(doc_store):
    """The duck-typed base's as_retriever hands `where_document` (and `filter`) of search_kwargs
    to both search types."""
    store, texts, emb, qs = doc_store
    wd = {"$contains": "高血压"}
    r = compat.VectorStoreBase.as_retriever(store, search_kwargs={"k": 3, "where_document": wd})
    got = r.invoke("2")
    assert len(got) == 3 and all("高血压" in d.page_content for d in got)
    assert [d.id for d in got] == [d.id for d in store.similarity_search("2", k=3, where_document=wd)]
    r = compat.VectorStoreBase.as_retriever(store, search_type="mmr",
                                            search_kwargs={"k": 3, "fetch_k": 12, "where_document": wd})
    got = r.invoke("2")
    assert len(got) == 3 and all("高血压" in d.page_content for d in got)
    r = compat.VectorStoreBase.as_retriever(store, search_kwargs={"k": 3, "where_document": wd,
                                                                   "filter": {"par": 2}})
    got = r.invoke("2")
    assert len(got) == 3 and all("高血压" in d.page_content and d.metadata["par"] == 2 for d in got)
