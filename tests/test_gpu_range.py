"""The device range search (K17, csrc/range.hip) against the float64 restatement of the
definition (tests/range_cases.py): bit-for-bit equality on the exact class - counts, ids,
scores, the order inside the large tie groups every cut falls into, the padding - over the row
counts, dims, batch sizes, max_hits, thresholds and masks at which the kernels change path;
one vector repeated (the row digits of the radix select); a case sized from the launch
geometry; host against device I/O and a reused scratch; agreement with the existing search;
the bound of the random class; then HipChroma's range methods, the count and the retrievers.

What the device showed on the random class (MI355X; the test prints the figures): the worst
|score - float64| was 5.1e-8 at dim 64 (bound 4.3e-6), 3.1e-8 at 256 (1.6e-5), 2.5e-8 at 768
(4.6e-5) and 2.3e-8 at 1024 (6.2e-5); undecided rows at most 191 of 13193 positions of a case
(1.4 %, cap 5 %)."""
import numpy as np
import pytest
import torch

import range_cases as rc
from mediquery_hip import Document, HipChroma, RangeResult, _lib
from mediquery_hip.native import FlatIndex, range_scan_blocks, range_scratch_bytes, range_select_blocks

pytestmark = pytest.mark.gpu

INF = float("inf")
_cache = {}


def _exact_index(dim, n):
    """(index, rows, float64 scores of the 40 exact queries) of an exact-class corpus; the
    index holds the rows bit for bit - the precondition of every equality."""
    key = (dim, n)
    if key not in _cache:
        rows = rc.exact_corpus(dim, n)
        ix = FlatIndex(dim=dim, device=0)
        ix.add(rows)
        assert np.array_equal(ix.get(), rows)
        _cache[key] = (ix, rows, rc.dots64(rows, rc.exact_queries(dim, max(rc.NQS))))
    return _cache[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached corpora are read-only


def _bits(mask):
    return None if mask is None else _dev(rc.mask_words(mask))


def _same(got, ref, where):
    (gc, gs, gi), (ref_c, ref_s, ref_i) = got, ref
    assert np.array_equal(gc, ref_c), where
    assert np.array_equal(gi, ref_i), where
    assert np.array_equal(gs.view(np.int32), ref_s.astype(np.float32).view(np.int32)), where


@pytest.mark.parametrize("dim", rc.DIMS)
def test_exact_class_equals_reference(require_gpu, dim):
    queries = rc.exact_queries(dim, max(rc.NQS))
    seen = set()
    for ni, n in enumerate(rc.NS):
        ix, rows, s_all = _exact_index(dim, n)
        for ti, tau in enumerate(rc.MIN_SCORES):
            for mi, mk in enumerate(rc.MASKS):
                # every n meets every nq, every max_hits and every min_score; each (min_score,
                # mask) pair meets several of the others
                nq = rc.NQS[(ti + mi + ni) % len(rc.NQS)]
                mh = rc.MAX_HITS[(2 * ti + mi + ni) % len(rc.MAX_HITS)]
                mask = rc.row_mask(mk, n)
                ref = rc.range_reference(s_all[:nq], mask, tau, mh)
                got = ix.search_range(queries[:nq], mh, tau, _bits(mask))
                _same(got, ref, (dim, n, tau, mk, nq, mh))
                seen.add((n, nq)), seen.add((n, "mh", mh)), seen.add((n, "tau", ti))
                if (ref[2] < 0).any():
                    seen.add("pads")
                if (ref[0] > mh).any():
                    seen.add("cut")
    assert all((n, nq) in seen for n in rc.NS for nq in rc.NQS)
    assert all((n, "mh", mh) in seen for n in rc.NS for mh in rc.MAX_HITS)
    assert all((n, "tau", ti) in seen for n in rc.NS for ti in range(len(rc.MIN_SCORES)))
    assert "pads" in seen and "cut" in seen


def test_all_rows_one_vector_walks_the_row_digits(require_gpu):
    """Every row the same vector: all scores are 1, the score digits cannot split the ranking,
    and the cut falls on a row: 4096 of 5000 crosses the row word's digit boundaries (row 4095
    = 3 x 1024 + 1023), 1 takes the lowest row."""
    dim, n = 64, 5000
    q = rc.exact_queries(dim, 1)
    ix = FlatIndex(dim=dim, device=0)
    ix.add(np.repeat(q, n, axis=0))
    for mh in (4096, 1, 1000, 1025):
        c, s, i = ix.search_range(q, mh, 0.5)
        assert c.tolist() == [n] and i[0].tolist() == list(range(mh)) and (s == 1.0).all(), mh
    mask = np.ones(n, bool)
    mask[:40] = False                                           # the lowest rows are masked out
    for mh in (4096, 1):
        c, s, i = ix.search_range(q, mh, -INF, _bits(mask))
        assert c.tolist() == [n - 40] and i[0].tolist() == list(range(40, 40 + mh)) and (s == 1.0).all(), mh
    c, s, i = ix.search_range(q, 7, 1.0000001)                  # the next float above every score
    assert c.tolist() == [0] and (i == -1).all() and np.isneginf(s).all()


def test_large_case_walks_every_workgroups_loop_twice_and_the_tails(require_gpu):
    """Row count from the launch geometry: the scan's 2 x CUs workgroups of 16 lane groups, two
    rows per iteration, n = 9 G + 37 as in the grouped scan's test; the histogram and collect
    kernels' workgroups each loop at least twice over it and end on a ragged tail."""
    dim = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = 16 * 2 * cus
    n = 9 * G + 37
    assert range_scan_blocks(n, cus) == 2 * cus
    sel = range_select_blocks(n, cus)
    assert sel > 1 and n >= 2 * 256 * sel and n % (256 * sel) != 0 and n % 256 != 0
    rows = rc.exact_corpus(dim, n)
    ix = FlatIndex(dim=dim, device=0)
    ix.add(rows)
    assert np.array_equal(ix.get(), rows)
    queries = rc.exact_queries(dim, 17)
    s_all = rc.dots64(rows, queries)
    for mk, mh, tau in (("none", 4096, -INF), ("third", 1000, 0.25), ("none", 65, 1 / 32)):
        mask = rc.row_mask(mk, n)
        ref = rc.range_reference(s_all, mask, tau, mh)
        _same(ix.search_range(queries, mh, tau, _bits(mask)), ref, (n, mk, mh, tau))
        assert (ref[0] > mh).all()
    c, s, i = ix.search_range(queries[:1], 1, -INF, _bits(np.arange(n) == n - 1))
    assert c.tolist() == [1] and i.tolist() == [[n - 1]]        # the last row is reachable


def test_host_and_device_io_agree_and_a_reused_scratch_leaves_nothing_behind(require_gpu):
    dim, n, nq, mh, tau = 256, 4097, 40, 300, 1 / 32
    ix, rows, s_all = _exact_index(dim, n)
    queries = rc.exact_queries(dim, nq)
    mask = rc.row_mask("third", n)
    bits = _bits(mask)
    ref = rc.range_reference(s_all, mask, tau, mh)
    scratch = torch.empty(range_scratch_bytes(n, nq, 4096), dtype=torch.uint8, device="cuda")
    host = ix.search_range(queries, mh, tau, bits, scratch)
    _same(host, ref, "host")
    dq = _dev(queries)

    def outs(m=mh):
        return (torch.empty(nq, dtype=torch.int64, device="cuda"),
                torch.empty((nq, m), dtype=torch.float32, device="cuda"),
                torch.empty((nq, m), dtype=torch.int64, device="cuda"))
    out = [outs() for _ in range(3)]
    # two calls in a row on one scratch, then one that follows calls with other queries,
    # another max_hits, another min_score and no mask on the same scratch: stale histograms,
    # counters, flags or candidates would show
    ix.search_range_device(dq, mh, *out[0], min_score=tau, bits=bits, scratch=scratch)
    ix.search_range_device(dq, mh, *out[1], min_score=tau, bits=bits, scratch=scratch)
    other = ix.search_range(queries[::-1].copy(), 4096, -INF, None, scratch)
    _same(other, rc.range_reference(s_all[::-1], None, -INF, 4096), "other")
    oc, os_, oi = outs(1)
    ix.search_range_device(dq, 1, oc, os_, oi, min_score=0.8, scratch=scratch)   # no hits: every query settles at once
    ix.search_range_device(dq, mh, *out[2], min_score=tau, bits=bits, scratch=scratch)
    torch.cuda.synchronize()
    assert (oc.cpu().numpy() == 0).all() and (oi.cpu().numpy() == -1).all()
    for c, s, i in out:
        _same((c.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy()), ref, "device")
    # a query alone gives what it gives inside the batch
    one = ix.search_range(queries[20:21], mh, tau, bits)
    _same(one, tuple(a[20:21] for a in ref), "alone")


def test_agrees_with_the_existing_search(require_gpu):
    """max_hits <= 64 and no threshold: the exact fp32 top-k of FlatIndex.search."""
    for dim, n in ((64, 1000), (768, 4097)):
        ix, rows, s_all = _exact_index(dim, n)
        ix.set_precision(_lib.MQ_DTYPE_F32)
        queries = rc.exact_queries(dim, 17)
        for k in (1, 5, 64):
            c, s, i = ix.search_range(queries, k)
            ks, ki = ix.search(queries, k)
            assert (c == n).all() and np.array_equal(i, ki), (dim, n, k)
            assert np.array_equal(s.view(np.int32), ks.view(np.int32)), (dim, n, k)


def test_empty_index_zero_mask_and_argument_errors(require_gpu):
    q = rc.exact_queries(64, 3)
    empty = FlatIndex(dim=64, device=0)
    c, s, i = empty.search_range(q, 4, 0.1)
    assert (c == 0).all() and (i == -1).all() and np.isneginf(s).all() and i.shape == (3, 4)
    dc = torch.ones(3, dtype=torch.int64, device="cuda")
    ds = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    di = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    empty.search_range_device(_dev(q), 4, dc, ds, di)
    torch.cuda.synchronize()
    assert (dc.cpu().numpy() == 0).all() and (di.cpu().numpy() == -1).all() and np.isneginf(ds.cpu().numpy()).all()
    ix, rows, _ = _exact_index(64, 65)
    c, s, i = ix.search_range(q, 4, -INF, _bits(np.zeros(65, bool)))   # an all-zero mask
    assert (c == 0).all() and (i == -1).all() and np.isneginf(s).all()
    for mh in (0, 4097):
        with pytest.raises(ValueError, match=r"max_hits must be in \[1, 4096\] \(got %d\)" % mh):
            ix.search_range(q, mh)
    with pytest.raises(ValueError, match="min_score must not be NaN"):
        ix.search_range(q, 4, float("nan"))
    with pytest.raises(ValueError, match="scratch must be"):
        ix.search_range(q, 4, 0.0, None, torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="bits must be"):
        ix.search_range(q, 4, 0.0, torch.zeros(2, dtype=torch.int32, device="cuda"))
    # the C call's own checks, with a real handle
    oc, os_, oi = np.empty(3, np.int64), np.empty((3, 4), np.float32), np.empty((3, 4), np.int64)
    big = torch.empty(range_scratch_bytes(65, 3, 4), dtype=torch.uint8, device="cuda")

    def call(h, mh, tau, scratch_p, nbytes, bits_p=None):
        return _lib.call("mq_index_search_range", h, _lib.ptr(q), 3, mh, tau, bits_p, _lib.ptr(oc), _lib.ptr(os_),
                         _lib.ptr(oi), 0, scratch_p, nbytes, None)
    with pytest.raises(_lib.MQError, match=r"scratch_bytes 100 is below"):
        call(ix._h, 4, 0.0, _lib.ptr(big), 100)
    with pytest.raises(_lib.MQError, match=r"max_hits must be in \[1, 4096\] \(got 4097\)"):
        call(ix._h, 4097, 0.0, _lib.ptr(big), big.numel())
    with pytest.raises(_lib.MQError, match="min_score must not be NaN"):
        call(ix._h, 4, float("nan"), _lib.ptr(big), big.numel())
    host_bits = np.zeros(3, np.int32)
    with pytest.raises(_lib.MQError, match="the mask must be device memory of the index's GPU 0"):
        call(ix._h, 4, 0.0, _lib.ptr(big), big.numel(), _lib.ptr(host_bits))
    host_scratch = np.zeros(big.numel() + 16, np.uint8)
    aligned = (host_scratch.ctypes.data + 15) & ~15
    with pytest.raises(_lib.MQError, match="scratch must be device memory of the index's GPU 0"):
        call(ix._h, 4, 0.0, _lib.ptr(aligned), big.numel())
    assert call(ix._h, 4, 0.0, _lib.ptr(big), big.numel()) == 0
    odd = FlatIndex(dim=96, device=0)
    odd.add(np.random.default_rng(0).standard_normal((5, 96)).astype(np.float32))
    with pytest.raises(_lib.MQError, match=r"dim <= 1024 \(got 96\)"):
        call(odd._h, 4, 0.0, _lib.ptr(big), big.numel())
    with pytest.raises(ValueError, match=r"got 96"):
        odd.search_range(np.zeros((1, 96), np.float32), 4)


@pytest.mark.parametrize("shape", rc.RANDOM_SHAPES)
def test_random_class_within_the_fp32_bound(require_gpu, shape):
    dim, n = shape
    ix = FlatIndex(dim=dim, device=0)
    ix.add(rc.random_corpus(dim, n))
    stored = ix.get()  # the device-normalised rows are the reference's
    queries = rc.random_queries(dim, rc.RANDOM_NQ)
    s_all = rc.dots64(stored, queries)
    ok = np.ones(n, bool)
    worst = 0.0
    for tau in rc.random_min_scores(dim):
        undecided = positions = 0
        for mh in rc.random_max_hits(n):
            c, s, i = ix.search_range(queries, mh, tau)
            again = ix.search_range(queries, mh, tau)
            assert all(np.array_equal(a.view(np.int64 if a.dtype == np.int64 else np.int32),
                                      b.view(np.int64 if b.dtype == np.int64 else np.int32))
                       for a, b in zip((c, s, i), again))      # repeated calls: the same bits
            for j in range(rc.RANDOM_NQ):
                fails = rc.check_random(int(c[j]), s[j], i[j], s_all[j], ok, tau, mh, dim)
                assert fails == [], (shape, tau, mh, j, fails)
                undecided += rc.undecided_rows(s_all[j], ok, tau, mh, dim)
                positions += rc.returned_positions(s_all[j], ok, tau, mh)
                valid = i[j] >= 0
                worst = max([worst] + np.abs(s[j][valid] - s_all[j][i[j][valid]]).tolist())
        print("random class %s min_score %s: %d undecided of %d positions" % (shape, tau, undecided, positions))
        assert undecided <= rc.NEAR_TIE_CAP * positions, (shape, tau, undecided, positions)
    print("random class %s: worst |score - float64| %.3g (bound %.3g)" % (shape, worst, rc.bound(dim)))


# ------------------------------------------------------------------------ the store ----
STORE_DIM, STORE_N = 64, 5000


class _Emb:
    """Texts are looked up in a table of vectors: the store's batch and text paths embed through
    its function, and the vectors pass through unchanged."""

    def __init__(self, table):
        self.table = table

    def embed_documents(self, texts):
        return [self.table[t].tolist() for t in texts]

    def embed_query(self, text):
        return self.table[text].tolist()


def _store_case(precision="screen"):
    """A store over the exact class: tag = r % 3, and the text says whether r is even."""
    key = ("store", precision)
    if key not in _cache:
        rows = rc.exact_corpus(STORE_DIM, STORE_N)
        queries = rc.exact_queries(STORE_DIM, 24)
        emb = _Emb({"q%d" % j: queries[j] for j in range(len(queries))})
        store = HipChroma(embedding_function=emb, dim=STORE_DIM, auto_persist=False, search_precision=precision)
        store.add_embeddings(rows, ["row %d is %s" % (r, "odd" if r % 2 else "even") for r in range(STORE_N)],
                             [{"tag": r % 3} for r in range(STORE_N)], ["id%d" % r for r in range(STORE_N)])
        assert np.array_equal(store._index.get(), rows)
        _cache[key] = (store, rows, queries, rc.dots64(rows, queries))
    return _cache[key]


def _want(s, mask, tau, limit):
    """-> ([(id, squared L2 distance)], total) of one query's float64 scores."""
    counts, ref_s, ref_i = rc.range_reference(s[None], mask, tau, limit)
    return [("id%d" % r, max(0.0, 2.0 - 2.0 * float(np.float32(x)))) for x, r in zip(ref_s[0], ref_i[0]) if r >= 0], \
        int(counts[0])


def _got(hits):
    return [(d.id, s) for d, s in hits]


def test_store_range_search_filters_batch_total_and_limit(require_gpu):
    store, rows, queries, s_all = _store_case()
    r = np.arange(STORE_N)
    cases = (({}, None),
             ({"filter": {"tag": 1}}, r % 3 == 1),
             ({"where_document": {"$contains": "odd"}}, r % 2 == 1),
             ({"filter": {"tag": {"$ne": 0}}, "where_document": {"$contains": "even"}}, (r % 3 != 0) & (r % 2 == 0)),
             ({"filter": {"tag": 7}}, np.zeros(STORE_N, bool)))
    for kw, mask in cases:
        for tau, limit in ((None, None), (0.25, 200), (0.5, 5), (-0.0, 65), (0.8, 10)):
            for j in (0, 5, 11):
                want, total = _want(s_all[j], mask, -INF if tau is None else tau, 4096 if limit is None else limit)
                got = store.similarity_search_range_with_score("q%d" % j, min_cosine=tau, limit=limit, **kw)
                assert isinstance(got, RangeResult) and _got(got) == want and got.total == total, (kw, tau, limit, j)
                assert store.count_similar("q%d" % j, tau, **kw) == total
        docs = store.similarity_search_range("q3", min_cosine=0.25, limit=30, **kw)
        want, total = _want(s_all[3], mask, 0.25, 30)
        assert [d.id for d in docs] == [i for i, _ in want] and docs.total == total
        assert all(isinstance(d, Document) for d in docs)
        texts = ["q%d" % j for j in range(20)]                  # two passes of the device call
        got = store.similarity_search_range_batch(texts, min_cosine=0.25, limit=70, **kw)
        for j in range(20):
            want, total = _want(s_all[j], mask, 0.25, 70)
            assert [d.id for d in got[j]] == [i for i, _ in want] and got[j].total == total, (kw, j)
    by_vec = store.similarity_search_range_by_vector_with_score(queries[2], 0.25, 100)
    assert _got(by_vec) == _want(s_all[2], None, 0.25, 100)[0]
    assert store.count_similar_by_vector(queries[2], 0.25) == by_vec.total
    # the limit rules: past the constant it raises over 5000 rows and is clipped to a filter's rows
    with pytest.raises(ValueError, match="MQ_RANGE_MAX_HITS=4096"):
        store.similarity_search_range("q1", limit=4097)
    got = store.similarity_search_range("q1", limit=10 ** 6, filter={"tag": 0})
    assert len(got) == got.total == int((r % 3 == 0).sum())
    got = store.similarity_search_range("q1", limit=10 ** 6, where_document={"$contains": "row 49"})
    want, total = _want(s_all[1], np.array(["row 49" in "row %d" % x for x in r]), -INF, 4096)
    assert [d.id for d in got] == [i for i, _ in want] and got.total == total == 111
    with pytest.raises(ValueError, match="min_cosine"):
        store.similarity_search_range("q1", min_cosine=float("nan"))
    # where the k <= 64 search stops, the range search goes on
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.similarity_search("q1", k=200)
    assert len(store.similarity_search_range("q1", limit=200)) == 200


def test_store_retrievers_and_relevance_threshold(require_gpu):
    store, rows, queries, s_all = _store_case()
    plain = store.similarity_search_with_relevance_scores("q2", k=30, filter={"tag": 1})
    cut = sorted({rel for _, rel in plain})[-2]
    want = [(d.id, rel) for d, rel in plain if rel >= cut]
    assert 0 < len(want) < len(plain) == 30
    got = store.similarity_search_with_relevance_scores("q2", k=30, score_threshold=cut, filter={"tag": 1})
    assert [(d.id, rel) for d, rel in got] == want
    ret = store.as_retriever(search_type="similarity_score_threshold",
                             search_kwargs={"score_threshold": cut, "k": 30, "filter": {"tag": 1}})
    assert [d.id for d in ret.invoke("q2")] == [i for i, _ in want]
    with pytest.raises(ValueError, match="score_threshold"):
        store.as_retriever(search_type="similarity_score_threshold", search_kwargs={"k": 30}).invoke("q2")
    ret = store.as_retriever(search_type="range", search_kwargs={"min_cosine": 0.25, "limit": 200,
                                                                 "where_document": {"$contains": "even"}})
    want, total = _want(s_all[4], np.arange(STORE_N) % 2 == 0, 0.25, 200)
    got = ret.invoke("q4")
    assert [d.id for d in got] == [i for i, _ in want] == [d.id for d in ret.get_relevant_documents("q4")]
    assert got.total == total


def test_store_bf16_precision_gives_the_same_range_results(require_gpu):
    store, rows, queries, s_all = _store_case("bf16")
    for j in range(6):
        want, total = _want(s_all[j], None, 0.25, 300)
        got = store.similarity_search_range_by_vector_with_score(queries[j], 0.25, 300)
        assert _got(got) == want and got.total == total
    got = store.similarity_search_range_batch(["q%d" % j for j in range(18)], limit=100, filter={"tag": 2})
    mask = np.arange(STORE_N) % 3 == 2
    for j in range(18):
        want, total = _want(s_all[j], mask, -INF, 100)
        assert [d.id for d in got[j]] == [i for i, _ in want] and got[j].total == total


def test_store_error_cases(require_gpu):
    odd = HipChroma(dim=96, auto_persist=False)
    odd.add_embeddings(np.random.default_rng(0).standard_normal((5, 96)).astype(np.float32), list("abcde"),
                       [{"t": 1}] * 5, list("vwxyz"))
    with pytest.raises(ValueError, match="dim is 96"):
        odd.similarity_search_range_by_vector_with_score(np.ones(96, np.float32), 0.1)
    with pytest.raises(ValueError, match="dim is 96"):
        odd.count_similar_by_vector(np.ones(96, np.float32), 0.1)
    empty = HipChroma(embedding_function=_Emb({}), dim=64, auto_persist=False)
    assert empty.similarity_search_range("q") == [] and empty.count_similar("q", 0.0) == 0
