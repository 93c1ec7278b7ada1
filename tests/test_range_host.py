"""The range search on the host: every argument check of mq_index_search_range answers
MQ_EINVAL and names the offending value before any HIP call (no GPU needed), the scratch size
is monotone and bounded in nq, `RangeResult` keeps its total, and the store's `limit` /
`min_cosine` rules, the relevance-score threshold and the two retriever types hold against a
store whose index is replaced by the float64 reference.

Without a GPU no index handle can be made, so the checks that need the index's shape are
reached through mq_debug_range_check, which runs the same function on a stated (dim, rows);
the checks of the scalars come before the handle is looked at and are reached directly."""
import ctypes
import math

import numpy as np
import pytest

import range_cases as rc
from mediquery_hip import Document, HipChroma, RangeResult, _lib
from mediquery_hip.native import range_scan_blocks, range_scratch_bytes, range_select_blocks

EINVAL = -1
INF = float("inf")


def _aligned(nbytes):
    buf = (ctypes.c_uint8 * (nbytes + 64))()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)


def _check(dim=64, n=10, queries=True, nq=1, max_hits=5, min_score=-INF, out_c=True, out_s=True, out_i=True,
           scratch=True, scratch_bytes=None, scratch_off=0):
    """mq_debug_range_check with sound defaults; True = a valid host buffer of its own."""
    keep = []

    def buf(flag, nbytes):
        if flag is not True:
            return flag
        b, p = _aligned(nbytes)
        keep.append(b)
        return p
    need = range_scratch_bytes(n, nq, max_hits)
    small = min(max(1, nq), 64)  # nothing is read: a refused call needs no room for 2^24 queries
    hits = min(max(1, max_hits), 4096)
    s = buf(scratch, min(need, 1 << 20) + 64)
    if s is not None and scratch_off:
        s = ctypes.c_void_p(s.value + scratch_off)
    return _lib.call("mq_debug_range_check", dim, n, buf(queries, small * min(max(dim, 1), 4096) * 4), nq, max_hits,
                     min_score, buf(out_c, small * 8), buf(out_s, small * hits * 4), buf(out_i, small * hits * 8), s,
                     need if scratch_bytes is None else scratch_bytes)


def _raises(match, **kw):
    with pytest.raises(_lib.MQError, match=match) as e:
        _check(**kw)
    assert e.value.code == EINVAL


def test_constant_is_the_headers():
    assert _lib.MQ_RANGE_MAX_HITS == 4096
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mq.h")
    assert "#define MQ_RANGE_MAX_HITS 4096" in open(header).read()


def test_scalar_checks_come_before_the_handle():
    """No handle, no buffers: max_hits, a NaN min_score and nq are refused first, then the NULL
    index."""
    def call(nq, max_hits, min_score):
        return _lib.call("mq_index_search_range", None, None, nq, max_hits, min_score, None, None, None, None, 0,
                         None, 0, None)
    for mh in (0, 4097, -3):
        with pytest.raises(_lib.MQError, match=r"max_hits must be in \[1, 4096\] \(got %d\)" % mh) as e:
            call(1, mh, 0.5)
        assert e.value.code == EINVAL
    with pytest.raises(_lib.MQError, match=r"min_score must not be NaN") as e:
        call(1, 5, float("nan"))
    assert e.value.code == EINVAL
    with pytest.raises(_lib.MQError, match=r"query count -1 out of range"):
        call(-1, 5, 0.5)
    for tau in (-INF, INF, 0.5):
        with pytest.raises(_lib.MQError, match="NULL index") as e:
            call(1, 5, tau)
        assert e.value.code == EINVAL


def test_every_shape_and_buffer_check_names_its_value():
    assert _check() == 0
    for mh in (0, 4097):
        _raises(r"max_hits must be in \[1, 4096\] \(got %d\)" % mh, max_hits=mh)
    for mh in (1, 64, 65, 4096):
        assert _check(max_hits=mh) == 0
    _raises("min_score must not be NaN", min_score=float("nan"))
    for tau in (-INF, -0.0, 0.25, INF):
        assert _check(min_score=tau) == 0
    for dim in (0, 32, 96, 1088, 2048, -64):
        _raises(r"dim %% 64 == 0, dim <= 1024 \(got %d\)" % dim, dim=dim)
    for dim in (64, 256, 768, 1024):
        assert _check(dim=dim) == 0
    _raises(r"fewer than 2\^31 rows \(got 2147483648\)", n=1 << 31)
    _raises(r"query count %d out of range" % ((1 << 24) + 1), nq=(1 << 24) + 1)
    # NULL pointers with rows in the index
    _raises("NULL queries", queries=None)
    _raises("NULL output buffer", out_c=None)
    _raises("NULL output buffer", out_s=None)
    _raises("NULL output buffer", out_i=None)
    _raises("NULL scratch", scratch=None)
    # the scratch: aligned, large enough, and none of the outputs
    _raises(r"scratch must be 16-byte aligned \(got 0x[0-9a-f]+8\)", scratch_off=8)
    need = range_scratch_bytes(10, 1, 5)
    _raises(r"scratch_bytes %d is below the %d bytes mq_range_scratch_bytes\(10, 1, 5\) asks" % (need - 1, need),
            scratch_bytes=need - 1)
    _raises(r"scratch_bytes 0 is below", scratch_bytes=0)
    _raises(r"scratch_bytes -5 is below", scratch_bytes=-5)
    buf, p = _aligned(need + 64)
    _raises(r"scratch overlaps out_counts \(0x[0-9a-f]+\)", scratch=p, out_c=ctypes.c_void_p(p.value + need - 8))
    _raises(r"scratch overlaps out_scores \(0x[0-9a-f]+\)", scratch=p, out_s=p)
    _raises(r"scratch overlaps out_ids \(0x[0-9a-f]+\)", scratch=p, out_i=ctypes.c_void_p(p.value + 256))
    # what needs no buffer: no queries; an empty index returns zero counts and padding without
    # reading the scratch (the outputs are still required)
    assert _check(nq=0, queries=None, out_c=None, out_s=None, out_i=None, scratch=None, scratch_bytes=0) == 0
    assert _check(n=0, scratch=None, scratch_bytes=0) == 0
    _raises("NULL output buffer", n=0, out_c=None)
    _raises(r"max_hits must be in", nq=0, max_hits=0)


def test_range_scratch_bytes_is_monotone_and_bounded_in_nq():
    f = range_scratch_bytes
    base = f(1000, 4, 8)
    assert base > 0 and base % 256 == 0
    for more in (f(10 ** 6, 4, 8), f(1000, 16, 8), f(1000, 4, 4096)):
        assert more >= base
    sizes = [f(10 ** 5, nq, 4096) for nq in (0, 1, 2, 15, 16, 17, 40, 256, 4096, 10 ** 9)]
    assert sizes == sorted(sizes) and sizes[0] == 0
    assert f(10 ** 5, 16, 64) == f(10 ** 5, 17, 64) == f(10 ** 5, 1 << 40, 64)  # the passes reuse the keys
    sizes = [f(n, 16, 4096) for n in (0, 1, 255, 256, 4097, 10 ** 5, 10 ** 6, 10 ** 8, (1 << 31) - 1)]
    assert sizes == sorted(sizes)
    sizes = [f(10 ** 5, 16, mh) for mh in (1, 5, 64, 65, 1000, 4096)]
    assert sizes == sorted(sizes)
    # the keys are 4 bytes per (query of a pass, row); everything else stays under 1 MB: about 65 MB
    # at a million rows
    assert 16 * 10 ** 6 * 4 <= f(10 ** 6, 256, 4096) < 16 * 10 ** 6 * 4 + (1 << 20)
    # arguments out of range are clamped
    assert f(1000, 4, 0) == f(1000, 4, 1) and f(1000, 4, 10 ** 6) == f(1000, 4, 4096)
    assert f(-5, -1, 8) == f(0, 0, 8) == 0 and f(1 << 40, 16, 8) == f((1 << 31) - 1, 16, 8)


def test_scan_and_select_geometry():
    assert range_scan_blocks(0, 256) == 1 and range_scan_blocks(129, 256) == 2
    assert range_scan_blocks(10 ** 6, 256) == 512 and range_scan_blocks(10 ** 6, 0) == 2
    assert range_select_blocks(0, 256) == 1 and range_select_blocks(4096, 256) == 1
    assert range_select_blocks(4097, 256) == 2 and range_select_blocks(10 ** 6, 256) == 245
    assert range_select_blocks(10 ** 7, 256) == 256 and range_select_blocks(10 ** 7, 0) == 1


def test_range_result():
    r = RangeResult(["a", "b"], total=7)
    assert r == ["a", "b"] and isinstance(r, list) and r.total == 7 and len(r) == 2
    assert RangeResult().total == 0 and RangeResult() == []
    assert RangeResult(["x"]).total == 1
    assert r[0] == "a" and [x for x in r] == ["a", "b"] and r.total >= len(r)
    with pytest.raises(ValueError, match="total 1 is below the 2 entries"):
        RangeResult(["a", "b"], total=1)


# ------------------------------------------------- the store over a reference index ----
DIM, N = 64, 5000


class _Emb:
    def __init__(self, table):
        self.table = table

    def embed_documents(self, texts):
        return [self.table[t].tolist() for t in texts]

    def embed_query(self, text):
        return self.table[text].tolist()


class _RefIndex:
    """FlatIndex's search and search_range, answered by the float64 reference."""

    def __init__(self, rows):
        self.rows, self.dim, self.calls = rows, rows.shape[1], []

    def __len__(self):
        return len(self.rows)

    def search_range(self, queries, max_hits, min_score=-INF, bits=None, scratch=None):
        assert 1 <= max_hits <= _lib.MQ_RANGE_MAX_HITS and not math.isnan(min_score)
        self.calls.append((len(queries), max_hits, min_score, bits is not None))
        c, s, i = rc.range_reference(rc.dots64(self.rows, queries), bits, min_score, max_hits)
        return c, s.astype(np.float32), i

    def search(self, queries, k):
        assert 1 <= k <= _lib.MQ_MAX_K
        _, s, i = rc.range_reference(rc.dots64(self.rows, queries), None, -INF, k)
        return s.astype(np.float32), i


class _Store(HipChroma):
    """HipChroma with the device behind it replaced: the index is `_RefIndex`, a filter
    {"tag": t} is the host mask r % 3 == t, and no scratch is made."""

    def __init__(self, rows, queries, **kw):
        super().__init__(embedding_function=_Emb({"q%d" % j: queries[j] for j in range(len(queries))}), dim=DIM,
                         auto_persist=False, **kw)
        n = len(rows)
        self._index = _RefIndex(rows)
        self._ids = ["id%d" % r for r in range(n)]
        self._texts = ["row %d" % r for r in range(n)]
        self._metas = [{"tag": r % 3} for r in range(n)]

    def _range_room(self, n, nq, limit):
        return None

    def _admit(self, k, filter, where_document):
        assert where_document is None
        return k, np.arange(len(self._ids)) % 3 == filter["tag"]

    def _mask_rows(self, bits):
        return bits


@pytest.fixture(scope="module")
def store():
    rows, queries = rc.exact_corpus(DIM, N), rc.exact_queries(DIM, 6)
    return _Store(rows, queries), rows, queries, rc.dots64(rows, queries)


def _want(s, mask, tau, limit):
    counts, ref_s, ref_i = rc.range_reference(s[None], mask, tau, limit)
    return [("id%d" % r, max(0.0, 2.0 - 2.0 * float(np.float32(x)))) for x, r in zip(ref_s[0], ref_i[0]) if r >= 0], \
        int(counts[0])


def test_store_range_search_limit_rules(store):
    st, rows, queries, s = store
    # no limit: MQ_RANGE_MAX_HITS, clipped to the rows
    got = st.similarity_search_range_by_vector_with_score(queries[0])
    want, total = _want(s[0], None, -INF, 4096)
    assert isinstance(got, RangeResult) and [(d.id, x) for d, x in got] == want and got.total == total == N
    assert st._index.calls[-1] == (1, 4096, -INF, False)
    got = st.similarity_search_range_with_score("q1", min_cosine=0.25, limit=200)
    want, total = _want(s[1], None, 0.25, 200)
    assert [(d.id, x) for d, x in got] == want and got.total == total > len(got) == 200
    assert all(a[1] <= b[1] for a, b in zip(got[:-1], got[1:]))  # nearest first
    # a limit past the constant raises when the candidates are that many
    with pytest.raises(ValueError, match=r"limit=4097 over 5000 rows\) exceeds .* MQ_RANGE_MAX_HITS=4096"):
        st.similarity_search_range("q1", limit=4097)
    with pytest.raises(ValueError, match="MQ_RANGE_MAX_HITS"):
        st.similarity_search_range_batch(["q1", "q2"], min_cosine=0.5, limit=10 ** 6)
    # and is clipped when the filter admits fewer: 1667 rows have tag 0
    mask = np.arange(N) % 3 == 0
    got = st.similarity_search_range("q2", limit=10 ** 6, filter={"tag": 0})
    want, total = _want(s[2], mask, -INF, int(mask.sum()))
    assert [d.id for d in got] == [i for i, _ in want] and got.total == total == mask.sum() == len(got)
    assert st._index.calls[-1] == (1, int(mask.sum()), -INF, True)
    assert all(isinstance(d, Document) and d.metadata == {"tag": 0} for d in got)
    # limit <= 0: the count alone
    got = st.similarity_search_range("q3", min_cosine=0.0, limit=0)
    assert got == [] and got.total == _want(s[3], None, 0.0, 1)[1] > 0
    # the batch: one encoder batch, one device call
    before = len(st._index.calls)
    got = st.similarity_search_range_batch(["q0", "q4", "q5"], min_cosine=0.25, limit=7)
    assert len(st._index.calls) == before + 1 and st._index.calls[-1] == (3, 7, 0.25, False)
    for j, hits in zip((0, 4, 5), got):
        want, total = _want(s[j], None, 0.25, 7)
        assert [d.id for d in hits] == [i for i, _ in want] and hits.total == total
    assert st.similarity_search_range_batch([]) == []


def test_store_count_similar(store):
    st, rows, queries, s = store
    for j, tau in ((0, 0.25), (1, -0.0), (2, 0.8), (3, None)):
        want = _want(s[j], None, -INF if tau is None else tau, 1)[1]
        assert st.count_similar("q%d" % j, tau) == want == st.count_similar_by_vector(queries[j], tau)
        assert isinstance(st.count_similar("q%d" % j, tau), int)
        assert st._index.calls[-1][1] == 1
    mask = np.arange(N) % 3 == 1
    assert st.count_similar("q0", 0.0, filter={"tag": 1}) == _want(s[0], mask, 0.0, 1)[1]


def test_store_refuses_a_bad_min_cosine_limit_and_dim(store):
    st = store[0]
    before = len(st._index.calls)
    for bad in (float("nan"), INF, -INF, "0.5", True, [0.5]):
        with pytest.raises(ValueError, match="min_cosine must be None or a finite number"):
            st.similarity_search_range("q0", min_cosine=bad)
        with pytest.raises(ValueError, match="min_cosine"):
            st.count_similar("q0", bad)
        with pytest.raises(ValueError, match="min_cosine"):
            st.similarity_search_range_batch(["q0"], min_cosine=bad)
    assert len(st._index.calls) == before
    assert len(st.similarity_search_range("q0", min_cosine=np.float32(0.25), limit=3)) == 3
    with pytest.raises(ValueError, match="where_document"):
        st.similarity_search_range("q0", where_document={"$has": "x"})
    odd = _Store(np.zeros((4, 96), np.float32), np.zeros((1, 96), np.float32))
    odd._dim = 96
    with pytest.raises(ValueError, match="dim is 96"):
        odd.similarity_search_range_by_vector_with_score(np.ones(96, np.float32))
    empty = HipChroma(embedding_function=_Emb({}), dim=DIM, auto_persist=False)
    got = empty.similarity_search_range("anything", min_cosine=0.1)
    assert got == [] and got.total == 0 and empty.count_similar("anything", 0.1) == 0
    assert empty.similarity_search_range_batch(["a", "b"]) == [[], []]


def test_relevance_score_threshold_filters_the_top_k(store):
    st, rows, queries, s = store
    plain = st.similarity_search_with_relevance_scores("q1", k=20)
    assert len(plain) == 20 and all(a[1] >= b[1] for a, b in zip(plain[:-1], plain[1:]))
    rel = sorted({r for _, r in plain})
    assert len(rel) >= 2
    cut = rel[-1]  # the best relevance: a threshold that removes documents the plain search returns
    got = st.similarity_search_with_relevance_scores("q1", k=20, score_threshold=cut)
    assert 0 < len(got) < 20 and [(d.id, r) for d, r in got] == [(d.id, r) for d, r in plain if r >= cut]
    assert st.similarity_search_with_relevance_scores("q1", k=20, score_threshold=2.0) == []
    assert len(st.similarity_search_with_relevance_scores("q1", k=20, score_threshold=-5)) == 20
    assert len(st.similarity_search_with_relevance_scores("q1", k=20, score_threshold=None)) == 20
    for bad in ("0.5", float("nan"), [1], True):
        with pytest.raises(ValueError, match="score_threshold must be a number"):
            st.similarity_search_with_relevance_scores("q1", k=5, score_threshold=bad)
    with pytest.raises(ValueError, match="MQ_MAX_K"):  # k keeps its rule
        st.similarity_search_with_relevance_scores("q1", k=65, score_threshold=0.1)
    # any relevance_score_fn
    other = _Store(rows, queries, relevance_score_fn=lambda d: -d)
    every = other.similarity_search_with_relevance_scores("q1", k=20)
    cut = max(r for _, r in every)
    got = other.similarity_search_with_relevance_scores("q1", k=20, score_threshold=cut)
    assert [(d.id, r) for d, r in got] == [(d.id, r) for d, r in every if r >= cut] and 0 < len(got) < 20


def test_the_two_new_retriever_types(store):
    st, rows, queries, s = store
    plain = st.similarity_search_with_relevance_scores("q2", k=30)
    cut = sorted({r for _, r in plain})[-2]
    want = [d.id for d, r in plain if r >= cut]
    assert 0 < len(want) < 30
    ret = st.as_retriever(search_type="similarity_score_threshold", search_kwargs={"score_threshold": cut, "k": 30})
    assert [d.id for d in ret.invoke("q2")] == want
    assert [d.id for d in st.as_retriever(search_kwargs={"k": 30}).invoke("q2")] == [d.id for d, _ in plain]
    # LangChain's ValueError: the threshold missing, or no float
    for kw in ({}, {"k": 5}, {"score_threshold": None}, {"score_threshold": "0.5"}, {"score_threshold": 1}):
        with pytest.raises(ValueError, match="score_threshold"):
            st.as_retriever(search_type="similarity_score_threshold", search_kwargs=kw).invoke("q2")
    # the default k
    ret = st.as_retriever(search_type="similarity_score_threshold", search_kwargs={"score_threshold": -5.0})
    assert [d.id for d in ret.invoke("q2")] == [d.id for d, _ in plain[:4]]
    # "range": min_cosine, limit and filter go to similarity_search_range
    ret = st.as_retriever(search_type="range", search_kwargs={"min_cosine": 0.25, "limit": 200, "filter": {"tag": 2}})
    got = ret.invoke("q3")
    want, total = _want(s[3], np.arange(N) % 3 == 2, 0.25, 200)
    assert [d.id for d in got] == [i for i, _ in want] and got.total == total
    assert [d.id for d in ret.get_relevant_documents("q3")] == [i for i, _ in want]
    assert len(st.as_retriever(search_type="range").invoke("q3")) == 4096
