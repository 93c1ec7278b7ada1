"""The device group scan (K16, csrc/grouped.hip) against the float64 restatement of the
definition (tests/grouped_cases.py): bit-for-bit equality on the exact class - ids, scores,
which duplicate represents a group, the order of tied groups, the padding - over the row
counts, dims, batch sizes, k, group layouts and masks at which the kernels change path; the
bound of the random class; then HipChroma's grouped search (certificate and scan), and the
parent-document retriever the feature exists for.

What the device showed on the random class (MI355X; the test prints the figures): the worst
|score - float64| over the seven cases was 5.0e-8 at dim 64 (bound 4.3e-6), 2.1e-8 at 256 and
768 (bounds 1.6e-5, 4.6e-5) and 1.8e-8 at 1024 (6.2e-5);
near-tie positions 2-15 of 1104-1173 per case (at most 1.3 %, cap 5 %)."""
import numpy as np
import pytest
import torch

import grouped_cases as gc
from mediquery_hip import Document, HipChroma, HipParentDocumentRetriever, WindowSplitter, _lib
from mediquery_hip.native import FlatIndex, group_scan_blocks, group_scratch_bytes

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 4097)
DIMS = (64, 256, 768, 1024)
NQS = (1, 2, 16, 17, 40)   # 17 and 40 cross the 16-query pass boundary
KS = (1, 5, 64)
_cache = {}


def _exact_index(dim, n):
    """(index, rows, float64 scores of the 40 exact queries) of an exact-class corpus; the
    index holds the rows bit for bit - the precondition of every equality."""
    key = (dim, n)
    if key not in _cache:
        rows = gc.exact_corpus(dim, n)
        ix = FlatIndex(dim=dim, device=0)
        ix.add(rows)
        assert np.array_equal(ix.get(), rows)
        _cache[key] = (ix, rows, gc.dots64(rows, gc.exact_queries(dim, max(NQS))))
    return _cache[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached corpora are read-only


def _bits(mask):
    return None if mask is None else _dev(gc.mask_words(mask))


def _same(gs, gi, ref_s, ref_i, where):
    assert np.array_equal(gi, ref_i), where
    assert np.array_equal(gs, ref_s.astype(np.float32)), where


@pytest.mark.parametrize("dim", DIMS)
def test_exact_class_equals_reference(require_gpu, dim):
    queries = gc.exact_queries(dim, max(NQS))
    seen = set()
    for ni, n in enumerate(NS):
        ix, rows, s_all = _exact_index(dim, n)
        for li, layout in enumerate(gc.LAYOUTS):
            codes, g = gc.group_codes(layout, n)
            dcodes = _dev(codes)
            for mi, mk in enumerate(gc.MASKS):
                # every n meets every nq and every k, and each (layout, mask) pair meets several
                nq, k = NQS[(li + mi + ni) % len(NQS)], KS[(2 * li + mi + ni) % len(KS)]
                mask = gc.row_mask(mk, n)
                ref_s, ref_i = gc.grouped_reference(rows, queries[:nq], codes, mask, k, g, scores=s_all[:nq])
                gs, gi = ix.search_grouped(queries[:nq], k, dcodes, g, _bits(mask))
                _same(gs, gi, ref_s, ref_i, (dim, n, layout, mk, nq, k))
                seen.add((n, nq)), seen.add((n, "k", k))
                if (ref_i < 0).any():
                    seen.add("pads")
    assert all((n, nq) in seen and (n, "k", k) in seen for n in NS for nq in NQS for k in KS) and "pads" in seen


def test_ties_pick_the_lowest_row_and_order_tied_groups_by_it(require_gpu):
    """Every row the same vector: all scores are 1, so each group is represented by its lowest
    admitted row and the groups come in the order of those rows."""
    dim, n = 64, 300
    q = gc.exact_queries(dim, 1)
    ix = FlatIndex(dim=dim, device=0)
    ix.add(np.repeat(q, n, axis=0))
    codes = ((np.arange(n) * 7) % 11).astype(np.int32)          # interleaved, not in row order
    gs, gi = ix.search_grouped(q, 64, _dev(codes), 11)
    want = sorted(int(np.flatnonzero(codes == c)[0]) for c in range(11))
    assert gi[0, :11].tolist() == want and (gi[0, 11:] == -1).all()
    assert (gs[0, :11] == 1.0).all() and np.isneginf(gs[0, 11:]).all()
    mask = np.ones(n, bool)
    mask[:40] = False                                           # the lowest rows are masked out
    gs, gi = ix.search_grouped(q, 5, _dev(codes), 11, _bits(mask))
    assert gi[0].tolist() == sorted(int(np.flatnonzero((codes == c) & mask)[0]) for c in range(11))[:5]


def test_large_case_walks_every_workgroups_loop_twice_and_both_tails(require_gpu):
    """Row count from the launch geometry: 2 x CUs workgroups of 16 lane groups, two rows per
    iteration; n = 9 G + 37 gives every lane group five iterations, the last with two rows in
    flight for 37 lane groups and one for the rest."""
    dim = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = 16 * 2 * cus
    n = 9 * G + 37
    assert group_scan_blocks(n, cus) == 2 * cus
    rows = gc.exact_corpus(dim, n)
    ix = FlatIndex(dim=dim, device=0)
    ix.add(rows)
    assert np.array_equal(ix.get(), rows)
    queries = gc.exact_queries(dim, 17)
    s_all = gc.dots64(rows, queries)
    for layout, mk, k in (("families", "none", 5), ("sprinkled", "third", 64), ("singletons", "none", 64)):
        codes, g = gc.group_codes(layout, n)
        mask = gc.row_mask(mk, n)
        ref_s, ref_i = gc.grouped_reference(rows, queries, codes, mask, k, g, scores=s_all)
        gs, gi = ix.search_grouped(queries, k, _dev(codes), g, _bits(mask))
        _same(gs, gi, ref_s, ref_i, (n, layout, mk, k))
        assert (ref_i >= 8 * G).any() or layout != "singletons"  # the last iteration's rows are reachable


def test_host_and_device_outputs_agree_and_repeat_bitwise(require_gpu):
    dim, n, nq, k = 256, 4097, 40, 64
    ix, rows, s_all = _exact_index(dim, n)
    queries = gc.exact_queries(dim, nq)
    codes, g = gc.group_codes("sprinkled", n)
    mask = gc.row_mask("third", n)
    dcodes, bits = _dev(codes), _bits(mask)
    ref_s, ref_i = gc.grouped_reference(rows, queries, codes, mask, k, g, scores=s_all)
    scratch = torch.empty(group_scratch_bytes(g, nq, k), dtype=torch.uint8, device="cuda")
    hs, hi = ix.search_grouped(queries, k, dcodes, g, bits, scratch)
    _same(hs, hi, ref_s, ref_i, "host")
    dq = _dev(queries)
    out = [(torch.empty((nq, k), dtype=torch.float32, device="cuda"),
            torch.empty((nq, k), dtype=torch.int64, device="cuda")) for _ in range(3)]
    # two calls in a row on one scratch (the table is zeroed again), then one that follows a
    # call with other queries and no mask on the same scratch
    ix.search_grouped_device(dq, k, dcodes, g, out[0][0], out[0][1], bits, scratch)
    ix.search_grouped_device(dq, k, dcodes, g, out[1][0], out[1][1], bits, scratch)
    ix.search_grouped(queries[::-1].copy(), k, dcodes, g, None, scratch)
    ix.search_grouped_device(dq, k, dcodes, g, out[2][0], out[2][1], bits, scratch)
    torch.cuda.synchronize()
    for s, i in out:
        assert np.array_equal(i.cpu().numpy(), hi)
        assert np.array_equal(s.cpu().numpy().view(np.int32), hs.view(np.int32))
    # a query alone gives what it gives inside the batch
    s1, i1 = ix.search_grouped(queries[20:21], k, dcodes, g, bits)
    assert np.array_equal(i1[0], hi[20]) and np.array_equal(s1[0], hs[20])


def test_empty_index_no_groups_and_argument_errors(require_gpu):
    q = gc.exact_queries(64, 3)
    empty = FlatIndex(dim=64, device=0)
    none = torch.empty(0, dtype=torch.int32, device="cuda")
    gs, gi = empty.search_grouped(q, 4, none, 7)
    assert (gi == -1).all() and np.isneginf(gs).all() and gi.shape == (3, 4)
    ds = torch.zeros((3, 4), dtype=torch.float32, device="cuda")
    di = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    empty.search_grouped_device(_dev(q), 4, none, 7, ds, di)
    torch.cuda.synchronize()
    assert (di.cpu().numpy() == -1).all() and np.isneginf(ds.cpu().numpy()).all()
    ix, rows, _ = _exact_index(64, 65)
    codes = _dev(np.zeros(65, np.int32))
    gs, gi = ix.search_grouped(q, 4, codes, 0)                  # n_groups == 0: padding only
    assert (gi == -1).all() and np.isneginf(gs).all()
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\] \(got %d\)" % k):
            ix.search_grouped(q, k, codes, 1)
    with pytest.raises(ValueError, match="codes must be"):
        ix.search_grouped(q, 4, codes[:64], 1)
    with pytest.raises(ValueError, match="scratch must be"):
        ix.search_grouped(q, 4, codes, 1, None, torch.empty(16, dtype=torch.uint8, device="cuda"))
    # the C call's own checks, with a real handle
    os_, oi = np.empty((3, 4), np.float32), np.empty((3, 4), np.int64)
    big = torch.empty(group_scratch_bytes(1, 3, 4), dtype=torch.uint8, device="cuda")

    def call(h, codes_p, scratch_p, nbytes):
        return _lib.call("mq_index_search_grouped", h, _lib.ptr(q), 3, 4, codes_p, 1, None, _lib.ptr(os_),
                         _lib.ptr(oi), 0, scratch_p, nbytes, None)
    with pytest.raises(_lib.MQError, match=r"scratch_bytes 100 is below"):
        call(ix._h, _lib.ptr(codes), _lib.ptr(big), 100)
    host_codes = np.zeros(65, np.int32)
    with pytest.raises(_lib.MQError, match="codes must be device memory of the index's GPU 0"):
        call(ix._h, _lib.ptr(host_codes), _lib.ptr(big), big.numel())
    odd = FlatIndex(dim=96, device=0)
    odd.add(np.random.default_rng(0).standard_normal((5, 96)).astype(np.float32))
    with pytest.raises(_lib.MQError, match=r"dim <= 1024 \(got 96\)"):
        call(odd._h, _lib.ptr(codes), _lib.ptr(big), big.numel())
    with pytest.raises(ValueError, match=r"got 96"):
        odd.search_grouped(np.zeros((1, 96), np.float32), 4, codes, 1)


@pytest.mark.parametrize("case", gc.RANDOM_CASES)
def test_random_class_within_the_fp32_bound(require_gpu, case):
    dim, n, layout, mk, nq, seed = case
    ix = FlatIndex(dim=dim, device=0)
    ix.add(gc.random_corpus(dim, n, seed))
    stored = ix.get()  # the device-normalised rows are the reference's
    queries = gc.random_queries(dim, nq, seed)
    codes, g = gc.group_codes(layout, n, seed)
    mask = gc.row_mask(mk, n)
    ok = gc.candidates(codes, mask, g)
    s_all = gc.dots64(stored, queries)
    near = positions = 0
    worst = 0.0
    for k in gc.RANDOM_KS:
        ref_s, ref_i = gc.grouped_reference(stored, queries, codes, mask, k, g, scores=s_all)
        gs, gi = ix.search_grouped(queries, k, _dev(codes), g, _bits(mask))
        for j in range(nq):
            fails, nt = gc.check_random(gs[j], gi[j], s_all[j], codes, ok, ref_s[j], ref_i[j], dim)
            assert fails == [], (case, k, j, fails)
            near += int(nt.sum())
            valid = gi[j] >= 0
            worst = max([worst] + np.abs(gs[j][valid] - s_all[j][gi[j][valid]]).tolist())
        positions += nq * k
    print("random class %s: worst |score - float64| %.3g (bound %.3g), near-tie positions %d of %d"
          % (case, worst, gc.bound(dim), near, positions))
    assert near <= gc.NEAR_TIE_CAP * positions, (case, near, positions)


# ------------------------------------------------------------------------ the store ----
STORE_DIM, STORE_N = 64, 1000


class _Emb:
    """Texts are looked up in a table of vectors: the store's batch and text paths embed through
    its function, and the vectors pass through unchanged."""

    def __init__(self, table):
        self.table = table

    def embed_documents(self, texts):
        return [self.table[t].tolist() for t in texts]

    def embed_query(self, text):
        return self.table[text].tolist()


def _store_case(precision="screen", layout="sprinkled"):
    """A store over the exact class: row r's parent is its code of `layout` ("doc_id" absent
    where the code is out of range), tag = r % 3, and the text says whether r is even."""
    key = ("store", precision, layout)
    if key not in _cache:
        rows = gc.exact_corpus(STORE_DIM, STORE_N)
        codes, g = gc.group_codes(layout, STORE_N)
        codes = np.where((codes >= 0) & (codes < g), codes, -1).astype(np.int32)
        queries = gc.exact_queries(STORE_DIM, 24)
        emb = _Emb({"q%d" % j: queries[j] for j in range(len(queries))})
        store = HipChroma(embedding_function=emb, dim=STORE_DIM, auto_persist=False, search_precision=precision)
        metas = [dict({"tag": r % 3}, **({"doc_id": "p%d" % codes[r]} if codes[r] >= 0 else {}))
                 for r in range(STORE_N)]
        store.add_embeddings(rows, ["row %d is %s" % (r, "odd" if r % 2 else "even") for r in range(STORE_N)], metas,
                             ["id%d" % r for r in range(STORE_N)])
        assert np.array_equal(store._index.get(), rows)
        _cache[key] = (store, rows, codes, queries, gc.dots64(rows, queries))
    return _cache[key]


def _want(rows, queries, codes, mask, k, s_all, j):
    ref_s, ref_i = gc.grouped_reference(rows, queries[j:j + 1], codes, mask, k, scores=s_all[j:j + 1])
    return [("id%d" % r, max(0.0, 2.0 - 2.0 * float(np.float32(x)))) for x, r in zip(ref_s[0], ref_i[0]) if r >= 0]


def _got(hits):
    return [(d.id, s) for d, s in hits]


def _certifies(s, codes, mask, k):
    """Whether the float64 top-64 of the candidate rows holds k distinct groups (or is short)."""
    ok = gc.candidates(codes, mask)
    rows = np.flatnonzero(ok)
    top = rows[np.lexsort((rows, -s[rows]))][:_lib.MQ_MAX_K]
    return len(top) < _lib.MQ_MAX_K or len(set(codes[top].tolist())) >= k


def test_store_certificate_and_forced_scan_agree_and_group_scans_counts(require_gpu):
    store, rows, codes, queries, s_all = _store_case()
    outcomes = set()
    for k in (1, 5, 20):
        for j in range(len(queries)):
            want = _want(rows, queries, codes, None, k, s_all, j)
            before = store.group_scans
            got = _got(store.similarity_search_grouped_by_vector_with_score(queries[j], k))
            scanned = store.group_scans - before
            cert = _certifies(s_all[j], codes, None, k)
            assert scanned == (0 if cert else 1), (k, j)
            outcomes.add(cert)
            assert got == want, (k, j, "certified" if cert else "scanned")
            before = store.group_scans
            assert _got(store.similarity_search_grouped_by_vector_with_score(queries[j], k, _force_scan=True)) == want
            assert store.group_scans == before + 1
    assert True in outcomes


def test_store_scans_when_one_parent_owns_the_top_64(require_gpu):
    """70 copies of the query under one parent: the top 64 rows hold a single group, so k = 3
    cannot be certified and goes to the scan; k = 1 is certified."""
    rows = gc.exact_corpus(STORE_DIM, 400)
    q = gc.exact_queries(STORE_DIM, 2)
    allrows = np.concatenate([np.repeat(q[:1], 70, axis=0), rows])
    codes = np.concatenate([np.zeros(70, np.int32), 1 + gc.group_codes("families", 400)[0]])
    emb = _Emb({"hit": q[0], "other": q[1]})
    store = HipChroma(embedding_function=emb, dim=STORE_DIM, auto_persist=False)
    store.add_embeddings(allrows, ["t%d" % r for r in range(470)], [{"doc_id": "p%d" % c} for c in codes],
                         ["id%d" % r for r in range(470)])
    s_all = gc.dots64(allrows, q)
    assert (np.sort(s_all[0])[::-1][:64] == 1.0).all() and not _certifies(s_all[0], codes, None, 3)
    want = _want(allrows, q, codes, None, 3, s_all, 0)
    assert want[0] == ("id0", 0.0) and len(want) == 3
    assert _got(store.similarity_search_grouped_with_score("hit", k=3)) == want and store.group_scans == 1
    assert [d.id for d in store.similarity_search_grouped("hit", k=1)] == ["id0"] and store.group_scans == 1
    # a batch sends only its uncertified queries to the scan
    cert1 = _certifies(s_all[1], codes, None, 3)
    got = store.similarity_search_grouped_batch(["hit", "other", "hit"], k=3)
    assert store.group_scans == 1 + 2 + (0 if cert1 else 1)
    assert [d.id for d in got[0]] == [i for i, _ in want] == [d.id for d in got[2]]
    assert [d.id for d in got[1]] == [i for i, _ in _want(allrows, q, codes, None, 3, s_all, 1)]


def test_store_filter_where_document_batch_and_retriever(require_gpu):
    store, rows, codes, queries, s_all = _store_case()
    r = np.arange(STORE_N)
    cases = (({"filter": {"tag": 1}}, r % 3 == 1),
             ({"where_document": {"$contains": "odd"}}, r % 2 == 1),
             ({"filter": {"tag": {"$ne": 0}}, "where_document": {"$contains": "even"}}, (r % 3 != 0) & (r % 2 == 0)),
             ({"filter": {"tag": 7}}, np.zeros(STORE_N, bool)))
    for kw, mask in cases:
        for k in (1, 5, 30):
            for j in (0, 5, 11):
                want = _want(rows, queries, codes, mask, k, s_all, j)
                assert _got(store.similarity_search_grouped_with_score("q%d" % j, k=k, **kw)) == want, (kw, k, j)
                assert _got(store.similarity_search_grouped_with_score("q%d" % j, k=k, _force_scan=True, **kw)) == want
    texts = ["q%d" % j for j in range(20)]
    for kw, mask in cases[:3] + (({}, None),):
        got = store.similarity_search_grouped_batch(texts, k=5, **kw)
        forced = store.similarity_search_grouped_batch(texts, k=5, _force_scan=True, **kw)
        for j in range(20):
            want = [i for i, _ in _want(rows, queries, codes, mask, 5, s_all, j)]
            assert [d.id for d in got[j]] == want and [d.id for d in forced[j]] == want, (kw, j)
    # the plain forms, another key, a key no row has, k <= 0
    want = _want(rows, queries, codes, None, 4, s_all, 2)
    assert [d.id for d in store.similarity_search_grouped("q2")] == [i for i, _ in want]  # DEFAULT_K = 4
    by_tag = store.similarity_search_grouped("q2", k=9, group_by="tag")
    assert sorted(d.metadata["tag"] for d in by_tag) == [0, 1, 2]
    assert _got(store.similarity_search_grouped_with_score("q2", k=9, group_by="tag")) == \
        _want(rows, queries, (r % 3).astype(np.int32), None, 9, s_all, 2)
    assert store.similarity_search_grouped("q2", group_by="no_such_key") == []
    assert store.similarity_search_grouped("q2", k=0) == []
    assert store.similarity_search_grouped_batch([], k=3) == []
    # the retriever is routed like the lexical types
    ret = store.as_retriever(search_type="grouped", search_kwargs={"k": 3, "filter": {"tag": 1}})
    want = [i for i, _ in _want(rows, queries, codes, r % 3 == 1, 3, s_all, 4)]
    assert [d.id for d in ret.invoke("q4")] == want == [d.id for d in ret.get_relevant_documents("q4")]
    assert all(isinstance(d, Document) for d in ret.invoke("q4"))


def test_store_bf16_precision_always_scans(require_gpu):
    store, rows, codes, queries, s_all = _store_case("bf16")
    before = store.group_scans
    for j in range(6):
        want = _want(rows, queries, codes, None, 5, s_all, j)
        assert _got(store.similarity_search_grouped_by_vector_with_score(queries[j], 5)) == want
    assert store.group_scans == before + 6
    got = store.similarity_search_grouped_batch(["q%d" % j for j in range(18)], k=2, filter={"tag": 2})
    assert store.group_scans == before + 6 + 18
    mask = np.arange(STORE_N) % 3 == 2
    for j in range(18):
        assert [d.id for d in got[j]] == [i for i, _ in _want(rows, queries, codes, mask, 2, s_all, j)]


def test_store_error_cases(require_gpu):
    store, rows, codes, queries, s_all = _store_case()
    n_groups = len(set(codes[codes >= 0].tolist()))
    assert n_groups <= _lib.MQ_MAX_K
    # no more than 64 groups exist: k past MQ_MAX_K returns them all
    assert len(store.similarity_search_grouped("q1", k=1000)) == n_groups
    single = _store_case(layout="singletons")[0]
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        single.similarity_search_grouped("q1", k=65)
    assert len(single.similarity_search_grouped("q1", k=64)) == 64
    with pytest.raises(ValueError, match="where_document"):
        store.similarity_search_grouped("q1", where_document={"$has": "x"})
    odd = HipChroma(dim=96, auto_persist=False)
    odd.add_embeddings(np.random.default_rng(0).standard_normal((5, 96)).astype(np.float32), list("abcde"),
                       [{"doc_id": "p"}] * 5, list("vwxyz"))
    with pytest.raises(ValueError, match="dim is 96"):
        odd.similarity_search_grouped_by_vector_with_score(np.ones(96, np.float32), 2)
    assert HipChroma(embedding_function=_Emb({}), dim=64, auto_persist=False).similarity_search_grouped("q") == []


def test_parent_retriever_returns_k_parents_where_the_collapse_of_a_top_k_does_not(require_gpu):
    """The reason for the feature.  Six children of one parent equal the query, so the plain
    similarity_search(k=5) collapsed LangChain's way names a single parent; the retriever with
    k = 5 returns the reference's five parents, in order."""
    dim, n = 64, 300
    q = gc.exact_queries(dim, 1)
    vectors = np.concatenate([np.repeat(q, 6, axis=0), gc.exact_corpus(dim, n)])
    tokens = ["c%07d" % r for r in range(len(vectors))]           # one 8-character chunk per row
    table = dict(zip(tokens, vectors))
    table["the query"] = q[0]
    bounds = [0, 6] + list(range(9, len(vectors), 3)) + [len(vectors)]  # parent 0: the six copies; then threes
    parents = [Document(page_content="".join(tokens[a:b]), metadata={"source": "s%d" % i})
               for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]
    codes = np.concatenate([np.full(b - a, i, np.int32) for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])
    store = HipChroma(embedding_function=_Emb(table), dim=dim, auto_persist=False)
    ret = HipParentDocumentRetriever(store, child_splitter=WindowSplitter(chunk_size=8), search_kwargs={"k": 5})
    ids = ret.add_documents(parents, ids=["parent%d" % i for i in range(len(parents))])
    assert len(store) == len(vectors) and np.array_equal(store._index.get(), vectors)
    # LangChain's way: the top-5 children, their distinct parents in order
    children = store.similarity_search("the query", k=5)
    collapsed = list(dict.fromkeys(d.metadata["doc_id"] for d in children))
    assert len(collapsed) < 5 and collapsed == ["parent0"]
    # the retriever: exactly the reference's five parents
    ref_s, ref_i = gc.grouped_reference(vectors, q, codes, None, 5)
    want = [parents[codes[r]] for r in ref_i[0]]
    assert len(want) == 5 and want[0] is parents[0]
    got = ret.invoke("the query")
    assert [d.page_content for d in got] == [d.page_content for d in want]
    assert [d.metadata for d in got] == [d.metadata for d in want] and ids[0] == "parent0"
