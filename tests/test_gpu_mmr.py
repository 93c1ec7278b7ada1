"""The device MMR selection (K11, csrc/mmr.hip) against the float64 restatement of
LangChain's maximal_marginal_relevance (tests/mmr_cases.py): exact equality on the exact
class, the per-step path check at 1e-5 on the random class; then mq_index_search_mmr, the
masked form, HipChroma's three methods and the argument checks.

Largest deficit the device showed on the random class (check_path's best-minus-picked
float64 score; MI355X, 256 queries per configuration, profiles/mmr/accuracy.txt): 0 - the
device took the float64 argmax at each of 96,768 steps."""
import numpy as np
import pytest

import mmr_cases as mc
from mediquery_hip import Document, HipBertEmbeddings, HipChroma, _lib, compat
from mediquery_hip.config import BertConfig
from mediquery_hip.native import FlatIndex

pytestmark = pytest.mark.gpu

N_FAM, FAM = 16, 24          # the small exact corpora of the selection tests
FETCH_KS = (1, 2, 20, 31, 32, 33, 63, 64)
KINDS = ("sorted", "shuffled", "tail", "holes", "allpad")
_cache = {}


def _index(rows, precision=None):
    ix = FlatIndex(dim=rows.shape[1], device=0)
    if precision is not None:
        ix.set_precision(precision)
    ix.add(rows)
    return ix


def _exact_index(dim, n_fam=N_FAM, fam=FAM):
    """(index, rows) of an exact-class corpus; the index holds the rows bit for bit (unit
    norms: the add step's 1/sqrt(1) is the identity) - the precondition of every equality."""
    key = ("exact", dim, n_fam, fam)
    if key not in _cache:
        rows = mc.exact_corpus(dim, n_fam, fam)
        ix = _index(rows)
        assert np.array_equal(ix.get(), rows)
        _cache[key] = (ix, rows)
    return _cache[key]


def _random_index(dim):
    key = ("random", dim)
    if key not in _cache:
        ix = _index(mc.random_corpus(dim))
        _cache[key] = (ix, ix.get())  # the stored (device-normalised) rows are the reference's
    return _cache[key]


def _lists(rows, fetch_k, kind, nq, n):
    """Candidate lists [nq, fetch_k] of the given kind -> (cand_s f32, cand_ids i64)."""
    cs = np.empty((nq, fetch_k), np.float32)
    ci = np.empty((nq, fetch_k), np.int64)
    rng = np.random.default_rng([fetch_k, KINDS.index(kind)])
    for q in range(nq):
        ids, s = mc.exact_candidates(rows, N_FAM, FAM, q % N_FAM, fetch_k, seed=q // N_FAM)
        s = s.astype(np.float32)
        if kind == "shuffled":
            p = rng.permutation(fetch_k)
            ids, s = ids[p], s[p]
        elif kind == "tail":
            cut = fetch_k - max(1, fetch_k // 3)
            ids[cut:], s[cut:] = -1, -np.inf
        elif kind == "holes":  # padding ids on both sides of [0, n), with scores that would win
            ids[1::3], s[1::3] = -1, 2.0
            ids[2::6] = n + 7
        elif kind == "allpad":
            ids[:], s[:] = -1, -np.inf
        ci[q], cs[q] = ids, s
    return cs, ci


def _valid_grams(rows, ci):
    """Per list: (positions of the valid candidates, their float64 Gram matrix)."""
    valid = [np.flatnonzero((c >= 0) & (c < len(rows))) for c in ci]
    return [(v, mc.gram64(rows, c[v])) for v, c in zip(valid, ci)]


def _expected(cs, ci, grams, lam, k):
    """mmr_reference over each list's valid candidates -> (scores [nq, k], ids [nq, k])."""
    es = np.full((len(ci), k), -np.inf, np.float32)
    ei = np.full((len(ci), k), -1, np.int64)
    for q, (valid, G) in enumerate(grams):
        picks = mc.mmr_reference(cs[q][valid].astype(np.float64), G, lam, k)
        ei[q, :len(picks)] = ci[q][valid][picks]
        es[q, :len(picks)] = cs[q][valid][picks]
    return es, ei


@pytest.mark.parametrize("dim", sorted(mc.EXACT_DIMS))
def test_select_exact_class_equals_reference(require_gpu, dim):
    ix, rows = _exact_index(dim)
    for fetch_k in FETCH_KS:
        for kind in KINDS:
            cs, ci = _lists(rows, fetch_k, kind, 5, len(rows))
            grams = _valid_grams(rows, ci)
            for lam in mc.LAMBDAS:
                # the greedy sequence for k = fetch_k holds every shorter one as its prefix
                es, ei = _expected(cs, ci, grams, lam, fetch_k)
                for k in sorted({1, min(5, fetch_k), fetch_k}):
                    for nq in (1, 5):
                        gs, gi = ix.mmr_select(cs[:nq], ci[:nq], k, lam)
                        where = (dim, fetch_k, kind, lam, k, nq)
                        assert np.array_equal(gi, ei[:nq, :k]), where
                        assert np.array_equal(gs, es[:nq, :k]), where


def test_select_more_queries_than_cus(require_gpu):
    ix, rows = _exact_index(32)
    cs, ci = _lists(rows, 20, "sorted", 300, len(rows))
    es, ei = _expected(cs, ci, _valid_grams(rows, ci), 0.5, 5)
    gs, gi = ix.mmr_select(cs, ci, 5, 0.5)
    assert np.array_equal(gi, ei) and np.array_equal(gs, es)


@pytest.mark.parametrize("dim", (96, 768))
def test_select_random_class_follows_the_float64_path(require_gpu, dim):
    ix, stored = _random_index(dim)
    queries = mc.random_queries(stored, 6)
    worst = 0.0
    for fetch_k in (20, 64):
        cands = [mc.top_candidates(stored, q, fetch_k) for q in queries]
        ci = np.stack([c[0] for c in cands])
        s64 = np.stack([c[1] for c in cands])
        G64 = [mc.gram64(stored, ids) for ids in ci]
        for k in (5, 16):
            for lam in (0.25, 0.5, 0.9):
                gs, gi = ix.mmr_select(s64.astype(np.float32), ci, k, lam)
                lam32 = float(np.float32(lam))  # the lambda the kernel receives
                for q in range(len(queries)):
                    picks = mc.positions(gi[q], ci[q])
                    worst = max([worst] + mc.path_deficits([p for p in picks if p >= 0], s64[q], G64[q], lam32))
                    fails = mc.check_path(picks, s64[q], G64[q], lam32, mc.TOL, k)
                    assert fails == [], (dim, fetch_k, k, lam, q, fails)
                    assert np.array_equal(gs[q], s64[q].astype(np.float32)[picks])
                # a query alone gives what it gives inside the batch
                g1 = ix.mmr_select(s64[3:4].astype(np.float32), ci[3:4], k, lam)[1]
                assert np.array_equal(g1[0], gi[3])
    print("dim %d: largest float64 deficit along the device's paths %.3g" % (dim, worst))


def test_select_on_device_buffers_equals_host_call(require_gpu):
    """mmr_select_device (device lists in, device results out, asynchronous on the stream)
    gives what the host-pointer call gives, for both kernel instances; on an empty index it
    fills the padding on the stream too."""
    import torch
    ix, rows = _exact_index(96)
    for fetch_k, k in ((20, 5), (64, 16)):
        cs, ci = _lists(rows, fetch_k, "holes", 5, len(rows))
        hs, hi = ix.mmr_select(cs, ci, k, 0.25)
        ds = torch.zeros((5, k), dtype=torch.float32, device="cuda:0")
        di = torch.zeros((5, k), dtype=torch.int64, device="cuda:0")
        ix.mmr_select_device(torch.from_numpy(cs).to("cuda:0"), torch.from_numpy(ci).to("cuda:0"), k, 0.25, ds, di)
        torch.cuda.synchronize()
        assert np.array_equal(di.cpu().numpy(), hi) and np.array_equal(ds.cpu().numpy(), hs)
    empty = FlatIndex(dim=96, device=0)
    ds = torch.zeros((2, 3), dtype=torch.float32, device="cuda:0")
    di = torch.zeros((2, 3), dtype=torch.int64, device="cuda:0")
    empty.mmr_select_device(torch.zeros((2, 4), device="cuda:0"), torch.zeros((2, 4), dtype=torch.int64, device="cuda:0"),
                            3, 0.5, ds, di)
    torch.cuda.synchronize()
    assert (di.cpu().numpy() == -1).all() and np.isneginf(ds.cpu().numpy()).all()


def test_threads_on_one_handle_serialise(require_gpu):
    """Two threads calling search_mmr on one index (ctypes drops the GIL; LangChain's async
    retriever runs in a thread pool) each get their own query's result: the calls hold the
    handle's workspace for their whole length.  Sizes alternate so that the workspace is
    regrown under way."""
    import threading
    ix, rows, n_fam = _family_index(20, "f32")
    queries = mc.exact_queries(rows, n_fam, 24)
    want = _reference_rows(rows, queries, 20, 0.5, 5)
    errors = []

    def worker(t):
        try:
            for it in range(40):
                q = (7 * it + 11 * t) % 20
                m = 1 + (it + t) % 4  # 1-4 queries per call
                got = ix.search_mmr(queries[q:q + m], 5, 20, 0.5)[1]
                if not np.array_equal(got, want[q:q + m]):
                    errors.append((t, it, q, m))
        except Exception as e:  # noqa: BLE001 - reported by the assertion below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert errors == []


# ---------------------------------------------------------------- search + select ----
SEARCH_DIM = 768
PRECISIONS = {"screen": _lib.MQ_DTYPE_F32_SCREEN, "f32": _lib.MQ_DTYPE_F32}


def _family_index(fetch_k, precision):
    """2,560 exact-class rows in families of exactly fetch_k members: a query on a family's
    base has that family as its top fetch_k, strictly above every other row, with the ties
    inside it ordered by row id."""
    n_fam = 2560 // fetch_k
    key = ("family", fetch_k, precision)
    if key not in _cache:
        rows = mc.exact_corpus(SEARCH_DIM, n_fam, fetch_k)
        ix = _index(rows, PRECISIONS[precision])
        assert np.array_equal(ix.get(), rows)
        _cache[key] = (ix, rows, n_fam)
    return _cache[key]


def _reference_rows(rows, queries, fetch_k, lam, k, allowed=None):
    """mmr_reference over the float64 top fetch_k of each query (score desc, id asc), as row
    ids [nq, k] padded with -1.  The list must end at a strict gap: which of several rows
    tied across the cut a search keeps is the search's business, not this test's."""
    out = np.full((len(queries), k), -1, np.int64)
    pool = np.arange(len(rows)) if allowed is None else np.flatnonzero(allowed)
    for q, vec in enumerate(queries):
        ids, s = mc.top_candidates(rows, vec, fetch_k, allowed)
        rest = np.setdiff1d(pool, ids)
        if len(rest):
            assert s[-1] > (rows[rest].astype(np.float64) @ vec.astype(np.float64)).max()
        picks = mc.mmr_reference(s, mc.gram64(rows, ids), lam, k)
        out[q, :len(picks)] = ids[picks]
    return out


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
@pytest.mark.parametrize("fetch_k", (20, 64))
def test_search_mmr_exact_class_equals_reference(require_gpu, precision, fetch_k):
    ix, rows, n_fam = _family_index(fetch_k, precision)
    queries = mc.exact_queries(rows, n_fam, 5)
    for lam in mc.LAMBDAS:
        gs, gi = ix.search_mmr(queries, 5, fetch_k, lam)
        assert np.array_equal(gi, _reference_rows(rows, queries, fetch_k, lam, 5)), (precision, fetch_k, lam)
        # the scores are the picked rows' cosines to the query (exact on this class)
        cos = np.einsum("qkd,qd->qk", rows[gi].astype(np.float64), queries.astype(np.float64))
        assert np.array_equal(gs, cos.astype(np.float32))
    # lambda = 1: the search's own order
    assert np.array_equal(ix.search_mmr(queries, 5, fetch_k, 1.0)[1], ix.search(queries, 5)[1])
    # a query alone and inside a batch of 67
    batch = mc.exact_queries(rows, n_fam, 67)
    gb = ix.search_mmr(batch, 5, fetch_k, 0.5)[1]
    for q in (0, 31, 66):
        assert np.array_equal(ix.search_mmr(batch[q:q + 1], 5, fetch_k, 0.5)[1][0], gb[q])


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_search_mmr_lambda_one_is_the_search_on_random_rows(require_gpu, precision):
    ix = _index(mc.random_corpus(768), PRECISIONS[precision])  # its own index: the cached one keeps its precision
    stored = ix.get()
    queries = mc.random_queries(stored, 6, seed=1)
    assert np.array_equal(ix.search_mmr(queries, 5, 20, 1.0)[1], ix.search(queries, 5)[1])
    # and lambda = 0.5 follows the float64 path over the float64 top 20
    gs, gi = ix.search_mmr(queries, 5, 20, 0.5)
    for q, vec in enumerate(queries):
        ids, s64 = mc.top_candidates(stored, vec, 20)
        assert mc.check_path(mc.positions(gi[q], ids), s64, mc.gram64(stored, ids), 0.5, mc.TOL, 5) == []


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_search_mmr_seven_rows(require_gpu, precision):
    rows = mc.exact_corpus(SEARCH_DIM, 7, 1)
    ix = _index(rows, PRECISIONS[precision])
    queries = rows[[2, 5]].copy()
    gs, gi = ix.search_mmr(queries, 10, 20, 0.5)
    want = _reference_rows(rows, queries, 20, 0.5, 10)
    assert np.array_equal(gi, want) and (gi[:, :7] >= 0).all() and (gi[:, 7:] == -1).all()
    assert np.isneginf(gs[:, 7:]).all() and np.isfinite(gs[:, :7]).all()
    # an empty index: padding only
    empty = FlatIndex(dim=SEARCH_DIM, device=0)
    gs, gi = empty.search_mmr(queries, 3, 20, 0.5)
    assert (gi == -1).all() and np.isneginf(gs).all()
    gs, gi = empty.mmr_select(np.zeros((2, 4), np.float32), np.arange(8).reshape(2, 4), 3, 0.5)
    assert (gi == -1).all() and np.isneginf(gs).all()


def _mask_bits(allowed):
    import torch
    words = np.packbits(np.pad(allowed, (0, -len(allowed) % 32)), bitorder="little").view(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")


@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_search_mmr_with_a_mask(require_gpu, precision):
    ix, rows, n_fam = _family_index(20, precision)
    # the exact copy and one near-copy of every family are filtered out: 18 members left
    member = np.arange(len(rows)) // n_fam
    allowed = ~np.isin(member, (1, 3))
    bits = _mask_bits(allowed)
    queries = mc.exact_queries(rows, n_fam, 5)
    for lam in (0.0, 0.5, 1.0):
        gs, gi = ix.search_mmr(queries, 5, 18, lam, bits=bits)
        assert allowed[gi].all()
        assert np.array_equal(gi, _reference_rows(rows, queries, 18, lam, 5, allowed)), (precision, lam)
    with pytest.raises(ValueError):
        ix.search_mmr(queries, 5, 18, 0.5, bits=bits[:3])


# --------------------------------------------------------------------- HipChroma ----
@pytest.fixture(scope="module")
def exact_store(require_gpu):
    rows = mc.exact_corpus(SEARCH_DIM, 128, 20)
    store = HipChroma(embedding_function=None, dim=SEARCH_DIM)
    n = len(rows)
    store.add_embeddings(rows, ["text %d" % r for r in range(n)], [{"member": int(r // 128)} for r in range(n)],
                         ["id%d" % r for r in range(n)])
    return store, rows


def test_store_mmr_by_vector(exact_store):
    store, rows = exact_store
    # family 3's base with the sign flips of its members 2, 3, 5, 6 and 7 applied: those five
    # are the most similar rows, together with member 4, the exact copy of member 2.  (A
    # query that IS a stored row would not do: at lambda 1/2 its copy ties with every
    # near-copy, s_i - G[i][base] being 0 for all of them, and the tie goes to the copy.)
    query = rows[3].copy()
    for v in (2, 3, 5, 6, 7):
        flipped = rows[v * 128 + 3] != rows[3]
        query[flipped] = -rows[3][flipped]
    want = _reference_rows(rows, query[None], 20, 0.5, 5)[0]
    docs = store.max_marginal_relevance_search_by_vector(query, k=5, fetch_k=20, lambda_mult=0.5)
    assert all(isinstance(d, Document) for d in docs)
    assert [d.page_content for d in docs] == ["text %d" % r for r in want]
    got = rows[[int(d.id[2:]) for d in docs]]
    assert len({g.tobytes() for g in got}) == 5  # no two exact copies: non-copies were left
    plain = store.similarity_search_by_vector(query, k=5)  # the plain search does return a copy
    assert {"id%d" % (2 * 128 + 3), "id%d" % (4 * 128 + 3)} <= {d.id for d in plain}
    assert len({rows[int(d.id[2:])].tobytes() for d in plain}) < 5
    # with a filter: no filtered row, the reference over the allowed rows
    allowed = np.arange(len(rows)) // 128 != 1
    docs = store.max_marginal_relevance_search_by_vector(query, k=5, fetch_k=19, lambda_mult=0.5,
                                                         filter={"member": {"$ne": 1}})
    assert [int(d.id[2:]) for d in docs] == list(_reference_rows(rows, query[None], 19, 0.5, 5, allowed)[0])
    # k > fetch_k: fetch_k documents; k <= 0: none; more than MQ_MAX_K candidates: an error
    assert len(store.max_marginal_relevance_search_by_vector(query, k=10, fetch_k=4)) == 4
    assert store.max_marginal_relevance_search_by_vector(query, k=0) == []
    with pytest.raises(ValueError, match="MQ_MAX_K"):
        store.max_marginal_relevance_search_by_vector(query, k=5, fetch_k=65)


def test_store_mmr_text_and_batch(require_gpu):
    emb = HipBertEmbeddings(model="shaw/dmeta-embedding-zh", synthetic=True, config=BertConfig(layers=2))
    assert HipChroma(embedding_function=emb).max_marginal_relevance_search("anything", k=3) == []
    assert HipChroma(embedding_function=emb).max_marginal_relevance_search_batch(["a", "b"]) == [[], []]
    texts = ["note %d on %s" % (i, ("fever", "cough", "rash", "pain")[i % 4]) for i in range(40)]
    store = HipChroma.from_texts(texts, emb, ids=["t%d" % i for i in range(40)])
    stored = store._index.get()
    queries = ["fever note", "a cough", "rash and pain"]

    def check(docs, vec, k, lam):
        ids, s64 = mc.top_candidates(stored, vec, 40)  # the whole store: no cut to tie across
        picks = mc.positions([int(d.id[1:]) for d in docs], ids)
        assert mc.check_path(picks, s64, mc.gram64(stored, ids), float(np.float32(lam)), mc.TOL, k) == []

    # fetch_k = 100 is clipped to the store's 40 rows (and so passes the MQ_MAX_K check)
    for q in queries:
        docs = store.max_marginal_relevance_search(q, k=6, fetch_k=100, lambda_mult=0.3)
        check(docs, np.asarray(emb.embed_query(q), np.float32), 6, 0.3)
    res = store.max_marginal_relevance_search_batch(queries, k=6, fetch_k=100, lambda_mult=0.3)
    assert len(res) == 3
    for vec, docs in zip(emb.embed_array(queries), res):
        check(docs, vec, 6, 0.3)
    assert len(store.max_marginal_relevance_search(queries[0], k=50, fetch_k=100)) == 40
    if not compat.HAVE_LANGCHAIN:
        got = store.as_retriever(search_type="mmr", search_kwargs={"k": 3, "fetch_k": 40}).invoke(queries[0])
        assert [d.id for d in got] == [d.id for d in store.max_marginal_relevance_search(queries[0], k=3, fetch_k=40)]


# --------------------------------------------------------------- argument checks ----
def test_bad_arguments_raise_with_a_message(require_gpu):
    ix, rows = _exact_index(32)
    cs, ci = _lists(rows, 20, "sorted", 2, len(rows))
    q = rows[:2].copy()
    for k, fetch_k, lam in ((21, 20, 0.5), (5, 65, 0.5), (5, 20, 1.5), (5, 20, float("nan")), (0, 20, 0.5),
                            (5, 20, -0.25)):
        with pytest.raises(_lib.MQError) as e:
            ix.search_mmr(q, k, fetch_k, lam)
        assert str(e.value).split(": ", 1)[1].strip(), (k, fetch_k, lam)
        if fetch_k <= 20:
            with pytest.raises(_lib.MQError) as e:
                ix.mmr_select(cs[:, :fetch_k], ci[:, :fetch_k], k, lam)
            assert "must be" in str(e.value)
    big = np.zeros((1, 65), np.float32)
    with pytest.raises(_lib.MQError, match="fetch_k"):
        ix.mmr_select(big, np.zeros((1, 65), np.int64), 5, 0.5)
