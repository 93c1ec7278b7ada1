"""Lexical and hybrid retrieval on the host: the argument checks of mq_lex_df / mq_lex_topk,
which come before any HIP call (no GPU needed), reciprocal rank fusion against the reference,
the body-token and term-key helpers, and the validation errors of the HipChroma methods."""
import ctypes

import numpy as np
import pytest

import lexical_cases as lc
from mediquery_hip import _lib
from mediquery_hip.tokenizer import CharTokenizer
from mediquery_hip.vectorstore import HipChroma, _LexicalRetriever, body_tokens, rrf_fuse, term_keys


def _bufs():
    a, b, c = ((ctypes.c_uint8 * 4096)() for _ in range(3))
    al = lambda x: ctypes.c_void_p((ctypes.addressof(x) + 15) & ~15)  # noqa: E731
    return (a, b, c), al(a), al(b), al(c)


def _keys(*v):
    return np.array(v, np.uint32)


def _df(tokens, n_tokens, offsets, n, ngram, keys, n_terms, df, scratch):
    return _lib.call("mq_lex_df", tokens, n_tokens, offsets, n, ngram, _lib.ptr(keys) if keys is not None else None,
                     n_terms, _lib.ptr(df) if df is not None else None, scratch, None)


def _topk(tokens, n_tokens, offsets, n, ngram, keys, w, n_terms, k, out_s, out_i, io, scratch, bits=None):
    return _lib.call("mq_lex_topk", tokens, n_tokens, offsets, n, ngram, _lib.ptr(keys) if keys is not None else None,
                     _lib.ptr(w) if w is not None else None, n_terms, ctypes.c_float(0.3), ctypes.c_float(0.01), bits,
                     k, out_s, out_i, io, scratch, None)


def test_constants_and_scratch_size():
    assert _lib.MQ_LEX_MAX_TERMS == 128
    small, big = _lib.lib().mq_lex_scratch_bytes(1, 1), _lib.lib().mq_lex_scratch_bytes(1 << 40, _lib.MQ_MAX_K)
    assert 128 * 8 < small < big < 4 << 20  # bounded: a persistent grid, not a list per 64 rows
    assert _lib.lib().mq_lex_scratch_bytes(10 ** 6, 64) == _lib.lib().mq_lex_scratch_bytes(10 ** 9, 64)


def test_lex_df_bad_arguments_raise_with_message():
    keep, p, q, r = _bufs()
    keys, df = _keys(5, 6), np.zeros(2, np.int64)
    with pytest.raises(_lib.MQError, match="negative size"):
        _df(p, 16, q, -1, 1, keys, 2, df, r)
    with pytest.raises(_lib.MQError, match="negative size"):
        _df(p, -16, q, 1, 1, keys, 2, df, r)
    for ngram in (0, 3, -1):
        with pytest.raises(_lib.MQError, match="ngram must be 1 or 2"):
            _df(p, 16, q, 1, ngram, keys, 2, df, r)
    for n_terms in (0, -1, 129):
        with pytest.raises(_lib.MQError, match="n_terms must be in"):
            _df(p, 16, q, 1, 1, keys, n_terms, df, r)
    with pytest.raises(_lib.MQError, match="NULL keys"):
        _df(p, 16, q, 1, 1, None, 2, df, r)
    with pytest.raises(_lib.MQError, match="keys must be distinct"):
        _df(p, 16, q, 1, 1, _keys(5, 9, 5), 3, np.zeros(3, np.int64), r)
    with pytest.raises(_lib.MQError, match="NULL df"):
        _df(p, 16, q, 1, 1, keys, 2, None, r)
    for args in ((None, 16, q, 1, 1, keys, 2, df, r), (p, 16, None, 1, 1, keys, 2, df, r),
                 (p, 16, q, 1, 1, keys, 2, df, None)):
        with pytest.raises(_lib.MQError, match="NULL buffer") as e:
            _df(*args)
        assert e.value.code == -1  # MQ_EINVAL
    with pytest.raises(_lib.MQError, match="16-byte aligned"):
        _df(ctypes.c_void_p(p.value + 2), 16, q, 1, 1, keys, 2, df, r)
    # n == 0: no row holds anything, whatever the pointers are; the scalars are still checked
    df[:] = 7
    assert _df(None, 0, None, 0, 2, keys, 2, df, None) == _lib.MQ_OK and df.tolist() == [0, 0]
    with pytest.raises(_lib.MQError, match="ngram must be 1 or 2"):
        _df(None, 0, None, 0, 0, keys, 2, df, None)
    # host pointers pass the argument checks and are then refused as not device memory
    with pytest.raises(_lib.MQError, match="device memory"):
        _df(p, 16, q, 1, 1, keys, 2, df, r)


def test_lex_topk_bad_arguments_raise_with_message():
    keep, p, q, r = _bufs()
    keys, w = _keys(5, 6), np.ones(2, np.float32)
    os_, oi = np.zeros(64, np.float32), np.zeros(64, np.int64)
    ps, pi = _lib.ptr(os_), _lib.ptr(oi)
    with pytest.raises(_lib.MQError, match="negative size"):
        _topk(p, 16, q, -1, 1, keys, w, 2, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="ngram must be 1 or 2"):
        _topk(p, 16, q, 1, 3, keys, w, 2, 5, ps, pi, 0, r)
    for n_terms in (0, 129):
        with pytest.raises(_lib.MQError, match="n_terms must be in"):
            _topk(p, 16, q, 1, 1, keys, w, n_terms, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="keys must be distinct"):
        _topk(p, 16, q, 1, 1, _keys(9, 9), w, 2, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL w"):
        _topk(p, 16, q, 1, 1, keys, None, 2, 5, ps, pi, 0, r)
    for k in (0, -1, 65):
        with pytest.raises(_lib.MQError, match="k must be in"):
            _topk(p, 16, q, 1, 1, keys, w, 2, k, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL output"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, None, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL output"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, ps, None, 0, r)
    with pytest.raises(_lib.MQError, match="io_on_device"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, ps, pi, 2, r)
    with pytest.raises(_lib.MQError, match="scratch must not be an output"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, r, pi, 1, r)
    with pytest.raises(_lib.MQError, match="scratch must not be an output"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, ps, r, 1, r)
    for args in ((None, 16, q, 1), (p, 16, None, 1)):
        with pytest.raises(_lib.MQError, match="NULL buffer"):
            _topk(*args, 1, keys, w, 2, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL buffer"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, ps, pi, 0, None)
    with pytest.raises(_lib.MQError, match="16-byte aligned"):
        _topk(ctypes.c_void_p(p.value + 2), 16, q, 1, 1, keys, w, 2, 5, ps, pi, 0, r)
    # n == 0 with host outputs: padding only, no HIP call
    assert _topk(None, 0, None, 0, 1, keys, w, 2, 5, ps, pi, 0, None) == _lib.MQ_OK
    assert np.isneginf(os_[:5]).all() and oi[:5].tolist() == [-1] * 5
    with pytest.raises(_lib.MQError, match="device memory"):
        _topk(p, 16, q, 1, 1, keys, w, 2, 5, ps, pi, 0, r)


def test_body_tokens_and_term_keys():
    tok = CharTokenizer(vocab_size=21128, max_length=8)
    texts = ["二甲双胍 500mg", "", "  ", "糖", "一二三四五六七八九十"]
    flat, lens = body_tokens(tok, texts)
    want = [tok.encode(t)[1:-1] for t in texts]
    assert lens.tolist() == [len(x) for x in want] == [8 - 2, 0, 0, 1, 6]  # truncated as the tokenizer truncates
    assert flat.dtype == np.uint16 and flat.tolist() == [i for x in want for i in x]
    assert body_tokens(tok, [])[0].size == 0
    assert term_keys([7, 8, 9], 1).tolist() == [7, 8, 9]
    assert term_keys([7, 8, 9], 2).tolist() == [(7 << 16) | 8, (8 << 16) | 9]
    assert term_keys([7], 2).size == 0 and term_keys([], 2).size == 0 and term_keys([], 1).size == 0
    assert np.array_equal(term_keys(flat[:6], 2), lc.query_terms(flat[:6], 2))
    with pytest.raises(ValueError, match="uint16"):
        body_tokens(CharTokenizer(vocab_size=200000, max_length=64), ["糖尿病的一线药物" * 4])


def test_rrf_fuse_equals_reference_and_validates():
    rng = np.random.default_rng(5)
    for trial in range(200):
        d = rng.permutation(200)[:int(rng.integers(0, 65))].tolist()
        x = rng.permutation(200)[:int(rng.integers(0, 65))].tolist()
        wts = [(0.5, 0.5), (1.0, 0.0), (0.0, 2.0), (0.3, 0.7)][trial % 4]
        c = [60, 0, 1, 7.5][trial % 4]
        k = int(rng.integers(1, 30))
        assert rrf_fuse(d, x, wts, c, k) == lc.rrf_reference(d, x, wts, c, k)
        if c > 0 and (d or x):
            assert rrf_fuse(d, x, wts, c, k) != lc.rrf_reference(d, x, wts, c, k, mutant="rrf_rank0")
    for bad in ((0.5,), (0.5, 0.5, 0.5), (0.0, 0.0), (-0.1, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), "ab", None,
                ("a", 1.0)):
        with pytest.raises(ValueError, match="weights"):
            rrf_fuse([1], [2], bad)
    for bad in (-1, float("nan"), float("inf"), "60", None, True):
        with pytest.raises(ValueError, match="c must be"):
            rrf_fuse([1], [2], (0.5, 0.5), bad)


class _Emb:
    """An embedding function with a tokenizer and no device."""
    tokenizer = CharTokenizer(max_length=32)

    def embed_query(self, text):
        return [0.0] * 64


def test_store_validates_before_any_device_work():
    """On an empty store with no GPU nothing but the validation can raise."""
    with pytest.raises(ValueError, match="lexical_ngram"):
        HipChroma(dim=64, lexical_ngram=3)
    with pytest.raises(ValueError, match="bm25"):
        HipChroma(dim=64, bm25_b=1.5)
    with pytest.raises(ValueError, match="bm25"):
        HipChroma(dim=64, bm25_k1=-1.0)
    bare = HipChroma(dim=64, auto_persist=False)
    for call in (lambda: bare.lexical_search("q"), lambda: bare.lexical_search_with_score("q"),
                 lambda: bare.lexical_search_batch(["q"]), lambda: bare.hybrid_search("q"),
                 lambda: bare.hybrid_search_with_score("q"), lambda: bare.hybrid_search_batch(["q"]),
                 lambda: bare.as_retriever(search_type="lexical").invoke("q"),
                 lambda: bare.as_retriever(search_type="hybrid").invoke("q")):
        with pytest.raises(ValueError, match="tokenizer"):
            call()
    big = HipChroma(dim=64, auto_persist=False, lexical_tokenizer=CharTokenizer(vocab_size=70000))
    with pytest.raises(ValueError, match="65536"):
        big.lexical_search("q")
    class Falsy(CharTokenizer):  # a tokenizer object that is falsy is still the one given
        def __len__(self):
            return 0
    falsy = HipChroma(dim=64, auto_persist=False, embedding_function=_Emb(), lexical_tokenizer=Falsy(vocab_size=70000))
    with pytest.raises(ValueError, match="65536"):
        falsy.lexical_search("q")
    for store in (HipChroma(dim=64, auto_persist=False, lexical_tokenizer=CharTokenizer()),
                  HipChroma(dim=64, auto_persist=False, embedding_function=_Emb(), lexical_ngram=2)):
        bad = {"$regex": "a"}
        for call in (lambda: store.lexical_search("q", where_document=bad),
                     lambda: store.lexical_search_with_score("q", where_document=bad),
                     lambda: store.lexical_search_batch(["q"], where_document=bad),
                     lambda: store.hybrid_search("q", where_document=bad),
                     lambda: store.hybrid_search_with_score("q", where_document=bad),
                     lambda: store.hybrid_search_batch(["q"], where_document=bad)):
            with pytest.raises(ValueError, match="where_document"):
                call()
        for wts in ((0.0, 0.0), (1.0,), (-1.0, 1.0), (float("nan"), 0.5)):
            with pytest.raises(ValueError, match="weights"):
                store.hybrid_search("q", weights=wts)
        with pytest.raises(ValueError, match="c must be"):
            store.hybrid_search("q", c=-2)
        assert store.lexical_search("q") == [] and store.lexical_search_with_score("q", k=3) == []
        assert store.lexical_search_batch(["a", "b"]) == [[], []]
        assert store._lex_mirror is None
    emb = HipChroma(dim=64, auto_persist=False, embedding_function=_Emb())
    assert emb.hybrid_search("q") == [] and emb.hybrid_search_batch(["a", "b"]) == [[], []]
    no_emb = HipChroma(dim=64, auto_persist=False, lexical_tokenizer=CharTokenizer())
    with pytest.raises(ValueError, match="embedding_function"):
        no_emb.hybrid_search("q")


def test_retriever_types():
    store = HipChroma(dim=64, auto_persist=False, embedding_function=_Emb())
    calls = []
    store.lexical_search = lambda q, **kw: calls.append(("lexical", q, kw)) or ["L"]
    store.hybrid_search = lambda q, **kw: calls.append(("hybrid", q, kw)) or ["H"]
    r = store.as_retriever(search_type="lexical", search_kwargs={"k": 7, "filter": {"a": 1}})
    assert isinstance(r, _LexicalRetriever) and r.invoke("q") == ["L"] and r.get_relevant_documents("q2") == ["L"]
    h = store.as_retriever(search_type="hybrid", search_kwargs={"k": 3, "fetch_k": 30, "weights": (0.3, 0.7), "c": 10})
    assert h.invoke("q") == ["H"]
    assert calls == [("lexical", "q", {"k": 7, "filter": {"a": 1}}), ("lexical", "q2", {"k": 7, "filter": {"a": 1}}),
                     ("hybrid", "q", {"k": 3, "fetch_k": 30, "weights": (0.3, 0.7), "c": 10})]
    assert not isinstance(store.as_retriever(search_kwargs={"k": 3}), _LexicalRetriever)
    assert not isinstance(store.as_retriever(search_type="mmr"), _LexicalRetriever)
