"""The batched BM25 calls on the host: every argument check of mq_lex_df_batch / mq_lex_topk_batch
comes before any HIP call (no GPU needed) and names the offending value, the batch scratch size
is monotone and bounded, and the fp32 definition alone stays inside the tie cap of
lexical_cases.py on the corpora that test_gpu_lexical_batch.py adds to the suite."""
import ctypes

import numpy as np
import pytest

import lexical_cases as lc
from mediquery_hip import _lib
from mediquery_hip.native import lex_batch_scratch_bytes


def _bufs():
    a, b, c = ((ctypes.c_uint8 * 4096)() for _ in range(3))
    al = lambda x: ctypes.c_void_p((ctypes.addressof(x) + 15) & ~15)  # noqa: E731
    return (a, b, c), al(a), al(b), al(c)


def _df(tokens, n_tokens, offsets, n, ngram, keys, n_keys, df, scratch):
    return _lib.call("mq_lex_df_batch", tokens, n_tokens, offsets, n, ngram,
                     _lib.ptr(keys) if keys is not None else None, n_keys, _lib.ptr(df) if df is not None else None,
                     scratch, None)


def _topk(tokens, n_tokens, offsets, n, ngram, term_start, keys, w, k, out_s, out_i, io, scratch, nq=None):
    ts = None if term_start is None else np.asarray(term_start, np.int64)
    nq = (len(ts) - 1) if nq is None else nq
    return _lib.call("mq_lex_topk_batch", tokens, n_tokens, offsets, n, ngram, nq,
                     _lib.ptr(ts) if ts is not None else None, _lib.ptr(keys) if keys is not None else None,
                     _lib.ptr(w) if w is not None else None, ctypes.c_float(0.3), ctypes.c_float(0.01), None, k,
                     out_s, out_i, io, scratch, None)


def test_constants_and_batch_scratch_size():
    assert _lib.MQ_LEX_BATCH_GROUP == 16 and _lib.MQ_LEX_BATCH_UNION == 512
    f = lex_batch_scratch_bytes
    base = f(1000, 4, 40, 8)
    assert base > 0
    # monotone in every argument
    for more in (f(10 ** 6, 4, 40, 8), f(1000, 400, 40, 8), f(1000, 4, 40000, 8), f(1000, 4, 40, 64)):
        assert more >= base
    sizes = [f(10 ** 6, nq, 12 * nq, 64) for nq in (0, 1, 2, 15, 16, 17, 70, 256, 4096, 10 ** 6)]
    assert sizes == sorted(sizes)
    sizes = [f(n, 256, 3000, 64) for n in (0, 1, 15, 16, 17, 1000, 10 ** 5, 10 ** 7, 10 ** 9)]
    assert sizes == sorted(sizes)
    sizes = [f(10 ** 6, 0, t, 1) for t in (1, 128, 512, 513, 1536, 10 ** 5, 10 ** 8)]
    assert sizes == sorted(sizes)
    # bounded in nq and in the terms: the workgroups' lists are reused from group to group
    top = f(1 << 40, 1 << 40, 1 << 40, _lib.MQ_MAX_K)
    assert f(10 ** 6, 10 ** 6, 10 ** 8, 64) == f(10 ** 6, 10 ** 9, 10 ** 11, 64) <= top < 32 << 20
    # k outside [1, MQ_MAX_K] and negative sizes are clamped, as mq_lex_scratch_bytes clamps them
    assert f(1000, 4, 40, 0) == f(1000, 4, 40, 1) and f(1000, 4, 40, 1000) == f(1000, 4, 40, 64)
    assert f(-5, -1, -1, 8) == f(0, 0, 0, 8)


def test_lex_df_batch_bad_arguments_raise_with_message():
    keep, p, q, r = _bufs()
    keys, df = np.array([5, 6], np.uint32), np.zeros(2, np.int64)
    with pytest.raises(_lib.MQError, match=r"negative size \(n -1"):
        _df(p, 16, q, -1, 1, keys, 2, df, r)
    with pytest.raises(_lib.MQError, match="negative size"):
        _df(p, -16, q, 1, 1, keys, 2, df, r)
    for ngram in (0, 3, -1):
        with pytest.raises(_lib.MQError, match=r"ngram must be 1 or 2 \(got %d\)" % ngram):
            _df(p, 16, q, 1, ngram, keys, 2, df, r)
    for n_keys in (0, -1):
        with pytest.raises(_lib.MQError, match=r"n_keys must be at least 1 \(got %d\)" % n_keys):
            _df(p, 16, q, 1, 1, keys, n_keys, df, r)
    with pytest.raises(_lib.MQError, match="NULL keys"):
        _df(p, 16, q, 1, 1, None, 2, df, r)
    with pytest.raises(_lib.MQError, match="NULL df"):
        _df(p, 16, q, 1, 1, keys, 2, None, r)
    many = np.arange(1000, 3000, dtype=np.uint32)
    many[1999] = many[3]
    with pytest.raises(_lib.MQError, match=r"keys must be distinct \(key 1003 is repeated\)"):
        _df(p, 16, q, 1, 1, many, many.size, np.zeros(many.size, np.int64), r)
    for args in ((None, 16, q, 1, 1, keys, 2, df, r), (p, 16, None, 1, 1, keys, 2, df, r),
                 (p, 16, q, 1, 1, keys, 2, df, None)):
        with pytest.raises(_lib.MQError, match="NULL buffer") as e:
            _df(*args)
        assert e.value.code == -1  # MQ_EINVAL
    with pytest.raises(_lib.MQError, match="tokens must be 16-byte aligned"):
        _df(ctypes.c_void_p(p.value + 2), 16, q, 1, 1, keys, 2, df, r)
    with pytest.raises(_lib.MQError, match="scratch must be 16-byte aligned"):
        _df(p, 16, q, 1, 1, keys, 2, df, ctypes.c_void_p(r.value + 8))
    # n == 0: every df is 0, for more keys than one pass takes too; the scalars are still checked
    many = np.arange(7, 7 + 1300, dtype=np.uint32)
    big = np.full(many.size, 7, np.int64)
    assert _df(None, 0, None, 0, 2, many, many.size, big, None) == _lib.MQ_OK and not big.any()
    with pytest.raises(_lib.MQError, match="ngram must be 1 or 2"):
        _df(None, 0, None, 0, 0, keys, 2, df, None)
    # more than 128 distinct keys and host pointers: past every argument check, refused as not device memory
    with pytest.raises(_lib.MQError, match="device memory"):
        _df(p, 16, q, 1, 1, many, many.size, big, r)


def test_lex_topk_batch_bad_arguments_raise_with_message():
    keep, p, q, r = _bufs()
    keys, w = np.array([5, 6, 5, 7], np.uint32), np.ones(4, np.float32)
    os_, oi = np.zeros(2 * 64, np.float32), np.zeros(2 * 64, np.int64)
    ps, pi = _lib.ptr(os_), _lib.ptr(oi)
    ts = [0, 2, 4]  # the two queries share key 5: accepted
    with pytest.raises(_lib.MQError, match="negative size"):
        _topk(p, 16, q, -1, 1, ts, keys, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match=r"ngram must be 1 or 2 \(got 3\)"):
        _topk(p, 16, q, 1, 3, ts, keys, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match=r"nq must not be negative \(got -2\)"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, pi, 0, r, nq=-2)
    for k in (0, -1, 65):
        with pytest.raises(_lib.MQError, match=r"k must be in \[1, 64\] \(got %d\)" % k):
            _topk(p, 16, q, 1, 1, ts, keys, w, k, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="io_on_device must be 0 or 1"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, pi, 2, r)
    with pytest.raises(_lib.MQError, match="NULL term_start"):
        _topk(p, 16, q, 1, 1, None, keys, w, 5, ps, pi, 0, r, nq=2)
    with pytest.raises(_lib.MQError, match=r"term_start must start at 0 \(got 1\)"):
        _topk(p, 16, q, 1, 1, [1, 2, 4], keys, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match=r"term_start must not decrease \(term_start\[2\] = 2 after 3\)"):
        _topk(p, 16, q, 1, 1, [0, 3, 2], keys, w, 5, ps, pi, 0, r)
    k129 = np.arange(100, 100 + 130, dtype=np.uint32)
    with pytest.raises(_lib.MQError, match=r"at most 128 terms \(query 1 has 129\)"):
        _topk(p, 16, q, 1, 1, [0, 1, 130], k129, np.ones(130, np.float32), 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match=r"distinct within a query \(key 5 is repeated in query 0\)"):
        _topk(p, 16, q, 1, 1, [0, 3, 4], keys, w, 5, ps, pi, 0, r)  # query 0 = 5, 6, 5
    with pytest.raises(_lib.MQError, match="NULL keys"):
        _topk(p, 16, q, 1, 1, ts, None, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL w"):
        _topk(p, 16, q, 1, 1, ts, keys, None, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL output"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, None, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL output"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, None, 0, r)
    with pytest.raises(_lib.MQError, match="scratch must not be an output"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, r, pi, 1, r)
    with pytest.raises(_lib.MQError, match="scratch must not be an output"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, r, 1, r)
    for args in ((None, 16, q, 1), (p, 16, None, 1)):
        with pytest.raises(_lib.MQError, match="NULL buffer"):
            _topk(*args, 1, ts, keys, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="NULL buffer"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, pi, 0, None)
    with pytest.raises(_lib.MQError, match="tokens must be 16-byte aligned"):
        _topk(ctypes.c_void_p(p.value + 2), 16, q, 1, 1, ts, keys, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="scratch must be 16-byte aligned"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, pi, 0, ctypes.c_void_p(r.value + 4))
    # nq == 0 is a no-op whatever the other pointers are
    assert _topk(None, 0, None, 0, 1, None, None, None, 5, None, None, 0, None, nq=0) == _lib.MQ_OK
    # n == 0 with host outputs: padding only, no HIP call; a query of 0 terms is accepted
    os_[:] = 3
    assert _topk(None, 0, None, 0, 1, [0, 0, 4], np.array([6, 5, 7, 8], np.uint32), w, 5, ps, pi, 0, None) == _lib.MQ_OK
    assert np.isneginf(os_[:10]).all() and oi[:10].tolist() == [-1] * 10 and os_[10] == 3
    # the same key in two different queries passes every argument check: refused only as not device memory
    with pytest.raises(_lib.MQError, match="device memory"):
        _topk(p, 16, q, 1, 1, ts, keys, w, 5, ps, pi, 0, r)
    with pytest.raises(_lib.MQError, match="device memory"):
        _topk(p, 16, q, 1, 1, [0, 0, 0], None, None, 5, ps, pi, 0, r)  # no terms at all: keys / w may be NULL


def test_repeated_key_is_found_in_any_query_and_group():
    """A repeat is reported with its key and query wherever the query lands: in the first group,
    behind a group cut by the query count, and behind one cut by the union size."""
    keep, p, q, r = _bufs()
    os_, oi = np.zeros(64 * 64, np.float32), np.zeros(64 * 64, np.int64)
    ps, pi = _lib.ptr(os_), _lib.ptr(oi)
    for at in (0, 15, 16, 17, 39):
        keys = np.arange(1000, 1000 + 80, dtype=np.uint32)  # 40 queries of 2 distinct keys each
        keys[2 * at + 1] = keys[2 * at]
        with pytest.raises(_lib.MQError, match=r"key %d is repeated in query %d\)" % (keys[2 * at], at)):
            _topk(p, 16, q, 1, 1, list(range(0, 81, 2)), keys, np.ones(80, np.float32), 5, ps, pi, 0, r)
    keys = np.arange(2000, 2000 + 6 * 128, dtype=np.uint32)  # 6 queries of 128 disjoint keys: unions of 512, 256
    keys[5 * 128 + 127] = keys[5 * 128 + 3]
    with pytest.raises(_lib.MQError, match=r"key %d is repeated in query 5\)" % keys[5 * 128 + 3]):
        _topk(p, 16, q, 1, 1, list(range(0, 6 * 128 + 1, 128)), keys, np.ones(keys.size, np.float32), 5, ps, pi, 0, r)


# the corpora test_gpu_lexical_batch.py uses that test_gpu_lexical.py does not: lc.zipf_rows(n, vocab, 11)
# at the batched kernel's block sizes (16, 32 and 64 rows) - 1 / + 0 / + 1 / x 2 + 1 that the single-query
# file's n = 1, 63, 64, 65, 129, 1000, 4097 do not cover
NEW_N = (15, 16, 17, 31, 32, 33)


@pytest.mark.parametrize("ngram", [1, 2])
def test_fp32_definition_stays_inside_the_tie_cap_on_the_new_corpora(ngram):
    tally = lc.Tally()
    for n in NEW_N:
        for vocab in (12, 60, 2000):
            rows = lc.zipf_rows(n, vocab, 11)
            corpus = lc.pack(rows)
            rng = np.random.default_rng([vocab, n])
            rand = rng.random(n) < 0.5
            for n_terms in (1, 2, 64, 128):
                qt = lc.query_tokens(rows, n_terms, n_terms + n, ngram, repeat=2 if n_terms > 1 else 0,
                                     absent=1 if n_terms > 2 else 0)
                setup = lc.bm25_setup(corpus, qt, ngram)
                if setup is None:
                    continue
                for mask, k in ((None, 5), (rand, 64), (None, 64), (rand, 1), (None, 1)):
                    ids, scores = lc.bm25_rank(setup, mask)
                    gi, gs = lc.bm25_fp32(setup, mask)
                    gi = np.concatenate([gi[:k], np.full(max(0, k - len(gi)), -1)])
                    gs = np.concatenate([gs[:k], np.full(max(0, k - len(gs)), -np.inf, np.float32)])
                    fails = lc.check_topk(gi, gs, ids, scores, k, len(setup["keys"]), tally)
                    assert not fails, (n, vocab, n_terms, k, fails[:4])
    assert tally.checked > 0 and tally.ok(), (tally.ambiguous, tally.checked)


@pytest.mark.parametrize("ngram", [1, 2])
def test_fp32_definition_stays_inside_the_tie_cap_on_the_several_blocks_corpus(ngram):
    """The 98,381-row corpus of test_gpu_lexical_batch.py with its G + 1 queries, masks and k."""
    import test_gpu_lexical_batch as gb
    corpus = gb._big_corpus()
    queries, sparse = gb._big_queries(corpus, ngram)
    tally = lc.Tally()
    for q in queries:
        setup = lc.bm25_setup(corpus, q, ngram)
        assert setup is not None
        for mask, k in ((None, 64), (sparse, 64), (None, 1)):
            ids, scores = lc.bm25_rank(setup, mask)
            gi, gs = lc.bm25_fp32(setup, mask)
            gi = np.concatenate([gi[:k], np.full(max(0, k - len(gi)), -1)])
            gs = np.concatenate([gs[:k], np.full(max(0, k - len(gs)), -np.inf, np.float32)])
            fails = lc.check_topk(gi, gs, ids, scores, k, len(setup["keys"]), tally)
            assert not fails, (ngram, k, fails[:4])
    assert tally.checked > 0 and tally.ok(), (tally.ambiguous, tally.checked)
