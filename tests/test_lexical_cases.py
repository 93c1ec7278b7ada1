"""CPU checks of the lexical retrieval test material (tests/lexical_cases.py): the float64
BM25 reference passes its own checker and so does a numpy fp32 restatement of the device's
arithmetic, the checker rejects every mutant on the same data, the query-term cap keeps the
128 highest-idf terms, and the product's host half (bm25_plan, rrf_fuse) computes what the
reference computes."""
import numpy as np
import pytest

import lexical_cases as lc
from mediquery_hip.vectorstore import bm25_plan, rrf_fuse


def _data(ngram, n=300, seed=0):
    rows = lc.zipf_rows(n, 40 if ngram == 1 else 12, seed, max_len=60)
    corpus = lc.pack(rows)
    mask = np.random.default_rng(seed + 1).random(n) < 0.6
    # a query over frequent terms; for ngram 2 it also holds the pair (last token of row 4,
    # first token of row 5), which the cross-row mutant matches
    q = lc.query_tokens(rows, 6 if ngram == 1 else 12, seed, ngram, repeat=1, absent=1)
    if ngram == 2:
        a = next(r for r in range(4, n - 1) if len(rows[r]) and len(rows[r + 1]))
        q += [3, int(rows[a][-1]), int(rows[a + 1][0])]
    return rows, corpus, mask, q


@pytest.mark.parametrize("ngram", [1, 2])
def test_reference_and_fp32_restatement_pass_the_checker(ngram):
    rows, corpus, mask, q = _data(ngram)
    tally = lc.Tally()
    for m in (None, mask):
        setup = lc.bm25_setup(corpus, q, ngram, mask=m)
        ids, s = lc.bm25_rank(setup, m)
        assert len(ids) > 64
        for k in (1, 5, 64):
            assert lc.check_topk(ids[:k], s[:k], ids, s, k, len(setup["keys"]), tally) == []
            gi, gs = lc.bm25_fp32(setup, m)
            assert lc.check_topk(gi[:k], gs[:k], ids, s, k, len(setup["keys"]), tally) == []
    assert tally.ok(), (tally.ambiguous, tally.checked)
    assert np.sum(np.diff(s) == 0) > 5  # the copied rows do tie exactly


def test_checker_rejects_wrong_shapes_padding_and_repeats():
    rows, corpus, mask, q = _data(1)
    ids, s = lc.bm25_reference(rows, q, 1)
    n_t = 6
    assert lc.check_topk(ids[:4], s[:4], ids, s, 5, n_t)
    few_i, few_s = ids[:3], s[:3]
    pad_i, pad_s = list(few_i) + [-1, -1], list(few_s) + [-np.inf, -np.inf]
    assert lc.check_topk(pad_i, pad_s, few_i, few_s, 5, n_t) == []
    assert lc.check_topk(list(few_i) + [0, -1], pad_s, few_i, few_s, 5, n_t)
    assert lc.check_topk([ids[0], ids[0], ids[2]], s[:3], ids, s, 3, n_t)
    off = s[:5].copy()
    off[2] *= 1.0 + 4 * lc.score_tol(n_t)
    assert lc.check_topk(ids[:5], off, ids, s, 5, n_t)


@pytest.mark.parametrize("mutant", [m for m in lc.MUTANTS if m != "rrf_rank0"])
def test_checker_rejects_every_mutant(mutant):
    ngram = 2 if mutant in ("dl_tokens", "cross_row") else 1
    rows, corpus, mask, q = _data(ngram)
    m = mask if mutant == "stats_masked" else None
    ids, s = lc.bm25_reference(corpus, q, ngram, mask=m)
    n_t = len(lc.bm25_setup(corpus, q, ngram)["keys"])
    bad_i, bad_s = lc.bm25_reference(corpus, q, ngram, mask=m, mutant=mutant)
    k = 64
    assert lc.check_topk(ids[:k], s[:k], ids, s, k, n_t) == []
    assert lc.check_topk(bad_i[:k], bad_s[:k], ids, s, k, n_t), mutant


def test_rrf_reference_and_its_mutant():
    dense, lex = [5, 9, 2, 7], [9, 11, 5, 3]
    ref = lc.rrf_reference(dense, lex, (0.5, 0.5), 60)
    assert [r for r, _ in ref] == [9, 5, 11, 2, 7, 3]  # 7 and 3 tie (rank 4 each): the dense list's first
    assert ref[0][1] == 0.5 / 62 + 0.5 / 61
    assert lc.rrf_reference(dense, lex, (0.5, 0.5), 60, mutant="rrf_rank0") != ref
    assert [r for r, _ in lc.rrf_reference(dense, lex, (1.0, 0.0), 60, k=3)] == [5, 9, 2]
    rng = np.random.default_rng(0)
    for trial in range(50):
        d = rng.permutation(40)[:int(rng.integers(0, 20))].tolist()
        x = rng.permutation(40)[:int(rng.integers(0, 20))].tolist()
        wts = (float(rng.random()), float(rng.random()) + 0.01)
        c = int(rng.integers(0, 80))
        assert rrf_fuse(d, x, wts, c) == lc.rrf_reference(d, x, wts, c)
        assert rrf_fuse(d, x, wts, c, k=5) == lc.rrf_reference(d, x, wts, c, k=5)


@pytest.mark.parametrize("ngram", [1, 2])
def test_query_term_cap_keeps_the_128_highest_idf(ngram):
    rows = lc.zipf_rows(400, 2000, 3, max_len=80)
    corpus = lc.pack(rows)
    q = lc.query_tokens(rows, 200, 1, ngram, repeat=3, absent=0)
    full = lc.bm25_setup(corpus, q, ngram, max_terms=10 ** 6)
    capped = lc.bm25_setup(corpus, q, ngram)
    assert len(full["keys"]) >= 200 and len(capped["keys"]) == lc.MAX_TERMS
    n = full["n"]
    idf = np.log(1.0 + (n - full["df"] + 0.5) / (full["df"] + 0.5))
    order = sorted(range(len(idf)), key=lambda j: (-idf[j], int(full["keys"][j])))[:lc.MAX_TERMS]
    assert sorted(int(full["keys"][j]) for j in order) == capped["keys"].tolist()
    assert min(idf[order]) >= max(np.delete(idf, order))
    # the product's host half computes the same call arguments
    qt = lc.query_terms(q, ngram)
    keys, qf = np.unique(qt, return_counts=True)
    dl = capped["dl"]
    pk, pw, pc0, pc1 = bm25_plan(keys, qf, full["df"], n, dl.sum() / n, lc.K1, lc.B)
    assert np.array_equal(pk, capped["keys"]) and np.array_equal(pw, capped["w"])
    assert pc0 == capped["c0"] and pc1 == capped["c1"]
    # the dropped terms contribute nothing
    ids, s = lc.bm25_rank(capped)
    ids_f, s_f = lc.bm25_rank(full)
    assert np.all(s_f[np.argsort(ids_f)][np.isin(np.sort(ids_f), ids)] >= s[np.argsort(ids)] - 1e-12)
