"""CPU checks of the maximal-marginal-relevance test material (tests/mmr_cases.py): the
float64 reference behaves as LangChain's algorithm, the exact class really is exact in
fp32, the checkers catch four wrong restatements, and the stand-in as_retriever routes
search_type="mmr"."""
import numpy as np
import pytest

import mmr_cases as mc


def _exact_cases(dim, fetch_k=20, n_fam=16, fam=24, nq=8):
    rows = mc.exact_corpus(dim, n_fam, fam)
    for q in range(nq):
        ids, s = mc.exact_candidates(rows, n_fam, fam, q, fetch_k)
        yield ids, s, mc.gram64(rows, ids)


def test_lambda_one_is_score_order():
    for dim, fetch_k in ((96, 20), (768, 64)):
        for s, G in mc.random_cases(dim, fetch_k):
            assert mc.mmr_reference(s, G, 1.0, fetch_k) == list(np.lexsort((np.arange(len(s)), -s)))
    for ids, s, G in _exact_cases(96):  # ties: the lowest list position first
        assert mc.mmr_reference(s, G, 1.0, len(s)) == list(range(len(s)))


@pytest.mark.parametrize("dim", sorted(mc.EXACT_DIMS))
def test_copy_never_ahead_of_an_equal_non_copy(dim):
    """lam < 1: while a candidate with the same s that is no exact copy of an earlier pick is
    left, the reference does not place an exact copy of an earlier pick."""
    seen = 0
    for ids, s, G in _exact_cases(dim):
        for lam in (0.0, 0.25, 0.5, 0.75):
            picks = mc.mmr_reference(s, G, lam, len(s))
            for t, p in enumerate(picks):
                if not any(G[p, e] == 1.0 for e in picks[:t]):
                    continue
                seen += 1
                left = [i for i in range(len(s)) if i not in picks[:t] and s[i] == s[p]]
                assert all(any(G[i, e] == 1.0 for e in picks[:t]) for i in left), (dim, lam, t, p)
    assert seen  # the class does plant copies


@pytest.mark.parametrize("dim", sorted(mc.EXACT_DIMS))
def test_exact_class_is_exact_in_fp32(dim):
    for fetch_k in (20, 64):
        for ids, s, G in _exact_cases(dim, fetch_k):
            assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
            assert np.array_equal(G.astype(np.float32).astype(np.float64), G)
            assert np.all(np.diag(G) == 1.0)
            for lam in mc.LAMBDAS:
                assert mc.mmr_fp32(s, G, lam, fetch_k) == mc.mmr_reference(s, G, lam, fetch_k), (fetch_k, lam)


def test_exact_class_has_ties():
    ids, s, G = next(_exact_cases(768))
    assert len(np.unique(s)) < len(s) // 2 and np.sum(np.triu(G, 1) == 1.0) >= 2


def test_reference_passes_its_own_checker():
    for dim, fetch_k in ((96, 20), (768, 64)):
        for s, G in mc.random_cases(dim, fetch_k):
            for lam in (0.25, 0.5, 0.9):
                picks = mc.mmr_reference(s, G, lam, 16)
                assert mc.check_path(picks, s, G, lam, mc.TOL, 16) == []
                assert max(mc.path_deficits(picks, s, G, lam)) == 0.0
                # and the fp32 restatement stays within the tolerance of its own path
                assert mc.check_path(mc.mmr_fp32(s, G, lam, 16), s, G, lam, mc.TOL, 16) == []


def test_checker_rejects_padding_repeats_and_short_results():
    s, G = mc.random_cases(96, 20)[0]
    good = mc.mmr_reference(s, G, 0.5, 5)
    assert mc.check_path(good[:4], s, G, 0.5, mc.TOL, 5)
    assert mc.check_path(good[:4] + [-1], s, G, 0.5, mc.TOL, 5)
    assert mc.check_path(good[:4] + [good[0]], s, G, 0.5, mc.TOL, 5)
    assert mc.positions([7, 3, 99, -1, -1], [3, 5, 7]) == [2, 0, -1]


@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_checkers_have_teeth(mutant):
    """Each wrong restatement fails check_path on the random cases and equality on the
    exact class."""
    path_fails = 0
    for dim, fetch_k in ((96, 20), (768, 64)):
        for s, G in mc.random_cases(dim, fetch_k):
            for lam in (0.25, 0.5, 0.9):
                path_fails += bool(mc.check_path(mc.mmr_fp32(s, G, lam, 16, mutant), s, G, lam, mc.TOL, 16))
    assert path_fails
    unequal = 0
    for dim in sorted(mc.EXACT_DIMS):
        for ids, s, G in _exact_cases(dim):
            for lam in mc.LAMBDAS:
                unequal += mc.mmr_fp32(s, G, lam, 16, mutant) != mc.mmr_reference(s, G, lam, 16)
    assert unequal


def test_stand_in_retriever_routes_mmr():
    from mediquery_hip import compat
    if compat.HAVE_LANGCHAIN:
        pytest.skip("langchain_core's own as_retriever is in use")

    class Stub(compat.VectorStoreBase):
        def __init__(self):
            self.calls = []

        def similarity_search(self, query, k=4, **kw):
            self.calls.append(("sim", query, k, kw))
            return ["sim"]

        def max_marginal_relevance_search(self, query, k=4, fetch_k=20, lambda_mult=0.5, filter=None, **kw):
            self.calls.append(("mmr", query, k, fetch_k, lambda_mult, filter, kw))
            return ["mmr"]

    st = Stub()
    kw = {"k": 5, "fetch_k": 30, "lambda_mult": 0.25, "filter": {"src": "a"}}
    assert st.as_retriever(search_type="mmr", search_kwargs=kw).invoke("q") == ["mmr"]
    assert st.calls == [("mmr", "q", 5, 30, 0.25, {"src": "a"}, {})]
    st.calls.clear()
    assert st.as_retriever(search_type="mmr").get_relevant_documents("q") == ["mmr"]
    assert st.calls == [("mmr", "q", 4, 20, 0.5, None, {})]
    st.calls.clear()
    # the default call and any other search_type: a plain similarity search, as before
    assert st.as_retriever(search_kwargs={"k": 3}).invoke("q") == ["sim"]
    assert st.as_retriever(search_type="similarity", search_kwargs={"k": 3, "fetch_k": 9}).invoke("q") == ["sim"]
    assert st.as_retriever().invoke("q") == ["sim"]
    assert st.calls == [("sim", "q", 3, {}), ("sim", "q", 3, {}), ("sim", "q", 4, {})]
