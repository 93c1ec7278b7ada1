"""The k-means reference and cases on the CPU, from the float64 definition alone: the vectorised
reference equals the plain loops; every case of test_gpu_kmeans.py stays inside its caps (near-tie
shares, trajectory margins, planted partitions); `pick_representatives` equals a literal
restatement of LangChain's loop; `kmeanspp_rows` equals a plain restatement."""
import numpy as np
import pytest

import kmeans_cases as kc
from mediquery_hip.vectorstore import kmeanspp_rows, pick_representatives


@pytest.mark.parametrize("dim,n,c,mk", ((64, 65, 17, "none"), (256, 33, 5, "third"), (64, 40, 1, "single"),
                                        (64, 31, 33, "ones"), (256, 20, 3, "zeros")))
def test_vectorised_reference_equals_the_loop(dim, n, c, mk):
    mask = kc.row_mask(mk, n)
    for rows, cents in ((kc.exact_corpus(dim, n), kc.exact_centroids(dim, n, c)),
                        (kc.neardup_corpus(dim, n), kc.neardup_corpus(dim, n + c)[n:])):
        lab, dots, _ = kc.assign64(rows, cents, mask)
        llab, ldots = kc.assign_by_loop(rows, cents, mask)
        assert np.array_equal(lab, llab)
        assert np.allclose(dots, ldots, rtol=0, atol=1e-12)
        new, counts = kc.update64(rows, lab, cents)
        lnew, lcounts = kc.update_by_loop(rows, lab, cents)
        assert np.array_equal(counts, lcounts) and np.allclose(new, lnew, rtol=0, atol=1e-12)
        empty = counts == 0
        assert np.array_equal(new[empty], np.asarray(cents, np.float64)[empty])


def test_exact_centroids_tie_scale_and_repeat():
    dim, n, c = 64, 257, 17
    rows, cents = kc.exact_corpus(dim, n), kc.exact_centroids(dim, n, c)
    assert np.array_equal(cents[2], cents[0]) and np.array_equal(cents[1], rows[7])
    norms = (cents.astype(np.float64) ** 2).sum(1)
    assert set(norms.tolist()) == {0.25, 1.0, 4.0}
    lab, _, d = kc.assign64(rows, cents, None)
    assert (d * 32 == np.round(d * 32)).all()  # exact in fp32 in any order
    assert not (lab == 2).any()  # the repeat never wins its tie


@pytest.mark.parametrize("dim,n,c", kc.RANDOM_CASES)
def test_random_cases_stay_inside_the_near_tie_cap(dim, n, c):
    rows = kc.neardup_corpus(dim, n)
    for mk in ("none", "third"):
        mask = kc.row_mask(mk, n)
        adm = np.arange(n) if mask is None else np.flatnonzero(mask)
        assert len(adm) >= c
        cents = rows[kc.random_centroid_rows(dim, n, c, adm)]
        assert (np.linalg.norm(cents.astype(np.float64), axis=1) <= 1 + 1e-6).all()
        d = kc.assign64(rows, cents, mask)[2]
        assert kc.undecided_rows(d, dim)[adm].mean() <= kc.NEAR_TIE_CAP


@pytest.mark.parametrize("case", kc.TRAJECTORY_CASES)
def test_trajectory_cases_have_their_updates_and_margins(case):
    dim, blobs, per, sigma, cs, sd = case
    rows, _ = kc.blob_corpus(dim, blobs, per, sigma, cs)
    init = rows[kc.trajectory_seeds(len(rows), blobs, sd)]
    _, labels, updates, converged, margins = kc.lloyd64(rows, init, None, 30)
    assert converged and updates >= 3 and len(margins) == updates + 1
    assert min(margins) >= kc.TRAJECTORY_MARGIN * kc.bprime(dim)
    assert (np.bincount(labels, minlength=blobs) > 0).all()
    assert (cs, sd) in [f[:2] for f in kc.search_trajectories(dim, blobs, per, sigma, [cs], [sd])]


def test_the_representatives_store_has_no_near_tie_where_it_matters():
    dim, blobs, per, sigma = kc.REP_CASE
    rows, planted = kc.blob_corpus(dim, blobs, per, sigma)
    init = rows[kc.planted_seeds(planted, blobs)]
    every = np.arange(len(rows))
    for adm in (every, every[every % 3 == 0]):
        mask = np.isin(every, adm)
        for n_iter in (0, 25):
            cents = kc.lloyd64(rows, init, mask, n_iter)[0]
            for num_closest in (1, 2, 3):
                hits = min(blobs * num_closest, len(adm))
                assert kc.ranking_gap(rows[adm], cents, hits) > 4 * kc.bound(dim)


@pytest.mark.parametrize("dim,blobs,per", kc.PLANTED_CASES + (kc.STORE_CASE,))
def test_planted_blobs_converge_to_the_partition(dim, blobs, per):
    rows, planted = kc.blob_corpus(dim, blobs, per, kc.PLANTED_SIGMA)
    init = rows[kc.planted_seeds(planted, blobs)]
    cents, labels, updates, converged, margins = kc.lloyd64(rows, init, None, 20)
    assert converged and np.array_equal(labels, planted)
    assert min(margins) >= 7000 * kc.bprime(dim)
    j0, j1 = kc.objective64(rows, init, kc.assign64(rows, init)[0]), kc.objective64(rows, cents, labels)
    assert j1 <= j0


def test_pick_representatives_is_langchains_loop():
    rng = np.random.default_rng(19)
    for n, c in ((40, 5), (7, 7), (12, 3), (300, 16)):
        dist = rng.random((c, n))
        dist[:, : n // 3] = np.round(dist[:, : n // 3], 1)  # ties: the stable order, lowest row first
        rankings = [np.argsort(dist[j], kind="stable") for j in range(c)]
        for num_closest in (1, 2, 3):
            for rd in (False, True):
                want = kc.langchain_closest_indices(dist, c, num_closest, rd)
                assert pick_representatives(rankings, num_closest, rd, False) == want
                assert pick_representatives(rankings, num_closest, rd, True) == sorted(want)
                # the first min(c x num_closest, n) of each ranking are enough
                short = [r[:min(c * num_closest, n)] for r in rankings]
                assert pick_representatives(short, num_closest, rd, False) == want
    # every centre nearest the same rows: without remove_duplicates each cluster moves on
    same = [np.arange(10)] * 3
    assert pick_representatives(same, 2, False) == [0, 1, 2, 3, 4, 5]
    assert pick_representatives(same, 2, True) == [0, 1]


def test_kmeanspp_rows_is_the_plain_restatement():
    for dim, n, k, seed in ((64, 50, 5, 0), (64, 50, 50, 1), (256, 33, 7, 2)):
        rows = kc.neardup_corpus(dim, n).astype(np.float64)
        dots = rows @ rows.T
        calls = []

        def dots_of_row(p):
            calls.append(p)
            return dots[p]
        got = kmeanspp_rows(n, k, np.random.default_rng(seed), dots_of_row)
        assert got.tolist() == kc.kmeanspp_restated(dots, k, np.random.default_rng(seed))
        assert len(set(got.tolist())) == k and calls == got.tolist()
    # coinciding rows: once every row sits on a seed the rest are drawn from the rows not yet taken
    rows = np.repeat(np.eye(64)[:2], 3, axis=0)
    got = kmeanspp_rows(6, 5, np.random.default_rng(3), lambda p: rows[p] @ rows.T)
    assert len(set(got.tolist())) == 5
    assert got.tolist() == kc.kmeanspp_restated(rows @ rows.T, 5, np.random.default_rng(3))
    with pytest.raises(ValueError, match="needs at least as many rows"):
        kmeanspp_rows(3, 4, np.random.default_rng(0), lambda p: np.ones(3))
