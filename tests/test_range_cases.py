"""The range search's reference and cases, on the CPU: `range_reference` (a sort) agrees with a
loop over the rows, the exact class is what the GPU test takes it for, and every random-class
case leaves at most NEAR_TIE_CAP of its returned positions undecided - computed from the
reference alone, before any device result exists."""
import numpy as np
import pytest

import range_cases as rc


@pytest.mark.parametrize("dim,n", [(64, 65), (256, 1000), (768, 33)])
def test_reference_agrees_with_a_loop(dim, n):
    rows, queries = rc.exact_corpus(dim, n), rc.exact_queries(dim, 5)
    s = rc.dots64(rows, queries)
    for mk in rc.MASKS:
        mask = rc.row_mask(mk, n)
        for max_hits in (1, 5, 64, 1000):
            for tau in rc.MIN_SCORES:
                counts, ref_s, ref_i = rc.range_reference(s, mask, tau, max_hits)
                for j in range(len(queries)):
                    count, hits = rc.reference_by_loop(s[j], mask, tau, max_hits)
                    assert counts[j] == count
                    m = len(hits)
                    assert m == min(count, max_hits)
                    assert ref_i[j, :m].tolist() == [r for _, r in hits]
                    assert ref_s[j, :m].tolist() == [x for x, _ in hits]
                    assert (ref_i[j, m:] == -1).all() and np.isneginf(ref_s[j, m:]).all()


def test_reference_edge_cases():
    s = np.array([[0.5, -0.0, 0.0, 0.5, -1.0]])
    counts, rs, ri = rc.range_reference(s, None, -0.0, 3)
    assert counts.tolist() == [4] and ri.tolist() == [[0, 3, 1]]          # -0.0 ranks as +0.0, row order
    assert not np.signbit(rs[0, 2])
    counts, rs, ri = rc.range_reference(s, None, 0.0, 8)
    assert counts.tolist() == [4] and ri[0, :5].tolist() == [0, 3, 1, 2, -1]
    counts, rs, ri = rc.range_reference(s, np.zeros(5, bool), -np.inf, 2)
    assert counts.tolist() == [0] and (ri == -1).all() and np.isneginf(rs).all()
    counts, rs, ri = rc.range_reference(np.zeros((2, 0)), None, -np.inf, 2)
    assert counts.tolist() == [0, 0] and ri.shape == (2, 2)


def test_exact_class_has_few_distinct_scores_and_the_thresholds_cut_it():
    """Every cut of the exact class falls inside a large tie group, and the thresholds of the
    GPU test select different sets: all rows, most, some, none."""
    dim, n = 64, 4097
    s = rc.dots64(rc.exact_corpus(dim, n), rc.exact_queries(dim, max(rc.NQS)))
    assert np.all(s * 16 == np.round(s * 16))
    assert len(np.unique(s)) <= 33
    counts = [int(rc.range_reference(s, None, tau, 1)[0].sum()) for tau in rc.MIN_SCORES]
    assert counts[0] == s.size and counts[2] == counts[3]                 # -inf: all; -0.0 as 0.0
    assert counts == sorted(counts, reverse=True) and counts[1] > counts[3] > counts[5] > counts[6] == counts[7] == 0
    assert counts[3] == counts[4] + int((s == 0).sum())                   # 1/32 lies between two scores


@pytest.mark.parametrize("shape", rc.RANDOM_SHAPES)
def test_random_cases_stay_inside_the_near_tie_cap(shape):
    dim, n = shape
    rows = rc.random_corpus(dim, n)
    s = rc.dots64(rows, rc.random_queries(dim, rc.RANDOM_NQ))
    ok = np.ones(n, bool)
    for tau in rc.random_min_scores(dim):
        undecided = positions = 0
        for max_hits in rc.random_max_hits(n):
            for j in range(rc.RANDOM_NQ):
                undecided += rc.undecided_rows(s[j], ok, tau, max_hits, dim)
                positions += rc.returned_positions(s[j], ok, tau, max_hits)
        print("random case %s min_score %s: %d undecided of %d positions" % (shape, tau, undecided, positions))
        assert positions > 0 and undecided <= rc.NEAR_TIE_CAP * positions, (shape, tau, undecided, positions)


def test_check_random_accepts_the_reference_and_catches_each_fault():
    dim, n, max_hits, tau = 64, 3000, 64, 0.05
    rows = rc.random_corpus(dim, n)
    s = rc.dots64(rows, rc.random_queries(dim, 1))[0]
    ok = np.ones(n, bool)
    counts, ref_s, ref_i = rc.range_reference(s[None], None, tau, max_hits)
    good = (int(counts[0]), ref_s[0].astype(np.float32), ref_i[0])
    assert rc.check_random(*good, s, ok, tau, max_hits, dim) == []
    assert counts[0] > max_hits

    def faults(count=good[0], sc=good[1], ids=good[2]):
        return rc.check_random(count, sc, ids, s, ok, tau, max_hits, dim)
    assert any("count" in f for f in faults(count=good[0] + 50))
    swapped = good[2].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert any("sorted" in f or "score off" in f for f in faults(ids=swapped))
    dup = good[2].copy()
    dup[1] = dup[0]
    assert any("repeat" in f for f in faults(ids=dup))
    low = good[2].copy()
    low[-1] = int(np.argmin(s))
    lows = good[1].copy()
    lows[-1] = np.float32(s[low[-1]])
    assert any("below" in f for f in faults(sc=lows, ids=low))
    gone = np.concatenate([good[2][1:], [-1]])                             # the best row is missing
    assert any("rows [%d] must be returned" % good[2][0] in f
               for f in faults(count=max_hits - 1, sc=np.concatenate([good[1][1:], [-np.inf]]), ids=gone))
    short = good[2].copy()
    short[-1] = -1
    assert faults(ids=short) != []
    off = good[1].copy()
    off[3] += np.float32(1e-3)
    assert any("score off" in f or "sorted" in f for f in faults(sc=off))
